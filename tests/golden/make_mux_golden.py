"""Writes tests/golden/mux_vectors.{json,bin}: a few batches of tests/mux_batch.py with what
tests/mux_model.py makes of them (plan arrays, final words, counts and the whole dgram). The vectors
pin the model: the reference sends one record per call into a live interface and has no batch form.
tests/test_mux_model.py holds every header checksum in them to the oracle's IP checksum. Run from the
repository root:
    python tests/golden/make_mux_golden.py"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import mux_batch as mb  # noqa: E402

CASES = [("status-all-16", lambda: mb.no_datagram(16, big=False)), ("status-no-tcb-8", lambda: mb.no_datagram(8, tcb=False, big=False)), ("wraps", mb.wraps),
         ("routes-2", lambda: mb.tables_routes(2)), ("routes-256", lambda: mb.tables_routes(256)), ("neigh-257", lambda: mb.tables_neigh(257)),
         ("mixed-200-30", lambda: mb.mixed(200, 30)), ("short-dgram", lambda: mb.mixed(30, 4, align=32, dgram_bytes=1000))]


def main():
    blob, cases = bytearray(), []
    for tag, mk in CASES:
        b = mk()
        p = b.plan
        ints = lambda a: [int(x) for x in np.asarray(a).ravel()]
        c = dict(tag=tag, n=b.n, align=b.align, id0=b.id0, q_bytes=int(b.q_bytes), dgram_bytes=int(b.dgram_bytes), rec=ints(b.rec[:b.n]),
                 sfirst=ints(b.sfirst), bind=ints(b.bind[:b.S]), tcb=None if b.tcb is None else [list(t) for t in b.tcb],
                 rt=[[r["network"], r["netmask"], r["gw"], r["iface"], r["mac"].hex()] for r in b.rt],
                 nb=[[a, bytes(m).hex(), v] for a, m, v in b.nb],
                 mstat=ints(p["mstat"]), off=ints(p["off"]), len=ints(p["len"]), tnext=ints(p["tnext"]), counts=ints(p["counts"]),
                 fin=ints(b.fin), q_at=len(blob), q_size=int(b.q.size))
        blob += b.q.tobytes()
        c.update(l2_at=len(blob))
        blob += p["l2"].tobytes()
        c.update(himg_at=len(blob))
        blob += p["himg"].tobytes()
        c.update(dgram_at=len(blob), dgram_size=int(b.dgram.size))
        blob += b.dgram.tobytes()
        cases.append(c)
    with open(os.path.join(HERE, "mux_vectors.bin"), "wb") as f:
        f.write(bytes(blob))
    with open(os.path.join(HERE, "mux_vectors.json"), "w") as f:
        json.dump(dict(blob="mux_vectors.bin", cases=cases), f, separators=(",", ":"))
        f.write("\n")
    print(len(cases), "cases,", len(blob), "bytes")


if __name__ == "__main__":
    main()
