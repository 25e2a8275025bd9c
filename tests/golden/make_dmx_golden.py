"""Writes tests/golden/dmx_vectors.{json,bin}: a few batches of tests/dmx_batch.py with what
tests/dmx_model.py makes of them (plan arrays, final words, qcounts and the whole q). The vectors pin
the model: no independent source exists, since the reference demultiplexes one datagram at a time
into live socket queues and has no batch form. Run from the repository root:
    python tests/golden/make_dmx_golden.py"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import dmx_batch as db  # noqa: E402

CASES = [("no-record-8", lambda: db.no_record(8)), ("no-record-128-capacity", lambda: db.no_record(128, n=24)),
         ("duplicate-keys", db.duplicate_keys), ("align-5-16", lambda: db.alignment(5, 16)), ("align-0-8", lambda: db.alignment(0, 8)),
         ("outside", db.outside), ("mixed-200-30", lambda: db.mixed(200, 30)), ("short-q", lambda: db.mixed(30, 4, align=32, q_bytes=1000))]


def main():
    blob, cases = bytearray(), []
    for tag, mk in CASES:
        b = mk()
        p = b.plan
        c = dict(tag=tag, m=b.m, n=b.n, align=b.align, drop_mask=b.drop_mask, out_bytes=int(b.out_bytes), q_bytes=int(b.q_bytes),
                 bind=[int(x) for x in b.bind], doff=[int(x) for x in b.doff], dlen=[int(x) for x in b.dlen],
                 dverdict=None if b.dverdict is None else [int(x) for x in b.dverdict],
                 dstat=[int(x) for x in p["dstat"]], dsock=[int(x) for x in p["dsock"]], rec=[int(x) for x in p["rec"]],
                 sbase=[int(x) for x in p["sbase"]], scnt=[int(x) for x in p["scnt"]], qcounts=[int(x) for x in p["qcounts"]],
                 fin=[int(x) for x in b.fin], out_at=len(blob), out_size=int(b.out.size))
        blob += b.out.tobytes()
        c.update(q_at=len(blob), q_size=int(b.q.size))
        blob += b.q.tobytes()
        cases.append(c)
    with open(os.path.join(HERE, "dmx_vectors.bin"), "wb") as f:
        f.write(bytes(blob))
    with open(os.path.join(HERE, "dmx_vectors.json"), "w") as f:
        json.dump(dict(blob="dmx_vectors.bin", cases=cases), f, separators=(",", ":"))
        f.write("\n")
    print(len(cases), "cases,", len(blob), "bytes")


if __name__ == "__main__":
    main()
