"""Generate the RX-coalescing fixtures (tests/golden/gro_vectors.{bin,json}).

    python tests/golden/make_gro_golden.py

Small batches of frames and what include/nstack_gro.h says becomes of them, WRITTEN BY THE MODEL
(tests/gro_model.py with the oracle's checksum functions, oracle/_build/liboracle_inet.so): the
reference has no coalescing step, so no output of it could back these vectors. They pin the model: a
change of it that moves a byte, a status word or a verdict word shows up as a diff of these files.
tests/test_gro_model.py checks the model and the host plan against them, tests/test_gpu_gro.py the
kernels.

A case is one batch. The .bin holds every case's frames back to back and then its expected datagrams
back to back; the .json their lengths, the call's arguments, the expected final status words, the
datagrams' lead frames and their verdict words.
"""
import ctypes
import itertools
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)


def inet_oracle():
    L = ctypes.CDLL(os.path.join(ROOT, "oracle", "_build", "liboracle_inet.so"))
    u16, u32, vp, sz = ctypes.c_uint16, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_size_t
    L.oracle_ip_checksum.restype = u16
    L.oracle_ip_checksum.argtypes = [vp, sz]
    L.oracle_tcp_checksum.restype = u16
    L.oracle_tcp_checksum.argtypes = [u32, u32, vp, sz]
    L.oracle_udp_checksum.restype = u16
    L.oracle_udp_checksum.argtypes = [vp, sz, u32, u32]
    return L


def cases(io):
    import gro_batch as gb
    import gro_model as gm
    rng = np.random.default_rng(20261021)
    C = []
    # a datagram of every header shape cut at three units, the segments of each reversed
    for mss in (536, 7, 1):
        fr = []
        for dg in gb.tso_datagrams(io, mss)[:4]:
            if len(dg) < 6000:
                fr += gb.cut(io, dg, mss)[::-1]
        C.append(dict(tag=f"cut_mss{mss}", frames=fr, flags=0))
    frames, verdict, mask, _ = gb.stays_apart(io)
    C.append(dict(tag="stays_apart", frames=frames, flags=0, verdict=[int(v) for v in verdict], drop_mask=mask))
    C.append(dict(tag="mixed_no_group", frames=gb.mixed_no_group(io), flags=1))
    # two windows of one flow and a run across 2^32, interleaved; room for all but the last datagram
    a = gb.cut(io, gm.tcp_datagram(io, gb.payload(rng, 700), (1 << 15) - 250, tflags=gm.ACK | gm.PSH), 100)
    b = gb.cut(io, gm.tcp_datagram(io, gb.payload(rng, 500), (1 << 32) - 250, sport=0x8100, hlen=24, thl=32), 100)
    fr = [x for pair in itertools.zip_longest(a, b) for x in pair if x is not None]
    C.append(dict(tag="windows", frames=fr, flags=0, align=16, short=1))
    return C


def main():
    import gro_batch as gb
    io = inet_oracle()
    blob, recs = bytearray(), []
    for c in cases(io):
        kw = dict(flags=c["flags"], verdict=c.get("verdict"), drop_mask=c.get("drop_mask", 0), align=c.get("align", 1))
        b = gb.GBatch(io, c["frames"], **kw)
        out_bytes = b.need - c["short"] if "short" in c else None
        if out_bytes is not None:
            b = gb.GBatch(io, c["frames"], out_bytes=out_bytes, **kw)
        dgs = b.datagrams()
        fits = [int(v) != 0x002 for v in b.dverdict]
        rec = dict(tag=c["tag"], out_bytes=out_bytes, at=len(blob), flen=[len(f) for f in c["frames"]],
                   fstat=[int(s) for s in b.fstat], dlead=[int(x) for x in b.plan["dlead"]],
                   dlen=[len(d) if f else 0 for d, f in zip(dgs, fits)], dsize=[int(x) for x in b.plan["dlen"]],
                   dverdict=[int(v) for v in b.dverdict], **kw)
        for f in c["frames"]:
            blob += f
        rec["dat"] = len(blob)
        for d, f in zip(dgs, fits):
            if f:
                blob += d
        recs.append(rec)
    assert len(blob) <= 64 << 10, len(blob)
    with open(os.path.join(HERE, "gro_vectors.bin"), "wb") as f:
        f.write(blob)
    with open(os.path.join(HERE, "gro_vectors.json"), "w") as f:
        json.dump({"arena": "gro_vectors.bin", "cases": recs}, f, separators=(",", ":"))
        f.write("\n")
    seen = 0
    for r in recs:
        for s in r["fstat"]:
            seen |= s
    print(f"{len(recs)} cases, {sum(len(r['flen']) for r in recs)} frames, {sum(len(r['dlen']) for r in recs)} datagrams, "
          f"{len(blob)} bytes, status bits seen 0x{seen:04x}")


if __name__ == "__main__":
    main()
