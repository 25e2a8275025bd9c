#!/usr/bin/env python3
"""Device-resident throughput of one-pass RX reassembly (include/nstack_rxr.h) beside a plain copy,
in one process, the versions alternated:

  X  ether_rx_reasm_plan_dev + ether_rx_reasm_dev           (wire frames in, datagrams out)
  P  the plan alone, and  D  the build alone (on the plan's arrays)
  A  one device-to-device copy of W bytes, W = sum(dlen): the build reads W bytes of the frames and
     writes W bytes, so the copy moves the same bytes once                              (the floor)
The frames come from ether_tx_frame_dev (mtu 1500, TXF_F_FCS, slot 1518) over the three workloads of
tools/bench_txf.py: datagrams of 8220 bytes (6 fragments each), of 1400 bytes (RXR_WHOLE) and a
60 / 572 / 1500 / 8220 / 65535 mix; each in slot order ("ordered") and again with a seeded
permutation of the slots ("permuted": a group's fragments lie anywhere in the batch). The datagram
bytes are splitmix bytes, so the group keys are random; the few groups whose keys collide come out
RXR_INCOMPLETE and are reported. Timing: one HIP-event pair per version, `--rounds` rounds of the
versions in turn after a warm-up round; per version the median and the spread (quartiles, extremes).
32 seeded datagrams per workload are compared with the model (tests/rxr_model.py on the oracle of
oracle/_build). Writes one JSON document (--out) and prints it.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

MIX = ((60, 0.40), (572, 0.25), (1500, 0.20), (8220, 0.14), (65535, 0.01))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=0.25, help="scales the batch sizes (1.0: tools/bench_txf.py's, 3.5 to 4 GB of frames each)")
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--skip", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rxr_bench.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import nstack_amd as na
    import rxr_model as rr
    from bench_rxv import alternate, stats
    from bench_txs import load_oracles
    _fcs_oracle, inet_oracle = load_oracles()
    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    cur = torch.cuda.current_stream
    MTU, SLOT, ALIGN = 1500, 1518, 16
    res = {"engine": na.version(), "mtu": MTU, "slot": SLOT, "align": ALIGN, "rounds": a.rounds, "scale": a.scale,
           "note": "X = plan + build, P = plan, D = build; A = one d2d copy of W = sum(dlen) bytes; times per group, "
                   "HIP events, versions alternated; GB_s = 2 W / time (bytes read plus bytes written)"}

    def frames_of(D_np, seed):
        """ether_tx_frame_dev over splitmix datagrams of the given lengths: (arena of slots, flen, slots)."""
        n = len(D_np)
        ln = torch.from_numpy(D_np.view(np.int32)).to(dev)
        off = torch.zeros(n, dtype=torch.int64, device=dev)
        off[1:] = torch.cumsum(ln[:-1].to(torch.int64), 0)
        R = int(off[-1].item()) + int(D_np[-1])
        arena = torch.empty(R, dtype=torch.uint8, device=dev)
        na.fill_splitmix_dev(arena, R, seed, 0)
        l64 = ln.to(torch.int64)
        for col, src in ((0, torch.full((n,), 0x45, dtype=torch.uint8, device=dev)), (2, (l64 >> 8).to(torch.uint8)),
                         (3, (l64 & 255).to(torch.uint8)), (6, torch.zeros(n, dtype=torch.uint8, device=dev)),
                         (7, torch.zeros(n, dtype=torch.uint8, device=dev))):
            arena.index_put_((off + col,), src)
        l2 = torch.zeros(12, dtype=torch.uint8, device=dev)
        first = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        flags = na.TXF_F_FCS | na.TXF_F_L2_ONE
        na.tx_frame_plan_dev(arena, R, off, ln, n, MTU, first, flags)
        torch.cuda.synchronize()
        slots = int(first[-1].item())
        out = torch.zeros(slots * SLOT, dtype=torch.uint8, device=dev)
        flen = torch.zeros(slots, dtype=torch.int32, device=dev)
        na.tx_frame_dev(arena, R, off, ln, l2, n, MTU, first, out, SLOT, slots, flags, flen)
        torch.cuda.synchronize()
        return out, flen, slots, n

    def measure(name, wire, off, ln, n, datagrams, seed):
        t = dict(fstat=torch.zeros(n, dtype=torch.int32, device=dev), dst=torch.zeros(n, dtype=torch.int64, device=dev),
                 dgi=torch.zeros(n, dtype=torch.int32, device=dev), doff=torch.zeros(n + 1, dtype=torch.int64, device=dev),
                 dlen=torch.zeros(n, dtype=torch.int32, device=dev), dlead=torch.zeros(n, dtype=torch.int32, device=dev),
                 counts=torch.zeros(2, dtype=torch.int64, device=dev), final=torch.zeros(n, dtype=torch.int32, device=dev))
        nbytes = wire.numel()

        def P():
            na.rx_reasm_plan_dev(wire, nbytes, off, ln, n, t["fstat"], t["dst"], t["dgi"], t["doff"], t["dlen"], t["dlead"],
                                 t["counts"], flags=na.RXR_F_TRAILER, align=ALIGN, stream=cur())

        P()
        torch.cuda.synchronize()
        m, total = (int(x) for x in t["counts"].cpu().numpy())
        out = torch.zeros(total + 16, dtype=torch.uint8, device=dev)
        W = int(t["dlen"][:m].to(torch.int64).sum().item())

        def D():
            na.rx_reasm_dev(wire, nbytes, off, ln, n, t["fstat"], t["dst"], t["dgi"], t["doff"], t["dlen"], out, total,
                            flags=na.RXR_F_TRAILER, fstat=t["final"], stream=cur())

        def X():
            P()
            D()

        ca = torch.empty(W, dtype=torch.uint8, device=dev)
        cb = torch.empty(W, dtype=torch.uint8, device=dev)

        def A():
            cb.copy_(ca)

        ms = alternate({"X": X, "P": P, "D": D, "A": A}, a.rounds, torch)
        r = {k: stats(v, 2 * W) for k, v in ms.items()}
        for k in ("X", "D"):
            r[k + "_over_A"] = r[k]["ms_median"] / r["A"]["ms_median"]
            r[k + "_over_A_q1q3"] = [r[k]["ms_q1"] / r["A"]["ms_q3"], r[k]["ms_q3"] / r["A"]["ms_q1"]]
        fin = t["final"].cpu().numpy().view(np.uint32)
        r.update({"frames": n, "framed_datagrams": datagrams, "datagrams": m, "delivered_bytes": W, "wire_bytes": int(ln.to(torch.int64).sum().item()),
                  "frames_incomplete": int(((fin & rr.INCOMPLETE) != 0).sum()), "frames_delivered": int(((fin & rr.DELIVERED) != 0).sum())})
        # ---- 32 seeded datagrams against the model ----
        dgi = t["dgi"].cpu().numpy().view(np.uint32)
        doff = t["doff"].cpu().numpy().view(np.uint64)
        dlen = t["dlen"].cpu().numpy().view(np.uint32)
        off_np, ln_np = off.cpu().numpy(), ln.cpu().numpy()
        order = np.argsort(dgi, kind="stable")
        lo = np.searchsorted(dgi[order], np.arange(m), "left")
        hi = np.searchsorted(dgi[order], np.arange(m), "right")
        bad = checked = 0
        for k in np.random.default_rng(seed).integers(0, m, 32):
            k = int(k)
            idx = order[lo[k]:hi[k]]
            frames = [wire[int(off_np[i]):int(off_np[i]) + int(ln_np[i])].cpu().numpy().tobytes() for i in idx]
            pl = rr.plan(frames, rr.F_TRAILER)
            ok = pl["m"] == 1 and int(pl["dlen"][0]) == int(dlen[k])
            if ok:
                want, _ = rr.build(inet_oracle, frames, pl, np.zeros(int(dlen[k]), dtype=np.uint8))
                got = out[int(doff[k]):int(doff[k]) + int(dlen[k])].cpu().numpy()
                ok = np.array_equal(got, want)
            bad += int(not ok)
            checked += len(frames)
        r["spot_datagrams"], r["spot_frames"], r["spot_bad"] = 32, checked, bad
        r["last_launch"] = na.rxr_last_launch()
        res[name] = r
        print(name, json.dumps(r), flush=True)

    def workload(name, D_np, seed):
        wire, flen, slots, datagrams = frames_of(D_np, seed)
        ln = (flen + 4).contiguous()
        off = torch.arange(slots, dtype=torch.int64, device=dev) * SLOT
        measure(name + "_ordered", wire, off, ln, slots, datagrams, seed + 3)
        perm = torch.from_numpy(np.random.default_rng(seed + 4).permutation(slots)).to(dev)
        measure(name + "_permuted", wire, off[perm].contiguous(), ln[perm].contiguous(), slots, datagrams, seed + 5)

    s = a.scale
    if "udp8220" not in a.skip:
        workload("udp8220", np.full(int(400_000 * s), 8220, dtype=np.uint32), 31)
        torch.cuda.empty_cache()
    if "whole1400" not in a.skip:
        workload("whole1400", np.full(int(2_500_000 * s), 1400, dtype=np.uint32), 41)
        torch.cuda.empty_cache()
    if "mix" not in a.skip:
        n = int(1_000_000 * s)
        counts = [int(n * w) for _, w in MIX]
        counts[0] += n - sum(counts)
        D = np.repeat(np.array([d for d, _ in MIX], dtype=np.uint32), counts)
        np.random.default_rng(7).shuffle(D)
        workload("mix", D, 51)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1), flush=True)


if __name__ == "__main__":
    main()
