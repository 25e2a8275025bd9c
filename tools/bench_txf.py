#!/usr/bin/env python3
"""Device-resident throughput of one-pass TX framing (include/nstack_txf.h) beside a plain copy and
beside a lower bound on what a caller does today, in one process, the versions alternated:

  X  ether_tx_frame_plan_dev + ether_tx_frame_dev          (datagrams in, wire bytes out)
  A  one device-to-device copy that moves as many bytes as X: X reads R = sum(D) and writes
     W = sum(F + 4) bytes, the copy reads and writes (R + W) / 2 bytes each           (the floor)
  B  a lower bound on today's way, on the frames X built: ether_tx_seal_*_dev with TXS_F_FCS over
     them plus the copy A. Today the frames are built on the host and copied to the device (A
     stands for that copy, at device speed) before they can be sealed. The fixed-stride form where
     every frame has one length, the variable form (off = k * slot, len = flen) otherwise.
at mtu 1500 with TXF_F_FCS, slot 1518, per-datagram MAC records, on three workloads: UDP-sized
datagrams of 8220 bytes (6 frames each), datagrams of 1400 bytes (the TXF_WHOLE path), and a
60 / 572 / 1500 / 8220 / 65535 mix. Datagram bytes are splitmix bytes with vhl, ip_len and ip_foff
stamped. Timing: one HIP-event pair per version, `--rounds` rounds of the versions in turn after a
warm-up round; per version the median and the spread (quartiles, extremes). All frames of 32 seeded
datagrams per workload are compared with the model (tests/txf_model.py on the oracles of
oracle/_build), with status, flen and fcs. Writes one JSON document (--out) and prints it.
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
    ap.add_argument("--scale", type=float, default=1.0, help="scales the batch sizes (1.0: 3.5 to 4 GB of output each)")
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--skip", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "txf_bench.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import nstack_amd as na
    import txf_model as fm
    from bench_rxv import alternate, stats
    from bench_txs import load_oracles
    fcs_oracle, inet_oracle = load_oracles()
    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    cur = torch.cuda.current_stream
    MTU, FLAGS, SLOT = 1500, na.TXF_F_FCS, 1518
    res = {"engine": na.version(), "mtu": MTU, "slot": SLOT, "rounds": a.rounds,
           "note": "X = plan + build; A = one d2d copy of (R + W) / 2 bytes (the bytes X reads plus writes, moved "
                   "once); B = ether_tx_seal over the built frames + A; times per group, HIP events, versions "
                   "alternated; GB_s = (R + W) / time"}

    def workload(name, D_np, seed):
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
        del l64, src
        l2 = torch.empty(n * 12, dtype=torch.uint8, device=dev)
        na.fill_splitmix_dev(l2, n * 12, seed + 1, 0)
        first = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        pst = torch.zeros(n, dtype=torch.int32, device=dev)
        na.tx_frame_plan_dev(arena, R, off, ln, n, MTU, first, FLAGS, pst)
        torch.cuda.synchronize()
        slots = int(first[-1].item())
        out = torch.zeros(slots * SLOT, dtype=torch.uint8, device=dev)
        flen = torch.zeros(slots, dtype=torch.int32, device=dev)
        fcs = torch.zeros(slots, dtype=torch.int32, device=dev)
        status = torch.zeros(n, dtype=torch.int32, device=dev)

        def X():
            na.tx_frame_plan_dev(arena, R, off, ln, n, MTU, first, FLAGS, pst, stream=cur())
            na.tx_frame_dev(arena, R, off, ln, l2, n, MTU, first, out, SLOT, slots, FLAGS, flen, status, fcs, stream=cur())

        X()
        torch.cuda.synchronize()
        W = int(flen.to(torch.int64).sum().item()) + 4 * slots
        half = (R + W) // 2
        ca = torch.empty(half, dtype=torch.uint8, device=dev)
        cb = torch.empty(half, dtype=torch.uint8, device=dev)
        fl_np = flen.cpu().numpy()
        one_len = int(fl_np[0]) if (fl_np == fl_np[0]).all() else 0
        soff = torch.arange(slots, dtype=torch.int64, device=dev) * SLOT
        sst = torch.zeros(slots, dtype=torch.int32, device=dev)

        def A():
            cb.copy_(ca)

        def B():
            if one_len:
                na.tx_seal_fixed_dev(out, SLOT, one_len, slots, flags=na.TXS_F_FCS, status=sst, stream=cur())
            else:
                na.tx_seal_dev(out, slots * SLOT, soff, flen, slots, flags=na.TXS_F_FCS, status=sst, stream=cur())
            A()

        ms = alternate({"X": X, "A": A, "B": B}, a.rounds, torch)
        r = {k: stats(v, R + W) for k, v in ms.items()}
        for k in ("A", "B"):
            r["X_over_" + k] = r["X"]["ms_median"] / r[k]["ms_median"]
            r["X_over_%s_q1q3" % k] = [r["X"]["ms_q1"] / r[k]["ms_q3"], r["X"]["ms_q3"] / r[k]["ms_q1"]]
        r.update({"datagrams": n, "frames": slots, "read_bytes": R, "written_bytes": W,
                  "B_seal_form": "fixed, len %d" % one_len if one_len else "variable"})
        # ---- all frames of 32 seeded datagrams against the model (after a last X: B sealed in place) ----
        X()
        torch.cuda.synchronize()
        first_np = first.cpu().numpy()
        st_np = status.cpu().numpy().view(np.uint32)
        bad = frames_checked = 0
        for i in np.random.default_rng(seed + 2).integers(0, n, 32):
            i = int(i)
            o, D = int(off[i].item()), int(D_np[i])
            dg = arena[o:o + D].cpu().numpy().tobytes()
            mac = l2[12 * i:12 * i + 12].cpu().numpy().tobytes()
            st, fr, crcs = fm.frames(fcs_oracle, inet_oracle, dg, mac, MTU, FLAGS)
            k0 = int(first_np[i])
            ok = st == int(st_np[i]) and int(first_np[i + 1]) - k0 == len(fr)
            for q, body in enumerate(fr):
                got = out[(k0 + q) * SLOT:(k0 + q) * SLOT + len(body)].cpu().numpy().tobytes()
                ok = ok and got == body and int(flen[k0 + q].item()) == len(body) - 4
                ok = ok and (int(fcs[k0 + q].item()) & 0xFFFFFFFF) == crcs[q]
                frames_checked += 1
            bad += int(not ok)
        r["spot_datagrams"], r["spot_frames"], r["spot_bad"] = 32, frames_checked, bad
        r["last_launch"] = na.txf_last_launch()
        res[name] = r
        print(name, json.dumps(r), flush=True)

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
