#!/usr/bin/env python3
"""Device-resident cost of TX framing with L4 checksums (include/nstack_txd.h) beside the plain
framer and beside today's two-pass way, in one process, the versions alternated:

  Xl4  ip_tx_frame_l4_dev                                   (X': frames with the UDP checksum filled)
  X    ether_tx_frame_dev on the same datagrams              (what the checksum costs: Xl4 / X)
  B    today's way: inet_csum_batch_dev("udp") over the segments, a device scatter of the results
       into the datagrams (torch index arithmetic: the library ships no kernel for it), then X. The
       seg_off / seg_len / addr arrays are prepared outside the timed window, so the host parse that
       produces them is not counted: B is a lower bound for the two-pass way.
  XS   whole1400 only: X followed by ether_tx_seal_fixed_dev (TXS_F_FCS) over the frames.
The plan (ether_tx_frame_plan_dev) is the same for all and runs once, outside the timed window.
Workloads and protocol are tools/bench_txf.py's: mtu 1500 (--mtu 9000: the field frames have six
segments), TXF_F_FCS, slot 14 + mtu + 4, per-datagram MAC records, datagrams of 8220 bytes (6 frames
each at mtu 1500), of 1400 bytes (TXF_WHOLE) and a 60 / 572 / 1500 /
8220 / 65535 mix; every datagram is UDP with a 20-byte header and garbage in its checksum field. One
HIP-event pair per version, `--rounds` rounds of the versions in turn after a warm-up round; median
and quartiles. Checks: the whole output arena of Xl4 equals that of B (and of XS), every status word
reads UDP with TXD_L4_CSUM_SET, and all frames of 32 seeded datagrams are compared with the model
(tests/txd_model.py on the oracles of oracle/_build). Writes one JSON document (--out) and prints it.
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
    ap.add_argument("--scale", type=float, default=0.25, help="scales the batch sizes of tools/bench_txf.py")
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--skip", default="")
    ap.add_argument("--mtu", type=int, default=1500, help="9000: datagrams of 8220 bytes become whole frames of six segments")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "txd_bench.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import nstack_amd as na
    import txd_model as dm
    from bench_rxv import alternate, stats
    from bench_txs import load_oracles
    fcs_oracle, inet_oracle = load_oracles()
    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    cur = torch.cuda.current_stream
    MTU, FLAGS, SLOT = a.mtu, na.TXF_F_FCS, 14 + a.mtu + 4
    res = {"engine": na.version(), "mtu": MTU, "slot": SLOT, "rounds": a.rounds, "scale": a.scale,
           "note": "Xl4 = ip_tx_frame_l4_dev, X = ether_tx_frame_dev, B = inet_csum_batch_dev(udp) + device scatter + X "
                   "(arrays prepared outside the timed window), XS = X + ether_tx_seal_fixed_dev; the plan runs once, "
                   "outside; HIP events, versions alternated; GB_s = (R + W) / time"}

    def workload(name, D_np, seed):
        n = len(D_np)
        ln = torch.from_numpy(D_np.view(np.int32)).to(dev)
        off = torch.zeros(n, dtype=torch.int64, device=dev)
        off[1:] = torch.cumsum(ln[:-1].to(torch.int64), 0)
        R = int(off[-1].item()) + int(D_np[-1])
        arena = torch.empty(R, dtype=torch.uint8, device=dev)
        na.fill_splitmix_dev(arena, R, seed, 0)
        l64 = ln.to(torch.int64)
        zero = torch.zeros(n, dtype=torch.uint8, device=dev)
        for col, src in ((0, torch.full((n,), 0x45, dtype=torch.uint8, device=dev)), (2, (l64 >> 8).to(torch.uint8)),
                         (3, (l64 & 255).to(torch.uint8)), (6, zero), (7, zero),
                         (9, torch.full((n,), 17, dtype=torch.uint8, device=dev))):
            arena.index_put_((off + col,), src)
        del l64
        l2 = torch.empty(n * 12, dtype=torch.uint8, device=dev)
        na.fill_splitmix_dev(l2, n * 12, seed + 1, 0)
        first = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        na.tx_frame_plan_dev(arena, R, off, ln, n, MTU, first, FLAGS)
        torch.cuda.synchronize()
        slots = int(first[-1].item())
        out = torch.zeros(slots * SLOT, dtype=torch.uint8, device=dev)      # Xl4's
        out2 = torch.zeros(slots * SLOT, dtype=torch.uint8, device=dev)     # X's, B's and XS's
        flen = torch.zeros(slots, dtype=torch.int32, device=dev)
        fcs = torch.zeros(slots, dtype=torch.int32, device=dev)
        status = torch.zeros(n, dtype=torch.int32, device=dev)
        status2 = torch.zeros(n, dtype=torch.int32, device=dev)
        # B's arrays: where the segments and the fields lie, the address words as they lie
        seg_off, seg_len = (off + 20).contiguous(), (ln - 20).contiguous()
        addr = torch.stack([arena[off + 12 + c] for c in range(8)], 1).contiguous().view(torch.int32)
        f_lo, f_hi = (off + 26).contiguous(), (off + 27).contiguous()
        csum = torch.zeros(n, dtype=torch.int16, device=dev)
        arena.index_put_((f_lo,), zero)      # today's way sums with the field zero
        arena.index_put_((f_hi,), zero)
        pristine = arena.clone()

        def Xl4():
            na.tx_frame_l4_dev(arena, R, off, ln, l2, n, MTU, first, out, SLOT, slots, FLAGS, flen, status, fcs, stream=cur())

        def X():
            na.tx_frame_dev(arena, R, off, ln, l2, n, MTU, first, out2, SLOT, slots, FLAGS, flen, status2, fcs, stream=cur())

        def B():
            arena.index_put_((f_lo,), zero)
            arena.index_put_((f_hi,), zero)
            na.inet_batch_dev("udp", arena, R, seg_off, seg_len, addr, csum, n, stream=cur())
            c32 = csum.to(torch.int32) & 0xFFFF
            c32 = torch.where(c32 == 0, torch.full_like(c32, 0xFFFF), c32)   # src/udp.c: a computed zero goes out as 0xffff
            arena.index_put_((f_lo,), (c32 & 255).to(torch.uint8))
            arena.index_put_((f_hi,), (c32 >> 8).to(torch.uint8))
            X()

        vers = {"Xl4": Xl4, "X": X, "B": B}
        X()
        torch.cuda.synchronize()
        W = int(flen.to(torch.int64).sum().item()) + 4 * slots
        fl_np = flen.cpu().numpy()
        one_len = int(fl_np[0]) if (fl_np == fl_np[0]).all() else 0
        if one_len and name == "whole1400":
            def XS():
                X()
                na.tx_seal_fixed_dev(out2, SLOT, one_len, slots, flags=na.TXS_F_FCS, stream=cur())
            vers["XS"] = XS
        ms = alternate(vers, a.rounds, torch)
        r = {k: stats(v, R + W) for k, v in ms.items()}
        for k in vers:
            if k != "Xl4":
                r["Xl4_over_" + k] = r["Xl4"]["ms_median"] / r[k]["ms_median"]
                r["Xl4_over_%s_q1q3" % k] = [r["Xl4"]["ms_q1"] / r[k]["ms_q3"], r["Xl4"]["ms_q3"] / r[k]["ms_q1"]]
        r.update({"datagrams": n, "frames": slots, "read_bytes": R, "written_bytes": W})
        # ---- the same bytes by every way; the datagram arena is not written by Xl4 ----
        arena.copy_(pristine)
        Xl4()
        torch.cuda.synchronize()
        r["arena_written_by_Xl4"] = int(not torch.equal(arena, pristine))
        B()
        torch.cuda.synchronize()
        r["out_differs_from_B"] = int(not torch.equal(out, out2))
        if "XS" in vers:
            arena.copy_(pristine)
            vers["XS"]()
            torch.cuda.synchronize()
            r["out_differs_from_XS"] = int(not torch.equal(out, out2))
        want = na.TXF_WHOLE | na.TXF_FRAGMENTED | na.TXD_L4_CSUM_SET | (17 << na.TXD_PROTO_SHIFT)
        st_np = status.cpu().numpy().view(np.uint32)
        r["status_not_udp_set"] = int(((st_np | (na.TXF_WHOLE | na.TXF_FRAGMENTED)) != want).sum())
        # ---- all frames of 32 seeded datagrams against the model ----
        arena.copy_(pristine)
        first_np = first.cpu().numpy()
        bad = frames_checked = 0
        for i in np.random.default_rng(seed + 2).integers(0, n, 32):
            i = int(i)
            o, D = int(off[i].item()), int(D_np[i])
            dg = arena[o:o + D].cpu().numpy().tobytes()
            mac = l2[12 * i:12 * i + 12].cpu().numpy().tobytes()
            st, fr, crcs = dm.frames(fcs_oracle, inet_oracle, dg, mac, MTU, FLAGS)
            k0 = int(first_np[i])
            ok = st == int(st_np[i]) and int(first_np[i + 1]) - k0 == len(fr)
            for q, body in enumerate(fr):
                got = out[(k0 + q) * SLOT:(k0 + q) * SLOT + len(body)].cpu().numpy().tobytes()
                ok = ok and got == body and int(flen[k0 + q].item()) == len(body) - 4
                frames_checked += 1
            bad += int(not ok)
        r["spot_datagrams"], r["spot_frames"], r["spot_bad"] = 32, frames_checked, bad
        r["last_launch"] = na.txd_last_launch()
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
