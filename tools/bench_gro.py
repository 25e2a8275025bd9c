#!/usr/bin/env python3
"""Device-resident cost of one-pass RX coalescing (include/nstack_gro.h) beside today's way, in one
process, the versions alternated:

  G    ip_rx_gro_plan_dev + ip_rx_gro_dev                   (the new plan, the coalescing build, the finishing launch)
  R    ether_rx_reasm_plan_dev + ip_rx_reasm_l4_dev         (today's way: every segment is delivered alone)
  A    one device-to-device copy of W = sum(dlen) bytes of G's datagrams                  (the floor)
Frames come from ip_tx_tso_dev (mtu 1500, TXF_F_FCS, slot 1518, mss as large as the mtu allows) over
TCP datagrams, each a flow of its own:
  tso32k          32 KiB datagrams whose seq is a multiple of 32768, in slot order
  tso32k_permuted the same frames with a seeded permutation of the slots
  mix             the 60 / 572 / 1500 / 8220 / 65535 mix as TCP (seq a multiple of 65536, so a 65535-byte
                  datagram comes back as two), in slot order
One HIP-event pair per version, `--rounds` rounds of the versions in turn after a warm-up round; median
and quartiles; G / R, G / A and the datagram-count ratio m_R / m_G. ip_tx_tso_dev fills every checksum,
so every datagram G delivers must read merged or checked-and-not-bad, and every one R delivers checked
and not bad: both verdict arrays are compared with that. Writes one JSON document (--out) and prints it.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

MIX = ((60, 0.40), (572, 0.25), (1500, 0.20), (8220, 0.14), (65535, 0.01))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=0.25, help="scales the batch sizes, as tools/bench_rxr.py")
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--skip", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gro_bench.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import nstack_amd as na
    from bench_rxv import alternate, stats
    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    cur = torch.cuda.current_stream
    MTU, SLOT, ALIGN = 1500, 1518, 16
    CLEAN = (6 << na.RXD_PROTO_SHIFT) | na.RXD_L4_CHECKED
    MERGED = (6 << na.RXD_PROTO_SHIFT) | na.GROD_MERGED
    res = {"engine": na.version(), "mtu": MTU, "slot": SLOT, "align": ALIGN, "rounds": a.rounds, "scale": a.scale,
           "note": "G = ip_rx_gro_plan_dev + ip_rx_gro_dev, R = ether_rx_reasm_plan_dev + ip_rx_reasm_l4_dev on the same frames, "
                   "A = one d2d copy of W = sum(dlen) bytes of G's datagrams; HIP events, versions alternated; GB_s = 2 W / time"}

    def frames_of(D_np, seq_step, seed):
        """ip_tx_tso_dev over splitmix TCP datagrams (20-byte headers both, ACK only), datagram i with
        source address i and seq i * seq_step."""
        n = len(D_np)
        ln = torch.from_numpy(D_np.view(np.int32)).to(dev)
        off = torch.zeros(n, dtype=torch.int64, device=dev)
        off[1:] = torch.cumsum(ln[:-1].to(torch.int64), 0)
        R = int(off[-1].item()) + int(D_np[-1])
        arena = torch.empty(R, dtype=torch.uint8, device=dev)
        na.fill_splitmix_dev(arena, R, seed, 0)
        l64 = ln.to(torch.int64)
        idx = torch.arange(n, dtype=torch.int64, device=dev)
        seq = (idx * seq_step) & 0xFFFFFFFF
        byte = lambda v, s: ((v >> s) & 255).to(torch.uint8)
        const = lambda v: torch.full((n,), v, dtype=torch.uint8, device=dev)
        cols = [(0, const(0x45)), (2, byte(l64, 8)), (3, byte(l64, 0)), (6, const(0)), (7, const(0)), (9, const(6)),
                (12, byte(idx, 24)), (13, byte(idx, 16)), (14, byte(idx, 8)), (15, byte(idx, 0))]
        tcp = [(24, byte(seq, 24)), (25, byte(seq, 16)), (26, byte(seq, 8)), (27, byte(seq, 0)), (32, const(0x50)), (33, const(0x10))]
        for col, src in cols:
            arena.index_put_((off + col,), src)
        has_tcp = l64 >= 40
        for col, src in tcp:
            arena.index_put_((off[has_tcp] + col,), src[has_tcp])
        l2 = torch.zeros(12, dtype=torch.uint8, device=dev)
        first = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        flags = na.TXF_F_FCS | na.TXF_F_L2_ONE
        na.tx_tso_plan_dev(arena, R, off, ln, None, n, MTU, first, flags)
        torch.cuda.synchronize()
        slots = int(first[-1].item())
        out = torch.zeros(slots * SLOT, dtype=torch.uint8, device=dev)
        flen = torch.zeros(slots, dtype=torch.int32, device=dev)
        na.tx_tso_dev(arena, R, off, ln, l2, None, n, MTU, first, out, SLOT, slots, flags, flen)
        torch.cuda.synchronize()
        return out, flen, slots, n

    def measure(name, wire, off, ln, n, datagrams):
        def arrays():
            return dict(fstat=torch.zeros(n, dtype=torch.int32, device=dev), dst=torch.zeros(n, dtype=torch.int64, device=dev),
                        dgi=torch.zeros(n, dtype=torch.int32, device=dev), doff=torch.zeros(n + 1, dtype=torch.int64, device=dev),
                        dlen=torch.zeros(n, dtype=torch.int32, device=dev), dlead=torch.zeros(n, dtype=torch.int32, device=dev),
                        counts=torch.zeros(2, dtype=torch.int64, device=dev), final=torch.zeros(n, dtype=torch.int32, device=dev),
                        dverdict=torch.zeros(n, dtype=torch.int32, device=dev), bad=torch.zeros(1, dtype=torch.int64, device=dev))
        g, r = arrays(), arrays()
        nbytes = wire.numel()

        def plan(fn, t):
            fn(wire, nbytes, off, ln, n, t["fstat"], t["dst"], t["dgi"], t["doff"], t["dlen"], t["dlead"], t["counts"],
               flags=na.RXR_F_TRAILER, align=ALIGN, stream=cur())

        def build(fn, t, out, total):
            fn(wire, nbytes, off, ln, n, t["fstat"], t["dst"], t["dgi"], t["doff"], t["dlen"], t["counts"], out, total,
               t["dverdict"], flags=na.RXR_F_TRAILER, fstat=t["final"], bad_mask=na.RXD_L4_BAD_CSUM, bad=t["bad"], stream=cur())

        plan(na.rx_gro_plan_dev, g)
        plan(na.rx_reasm_plan_dev, r)
        torch.cuda.synchronize()
        (mg, tg), (mr, tr) = ((int(x) for x in t["counts"].cpu().numpy()) for t in (g, r))
        out_g = torch.zeros(tg + 16, dtype=torch.uint8, device=dev)
        out_r = torch.zeros(tr + 16, dtype=torch.uint8, device=dev)
        W = int(g["dlen"][:mg].to(torch.int64).sum().item())
        Wr = int(r["dlen"][:mr].to(torch.int64).sum().item())

        def G():
            plan(na.rx_gro_plan_dev, g)
            build(na.rx_gro_dev, g, out_g, tg)

        def R():
            plan(na.rx_reasm_plan_dev, r)
            build(na.rx_reasm_l4_dev, r, out_r, tr)

        ca = torch.empty(W, dtype=torch.uint8, device=dev)
        cb = torch.empty(W, dtype=torch.uint8, device=dev)

        def A():
            cb.copy_(ca)

        ms = alternate({"G": G, "R": R, "A": A}, a.rounds, torch)
        o = {k: stats(v, 2 * W) for k, v in ms.items()}
        for k, over in (("G", "R"), ("G", "A"), ("R", "A")):
            o[f"{k}_over_{over}"] = o[k]["ms_median"] / o[over]["ms_median"]
            o[f"{k}_over_{over}_q1q3"] = [o[k]["ms_q1"] / o[over]["ms_q3"], o[k]["ms_q3"] / o[over]["ms_q1"]]
        G()
        R()
        torch.cuda.synchronize()
        dg = g["dverdict"][:mg].cpu().numpy().view(np.uint32)
        dr = r["dverdict"][:mr].cpu().numpy().view(np.uint32)
        fin = g["final"].cpu().numpy().view(np.uint32)
        o.update({"frames": n, "segmented_datagrams": datagrams, "datagrams_G": mg, "datagrams_R": mr, "mR_over_mG": mr / max(mg, 1),
                  "delivered_bytes_G": W, "delivered_bytes_R": Wr, "merged_datagrams": int((dg == MERGED).sum()),
                  "frames_merged": int(((fin & na.GRO_MERGED) != 0).sum()),
                  "verdicts_G_not_merged_or_clean": int(((dg != MERGED) & (dg != CLEAN)).sum()),
                  "verdicts_R_not_clean": int((dr != CLEAN).sum()), "bad_G": int(g["bad"].item()), "bad_R": int(r["bad"].item()),
                  "last_launch": na.gro_last_launch()})
        res[name] = o
        print(name, json.dumps(o), flush=True)

    s = a.scale
    if "tso32k" not in a.skip:
        wire, flen, slots, datagrams = frames_of(np.full(int(100_000 * s), 32768, dtype=np.uint32), 32768, 61)
        ln = (flen + 4).contiguous()
        off = torch.arange(slots, dtype=torch.int64, device=dev) * SLOT
        measure("tso32k", wire, off, ln, slots, datagrams)
        perm = torch.from_numpy(np.random.default_rng(65).permutation(slots)).to(dev)
        measure("tso32k_permuted", wire, off[perm].contiguous(), ln[perm].contiguous(), slots, datagrams)
        del wire
        torch.cuda.empty_cache()
    if "mix" not in a.skip:
        n = int(1_000_000 * s)
        counts = [int(n * w) for _, w in MIX]
        counts[0] += n - sum(counts)
        D = np.repeat(np.array([d for d, _ in MIX], dtype=np.uint32), counts)
        np.random.default_rng(7).shuffle(D)
        wire, flen, slots, datagrams = frames_of(D, 65536, 71)
        ln = (flen + 4).contiguous()
        off = torch.arange(slots, dtype=torch.int64, device=dev) * SLOT
        measure("mix", wire, off, ln, slots, datagrams)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1), flush=True)


if __name__ == "__main__":
    main()
