#!/usr/bin/env python3
"""Device-resident cost of the L4 verdicts of reassembled datagrams (include/nstack_rxd.h) beside the
plain build and beside today's two-pass way, in one process, the versions alternated:

  D    ether_rx_reasm_dev                                   (the plain build, on the plan's arrays)
  Dl4  ip_rx_reasm_l4_dev                                   (D': the build with sums plus the verdict launch)
  B    D + one inet_csum_batch_dev("udp") over the delivered segments; its seg_off / seg_len / addr
       arrays are prepared outside the timed window, so B is a lower bound for the two-pass way (the
       host parse that produces them is not counted)
  A    one device-to-device copy of W = sum(dlen) bytes                                   (the floor)
Workloads and protocol are tools/bench_rxr.py's: frames from ether_tx_frame_dev (mtu 1500, TXF_F_FCS,
slot 1518) over datagrams of 8220 bytes, of 1400 bytes and a 60 / 572 / 1500 / 8220 / 65535 mix, each
in slot order and with a seeded permutation of the slots; one HIP-event pair per version, `--rounds`
rounds of the versions in turn after a warm-up round; median and quartiles. Every datagram is UDP with
a valid checksum (computed on the device with inet_csum_batch_dev and stamped into the field), so
every delivered datagram's verdict must read checked and not bad: the whole dverdict array is compared
with that, and with B's checksums. Writes one JSON document (--out) and prints it.
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rxd_bench.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import nstack_amd as na
    from bench_rxv import alternate, stats
    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    cur = torch.cuda.current_stream
    MTU, SLOT, ALIGN = 1500, 1518, 16
    CLEAN = (17 << na.RXD_PROTO_SHIFT) | na.RXD_L4_CHECKED
    res = {"engine": na.version(), "mtu": MTU, "slot": SLOT, "align": ALIGN, "rounds": a.rounds, "scale": a.scale,
           "note": "D = plain build, Dl4 = build with sums + verdict launch (D'), B = D + inet_csum_batch_dev(udp) over the "
                   "delivered segments (arrays prepared outside the timed window), A = one d2d copy of W = sum(dlen) bytes; "
                   "HIP events, versions alternated; GB_s = 2 W / time"}

    def frames_of(D_np, seed):
        """ether_tx_frame_dev over splitmix UDP datagrams (20-byte headers) with valid checksums."""
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
                         (9, torch.full((n,), 17, dtype=torch.uint8, device=dev)), (26, zero), (27, zero)):
            arena.index_put_((off + col,), src)
        # the UDP checksum of every datagram's segment, computed where it lies and stamped into its field
        seg_off, seg_len = (off + 20).contiguous(), (ln - 20).contiguous()
        addr = torch.stack([arena[off + 12 + c] for c in range(8)], 1).contiguous().view(torch.int32)   # the words as they lie
        csum = torch.zeros(n, dtype=torch.int16, device=dev)
        na.inet_batch_dev("udp", arena, R, seg_off, seg_len, addr, csum, n)
        torch.cuda.synchronize()
        c32 = csum.to(torch.int32) & 0xFFFF
        c32 = torch.where(c32 == 0, torch.full_like(c32, 0xFFFF), c32)   # src/udp.c: a computed zero goes out as 0xffff
        arena.index_put_((off + 26,), (c32 & 255).to(torch.uint8))
        arena.index_put_((off + 27,), (c32 >> 8).to(torch.uint8))
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

    def measure(name, wire, off, ln, n, datagrams):
        t = dict(fstat=torch.zeros(n, dtype=torch.int32, device=dev), dst=torch.zeros(n, dtype=torch.int64, device=dev),
                 dgi=torch.zeros(n, dtype=torch.int32, device=dev), doff=torch.zeros(n + 1, dtype=torch.int64, device=dev),
                 dlen=torch.zeros(n, dtype=torch.int32, device=dev), dlead=torch.zeros(n, dtype=torch.int32, device=dev),
                 counts=torch.zeros(2, dtype=torch.int64, device=dev), final=torch.zeros(n, dtype=torch.int32, device=dev),
                 dverdict=torch.zeros(n, dtype=torch.int32, device=dev), bad=torch.zeros(1, dtype=torch.int64, device=dev))
        nbytes = wire.numel()
        na.rx_reasm_plan_dev(wire, nbytes, off, ln, n, t["fstat"], t["dst"], t["dgi"], t["doff"], t["dlen"], t["dlead"],
                             t["counts"], flags=na.RXR_F_TRAILER, align=ALIGN, stream=cur())
        torch.cuda.synchronize()
        m, total = (int(x) for x in t["counts"].cpu().numpy())
        out = torch.zeros(total + 16, dtype=torch.uint8, device=dev)
        W = int(t["dlen"][:m].to(torch.int64).sum().item())

        def D():
            na.rx_reasm_dev(wire, nbytes, off, ln, n, t["fstat"], t["dst"], t["dgi"], t["doff"], t["dlen"], out, total,
                            flags=na.RXR_F_TRAILER, fstat=t["final"], stream=cur())

        def Dl4():
            na.rx_reasm_l4_dev(wire, nbytes, off, ln, n, t["fstat"], t["dst"], t["dgi"], t["doff"], t["dlen"], t["counts"], out,
                               total, t["dverdict"], flags=na.RXR_F_TRAILER, fstat=t["final"], bad_mask=na.RXD_L4_BAD_CSUM,
                               bad=t["bad"], stream=cur())

        # B's arrays, from the datagrams a first build delivered (outside the timed window)
        D()
        torch.cuda.synchronize()
        doff = t["doff"][:m]
        seg_off, seg_len = (doff + 20).contiguous(), (t["dlen"][:m] - 20).contiguous()
        addr = torch.stack([out[doff + 12 + c] for c in range(8)], 1).contiguous().view(torch.int32)
        sums = torch.full((m,), 0x5555, dtype=torch.int16, device=dev)

        def B():
            D()
            na.inet_batch_dev("udp", out, total, seg_off, seg_len, addr, sums, m, stream=cur())

        ca = torch.empty(W, dtype=torch.uint8, device=dev)
        cb = torch.empty(W, dtype=torch.uint8, device=dev)

        def A():
            cb.copy_(ca)

        ms = alternate({"D": D, "Dl4": Dl4, "B": B, "A": A}, a.rounds, torch)
        r = {k: stats(v, 2 * W) for k, v in ms.items()}
        for k, over in (("Dl4", "D"), ("Dl4", "B"), ("D", "A"), ("Dl4", "A")):
            r[f"{k}_over_{over}"] = r[k]["ms_median"] / r[over]["ms_median"]
            r[f"{k}_over_{over}_q1q3"] = [r[k]["ms_q1"] / r[over]["ms_q3"], r[k]["ms_q3"] / r[over]["ms_q1"]]
        # every delivered datagram is valid UDP: checked and not bad, by both ways
        Dl4()
        B()
        torch.cuda.synchronize()
        dv = t["dverdict"][:m].cpu().numpy().view(np.uint32)
        fin = t["final"].cpu().numpy().view(np.uint32)
        r.update({"frames": n, "framed_datagrams": datagrams, "datagrams": m, "delivered_bytes": W,
                  "frames_incomplete": int(((fin & na.RXR_INCOMPLETE) != 0).sum()),
                  "verdicts_not_clean": int((dv != CLEAN).sum()), "bad": int(t["bad"].item()),
                  "two_pass_not_zero": int((sums != 0).sum().item()), "last_launch": na.rxd_last_launch()})
        res[name] = r
        print(name, json.dumps(r), flush=True)

    def workload(name, D_np, seed):
        wire, flen, slots, datagrams = frames_of(D_np, seed)
        ln = (flen + 4).contiguous()
        off = torch.arange(slots, dtype=torch.int64, device=dev) * SLOT
        measure(name + "_ordered", wire, off, ln, slots, datagrams)
        perm = torch.from_numpy(np.random.default_rng(seed + 4).permutation(slots)).to(dev)
        measure(name + "_permuted", wire, off[perm].contiguous(), ln[perm].contiguous(), slots, datagrams)

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
