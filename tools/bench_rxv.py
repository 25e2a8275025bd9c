#!/usr/bin/env python3
"""Device-resident throughput of the one-pass RX validator (include/nstack_rxv.h) beside what a
caller has to launch without it, on the same buffer, in one process, the versions alternated:

  A  ether_fcs_verify_fixed_dev alone                    (the floor: the same bytes, CRC only)
  B  A + inet_csum_fixed_dev(IP, +14, 20) + inet_csum_fixed_dev(TCP, +34, 1480)
                                                         (three launches: what a caller needs today)
  C  ether_rx_validate_fixed_dev through the LDS-DMA kernel (one launch, one read)
  D  ether_rx_validate_fixed_dev through the general kernel
on N x 1518-B frames (splitmix bytes, the headers stamped so that every frame takes the full TCP
path: ethertype 0x0800, vhl 0x45, ip_len 1500, proto 6, foff 0; the checksums themselves read "bad",
which costs the same work), A, B and D on 2 N IMIX frames (7:4:1 of 64/576/1518 B, packed;
variable forms, ip_len = len - 18; the general kernel only), and C and D with RXV_F_TRAILER off. Timing: one HIP-event pair per
launch (B: around its three launches), `--rounds` rounds of the versions in turn after a
warm-up round; per version the median, the minimum and the spread (quartiles, extremes) of its
rounds. Spot checks use the independent witness of tests/golden/make_rxv_golden.py. Writes one JSON
document (--out) and prints it.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))


def stats(ms, nbytes):
    import numpy as np
    a = np.sort(np.array(ms))
    med = float(np.median(a))
    return {"ms_median": med, "ms_min": float(a[0]), "ms_max": float(a[-1]), "ms_q1": float(np.percentile(a, 25)),
            "ms_q3": float(np.percentile(a, 75)), "rounds": len(ms), "GB_s_median": nbytes / med / 1e6,
            "spread_pct": 100.0 * float(np.percentile(a, 75) - np.percentile(a, 25)) / med}


def alternate(versions, rounds, torch):
    """versions: {name: fn}. One warm-up round, then `rounds` rounds of every version in turn, each
    launch (group) between its own pair of events."""
    st = torch.cuda.current_stream()
    for fn in versions.values():
        fn()
    torch.cuda.synchronize()
    ev = {k: [] for k in versions}
    for _ in range(rounds):
        for k, fn in versions.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            fn()
            e1.record(st)
            ev[k].append((e0, e1))
    torch.cuda.synchronize()
    return {k: [e0.elapsed_time(e1) for e0, e1 in v] for k, v in ev.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64 << 20, help="1518-B frames (IMIX: twice as many)")
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--skip", default="")
    ap.add_argument("--only", default="", help="run only this version's launches (for a profiler run): A, B, C or D")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rxv_bench.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import nstack_amd as na
    import make_rxv_golden as gen
    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(23)
    cur = torch.cuda.current_stream
    res = {"engine": na.version(), "frames_1518": a.frames, "rounds": a.rounds,
           "note": "A = FCS verify alone; B = A + inet IP header + inet TCP segment (3 launches); "
                   "C / D = ether_rx_validate (1 launch) through the LDS-DMA / the general kernel; times per launch (group), HIP events, versions alternated"}

    def keep(versions):
        return {k: f for k, f in versions.items() if not a.only or k.split("_")[0] == a.only}

    def spot(arena_t, offs, lens, got, flags):
        bad = 0
        for i in rng.integers(0, len(got), 32):
            o, L = int(offs[i]), int(lens[i])
            bad += int(gen.expect(arena_t[o:o + L].cpu().numpy().tobytes(), flags) != int(got[i]))
        return bad

    def report(name, ms, nbytes):
        out = {k: stats(v, nbytes) for k, v in ms.items()}
        for x in ("C", "D"):
            if x in out and "A" in out and "B" in out:
                out[x + "_over_A"] = out[x]["ms_median"] / out["A"]["ms_median"]
                out[x + "_over_B"] = out[x]["ms_median"] / out["B"]["ms_median"]
        if "C" in out and "D" in out:
            out["C_over_D"] = out["C"]["ms_median"] / out["D"]["ms_median"]
        res[name] = out
        print(name, json.dumps(out), flush=True)

    n, S = a.frames, 1518
    if "fixed" not in a.skip:
        frames = torch.empty(n * S + 64, dtype=torch.uint8, device=dev)
        na.fill_splitmix_dev(frames, n * S + 64, 5, 0)
        v2 = frames[:n * S].view(n, S)
        for col, val in ((12, 0x08), (13, 0x00), (14, 0x45), (16, 1500 >> 8), (17, 1500 & 255), (20, 0), (21, 0), (23, 6)):
            v2[:, col] = val
        ok = torch.empty(n, dtype=torch.uint8, device=dev)
        bad = torch.zeros(1, dtype=torch.int64, device=dev)
        c16 = torch.empty(n, dtype=torch.int16, device=dev)
        addr = torch.zeros(2 * n, dtype=torch.int32, device=dev)
        verdict = torch.empty(n, dtype=torch.int32, device=dev)
        p = frames.data_ptr()

        def A():
            na.verify_fixed_dev(p, S, S, n, ok, bad, cur())

        def B():
            A()
            na.inet_fixed_dev("ip", p + 14, S, 20, n, None, c16, cur())
            na.inet_fixed_dev("tcp", p + 34, S, 1480, n, addr, c16, cur())

        def rxv(dma, flags, mask):
            def go():
                na.rx_validate_set_dma_threshold(0 if dma else (1 << 63))   # the route is taken at launch
                na.rx_validate_fixed_dev(p, S, S, n, verdict, flags=flags, bad_mask=mask, bad=bad, stream=cur())
            return go

        C, D = rxv(True, na.RXV_F_TRAILER, na.RXV_FCS_BAD), rxv(False, na.RXV_F_TRAILER, na.RXV_FCS_BAD)
        C_plain, D_plain = rxv(True, 0, na.RXV_L4_BAD_CSUM), rxv(False, 0, na.RXV_L4_BAD_CSUM)
        ms = alternate(keep({"A": A, "B": B, "C": C, "D": D, "C_plain": C_plain, "D_plain": D_plain}), a.rounds, torch)
        report("fixed_1518", ms, n * S)
        if not a.only:
            C()
            torch.cuda.synchronize()
            assert na.rxv_last_launch() == "lds-dma"
            vc = verdict.clone()
            D()
            torch.cuda.synchronize()
            assert na.rxv_last_launch() == "general"
            res["fixed_1518"]["C_differs_from_D"] = int((vc != verdict).sum().item())
        if not a.only:
            offs, lens = np.arange(n, dtype=np.int64) * S, np.full(n, S)
            D()
            torch.cuda.synchronize()
            got = verdict.cpu().numpy().view(np.uint32)
            res["fixed_1518"]["spot_bad"] = spot(frames, offs, lens, got, 1)
            res["fixed_1518"]["verdict_histogram"] = {hex(int(k)): int(c) for k, c in
                                                      zip(*np.unique(got & 0xFFFF, return_counts=True))}
        del frames, v2, ok, c16, addr, verdict
        torch.cuda.empty_cache()

    if "imix" not in a.skip:
        m = 2 * n
        counts = [m * 7 // 12, m * 4 // 12]
        counts.append(m - sum(counts))
        ln_np = np.repeat(np.array([64, 576, 1518], dtype=np.uint32), counts)
        np.random.default_rng(7).shuffle(ln_np)
        ln = torch.from_numpy(ln_np.view(np.int32)).to(dev)
        off = torch.zeros(m, dtype=torch.int64, device=dev)
        off[1:] = torch.cumsum(ln[:-1].to(torch.int64), 0)
        total = int(off[-1].item()) + int(ln_np[-1])
        arena = torch.empty(total, dtype=torch.uint8, device=dev)
        na.fill_splitmix_dev(arena, total, 6, 0)
        ipl = (ln - 18).to(torch.int64)
        for col, val in ((12, 0x08), (13, 0x00), (14, 0x45), (16, None), (17, None), (20, 0), (21, 0), (23, 6)):
            src = (ipl >> 8 if col == 16 else ipl & 255).to(torch.uint8) if val is None else \
                torch.full((m,), val, dtype=torch.uint8, device=dev)
            arena.index_put_((off + col,), src)
        del src
        ok = torch.empty(m, dtype=torch.uint8, device=dev)
        bad = torch.zeros(1, dtype=torch.int64, device=dev)
        c16 = torch.empty(m, dtype=torch.int16, device=dev)
        addr = torch.zeros(2 * m, dtype=torch.int32, device=dev)
        verdict = torch.empty(m, dtype=torch.int32, device=dev)
        off_ip, off_tcp = off + 14, off + 34
        len_ip = torch.full((m,), 20, dtype=torch.int32, device=dev)
        len_tcp = ln - 38
        del ipl
        torch.cuda.empty_cache()

        def A():
            na.verify_dev(arena, total, off, ln, ok, bad, m, cur())

        def B():
            A()
            na.inet_batch_dev("ip", arena, total, off_ip, len_ip, None, c16, m, cur())
            na.inet_batch_dev("tcp", arena, total, off_tcp, len_tcp, addr, c16, m, cur())

        def D():
            na.rx_validate_dev(arena, total, off, ln, verdict, m, flags=na.RXV_F_TRAILER, bad_mask=na.RXV_FCS_BAD,
                               bad=bad, stream=cur())

        def D_plain():
            na.rx_validate_dev(arena, total, off, ln, verdict, m, flags=0, bad_mask=na.RXV_L4_BAD_CSUM, bad=bad,
                               stream=cur())

        ms = alternate(keep({"A": A, "B": B, "D": D, "D_plain": D_plain}), a.rounds, torch)
        report("imix", ms, total)
        res["imix"]["frames"] = m
        res["imix"]["bytes"] = total
        if not a.only:
            D()
            torch.cuda.synchronize()
            got = verdict.cpu().numpy().view(np.uint32)
            res["imix"]["spot_bad"] = spot(arena, off.cpu().numpy(), ln_np, got, 1)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1), flush=True)


if __name__ == "__main__":
    main()
