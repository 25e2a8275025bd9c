#!/usr/bin/env python3
"""Device-resident throughput of one-pass TX sealing (include/nstack_txs.h) beside what a caller
has to launch without it, on the same buffer, in one process, the versions alternated:

  A  ether_fcs_fixed_dev alone                           (the floor: the same bytes, CRC only)
  B  A + inet_csum_fixed_dev(IP, +14, 20) + inet_csum_fixed_dev(TCP, +34, 1480)
                                                         (the three launches a caller runs today)
  C  ether_tx_seal_fixed_dev through the LDS-DMA kernel  (one launch, one read, fields stored)
  D  ether_tx_seal_fixed_dev through the general kernel
on N x 1514-B frames at stride 1518 (the packed TX shape; splitmix bytes, the headers stamped so that
every frame takes the full TCP path: ethertype 0x0800, vhl 0x45, ip_len 1500, proto 6, foff 0), A, B
and D on 2 N IMIX frames (7:4:1 of 60/572/1514 B, each with its FCS place; variable forms; the general
kernel only), and C and D without TXS_F_FCS. B UNDERSTATES today's cost: it leaves out the caller's
two scatter kernels, and its FCS is that of the unpatched bytes. Sealing ignores the fields' old
content, so every round does the same work on the same buffer. Timing: one HIP-event pair per launch
(B: around its three launches), `--rounds` rounds of the versions in turn after a warm-up round; per
version the median, the minimum and the spread (quartiles, extremes) of its rounds. All status words
and fields records and every arena byte of C and D are compared, and a seeded sample of frames (copied
out before the first sealing) against the model (tests/txs_model.py on the oracles of oracle/_build)
and against the independent witness of tests/golden/make_txs_golden.py. Writes one JSON document
(--out) and prints it.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def load_oracles():
    """The CPU restatements the model takes its arithmetic from (built by `make -C oracle`)."""
    import ctypes
    build = os.path.join(ROOT, "oracle", "_build")
    fcs = ctypes.CDLL(os.path.join(build, "liboracle.so"))
    fcs.oracle_ether_fcs.restype = ctypes.c_uint32
    fcs.oracle_ether_fcs.argtypes = [ctypes.c_void_p, ctypes.c_size_t]
    inet = ctypes.CDLL(os.path.join(build, "liboracle_inet.so"))
    u16, u32, vp, sz = ctypes.c_uint16, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_size_t
    inet.oracle_ip_checksum.restype = u16
    inet.oracle_ip_checksum.argtypes = [vp, sz]
    inet.oracle_tcp_checksum.restype = u16
    inet.oracle_tcp_checksum.argtypes = [u32, u32, vp, sz]
    inet.oracle_udp_checksum.restype = u16
    inet.oracle_udp_checksum.argtypes = [vp, sz, u32, u32]
    return fcs, inet


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=32 << 20, help="1514-B frames (IMIX: twice as many)")
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--skip", default="")
    ap.add_argument("--only", default="", help="run only this version's launches (for a profiler run): A, B, C or D")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "txs_bench.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import nstack_amd as na
    import make_txs_golden as gen
    import txs_model as tm
    fcs_oracle, inet_oracle = load_oracles()
    from bench_rxv import alternate, stats
    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    cur = torch.cuda.current_stream
    FCS = na.TXS_F_FCS
    res = {"engine": na.version(), "frames_1514": a.frames, "rounds": a.rounds,
           "note": "A = FCS alone; B = A + inet IP header + inet TCP segment (3 launches, no scatter, FCS of the "
                   "unpatched bytes); C / D = ether_tx_seal (1 launch, fields and FCS stored) through the LDS-DMA / "
                   "the general kernel; times per launch (group), HIP events, versions alternated"}

    def keep(versions):
        return {k: f for k, f in versions.items() if not a.only or k.split("_")[0] == a.only}

    def report(name, ms, nbytes):
        out = {k: stats(v, nbytes) for k, v in ms.items()}
        for x in ("C", "D"):
            if x in out and "A" in out and "B" in out:
                out[x + "_over_A"] = out[x]["ms_median"] / out["A"]["ms_median"]
                out[x + "_over_B"] = out[x]["ms_median"] / out["B"]["ms_median"]
        if "C" in out and "D" in out:
            c, d = out["C"], out["D"]
            out["C_over_D"] = c["ms_median"] / d["ms_median"]
            gain = d["ms_median"] - c["ms_median"]
            out["C_beats_D_by_more_than_the_larger_spread"] = bool(
                gain > max(c["ms_q3"] - c["ms_q1"], d["ms_q3"] - d["ms_q1"]))
        res[name] = out
        print(name, json.dumps(out), flush=True)

    def sample(arena_t, offs, lens, k=32, seed=23):
        """[(index, bytes of the frame and its FCS place)] of k seeded frames, as they lie now."""
        idx = np.random.default_rng(seed).integers(0, len(offs), k)
        return [(int(i), arena_t[int(offs[i]):int(offs[i]) + int(lens[i]) + 4].cpu().numpy().tobytes()) for i in idx]

    def spot(before, arena_t, offs, status, fields, flags):
        """(sample frames that differ from the model, from the independent witness)."""
        bad_model = bad_witness = 0
        for i, raw in before:
            o, L = int(offs[i]), len(raw) - 4
            rec = fields[i].cpu().numpy().view(np.uint32)
            got_fl = [int(rec[0] & 0xFFFF), int(rec[0] >> 16), int(rec[1])]
            got_st = int(status[i].item()) & 0xFFFFFFFF
            out, st, fl = tm.seal(fcs_oracle, inet_oracle, raw[:L], flags)
            now = arena_t[o:o + len(out)].cpu().numpy().tobytes()
            bad_model += int(now != out or st != got_st or got_fl != list(fl))
            out, st, fl, _ = gen.expect(raw[:L], flags)
            bad_witness += int(now != out or st != got_st or got_fl != fl)
        return bad_model, bad_witness

    n, F, S = a.frames, 1514, 1518
    if "fixed" not in a.skip:
        frames = torch.empty(n * S + 64, dtype=torch.uint8, device=dev)
        na.fill_splitmix_dev(frames, n * S + 64, 5, 0)
        v2 = frames[:n * S].view(n, S)
        for col, val in ((12, 0x08), (13, 0x00), (14, 0x45), (16, 1500 >> 8), (17, 1500 & 255), (20, 0), (21, 0), (23, 6)):
            v2[:, col] = val
        crc = torch.empty(n, dtype=torch.int32, device=dev)
        cnt = torch.zeros(1, dtype=torch.int64, device=dev)
        c16 = torch.empty(n, dtype=torch.int16, device=dev)
        addr = torch.zeros(2 * n, dtype=torch.int32, device=dev)
        status = torch.empty(n, dtype=torch.int32, device=dev)
        fields = torch.empty((n, 2), dtype=torch.int32, device=dev)
        p = frames.data_ptr()
        offs, lens = np.arange(n, dtype=np.int64) * S, np.full(n, F)
        before = None if a.only else sample(frames, offs, lens)

        def A():
            na.fixed_dev(p, S, F, n, crc, cur())

        def B():
            A()
            na.inet_fixed_dev("ip", p + 14, S, 20, n, None, c16, cur())
            na.inet_fixed_dev("tcp", p + 34, S, 1480, n, addr, c16, cur())

        def seal(dma, flags):
            def go():
                na.tx_seal_set_dma_threshold(0 if dma else (1 << 63))   # the route is taken at launch
                na.tx_seal_fixed_dev(p, S, F, n, flags=flags, count_mask=na.TXS_L4_CSUM_SET, status=status,
                                     fields=fields, count=cnt, stream=cur())
            return go

        C, D = seal(True, FCS), seal(False, FCS)
        C_nofcs, D_nofcs = seal(True, 0), seal(False, 0)
        ms = alternate(keep({"A": A, "B": B, "C": C, "D": D, "C_nofcs": C_nofcs, "D_nofcs": D_nofcs}), a.rounds, torch)
        report("fixed_1514", ms, n * S)
        if not a.only:
            C()
            torch.cuda.synchronize()
            assert na.txs_last_launch() == "lds-dma"
            sc, fc, ac = status.clone(), fields.clone(), frames.clone()
            D()
            torch.cuda.synchronize()
            assert na.txs_last_launch() == "general"
            r = res["fixed_1514"]
            r["C_differs_from_D"] = int((sc != status).sum().item()) + int((fc != fields).sum().item())
            r["C_arena_equals_D_arena"] = bool(torch.equal(ac, frames))   # every byte
            del sc, fc, ac
            r["count"] = int(cnt.item())
            r["spot_bad_model"], r["spot_bad_witness"] = spot(before, frames, offs, status, fields, FCS)
            r["status_histogram"] = {hex(int(k)): int(c) for k, c in
                                     zip(*np.unique(status.cpu().numpy().view(np.uint32) & 0xFFFF, return_counts=True))}
        del frames, v2, crc, c16, addr, status, fields
        torch.cuda.empty_cache()

    if "imix" not in a.skip:
        m = 2 * n
        counts = [m * 7 // 12, m * 4 // 12]
        counts.append(m - sum(counts))
        ln_np = np.repeat(np.array([60, 572, 1514], dtype=np.uint32), counts)
        np.random.default_rng(7).shuffle(ln_np)
        ln = torch.from_numpy(ln_np.view(np.int32)).to(dev)
        off = torch.zeros(m, dtype=torch.int64, device=dev)
        off[1:] = torch.cumsum(ln[:-1].to(torch.int64) + 4, 0)     # every frame with its FCS place
        total = int(off[-1].item()) + int(ln_np[-1]) + 4
        arena = torch.empty(total, dtype=torch.uint8, device=dev)
        na.fill_splitmix_dev(arena, total, 6, 0)
        ipl = (ln - 14).to(torch.int64)
        for col, val in ((12, 0x08), (13, 0x00), (14, 0x45), (16, None), (17, None), (20, 0), (21, 0), (23, 6)):
            src = (ipl >> 8 if col == 16 else ipl & 255).to(torch.uint8) if val is None else \
                torch.full((m,), val, dtype=torch.uint8, device=dev)
            arena.index_put_((off + col,), src)
        del src
        crc = torch.empty(m, dtype=torch.int32, device=dev)
        cnt = torch.zeros(1, dtype=torch.int64, device=dev)
        c16 = torch.empty(m, dtype=torch.int16, device=dev)
        addr = torch.zeros(2 * m, dtype=torch.int32, device=dev)
        status = torch.empty(m, dtype=torch.int32, device=dev)
        fields = torch.empty((m, 2), dtype=torch.int32, device=dev)
        off_ip, off_tcp = off + 14, off + 34
        len_ip = torch.full((m,), 20, dtype=torch.int32, device=dev)
        len_tcp = ln - 34
        del ipl
        torch.cuda.empty_cache()
        off_np = off.cpu().numpy()
        before = None if a.only else sample(arena, off_np, ln_np)

        def A():
            na.batch_dev(arena, total, off, ln, crc, m, cur())

        def B():
            A()
            na.inet_batch_dev("ip", arena, total, off_ip, len_ip, None, c16, m, cur())
            na.inet_batch_dev("tcp", arena, total, off_tcp, len_tcp, addr, c16, m, cur())

        def D():
            na.tx_seal_dev(arena, total, off, ln, m, flags=FCS, count_mask=na.TXS_L4_CSUM_SET, status=status,
                           fields=fields, count=cnt, stream=cur())

        def D_nofcs():
            na.tx_seal_dev(arena, total, off, ln, m, flags=0, count_mask=na.TXS_L4_CSUM_SET, status=status,
                           fields=fields, count=cnt, stream=cur())

        ms = alternate(keep({"A": A, "B": B, "D": D, "D_nofcs": D_nofcs}), a.rounds, torch)
        report("imix", ms, total)
        res["imix"]["frames"] = m
        res["imix"]["bytes"] = total
        if not a.only:
            D()
            torch.cuda.synchronize()
            res["imix"]["count"] = int(cnt.item())
            res["imix"]["spot_bad_model"], res["imix"]["spot_bad_witness"] = spot(before, arena, off_np, status, fields, FCS)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1), flush=True)


if __name__ == "__main__":
    main()
