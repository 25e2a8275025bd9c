#!/usr/bin/env python3
"""Device-resident cost of one-pass TCP segmentation (include/nstack_tso.h) beside IP fragmentation of
the same datagrams and beside today's two-pass way, in one process, the versions alternated:

  T    ip_tx_tso_dev                                        (the new call: MSS segments, each sealed)
  Xl4  ip_tx_frame_l4_dev on the same datagrams             (X': IP fragments, about the same bytes; T / Xl4
       is what per-frame headers and per-frame checksums cost)
  B    today's way: a device gather (torch index arithmetic: the library ships no kernel for it) that
       writes the expanded datagrams, headers replicated, into a second arena, an index_put_ of every
       segment's ip_len, ip_id, tcp_seqno and flags, then ip_tx_frame_l4_dev over the expanded
       datagrams. The gather moves dwords (datagrams lie at multiples of 4 for that) through an int32
       index; index and field arrays are prepared outside the timed window, so the host parse and
       the host arithmetic that produce them are not counted: B is a lower bound for the two-pass way.
The plans (ip_tx_tso_plan_dev, ether_tx_frame_plan_dev) run once, outside the timed window.
Workloads: every datagram TCP (ACK | PSH) with hlen 20 and thl 20 and garbage in both checksum fields;
25 k x 65535 B, 100 k x 8220 B and the 60 / 572 / 1500 / 8220 / 65535 mix of tools/bench_txf.py at a
quarter of its size. mtu 1500 (--mtu 9000: every full frame of a segmented datagram has six walk
segments and is visited twice), TXF_F_FCS, slot 14 + mtu + 4, per-datagram MAC records, the NULL mss
array. One HIP-event pair per version, `--rounds` rounds of the versions in turn after a warm-up round;
median and quartiles. Checks: the whole output arena of T equals B's, the datagram arena is not written
by T, and all frames of 32 seeded datagrams are compared with the model (tests/tso_model.py on the
oracles of oracle/_build). Writes one JSON document (--out) and prints it.
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
HB = 40   # hlen 20 + thl 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=0.25, help="scales the batch sizes")
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--skip", default="")
    ap.add_argument("--mtu", type=int, default=1500)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tso_bench.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import nstack_amd as na
    import tso_model as tm
    from bench_rxv import alternate, stats
    from bench_txs import load_oracles
    fcs_oracle, inet_oracle = load_oracles()
    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    cur = torch.cuda.current_stream
    MTU, FLAGS, SLOT = a.mtu, na.TXF_F_FCS, 14 + a.mtu + 4
    M = MTU - HB   # the effective MSS of every datagram: a multiple of 4 at both mtus
    assert M % 4 == 0
    res = {"engine": na.version(), "mtu": MTU, "slot": SLOT, "rounds": a.rounds, "scale": a.scale,
           "note": "T = ip_tx_tso_dev, Xl4 = ip_tx_frame_l4_dev on the same datagrams (IP fragments), B = device gather of "
                   "the expanded datagrams + index_put_ of their fields + ip_tx_frame_l4_dev (index and field arrays "
                   "prepared outside the timed window); the plans run once, outside; HIP events, versions alternated; "
                   "GB_s = (R + W) / time"}

    def workload(name, D_np, seed):
        n = len(D_np)
        ln = torch.from_numpy(D_np.view(np.int32)).to(dev)
        stride = (D_np.astype(np.int64) + 3) & ~3                   # datagrams at multiples of 4: B gathers dwords
        off_np = np.zeros(n, dtype=np.int64)
        off_np[1:] = np.cumsum(stride[:-1])
        R = int(off_np[-1] + stride[-1]) + 4
        off = torch.from_numpy(off_np).to(dev)
        arena = torch.empty(R, dtype=torch.uint8, device=dev)
        na.fill_splitmix_dev(arena, R, seed, 0)
        l64 = ln.to(torch.int64)
        full = lambda v: torch.full((n,), v, dtype=torch.uint8, device=dev)
        for col, src in ((0, full(0x45)), (2, (l64 >> 8).to(torch.uint8)), (3, (l64 & 255).to(torch.uint8)), (6, full(0)),
                         (7, full(0)), (9, full(6)), (20 + 12, full(0x50)), (20 + 13, full(tm.ACK | tm.PSH))):
            arena.index_put_((off + col,), src)
        del l64
        l2 = torch.empty(n * 12, dtype=torch.uint8, device=dev)
        na.fill_splitmix_dev(l2, n * 12, seed + 1, 0)
        first = torch.zeros(n + 1, dtype=torch.int64, device=dev)      # T's plan
        status = torch.zeros(n, dtype=torch.int32, device=dev)
        na.tx_tso_plan_dev(arena, R, off, ln, None, n, MTU, first, FLAGS, status)
        first_x = torch.zeros(n + 1, dtype=torch.int64, device=dev)    # Xl4's plan
        na.tx_frame_plan_dev(arena, R, off, ln, n, MTU, first_x, FLAGS)
        torch.cuda.synchronize()
        slots, slots_x = int(first[-1].item()), int(first_x[-1].item())
        first_np = first.cpu().numpy()
        cnt = np.diff(first_np)
        P = D_np.astype(np.int64) - HB
        assert (cnt == np.maximum(1, -(-P // M))).all()
        out = torch.zeros(slots * SLOT, dtype=torch.uint8, device=dev)        # T's
        out_b = torch.zeros(slots * SLOT, dtype=torch.uint8, device=dev)      # B's
        out_x = torch.zeros(slots_x * SLOT, dtype=torch.uint8, device=dev)    # Xl4's
        flen = torch.zeros(slots, dtype=torch.int32, device=dev)
        flen_x = torch.zeros(max(slots, slots_x), dtype=torch.int32, device=dev)
        fcs = torch.zeros(max(slots, slots_x), dtype=torch.int32, device=dev)
        st2 = torch.zeros(max(n, slots), dtype=torch.int32, device=dev)
        # ---- B's arrays, on the host: expanded datagram e = segment s of datagram i ----
        owner = np.repeat(np.arange(n), cnt)
        s_of = np.arange(slots) - first_np[owner]
        plen = np.minimum(M, P[owner] - s_of * M)
        plen = np.where(cnt[owner] == 1, P[owner], plen)
        elen = (HB + plen).astype(np.int64)
        eoff = np.zeros(slots, dtype=np.int64)
        eoff[1:] = np.cumsum((elen[:-1] + 3) & ~3)
        R2 = int(eoff[-1] + ((elen[-1] + 3) & ~3))
        edw = ((elen + 3) >> 2)                                             # dwords of every expanded datagram
        e_of_dw = np.repeat(np.arange(slots), edw)
        x = np.arange(int(edw.sum()), dtype=np.int64) - np.repeat(eoff >> 2, edw)   # dword within its datagram
        src_dw = (off_np[owner][e_of_dw] >> 2) + x + np.where(x >= HB // 4, (s_of * M >> 2)[e_of_dw], 0)
        assert src_dw.max() < (R >> 2) and src_dw.max() < 2**31
        gidx = torch.from_numpy(src_dw.astype(np.int32)).to(dev)
        del e_of_dw, x, src_dw
        # the fields of the segments of datagrams that are cut (ip_len, ip_id, tcp_seqno, flags), as bytes
        hdr = arena[(off[:, None] + torch.arange(HB, device=dev)[None, :])].cpu().numpy()
        cut = cnt[owner] > 1
        ec, oc, sc = np.flatnonzero(cut), owner[cut], s_of[cut]
        id0 = (hdr[oc, 4].astype(np.int64) << 8) | hdr[oc, 5]
        seq0 = (hdr[oc, 24].astype(np.int64) << 24) | (hdr[oc, 25].astype(np.int64) << 16) | (hdr[oc, 26].astype(np.int64) << 8) | hdr[oc, 27]
        idv, seqv, lenv = (id0 + sc) & 0xFFFF, (seq0 + sc * M) & 0xFFFFFFFF, elen[cut]
        fl0 = hdr[oc, 33].astype(np.int64)
        flv = np.where(sc + 1 < cnt[oc], fl0 & (0xFF ^ (tm.FIN | tm.PSH)), fl0)
        flv = np.where(sc > 0, flv & (0xFF ^ tm.CWR), flv)
        cols = ((2, lenv >> 8), (3, lenv), (4, idv >> 8), (5, idv), (24, seqv >> 24), (25, seqv >> 16), (26, seqv >> 8),
                (27, seqv), (33, flv))
        fidx = torch.from_numpy(np.concatenate([eoff[ec] + c for c, _ in cols])).to(dev)
        fval = torch.from_numpy(np.concatenate([(v & 0xFF).astype(np.uint8) for _, v in cols])).to(dev)
        exp = torch.zeros(R2, dtype=torch.uint8, device=dev)
        e_off, e_ln = torch.from_numpy(eoff).to(dev), torch.from_numpy(elen.astype(np.int32)).to(dev)
        e_first = torch.arange(slots + 1, dtype=torch.int64, device=dev)
        e_l2 = l2.view(n, 12)[torch.from_numpy(owner).to(dev)].contiguous().view(-1)
        arena32, exp32 = arena[:R & ~3].view(torch.int32), exp.view(torch.int32)
        pristine = arena.clone()

        def T():
            na.tx_tso_dev(arena, R, off, ln, l2, None, n, MTU, first, out, SLOT, slots, FLAGS, flen, status, fcs, stream=cur())

        def Xl4():
            na.tx_frame_l4_dev(arena, R, off, ln, l2, n, MTU, first_x, out_x, SLOT, slots_x, FLAGS, flen_x, st2, fcs,
                               stream=cur())

        def B():
            torch.index_select(arena32, 0, gidx, out=exp32)
            exp.index_put_((fidx,), fval)
            na.tx_frame_l4_dev(exp, R2, e_off, e_ln, e_l2, slots, MTU, e_first, out_b, SLOT, slots, FLAGS, flen_x, st2, fcs,
                               stream=cur())

        def gather():   # B's first two steps alone: where B's time goes
            torch.index_select(arena32, 0, gidx, out=exp32)
            exp.index_put_((fidx,), fval)

        vers = {"T": T, "Xl4": Xl4, "B": B, "B_gather_only": gather}
        T()
        torch.cuda.synchronize()
        W = int(flen.to(torch.int64).sum().item()) + 4 * slots
        ms = alternate(vers, a.rounds, torch)
        r = {k: stats(v, R + W) for k, v in ms.items()}
        for k in ("Xl4", "B"):
            r["T_over_" + k] = r["T"]["ms_median"] / r[k]["ms_median"]
            r["T_over_%s_q1q3" % k] = [r["T"]["ms_q1"] / r[k]["ms_q3"], r["T"]["ms_q3"] / r[k]["ms_q1"]]
        r.update({"datagrams": n, "frames": slots, "frames_Xl4": slots_x, "read_bytes": R, "written_bytes": W,
                  "expanded_bytes": R2})
        # ---- the same bytes both ways; the datagram arena is not written by T ----
        T()
        torch.cuda.synchronize()
        r["arena_written_by_T"] = int(not torch.equal(arena, pristine))
        B()
        torch.cuda.synchronize()
        r["out_differs_from_B"] = int(not torch.equal(out, out_b))
        st_np = status.cpu().numpy().view(np.uint32)
        seg = na.TSO_SEGMENTED | na.TXD_L4_CSUM_SET | (6 << na.TXD_PROTO_SHIFT)
        whole = na.TXF_WHOLE | na.TXD_L4_CSUM_SET | (6 << na.TXD_PROTO_SHIFT)
        r["status_unexpected"] = int((st_np != np.where(cnt > 1, seg, whole)).sum())
        # ---- all frames of 32 seeded datagrams against the model ----
        bad = frames_checked = 0
        for i in np.random.default_rng(seed + 2).integers(0, n, 32):
            i = int(i)
            o, D = int(off_np[i]), int(D_np[i])
            dg = arena[o:o + D].cpu().numpy().tobytes()
            mac = l2[12 * i:12 * i + 12].cpu().numpy().tobytes()
            st, fr, crcs = tm.frames(fcs_oracle, inet_oracle, dg, mac, MTU, FLAGS, 0)
            k0 = int(first_np[i])
            ok = st == int(st_np[i]) and int(first_np[i + 1]) - k0 == len(fr)
            for q, body in enumerate(fr):
                got = out[(k0 + q) * SLOT:(k0 + q) * SLOT + len(body)].cpu().numpy().tobytes()
                ok = ok and got == body and int(flen[k0 + q].item()) == len(body) - 4
                frames_checked += 1
            bad += int(not ok)
        r["spot_datagrams"], r["spot_frames"], r["spot_bad"] = 32, frames_checked, bad
        r["last_launch"] = na.tso_last_launch()
        res[name] = r
        print(name, json.dumps(r), flush=True)

    s = a.scale
    if "tcp65535" not in a.skip:
        workload("tcp65535", np.full(int(100_000 * s), 65535, dtype=np.uint32), 61)
        torch.cuda.empty_cache()
    if "tcp8220" not in a.skip:
        workload("tcp8220", np.full(int(400_000 * s), 8220, dtype=np.uint32), 71)
        torch.cuda.empty_cache()
    if "mix" not in a.skip:
        n = int(1_000_000 * s)
        counts = [int(n * w) for _, w in MIX]
        counts[0] += n - sum(counts)
        D = np.repeat(np.array([d for d, _ in MIX], dtype=np.uint32), counts)
        np.random.default_rng(7).shuffle(D)
        workload("mix", D, 81)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1), flush=True)


if __name__ == "__main__":
    main()
