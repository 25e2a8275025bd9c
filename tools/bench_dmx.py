#!/usr/bin/env python3
"""Device-resident cost of one-pass RX demultiplexing (include/nstack_dmx.h), in one process, the
versions alternated:

  X    ip_rx_demux_plan_dev + ip_rx_demux_dev      (the plan and the build)
  P    ip_rx_demux_plan_dev                         (the plan alone)
  A    one device-to-device copy of the bytes X writes (sbase[S], the records with their pad)   (the floor)
Datagrams lie packed at 16-byte starts in a device arena, as ip_rx_reasm_l4_dev leaves them at align 16;
datagram i goes to socket (i * 2654435761) mod S:
  udp1400_s1 / _s256 / _s65536   UDP datagrams with 1400 payload bytes to 1, 256 and 65536 sockets
  mix_s256                       the 60 / 572 / 1500 / 8220 / 65535 mix as UDP to 256 sockets
  tcp32k_s16                     32 KiB TCP datagrams (what ip_rx_gro_dev leaves of a bulk flow) to 16 sockets
One HIP-event pair per version, `--rounds` rounds of the versions in turn after a warm-up round; median
and quartiles; X / A and P / X with quartile ratios. Every datagram must come out DMX_QUEUED |
DMX_DELIVERED and qcounts must read {n, sbase[S], 0, 0}: both are checked. Writes one JSON document
(--out) and prints it.
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
    ap.add_argument("--scale", type=float, default=1.0, help="scales the batch sizes")
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--skip", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dmx_bench.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import nstack_amd as na
    from bench_rxv import alternate, stats
    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    cur = torch.cuda.current_stream
    ALIGN = 16
    res = {"engine": na.version(), "align": ALIGN, "rounds": a.rounds, "scale": a.scale,
           "note": "X = ip_rx_demux_plan_dev + ip_rx_demux_dev, P = the plan alone, A = one d2d copy of the sbase[S] bytes X writes; "
                   "HIP events, versions alternated; GB_s = 2 * sbase[S] / time"}

    def sock_key(s):
        return na.dmx_key(17, 1024 + (s & 16383), 0x0A000002 + (s >> 14))

    def workload(name, D_np, S, proto, seed):
        n = len(D_np)
        ln = torch.from_numpy(D_np.view(np.int32)).to(dev)
        l64 = ln.to(torch.int64)
        stride = (l64 + 15) & ~15
        off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        off[1:] = torch.cumsum(stride, 0)
        R = int(off[-1].item())
        arena = torch.empty(R + 16, dtype=torch.uint8, device=dev)
        na.fill_splitmix_dev(arena, R, seed, 0)
        idx = torch.arange(n, dtype=torch.int64, device=dev)
        sock = (idx * 2654435761) % S
        port, addr = 1024 + (sock & 16383), 0x0A000002 + (sock >> 14)
        byte = lambda v, s: ((v >> s) & 255).to(torch.uint8)
        const = lambda v: torch.full((n,), v, dtype=torch.uint8, device=dev)
        cols = [(0, const(0x45)), (2, byte(l64, 8)), (3, byte(l64, 0)), (6, const(0)), (7, const(0)), (9, const(proto)),
                (16, byte(addr, 24)), (17, byte(addr, 16)), (18, byte(addr, 8)), (19, byte(addr, 0)),
                (22, byte(port, 8)), (23, byte(port, 0))]
        if proto == 6:
            cols += [(32, const(0x50)), (33, const(0x18))]
        for col, src in cols:
            arena.index_put_((off[:n] + col,), src)
        bind = np.array([sock_key(s) if proto == 17 else na.dmx_key(6, 1024 + (s & 16383), 0x0A000002 + (s >> 14)) for s in range(S)],
                        dtype=np.uint64)
        d_bind = torch.from_numpy(bind.view(np.int64)).to(dev)
        counts = torch.tensor([n, R], dtype=torch.int64, device=dev)
        i32 = lambda k: torch.zeros(k, dtype=torch.int32, device=dev)
        i64 = lambda k: torch.zeros(k, dtype=torch.int64, device=dev)
        t = dict(dstat=i32(n), dsock=i32(n), rec=i64(n), sbase=i64(S + 1), scnt=i32(S), qcounts=i64(4), fin=i32(n))

        def plan():
            na.rx_demux_plan_dev(arena, R, off, ln, counts, n, d_bind, S, t["dstat"], t["dsock"], t["rec"], t["sbase"], t["scnt"],
                                 t["qcounts"], None, 0, ALIGN, cur())

        plan()
        torch.cuda.synchronize()
        qc = [int(x) for x in t["qcounts"].cpu().numpy()]
        W = qc[1]
        q = torch.zeros(W + 128, dtype=torch.uint8, device=dev)

        def X():
            plan()
            na.rx_demux_dev(arena, R, off, ln, counts, n, t["dstat"], t["rec"], q, W, ALIGN, t["fin"], cur())

        ca = torch.empty(W, dtype=torch.uint8, device=dev)
        cb = torch.empty(W, dtype=torch.uint8, device=dev)

        def A():
            cb.copy_(ca)

        ms = alternate({"X": X, "P": plan, "A": A}, a.rounds, torch)
        o = {k: stats(v, 2 * W) for k, v in ms.items()}
        for k, over in (("X", "A"), ("P", "X")):
            o[f"{k}_over_{over}"] = o[k]["ms_median"] / o[over]["ms_median"]
            o[f"{k}_over_{over}_q1q3"] = [o[k]["ms_q1"] / o[over]["ms_q3"], o[k]["ms_q3"] / o[over]["ms_q1"]]
        X()
        torch.cuda.synchronize()
        fin = t["fin"].cpu().numpy().view(np.uint32)
        scnt = t["scnt"].cpu().numpy().view(np.uint32)
        # one record, read back: socket 0's first
        k0 = int(np.flatnonzero(t["dsock"].cpu().numpy() == 0)[0])
        r0 = int(t["rec"][k0].item())
        P0 = int(D_np[k0]) - (28 if proto == 17 else 40)
        head = q[r0:r0 + 24].cpu().numpy()
        same = bool(torch.equal(q[r0 + 24:r0 + 24 + P0], arena[int(off[k0].item()) + int(D_np[k0]) - P0:int(off[k0].item()) + int(D_np[k0])]))
        o.update({"datagrams": n, "sockets": S, "datagram_bytes": int(D_np.astype(np.int64).sum()), "record_bytes": W, "qcounts": qc,
                  "not_delivered": int((fin != (na.DMX_QUEUED | na.DMX_DELIVERED)).sum()), "scnt_min": int(scnt.min()),
                  "scnt_max": int(scnt.max()), "first_record_buf_size": int(head[16:24].view(np.uint64)[0]),
                  "first_record_payload_equal": same and int(head[16:24].view(np.uint64)[0]) == P0, "last_launch": na.dmx_last_launch()})
        assert qc == [n, W, 0, 0] and o["not_delivered"] == 0 and o["first_record_payload_equal"], o
        res[name] = o
        print(name, json.dumps(o), flush=True)
        del arena, q, ca, cb
        torch.cuda.empty_cache()

    s = a.scale
    for S in (1, 256, 65536):
        if f"udp1400_s{S}" not in a.skip.split(","):
            workload(f"udp1400_s{S}", np.full(int(625_000 * s), 1428, dtype=np.uint32), S, 17, 81 + S)
    if "mix_s256" not in a.skip.split(","):
        n = int(250_000 * s)
        cnt = [int(n * w) for _, w in MIX]
        cnt[0] += n - sum(cnt)
        D = np.repeat(np.array([d for d, _ in MIX], dtype=np.uint32), cnt)
        np.random.default_rng(7).shuffle(D)
        workload("mix_s256", D, 256, 17, 91)
    if "tcp32k_s16" not in a.skip.split(","):
        workload("tcp32k_s16", np.full(int(25_000 * s), 32768, dtype=np.uint32), 16, 6, 95)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1), flush=True)


if __name__ == "__main__":
    main()
