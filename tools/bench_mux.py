#!/usr/bin/env python3
"""Device-resident cost of one-pass TX multiplexing (include/nstack_mux.h), in one process, the
versions alternated:

  X    ip_tx_mux_plan_dev + ip_tx_mux_dev          (the plan and the build)
  P    ip_tx_mux_plan_dev                          (the plan alone)
  A    one device-to-device copy of the counts[1] bytes X writes (the datagrams with their pad)   (the floor)
A is the only comparable thing that exists: today's way to the same arrays is host code, record by
record, over data that would first have to leave the device. It is not measured here.
Records lie at 16-byte starts in a device q, socket-major, record k in socket floor(k * S / n), its
destination one of 4096 neighbours behind 64 /26 routes (the lookup takes step 2):
  udp1400_s1 / _s256 / _s65536   UDP records with 1400 payload bytes from 1, 256 and 65536 sockets
  mix_s256                       the 60 / 572 / 1500 / 8220 / 65535 datagram mix as UDP from 256 sockets, clipped to UDP's bound
  tcp32k_s16                     32 KiB TCP records from 16 sockets
One HIP-event pair per version, `--rounds` rounds of the versions in turn after a warm-up round; median
and quartiles; X / A and P / X with quartile ratios. After the timed rounds every record must read
MUX_PLANNED | MUX_BUILT, counts must read {n, bytes, 0, 0}, and one datagram is compared with its image
and its record's payload. Writes one JSON document (--out) and prints it.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

MIX = ((60, 0.40), (572, 0.25), (1500, 0.20), (8220, 0.14), (65535, 0.01))
NROUTES, NNEIGH = 64, 4096


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0, help="scales the batch sizes")
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--skip", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mux_bench.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import nstack_amd as na
    from bench_rxv import alternate, stats
    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    cur = torch.cuda.current_stream
    ALIGN = 16
    res = {"engine": na.version(), "align": ALIGN, "rounds": a.rounds, "scale": a.scale, "routes": NROUTES, "neighbours": NNEIGH,
           "note": "X = ip_tx_mux_plan_dev + ip_tx_mux_dev, P = the plan alone, A = one d2d copy of the counts[1] bytes X writes; "
                   "HIP events, versions alternated; GB_s = 2 * counts[1] / time; the host path this replaces is not measured"}
    rt = np.zeros(NROUTES, na.MUX_ROUTE_DTYPE)
    rt["network"] = 0x0A000000 + 64 * np.arange(NROUTES)
    rt["netmask"] = 0xFFFFFFC0
    rt["iface"] = rt["network"] + 1
    rt["mac"][:, 0] = 2
    rt["mac"][:, 5] = np.arange(NROUTES)
    nb = np.zeros(NNEIGH, na.MUX_NEIGH_DTYPE)
    nb["addr"] = 0x0A000000 + np.arange(NNEIGH)
    nb["mac"][:, 0] = 2
    nb["mac"][:, 4] = np.arange(NNEIGH) >> 8
    nb["mac"][:, 5] = np.arange(NNEIGH) & 255
    nb["valid"] = 1
    d_rt = torch.from_numpy(rt.view(np.uint8)).to(dev)
    d_nb = torch.from_numpy(nb.view(np.uint8)).to(dev)

    def workload(name, P_np, S, proto, seed):
        n, hl = len(P_np), 28 if proto == 17 else 40
        p64 = torch.from_numpy(P_np.astype(np.int64)).to(dev)
        stride = (p64 + 24 + 15) & ~15
        rec = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        rec[1:] = torch.cumsum(stride, 0)
        Q = int(rec[-1].item())
        q = torch.empty(Q + 16, dtype=torch.uint8, device=dev)
        na.fill_splitmix_dev(q, Q, seed, 0)
        idx = torch.arange(n, dtype=torch.int64, device=dev)
        dst = 0x0A000000 + (idx * 2654435761) % NNEIGH
        dport = 1024 + (idx & 16383)
        byte = lambda v, s: ((v >> s) & 255).to(torch.uint8)
        const = lambda v: torch.full((n,), v, dtype=torch.uint8, device=dev)
        cols = [(8 + i, byte(dst, 8 * i)) for i in range(4)] + [(12 + i, byte(dport, 8 * i)) for i in range(4)]
        cols += [(16 + i, byte(p64, 8 * i)) for i in range(4)] + [(20 + i, const(0)) for i in range(4)]
        for col, src in cols:
            q.index_put_((rec[:n] + col,), src)
        sfirst = torch.from_numpy((np.arange(S + 1, dtype=np.int64) * n + S - 1) // S).to(dev)   # socket s: the k with k * S // n == s
        bind = np.array([na.dmx_key(proto, 1024 + (s & 16383), 0x0A000001 + 64 * (s >> 14)) for s in range(S)], dtype=np.uint64)
        d_bind = torch.from_numpy(bind.view(np.int64)).to(dev)
        tcb = np.zeros(S, na.MUX_TCB_DTYPE)
        tcb["seq"], tcb["ack"], tcb["win"], tcb["flags"] = 1000, 2000, 502, 0x18
        d_tcb = torch.from_numpy(tcb.view(np.uint8)).to(dev)
        i32 = lambda k: torch.zeros(k, dtype=torch.int32, device=dev)
        i64 = lambda k: torch.zeros(k, dtype=torch.int64, device=dev)
        t = dict(mstat=i32(n), off=i64(n), len=i32(n), l2=torch.zeros(12 * n, dtype=torch.uint8, device=dev),
                 himg=torch.zeros(40 * n, dtype=torch.uint8, device=dev), tnext=i32(S), counts=i64(4), fin=i32(n))

        def plan():
            na.tx_mux_plan_dev(q, Q, rec, n, sfirst, d_bind, S, d_tcb, d_rt, NROUTES, d_nb, NNEIGH, t["mstat"], t["off"], t["len"], t["l2"],
                               t["himg"], t["tnext"], t["counts"], 7, ALIGN, cur())

        plan()
        torch.cuda.synchronize()
        cn = [int(x) for x in t["counts"].cpu().numpy()]
        W = cn[1]
        dg = torch.zeros(W + 128, dtype=torch.uint8, device=dev)

        def X():
            plan()
            na.tx_mux_dev(q, Q, rec, n, t["mstat"], t["off"], t["len"], t["himg"], dg, W, ALIGN, t["fin"], cur())

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
        # one datagram, read back: the last record's
        k0 = n - 1
        o0, l0, r0, P0 = int(t["off"][k0].item()), int(t["len"][k0].item()), int(rec[k0].item()), int(P_np[k0])
        hdr_same = bool(torch.equal(dg[o0:o0 + hl], t["himg"][40 * k0:40 * k0 + hl]))
        pay_same = bool(torch.equal(dg[o0 + hl:o0 + l0], q[r0 + 24:r0 + 24 + P0]))
        o.update({"records": n, "sockets": S, "payload_bytes": int(P_np.astype(np.int64).sum()), "datagram_bytes": W, "counts": cn,
                  "not_built": int((fin != (na.MUX_PLANNED | na.MUX_BUILT)).sum()), "last_datagram_len": l0,
                  "last_datagram_equal": hdr_same and pay_same and l0 == hl + P0, "last_launch": na.mux_last_launch()})
        assert cn == [n, W, 0, 0] and o["not_built"] == 0 and o["last_datagram_equal"], o
        res[name] = o
        print(name, json.dumps(o), flush=True)
        del q, dg, ca, cb
        torch.cuda.empty_cache()

    s = a.scale
    for S in (1, 256, 65536):
        if f"udp1400_s{S}" not in a.skip.split(","):
            workload(f"udp1400_s{S}", np.full(int(625_000 * s), 1400, dtype=np.uint32), S, 17, 81 + S)
    if "mix_s256" not in a.skip.split(","):
        n = int(250_000 * s)
        cnt = [int(n * w) for _, w in MIX]
        cnt[0] += n - sum(cnt)
        D = np.repeat(np.array([d for d, _ in MIX], dtype=np.uint32), cnt)
        np.random.default_rng(7).shuffle(D)
        workload("mix_s256", np.minimum(D - 28, na.MUX_UDP_MAX).astype(np.uint32), 256, 17, 91)
    if "tcp32k_s16" not in a.skip.split(","):
        workload("tcp32k_s16", np.full(int(25_000 * s), 32768 - 40, dtype=np.uint32), 16, 6, 95)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1), flush=True)


if __name__ == "__main__":
    main()
