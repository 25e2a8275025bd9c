"""Batches for the TX-multiplexing tests (include/nstack_mux.h): per-socket send queues laid out in a q
arena, the tables, the model's result (tests/mux_model.py), and the calls that run a batch through
the C ABI and compare everything: plan arrays, counts, tnext, the whole canaried dgram and the final
words. BATCHES is the list tests/test_gpu_mux.py runs on the device and tests/test_mux_model.py holds
the host plan to. Test infrastructure only."""
import numpy as np

import mux_model as mm
import nstack_amd as na

UNSET = 0xCCCCCCCC
CANARY = 0xC3
NET1, NET2 = 0x0A000000, 0xC0A80100      # 10.0.0.0/24 and 192.168.1.0/24
IF1, IF2, IF0 = 0x0A000001, 0xC0A80101, 0xAC100001
MAC = lambda x: bytes([0x02, 0x00, (x >> 24) & 255, (x >> 16) & 255, (x >> 8) & 255, x & 255])
ROUTES = [mm.route(NET1, 0xFFFFFF00, IF1, MAC(IF1)), mm.route(NET2, 0xFFFFFF00, IF2, MAC(IF2)), mm.route(0, 0, IF0, MAC(IF0))]


def to_dev(arr, dev):
    import torch
    arr = np.ascontiguousarray(arr)
    if arr.dtype.fields is not None:
        arr = arr.view(np.uint8)
    return torch.from_numpy(arr if arr.flags.writeable else arr.copy()).to(dev)


def payload(rng, n):
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes()


def neigh(addrs):
    return [(a, MAC(a), 1) for a in addrs]


class MuxBatch:
    """socks: [(key, tcb or None, [record bytes, ...])]; a tcb is (seq, ack, win, flags). The records are
    laid out from byte `lead` on, each on the next multiple of 8 (or at `starts`). tcb=False: the call
    gets no tcb array. q_bytes / dgram_bytes None: the arena's size / what the plan asks for."""

    def __init__(self, socks, rt, nb, align=16, id0=0, tcb=True, lead=0, starts=None, q_bytes=None, rec_override=None,
                 dgram_bytes=None):
        recs = [r for _, _, rs in socks for r in rs]
        self.n, self.S = len(recs), len(socks)
        if starts is None:
            starts, at = [], lead
            for r in recs:
                at = (at + 7) & ~7
                starts.append(at)
                at += len(r)
        end = max([s + len(r) for s, r in zip(starts, recs)] + [lead])
        self.q = np.full(max(end, 8), 0xEE, np.uint8)
        for s, r in zip(starts, recs):
            self.q[s:s + len(r)] = np.frombuffer(r, np.uint8)
        self.q_bytes = end if q_bytes is None else q_bytes
        self.rec = np.zeros(max(self.n, 1), np.uint64)
        self.rec[:self.n] = starts
        for k, v in (rec_override or {}).items():
            self.rec[k] = v
        self.sfirst = np.zeros(self.S + 1, np.uint64)
        self.sfirst[1:] = np.cumsum([len(rs) for _, _, rs in socks], dtype=np.uint64)
        self.bind = np.array([k for k, _, _ in socks] + [0], np.uint64)[:max(self.S, 1)]
        self.tcb = [t if t is not None else ((1000 * s) & 0xFFFFFFFF, 77 + s, 502, mm.PSH_ACK) for s, (_, t, _) in enumerate(socks)] if tcb else None
        self.rt, self.nb, self.align, self.id0 = rt, nb, align, id0
        self.R, self.N = len(rt), len(nb)
        self.tcb_np = None
        if self.tcb is not None:
            self.tcb_np = np.zeros(max(self.S, 1), na.MUX_TCB_DTYPE)
            for s, t in enumerate(self.tcb):
                self.tcb_np[s] = (t[0], t[1], t[2], t[3], 0)
        self.rt_np = np.zeros(max(self.R, 1), na.MUX_ROUTE_DTYPE)
        for i, r in enumerate(rt):
            self.rt_np[i] = (r["network"], r["netmask"], r["gw"], r["iface"], list(r["mac"]), 0)
        self.nb_np = np.zeros(max(self.N, 1), na.MUX_NEIGH_DTYPE)
        if self.N:
            self.nb_np["addr"][:self.N] = [a for a, _, _ in nb]
            self.nb_np["mac"][:self.N] = np.frombuffer(b"".join(bytes(m) for _, m, _ in nb), np.uint8).reshape(self.N, 6)
            self.nb_np["valid"][:self.N] = [v for _, _, v in nb]
        self.plan = mm.plan(self.q, self.q_bytes, self.rec[:self.n], self.sfirst, self.bind[:self.S], self.tcb, rt, nb, id0, align)
        self.need = int(self.plan["counts"][1])
        self.dgram_bytes = self.need if dgram_bytes is None else dgram_bytes
        self.dgram = np.full(max(self.need, self.dgram_bytes) + 256, CANARY, np.uint8)   # dgram itself starts 128 bytes in
        self.fin = mm.build(self.plan, self.dgram[128:], self.dgram_bytes)

    def _tables(self):
        return (self.sfirst, self.bind if self.S else None, self.S, self.tcb_np, self.rt_np if self.R else None, self.R,
                self.nb_np if self.N else None, self.N)

    def _outputs(self, extra=0):
        n, S = self.n + extra, self.S + extra
        return dict(mstat=np.full(max(n, 1), UNSET, np.uint32), off=np.full(max(n, 1), UNSET, np.uint64), len=np.full(max(n, 1), UNSET, np.uint32),
                    l2=np.full(max(n, 1) * 12, 0xCC, np.uint8), himg=np.full(max(n, 1) * 40, 0xCC, np.uint8),
                    tnext=np.full(max(S, 1), UNSET, np.uint32), counts=np.full(4 + extra, UNSET, np.uint64))

    def _check_plan(self, r, what):
        n, S, p = self.n, self.S, self.plan
        assert np.array_equal(r["mstat"][:n], p["mstat"]), (what, "mstat")
        assert np.array_equal(r["off"][:n], p["off"]), (what, "off")
        assert np.array_equal(r["len"][:n], p["len"]), (what, "len")
        assert np.array_equal(r["l2"][:n * 12].reshape(n, 12), p["l2"]), (what, "l2")
        assert np.array_equal(r["himg"][:n * 40].reshape(n, 40), p["himg"]), (what, "himg")
        assert np.array_equal(r["tnext"][:S], p["tnext"]), (what, "tnext")
        assert np.array_equal(r["counts"][:4], p["counts"]), (what, r["counts"], p["counts"])

    # ---- the host plan ----
    def check_plan_host(self):
        r = self._outputs()
        got = na.tx_mux_plan_host(self.q, self.q_bytes, self.rec, self.n, *self._tables(), r["mstat"], r["off"], r["len"], r["l2"], r["himg"],
                                  r["tnext"], r["counts"], self.id0, self.align)
        assert got == int(self.plan["counts"][0])
        self._check_plan(r, "host plan")

    # ---- the device forms ----
    def run_dev(self, dev, build=True, pstat_inplace=False, stream=None, corrupt=None):
        """corrupt(t): changes the plan's device arrays between the plan and the build."""
        import torch
        n = self.n
        sfirst, bind, S, tcb, rt, R, nb, N = self._tables()
        t = dict(q=to_dev(np.concatenate([self.q, np.zeros(8, np.uint8)]), dev), rec=to_dev(self.rec, dev), sfirst=to_dev(sfirst, dev))
        up = lambda a: None if a is None else to_dev(a, dev)
        t.update({k: to_dev(v, dev) for k, v in self._outputs(extra=1).items()})
        t["fin"] = to_dev(np.full(n + 1, UNSET, np.uint32), dev)
        na.tx_mux_plan_dev(t["q"], self.q_bytes, t["rec"], n, t["sfirst"], up(bind), S, up(tcb), up(rt), R, up(nb), N, t["mstat"], t["off"],
                           t["len"], t["l2"], t["himg"], t["tnext"], t["counts"], self.id0, self.align, stream)
        t["dgram"] = to_dev(np.full(self.dgram.size, CANARY, np.uint8), dev)
        assert t["dgram"].data_ptr() % 128 == 0
        if corrupt is not None:
            torch.cuda.synchronize()
            corrupt(t)
        if build:
            fin = t["mstat"] if pstat_inplace else t["fin"]
            na.tx_mux_dev(t["q"], self.q_bytes, t["rec"], n, t["mstat"], t["off"], t["len"], t["himg"], t["dgram"].data_ptr() + 128,
                          self.dgram_bytes, self.align, fin, stream)
        torch.cuda.synchronize()
        r = {k: v.cpu().numpy() for k, v in t.items()}
        r["dev"] = t
        if pstat_inplace:
            r["fin"] = r["mstat"]
        return r

    def check_dev(self, r, build=True):
        n, S = self.n, self.S
        self._check_plan(r, "device plan")
        # nothing behind the arrays' ends
        for k, e in dict(mstat=n, off=n, len=n, tnext=S, counts=4).items():
            assert (r[k][e:] == r[k].dtype.type(UNSET)).all(), k
        assert (r["l2"][n * 12:] == 0xCC).all() and (r["himg"][n * 40:] == 0xCC).all()
        if build:
            assert np.array_equal(r["fin"][:n], self.fin), "final words"
            assert r["fin"][n] == UNSET
            assert np.array_equal(r["dgram"], self.dgram), "dgram"       # canaries around and between the datagrams included
        else:
            assert (r["dgram"] == CANARY).all()

    # ---- the host form ----
    def run_host(self):
        r = self._outputs()
        r["dgram"] = np.full(self.dgram.size, CANARY, np.uint8)
        r["planned"] = na.tx_mux_host(self.q, self.q_bytes, self.rec, self.n, *self._tables(), r["dgram"][128:], self.dgram_bytes, self.id0,
                                      self.align, r["mstat"], r["off"], r["len"], r["l2"], r["himg"], r["tnext"], r["counts"])
        return r

    def check_host(self, r):
        assert r["planned"] == int(self.plan["counts"][0])
        p, self.plan = self.plan, dict(self.plan, mstat=self.fin)
        try:
            self._check_plan(r, "host form")
        finally:
            self.plan = p
        assert np.array_equal(r["dgram"], self.dgram)


# ---------------------------------------------------------------------------------------------
# The batches.
# ---------------------------------------------------------------------------------------------
HOSTS = [NET1 + 2 + i for i in range(20)] + [NET2 + 2 + i for i in range(20)] + [0x08080800 + i for i in range(8)]


def keys(S):
    """S socket keys, UDP and TCP alternating."""
    return [mm.key((17, 6)[s & 1], 2000 + (s >> 1), (IF1, IF2)[(s >> 1) & 1]) for s in range(S)]


def mixed(n, S, seed=5, align=16, sizes=(1, 60), id0=0x1234, **kw):
    """n records spread over S sockets (contiguous per socket, some sockets empty) to HOSTS, of which the
    last two have no neighbour."""
    rng = np.random.default_rng(seed)
    own = np.sort(rng.integers(0, S, n)) if S else []
    socks = [(k, None, []) for k in keys(S)]
    for s in own:
        socks[s][2].append(mm.record(HOSTS[int(rng.integers(0, len(HOSTS)))], int(rng.integers(1, 65536)),
                                     payload(rng, int(rng.integers(sizes[0], sizes[1] + 1)))))
    return MuxBatch(socks, ROUTES, neigh(HOSTS[:-2]), align, id0, **kw)


COPY_SIZES = tuple(range(1, 65)) + (1023, 1024, 1025, 4095, 4096, 4097)


def copy(proto, align):
    """Every payload size of COPY_SIZES and the protocol's bounds from one socket: with the record starts
    on multiples of 8 and datagram starts on multiples of align, off + hl reaches every phase of 4."""
    rng = np.random.default_rng(100 * proto + align)
    sizes = COPY_SIZES + ((65506,) if proto == 17 else (0, 65495))
    recs = [mm.record(HOSTS[i % 40], 7 + i, payload(rng, P)) for i, P in enumerate(sizes)]
    b = MuxBatch([(mm.key(proto, 4000, IF1), (0xFFFF0000, 9, 502, mm.PSH_ACK), recs)], ROUTES, neigh(HOSTS), align)
    assert int(b.rec[b.n - 1]) + len(recs[-1]) == b.q_bytes               # the last record ends exactly at q_bytes
    return b


def tables_routes(R):
    """R routes: R = 2 is an exact match behind a mask match of a lower index; R = 256 has the matching
    routes at the far end."""
    rng = np.random.default_rng(R)
    x = NET1 + 9
    if R == 0:
        rt = []
    elif R == 1:
        rt = [mm.route(0, 0, IF0, MAC(IF0))]                              # the default route, found in step 2
    elif R == 2:
        rt = [mm.route(NET1, 0xFFFFFF00, IF1, MAC(IF1)), mm.route(x, 0xFFFFFFFF, IF2, MAC(IF2))]
    else:
        rt = [mm.route(0x64000000 + (i << 8), 0xFFFFFF00, 0x64000001 + (i << 8), MAC(i)) for i in range(R - 3)]
        rt += [mm.route(NET1, 0xFFFFFF00, IF1, MAC(IF1)), mm.route(NET1, 0xFFFF0000, IF2, MAC(IF2)),
               mm.route(0, 0xFF000000, IF0, MAC(IF0))]                    # two mask matches; a default found in step 3 only
    dsts = [x, NET1 + 3, NET2 + 5, 0x64000507, 0x08080808]
    recs = [mm.record(d, 53, payload(rng, 9 + i)) for i, d in enumerate(dsts)]
    return MuxBatch([(mm.key(17, 1, IF1), None, recs), (mm.key(6, 2, IF1), None, recs[::-1])], rt, neigh(dsts), 8)


def tables_neigh(N):
    """N neighbours with duplicate, invalid and missing entries."""
    rng = np.random.default_rng(N)
    nb = [(NET1 + 2 + (i % 60000) + ((i // 60000) << 16), MAC(i), 1) for i in range(N)]
    if N >= 2:
        nb[1] = (nb[0][0], MAC(0xABCDEF), 1)                              # a duplicate: the lowest index wins
    if N >= 255:
        nb[7] = (nb[7][0], nb[7][1], 0)                                   # invalid: matches nothing
        nb[N - 1] = (nb[3][0], MAC(0x123456), 1)                          # a duplicate at the far end
        nb[2] = (nb[N - 2][0], MAC(0x654321), 1)                          # and one whose lowest index lies in front
    dsts = [nb[i][0] for i in (0, 1, 2, 3, 7, N // 2, N - 2, N - 1) if 0 <= i < N] + [NET1 + 0x00F00000, 0]
    recs = [mm.record(d, 9, payload(rng, 5 + i)) for i, d in enumerate(dsts)]
    rt = [mm.route(0x0A000000, 0xFF000000, IF1, MAC(IF1)), mm.route(0, 0, IF0, MAC(IF0))]
    return MuxBatch([(mm.key(17, 1, IF1), None, recs)], rt, nb, 16)


def tables_socks(S):
    """S sockets with empty ones in front, between and behind."""
    rng = np.random.default_rng(S)
    socks = [(k, None, []) for k in keys(S)]
    for s in sorted({1, 2, S // 2, S - 2} & set(range(S))) if S > 2 else range(S):
        for i in range(1 + s % 3):
            socks[s][2].append(mm.record(HOSTS[(s + i) % 40], 80, payload(rng, 1 + (s + i) % 50)))
    return MuxBatch(socks, ROUTES, neigh(HOSTS), 16)


NO_DATAGRAM = ("plain", "misaligned", "hdr-outside", "size-outside", "huge-size", "port-neg", "port-big", "bad-key", "udp-0", "udp-65507",
               "tcp-65496", "no-route", "no-neigh", "neigh-invalid", "tcp-0")


def no_datagram(align=16, tcb=True, big=True):
    """Every way to make no datagram, in one batch, between records that make one. big=False leaves out
    the three records at the 64 KiB bounds (the golden file stays small)."""
    rng = np.random.default_rng(11)
    ok = lambda P=30, dst=HOSTS[0], dport=53: mm.record(dst, dport, payload(rng, P))
    rt = ROUTES[:2]                                                       # no default route
    nb = neigh(HOSTS[:20]) + [(HOSTS[20], MAC(1), 0)]
    udp = [("plain", ok()), ("misaligned", ok()), ("huge-size", mm.record(HOSTS[0], 53, b"", size=1 << 63)),
           ("port-neg", ok(dport=-1)), ("port-big", ok(dport=65536)), ("plain", ok(dport=65535)), ("plain", ok(dport=0)),
           ("udp-0", ok(0)), ("udp-65507", ok(65507)), ("no-route", ok(dst=0x08080808)), ("no-neigh", ok(dst=HOSTS[21])),
           ("neigh-invalid", ok(dst=HOSTS[20])), ("plain", ok(1))]
    tcp = [("plain", ok(5)), ("tcp-0", ok(0)), ("tcp-65496", ok(65496)), ("no-route", ok(dst=0x7F000001)), ("plain", ok(65495))]
    if not big:
        udp, tcp = [c for c in udp if len(c[1]) < 60000], [c for c in tcp if len(c[1]) < 60000]
    bad = [("bad-key", ok()), ("bad-key", ok(0))]
    tail = [("plain", ok(3)), ("hdr-outside", ok(0)), ("size-outside", mm.record(HOSTS[0], 53, payload(rng, 10), size=11))]
    socks = [(mm.key(17, 1, IF1), None, [c[1] for c in udp]), (mm.key(6, 2, IF1), (0xFFFFFF00, 5, 502, 0x18), [c[1] for c in tcp]),
             (mm.key(1, 3, IF1), None, [c[1] for c in bad]), (mm.key(17, 4, IF2), None, [c[1] for c in tail])]
    cases = udp + tcp + bad + tail
    assert {c[0] for c in cases} == set(NO_DATAGRAM) - (set() if big else {"udp-65507", "tcp-65496"})
    b0 = MuxBatch(socks, rt, nb, align, tcb=tcb)
    k_mis, k_hdr = 1, len(cases) - 2
    over = {k_mis: int(b0.rec[k_mis]) + 4, k_hdr: (b0.q_bytes - 23 + 7) & ~7}   # the lowest multiple of 8 with r + 24 > q_bytes
    assert int(b0.rec[-1]) + 24 + 10 == b0.q_bytes                        # the last record claims one byte more than q holds
    b = MuxBatch(socks, rt, nb, align, tcb=tcb, rec_override=over, id0=0xFFFE)
    want = {"plain": mm.PLANNED, "tcp-0": mm.PLANNED, "no-route": mm.NO_ROUTE, "no-neigh": mm.NO_NEIGH, "neigh-invalid": mm.NO_NEIGH,
            "udp-0": mm.BAD_SIZE, "udp-65507": mm.BAD_SIZE, "tcp-65496": mm.BAD_SIZE}
    for k, c in enumerate(cases):
        w = want.get(c[0], mm.BAD_REC)
        if not tcb and len(udp) <= k < len(udp) + len(tcp):
            w = mm.NO_TCB | (mm.BAD_SIZE if c[0] == "tcp-65496" else 0)
        assert int(b.plan["mstat"][k]) == w, (c[0], k, int(b.plan["mstat"][k]))
    return b


def wraps():
    """ip_id wrap: id0 = 0xfffe and five datagrams with an unplanned record between them. seq wrap:
    tcb.seq = 0xffffff00 with unplanned records of the same socket in between."""
    rng = np.random.default_rng(12)
    r = lambda P, dst=HOSTS[0]: mm.record(dst, 80, payload(rng, P))
    tcp = [r(300), r(10, 0x08080808), r(200), r(65496), r(0), r(7)]
    udp = [r(9), r(0), r(11)]
    b = MuxBatch([(mm.key(6, 1, IF1), (0xFFFFFF00, 1, 502, 0x18), tcp[:3]), (mm.key(17, 2, IF1), None, udp),
                  (mm.key(6, 3, IF1), (0xFFFFFFFF, 2, 1, 0x10), tcp[3:])], ROUTES[:2], neigh(HOSTS), 4, id0=0xFFFE)
    return b


# name -> a callable that makes the batch (the GPU list; the CPU test holds the host plan to each)
BATCHES = {}
for _n in (0, 1, 7, 8, 9, 31, 32, 33):
    BATCHES[f"rows-{_n}"] = (lambda n=_n: mixed(n, 3, seed=n, align=(4, 16)[n & 1]))
for _n in (255, 256, 257):
    BATCHES[f"blocks-{_n}"] = (lambda n=_n: mixed(n, 40, seed=n, align=8))
BATCHES["blocks-65537"] = lambda: mixed(65537, 300, seed=1, align=4, sizes=(1, 1))
for _al in (4, 8, 16, 128):
    for _pr in (17, 6):
        BATCHES[f"copy-{_pr}-{_al}"] = (lambda pr=_pr, al=_al: copy(pr, al))
for _R in (0, 1, 2, 256):
    BATCHES[f"routes-{_R}"] = (lambda R=_R: tables_routes(R))
for _N in (0, 1, 2, 255, 256, 257, 65536):
    BATCHES[f"neigh-{_N}"] = (lambda N=_N: tables_neigh(N))
for _S in (0, 1, 2, 65536):
    BATCHES[f"socks-{_S}"] = (lambda S=_S: tables_socks(S))
BATCHES["status-all"] = no_datagram
BATCHES["status-all-128"] = lambda: no_datagram(128)
BATCHES["status-no-tcb"] = lambda: no_datagram(8, tcb=False)
BATCHES["wraps"] = wraps
