"""Batches for the demultiplexing tests (include/nstack_dmx.h): a batch of datagrams laid out in an
`out` arena, a bind table, the model's result (tests/dmx_model.py), and the calls that run it through
the C ABI and compare everything: plan arrays, the whole canaried q, final words and qcounts.
BATCHES is the list tests/test_gpu_dmx.py runs on the device and tests/test_dmx_model.py holds the
host plan to. Test infrastructure only."""
import numpy as np

import dmx_model as dm
import nstack_amd as na
import rxd_model as rd

UNSET = 0xCCCCCCCC
CANARY = 0xC3
A, B = 0x0A000002, 0xC0A80101            # two local addresses
TILE = 1024                              # the partition's tile (dmx_launch.hpp)


def to_dev(arr, dev):
    import torch
    arr = np.ascontiguousarray(arr)
    return torch.from_numpy(arr if arr.flags.writeable else arr.copy()).to(dev)


def payload(rng, n):
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes()


class DmxBatch:
    """dgs: the datagrams, laid out from byte `lead` on with `gap` bytes between them (or at `starts`).
    n: the arrays' capacity (default m). out_bytes / q_bytes None: the arena's size / what the plan
    asks for. dlen_override: {k: dlen[k]} declares another length than the bytes laid out."""

    def __init__(self, dgs, bind, align=8, lead=0, gap=0, starts=None, dverdict=None, drop_mask=0, n=None, out_bytes=None,
                 q_bytes=None, doff_override=None, dlen_override=None):
        self.m = len(dgs)
        self.n = self.m if n is None else n
        if starts is None:
            starts, at = [], lead
            for d in dgs:
                starts.append(at)
                at += len(d) + gap
        end = max([s + len(d) for s, d in zip(starts, dgs)] + [lead])
        self.out = np.full(end + 3, 0xEE, np.uint8)
        for s, d in zip(starts, dgs):
            self.out[s:s + len(d)] = np.frombuffer(d, np.uint8)
        self.out_bytes = end if out_bytes is None else out_bytes
        self.doff = np.zeros(self.n + 1, np.uint64)
        self.dlen = np.zeros(max(self.n, 1), np.uint32)
        self.doff[:self.m] = starts
        self.dlen[:self.m] = [len(d) for d in dgs]
        for k, v in (doff_override or {}).items():
            self.doff[k] = v
        for k, v in (dlen_override or {}).items():
            self.dlen[k] = v
        self.doff[self.m] = end
        self.bind = np.asarray(bind, np.uint64)
        self.S, self.align, self.drop_mask = len(self.bind), align, drop_mask
        self.dverdict = None if dverdict is None else np.asarray(dverdict, np.uint32)
        self.plan = dm.plan(self.out, self.out_bytes, self.doff[:self.m], self.dlen[:self.m], self.bind, align, self.dverdict,
                            drop_mask, self.n)
        self.need = int(self.plan["sbase"][self.S])
        self.q_bytes = self.need if q_bytes is None else q_bytes
        self.q = np.full(max(self.need, self.q_bytes) + 256, CANARY, np.uint8)   # q itself starts 128 bytes in
        self.fin = dm.build(self.plan, self.q[128:], self.q_bytes)

    def host_bind(self):
        """The bind table for the host forms, which refuse an invalid key (the device forms let it match
        nothing): every invalid key gives way to a valid one that no datagram is sent to."""
        b = self.bind.copy()
        for s in range(self.S):
            if not dm.key_valid(int(b[s])):
                b[s] = dm.key(17, 60000 + (s & 1023), 0x01010101 + (s >> 10))
        return b

    # ---- the host plan ----
    def check_plan_host(self):
        n, S = self.m, self.S
        self.bind, device_bind = self.host_bind(), self.bind
        try:
            self._check_plan_host(n, S)
        finally:
            self.bind = device_bind

    def _check_plan_host(self, n, S):
        dstat, dsock = np.full(max(n, 1), UNSET, np.uint32), np.full(max(n, 1), UNSET, np.uint32)
        rec, sbase, scnt = np.full(max(n, 1), UNSET, np.uint64), np.full(S + 1, UNSET, np.uint64), np.full(max(S, 1), UNSET, np.uint32)
        r = na.rx_demux_plan_host(self.out, self.out_bytes, self.doff, self.dlen, n, self.bind if S else None, S, dstat, dsock, rec,
                                  sbase, scnt, self.dverdict, self.drop_mask, self.align)
        p = self.plan
        assert r == int(p["qcounts"][0])
        assert np.array_equal(dstat[:n], p["dstat"][:n]) and np.array_equal(dsock[:n], p["dsock"][:n])
        assert np.array_equal(rec[:n], p["rec"][:n]) and np.array_equal(sbase, p["sbase"]) and np.array_equal(scnt[:S], p["scnt"])

    # ---- the device forms ----
    def run_dev(self, dev, build=True, pstat_inplace=False, stream=None, given=None):
        """given: device tensors out, doff, dlen, counts, dverdict that another call left (the batch was
        made from their contents), used in place of uploads."""
        import torch
        n, S = self.n, self.S
        t = dict(out=to_dev(self.out, dev), doff=to_dev(self.doff, dev), dlen=to_dev(self.dlen, dev),
                 counts=to_dev(np.array([self.m, int(self.doff[self.m])], np.uint64), dev),
                 bind=to_dev(self.bind if S else np.zeros(1, np.uint64), dev))
        d_verdict = None if self.dverdict is None else to_dev(np.concatenate([self.dverdict, np.zeros(n - self.m, np.uint32)]), dev)
        if given is not None:
            t.update({k: given[k] for k in ("out", "doff", "dlen", "counts")})
            d_verdict = given["dverdict"]
        for k, (size, dt) in dict(dstat=(n + 1, np.uint32), dsock=(n + 1, np.uint32), rec=(n + 1, np.uint64), sbase=(S + 2, np.uint64),
                                  scnt=(S + 1, np.uint32), qcounts=(5, np.uint64), fin=(n + 1, np.uint32)).items():
            t[k] = to_dev(np.full(size, UNSET, dt), dev)
        na.rx_demux_plan_dev(t["out"], self.out_bytes, t["doff"], t["dlen"], t["counts"], n, t["bind"] if S else None, S, t["dstat"],
                             t["dsock"], t["rec"], t["sbase"], t["scnt"], t["qcounts"], d_verdict, self.drop_mask, self.align, stream)
        t["q"] = to_dev(np.full(self.q.size, CANARY, np.uint8), dev)
        assert t["q"].data_ptr() % 128 == 0
        if build:
            fin = t["dstat"] if pstat_inplace else t["fin"]
            na.rx_demux_dev(t["out"], self.out_bytes, t["doff"], t["dlen"], t["counts"], n, t["dstat"], t["rec"],
                            t["q"].data_ptr() + 128, self.q_bytes, self.align, fin, stream)
        torch.cuda.synchronize()
        r = {k: v.cpu().numpy() for k, v in t.items()}
        if pstat_inplace:
            r["fin"] = r["dstat"]
        return r

    def check_dev(self, r, build=True, pstat_inplace=False):
        n, S, p = self.n, self.S, self.plan
        if not pstat_inplace:
            assert np.array_equal(r["dstat"][:n], p["dstat"]), "dstat"
        assert np.array_equal(r["dsock"][:n], p["dsock"]), "dsock"
        assert np.array_equal(r["rec"][:n], p["rec"]), "rec"
        assert np.array_equal(r["sbase"][:S + 1], p["sbase"]), "sbase"
        assert np.array_equal(r["scnt"][:S], p["scnt"]), "scnt"
        assert np.array_equal(r["qcounts"][:4], p["qcounts"]), (r["qcounts"], p["qcounts"])
        # nothing behind the arrays' ends
        for k, e in dict(dstat=n, dsock=n, rec=n, sbase=S + 1, scnt=S, qcounts=4).items():
            assert (r[k][e:] == r[k].dtype.type(UNSET)).all(), k
        if build:
            assert np.array_equal(r["fin"][:n], self.fin), "final words"
            assert r["fin"][n] == UNSET
            assert np.array_equal(r["q"], self.q), "q"               # canaries around and between the records included
        else:
            assert (r["q"] == CANARY).all()

    # ---- the host form ----
    def run_host(self):
        n, S = self.m, self.S
        r = dict(dstat=np.full(max(n, 1), UNSET, np.uint32), dsock=np.full(max(n, 1), UNSET, np.uint32),
                 rec=np.full(max(n, 1), UNSET, np.uint64), sbase=np.full(S + 1, UNSET, np.uint64), scnt=np.full(max(S, 1), UNSET, np.uint32),
                 q=np.full(self.q.size, CANARY, np.uint8))
        r["records"] = na.rx_demux_host(self.out, self.out_bytes, self.doff, self.dlen, n, self.host_bind() if S else None, S,
                                        r["q"][128:], self.q_bytes, self.dverdict, self.drop_mask, self.align, r["dstat"], r["dsock"],
                                        r["rec"], r["sbase"], r["scnt"])
        return r

    def check_host(self, r):
        n, S, p = self.m, self.S, self.plan
        assert r["records"] == int(p["qcounts"][0])
        assert np.array_equal(r["dstat"][:n], self.fin[:n]) and np.array_equal(r["dsock"][:n], p["dsock"][:n])
        assert np.array_equal(r["rec"][:n], p["rec"][:n]) and np.array_equal(r["sbase"], p["sbase"])
        assert np.array_equal(r["scnt"][:S], p["scnt"]) and np.array_equal(r["q"], self.q)


# ---------------------------------------------------------------------------------------------
# The batches.
# ---------------------------------------------------------------------------------------------
def binds(S, rng=None):
    """S distinct valid keys: UDP and TCP ports on two addresses."""
    return [dm.key((17, 6)[s & 1], 1000 + (s >> 2), (A, B)[(s >> 1) & 1]) for s in range(S)]


def to_key(k, rng, n, **kw):
    """A datagram with n payload bytes for bind key k."""
    proto, port, addr = k >> 48, (k >> 32) & 0xFFFF, k & 0xFFFFFFFF
    return (dm.udp if proto == 17 else dm.tcp)(payload(rng, n), port, dst=addr, **kw)


PAYLOADS = (0, 1, 7, 8, 9, 15, 16, 17, 63, 64, 65)


def alignment(src_align, align):
    """Source alignment src_align (the payload's address mod 16) times every payload size of PAYLOADS, UDP
    and TCP with thl 20 and 60, to three sockets."""
    rng = np.random.default_rng(100 * src_align + align)
    bind = [dm.key(17, 53, A), dm.key(6, 80, A), dm.key(6, 81, A)]
    dgs, starts, at = [], [], 0
    for P in PAYLOADS:
        for mk, hdr in ((lambda p: dm.udp(p, 53, dst=A), 28), (lambda p: dm.tcp(p, 80, dst=A), 40),
                        (lambda p: dm.tcp(p, 81, dst=A, thl=60, hlen=24), 84)):
            d = mk(payload(rng, max(P, 1) if hdr != 28 and P == 0 else P))
            at = at + (src_align - (at + hdr)) % 16                       # the payload starts at src_align mod 16
            dgs.append(d)
            starts.append(at)
            at += len(d)
    return DmxBatch(dgs, bind, align, starts=starts)


def big_udp(align=16):
    rng = np.random.default_rng(3)
    return DmxBatch([dm.udp(payload(rng, 65507), 7, dst=A), dm.udp(payload(rng, 3), 7, dst=A)], [dm.key(17, 7, A)], align, lead=1)


PART_S = (0, 1, 2, 255, 256, 257, 65535, 65536)
PART_M = (TILE, TILE - 1, TILE + 1, 3 * TILE + 1)


def partition(S, m, seed=0):
    """m small datagrams spread over S sockets (and a few to none), every third one a pure ACK."""
    rng = np.random.default_rng(S * 7 + m + seed)
    bind = binds(S)
    dgs = []
    for k in range(m):
        if S == 0 or k % 11 == 10:
            dgs.append(dm.udp(payload(rng, k % 5), 9, dst=A))            # no socket
        else:
            s = int(rng.integers(0, S))
            if k % 3 == 2 and (s & 1):
                dgs.append(dm.tcp(b"", 1000 + (s >> 2), dst=(A, B)[(s >> 1) & 1], tflags=0x10))
            else:
                dgs.append(to_key(bind[s], rng, 1 + k % 23))
    return DmxBatch(dgs, bind, (8, 16, 128)[m % 3], gap=m & 1)


def one_socket(m=TILE + 5):
    rng = np.random.default_rng(8)
    bind = binds(300)
    return DmxBatch([to_key(bind[299], rng, 1 + k % 40) for k in range(m)], bind, 16)


def descending(S):
    """Every socket exactly once, in descending index order."""
    rng = np.random.default_rng(S)
    bind = binds(S)
    return DmxBatch([to_key(bind[s], rng, 1 + s % 9) for s in range(S - 1, -1, -1)], bind, 8)


def half_none(m=2 * TILE + 3):
    rng = np.random.default_rng(9)
    bind = binds(40)
    dgs = [to_key(bind[k % 40], rng, 5 + k % 7) if k & 1 else dm.ip_datagram(1, payload(rng, 8 + k % 5)) for k in range(m)]
    return DmxBatch(dgs, bind, 8)


def duplicate_keys():
    rng = np.random.default_rng(10)
    k0, k1 = dm.key(17, 53, A), dm.key(6, 80, B)
    bind = [k1, k0, k0, k1, dm.key(17, 54, A), k0]
    dgs = [to_key(bind[s], rng, 10 + s) for s in (5, 3, 2, 4, 0, 1)]
    b = DmxBatch(dgs, bind, 8)
    assert b.plan["dsock"].tolist() == [1, 0, 1, 4, 0, 1] and b.plan["scnt"].tolist() == [2, 3, 0, 0, 1, 0]
    return b


NO_RECORD = ("mask", "noroom", "tiny", "hlen", "icmp", "udp-short", "tcp-short", "thl", "ack", "syn", "rst", "nosock",
             "proto", "addr", "plain")


def no_record(align=8, n=None):
    """Every way to make no record, in one batch, between datagrams that make one."""
    rng = np.random.default_rng(11)
    bind = [dm.key(17, 53, A), dm.key(6, 80, A), dm.key(0, 53, A), dm.key(17, 53, A) | (1 << 56)]   # the last two match nothing
    ok = lambda: dm.udp(payload(rng, 30), 53, dst=A)
    bad_hlen = bytearray(ok())
    bad_hlen[0] = 0x44
    long_hlen = bytearray(dm.udp(b"", 53, dst=A))
    long_hlen[0] = 0x4F
    bad_thl = bytearray(dm.tcp(payload(rng, 9), 80, dst=A))
    bad_thl[32] = 0x40
    long_thl = bytearray(dm.tcp(payload(rng, 9), 80, dst=A))
    long_thl[32] = 0xF0
    cases = [("plain", ok()), ("mask", ok()), ("noroom", ok()), ("tiny", ok()[:19]), ("hlen", bytes(bad_hlen)), ("hlen", bytes(long_hlen)),
             ("icmp", dm.ip_datagram(1, payload(rng, 12), dst=A)), ("udp-short", dm.ip_datagram(17, payload(rng, 7), dst=A)),
             ("tcp-short", dm.ip_datagram(6, payload(rng, 19), dst=A)), ("thl", bytes(bad_thl)), ("thl", bytes(long_thl)),
             ("ack", dm.tcp(b"", 80, dst=A, tflags=0x10)), ("syn", dm.tcp(payload(rng, 4), 80, dst=A, tflags=0x02)),
             ("rst", dm.tcp(payload(rng, 4), 80, dst=A, tflags=0x14)), ("nosock", dm.udp(payload(rng, 5), 54, dst=A)),
             ("nosock", dm.tcp(b"", 81, dst=A, tflags=0x12)),
             ("proto", dm.tcp(payload(rng, 5), 53, dst=A)), ("addr", dm.udp(payload(rng, 5), 53, dst=B)),
             ("plain", dm.tcp(payload(rng, 33), 80, dst=A)), ("plain", dm.udp(b"", 53, dst=A))]
    assert {c[0] for c in cases} == set(NO_RECORD)
    verdict = [0x100 if c[0] == "mask" else rd.NO_ROOM if c[0] == "noroom" else 0x80 for c in cases]
    b = DmxBatch([c[1] for c in cases], bind, align, dverdict=verdict, drop_mask=0x100, lead=3, gap=1, n=n)
    want = dict(plain=dm.QUEUED, mask=dm.DROPPED, noroom=dm.DROPPED, tiny=dm.DROPPED, hlen=dm.DROPPED, icmp=dm.NO_PROTO,
                proto=dm.NO_SOCK, addr=dm.NO_SOCK, ack=dm.CTRL, syn=dm.CTRL, rst=dm.CTRL)
    want.update({"udp-short": dm.SHORT, "tcp-short": dm.SHORT, "thl": dm.SHORT})
    for k, c in enumerate(cases):
        if c[0] == "nosock":
            assert int(b.plan["dstat"][k]) in (dm.NO_SOCK, dm.NO_SOCK | dm.CTRL)
        else:
            assert int(b.plan["dstat"][k]) == want[c[0]], c[0]
    assert [int(b.plan["dsock"][k]) for k, c in enumerate(cases) if c[0] in ("ack", "syn", "rst")] == [1, 1, 1]
    return b


def outside():
    """Rule 1's first clause: a datagram that does not lie inside out_bytes, declared by doff or by dlen."""
    rng = np.random.default_rng(12)
    dgs = [dm.udp(payload(rng, 20), 53, dst=A) for _ in range(4)]
    end = sum(len(d) for d in dgs)
    b = DmxBatch(dgs, [dm.key(17, 53, A)], 8, out_bytes=end - 1, doff_override={1: 1 << 40}, dlen_override={2: 0xFFFFFFFF})
    assert b.plan["dstat"].tolist() == [dm.QUEUED, dm.DROPPED, dm.DROPPED, dm.DROPPED]
    return b


def mixed(m, S, seed=5, align=8, **kw):
    rng = np.random.default_rng(seed)
    bind = binds(S)
    return DmxBatch([to_key(bind[int(rng.integers(0, S))], rng, int(rng.integers(1, 60))) for _ in range(m)], bind, align, **kw)


# name -> a callable that makes the batch (the GPU list; the CPU test holds the host plan to each)
BATCHES = {}
for _sa in range(16):
    for _al in (8, 16, 128):
        BATCHES[f"align-{_sa}-{_al}"] = (lambda sa=_sa, al=_al: alignment(sa, al))
BATCHES["big-udp"] = big_udp
for _i, _S in enumerate(PART_S):
    for _m in PART_M if _S in (2, 257) else (PART_M[_i % 4],):
        BATCHES[f"part-{_S}-{_m}"] = (lambda S=_S, m=_m: partition(S, m))
BATCHES["one-socket"] = one_socket
BATCHES["descending-300"] = lambda: descending(300)
BATCHES["descending-65536"] = lambda: descending(65536)
BATCHES["half-none"] = half_none
BATCHES["duplicate-keys"] = duplicate_keys
BATCHES["no-record"] = no_record
BATCHES["no-record-128"] = lambda: no_record(128)
BATCHES["outside"] = outside
BATCHES["capacity"] = lambda: no_record(16, n=40)                       # n beyond m: the entries [m, n)
BATCHES["null-verdict"] = lambda: mixed(50, 7)
