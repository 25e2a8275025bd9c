"""CPU tests of one-pass RX coalescing (include/nstack_gro.h): the header, the binding and the model
agree; the model (tests/gro_model.py) against the host plan ip_rx_gro_plan_host and against its
golden vectors; the stand-alone ASan + UBSan check of the planning header; and both directions of the
round trip with the segmentation model (tests/tso_model.py)."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import gro_model as gm
import nstack_amd as na
import rxd_model as rd
import rxr_model as rr
from gro_batch import ALL_FLAGS, GBatch, cut, mixed_no_group, payload, stays_apart, tso_datagrams

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MERGED_WORD = gm.GROD_MERGED | (6 << rd.PROTO_SHIFT)


def _header():
    with open(os.path.join(ROOT, "include", "nstack_gro.h")) as f:
        return f.read()


# ---- ABI and constants ----
def test_the_header_declares_exactly_the_listed_and_exported_functions():
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    decl = re.findall(r"\b(\w+)\s*\(", code)
    assert sorted(decl) == sorted(na.GRO_EXPORTS) and len(decl) == 5
    out = subprocess.run(["nm", "-D", "--defined-only", na.LIB_PATH], capture_output=True, text=True, check=True).stdout
    syms = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in decl:
        assert name in syms, name
        assert getattr(na.load(), name).argtypes is not None, name
    others = (set(na.EXPORTS) | set(na.RXV_EXPORTS) | set(na.TXS_EXPORTS) | set(na.TXF_EXPORTS) | set(na.RXR_EXPORTS) |
              set(na.RXD_EXPORTS) | set(na.TXD_EXPORTS) | set(na.TSO_EXPORTS))
    assert not set(na.GRO_EXPORTS) & others
    for name in ("rx_gro_plan_host", "rx_gro_plan_dev", "rx_gro_dev", "rx_gro_host", "gro_last_launch"):
        assert callable(getattr(na, name)) and name in na.__all__
    assert na.gro_last_launch() in ("none", "gro")
    # the argument lists are those of the calls they extend
    sig = lambda n: getattr(na.load(), n).argtypes
    assert sig("ip_rx_gro_plan_host") == sig("ether_rx_reasm_plan_host") and sig("ip_rx_gro_plan_dev") == sig("ether_rx_reasm_plan_dev")
    assert sig("ip_rx_gro_dev") == sig("ip_rx_reasm_l4_dev") and sig("ip_rx_gro_host") == sig("ip_rx_reasm_l4_host")


def test_the_constants_of_header_binding_and_model_agree():
    defs = {k: int(v, 16) for k, v in re.findall(r"#define\s+(GROD?_\w+)\s+(0x[0-9a-fA-F]+)u", _header())}
    assert defs == dict(GRO_CAND=0x1000, GRO_MERGED=0x2000, GRO_FIN=0x4000, GRO_PSH=0x8000, GROD_MERGED=0x400)
    for k, v in defs.items():
        assert getattr(na, k) == v and k in na.__all__
    assert (gm.CAND, gm.MERGED, gm.GFIN, gm.GPSH, gm.GROD_MERGED) == (na.GRO_CAND, na.GRO_MERGED, na.GRO_FIN, na.GRO_PSH, na.GROD_MERGED)
    used = na.RXR_DELIVERED | na.RXR_NO_ROOM | na.RXR_TOO_BIG | na.RXR_INCOMPLETE | 0xFF
    assert not used & (gm.CAND | gm.MERGED | gm.GFIN | gm.GPSH)
    assert not gm.GROD_MERGED & (rd.NO_ROOM | rd.L4_CHECKED | rd.L4_BAD_CSUM | rd.L4_SHORT | 0xFF << rd.PROTO_SHIFT)


# ---- the stand-alone check of the planning header ----
def test_the_standalone_plan_check_runs_clean():
    exe = os.path.join(ROOT, "tests", "c", "gro_plan_check")
    if not os.path.exists(exe):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tests", "c"), "-f", "gro_plan_check.mk"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "gro_plan_check: ok", (r.stdout[-2000:], r.stderr[-2000:])


# ---- the model against the golden vectors ----
def test_the_model_reproduces_its_golden_vectors(inet_oracle):
    vec = gm.load_golden()
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", vec["arena"])) <= 64 << 10
    seen, words = 0, set()
    for c in vec["cases"]:
        b = GBatch(inet_oracle, c["frames"], c["flags"], c["verdict"], c["drop_mask"], c["align"], out_bytes=c["out_bytes"])
        assert [int(s) for s in b.fstat] == c["fstat"], c["tag"]
        assert [int(x) for x in b.plan["dlead"]] == c["dlead"] and [int(x) for x in b.plan["dlen"]] == c["dsize"], c["tag"]
        assert [int(v) for v in b.dverdict] == c["dverdict"], c["tag"]
        for k, dg in enumerate(b.datagrams()):
            if c["dverdict"][k] != rd.NO_ROOM:
                assert dg == c["dgrams"][k], (c["tag"], k)
        for s in c["fstat"]:
            seen |= s
        words |= set(c["dverdict"])
    assert seen & gm.CAND and seen & gm.MERGED and seen & gm.GFIN and seen & gm.GPSH and seen & rr.NO_ROOM and seen & rr.INCOMPLETE
    assert {MERGED_WORD, rd.NO_ROOM, (6 << 16) | rd.L4_CHECKED, (6 << 16) | rd.L4_CHECKED | rd.L4_BAD_CSUM} <= words


def test_the_host_plan_equals_the_model_on_the_golden_batches(inet_oracle):
    for c in gm.load_golden()["cases"]:
        for align in (1, 16, 128):
            GBatch(inet_oracle, c["frames"], c["flags"], c["verdict"], c["drop_mask"], align, lead=align & 3, gap=1).check_plan_host()


# ---- the model against ip_rx_gro_plan_host ----
def test_stays_apart_every_frame_is_delivered_alone(inet_oracle):
    frames, verdict, mask, cases = stays_apart(inet_oracle)
    b = GBatch(inet_oracle, frames, 0, verdict, mask)
    assert not (b.fstat & gm.MERGED).any() and not b.plan["merged"]
    dropped = cases["dropped"][1]
    assert b.m == len(frames) - 1 and b.fstat[dropped] == rr.DROPPED
    for name, idx in cases.items():
        cand = [bool(b.fstat[i] & gm.CAND) for i in idx]
        want = {"syn": [True, False], "rst": [True, False], "urg": [False, True], "p0": [True, False],
                "dropped": [True, False, True]}.get(name, [True] * len(idx))
        assert cand == want, name
    assert (b.dverdict == (6 << 16) | rd.L4_CHECKED).all()                # every one judged by nstack_rxd.h, and valid
    b.check_plan_host()
    # each case merges once its one difference is taken away: the traffic is otherwise coalescible
    ok = GBatch(inet_oracle, [frames[i] for i in cases["gap"][:1]] + [frames[i] for i in cases["duplicate"][1:2]])
    assert ok.m == 2                                                      # (other flows: still apart)


def test_windows_wrap_and_the_size_limit(inet_oracle):
    rng = np.random.default_rng(5)
    # a flow across a 32 KiB boundary: two datagrams, the straddling segment goes by its seq
    a = cut(inet_oracle, gm.tcp_datagram(inet_oracle, payload(rng, 1000), (3 << 15) - 450, tflags=gm.ACK | gm.PSH), 100)
    b = GBatch(inet_oracle, a)
    assert b.m == 2 and b.plan["dlen"].tolist() == [40 + 500, 40 + 500]
    assert [len(v) for v in b.plan["merged"].values()] == [5, 5]
    assert b.fstat[0] & gm.GPSH == 0 and b.fstat[5] & gm.GPSH and b.fstat[5] & rr.HEAD
    b.check_plan_host()
    # a flow across 2^32
    w = cut(inet_oracle, gm.tcp_datagram(inet_oracle, payload(rng, 300), (1 << 32) - 130, hlen=24, thl=32), 60)
    b = GBatch(inet_oracle, w[::-1], align=16)
    assert b.m == 2 and sorted(b.plan["dlen"].tolist()) == [56 + 120, 56 + 180]
    b.check_plan_host()
    # I = 32768 is a candidate, I = 32769 is not: the pair merges, or does not
    for I, merges in ((32768, True), (32769, False)):
        big = gm.tcp_datagram(inet_oracle, payload(rng, I - 40), 0)
        nxt = gm.tcp_datagram(inet_oracle, payload(rng, 10), I - 40)
        b = GBatch(inet_oracle, [rr_frame(big), rr_frame(nxt)])
        assert bool(b.fstat[0] & gm.CAND) == merges and b.m == (1 if merges else 2)
        if merges:
            assert int(b.plan["dlen"][0]) == 32768 + 10
        b.check_plan_host()
    # the largest merged datagram: 32767 + 32768 bytes
    first = gm.tcp_datagram(inet_oracle, payload(rng, 16000), 0)
    mid = gm.tcp_datagram(inet_oracle, payload(rng, 16767), 16000)
    last = gm.tcp_datagram(inet_oracle, payload(rng, 32768 - 40), 32767)
    b = GBatch(inet_oracle, [rr_frame(last), rr_frame(first), rr_frame(mid)])
    assert b.m == 1 and int(b.plan["dlen"][0]) == 65535 and b.dverdict.tolist() == [MERGED_WORD]
    b.check_plan_host()


def rr_frame(dg):
    from rxr_batch import mg
    return mg.frame(dg, False)


def test_mixed_batch_without_a_group_equals_the_reassembly_plan(inet_oracle):
    frames = mixed_no_group(inet_oracle)
    b = GBatch(inet_oracle, frames, rr.F_TRAILER, align=16)
    ref = rr.plan(frames, rr.F_TRAILER, align=16)
    assert not b.plan["merged"] and ((b.fstat & gm.CAND) != 0).sum() == 4
    for k in ("dst", "dgi", "doff", "dlen", "dlead"):
        assert np.array_equal(b.plan[k], ref[k]), k
    assert np.array_equal(b.plan["fstat"] & ~np.uint32(gm.CAND), ref["fstat"])
    b.check_plan_host()


# ---- both directions of the round trip with segmentation ----
@pytest.mark.parametrize("mss", [1460, 1459, 536, 7, 1])
@pytest.mark.parametrize("id_fixed", [False, True])
def test_round_trip_with_the_segmentation_model(inet_oracle, mss, id_fixed):
    dgs = tso_datagrams(inet_oracle, mss)
    assert {(1 << 32) - (1 << 15), 0} <= {struct.unpack_from(">I", d, (d[0] & 15) * 4 + 4)[0] for d in dgs}
    per = [cut(inet_oracle, dg, mss, id_fixed) for dg in dgs]
    assert any(len(p) == 1 for p in per) and any(len(p) > 2 for p in per)
    frames = [f for p in per for f in p]
    order = np.random.default_rng(mss).permutation(len(frames))
    b = GBatch(inet_oracle, [frames[i] for i in order])
    got = b.datagrams()
    assert sorted(got) == sorted(dgs)                                     # every datagram comes back byte for byte
    assert all(d[(d[0] & 15) * 4 + 13] == ALL_FLAGS for d in got)
    assert (b.dverdict == MERGED_WORD).sum() == sum(len(p) > 1 for p in per)
    b.check_plan_host()
    # and segmentation over the output gives the original frames back
    again = [f for dg in got for f in cut(inet_oracle, dg, mss, id_fixed)]
    assert sorted(again) == sorted(frames) and len(again) == b.n


# ---- argument errors (decided before any device call: no GPU needed) and -ENODEV ----
def _args(inet_oracle):
    rng = np.random.default_rng(1)
    frames = cut(inet_oracle, gm.tcp_datagram(inet_oracle, payload(rng, 100), 0), 40)
    arena, off, ln = rr.layout(frames)
    n, bad = len(frames), 0xDEADBEEF
    return dict(arena=arena, off=off, ln=ln, fstat=np.full(n, bad, np.uint32), dst=np.full(n, bad, np.uint64),
                dgi=np.full(n, bad, np.uint32), doff=np.full(n + 1, bad, np.uint64), dlen=np.full(n, bad, np.uint32),
                dlead=np.full(n, bad, np.uint32), counts=np.full(2, bad, np.uint64), out=np.full(400, 0xA5, np.uint8),
                dverdict=np.full(n, bad, np.uint32), bad=np.full(1, bad, np.uint64), n=n)


def _plan_dev(L, a, flags=0, align=1, null=None, n=None):
    p = lambda k: None if k == null else a[k].ctypes.data
    return L.ip_rx_gro_plan_dev(p("arena"), a["arena"].size, p("off"), p("ln"), a["n"] if n is None else n, flags, None, 0, align,
                                p("fstat"), p("dst"), p("dgi"), p("doff"), p("dlen"), p("dlead"), p("counts"), None)


def _plan_host(L, a, flags=0, align=1, null=None, n=None):
    p = lambda k: None if k == null else a[k].ctypes.data
    return L.ip_rx_gro_plan_host(p("arena"), a["arena"].size, p("off"), p("ln"), a["n"] if n is None else n, flags, None, 0, align,
                                 p("fstat"), p("dst"), p("dgi"), p("doff"), p("dlen"), p("dlead"))


def _dev(L, a, flags=0, null=None, n=None):
    p = lambda k: None if k == null else a[k].ctypes.data
    return L.ip_rx_gro_dev(p("arena"), a["arena"].size, p("off"), p("ln"), a["n"] if n is None else n, flags, p("fstat"), p("dst"),
                           p("dgi"), p("doff"), p("dlen"), p("counts"), p("out"), a["out"].size, None, 0x100, p("dverdict"),
                           p("bad"), None)


def _host(L, a, flags=0, align=1, null=None, n=None):
    p = lambda k: None if k == null else a[k].ctypes.data
    return L.ip_rx_gro_host(p("arena"), a["arena"].size, p("off"), p("ln"), a["n"] if n is None else n, flags, None, 0, align,
                            p("out"), a["out"].size, p("fstat"), p("doff"), p("dlen"), p("dlead"), 0x100, p("dverdict"), p("bad"))


def _untouched(a):
    keys = ("fstat", "dst", "dgi", "doff", "dlen", "dlead", "counts", "dverdict", "bad")
    return all((a[k] == 0xDEADBEEF).all() for k in keys) and (a["out"] == 0xA5).all()


def test_argument_errors_are_einval_before_any_device_call(inet_oracle):
    import errno
    L = na.load()
    a = _args(inet_oracle)
    E = -errno.EINVAL
    calls = (_plan_dev, _plan_host, _dev, _host)
    for flags in (2, 0x80000001):                                        # unknown flags
        assert [f(L, a, flags=flags) for f in calls] == [E] * 4, flags
        assert "flag" in L.fcs_last_error().decode()
    for align in (0, 3, 24, 129, 256, 1 << 31):                          # the build takes no align
        assert [f(L, a, align=align) for f in (_plan_dev, _plan_host, _host)] == [E] * 3
        assert "align" in L.fcs_last_error().decode()
    assert [f(L, a, n=1 << 30) for f in calls] == [E] * 4
    for null in ("arena", "off", "ln"):
        assert [f(L, a, null=null) for f in calls] == [E] * 4, null
    for null in ("fstat", "dst", "dgi", "doff", "dlen"):
        assert [f(L, a, null=null) for f in (_plan_dev, _plan_host, _dev)] == [E] * 3, null
    assert _dev(L, a, null="counts") == E and "counts" in L.fcs_last_error().decode()
    assert (_dev(L, a, null="dverdict"), _host(L, a, null="dverdict")) == (E, E)
    off2 = a["off"].copy()
    off2[1] = a["arena"].size
    b = dict(a, off=off2)
    assert (_plan_host(L, b), _host(L, b)) == (E, E) and "frame 1 " in L.fcs_last_error().decode()
    assert _host(L, dict(a, out=a["out"][:139])) == -errno.ENOSPC       # the merged datagram has 140 bytes
    assert _untouched(a)
    assert _plan_host(L, a) == 1 and a["dlen"][0] == 140 and a["doff"][1] == 140


def _no_gpu():
    try:
        import torch
        return not torch.cuda.is_available()
    except Exception:
        return True


@pytest.mark.skipif(not _no_gpu(), reason="a GPU is present")
def test_no_gpu_is_enodev_without_touching_the_host_counters(inet_oracle):
    import errno
    L = na.load()
    a = _args(inet_oracle)
    before = (L.fcs_engine_host_batches(), L.fcs_engine_host_fallbacks())
    assert (_plan_dev(L, a), _dev(L, a), _host(L, a)) == (-errno.ENODEV,) * 3
    assert (L.fcs_engine_host_batches(), L.fcs_engine_host_fallbacks()) == before
    assert _untouched(a)
