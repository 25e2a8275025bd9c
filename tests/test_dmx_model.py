"""CPU tests of one-pass RX demultiplexing (include/nstack_dmx.h): the header, the binding and the
model agree; the record layout against the reference's struct nstack_dgram; the model
(tests/dmx_model.py) against the host plan ip_rx_demux_plan_host on every batch the GPU tests run, and
against its golden vectors; the stand-alone ASan + UBSan check of the planning header; the argument
errors and -ENODEV."""
import errno
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import dmx_batch as db
import dmx_model as dm
import nstack_amd as na
import rxd_model as rd
from dmx_batch import A, BATCHES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_HEADER = "/root/reference/include/nstack_socket.h"


def _header():
    with open(os.path.join(ROOT, "include", "nstack_dmx.h")) as f:
        return f.read()


# ---- ABI and constants ----
def test_the_header_declares_exactly_the_listed_and_exported_functions():
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    decl = re.findall(r"\b(\w+)\s*\(", code)
    assert sorted(decl) == sorted(na.DMX_EXPORTS) and len(decl) == 6
    out = subprocess.run(["nm", "-D", "--defined-only", na.LIB_PATH], capture_output=True, text=True, check=True).stdout
    syms = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in decl:
        assert name in syms, name
        assert getattr(na.load(), name).argtypes is not None, name
    others = (set(na.EXPORTS) | set(na.RXV_EXPORTS) | set(na.TXS_EXPORTS) | set(na.TXF_EXPORTS) | set(na.RXR_EXPORTS) |
              set(na.RXD_EXPORTS) | set(na.TXD_EXPORTS) | set(na.TSO_EXPORTS) | set(na.GRO_EXPORTS))
    assert not set(na.DMX_EXPORTS) & others
    for name in ("rx_demux_plan_host", "rx_demux_plan_dev", "rx_demux_dev", "rx_demux_host", "dmx_last_launch", "dmx_last_host_chunks"):
        assert callable(getattr(na, name)) and name in na.__all__
    assert na.dmx_last_launch() in ("none", "demux")


def test_the_constants_of_header_binding_and_model_agree():
    defs = {k: int(v.rstrip("ul"), 0) for k, v in re.findall(r"#define\s+(DMX_\w+)\s+(0x[0-9a-fA-F]+u(?:ll)?|\d+u)", _header())}
    assert defs == dict(DMX_DROPPED=1, DMX_NO_PROTO=2, DMX_SHORT=4, DMX_CTRL=8, DMX_NO_SOCK=0x10, DMX_QUEUED=0x20, DMX_NO_ROOM=0x40,
                        DMX_DELIVERED=0x80, DMX_NONE32=0xFFFFFFFF, DMX_NONE64=(1 << 64) - 1, DMX_MAX_SOCKS=65536, DMX_REC_HDR=24,
                        DMX_SCRATCH_PER_N=26, DMX_SCRATCH_PER_S=48, DMX_SCRATCH_FIXED=4096)
    for k, v in defs.items():
        assert getattr(na, k) == v and k in na.__all__, k
    assert (dm.DROPPED, dm.NO_PROTO, dm.SHORT, dm.CTRL, dm.NO_SOCK, dm.QUEUED, dm.NO_ROOM, dm.DELIVERED) == \
        (na.DMX_DROPPED, na.DMX_NO_PROTO, na.DMX_SHORT, na.DMX_CTRL, na.DMX_NO_SOCK, na.DMX_QUEUED, na.DMX_NO_ROOM, na.DMX_DELIVERED)
    assert (dm.NONE32, dm.NONE64, dm.REC_HDR, dm.MAX_SOCKS) == (na.DMX_NONE32, na.DMX_NONE64, na.DMX_REC_HDR, na.DMX_MAX_SOCKS)
    assert rd.NO_ROOM == na.RXD_NO_ROOM and dm.key(17, 53, A) == na.dmx_key(17, 53, A) == (17 << 48) | (53 << 32) | A


def test_the_scratch_bound_holds():
    """dmx_launch.hpp's scratch_bytes restated, against the bound the header states (the header also
    static_asserts its terms)."""
    with open(os.path.join(ROOT, "nstack_amd", "csrc", "dmx_launch.hpp")) as f:
        src = f.read()
    assert "static_assert(DMX_SCRATCH_PER_N >= 24 + 1 + 1" in src and "kTile = 1024" in src and "kPlanThreads = 256" in src
    up16 = lambda x: (x + 15) & ~15

    def scratch(n, S):
        t = 16
        while t < 2 * S:
            t <<= 1
        return t * 8 + up16(t * 4) + 6 * up16(n * 4) + up16(-(-n // 1024) * 1024) + up16(-(-n // 256) * 8)
    for n in (1, 2, 3, 255, 256, 257, 1023, 1024, 1025, 4097, 625000, (1 << 30) - 1):
        for S in (0, 1, 7, 8, 9, 255, 256, 257, 32769, 65535, 65536):
            assert scratch(n, S) <= n * na.DMX_SCRATCH_PER_N + S * na.DMX_SCRATCH_PER_S + na.DMX_SCRATCH_FIXED, (n, S)


# ---- the record layout against the reference ----
@pytest.mark.skipif(not os.path.exists(REF_HEADER), reason="the reference's headers are not on this machine")
def test_the_record_is_the_references_struct_nstack_dgram():
    prog = r"""
#include <stddef.h>
#include <stdio.h>
#include <stdint.h>
#include <sys/types.h>
#include <netinet/in.h>
#include "nstack_socket.h"
int main(void) {
    printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(struct nstack_dgram), offsetof(struct nstack_dgram, srcaddr),
           offsetof(struct nstack_dgram, dstaddr), offsetof(struct nstack_dgram, buf_size), offsetof(struct nstack_dgram, buf),
           sizeof(struct nstack_sockaddr), offsetof(struct nstack_sockaddr, inet4_addr), offsetof(struct nstack_sockaddr, port),
           sizeof(size_t));
    return 0;
}
"""
    with tempfile.TemporaryDirectory() as tmp:
        with open(os.path.join(tmp, "layout.c"), "w") as f:
            f.write(prog)
        subprocess.run(["cc", "-std=gnu99", "-I", os.path.dirname(REF_HEADER), "-o", os.path.join(tmp, "layout"),
                        os.path.join(tmp, "layout.c")], check=True, capture_output=True)
        got = [int(x) for x in subprocess.run([os.path.join(tmp, "layout")], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [24, 0, 8, 16, 24, 8, 0, 4, 8]
    r = dm.record(dict(src=0x0A000001, sport=0x1234, dst=A, dport=53, pay=b"xyz"), 8)
    assert r == bytes.fromhex("0100000a" "34120000" "0200000a" "35000000" "0300000000000000") + b"xyz" + bytes(5)
    assert len(dm.record(dict(src=1, sport=2, dst=3, dport=4, pay=b""), 128)) == 128


# ---- the stand-alone check of the planning header ----
def test_the_standalone_plan_check_runs_clean():
    exe = os.path.join(ROOT, "tests", "c", "dmx_plan_check")
    if not os.path.exists(exe):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tests", "c"), "-f", "dmx_plan_check.mk"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "dmx_plan_check: ok", (r.stdout[-2000:], r.stderr[-2000:])


# ---- the model against the golden vectors, and the host plan on them ----
def test_the_model_reproduces_its_golden_vectors():
    vec, blob = dm.load_golden()
    assert blob.size <= 96 << 10 and len(vec["cases"]) >= 8
    seen = 0
    for c in vec["cases"]:
        m, n, S = c["m"], c["n"], len(c["bind"])
        out = blob[c["out_at"]:c["out_at"] + c["out_size"]]
        pl = dm.plan(out, c["out_bytes"], np.array(c["doff"][:m], np.uint64), np.array(c["dlen"][:m], np.uint32), c["bind"], c["align"],
                     c["dverdict"], c["drop_mask"], n)
        for k in ("dstat", "dsock", "rec", "sbase", "scnt", "qcounts"):
            assert [int(x) for x in pl[k]] == c[k], (c["tag"], k)
        q = np.full(c["q_size"], db.CANARY, np.uint8)
        fin = dm.build(pl, q[128:], c["q_bytes"])
        assert [int(x) for x in fin] == c["fin"], c["tag"]
        assert np.array_equal(q, blob[c["q_at"]:c["q_at"] + c["q_size"]]), c["tag"]
        for s in c["fin"]:
            seen |= s
        # and the host plan (an invalid key is -EINVAL there; the device forms let it match nothing)
        bind = np.array(c["bind"], np.uint64)
        if all(dm.key_valid(int(k)) for k in bind):
            dstat, dsock, rec = np.zeros(max(m, 1), np.uint32), np.zeros(max(m, 1), np.uint32), np.zeros(max(m, 1), np.uint64)
            sbase, scnt = np.zeros(S + 1, np.uint64), np.zeros(max(S, 1), np.uint32)
            r = na.rx_demux_plan_host(out, c["out_bytes"], np.array(c["doff"], np.uint64), np.array(c["dlen"], np.uint32), m, bind, S,
                                      dstat, dsock, rec, sbase, scnt, None if c["dverdict"] is None else np.array(c["dverdict"], np.uint32),
                                      c["drop_mask"], c["align"])
            assert r == c["qcounts"][0] and dstat[:m].tolist() == c["dstat"][:m] and rec[:m].tolist() == c["rec"][:m]
            assert sbase.tolist() == c["sbase"] and scnt[:S].tolist() == c["scnt"]
    assert seen == 0xFF                                                   # every status bit occurs


# ---- the model against ip_rx_demux_plan_host on every batch of the GPU list ----
@pytest.mark.parametrize("group", sorted({n.split("-")[0] for n in BATCHES}))
def test_the_host_plan_equals_the_model(group):
    for name, mk in BATCHES.items():
        if name.split("-")[0] == group:
            mk().check_plan_host()


def test_the_batches_cover_what_they_are_for():
    b = db.no_record()
    assert {int(x) for x in b.plan["dstat"]} == {dm.DROPPED, dm.NO_PROTO, dm.SHORT, dm.CTRL, dm.NO_SOCK, dm.NO_SOCK | dm.CTRL, dm.QUEUED}
    assert int(b.plan["qcounts"][0]) == 3 and not all(dm.key_valid(int(k)) for k in b.bind)
    cap = db.no_record(16, n=40)
    assert cap.n == 40 > cap.m and (cap.plan["dstat"][cap.m:] == 0).all() and (cap.plan["rec"][cap.m:] == dm.NONE64).all()
    for sa in range(16):
        a = db.alignment(sa, 8)
        pay_at = {(int(a.doff[k]) + int(a.dlen[k]) - len(a.plan["fields"][k]["pay"])) % 16 for k in a.plan["recs"]}
        assert pay_at == {sa} and len(a.plan["recs"]) == 33
        assert {len(f["pay"]) for f in a.plan["fields"] if f} == set(db.PAYLOADS) | {1}
        assert {int(x) & 15 for x in a.plan["rec"][:a.m]} == {0, 8}      # the record start's phase at align 8
    assert len(db.big_udp().plan["fields"][0]["pay"]) == 65507
    d = db.descending(300)
    assert d.plan["scnt"].tolist() == [1] * 300 and d.plan["dsock"].tolist() == list(range(299, -1, -1))
    assert (np.diff(d.plan["rec"].astype(np.int64)) < 0).all()
    h = db.half_none()
    assert int(h.plan["qcounts"][0]) == h.m // 2
    one = db.one_socket()
    assert int(one.plan["scnt"][299]) == one.m and (np.diff(one.plan["rec"].astype(np.int64)) > 0).all()
    assert {b.S for b in (db.partition(S, db.TILE) for S in db.PART_S)} == {0, 1, 2, 255, 256, 257, 65535, 65536}


# ---- argument errors (decided before any device call: no GPU needed) and -ENODEV ----
def _args():
    b = db.mixed(6, 3)
    bad = 0xDEADBEEF
    n, S = b.m, b.S
    return dict(out=b.out, doff=b.doff, dlen=b.dlen, bind=b.bind, counts=np.array([n, 0], np.uint64), dstat=np.full(n, bad, np.uint32),
                dsock=np.full(n, bad, np.uint32), rec=np.full(n, bad, np.uint64), sbase=np.full(S + 1, bad, np.uint64),
                scnt=np.full(S, bad, np.uint32), qcounts=np.full(4, bad, np.uint64), q=np.full(1024 + 128, 0xA5, np.uint8),
                n=n, S=S, out_bytes=b.out_bytes, need=b.need)


def _q(a):
    return (a["q"].ctypes.data + 127) & ~127


def _plan_host(L, a, align=8, null=None, n=None, S=None, bind=None):
    p = lambda k: None if k == null else (a[k] if bind is None or k != "bind" else bind).ctypes.data
    return L.ip_rx_demux_plan_host(p("out"), a["out_bytes"], p("doff"), p("dlen"), None, a["n"] if n is None else n, p("bind"),
                                   a["S"] if S is None else S, 0, align, p("dstat"), p("dsock"), p("rec"), p("sbase"), p("scnt"))


def _plan_dev(L, a, align=8, null=None, n=None, S=None, bind=None):
    p = lambda k: None if k == null else a[k].ctypes.data
    return L.ip_rx_demux_plan_dev(p("out"), a["out_bytes"], p("doff"), p("dlen"), None, p("counts"), a["n"] if n is None else n,
                                  p("bind"), a["S"] if S is None else S, 0, align, p("dstat"), p("dsock"), p("rec"), p("sbase"),
                                  p("scnt"), p("qcounts"), None)


def _dev(L, a, align=8, null=None, n=None, q_off=0, **_):
    p = lambda k: None if k == null else a[k].ctypes.data
    return L.ip_rx_demux_dev(p("out"), a["out_bytes"], p("doff"), p("dlen"), p("counts"), a["n"] if n is None else n, p("dstat"),
                             p("rec"), align, None if null == "q" else _q(a) + q_off, 1024, None, None)


def _host(L, a, align=8, null=None, n=None, S=None, bind=None, q_bytes=1024):
    p = lambda k: None if k == null else (a[k] if bind is None or k != "bind" else bind).ctypes.data
    return L.ip_rx_demux_host(p("out"), a["out_bytes"], p("doff"), p("dlen"), None, a["n"] if n is None else n, p("bind"),
                              a["S"] if S is None else S, 0, align, None if null == "q" else _q(a), q_bytes, p("dstat"), p("dsock"),
                              p("rec"), p("sbase"), p("scnt"))


def _untouched(a):
    return all((a[k] == 0xDEADBEEF).all() for k in ("dstat", "dsock", "rec", "sbase", "scnt", "qcounts")) and (a["q"] == 0xA5).all()


def test_argument_errors_are_einval_before_any_device_call():
    L = na.load()
    a = _args()
    E = -errno.EINVAL
    calls = (_plan_host, _plan_dev, _dev, _host)
    for align in (0, 1, 4, 12, 24, 129, 256, 1 << 31):
        assert [f(L, a, align=align) for f in calls] == [E] * 4, align
        assert "align" in L.fcs_last_error().decode()
    assert [f(L, a, S=65537) for f in (_plan_host, _plan_dev, _host)] == [E] * 3 and "65536" in L.fcs_last_error().decode()
    assert [f(L, a, n=1 << 30) for f in calls] == [E] * 4
    for null in ("out", "doff", "dlen"):
        assert [f(L, a, null=null) for f in calls] == [E] * 4, null
    for null in ("dstat", "dsock", "rec", "sbase", "scnt", "bind"):
        assert [f(L, a, null=null) for f in (_plan_host, _plan_dev)] == [E] * 2, null
    assert _host(L, a, null="bind") == E and _host(L, a, null="q") == E
    assert _plan_dev(L, a, null="qcounts") == E and _plan_dev(L, a, null="counts") == E and "counts" in L.fcs_last_error().decode()
    assert [_dev(L, a, null=k) for k in ("counts", "dstat", "rec", "q")] == [E] * 4
    for q_off, align in ((8, 16), (64, 128), (4, 8)):                    # the device build wants q aligned to align
        assert _dev(L, a, align=align, q_off=q_off) == E and "aligned" in L.fcs_last_error().decode()
    for key in (dm.key(1, 53, A), 0, dm.key(17, 53, A) | (1 << 56), dm.key(6, 80, A) | (1 << 63)):   # a bad key, in the host forms
        bind = a["bind"].copy()
        bind[1] = key
        assert (_plan_host(L, a, bind=bind), _host(L, a, bind=bind)) == (E, E) and "bind key 1 " in L.fcs_last_error().decode()
    assert _host(L, a, q_bytes=a["need"] - 1) == -errno.ENOSPC            # decided on the host plan, before the device
    assert _untouched(a)
    assert _plan_host(L, a) == 6 and a["sbase"][a["S"]] == a["need"]
    # n = 0 needs no per-datagram array
    z = dict(a, n=0)
    assert _plan_host(L, z, null="dstat") == 0 and a["sbase"][a["S"]] == 0


def _no_gpu():
    try:
        import torch
        return not torch.cuda.is_available()
    except Exception:
        return True


@pytest.mark.skipif(not _no_gpu(), reason="a GPU is present")
def test_no_gpu_is_enodev_without_touching_the_host_counters():
    L = na.load()
    a = _args()
    before = (L.fcs_engine_host_batches(), L.fcs_engine_host_fallbacks())
    assert (_plan_dev(L, a), _dev(L, a), _host(L, a)) == (-errno.ENODEV,) * 3
    assert (_plan_dev(L, a, n=0), _dev(L, a, n=0), _host(L, a, n=0)) == (-errno.ENODEV,) * 3
    assert (L.fcs_engine_host_batches(), L.fcs_engine_host_fallbacks()) == before
    assert _untouched(a)
