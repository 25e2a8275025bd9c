"""CPU tests of one-pass TX multiplexing (include/nstack_mux.h): the header, the binding and the model
agree; the record and route layouts against the reference's structs; the model (tests/mux_model.py)
against the host plan ip_tx_mux_plan_host on every batch the GPU tests run, and against its golden
vectors; the model's datagrams against the oracle's IP checksum and the framing model; the
stand-alone ASan + UBSan check of the planning header; the argument errors and -ENODEV."""
import errno
import os
import re
import struct
import subprocess
import tempfile

import numpy as np
import pytest

import mux_batch as mb
import mux_model as mm
import nstack_amd as na
import txf_model as fm
from mux_batch import BATCHES, HOSTS, IF1, IF2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_SOCKET_H = "/root/reference/include/nstack_socket.h"
REF_IP_H = "/root/reference/src/nstack_ip.h"


def _header():
    with open(os.path.join(ROOT, "include", "nstack_mux.h")) as f:
        return f.read()


# ---- ABI and constants ----
def test_the_header_declares_exactly_the_listed_and_exported_functions():
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    decl = re.findall(r"\b(\w+)\s*\(", code)
    assert sorted(decl) == sorted(na.MUX_EXPORTS) and len(decl) == 6
    out = subprocess.run(["nm", "-D", "--defined-only", na.LIB_PATH], capture_output=True, text=True, check=True).stdout
    syms = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in decl:
        assert name in syms, name
        assert getattr(na.load(), name).argtypes is not None, name
    others = (set(na.EXPORTS) | set(na.RXV_EXPORTS) | set(na.TXS_EXPORTS) | set(na.TXF_EXPORTS) | set(na.RXR_EXPORTS) |
              set(na.RXD_EXPORTS) | set(na.TXD_EXPORTS) | set(na.TSO_EXPORTS) | set(na.GRO_EXPORTS) | set(na.DMX_EXPORTS))
    assert not set(na.MUX_EXPORTS) & others
    for name in ("tx_mux_plan_host", "tx_mux_plan_dev", "tx_mux_dev", "tx_mux_host", "mux_last_launch", "mux_last_host_chunks"):
        assert callable(getattr(na, name)) and name in na.__all__
    assert na.mux_last_launch() in ("none", "mux")


def test_the_constants_of_header_binding_and_model_agree():
    defs = {k: int(v.rstrip("ul"), 0) for k, v in re.findall(r"#define\s+(MUX_\w+)\s+(0x[0-9a-fA-F]+u(?:ll)?|\d+u)", _header())}
    assert defs == dict(MUX_BAD_REC=1, MUX_BAD_SIZE=2, MUX_NO_TCB=4, MUX_NO_ROUTE=8, MUX_NO_NEIGH=0x10, MUX_PLANNED=0x20, MUX_NO_ROOM=0x40,
                        MUX_BUILT=0x80, MUX_MAX_SOCKS=65536, MUX_MAX_ROUTES=256, MUX_MAX_NEIGH=65536, MUX_REC_HDR=24, MUX_IMG=40,
                        MUX_UDP_MAX=65506, MUX_TCP_MAX=65495, MUX_SCRATCH_PER_N=25, MUX_SCRATCH_PER_S=0, MUX_SCRATCH_PER_NB=48,
                        MUX_SCRATCH_FIXED=1024)
    for k, v in defs.items():
        assert getattr(na, k) == v and k in na.__all__, k
    assert (mm.BAD_REC, mm.BAD_SIZE, mm.NO_TCB, mm.NO_ROUTE, mm.NO_NEIGH, mm.PLANNED, mm.NO_ROOM, mm.BUILT) == \
        (na.MUX_BAD_REC, na.MUX_BAD_SIZE, na.MUX_NO_TCB, na.MUX_NO_ROUTE, na.MUX_NO_NEIGH, na.MUX_PLANNED, na.MUX_NO_ROOM, na.MUX_BUILT)
    assert (mm.REC_HDR, mm.IMG, mm.UDP_MAX, mm.TCP_MAX, mm.MAX_SOCKS, mm.MAX_ROUTES, mm.MAX_NEIGH) == \
        (na.MUX_REC_HDR, na.MUX_IMG, na.MUX_UDP_MAX, na.MUX_TCP_MAX, na.MUX_MAX_SOCKS, na.MUX_MAX_ROUTES, na.MUX_MAX_NEIGH)
    assert mm.key(17, 53, IF1) == na.dmx_key(17, 53, IF1)                 # the socket keys are the demux keys
    assert (np.dtype(na.MUX_TCB_DTYPE).itemsize, np.dtype(na.MUX_ROUTE_DTYPE).itemsize, np.dtype(na.MUX_NEIGH_DTYPE).itemsize) == (12, 24, 12)
    for name, fields in (("mux_tcb", "uint32_t seq, ack; uint16_t win; uint8_t flags, pad;"),
                         ("mux_route", "uint32_t network, netmask, gw, iface; uint8_t mac[6]; uint16_t pad;"),
                         ("mux_neigh", "uint32_t addr; uint8_t mac[6]; uint16_t valid;")):
        assert f"struct {name} {{ {fields} }};" in _header(), name


def test_the_scratch_bound_holds():
    """mux_launch.hpp's scratch_bytes restated, against the bound the header states (the header also
    static_asserts its terms)."""
    with open(os.path.join(ROOT, "nstack_amd", "csrc", "mux_launch.hpp")) as f:
        src = f.read()
    assert "static_assert(MUX_SCRATCH_PER_N >= 24 + 1" in src and "6 * up16(n * 4) + up16(b * 8) + 2 * up16(b * 4)" in src
    up16 = lambda x: (x + 15) & ~15

    def scratch(n, N):
        t = 16
        while t < 2 * N:
            t <<= 1
        b = -(-n // 256) + 1
        return t * 8 + up16(t * 4) + 6 * up16(n * 4) + up16(b * 8) + 2 * up16(b * 4)
    for n in (0, 1, 2, 3, 255, 256, 257, 1023, 1024, 1025, 4097, 625000, (1 << 30) - 1):
        for S in (0, 1, 65536):
            for N in (0, 1, 7, 8, 9, 255, 256, 257, 32769, 65535, 65536):
                assert scratch(n, N) <= n * na.MUX_SCRATCH_PER_N + S * na.MUX_SCRATCH_PER_S + N * na.MUX_SCRATCH_PER_NB + na.MUX_SCRATCH_FIXED, (n, N)


# ---- the layouts against the reference ----
def _layout(prog, *incs):
    with tempfile.TemporaryDirectory() as tmp:
        with open(os.path.join(tmp, "layout.c"), "w") as f:
            f.write(prog)
        cmd = ["cc", "-std=gnu99"] + [x for i in incs for x in ("-I", i)] + ["-o", os.path.join(tmp, "layout"), os.path.join(tmp, "layout.c")]
        subprocess.run(cmd, check=True, capture_output=True)
        return [int(x) for x in subprocess.run([os.path.join(tmp, "layout")], capture_output=True, text=True, check=True).stdout.split()]


@pytest.mark.skipif(not (os.path.exists(REF_SOCKET_H) and os.path.exists(REF_IP_H)), reason="the reference's headers are not on this machine")
def test_the_layouts_are_the_references_structs():
    got = _layout(r"""
#include <stddef.h>
#include <stdio.h>
#include <stdint.h>
#include <sys/types.h>
#include <netinet/in.h>
#include "nstack_socket.h"
int main(void) {
    printf("%zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(struct nstack_dgram), offsetof(struct nstack_dgram, srcaddr),
           offsetof(struct nstack_dgram, dstaddr), offsetof(struct nstack_dgram, buf_size), offsetof(struct nstack_dgram, buf),
           sizeof(struct nstack_sockaddr), offsetof(struct nstack_sockaddr, inet4_addr), offsetof(struct nstack_sockaddr, port));
    return 0;
}
""", os.path.dirname(REF_SOCKET_H))
    assert got == [24, 0, 8, 16, 24, 8, 0, 4]
    r = mm.record(HOSTS[0], 53, b"xyz", src=0x0A000001, sport=0x1234)
    assert r == bytes.fromhex("0100000a" "34120000" "0200000a" "35000000" "0300000000000000") + b"xyz"
    got = _layout(r"""
#include <stddef.h>
#include <stdio.h>
#include <stdint.h>
#include <sys/types.h>
#include <netinet/in.h>
#include "nstack_ip.h"
int main(void) {
    printf("%zu %zu %zu %zu %zu %zu\n", sizeof(struct ip_route), offsetof(struct ip_route, r_network), offsetof(struct ip_route, r_netmask),
           offsetof(struct ip_route, r_gw), offsetof(struct ip_route, r_iface), offsetof(struct ip_route, r_iface_handle));
    return 0;
}
""", os.path.dirname(REF_IP_H), os.path.dirname(REF_SOCKET_H))
    assert got == [20, 0, 4, 8, 12, 16]                                   # the MAC takes the handle's place, at 16
    dt = np.dtype(na.MUX_ROUTE_DTYPE)
    assert [dt.fields[k][1] for k in ("network", "netmask", "gw", "iface", "mac")] == [0, 4, 8, 12, 16]


# ---- the stand-alone check of the planning header ----
def test_the_standalone_plan_check_runs_clean():
    exe = os.path.join(ROOT, "tests", "c", "mux_plan_check")
    if not os.path.exists(exe):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tests", "c"), "-f", "mux_plan_check.mk"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "mux_plan_check: ok", (r.stdout[-2000:], r.stderr[-2000:])


# ---- the model against the golden vectors, the oracle and the framing model; the host plan on them ----
def test_the_model_reproduces_its_golden_vectors(inet_oracle):
    vec, blob = mm.load_golden()
    assert blob.size <= 160 << 10 and len(vec["cases"]) >= 8
    seen, dgs = 0, 0
    for c in vec["cases"]:
        n, S = c["n"], len(c["bind"])
        q = blob[c["q_at"]:c["q_at"] + c["q_size"]]
        rt = [mm.route(r[0], r[1], r[3], bytes.fromhex(r[4]), gw=r[2]) for r in c["rt"]]
        nb = [(a, bytes.fromhex(m), v) for a, m, v in c["nb"]]
        tcb = None if c["tcb"] is None else [tuple(t) for t in c["tcb"]]
        pl = mm.plan(q, c["q_bytes"], c["rec"], c["sfirst"], c["bind"], tcb, rt, nb, c["id0"], c["align"])
        for k in ("mstat", "off", "len", "tnext", "counts"):
            assert [int(x) for x in pl[k]] == c[k], (c["tag"], k)
        himg = blob[c["himg_at"]:c["himg_at"] + 40 * n].reshape(n, 40)
        assert np.array_equal(pl["l2"], blob[c["l2_at"]:c["l2_at"] + 12 * n].reshape(n, 12)) and np.array_equal(pl["himg"], himg), c["tag"]
        dgram = np.full(c["dgram_size"], mb.CANARY, np.uint8)
        fin = mm.build(pl, dgram[128:], c["dgram_bytes"])
        assert [int(x) for x in fin] == c["fin"], c["tag"]
        assert np.array_equal(dgram, blob[c["dgram_at"]:c["dgram_at"] + c["dgram_size"]]), c["tag"]
        for s in c["fin"]:
            seen |= s
        # other witnesses than the model: the oracle's IP checksum over every header in the file, and the
        # framing model on every datagram
        for k in range(n):
            if c["mstat"][k] & mm.PLANNED:
                hdr = himg[k, :20].tobytes()
                assert inet_oracle.oracle_ip_checksum(hdr, 20) == 0, (c["tag"], k)
                assert hdr[10:12] == struct.pack("<H", inet_oracle.oracle_ip_checksum(hdr[:10] + bytes(2) + hdr[12:], 20))
                st = fm.plan(pl["dgs"][k], 1500)[0]
                assert st & (fm.WHOLE | fm.FRAGMENTED) and not st & (fm.BAD_HDR | fm.BAD_LEN), (c["tag"], k)
                dgs += 1
            else:
                assert not himg[k].any() and c["len"][k] == 0
                assert fm.plan(b"", 1500)[0] == fm.BAD_HDR                # what the framing calls make of len = 0
        # and the host plan
        o = dict(mstat=np.zeros(max(n, 1), np.uint32), off=np.zeros(max(n, 1), np.uint64), len=np.zeros(max(n, 1), np.uint32))
        r = na.tx_mux_plan_host(q, c["q_bytes"], np.array(c["rec"] + [0], np.uint64), n, np.array(c["sfirst"], np.uint64),
                                np.array(c["bind"], np.uint64), S, _tcb_np(tcb, S), _rt_np(rt), len(rt), _nb_np(nb), len(nb), o["mstat"],
                                o["off"], o["len"], np.zeros(max(n, 1) * 12, np.uint8), np.zeros(max(n, 1) * 40, np.uint8), None, None,
                                c["id0"], c["align"])
        assert r == c["counts"][0] and o["mstat"][:n].tolist() == c["mstat"] and o["off"][:n].tolist() == c["off"] and o["len"][:n].tolist() == c["len"]
    assert seen == 0xFF and dgs > 150                                     # every status bit occurs


def _tcb_np(tcb, S):
    if tcb is None:
        return None
    a = np.zeros(max(S, 1), na.MUX_TCB_DTYPE)
    for s, t in enumerate(tcb):
        a[s] = (t[0], t[1], t[2], t[3], 0)
    return a


def _rt_np(rt):
    a = np.zeros(max(len(rt), 1), na.MUX_ROUTE_DTYPE)
    for i, r in enumerate(rt):
        a[i] = (r["network"], r["netmask"], r["gw"], r["iface"], list(r["mac"]), 0)
    return a


def _nb_np(nb):
    a = np.zeros(max(len(nb), 1), na.MUX_NEIGH_DTYPE)
    for i, (addr, mac, valid) in enumerate(nb):
        a[i] = (addr, list(mac), valid)
    return a


# ---- the model against ip_tx_mux_plan_host on every batch of the GPU list ----
@pytest.mark.parametrize("group", sorted({n.split("-")[0] for n in BATCHES}))
def test_the_host_plan_equals_the_model(group):
    for name, mk in BATCHES.items():
        if name.split("-")[0] == group:
            mk().check_plan_host()


def test_every_modelled_datagram_passes_the_framing_model(inet_oracle):
    for name in ("status-all", "wraps", "copy-17-4", "copy-6-16", "routes-256", "neigh-257", "rows-33"):
        b = BATCHES[name]()
        for k, d in b.plan["dgs"].items():
            st = fm.plan(d, 1500)[0]
            assert st & (fm.WHOLE | fm.FRAGMENTED) and not st & (fm.BAD_HDR | fm.BAD_LEN), (name, k)
            assert inet_oracle.oracle_ip_checksum(d[:20], 20) == 0, (name, k)


# ---- the route lookup, the id wrap and the seq wrap at their edges ----
def _src(b, k):
    return struct.unpack_from(">I", b.plan["himg"][k].tobytes(), 12)[0]


def test_the_three_step_route_lookup_at_its_edges():
    x = mb.NET1 + 9
    b = mb.tables_routes(2)                                               # an exact match behind a mask match of a lower index
    assert _src(b, 0) == IF2 and _src(b, 1) == IF1 and b.plan["mstat"][2:5].tolist() == [mm.NO_ROUTE] * 3
    b = mb.tables_routes(256)                                             # two mask matches: the lower index; a default through step 3
    assert _src(b, 0) == IF1 and _src(b, 1) == IF1 and _src(b, 4) == mb.IF0 and _src(b, 3) == 0x64000501 and _src(b, 2) == mb.IF0
    assert mm.route_find(b.rt, x) == 253 and mm.route_find(b.rt, 0x08080808) == 255 and mm.route_find(b.rt, 0x64000507) == 5
    b = mb.tables_routes(1)                                               # a default route (netmask 0) through step 2
    assert int(b.plan["counts"][0]) == b.n and _src(b, 0) == mb.IF0
    assert mm.route_find([mm.route(0, 0xFF000000, 1, bytes(6))], x) == 0 and mm.route_find([mm.route(0, 0xFF000000, 1, bytes(6))], 0x00000005) == 0
    b = mb.tables_routes(0)                                               # R = 0
    assert int(b.plan["counts"][0]) == 0 and int(b.plan["counts"][2]) == b.n and (b.plan["mstat"] == mm.NO_ROUTE).all()
    for R in (0, 1, 2, 256):
        mb.tables_routes(R).check_plan_host()


def test_the_ip_id_and_the_sequence_number_wrap():
    b = mb.wraps()
    ids = {k: struct.unpack_from(">H", d, 4)[0] for k, d in b.plan["dgs"].items()}
    assert ids == {0: 0xFFFE, 2: 0xFFFF, 3: 0, 5: 1, 7: 2, 8: 3} and b.plan["mstat"][1] == mm.NO_ROUTE and b.plan["mstat"][4] == mm.BAD_SIZE
    seqs = {k: struct.unpack_from(">I", d, 24)[0] for k, d in b.plan["dgs"].items() if d[9] == 6}
    assert seqs == {0: 0xFFFFFF00, 2: 0x0000002C, 7: 0xFFFFFFFF, 8: 0xFFFFFFFF}   # the unplanned records add nothing; P = 0 adds nothing
    assert b.plan["tnext"].tolist() == [0x2C + 200, 0, 6]
    b.check_plan_host()


def test_the_batches_cover_what_they_are_for():
    b = mb.no_datagram()
    assert {int(x) for x in b.plan["mstat"]} == {mm.BAD_REC, mm.BAD_SIZE, mm.NO_ROUTE, mm.NO_NEIGH, mm.PLANNED}
    assert {int(x) for x in mb.no_datagram(8, tcb=False).plan["mstat"]} >= {mm.NO_TCB, mm.NO_TCB | mm.BAD_SIZE}
    assert {len(d) - 28 for d in mb.copy(17, 4).plan["dgs"].values()} == set(mb.COPY_SIZES) | {65506}
    assert {len(d) - 40 for d in mb.copy(6, 4).plan["dgs"].values()} == set(mb.COPY_SIZES) | {0, 65495}
    nb = mb.tables_neigh(257)
    assert nb.plan["l2"][1, :6].tobytes() == mb.MAC(0) and nb.plan["l2"][6, :6].tobytes() == mb.MAC(0x654321)   # duplicates: the lowest index
    assert nb.plan["mstat"][4] == mm.NO_NEIGH and nb.plan["l2"][7, :6].tobytes() == mb.MAC(3)
    s = mb.tables_socks(65536)
    assert s.S == 65536 and s.sfirst[1] == 0 and s.sfirst[65535] == s.n == s.sfirst[65536]
    big = BATCHES["blocks-65537"]()
    assert big.n == 65537 and int(big.plan["counts"][0]) > 256 * 200


# ---- argument errors (decided before any device call: no GPU needed) and -ENODEV ----
def _args():
    b = mb.mixed(6, 3, seed=3, align=8)
    bad = 0xDEADBEEF
    n, S = b.n, b.S
    a = dict(q=b.q, rec=b.rec, sfirst=b.sfirst, bind=b.bind, tcb=b.tcb_np, rt=b.rt_np, nb=b.nb_np, mstat=np.full(n, bad, np.uint32),
             off=np.full(n, bad, np.uint64), len=np.full(n, bad, np.uint32), l2=np.full(n * 12, 0xA5, np.uint8), himg=np.full(n * 40, 0xA5, np.uint8),
             tnext=np.full(S, bad, np.uint32), counts=np.full(4, bad, np.uint64), dgram=np.full(4096 + 128, 0xA5, np.uint8),
             n=n, S=S, R=b.R, N=b.N, q_bytes=b.q_bytes, need=b.need, planned=int(b.plan["counts"][0]))
    return a


def _dg(a):
    return (a["dgram"].ctypes.data + 127) & ~127


def _ptrs(a, null, over):
    return lambda k: None if k == null else (over[k] if k in over else a[k]).ctypes.data


def _plan_host(L, a, align=8, null=None, **kw):
    p, g = _ptrs(a, null, {k: v for k, v in kw.items() if isinstance(v, np.ndarray)}), lambda k: kw.get(k, a[k])
    return L.ip_tx_mux_plan_host(p("q"), a["q_bytes"], p("rec"), g("n"), p("sfirst"), p("bind"), g("S"), p("tcb"), p("rt"), g("R"), p("nb"),
                                 g("N"), 0, align, p("mstat"), p("off"), p("len"), p("l2"), p("himg"), p("tnext"), p("counts"))


def _plan_dev(L, a, align=8, null=None, **kw):
    p, g = _ptrs(a, null, {k: v for k, v in kw.items() if isinstance(v, np.ndarray)}), lambda k: kw.get(k, a[k])
    return L.ip_tx_mux_plan_dev(p("q"), a["q_bytes"], p("rec"), g("n"), p("sfirst"), p("bind"), g("S"), p("tcb"), p("rt"), g("R"), p("nb"),
                                g("N"), 0, align, p("mstat"), p("off"), p("len"), p("l2"), p("himg"), p("tnext"), p("counts"), None)


def _dev(L, a, align=8, null=None, d_off=0, **kw):
    p, g = _ptrs(a, null, {}), lambda k: kw.get(k, a[k])
    return L.ip_tx_mux_dev(p("q"), a["q_bytes"], p("rec"), g("n"), p("mstat"), p("off"), p("len"), p("himg"), align,
                           None if null == "dgram" else _dg(a) + d_off, 4096, None, None)


def _host(L, a, align=8, null=None, dgram_bytes=4096, **kw):
    p, g = _ptrs(a, null, {k: v for k, v in kw.items() if isinstance(v, np.ndarray)}), lambda k: kw.get(k, a[k])
    return L.ip_tx_mux_host(p("q"), a["q_bytes"], p("rec"), g("n"), p("sfirst"), p("bind"), g("S"), p("tcb"), p("rt"), g("R"), p("nb"), g("N"),
                            0, align, None if null == "dgram" else _dg(a), dgram_bytes, p("mstat"), p("off"), p("len"), p("l2"), p("himg"),
                            p("tnext"), p("counts"))


def _untouched(a):
    return (all((a[k] == 0xDEADBEEF).all() for k in ("mstat", "off", "len", "tnext", "counts")) and
            all((a[k] == 0xA5).all() for k in ("l2", "himg", "dgram")))


def test_argument_errors_are_einval_before_any_device_call():
    L = na.load()
    a = _args()
    E = -errno.EINVAL
    calls = (_plan_host, _plan_dev, _dev, _host)
    tables = (_plan_host, _plan_dev, _host)
    for align in (0, 1, 2, 3, 12, 24, 129, 256, 1 << 31):
        assert [f(L, a, align=align) for f in calls] == [E] * 4, align
        assert "align" in L.fcs_last_error().decode()
    assert [f(L, a, S=65537) for f in tables] == [E] * 3 and "65536" in L.fcs_last_error().decode()
    assert [f(L, a, R=257) for f in tables] == [E] * 3 and "256" in L.fcs_last_error().decode()
    assert [f(L, a, N=65537) for f in tables] == [E] * 3 and "neighbours" in L.fcs_last_error().decode()
    assert [f(L, a, n=1 << 30) for f in calls] == [E] * 4
    assert [f(L, a, S=0) for f in tables] == [E] * 3 and "no socket" in L.fcs_last_error().decode()
    for null in ("q", "rec"):
        assert [f(L, a, null=null) for f in calls] == [E] * 4, null
    for null in ("sfirst", "bind", "rt", "nb"):
        assert [f(L, a, null=null) for f in tables] == [E] * 3, null
    for null in ("mstat", "off", "len", "l2", "himg"):
        assert [f(L, a, null=null) for f in (_plan_host, _plan_dev)] == [E] * 2, null
    assert _plan_dev(L, a, null="counts") == E and "counts" in L.fcs_last_error().decode()
    assert [_dev(L, a, null=k) for k in ("mstat", "off", "len", "himg", "dgram")] == [E] * 5 and _host(L, a, null="dgram") == E
    for d_off, align in ((8, 16), (64, 128), (4, 8)):                    # the device build wants dgram aligned to align
        assert _dev(L, a, align=align, d_off=d_off) == E and "aligned" in L.fcs_last_error().decode()
    n = a["n"]
    for bad in ([1, 2, 4, n], [0, 4, 2, n], [0, 2, 4, n + 1], [0, 2, 4, n - 1]):   # sfirst: not from 0, not monotone, not to n
        sf = np.array(bad, np.uint64)
        assert (_plan_host(L, a, sfirst=sf), _host(L, a, sfirst=sf)) == (E, E) and "sfirst" in L.fcs_last_error().decode(), bad
    assert _host(L, a, dgram_bytes=a["need"] - 8) == -errno.ENOSPC       # decided on the host plan, before the device
    assert _untouched(a)
    assert _plan_host(L, a) == a["planned"] and a["counts"][1] == a["need"]
    # n = 0 needs no per-record array, and S = 0 no table
    z = dict(a, n=0, sfirst=np.zeros(4, np.uint64))
    assert _plan_host(L, z, null="mstat") == 0 and a["counts"].tolist() == [0, 0, 0, 0]
    assert _plan_host(L, z, S=0, null="bind") == 0 and _plan_host(L, z, R=0, N=0, null="rt") == 0


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
    z = dict(a, n=0, sfirst=np.zeros(4, np.uint64))
    assert (_plan_dev(L, z), _dev(L, z), _host(L, z)) == (-errno.ENODEV,) * 3
    assert (L.fcs_engine_host_batches(), L.fcs_engine_host_fallbacks()) == before
    assert _untouched(a)
