"""CPU tests of reassembly with L4 verdicts (include/nstack_rxd.h): the ABI, the constants, the argument
errors that need no GPU, the additivity argument the kernels rest on (a datagram's L4 sum is the sum of
its fragments' payload sums on the datagram's 16-bit grid), stated with the oracle's own checksums, and
the model (tests/rxd_model.py) against the validator's model on unfragmented frames."""
import errno
import os
import random
import re
import socket
import struct
import subprocess

import numpy as np
import pytest

import nstack_amd as na
import rxd_model as rd
import rxr_model as rr
import rxv_model as rv
from rxd_batch import Traffic, whole_mix
from rxr_batch import mg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "nstack_rxd.h")).read()


# ---- ABI ----
def test_the_header_declares_exactly_three_exported_and_listed_functions():
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    decl = re.findall(r"\b(\w+)\s*\(", code)
    assert sorted(decl) == sorted(na.RXD_EXPORTS) and len(decl) == 3
    assert not any(re.fullmatch(r"ether_rx_reasm\w*|fcs_debug_rxr_\w*", name) for name in decl)
    out = subprocess.run(["nm", "-D", "--defined-only", na.LIB_PATH], capture_output=True, text=True, check=True).stdout
    syms = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in decl:
        assert name in syms, name
        assert getattr(na.load(), name).argtypes is not None, name
    others = set(na.EXPORTS) | set(na.RXV_EXPORTS) | set(na.TXS_EXPORTS) | set(na.TXF_EXPORTS) | set(na.RXR_EXPORTS)
    assert not set(na.RXD_EXPORTS) & others
    for name in ("rx_reasm_l4_dev", "rx_reasm_l4_host", "rxd_last_launch"):
        assert callable(getattr(na, name)) and name in na.__all__


def test_the_l4_bits_are_the_validators_and_the_header_the_binding_and_the_model_agree():
    assert (na.RXD_L4_CHECKED, na.RXD_L4_BAD_CSUM, na.RXD_L4_SHORT, na.RXD_PROTO_SHIFT) == \
        (na.RXV_L4_CHECKED, na.RXV_L4_BAD_CSUM, na.RXV_L4_SHORT, na.RXV_PROTO_SHIFT)
    found = dict(re.findall(r"#define\s+(RXD_\w+)\s+(0x[0-9a-fA-F]+|\d+)u?\b", _header()))
    assert sorted(found) == ["RXD_L4_BAD_CSUM", "RXD_L4_CHECKED", "RXD_L4_SHORT", "RXD_NO_ROOM", "RXD_PROTO_SHIFT"]
    for name, val in found.items():
        assert getattr(na, name) == int(val, 0) == getattr(rd, name[4:]), name
    assert na.RXD_NO_ROOM == 0x002 and not na.RXD_NO_ROOM & rd.L4_BITS
    assert na.rxd_last_launch() in ("none", "general-l4")


# ---- argument errors (decided before any device call: no GPU needed) ----
def _args(n=3):
    frames = mg.fragments(None, bytes(range(100)), [48], False) + [mg.frame(mg.ip_packet(bytes(30)), False)]
    arena, off, ln = rr.layout(frames[:n])
    a = dict(arena=arena, off=off, ln=ln, fstat=np.full(n, 0xDEADBEEF, np.uint32), dst=np.full(n, 0xDEADBEEF, np.uint64),
             dgi=np.full(n, 0xDEADBEEF, np.uint32), doff=np.full(n + 1, 0xDEADBEEF, np.uint64),
             dlen=np.full(n, 0xDEADBEEF, np.uint32), dlead=np.full(n, 0xDEADBEEF, np.uint32), counts=np.full(2, 0xDEADBEEF, np.uint64),
             out=np.full(400, 0xA5, np.uint8), dverdict=np.full(n, 0xDEADBEEF, np.uint32), bad=np.full(1, 0xDEADBEEF, np.uint64), n=n)
    return a


def _dev(L, a, flags=0, null=None, n=None):
    p = lambda k: None if k == null else a[k].ctypes.data
    return L.ip_rx_reasm_l4_dev(p("arena"), a["arena"].size, p("off"), p("ln"), a["n"] if n is None else n, flags, p("fstat"),
                                p("dst"), p("dgi"), p("doff"), p("dlen"), p("counts"), p("out"), a["out"].size, None, 0x100,
                                p("dverdict"), p("bad"), None)


def _host(L, a, flags=0, align=1, null=None, n=None):
    p = lambda k: None if k == null else a[k].ctypes.data
    return L.ip_rx_reasm_l4_host(p("arena"), a["arena"].size, p("off"), p("ln"), a["n"] if n is None else n, flags, None, 0, align,
                                 p("out"), a["out"].size, p("fstat"), p("doff"), p("dlen"), p("dlead"), 0x100, p("dverdict"),
                                 p("bad"))


def _untouched(a):
    keys = ("fstat", "dst", "dgi", "doff", "dlen", "dlead", "counts", "dverdict", "bad")
    return all((a[k] == 0xDEADBEEF).all() for k in keys) and (a["out"] == 0xA5).all()


def test_argument_errors_are_einval_before_any_device_call():
    L = na.load()
    a = _args()
    E = -errno.EINVAL
    for flags in (2, 0x80000001):                                        # unknown flags
        assert (_dev(L, a, flags=flags), _host(L, a, flags=flags)) == (E, E), flags
        assert "flag" in L.fcs_last_error().decode()
    assert _dev(L, a, null="counts") == E and "counts" in L.fcs_last_error().decode()
    assert _dev(L, a, null="counts", n=0) == E                           # required whatever n is
    assert (_dev(L, a, null="dverdict"), _host(L, a, null="dverdict")) == (E, E)
    assert "dverdict" in L.fcs_last_error().decode()
    for align in (0, 3, 24, 129, 256, 1 << 31):                          # the device form takes no align
        assert _host(L, a, align=align) == E and "align" in L.fcs_last_error().decode()
    assert (_dev(L, a, n=1 << 30), _host(L, a, n=1 << 30)) == (E, E)
    for null in ("arena", "off", "ln"):
        assert (_dev(L, a, null=null), _host(L, a, null=null)) == (E, E), null
    for null in ("fstat", "dst", "dgi", "doff", "dlen", "out"):          # fstat here is the device form's pstat
        assert _dev(L, a, null=null) == E, null
    with pytest.raises(na.FcsError) as e:
        na.rx_reasm_l4_host(a["arena"], a["arena"].size, a["off"], a["ln"], 3, a["out"], a["out"].size, a["dverdict"], align=3)
    assert e.value.rc == E
    # the host form checks the arena and the capacity as ether_rx_reasm_host does
    off2 = a["off"].copy()
    off2[1] = a["arena"].size
    b = dict(a, off=off2)
    assert _host(L, b) == E and "frame 1 " in L.fcs_last_error().decode()
    a2 = dict(a, out=a["out"][:169])
    assert _host(L, a2) == -errno.ENOSPC
    assert _untouched(a)
    assert _host(L, a, n=0) == 0 and a["bad"][0] == 0 and a["doff"][0] == 0   # the empty batch: bad and doff[0], nothing else
    a["bad"][0] = a["doff"][0] = 0xDEADBEEF
    assert _untouched(a)


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
    assert (_dev(L, a), _host(L, a)) == (-errno.ENODEV,) * 2
    assert (L.fcs_engine_host_batches(), L.fcs_engine_host_fallbacks()) == before
    assert _untouched(a)


# ---- additivity: what the kernels rest on ----
def _fold(x):
    while x >> 16:
        x = (x & 0xFFFF) + (x >> 16)
    return x


def _sum_of(inet_oracle, b: bytes) -> int:
    """The one's-complement sum of b's 16-bit words (as ip_checksum reads them), from the oracle's own
    checksum: ip_checksum returns the complement of 0xffff + sum."""
    return ~inet_oracle.oracle_ip_checksum(b, len(b)) & 0xFFFF


def _verdict_from_fragments(inet_oracle, frames, cls, dg):
    """The verdict word of the datagram `dg` the fragments `frames` make, its L4 sum taken from the
    fragments' payloads alone: every payload starts at an even datagram position (offsets are multiples
    of 8, header lengths of 4), so each one's own sum is its part of the datagram's sum."""
    hlen, proto, D = (dg[0] & 15) * 4, dg[9], len(dg)
    L = D - hlen
    v = proto << rd.PROTO_SHIFT
    src_raw, dst_raw = struct.unpack_from("<II", dg, 12)
    zeros = bytes(L)
    if proto == 6:
        if L < 20:
            return v | rd.L4_SHORT
        pseudo = ~inet_oracle.oracle_tcp_checksum(socket.ntohl(src_raw), socket.ntohl(dst_raw), zeros, L) & 0xFFFF
    elif proto == 17:
        if L < 8:
            return v | rd.L4_SHORT
        if dg[hlen + 6:hlen + 8] == b"\x00\x00":
            return v
        pseudo = ~inet_oracle.oracle_udp_checksum(zeros, L, src_raw, dst_raw) & 0xFFFF
    elif proto == 1:
        if L < 4:
            return v | rd.L4_SHORT
        pseudo = ~inet_oracle.oracle_ip_checksum(zeros, L) & 0xFFFF
    else:
        return v
    total = pseudo
    for f, c in zip(frames, cls):
        fh, I, o = c[1], c[2], c[3]
        assert o % 2 == 0 and fh % 2 == 0
        total = _fold(total + _sum_of(inet_oracle, f[14 + fh:14 + I]))
    return v | rd.L4_CHECKED | (rd.L4_BAD_CSUM if total != 0xFFFF else 0)


def _valid_fragmented(inet_oracle):
    """Fragmented datagrams of the three protocols with valid checksums, odd lengths among them."""
    rng = random.Random(11)
    frames = []
    for q, (kind, n, cuts, hh) in enumerate((("udp", 91, [24, 64], 20), ("tcp", 70, [16, 40, 72], 24), ("icmp", 57, [8, 48], 60),
                                             ("udp", 300, [128, 256], 60), ("tcp", 33, [24], 20), ("icmp", 130, [64], 24))):
        src, dst = 0x0A000001 + q, 0xC0A80001 + 3 * q
        seg = rd.segment(inet_oracle, kind, bytes(rng.randrange(256) for _ in range(n)), src, dst)
        frames += mg.fragments(rng, seg, cuts, False, hlen_head=hh, hlen_rest=20, ident=q, src=src, dst=dst, proto=rd.PROTO[kind])
    return frames


def test_a_datagrams_l4_sum_is_the_sum_of_its_fragments_payload_sums(inet_oracle):
    golden = rr.load_golden()
    batches = [(c["tag"], c["frames"], c["flags"], c["verdict"], c["drop_mask"]) for c in golden["cases"]]
    valid = _valid_fragmented(inet_oracle)
    batches.append(("valid", valid, 0, None, 0))
    bent = list(valid)
    f = bytearray(bent[1])
    f[14 + 20 + 5] ^= 0x04                                               # a payload bit of a middle fragment
    bent[1] = bytes(f)
    batches.append(("bent", bent, 0, None, 0))
    groups = checked = bad = 0
    for tag, frames, flags, verdict, drop_mask in batches:
        pl = rr.plan(frames, flags, verdict, drop_mask)
        arena, _ = rr.build(inet_oracle, frames, pl, np.zeros(int(pl["doff"][-1]), dtype=np.uint8))
        want = rd.verdicts(inet_oracle, arena, pl)
        dgs = rr.datagrams(arena, pl)
        for k in range(pl["m"]):
            idx = [i for i in range(len(frames)) if pl["dgi"][i] == k]
            if len(idx) < 2:
                continue
            got = _verdict_from_fragments(inet_oracle, [frames[i] for i in idx], [pl["cls"][i] for i in idx], dgs[k])
            assert got == int(want[k]), (tag, k, hex(got), hex(int(want[k])))
            groups += 1
            checked += bool(got & rd.L4_CHECKED)
            bad += bool(got & rd.L4_BAD_CSUM)
        if tag == "valid":
            assert (want == [(rd.PROTO[k] << 16) | rd.L4_CHECKED for k in ("udp", "tcp", "icmp") * 2]).all()
        if tag == "bent":
            assert int(want[0]) == (17 << 16) | rd.L4_CHECKED | rd.L4_BAD_CSUM and (want[1:] & rd.L4_BAD_CSUM == 0).all()
    assert groups > 40 and checked > 20 and 0 < bad < checked


def test_on_unfragmented_frames_the_model_agrees_with_the_validators_model(oracle, inet_oracle):
    frames = whole_mix(inet_oracle)
    pl = rr.plan(frames, rr.F_TRAILER)
    assert pl["m"] == len(frames)
    arena, _ = rr.build(inet_oracle, frames, pl, np.zeros(int(pl["doff"][-1]), dtype=np.uint8))
    got = rd.verdicts(inet_oracle, arena, pl)
    want = np.array([rv.verdict(oracle, inet_oracle, f, rv.F_TRAILER) for f in frames], dtype=np.uint32)
    assert np.array_equal(got & rd.L4_BITS, want & rd.L4_BITS), [(hex(a), hex(b)) for a, b in zip(got, want)]
    assert (got & rd.L4_BITS == got).all()
    seen = 0
    for v in got:
        seen |= int(v) & 0xFFFF
    assert seen == rd.L4_CHECKED | rd.L4_BAD_CSUM | rd.L4_SHORT


def test_the_traffic_variants_turn_exactly_their_datagrams_bad(inet_oracle):
    """The GPU tests' valid traffic and its one-bit variants (tests/rxd_batch.py), on the model alone."""
    from rxd_batch import VARIANTS
    t = Traffic(inet_oracle)

    def model(frames):
        pl = rr.plan(frames, rr.F_TRAILER)
        arena, _ = rr.build(inet_oracle, frames, pl, np.zeros(int(pl["doff"][-1]), dtype=np.uint8))
        return pl, rd.verdicts(inet_oracle, arena, pl)

    pl, base = model(t.frames)
    m = len(t.groups)
    assert pl["m"] == m == 21 and (base & 0xFFFF == rd.L4_CHECKED).all()
    assert {int(d) & 1 for d in pl["doff"][:m]} == {0, 1} and (pl["dlen"] & 1).all()
    turned = set()
    for which in VARIANTS:
        for sel in (range(0, m, 2), range(1, m, 2)):
            frames, hit = t.bent(which, sel)
            pl2, v = model(frames)
            assert pl2["m"] == m, which
            want = base.copy()
            want[hit] |= rd.L4_BAD_CSUM
            assert np.array_equal(v, want), (which, np.flatnonzero(v != want))
            turned |= {(which, k) for k in hit}
    assert {w for w, _k in turned} == {"front", "line", "tail", "src", "dst"}
    assert len([1 for w, _k in turned if w == "line"]) == m and len([1 for w, _k in turned if w == "src"]) == 14
