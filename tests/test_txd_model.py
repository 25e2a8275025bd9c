"""CPU tests of TX framing with L4 checksums (include/nstack_txd.h): the expected-result model
(tests/txd_model.py: the oracle's checksum functions fill the field, tests/txf_model.py frames the
result) against an independent big-endian RFC 1071 formulation written here, its composition with
the sealer's, the validator's and the reassembly models, the ABI, the constants and the argument
errors that need no GPU."""
import errno
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import nstack_amd as na
import rxd_model as rd
import rxr_model as rr
import rxv_model as rv
import txd_model as dm
import txf_model as fm
import txs_model as sm
from txd_batch import l4_datagram, udp_summing_to_zero

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROTOS, HLENS = (6, 17, 1), (20, 24, 60)
MAC = bytes(range(0x10, 0x1C))


def _header():
    return open(os.path.join(ROOT, "include", "nstack_txd.h")).read()


# ---- an independent statement of the checksums: RFC 1071 on big-endian 16-bit words ----
def rfc1071(data: bytes, start: int = 0) -> int:
    """~(one's-complement sum of the big-endian 16-bit words of `data`). start = 0xffff is the reference's
    quirk (src/ip.c:42, src/tcp.c: the running sum starts at 0xffff, the other zero): the only result
    it changes is that of all-zero data, 0 instead of 0xffff."""
    if len(data) & 1:
        data += b"\x00"
    s = start + sum(struct.unpack(f">{len(data) // 2}H", data))
    while s >> 16:
        s = (s & 0xFFFF) + (s >> 16)
    return ~s & 0xFFFF


def expected_field(dg: bytes, udp_zero=False):
    """The two bytes RFC 793 / 768 / 792 put into the field of an unfragmented datagram, or None."""
    hlen, proto = (dg[0] & 15) * 4, dg[9]
    seg = bytearray(dg[hlen:])
    L = len(seg)
    if proto not in dm.L4_FIELD or L < dm.L4_MIN[proto]:
        return None
    q = dm.L4_FIELD[proto]
    seg[q:q + 2] = b"\x00\x00"
    if proto == 1:
        c = rfc1071(bytes(seg), 0xFFFF)
    elif proto == 17 and udp_zero:
        return b"\x00\x00"
    else:
        c = rfc1071(dg[12:20] + bytes([0, proto]) + struct.pack(">H", L) + bytes(seg), 0xFFFF if proto == 6 else 0)
        if proto == 17 and c == 0:
            c = 0xFFFF
    return struct.pack(">H", c)


@pytest.fixture(scope="module")
def cases(inet_oracle):
    """(datagram, mtu) pairs: three protocols x header lengths 20, 24, 60 x every short bound +- 1 and
    longer segments (odd and even, whole and fragmented), UDP payloads that sum to 0, all-zero ICMP."""
    rng = np.random.default_rng(700)
    out = []
    for p in PROTOS:
        for h in HLENS:
            for L in sorted({0, 1, 3, 4, 5, 7, 8, 9, 19, 20, 21, 37, 100, 1479, 1480}):
                out.append((l4_datagram(rng, p, h, L), 1500))
            for L, mtu in ((57, 76), (200, 76), (1481, 1500), (4001, 1500), (20000, 9000)):
                out.append((l4_datagram(rng, p, h, L), mtu))
    for h in HLENS:
        for n in (2, 3, 1000, 3000):
            out.append((udp_summing_to_zero(inet_oracle, rng, h, n), 1500))
        for L in (4, 5, 64, 1999):
            out.append((l4_datagram(rng, 1, h, L, seg=bytes(L)), 1500))
    return out


def test_the_model_fills_what_rfc_1071_says(inet_oracle, cases):
    short = setw = zero = 0
    for dg, mtu in cases:
        for flags in (0, dm.F_UDP_ZERO):
            filled, bits = dm.fill(inet_oracle, dg, mtu, flags)
            hlen, proto = (dg[0] & 15) * 4, dg[9]
            want = expected_field(dg, bool(flags))
            assert bits >> 16 == proto and len(filled) == len(dg)
            if want is None:
                assert filled == dg and bits & 0xFFFF == dm.L4_SHORT
                short += 1
                continue
            q = hlen + dm.L4_FIELD[proto]
            assert filled[q:q + 2] == want, (proto, hlen, len(dg), flags)
            assert filled[:q] == dg[:q] and filled[q + 2:] == dg[q + 2:]
            assert bits & 0xFFFF == (0 if proto == 17 and flags else dm.L4_CSUM_SET)
            setw += 1
            zero += want == b"\xff\xff" and proto == 17
    assert short == 2 * 3 * (9 + 6 + 3) and setw >= 300 and zero == 12


def test_field_garbage_and_fragment_inputs(inet_oracle):
    rng = np.random.default_rng(701)
    for p in PROTOS:
        for h in HLENS:
            dg = l4_datagram(rng, p, h, 3000)
            q = h + dm.L4_FIELD[p]
            other = dg[:q] + bytes(x ^ 0xFF for x in dg[q:q + 2]) + dg[q + 2:]
            for mtu in (1500, 9000):
                assert dm.fill(inet_oracle, dg, mtu) == dm.fill(inet_oracle, other, mtu)
            # an input that is itself a fragment: framed whole, no L4 work; refused when it does not fit
            for foff in (0x2000, 0x00B9, 0x2001):
                fr = l4_datagram(rng, p, h, 300, foff=foff)
                assert dm.fill(inet_oracle, fr, 1500) == (fr, p << 16)
                assert dm.field_fragment(fr, 1500) is None
                st, out, _ = dm.frames(None, inet_oracle, fr, MAC, 1500, 0)
                assert st == fm.WHOLE | (p << 16) and out == fm.frames(None, inet_oracle, fr, MAC, 1500, 0)[1]
                big = l4_datagram(rng, p, h, 3000, foff=foff)
                assert dm.frames(None, inet_oracle, big, MAC, 1500, 0)[0] == fm.REFRAG | (p << 16)
    # rules 1 and 2 refuse: no protocol bits
    bad = bytearray(l4_datagram(rng, 6, 20, 100))
    bad[3] ^= 1
    assert dm.frames(None, inet_oracle, bytes(bad), MAC, 1500, 0)[0] == fm.BAD_LEN
    assert dm.frames(None, inet_oracle, b"\x45" + bytes(18), MAC, 1500, 0)[0] == fm.BAD_HDR


def test_the_field_lies_in_fragment_fo_over_max(inet_oracle):
    rng = np.random.default_rng(702)
    for h, q in ((20, 0), (52, 1), (60, 2)):
        dg = l4_datagram(rng, 6, h, 500)
        assert dm.field_fragment(dg, 76) == q == 16 // fm.frag_unit(76, h)
        filled, _ = dm.fill(inet_oracle, dg, 76)
        _, fr, _ = dm.frames(None, inet_oracle, dg, MAC, 76, 0)
        _, plain, _ = fm.frames(None, inet_oracle, dg, MAC, 76, 0)
        differ = [j for j in range(len(fr)) if fr[j] != plain[j]]
        assert differ in ([q], []) and filled[h + 16:h + 18] == fr[q][14 + h + 16 - q * fm.frag_unit(76, h):][:2]
        for p in (17, 1):
            assert dm.field_fragment(l4_datagram(rng, p, h, 500), 76) == 0


# ---- composition with the other models ----
def test_whole_frames_equal_framing_then_sealing(oracle, inet_oracle, cases):
    n = 0
    for dg, mtu in cases:
        if len(dg) > mtu:
            continue
        for flags, sflags in ((fm.F_FCS, sm.F_FCS), (fm.F_FCS | dm.F_UDP_ZERO, sm.F_FCS | sm.F_UDP_ZERO), (0, 0)):
            st, fr, _ = dm.frames(oracle, inet_oracle, dg, MAC, mtu, flags)
            _, plain, _ = fm.frames(oracle, inet_oracle, dg, MAC, mtu, flags & dm.TXF_FLAGS)
            T = 4 if flags & fm.F_FCS else 0
            sealed, sst, _ = sm.seal(oracle, inet_oracle, plain[0][:len(plain[0]) - T], sflags)
            assert fr == [sealed], (len(dg), dg[9], flags)
            assert st & (dm.L4_CSUM_SET | dm.L4_SHORT) == sst & (sm.L4_CSUM_SET | sm.L4_SHORT) and st >> 16 == sst >> 16
            n += 1
    assert n > 400


def test_model_frames_pass_the_validator_and_the_reassembled_datagram_its_check(oracle, inet_oracle, cases):
    frames, want = [], []
    for q, (dg, mtu) in enumerate(cases):
        dg = dg[:4] + (0x2000 + q).to_bytes(2, "big") + dg[6:]          # distinct ids
        st, fr, _ = dm.frames(oracle, inet_oracle, dg, MAC, mtu, fm.F_FCS)
        for f in fr:
            v = rv.verdict(oracle, inet_oracle, f, rv.F_TRAILER)
            assert v & ~(rv.IPV4 | rv.FRAG | rv.IP_BAD_LEN | rv.L4_CHECKED | rv.L4_SHORT | (0xFF << rv.PROTO_SHIFT)) == 0, hex(v)
            assert bool(v & rv.L4_SHORT) <= bool(st & dm.L4_SHORT)
        frames += fr
        want.append((dm.fill(inet_oracle, dg, mtu)[0], st))
    pl = rr.plan(frames, rr.F_TRAILER)
    assert pl["m"] == len(cases)
    need = int(pl["doff"][pl["m"]])
    out, _ = rr.build(inet_oracle, frames, pl, np.zeros(need, dtype=np.uint8))
    for k, dg in enumerate(rr.datagrams(out, pl)):
        filled, st = want[k]
        assert bytes(dg)[12:] == filled[12:] and len(dg) == len(filled)
        v = rd.verdict(inet_oracle, bytes(dg))
        if st & dm.L4_SHORT:
            assert v & rd.L4_SHORT
        else:
            assert v & rd.L4_CHECKED and not v & rd.L4_BAD_CSUM, (k, hex(v))


# ---- ABI and constants ----
def test_the_header_declares_exactly_the_listed_and_exported_functions():
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    decl = re.findall(r"\b(\w+)\s*\(", code)
    assert sorted(decl) == sorted(na.TXD_EXPORTS) and len(decl) == 3
    out = subprocess.run(["nm", "-D", "--defined-only", na.LIB_PATH], capture_output=True, text=True, check=True).stdout
    syms = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in decl:
        assert name in syms, name
        assert getattr(na.load(), name).argtypes is not None, name
    others = (set(na.EXPORTS) | set(na.RXV_EXPORTS) | set(na.TXS_EXPORTS) | set(na.TXF_EXPORTS) | set(na.RXR_EXPORTS) |
              set(na.RXD_EXPORTS))
    assert not set(na.TXD_EXPORTS) & others
    for name in ("tx_frame_l4_dev", "tx_frame_l4_host", "txd_last_launch"):
        assert callable(getattr(na, name)) and name in na.__all__
    assert na.txd_last_launch() in ("none", "general-l4", "general-l4-fcs")


def test_constants_agree_between_header_binding_and_model():
    found = dict(re.findall(r"#define\s+(TXD_\w+)\s+(0x[0-9a-fA-F]+|\d+)u?\b", _header()))
    assert sorted(found) == ["TXD_F_UDP_ZERO", "TXD_L4_CSUM_SET", "TXD_L4_SHORT", "TXD_PROTO_SHIFT"]
    for name, val in found.items():
        assert getattr(na, name) == int(val, 0) == getattr(dm, name[4:]), name
    assert (na.TXD_L4_CSUM_SET, na.TXD_L4_SHORT, na.TXD_PROTO_SHIFT) == (na.TXS_L4_CSUM_SET, na.TXS_L4_SHORT, na.TXS_PROTO_SHIFT)
    txf_bits = (na.TXF_WHOLE | na.TXF_FRAGMENTED | na.TXF_BAD_HDR | na.TXF_BAD_LEN | na.TXF_REFRAG | na.TXF_DF_DROP |
                na.TXF_NO_ROOM)
    assert not txf_bits & (na.TXD_L4_CSUM_SET | na.TXD_L4_SHORT | (0xFF << na.TXD_PROTO_SHIFT))
    assert not na.TXD_F_UDP_ZERO & (na.TXF_F_FCS | na.TXF_F_HONOR_DF | na.TXF_F_L2_ONE) and na.TXD_F_UDP_ZERO > 8
    assert "nstack_txd.h" in open(os.path.join(ROOT, "include", "nstack_txf.h")).read()


# ---- argument errors (no GPU needed: they are decided before any device call) ----
def _args(n=2, D=100):
    dg = bytearray()
    for _ in range(n):
        dg += struct.pack(">BBHHHBBHII", 0x45, 0, D, 1, 0, 64, 17, 0, 1, 2) + bytes(D - 20)
    a = dict(dgram=np.frombuffer(bytes(dg), dtype=np.uint8).copy(), off=np.arange(n, dtype=np.uint64) * D,
             ln=np.full(n, D, dtype=np.uint32), l2=np.zeros(n, dtype=fm.L2_DTYPE), out=np.full(n * 1600, 0xA5, dtype=np.uint8),
             first=np.arange(n + 1, dtype=np.uint64), st=np.full(n, 0xDEADBEEF, dtype=np.uint32),
             flen=np.full(n, 0xDEADBEEF, dtype=np.uint32))
    return a


def _host(L, a, mtu, flags, slot, slots=2, null=None, n=2):
    p = lambda k: None if k == null else a[k].ctypes.data
    return L.ip_tx_frame_l4_host(p("dgram"), a["dgram"].size, p("off"), p("ln"), p("l2"), n, mtu, flags, p("out"), slot,
                                 slots, p("flen"), p("st"))


def _calls(L, a, mtu, flags, slot, slots=2, null=None, n=2):
    p = lambda k: None if k == null else a[k].ctypes.data
    return (_host(L, a, mtu, flags, slot, slots, null, n),
            L.ip_tx_frame_l4_dev(p("dgram"), a["dgram"].size, p("off"), p("ln"), p("l2"), n, mtu, flags, p("first"), p("out"),
                                 slot, slots, p("flen"), p("st"), None, None))


def _untouched(a):
    return (a["st"] == 0xDEADBEEF).all() and (a["flen"] == 0xDEADBEEF).all() and (a["out"] == 0xA5).all()


def test_argument_errors_are_einval_with_nothing_written():
    L = na.load()
    a = _args()
    E = -errno.EINVAL
    for mtu, flags, slot, word in ((75, 1, 1600, "mtu"), (65536, 1, 70000, "mtu"), (1500, 1, 1517, "slot"),
                                   (1500, 0x100, 1513, "slot"), (76, 1, 93, "slot"), (1500, 8, 1600, "flag"),
                                   (1500, 0x80, 1600, "flag"), (1500, 0x200, 1600, "flag"), (1500, 0x80000101, 1600, "flag")):
        assert _calls(L, a, mtu, flags, slot) == (E, E), (mtu, flags, slot)
        assert word in L.fcs_last_error().decode()
    assert _calls(L, a, 1500, 1, 1 << 63, slots=4) == (E, E)                 # slot * slots overflows
    for null in ("dgram", "off", "ln", "l2", "out"):
        assert _calls(L, a, 1500, 1, 1600, null=null) == (E, E), null
    assert _calls(L, a, 1500, 1, 1600, null="first")[1] == E
    with pytest.raises(na.FcsError):
        na.tx_frame_l4_host(a["dgram"], a["dgram"].size, a["off"], a["ln"], a["l2"], 2, 75, a["out"], 1600, 2)
    # the plain framer still refuses the new flag bit
    p = lambda k: a[k].ctypes.data
    assert L.ether_tx_frame_dev(p("dgram"), a["dgram"].size, p("off"), p("ln"), p("l2"), 2, 1500, 0x101, p("first"), p("out"),
                                1600, 2, None, p("st"), None, None) == E
    # the host form checks the arena and the capacity before any work
    off2 = a["off"].copy()
    off2[1] = a["dgram"].size - 99
    b = dict(a, off=off2)
    assert _host(L, b, 1500, 0x101, 1600) == E and "datagram 1 " in L.fcs_last_error().decode()
    assert _host(L, a, 1500, 0x101, 1600, slots=1) == -errno.ENOSPC
    assert _untouched(a)
    assert _host(L, a, 1500, 0x101, 1600, n=0, slots=0) == 0


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
    for flags in (1, 0x101, 0):
        assert _calls(L, a, 1500, flags, 1600) == (-errno.ENODEV, -errno.ENODEV)
    assert (L.fcs_engine_host_batches(), L.fcs_engine_host_fallbacks()) == before
    assert _untouched(a)
