"""CPU tests of one-pass TCP segmentation (include/nstack_tso.h): the expected-result model
(tests/tso_model.py: byte surgery per segment, then tests/txd_model.py and tests/txf_model.py) against an
independent big-endian RFC 1071 formulation written here, the eligibility bounds, ip_tx_tso_count and the
host plan (through the stand-alone sanitizer program tests/c/tso_plan_check.cpp) against the model, the
round trip through the validator's model, the ABI, the constants and the argument errors that need no GPU."""
import errno
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import nstack_amd as na
import rxv_model as rv
import tso_model as tm
import txd_model as dm
import txf_model as fm
from tso_batch import tcp_datagram
from txd_batch import l4_datagram

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAC = bytes(range(0x20, 0x2C))
SEG = tm.SEGMENTED | dm.L4_CSUM_SET | 6 << 16
ALL = tm.FIN | tm.PSH | tm.ACK | tm.ECE | tm.CWR


def _header():
    return open(os.path.join(ROOT, "include", "nstack_tso.h")).read()


def rfc1071(data: bytes) -> int:
    """~(one's-complement sum of the big-endian 16-bit words of `data`), RFC 1071."""
    if len(data) & 1:
        data += b"\x00"
    s = sum(struct.unpack(f">{len(data) // 2}H", data))
    while s >> 16:
        s = (s & 0xFFFF) + (s >> 16)
    return ~s & 0xFFFF


def check_segment_frame(frame: bytes, mac: bytes, hlen: int):
    """A built frame (without FCS) holds a TCP segment whose two checksums RFC 791 / 793 accept."""
    assert frame[:12] == mac and frame[12:14] == b"\x08\x00"
    ip_len = struct.unpack_from(">H", frame, 16)[0]
    ip = frame[14:14 + ip_len]
    assert len(frame) == 14 + max(ip_len, 56) and not any(frame[14 + ip_len:])
    assert rfc1071(ip[:hlen]) == 0
    seg = ip[hlen:]
    assert rfc1071(ip[12:20] + bytes([0, 6]) + struct.pack(">H", len(seg)) + seg) == 0
    return ip


@pytest.fixture(scope="module")
def cases():
    """(datagram, mtu, mss, flags): header lengths, odd and tiny units, wraps, every flag."""
    rng = np.random.default_rng(900)
    out = []
    for hlen, thl in ((20, 20), (20, 32), (20, 60), (24, 60), (60, 52), (32, 20)):
        for P, mtu, mss in ((3000, 1500, 0), (1461, 1500, 0), (4381, 1500, 1459), (40, 1500, 7), (33, 1500, 3), (9, 1500, 1),
                            (700, 200, 0), (20000, 9000, 0), (2921, 1500, 1460)):
            if mtu - hlen - thl >= 1:
                out.append((tcp_datagram(rng, hlen, thl, P, ALL), mtu, mss, 0))
    out.append((tcp_datagram(rng, 20, 20, 5000, ALL, id0=0xFFFE, seq0=0xFFFFFFF0), 1500, 0, 0))
    out.append((tcp_datagram(rng, 20, 20, 5000, ALL, id0=0xFFFE, seq0=0xFFFFFFF0), 1500, 0, tm.F_ID_FIXED))
    out.append((tcp_datagram(rng, 20, 20, 65535 - 40, tm.ACK | tm.PSH, foff=0x4000), 1500, 0, 0))
    return out


def test_the_model_builds_what_rfc_793_says(inet_oracle, cases):
    nseg = 0
    for dg, mtu, mss, flags in cases:
        hlen = (dg[0] & 15) * 4
        m, thl = tm.unit(dg, mtu, mss)
        hb = hlen + thl
        st, fr, _ = tm.frames(None, inet_oracle, dg, MAC, mtu, flags, mss)
        assert st == SEG and len(fr) == tm.count(dg, mtu, mss) == -(-(len(dg) - hb) // m) >= 2
        id0, seq0 = struct.unpack_from(">H", dg, 4)[0], struct.unpack_from(">I", dg, hlen + 4)[0]
        pay = b""
        for s, f in enumerate(fr):
            ip = check_segment_frame(f, MAC, hlen)
            assert len(ip) - hb == min(m, len(dg) - hb - s * m) and len(ip) <= mtu
            assert struct.unpack_from(">H", ip, 4)[0] == (id0 if flags & tm.F_ID_FIXED else (id0 + s) & 0xFFFF)
            assert ip[6:8] == dg[6:8]
            assert struct.unpack_from(">I", ip, hlen + 4)[0] == (seq0 + len(pay)) & 0xFFFFFFFF      # contiguous
            want = dg[hlen + 13]
            if s < len(fr) - 1:
                want &= ~(tm.FIN | tm.PSH)
            if s:
                want &= ~tm.CWR
            assert ip[hlen + 13] == want
            # every other header byte is the datagram's
            keep = [q for q in range(hb) if q not in (2, 3, 4, 5, 10, 11, hlen + 4, hlen + 5, hlen + 6, hlen + 7,
                                                       hlen + 13, hlen + 16, hlen + 17)]
            assert all(ip[q] == dg[q] for q in keep)
            pay += ip[hb:]
            nseg += 1
        assert pay == dg[hb:]
    assert nseg > 300


def test_field_garbage_is_ignored(inet_oracle):
    rng = np.random.default_rng(901)
    dg = tcp_datagram(rng, 24, 32, 4000, ALL)
    other = bytearray(dg)
    for q in (10, 11, 24 + 16, 24 + 17):
        other[q] ^= 0xFF
    assert tm.frames(None, inet_oracle, dg, MAC, 1500, 0) == tm.frames(None, inet_oracle, bytes(other), MAC, 1500, 0)


def test_every_eligibility_bound(inet_oracle):
    rng = np.random.default_rng(902)

    def seg(dg, mtu=1500, mss=0):
        st = tm.frames(None, inet_oracle, dg, MAC, mtu, 0, mss)[0]
        assert bool(st & tm.SEGMENTED) == (tm.unit(dg, mtu, mss) is not None) == (tm.count(dg, mtu, mss) > 0)
        if not st & tm.SEGMENTED:   # everything else is txd_model's, word for word
            assert tm.frames(None, inet_oracle, dg, MAC, mtu, 0, mss) == dm.frames(None, inet_oracle, dg, MAC, mtu, 0)
        return bool(st & tm.SEGMENTED)

    assert not seg(tcp_datagram(rng, 20, 16, 3000)) and seg(tcp_datagram(rng, 20, 20, 3000)) and seg(tcp_datagram(rng, 20, 60, 3000))
    assert seg(tcp_datagram(rng, 52, 60, 3000)) and not seg(tcp_datagram(rng, 56, 60, 3000))         # hlen + thl 112 / 116
    assert seg(tcp_datagram(rng, 60, 52, 3000)) and not seg(tcp_datagram(rng, 60, 56, 3000))
    assert not seg(tcp_datagram(rng, 20, 20, 1460)) and seg(tcp_datagram(rng, 20, 20, 1461))         # P = m, m + 1
    assert not seg(tcp_datagram(rng, 20, 20, 100), mss=100) and seg(tcp_datagram(rng, 20, 20, 101), mss=100)
    assert not seg(tcp_datagram(rng, 40, 36, 300), mtu=76) and seg(tcp_datagram(rng, 40, 36, 300), mtu=77)   # cap 0 / 1
    for bit in (tm.SYN, tm.RST, tm.URG):
        assert not seg(tcp_datagram(rng, 20, 20, 3000, tm.ACK | bit))
    assert seg(tcp_datagram(rng, 20, 20, 3000, ALL))
    assert seg(tcp_datagram(rng, 20, 20, 3000, foff=0x4000)) and not seg(tcp_datagram(rng, 20, 20, 3000, foff=0x0001))
    assert not seg(tcp_datagram(rng, 20, 20, 300, foff=0x2000), mss=100)                            # a fragment that fits
    assert not seg(tcp_datagram(rng, 20, 20, 3000, proto=17)) and not seg(l4_datagram(rng, 6, 20, 19), mss=1)
    thl_past_L = bytearray(l4_datagram(rng, 6, 20, 24))
    thl_past_L[20 + 12] = 0x70                                                                       # thl 28 > L 24
    assert not seg(bytes(thl_past_L), mss=1)
    bad = bytearray(tcp_datagram(rng, 20, 20, 3000))
    bad[3] ^= 1
    assert tm.frames(None, inet_oracle, bytes(bad), MAC, 1500, 0)[0] == fm.BAD_LEN
    # DF is honoured by construction: with TXF_F_HONOR_DF a DF datagram is segmented, a SYN one dropped
    df = tcp_datagram(rng, 20, 20, 3000, foff=0x4000)
    assert tm.frames(None, inet_oracle, df, MAC, 1500, fm.F_HONOR_DF)[0] == SEG
    syn = tcp_datagram(rng, 20, 20, 3000, tm.SYN, foff=0x4000)
    assert tm.frames(None, inet_oracle, syn, MAC, 1500, fm.F_HONOR_DF)[0] == fm.DF_DROP | 6 << 16


def test_every_segment_frame_passes_the_validator(oracle, inet_oracle, cases):
    padded = 0
    for dg, mtu, mss, flags in cases[::2]:
        _, fr, crcs = tm.frames(oracle, inet_oracle, dg, MAC, mtu, flags | fm.F_FCS, mss)
        for f, c in zip(fr, crcs):
            v = rv.verdict(oracle, inet_oracle, f, rv.F_TRAILER)
            assert v & rv.L4_CHECKED and not v & (rv.FRAG | rv.L4_BAD_CSUM), hex(v)
            assert v & ~(rv.IPV4 | rv.L4_CHECKED | rv.IP_BAD_LEN | 0xFF << rv.PROTO_SHIFT) == 0 and v >> 16 == 6, hex(v)
            ip_len = struct.unpack_from(">H", f, 16)[0]
            assert bool(v & rv.IP_BAD_LEN) == (ip_len < 56)
            padded += ip_len < 56
            assert f[-4:] == struct.pack("<I", c)
    assert padded > 10


# ---- the count and the host plan against the model ----
def _plan_batch():
    rng = np.random.default_rng(903)
    dgs, mss = [], []
    for q in range(60):
        hlen, thl = (20, 24, 60, 52)[q % 4], (20, 32, 60, 52)[(q // 4) % 4]
        P = int(rng.integers(0, 6000))
        kind = q % 6
        if kind == 0:
            dgs.append(l4_datagram(rng, (17, 1, 6)[q % 3], hlen, int(rng.integers(0, 4000))))
        elif kind == 1:
            dgs.append(tcp_datagram(rng, hlen, thl, P, tm.ACK | (tm.SYN, tm.RST, tm.URG)[q % 3]))
        elif kind == 2:
            dgs.append(tcp_datagram(rng, hlen, thl, P, ALL, foff=(0x2000, 0x4000, 0x0007)[q % 3]))
        else:
            dgs.append(tcp_datagram(rng, hlen, thl, P, ALL))
        mss.append((0, 1, 536, 1460, 9000, 65535)[q % 6] if q % 5 else 0)
    dgs += [b"", b"\x45" * 19, tcp_datagram(rng, 20, 20, 65535 - 40), tcp_datagram(rng, 20, 20, 12000, tm.SYN, foff=0x4000),
            l4_datagram(rng, 6, 24, 13)]
    mss += [0, 7, 3, 0, 1]
    return dgs, mss


def test_count_and_host_plan_against_the_model(inet_oracle, tmp_path):
    cdir = os.path.join(ROOT, "tests", "c")
    subprocess.run(["make", "-s", "-C", cdir, "-f", "tso_plan_check.mk"], check=True)
    r = subprocess.run([os.path.join(cdir, "tso_plan_check")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "tso_plan_check: ok" in r.stdout and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr
    dgs, mss = _plan_batch()
    seen = 0
    for mtu, flags, use in ((1500, 0, "each"), (1500, fm.F_HONOR_DF | dm.F_UDP_ZERO, "one"), (76, 0, "null"), (9000, 0, "each")):
        arr = None if use == "null" else np.array(mss if use == "each" else [536], dtype=np.uint16)
        fl = flags | (tm.F_MSS_ONE if use == "one" else 0)
        path = tmp_path / f"batch_{mtu}_{use}.bin"
        with open(path, "wb") as f:
            f.write(struct.pack("<IIII", len(dgs), mtu, fl, 0 if arr is None else 1))
            for i, dg in enumerate(dgs):
                f.write(struct.pack("<II", len(dg), 0 if arr is None else int(arr[0 if use == "one" else i])) + dg)
        r = subprocess.run([os.path.join(cdir, "tso_plan_check"), str(path)], capture_output=True, text=True)
        assert r.returncode == 0 and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stdout + r.stderr
        lines = r.stdout.split("\n")
        want_st, want_first = tm.plan_status(inet_oracle, dgs, mtu, fl, arr)
        got = np.array([[int(x) for x in ln.split()] for ln in lines[:len(dgs)]], dtype=np.uint64)
        assert (got[:, 0] == want_st).all(), [(i, hex(int(got[i, 0])), hex(int(want_st[i]))) for i in
                                              np.flatnonzero(got[:, 0] != want_st)[:8]]
        assert (got[:, 1] == np.diff(want_first)).all() and lines[len(dgs)] == f"total {int(want_first[-1])}"
        seen |= int(np.bitwise_or.reduce(want_st))
        # ip_tx_tso_count: the same count from the fields alone
        for i, dg in enumerate(dgs):
            if len(dg) < 20 or (dg[0] & 15) * 4 + 14 > len(dg) or dg[9] != 6:
                continue
            hlen = (dg[0] & 15) * 4
            m = 0 if arr is None else int(arr[0 if use == "one" else i])
            c = na.tx_tso_count(len(dg), hlen, (dg[hlen + 12] >> 4) * 4, dg[hlen + 13], struct.unpack_from(">H", dg, 6)[0], m, mtu)
            assert c == tm.count(dg, mtu, m), (i, mtu, m)
    assert seen & 0xFFFF == (tm.SEGMENTED | fm.WHOLE | fm.FRAGMENTED | fm.BAD_HDR | fm.REFRAG | fm.DF_DROP | dm.L4_CSUM_SET |
                             dm.L4_SHORT)
    assert na.tx_tso_count(3000, 20, 20, tm.ACK, 0, 0, 75) == 0 and na.tx_tso_count(65535, 20, 20, tm.ACK, 0, 1, 1500) == 65495


# ---- ABI and constants ----
def test_the_header_declares_exactly_the_listed_and_exported_functions():
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    decl = re.findall(r"\b(\w+)\s*\(", code)
    assert sorted(decl) == sorted(na.TSO_EXPORTS) and len(decl) == 5
    out = subprocess.run(["nm", "-D", "--defined-only", na.LIB_PATH], capture_output=True, text=True, check=True).stdout
    syms = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in decl:
        assert name in syms, name
        assert getattr(na.load(), name).argtypes is not None, name
    others = (set(na.EXPORTS) | set(na.RXV_EXPORTS) | set(na.TXS_EXPORTS) | set(na.TXF_EXPORTS) | set(na.RXR_EXPORTS) |
              set(na.RXD_EXPORTS) | set(na.TXD_EXPORTS))
    assert not set(na.TSO_EXPORTS) & others
    for name in ("tx_tso_count", "tx_tso_plan_dev", "tx_tso_dev", "tx_tso_host", "tso_last_launch"):
        assert callable(getattr(na, name)) and name in na.__all__
    assert na.tso_last_launch() in ("none", "tso", "tso-fcs")
    assert na.txd_last_launch() in ("none", "general-l4", "general-l4-fcs")


def test_constants_agree_between_header_binding_and_model():
    found = dict(re.findall(r"#define\s+(TSO_\w+)\s+(0x[0-9a-fA-F]+|\d+)u?\b", _header()))
    assert sorted(found) == ["TSO_F_ID_FIXED", "TSO_F_MSS_ONE", "TSO_SEGMENTED"]
    for name, val in found.items():
        assert getattr(na, name) == int(val, 0) == getattr(tm, name[4:]), name
    assert (na.TSO_F_ID_FIXED, na.TSO_F_MSS_ONE, na.TSO_SEGMENTED) == (0x200, 0x400, 0x400)
    status_bits = (na.TXF_WHOLE | na.TXF_FRAGMENTED | na.TXF_BAD_HDR | na.TXF_BAD_LEN | na.TXF_REFRAG | na.TXF_DF_DROP |
                   na.TXF_NO_ROOM | na.TXD_L4_CSUM_SET | na.TXD_L4_SHORT | 0xFF << na.TXD_PROTO_SHIFT)
    assert not status_bits & na.TSO_SEGMENTED
    flag_bits = na.TXF_F_FCS | na.TXF_F_HONOR_DF | na.TXF_F_L2_ONE | na.TXD_F_UDP_ZERO
    assert not flag_bits & (na.TSO_F_ID_FIXED | na.TSO_F_MSS_ONE) and na.TSO_F_ID_FIXED != na.TSO_F_MSS_ONE
    assert "#define TSO" not in open(os.path.join(ROOT, "include", "nstack_txd.h")).read()


# ---- argument errors (no GPU needed: they are decided before any device call) ----
def _args(n=2, D=3000):
    rng = np.random.default_rng(904)
    dg = b"".join(tcp_datagram(rng, 20, 20, D - 40) for _ in range(n))
    return dict(dgram=np.frombuffer(dg, dtype=np.uint8).copy(), off=np.arange(n, dtype=np.uint64) * D,
                ln=np.full(n, D, dtype=np.uint32), l2=np.zeros(n, dtype=fm.L2_DTYPE), mss=np.zeros(n, dtype=np.uint16),
                out=np.full(8 * 1600, 0xA5, dtype=np.uint8), first=np.arange(n + 1, dtype=np.uint64) * 3,
                st=np.full(n, 0xDEADBEEF, dtype=np.uint32), flen=np.full(8, 0xDEADBEEF, dtype=np.uint32))


def _host(L, a, mtu, flags, slot, slots=8, null=None, n=2):
    p = lambda k: None if k == null else a[k].ctypes.data
    return L.ip_tx_tso_host(p("dgram"), a["dgram"].size, p("off"), p("ln"), p("l2"), p("mss"), n, mtu, flags, p("out"), slot,
                            slots, p("flen"), p("st"))


def _calls(L, a, mtu, flags, slot, slots=8, null=None, n=2):
    p = lambda k: None if k == null else a[k].ctypes.data
    return (_host(L, a, mtu, flags, slot, slots, null, n),
            L.ip_tx_tso_dev(p("dgram"), a["dgram"].size, p("off"), p("ln"), p("l2"), p("mss"), n, mtu, flags, p("first"),
                            p("out"), slot, slots, p("flen"), p("st"), None, None))


def _plan(L, a, mtu, flags, null=None, n=2):
    p = lambda k: None if k == null else a[k].ctypes.data
    return L.ip_tx_tso_plan_dev(p("dgram"), a["dgram"].size, p("off"), p("ln"), p("mss"), n, mtu, flags, p("st"), p("first"), None)


def _untouched(a):
    return (a["st"] == 0xDEADBEEF).all() and (a["flen"] == 0xDEADBEEF).all() and (a["out"] == 0xA5).all()


def test_argument_errors_are_einval_with_nothing_written():
    L = na.load()
    a = _args()
    E = -errno.EINVAL
    for mtu, flags, slot, word in ((75, 1, 1600, "mtu"), (65536, 1, 70000, "mtu"), (1500, 1, 1517, "slot"),
                                   (1500, 0x700, 1513, "slot"), (76, 1, 93, "slot"), (1500, 8, 1600, "flag"),
                                   (1500, 0x80, 1600, "flag"), (1500, 0x800, 1600, "flag"), (1500, 0x80000701, 1600, "flag")):
        assert _calls(L, a, mtu, flags, slot) == (E, E), (mtu, flags, slot)
        assert word in L.fcs_last_error().decode()
        if word != "slot":
            assert _plan(L, a, mtu, flags) == E
    assert _calls(L, a, 1500, 1, 1 << 63, slots=4) == (E, E)                 # slot * slots overflows
    for null in ("dgram", "off", "ln", "l2", "out"):
        assert _calls(L, a, 1500, 1, 1600, null=null) == (E, E), null
    assert _calls(L, a, 1500, 1, 1600, null="first")[1] == E
    for null in ("dgram", "off", "ln", "first"):
        assert _plan(L, a, 1500, 0, null=null) == E, null
    with pytest.raises(na.FcsError):
        na.tx_tso_host(a["dgram"], a["dgram"].size, a["off"], a["ln"], a["l2"], None, 2, 75, a["out"], 1600, 8)
    # the older calls still refuse the new flag bits
    p = lambda k: a[k].ctypes.data
    for flags in (0x201, 0x401):
        assert L.ip_tx_frame_l4_dev(p("dgram"), a["dgram"].size, p("off"), p("ln"), p("l2"), 2, 1500, flags, p("first"), p("out"),
                                    1600, 8, None, p("st"), None, None) == E
        assert L.ether_tx_frame_plan_dev(p("dgram"), a["dgram"].size, p("off"), p("ln"), 2, 1500, flags, p("st"), p("first"),
                                         None) == E
    # the host form checks the arena and the capacity before any work: two datagrams of three segments
    off2 = a["off"].copy()
    off2[1] = a["dgram"].size - 2999
    assert _host(L, dict(a, off=off2), 1500, 0x701, 1600) == E and "datagram 1 " in L.fcs_last_error().decode()
    assert _host(L, a, 1500, 0x301, 1600, slots=5) == -errno.ENOSPC
    assert _untouched(a)
    assert _host(L, a, 1500, 0x701, 1600, n=0, slots=0) == 0


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
    for flags in (1, 0x701, 0):
        assert _calls(L, a, 1500, flags, 1600) == (-errno.ENODEV, -errno.ENODEV)
        assert _plan(L, a, 1500, flags & ~1) == -errno.ENODEV
    assert _calls(L, a, 1500, 1, 1600, null="mss") == (-errno.ENODEV, -errno.ENODEV)     # mss may be NULL
    assert (L.fcs_engine_host_batches(), L.fcs_engine_host_fallbacks()) == before
    assert _untouched(a)
