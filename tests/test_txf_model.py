"""CPU tests of one-pass TX framing (include/nstack_txf.h): the expected-result model
(tests/txf_model.py: the header's rules with the oracle's arithmetic) against the independently
generated golden vectors (tests/golden/make_txf_golden.py), the frame-count arithmetic, reassembly,
the round trip through the validator's model, the ABI, the argument errors that need no GPU, and the
stand-alone sanitizer check of the host planning header (tests/c/txf_plan_check.cpp)."""
import errno
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import nstack_amd as na
import rxv_model as rm
import txf_model as fm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def txf_golden():
    return fm.load_golden()


@pytest.fixture(scope="module")
def modelled(oracle, inet_oracle, txf_golden):
    """The model's frames of every golden datagram, computed once: tag -> (record, status, frames)."""
    a = txf_golden["input_bytes"]
    out = {}
    for r in txf_golden["datagrams"]:
        dg = a[r["off"]:r["off"] + r["len"]]
        st, fr, _ = fm.frames(oracle, inet_oracle, dg, bytes.fromhex(r["mac"]), r["mtu"], r["flags"] | fm.F_FCS)
        out[r["tag"]] = (r, st, fr)
    return out


def test_model_matches_golden(txf_golden, modelled):
    assert len(txf_golden["datagrams"]) >= 300
    bad = []
    for tag, (r, st, fr) in modelled.items():
        want, at = txf_golden["frame_bytes"][r["mtu"]], r["at"]
        if st != r["status"] or [len(f) - 4 for f in fr] != r["flen"]:
            bad.append((tag, hex(st), hex(r["status"]), len(fr), len(r["flen"])))
            continue
        for f in fr:
            if f != want[at:at + len(f)]:
                bad.append((tag, at))
                break
            at += len(f)
    assert not bad, bad[:10]


def test_golden_covers_what_the_issue_lists(txf_golden):
    recs = txf_golden["datagrams"]
    seen = 0
    for r in recs:
        seen |= r["status"]
    for bit in (fm.WHOLE, fm.FRAGMENTED, fm.BAD_HDR, fm.BAD_LEN, fm.REFRAG, fm.DF_DROP):
        assert seen & bit, hex(bit)
    a = txf_golden["input_bytes"]
    made = [r for r in recs if r["flen"]]
    assert {(a[r["off"]] & 15) * 4 for r in made} == set(range(20, 64, 4))
    assert {r["mtu"] for r in made} == {76, 100, 576, 1500, 9000}
    assert {r["off"] & 3 for r in made} == {0, 1, 2, 3}
    by = {r["tag"]: r for r in recs}
    # 65475 payload bytes in units of 8: 8184 frames of 82 bytes and a last one with 3 payload bytes
    assert by["max_m76_h60"]["flen"] == [82] * 8184 + [77] and by["max_m76_h60"]["len"] == 65535
    assert len(by["max_m1500_h20"]["flen"]) == 45 and by["max_m1500_h20"]["flen"][0] == 1506
    # last fragments of 1..8 payload bytes: 70-byte frames whose IP bytes end before byte 70
    for mtu in (76, 100, 576, 1500, 9000):
        for t in range(1, 9):
            r = by[f"m{mtu}_h20_tail{t}"]
            assert r["flen"][-1] == 70 and len(r["flen"]) >= 2, r["tag"]
    assert by["m1500_h20_D1501"]["status"] == fm.FRAGMENTED and by["m1500_h20_D1500"]["status"] == fm.WHOLE


def test_frame_count_equals_the_model():
    for mtu in (76, 77, 83, 84, 576, 1500, 9000, 65535):
        for hlen in range(20, 64, 4):
            mx = fm.frag_unit(mtu, hlen)
            assert mx >= 8 and mx % 8 == 0
            ds = {20, hlen, mtu - 1, mtu, mtu + 1, 65535}
            for k in range(0, 5):
                ds |= {hlen + k * mx + e for e in (-1, 0, 1)}
            for D in sorted(d for d in ds if hlen <= d <= 65535):
                dg = struct.pack(">BBHHH", 0x40 | hlen // 4, 0, D, 0, 0) + bytes(D - 8)
                _, cnt, _, _ = fm.plan(dg, mtu)
                assert na.tx_frame_count(D, hlen, mtu) == cnt, (D, hlen, mtu)
                assert cnt <= 8185
    assert na.tx_frame_count(65535, 60, 76) == 8185
    for D, hlen, mtu in ((19, 20, 1500), (40, 16, 1500), (40, 44, 1500), (100, 20, 75), (100, 20, 65536), (100, 64, 1500)):
        assert na.tx_frame_count(D, hlen, mtu) == 0, (D, hlen, mtu)


def test_reassembly_gives_back_the_payload(txf_golden, modelled):
    a = txf_golden["input_bytes"]
    frag = 0
    for tag, (r, st, fr) in modelled.items():
        if not fr:
            continue
        dg = a[r["off"]:r["off"] + r["len"]]
        hlen = (dg[0] & 15) * 4
        got = bytearray(len(dg) - hlen)
        mf = []
        for f in fr:
            ip_len, _id, foff = struct.unpack_from(">HHH", f, 16)
            assert f[14:16] == dg[0:2] and f[26:14 + hlen] == dg[12:hlen], tag   # the header but for three fields
            at = (foff & 0x1FFF) * 8 if st & fm.FRAGMENTED else 0
            got[at:at + ip_len - hlen] = f[14 + hlen:14 + ip_len]
            mf.append(bool(foff & 0x2000))
            if st & fm.FRAGMENTED:
                assert not foff & 0xC000, tag
            else:
                assert f[20:22] == dg[6:8], tag
        assert bytes(got) == dg[hlen:], tag
        if st & fm.FRAGMENTED:
            assert mf == [True] * (len(fr) - 1) + [False], tag
            frag += 1
    assert frag > 100


def test_model_frames_pass_the_validator_model(oracle, inet_oracle, modelled):
    checked = padded = 0
    for tag, (r, st, fr) in modelled.items():
        for q, f in enumerate(fr):
            v = rm.verdict(oracle, inet_oracle, f, rm.F_TRAILER)
            I = int.from_bytes(f[16:18], "big")
            foff = int.from_bytes(f[20:22], "big")
            want = rm.IPV4 | (f[23] << rm.PROTO_SHIFT)
            if foff & 0x3FFF:
                want |= rm.FRAG
            if I < 56:
                want |= rm.IP_BAD_LEN
                padded += 1
            # defect bits: none but RXV_FRAG on fragments and RXV_IP_BAD_LEN exactly on padded frames
            assert v == want, (tag, q, hex(v), hex(want))
            checked += 1
    assert checked > 9000 and padded > 50


def test_model_constants_match_the_binding_and_the_header():
    for name in ("F_FCS", "F_HONOR_DF", "F_L2_ONE", "WHOLE", "FRAGMENTED", "BAD_HDR", "BAD_LEN", "REFRAG", "DF_DROP",
                 "NO_ROOM"):
        assert getattr(fm, name) == getattr(na, "TXF_" + name), name
    hdr = open(os.path.join(ROOT, "include", "nstack_txf.h")).read()
    found = re.findall(r"#define\s+(TXF_\w+)\s+(0x[0-9a-fA-F]+|\d+)u?", hdr)
    assert len(found) == 10
    for name, val in found:
        assert getattr(na, name) == int(val, 0), name
    assert np.dtype(na.TXF_L2_DTYPE) == fm.L2_DTYPE and fm.L2_DTYPE.itemsize == 12


# ---- ABI ----
def _declared():
    hdr = open(os.path.join(ROOT, "include", "nstack_txf.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return re.findall(r"\b((?:ether_tx_frame|fcs_debug_txf_)\w*)\s*\(", hdr)


def test_every_declared_function_is_exported_and_listed():
    decl = _declared()
    assert sorted(decl) == sorted(na.TXF_EXPORTS) and len(decl) == 5
    out = subprocess.run(["nm", "-D", "--defined-only", na.LIB_PATH], capture_output=True, text=True, check=True).stdout
    syms = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in decl:
        assert name in syms, name
        assert getattr(na.load(), name).argtypes is not None, name
    assert not set(na.TXF_EXPORTS) & (set(na.EXPORTS) | set(na.RXV_EXPORTS) | set(na.TXS_EXPORTS))


# ---- argument errors (no GPU needed: they are decided before any device call) ----
def _args(n=2, D=100):
    dg = bytearray()
    for _ in range(n):
        dg += struct.pack(">BBHHHBBHII", 0x45, 0, D, 1, 0, 64, 17, 0, 1, 2) + bytes(D - 20)
    dgram = np.frombuffer(bytes(dg), dtype=np.uint8).copy()
    off = np.arange(n, dtype=np.uint64) * D
    ln = np.full(n, D, dtype=np.uint32)
    l2 = np.zeros(n, dtype=fm.L2_DTYPE)
    out = np.full(n * 1600, 0xA5, dtype=np.uint8)
    first = np.arange(n + 1, dtype=np.uint64)
    st = np.full(n, 0xDEADBEEF, dtype=np.uint32)
    return dgram, off, ln, l2, out, first, st


def _calls(L, a, mtu, flags, slot, slots=2):
    dgram, off, ln, l2, out, first, st = a
    p = lambda x: x.ctypes.data
    return (L.ether_tx_frame_host(p(dgram), dgram.size, p(off), p(ln), p(l2), 2, mtu, flags, p(out), slot, slots, None,
                                  p(st)),
            L.ether_tx_frame_dev(p(dgram), dgram.size, p(off), p(ln), p(l2), 2, mtu, flags, p(first), p(out), slot,
                                 slots, None, p(st), None, None))


def test_bad_mtu_slot_and_flags_are_einval():
    L = na.load()
    a = _args()
    for mtu, flags, slot, word in ((75, 1, 1600, "mtu"), (65536, 1, 70000, "mtu"), (1500, 1, 1517, "slot"),
                                   (1500, 0, 1513, "slot"), (76, 1, 93, "slot"), (1500, 8, 1600, "flag"),
                                   (1500, 0x80000001, 1600, "flag")):
        assert _calls(L, a, mtu, flags, slot) == (-errno.EINVAL, -errno.EINVAL), (mtu, flags, slot)
        assert word in L.fcs_last_error().decode()
        if word != "slot":
            dgram, off, ln = a[0], a[1], a[2]
            assert L.ether_tx_frame_plan_dev(dgram.ctypes.data, dgram.size, off.ctypes.data, ln.ctypes.data, 2, mtu,
                                             flags, a[6].ctypes.data, a[5].ctypes.data, None) == -errno.EINVAL
    with pytest.raises(na.FcsError):
        na.tx_frame_host(a[0], a[0].size, a[1], a[2], a[3], 2, 75, a[4], 1600, 2)
    assert (a[6] == 0xDEADBEEF).all() and (a[4] == 0xA5).all()


def test_host_form_checks_the_arena_and_the_capacity_before_any_work():
    L = na.load()
    a = _args()
    dgram, off, ln, l2, out, first, st = a
    p = lambda x: x.ctypes.data
    off2 = off.copy()
    off2[1] = dgram.size - 99          # datagram 1 ends one byte past the arena
    assert L.ether_tx_frame_host(p(dgram), dgram.size, p(off2), p(ln), p(l2), 2, 1500, 1, p(out), 1600, 2, None,
                                 p(st)) == -errno.EINVAL
    assert "datagram 1 " in L.fcs_last_error().decode()
    off2[1] = 2**64 - 50               # off + len wraps
    assert L.ether_tx_frame_host(p(dgram), dgram.size, p(off2), p(ln), p(l2), 2, 1500, 1, p(out), 1600, 2, None,
                                 p(st)) == -errno.EINVAL
    assert "datagram 1 " in L.fcs_last_error().decode()
    # two frames into one slot: -ENOSPC; at mtu 76 the two datagrams are 2 x 2 frames
    assert L.ether_tx_frame_host(p(dgram), dgram.size, p(off), p(ln), p(l2), 2, 1500, 1, p(out), 1600, 1, None,
                                 p(st)) == -errno.ENOSPC
    assert L.ether_tx_frame_host(p(dgram), dgram.size, p(off), p(ln), p(l2), 2, 76, 1, p(out), 94, 3, None,
                                 p(st)) == -errno.ENOSPC
    assert (st == 0xDEADBEEF).all() and (out == 0xA5).all()   # nothing written
    assert L.ether_tx_frame_host(p(dgram), dgram.size, p(off), p(ln), p(l2), 0, 1500, 1, p(out), 1600, 0, None, None) == 0


def test_host_form_refuses_a_datagram_larger_than_a_chunk_before_any_work():
    """65535 bytes with a 60-byte header at mtu 76 are 8185 frames; in slots of 16 KiB they are more
    than the 64 MiB of slots one chunk of the host pipeline holds."""
    L = na.load()
    D, slot, slots = 65535, 16384, 8185
    small = struct.pack(">BBHHHBBHII", 0x45, 0, 40, 1, 0, 64, 17, 0, 1, 2) + bytes(20)
    big = struct.pack(">BBHHHBBHII", 0x4F, 0, D, 1, 0, 64, 17, 0, 1, 2) + bytes(D - 20)
    assert na.tx_frame_count(D, 60, 76) == slots and slots * slot > 64 << 20 > (slots // 2) * slot
    dgram = np.frombuffer(small + big, dtype=np.uint8).copy()
    off = np.array([0, 40], dtype=np.uint64)
    ln = np.array([40, D], dtype=np.uint32)
    l2 = np.zeros(2, dtype=fm.L2_DTYPE)
    out = np.full((slots + 1) * slot, 0xA5, dtype=np.uint8)
    flen = np.full(slots + 1, 0xCCCCCCCC, dtype=np.uint32)
    st = np.full(2, 0xDEADBEEF, dtype=np.uint32)
    p = lambda x: x.ctypes.data
    assert L.ether_tx_frame_host(p(dgram), dgram.size, p(off), p(ln), p(l2), 2, 76, 1, p(out), slot, slots + 1, p(flen),
                                 p(st)) == -errno.EINVAL
    msg = L.fcs_last_error().decode()
    assert "datagram 1:" in msg and "8185 slots" in msg and "host chunk" in msg
    assert (out == 0xA5).all() and (flen == 0xCCCCCCCC).all() and (st == 0xDEADBEEF).all()


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
    dgram, off, ln = a[0], a[1], a[2]
    before = (L.fcs_engine_host_batches(), L.fcs_engine_host_fallbacks())
    assert _calls(L, a, 1500, 1, 1600) == (-errno.ENODEV, -errno.ENODEV)
    assert L.ether_tx_frame_plan_dev(dgram.ctypes.data, dgram.size, off.ctypes.data, ln.ctypes.data, 2, 1500, 0,
                                     a[6].ctypes.data, a[5].ctypes.data, None) == -errno.ENODEV
    assert (L.fcs_engine_host_batches(), L.fcs_engine_host_fallbacks()) == before
    assert (a[6] == 0xDEADBEEF).all() and (a[4] == 0xA5).all()
    assert na.tx_frame_count(100, 20, 1500) == 1               # the arithmetic needs no GPU


# ---- the host planning header under the sanitizers (a stand-alone program: nothing is loaded into Python) ----
def test_plan_header_check_runs_clean_under_asan_and_ubsan():
    cdir = os.path.join(ROOT, "tests", "c")
    subprocess.run(["make", "-s", "-C", cdir, "-f", "txf_plan_check.mk"], check=True)
    r = subprocess.run([os.path.join(cdir, "txf_plan_check")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "txf_plan_check: ok" in r.stdout and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr
