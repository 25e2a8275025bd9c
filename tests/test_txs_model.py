"""CPU tests of one-pass TX sealing (include/nstack_txs.h): the expected-result model
(tests/txs_model.py: the header's rules with the oracle's arithmetic) against the independently
generated golden vectors (tests/golden/make_txs_golden.py), the round trip through the validator's
model, the ABI, and the argument errors and routing arithmetic that need no GPU."""
import errno
import json
import os
import re
import subprocess

import numpy as np
import pytest

import nstack_amd as na
import rxv_model as rm
import txs_model as tm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def txs_golden():
    with open(os.path.join(GOLDEN, "txs_vectors.json")) as f:
        vec = json.load(f)
    with open(os.path.join(GOLDEN, vec["input"]), "rb") as f:
        vec["input_bytes"] = f.read()
    vec["sealed_bytes"] = []
    for name in vec["sealed"]:
        with open(os.path.join(GOLDEN, name), "rb") as f:
            vec["sealed_bytes"].append(f.read())
    return vec


def test_model_matches_golden(oracle, inet_oracle, txs_golden):
    a = txs_golden["input_bytes"]
    assert len(txs_golden["frames"]) >= 300
    for flags in range(4):
        want = txs_golden["sealed_bytes"][flags]
        bad = []
        for r in txs_golden["frames"]:
            o, l = r["off"], r["len"]
            out, st, fl = tm.seal(oracle, inet_oracle, a[o:o + l], flags)
            if out != want[o:o + len(out)] or st != r["status"][flags] or list(fl) != r["fields"][flags]:
                bad.append((r["tag"], l, hex(st), hex(r["status"][flags]), fl, r["fields"][flags]))
        assert not bad, (flags, bad[:10])
        # the whole arena: nothing but the fields and the FCS places differs from the input
        arena = np.frombuffer(a, dtype=np.uint8)
        off = [r["off"] for r in txs_golden["frames"]]
        ln = [r["len"] for r in txs_golden["frames"]]
        out, _, _ = tm.seal_arena(oracle, inet_oracle, arena, off, ln, flags)
        assert out.tobytes() == want


def test_golden_covers_every_bit_and_garbage_fields(txs_golden):
    seen = 0
    for r in txs_golden["frames"]:
        seen |= r["status"][tm.F_FCS]
    for bit in (tm.FCS_SET, tm.RUNT, tm.IPV4, tm.IP_BAD_HDR, tm.IP_BAD_LEN, tm.IP_CSUM_SET, tm.FRAG, tm.L4_CSUM_SET,
                tm.L4_SHORT):
        assert seen & bit, hex(bit)
    protos = {(r["status"][0] >> 16) & 0xFF for r in txs_golden["frames"] if r["status"][0] & tm.L4_CSUM_SET}
    assert protos == {1, 6, 17}
    by = {r["tag"]: r for r in txs_golden["frames"]}
    assert by["udp_sums_to_zero"]["fields"][0][1] == 0xFFFF          # a computed 0 goes out as all ones
    assert by["udp_sums_to_zero"]["fields"][tm.F_UDP_ZERO][1] == 0
    assert not by["udp_sums_to_zero"]["status"][tm.F_UDP_ZERO] & tm.L4_CSUM_SET
    # the input's fields are garbage: sealing changes nearly all of them
    a, s = txs_golden["input_bytes"], txs_golden["sealed_bytes"][0]
    changed = sum(1 for r in txs_golden["frames"]
                  if r["status"][0] & tm.IP_CSUM_SET and a[r["off"] + 24:r["off"] + 26] != s[r["off"] + 24:r["off"] + 26])
    assert changed > 300


def test_sealed_golden_frames_pass_the_validator_model(oracle, inet_oracle, txs_golden):
    """Round trip: sealed frames (F + 4 bytes) get clean verdicts from tests/rxv_model.py."""
    s = txs_golden["sealed_bytes"][tm.F_FCS]
    checked = 0
    for r in txs_golden["frames"]:
        o, l, st = r["off"], r["len"], r["status"][tm.F_FCS]
        v = rm.verdict(oracle, inet_oracle, s[o:o + l + 4], rm.F_TRAILER)
        assert not v & (rm.FCS_BAD | rm.IP_BAD_CSUM | rm.L4_BAD_CSUM), (r["tag"], hex(v))
        assert bool(v & rm.RUNT) == bool(st & tm.RUNT) and bool(v & rm.IPV4) == bool(st & tm.IPV4), r["tag"]
        assert bool(v & rm.IP_BAD_HDR) == bool(st & tm.IP_BAD_HDR), r["tag"]
        if st & tm.L4_CSUM_SET:
            assert v & rm.L4_CHECKED, r["tag"]
            checked += 1
        if st & tm.IP_CSUM_SET and not st & tm.IP_BAD_LEN:
            ip_len = int.from_bytes(s[o + 16:o + 18], "big")
            assert bool(v & rm.IP_BAD_LEN) == (ip_len != l - 14), r["tag"]   # exactly the padded frames
    assert checked > 300


def test_model_constants_match_the_binding_and_the_header():
    for name in ("F_FCS", "F_UDP_ZERO", "FCS_SET", "RUNT", "IPV4", "IP_BAD_HDR", "IP_BAD_LEN", "IP_CSUM_SET", "FRAG",
                 "L4_CSUM_SET", "L4_SHORT", "PROTO_SHIFT"):
        assert getattr(tm, name) == getattr(na, "TXS_" + name), name
    hdr = open(os.path.join(ROOT, "include", "nstack_txs.h")).read()
    found = re.findall(r"#define\s+(TXS_\w+)\s+(0x[0-9a-fA-F]+|\d+)u?", hdr)
    assert len(found) == 12
    for name, val in found:
        assert getattr(na, name) == int(val, 0), name
    assert np.dtype(na.TXS_FIELDS_DTYPE) == tm.FIELDS_DTYPE and tm.FIELDS_DTYPE.itemsize == 8


# ---- ABI ----
def _declared():
    hdr = open(os.path.join(ROOT, "include", "nstack_txs.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return re.findall(r"\b((?:ether_tx_seal|fcs_debug_txs_)\w*)\s*\(", hdr)


def test_every_declared_function_is_exported_and_listed():
    decl = _declared()
    assert sorted(decl) == sorted(na.TXS_EXPORTS) and len(decl) == 6
    out = subprocess.run(["nm", "-D", "--defined-only", na.LIB_PATH], capture_output=True, text=True, check=True).stdout
    syms = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in decl:
        assert name in syms, name
        assert getattr(na.load(), name).argtypes is not None, name
    assert not set(na.TXS_EXPORTS) & (set(na.EXPORTS) | set(na.RXV_EXPORTS))


# ---- argument errors (no GPU needed: they are decided before any device call) ----
def _args(n=2, length=64, gap=4):
    arena = np.full(n * (length + gap), 0xA5, dtype=np.uint8)
    off = np.arange(n, dtype=np.uint64) * (length + gap)
    ln = np.full(n, length, dtype=np.uint32)
    status = np.full(n, 0xDEADBEEF, dtype=np.uint32)
    return arena, off, ln, status


def test_unknown_flag_bits_are_einval():
    L = na.load()
    arena, off, ln, st = _args()
    for flags in (4, 0x80000000, 7):
        assert L.ether_tx_seal_host(arena.ctypes.data, arena.size, off.ctypes.data, ln.ctypes.data, flags, 0,
                                    st.ctypes.data, 2) == -errno.EINVAL
        assert L.ether_tx_seal_dev(arena.ctypes.data, arena.size, off.ctypes.data, ln.ctypes.data, flags, 0,
                                   st.ctypes.data, None, None, 2, None) == -errno.EINVAL
        assert L.ether_tx_seal_fixed_dev(arena.ctypes.data, 68, 64, 2, flags, 0, st.ctypes.data, None, None,
                                         None) == -errno.EINVAL
        with pytest.raises(na.FcsError):
            na.tx_seal_host(arena, arena.size, off, ln, 2, flags=flags, status=st)
    assert "flag" in L.fcs_last_error().decode()
    assert (st == 0xDEADBEEF).all() and (arena == 0xA5).all()


def test_fixed_stride_must_hold_the_frame_and_its_fcs_place():
    L = na.load()
    arena, _, _, st = _args()
    for stride, flags in ((32, 0), (63, 0), (64, na.TXS_F_FCS), (67, na.TXS_F_FCS), (67, na.TXS_F_FCS | na.TXS_F_UDP_ZERO)):
        assert L.ether_tx_seal_fixed_dev(arena.ctypes.data, stride, 64, 2, flags, 0, st.ctypes.data, None, None,
                                         None) == -errno.EINVAL, (stride, flags)
        assert "stride" in L.fcs_last_error().decode()
    assert (st == 0xDEADBEEF).all() and (arena == 0xA5).all()


def test_host_form_names_the_first_frame_or_fcs_place_outside_the_arena():
    L = na.load()
    arena, off, ln, st = _args(n=4)
    # frame 3's FCS place [268, 272) is the arena's last four bytes: one byte less and it is outside
    assert L.ether_tx_seal_host(arena.ctypes.data, arena.size - 1, off.ctypes.data, ln.ctypes.data, na.TXS_F_FCS, 0,
                                st.ctypes.data, 4) == -errno.EINVAL
    msg = L.fcs_last_error().decode()
    assert "FCS place of frame 3 " in msg, msg
    ln2 = ln.copy()
    ln2[3] = 69         # frame 3 itself ends one byte past the arena
    assert L.ether_tx_seal_host(arena.ctypes.data, arena.size, off.ctypes.data, ln2.ctypes.data, na.TXS_F_FCS, 0,
                                st.ctypes.data, 4) == -errno.EINVAL
    msg = L.fcs_last_error().decode()
    assert msg.startswith("frame 3 ") or " frame 3 " in msg, msg
    assert "FCS place" not in msg
    off2 = off.copy()
    off2[1] = arena.size + 1
    assert L.ether_tx_seal_host(arena.ctypes.data, arena.size, off2.ctypes.data, ln.ctypes.data, 0, 0,
                                st.ctypes.data, 4) == -errno.EINVAL
    assert "frame 1 " in L.fcs_last_error().decode()
    assert (st == 0xDEADBEEF).all() and (arena == 0xA5).all()   # nothing written
    # n == 0 needs nothing (decided without a device)
    assert L.ether_tx_seal_host(arena.ctypes.data, arena.size, off.ctypes.data, ln.ctypes.data, 1, 0, None, 0) == 0


def _no_gpu():
    try:
        import torch
        return not torch.cuda.is_available()
    except Exception:
        return True


@pytest.mark.skipif(not _no_gpu(), reason="a GPU is present")
def test_no_gpu_is_enodev_without_touching_the_host_counters():
    L = na.load()
    arena, off, ln, st = _args()
    before = (L.fcs_engine_host_batches(), L.fcs_engine_host_fallbacks())
    assert L.ether_tx_seal_host(arena.ctypes.data, arena.size, off.ctypes.data, ln.ctypes.data, 1, 0,
                                st.ctypes.data, 2) == -errno.ENODEV
    assert L.ether_tx_seal_dev(arena.ctypes.data, arena.size, off.ctypes.data, ln.ctypes.data, 1, 0,
                               st.ctypes.data, None, None, 2, None) == -errno.ENODEV
    assert L.ether_tx_seal_fixed_dev(arena.ctypes.data, 68, 64, 2, 1, 0, st.ctypes.data, None, None,
                                     None) == -errno.ENODEV
    assert (L.fcs_engine_host_batches(), L.fcs_engine_host_fallbacks()) == before
    assert (st == 0xDEADBEEF).all() and (arena == 0xA5).all()


# ---- txs::route arithmetic (fcs_debug_txs_route: host arithmetic only) ----
@pytest.fixture
def dma_threshold():
    old = na.tx_seal_set_dma_threshold(16384)
    yield
    na.tx_seal_set_dma_threshold(old)


def test_route_band_edges_threshold_and_fcs_place(dma_threshold):
    base, big = 1 << 20, 1 << 20
    for length, want in ((1495, "general"), (1496, "lds-dma"), (1514, "lds-dma"), (1524, "lds-dma"), (1525, "general")):
        for flags in (0, na.TXS_F_FCS, na.TXS_F_FCS | na.TXS_F_UDP_ZERO):
            assert na.txs_route(base, length + 4, length, big, flags) == want, (length, flags)
            assert na.txs_route(base + 3, length + 4, length, big, flags) == want, (length, flags)
    # the FCS place must fit the stride: stride >= F + 4 with TXS_F_FCS only
    assert na.txs_route(base, 1518, 1514, big, na.TXS_F_FCS) == "lds-dma"        # the packed TX shape
    assert na.txs_route(base, 1517, 1514, big, na.TXS_F_FCS) == "general"
    assert na.txs_route(base, 1517, 1514, big, 0) == "lds-dma"
    assert na.txs_route(base, 1514, 1514, big, na.TXS_F_UDP_ZERO) == "lds-dma"
    # the threshold: more than `frames` frames
    assert na.txs_route(base, 1518, 1514, 16384) == "general"
    assert na.txs_route(base, 1518, 1514, 16385) == "lds-dma"
    assert na.txs_route(base, 1518, 1514, 0) == "none"
    assert na.tx_seal_set_dma_threshold(0) == 16384
    assert na.txs_route(base, 1518, 1514, 9) == "lds-dma"      # nine frames hold two slots
    assert na.txs_route(base, 1518, 1514, 4) == "general"      # the arena must hold two whole slots
    assert na.tx_seal_set_dma_threshold(1 << 63) == 0
    assert na.txs_route(base, 1518, 1514, big) == "general"
    na.tx_seal_set_dma_threshold(0)
    # four frames must fit a 6 KiB slot: 3 * stride + len <= 6126, stride <= 2048
    assert na.txs_route(base, 1536, 1518, big) == "lds-dma"
    assert na.txs_route(base, 1536, 1524, big) == "general"      # 3 * 1536 + 1524 = 6132
    assert na.txs_route(base, 1534, 1524, big) == "lds-dma"      # 6126
    assert na.txs_route(base, 1535, 1522, big) == "general"      # 6127
    assert na.txs_route(base, 2048, 1514, big) == "general"
    assert na.txs_route(base, 64, 60, big) == "general"
    assert na.txs_route(base, 9022, 9018, big) == "general"
