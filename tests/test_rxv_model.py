"""CPU tests of the one-pass RX validator (include/nstack_rxv.h): the expected-verdict model
(tests/rxv_model.py: the header's rules with the oracle's arithmetic) against the independently
generated golden vectors (tests/golden/make_rxv_golden.py), the ABI, and the argument errors that
need no GPU."""
import ctypes
import errno
import json
import os
import re
import subprocess

import numpy as np
import pytest

import nstack_amd as na
import rxv_model as rm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def rxv_golden():
    with open(os.path.join(GOLDEN, "rxv_vectors.json")) as f:
        vec = json.load(f)
    with open(os.path.join(GOLDEN, vec["arena"]), "rb") as f:
        vec["arena_bytes"] = f.read()
    return vec


def test_model_matches_golden(oracle, inet_oracle, rxv_golden):
    a = rxv_golden["arena_bytes"]
    assert len(rxv_golden["frames"]) >= 300
    for key, flags in (("expect_trailer", rm.F_TRAILER), ("expect_plain", 0)):
        bad = []
        for r in rxv_golden["frames"]:
            got = rm.verdict(oracle, inet_oracle, a[r["off"]:r["off"] + r["len"]], flags)
            if got != r[key]:
                bad.append((r["tag"], r["len"], hex(got), hex(r[key])))
        assert not bad, (key, bad[:10])


def test_golden_covers_every_bit(rxv_golden):
    seen = 0
    for r in rxv_golden["frames"]:
        seen |= r["expect_trailer"]
    for bit in (rm.FCS_BAD, rm.RUNT, rm.IPV4, rm.IP_BAD_HDR, rm.IP_BAD_LEN, rm.IP_BAD_CSUM, rm.FRAG, rm.L4_CHECKED,
                rm.L4_BAD_CSUM, rm.L4_SHORT):
        assert seen & bit, hex(bit)
    protos = {(r["expect_trailer"] >> 16) & 0xFF for r in rxv_golden["frames"] if r["expect_trailer"] & rm.L4_CHECKED}
    assert protos == {1, 6, 17}


def test_golden_pcap_holds_the_listed_frames(rxv_golden):
    arena, off, ln, lt = na.pcap_read(os.path.join(GOLDEN, rxv_golden["pcap"]))
    assert lt == 1 and len(off) == len(rxv_golden["pcap_frames"])
    assert [int(x) for x in ln] == [r["len"] for r in rxv_golden["pcap_frames"]]


def test_model_constants_match_the_binding():
    for name in ("F_TRAILER", "FCS_BAD", "RUNT", "IPV4", "IP_BAD_HDR", "IP_BAD_LEN", "IP_BAD_CSUM", "FRAG", "L4_CHECKED",
                 "L4_BAD_CSUM", "L4_SHORT", "PROTO_SHIFT"):
        assert getattr(rm, name) == getattr(na, "RXV_" + name), name
    hdr = open(os.path.join(ROOT, "include", "nstack_rxv.h")).read()
    for name, val in re.findall(r"#define\s+(RXV_\w+)\s+(0x[0-9a-fA-F]+|\d+)u?", hdr):
        assert getattr(na, name) == int(val, 0), name


# ---- ABI ----
def _declared():
    hdr = open(os.path.join(ROOT, "include", "nstack_rxv.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return re.findall(r"\b((?:ether_rx_|fcs_debug_rxv_)\w+)\s*\(", hdr)


def test_every_declared_function_is_exported_and_listed():
    decl = _declared()
    assert sorted(decl) == sorted(na.RXV_EXPORTS)
    for name in ("ether_rx_validate_dev", "ether_rx_validate_fixed_dev", "ether_rx_validate_host",
                 "ether_rx_validate_set_dma_threshold"):
        assert name in decl, name
    out = subprocess.run(["nm", "-D", "--defined-only", na.LIB_PATH], capture_output=True, text=True, check=True).stdout
    syms = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in decl:
        assert name in syms, name
        assert getattr(na.load(), name).argtypes is not None, name
    assert not set(na.RXV_EXPORTS) & set(na.EXPORTS)   # EXPORTS mirrors the five older headers only


# ---- argument errors (no GPU needed: they are decided before any device call) ----
def _args(n=2, length=64):
    arena = np.zeros(n * length, dtype=np.uint8)
    off = (np.arange(n, dtype=np.uint64) * length)
    ln = np.full(n, length, dtype=np.uint32)
    verdict = np.full(n, 0xDEADBEEF, dtype=np.uint32)
    return arena, off, ln, verdict


def test_unknown_flag_bits_are_einval():
    L = na.load()
    arena, off, ln, v = _args()
    for flags in (2, 0x80000000, 3):
        assert L.ether_rx_validate_host(arena.ctypes.data, arena.size, off.ctypes.data, ln.ctypes.data, flags, 0,
                                        v.ctypes.data, 2) == -errno.EINVAL
        assert L.ether_rx_validate_dev(arena.ctypes.data, arena.size, off.ctypes.data, ln.ctypes.data, flags, 0,
                                       v.ctypes.data, None, 2, None) == -errno.EINVAL
        assert L.ether_rx_validate_fixed_dev(arena.ctypes.data, 64, 64, 2, flags, 0, v.ctypes.data, None,
                                             None) == -errno.EINVAL
        with pytest.raises(na.FcsError):
            na.rx_validate_host(arena, arena.size, off, ln, v, 2, flags=flags)
    assert "flag" in L.fcs_last_error().decode()
    assert (v == 0xDEADBEEF).all()


def test_null_verdict_is_einval():
    L = na.load()
    arena, off, ln, _ = _args()
    assert L.ether_rx_validate_host(arena.ctypes.data, arena.size, off.ctypes.data, ln.ctypes.data, 1, 0, None,
                                    2) == -errno.EINVAL
    assert L.ether_rx_validate_dev(arena.ctypes.data, arena.size, off.ctypes.data, ln.ctypes.data, 1, 0, None, None,
                                   2, None) == -errno.EINVAL
    assert L.ether_rx_validate_fixed_dev(arena.ctypes.data, 64, 64, 2, 1, 0, None, None, None) == -errno.EINVAL
    # n == 0 needs no verdict array (host form: decided without a device)
    assert L.ether_rx_validate_host(arena.ctypes.data, arena.size, off.ctypes.data, ln.ctypes.data, 1, 0, None, 0) == 0


def test_fixed_stride_below_len_is_einval():
    arena, _, _, v = _args()
    assert na.load().ether_rx_validate_fixed_dev(arena.ctypes.data, 32, 64, 2, 1, 0, v.ctypes.data, None,
                                                 None) == -errno.EINVAL


def test_host_form_names_the_first_frame_outside_the_arena():
    L = na.load()
    arena, off, ln, v = _args(n=4)
    ln[2] = 65          # frame 2 ends one byte past its neighbour's start: still inside
    ln[3] = 65          # frame 3 ends one byte past the arena
    off2 = off.copy()
    assert L.ether_rx_validate_host(arena.ctypes.data, arena.size, off2.ctypes.data, ln.ctypes.data, 1, 0,
                                    v.ctypes.data, 4) == -errno.EINVAL
    assert "frame 3 " in L.fcs_last_error().decode()
    off2[1] = arena.size + 1
    assert L.ether_rx_validate_host(arena.ctypes.data, arena.size, off2.ctypes.data, ln.ctypes.data, 1, 0,
                                    v.ctypes.data, 4) == -errno.EINVAL
    assert "frame 1 " in L.fcs_last_error().decode()
    assert (v == 0xDEADBEEF).all()   # nothing written


def _no_gpu():
    try:
        import torch
        return not torch.cuda.is_available()
    except Exception:
        return True


@pytest.mark.skipif(not _no_gpu(), reason="a GPU is present")
def test_no_gpu_is_enodev_without_touching_the_host_counters():
    L = na.load()
    arena, off, ln, v = _args()
    before = (L.fcs_engine_host_batches(), L.fcs_engine_host_fallbacks())
    assert L.ether_rx_validate_host(arena.ctypes.data, arena.size, off.ctypes.data, ln.ctypes.data, 1, 0,
                                    v.ctypes.data, 2) == -errno.ENODEV
    assert L.ether_rx_validate_dev(arena.ctypes.data, arena.size, off.ctypes.data, ln.ctypes.data, 1, 0,
                                   v.ctypes.data, None, 2, None) == -errno.ENODEV
    assert L.ether_rx_validate_fixed_dev(arena.ctypes.data, 64, 64, 2, 1, 0, v.ctypes.data, None,
                                         None) == -errno.ENODEV
    assert (L.fcs_engine_host_batches(), L.fcs_engine_host_fallbacks()) == before
    assert (v == 0xDEADBEEF).all()


# ---- rxv::route arithmetic (fcs_debug_rxv_route: host arithmetic only) ----
@pytest.fixture
def dma_threshold():
    old = na.rx_validate_set_dma_threshold(16384)
    yield
    na.rx_validate_set_dma_threshold(old)


def test_route_band_edges_and_threshold(dma_threshold):
    base, big = 1 << 20, 1 << 20
    for length, want in ((1495, "general"), (1496, "lds-dma"), (1518, "lds-dma"), (1524, "lds-dma"), (1525, "general")):
        assert na.rxv_route(base, length, length, big) == want, length
        assert na.rxv_route(base + 3, length, length, big) == want, length
    # the threshold: more than `frames` frames
    assert na.rxv_route(base, 1518, 1518, 16384) == "general"
    assert na.rxv_route(base, 1518, 1518, 16385) == "lds-dma"
    assert na.rxv_route(base, 1518, 1518, 0) == "none"
    assert na.rx_validate_set_dma_threshold(0) == 16384
    assert na.rxv_route(base, 1518, 1518, 9) == "lds-dma"      # nine frames hold two slots
    assert na.rxv_route(base, 1518, 1518, 4) == "general"      # the arena must hold two whole slots
    assert na.rx_validate_set_dma_threshold(1 << 63) == 0
    assert na.rxv_route(base, 1518, 1518, big) == "general"
    na.rx_validate_set_dma_threshold(0)
    # four frames must fit a 6 KiB slot: 3 * stride + len <= 6126, stride <= 2048
    assert na.rxv_route(base, 1536, 1518, big) == "lds-dma"
    assert na.rxv_route(base, 1536, 1524, big) == "general"      # 3 * 1536 + 1524 = 6132
    assert na.rxv_route(base, 1534, 1524, big) == "lds-dma"      # 6126
    assert na.rxv_route(base, 1535, 1522, big) == "general"      # 6127
    assert na.rxv_route(base, 2048, 1514, big) == "general"
    assert na.rxv_route(base, 64, 60, big) == "general"
    assert na.rxv_route(base, 9018, 9018, big) == "general"
