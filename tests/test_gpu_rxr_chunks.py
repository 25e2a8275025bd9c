"""GPU tests of the host form of one-pass RX reassembly (ether_rx_reasm_host) across the chunks of its
host pipeline: batches that the pipeline cuts into three and four chunks, by each bound that can
cut, with a 65535-byte datagram first and last in a chunk and with long runs of frames that belong to
no datagram between the chunks' frames. A chunk is a run of consecutive datagrams, so frames that are
dropped or incomplete never travel: a run of them makes no chunk of its own, it only lies between the
frames the chunks gather. Each case asserts its chunk composition from the constants read from
rxr_engine.cpp. Method as in tests/test_gpu_rxr.py: the whole canaried output arena and every array
against the model."""
import struct

import numpy as np
import pytest

import nstack_amd as na
import rxr_model as rr
from rxr_batch import RBatch, engine_constants, host_chunks, mg

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)
    na.load()
    return torch.device("cuda:0")


def stamped(frame: bytes, q: int) -> bytes:
    """The frame with ip_id = q & 0xffff and the source address' low bytes = q >> 16: its own key."""
    return frame[:18] + struct.pack(">H", q & 0xFFFF) + frame[20:28] + struct.pack(">H", q >> 16) + frame[30:]


def bounds_of(b):
    ch = host_chunks(b.plan)
    return ch, [c[3] for c in ch]


def test_constants_are_what_the_cases_assume():
    k = engine_constants()
    assert k == {"kInBytes": 32 << 20, "kOutBytes": 32 << 20, "kChunkDgs": 1 << 16, "kChunkFrames": 1 << 18}


def test_cut_by_the_datagram_bound_four_chunks(dev, inet_oracle):
    k = engine_constants()
    rng = mg.random.Random(1)
    whole = mg.frame(mg.ip_packet(bytes(rng.randrange(256) for _ in range(9)), ident=0), False)
    n = 3 * k["kChunkDgs"] + 5
    b = RBatch(inet_oracle, [stamped(whole, q) for q in range(n)], 0, align=4, lead=1)
    ch, bounds = bounds_of(b)
    assert bounds == ["dgs", "dgs", "dgs", "end"] and [c[1] - c[0] for c in ch] == [k["kChunkDgs"]] * 3 + [5]
    b.check_host()
    assert b.host_cut == [c[1] - c[0] for c in ch]                       # the engine's own cuts, not only their restatement


def test_cut_by_the_frame_bound_three_chunks_with_runs_that_do_not_travel(dev, inet_oracle):
    """Six-fragment datagrams: 2^18 frames are fewer than 2^16 datagrams. Between them lie runs of 64
    dropped frames and lone fragments: they belong to no chunk."""
    k = engine_constants()
    rng = mg.random.Random(2)
    grp = mg.fragments(rng, bytes(rng.randrange(256) for _ in range(44)), [8, 16, 24, 32, 40], False, hlen_head=24)
    per = k["kChunkFrames"] // 6
    groups = 2 * per + 100
    frames, verdict = [], []
    for q in range(groups):
        frames += [stamped(f, q) for f in grp]
        verdict += [0] * 6
        if q % 5000 == 0:
            frames += [stamped(grp[2], groups + q)] * 3 + [stamped(grp[0], q)] * 64   # lone fragments; dropped copies of a head
            verdict += [0] * 3 + [1] * 64
    b = RBatch(inet_oracle, frames, 0, verdict, 1, align=1)
    ch, bounds = bounds_of(b)
    assert b.m == groups and bounds == ["frames", "frames", "end"] and [c[2] for c in ch] == [6 * per, 6 * per, 600]
    assert (b.fstat == rr.DROPPED).sum() == 64 * len(range(0, groups, 5000))
    b.check_host()
    assert b.host_cut == [c[1] - c[0] for c in ch]                       # the engine's own cuts, not only their restatement


def jumbo(rng, D, ident):
    return mg.frame(mg.ip_packet(rng.integers(0, 256, D - 20, dtype=np.uint8).tobytes(), ident=ident), True)


def test_cut_by_the_input_bound_with_the_largest_datagram_first_and_last_in_a_chunk(dev, inet_oracle):
    """Whole datagrams of 65535 bytes: 14 + 65535 gathered bytes each, so the staging fills before the
    output range does. A chunk is exactly 511 of them: each chunk begins and ends with one."""
    k = engine_constants()
    rng = np.random.default_rng(3)
    per = k["kInBytes"] // (14 + 65535)
    pool = [jumbo(rng, 65535, q) for q in range(3)]
    small = mg.frame(mg.ip_packet(bytes(30), ident=7), True)
    frames = [stamped(pool[q % 3], q) for q in range(2 * per)] + [stamped(pool[1], 2 * per), stamped(small, 9), stamped(pool[0], 2 * per + 1)]
    b = RBatch(inet_oracle, frames, rr.F_TRAILER, align=1, lead=3)
    ch, bounds = bounds_of(b)
    assert bounds == ["in", "in", "end"] and [c[1] - c[0] for c in ch] == [per, per, 3]
    assert all(int(b.plan["dlen"][c[0]]) == 65535 and int(b.plan["dlen"][c[1] - 1]) == 65535 for c in ch)
    b.check_host()
    assert b.host_cut == [c[1] - c[0] for c in ch]                       # the engine's own cuts, not only their restatement


def test_cut_by_the_output_bound_three_chunks(dev, inet_oracle):
    """Datagrams of 1000 bytes at align 128 take 1024 bytes of output and 1014 of staging: the output
    range fills first."""
    k = engine_constants()
    rng = np.random.default_rng(4)
    pool = [jumbo(rng, 1000, q) for q in range(4)]
    per = k["kOutBytes"] // 1024
    n = 2 * per + 7
    b = RBatch(inet_oracle, [stamped(pool[q % 4], q) for q in range(n)], rr.F_TRAILER, align=128, lead=2)
    ch, bounds = bounds_of(b)
    assert bounds == ["out", "out", "end"] and [c[1] - c[0] for c in ch] == [per, per, 7]
    b.check_host()
    assert b.host_cut == [c[1] - c[0] for c in ch]                       # the engine's own cuts, not only their restatement
