"""GPU tests of one-pass TX framing at the sizes where its persistent grid and its host pipeline do
what small batches never make them do: more datagrams than the grid cap of one workgroup per CU
covers at once, so every row comes back to the work counter several times (with rows of the same wave
in the middle of a frame, with runs that are refused entirely, with a partial last run), and host
batches that the pipeline cuts into three or more chunks, by each bound that can cut. Method as in
tests/test_gpu_txf.py: the whole canaried output arena, flen, fcs, status, first and the plan's
status against the model (memoised: the datagrams are drawn from a small pool)."""
import numpy as np
import pytest

import nstack_amd as na
import txf_model as fm
from txf_batch import FCS, Batch, datagram, engine_constants, host_chunks, pack

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROWS_PER_GROUP, RUN = 32, 8   # txf_kernel: 512 threads are 32 quarter-waves, kRun datagrams a run
HEAVY = 8185                  # frames of 65535 bytes with a 60-byte header at mtu 76


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)
    na.load()
    return torch.device("cuda:0")


def refused(rng, mtu):
    """Datagrams that become no frame: TXF_BAD_HDR (three ways), TXF_BAD_LEN, TXF_REFRAG."""
    return [b"", rng.integers(0, 256, 19, dtype=np.uint8).tobytes(), datagram(rng, 20, 30, vhl=0x05),
            datagram(rng, 24, 17, ip_len=40), datagram(rng, 20, 3, ip_len=24),
            datagram(rng, 20, mtu, foff=0x2000), datagram(rng, 28, 2 * mtu, foff=0x0003)]


# ---- A: the full grid, rows that come back ----
N_GRID = 2 * (1 << 18) + 77


@pytest.fixture(scope="module")
def grid():
    """n datagrams at mtu 76 drawn by index from a pool of 100: (arena, off, len, l2, planted)."""
    mtu, n, rng = 76, N_GRID, np.random.default_rng(80)
    whole = [datagram(rng, hlen, int(rng.integers(0, 77 - hlen))) for hlen in range(20, 64, 4) for _ in range(7)]
    frag = []
    for c in (2, 3, 4, 5, 6):
        for hlen in (20, 24, 40, 60):
            mx = fm.frag_unit(mtu, hlen)
            lo = max((c - 1) * mx + 1, mtu + 1 - hlen)   # c frames, and more than the mtu
            if lo <= c * mx:
                frag.append(datagram(rng, hlen, int(rng.integers(lo, c * mx + 1))))
    bad = refused(rng, mtu)
    heavy = [datagram(rng, 60, 65535 - 60) for _ in range(2)]
    pool = whole + frag + bad + heavy
    assert 90 <= len(pool) <= 110
    arena, poff, pln = pack(pool, seed=81)
    W, Fr, Bd = len(whole), len(frag), len(bad)
    pick = np.where(rng.random(n) < 0.2, W + rng.integers(0, Fr, n), rng.integers(0, W, n))
    last_run = n - n % RUN
    planted = {"heavy": [3, n // 4 + 1, n // 2 + 6, 3 * n // 4 + 2, last_run + 2],
               "refused": [(1001, 1031), (n // 2 + 100, n // 2 + 164), (last_run - 24, last_run)]}
    for q, i in enumerate(planted["heavy"]):
        pick[i] = W + Fr + Bd + q % 2
    for lo, hi in planted["refused"]:
        pick[lo:hi] = W + Fr + rng.integers(0, Bd, hi - lo)
    l2 = np.random.default_rng(82).integers(0, 256, (4, 12), dtype=np.uint8)[rng.integers(0, 4, n)]
    return arena, poff[pick], pln[pick], l2, planted


@pytest.mark.parametrize("flags", [FCS, FCS | fm.F_L2_ONE])
def test_full_grid_with_returning_rows(dev, oracle, inet_oracle, grid, flags):
    """More than 4 x CUs x 256 datagrams, so the grid is capped at one workgroup per CU and a row takes
    at least four runs on average. Planted: five datagrams of 8185 frames (index 3, three in between,
    one in the partial last run), three stretches of 24 or more refused datagrams (one fills the
    second-to-last run), n mod 8 = 5. The host form cuts the same batch at 2^18 datagrams twice, so a
    staging slot is used again, with per-datagram MAC records and with the single record."""
    arena, off, ln, l2, planted = grid
    n, cus = N_GRID, torch.cuda.get_device_properties(0).multi_processor_count
    assert n > 4 * cus * ROWS_PER_GROUP * RUN and n % RUN == 5
    b = Batch(oracle, inet_oracle, None, 76, flags, placed=(arena, off, ln), l2=l2, base=1, seed=83)
    cnt = np.diff(b.plan_first.astype(np.int64))
    for i in planted["heavy"]:
        assert ln[i] == 65535 and cnt[i] == HEAVY and b.status[i] == fm.FRAGMENTED
    assert planted["heavy"][0] == 3 and planted["heavy"][-1] >= n - n % RUN
    seen = 0
    for lo, hi in planted["refused"]:
        assert hi - lo >= 24 and (cnt[lo:hi] == 0).all()
        seen |= int(np.bitwise_or.reduce(b.status[lo:hi]))
    assert seen == fm.BAD_HDR | fm.BAD_LEN | fm.REFRAG
    lo, hi = planted["refused"][-1]
    assert hi == n - n % RUN and lo <= hi - RUN                       # the whole second-to-last run
    frac = (cnt > 1).mean()
    assert 0.15 < frac < 0.25 and set(np.unique(cnt)) >= {0, 1, 2, 3, 4, 5, 6, HEAVY}
    if flags & fm.F_L2_ONE:
        assert (b.expect[b.base:b.base + 12] == l2[0]).all() and not (l2[1:65] == l2[0]).all()
    b.check_dev(b.run_dev(dev))
    k = engine_constants()
    chunks = host_chunks(b.plan_first, ln, b.slot, k)
    assert [(e - i, bound) for i, e, _, bound in chunks] == [(k["kChunkDgs"], "dgs"), (k["kChunkDgs"], "dgs"), (77, "end")]
    assert all(fr > 0 for _, _, fr, _ in chunks)
    b.check_host()


# ---- B: the host pipeline's chunk bounds ----
def test_host_chunks_cut_by_the_slot_bytes(dev, oracle, inet_oracle):
    """slot = 1 MiB: 64 frames fill a chunk's 64 MiB of slots. A stretch of refused datagrams travels
    in the chunk it follows (a refused datagram never ends a chunk: it adds neither bytes nor frames)."""
    rng, mtu = np.random.default_rng(90), 1500
    dgs = []
    for i in range(60):
        if 20 <= i < 32:
            dgs.append(refused(rng, mtu)[i % 7])
        else:
            dgs.append(datagram(rng, 20 + 4 * (i % 5), int(rng.integers(0, 1400)) if i % 2 else int(rng.integers(3000, 9000))))
    b = Batch(oracle, inet_oracle, dgs, mtu, FCS, slot=1 << 20, seed=91)
    assert 120 <= b.total <= 200
    k = engine_constants()
    chunks = host_chunks(b.plan_first, b.ln, b.slot, k)
    assert len(chunks) >= 3 and [c[3] for c in chunks] == ["out"] * (len(chunks) - 1) + ["end"]
    assert all(58 <= c[2] <= 64 for c in chunks[:-1]) and k["kOutBytes"] // b.slot == 64
    assert any(i < 20 and e >= 32 for i, e, _, _ in chunks)            # the refused stretch, inside one chunk
    b.check(dev)


def test_host_chunks_cut_by_the_datagram_bytes(dev, oracle, inet_oracle):
    """1030 datagrams of 65535 bytes at mtu 9000, three distinct ones gathered through repeated off[]:
    512 of them fill a chunk's 32 MiB of datagrams, so there are three chunks and a staging slot is used
    again (520 datagrams, 34 MB, would make two)."""
    rng, mtu, n = np.random.default_rng(92), 9000, 1030
    pool = [datagram(rng, hlen, 65535 - hlen) for hlen in (20, 36, 60)]
    arena, poff, pln = pack(pool, seed=93)
    pick = rng.integers(0, 3, n)
    b = Batch(oracle, inet_oracle, None, mtu, FCS, placed=(arena, poff[pick], pln[pick]),
              l2=np.random.default_rng(94).integers(0, 256, (2, 12), dtype=np.uint8)[rng.integers(0, 2, n)], seed=95)
    assert b.total == 8 * n and set(pick) == {0, 1, 2}
    k = engine_constants()
    chunks = host_chunks(b.plan_first, b.ln, b.slot, k)
    assert [(e - i, bound) for i, e, _, bound in chunks] == [(512, "in"), (512, "in"), (6, "end")]
    assert 513 * 65535 > k["kInBytes"] >= 512 * 65535
    b.check(dev)


def test_host_chunk_without_frames_between_live_ones(dev, oracle, inet_oracle):
    """2^18 refused datagrams from a chunk border on: the only way to a chunk that needs no device,
    since a refused datagram is taken into any chunk. The chunks before and behind it build frames,
    the one behind it in the staging slot the first one used."""
    rng, mtu = np.random.default_rng(96), 1500
    k = engine_constants()
    C = k["kChunkDgs"]
    n = 2 * C + 3
    pool = refused(rng, mtu) + [datagram(rng, 20, 100), datagram(rng, 24, 4000), datagram(rng, 60, 1441)]
    arena, poff, pln = pack(pool, seed=97)
    pick = rng.integers(0, 7, n)
    live = [0, 5, 77, C - 1, 2 * C, 2 * C + 1, 2 * C + 2]
    pick[live] = 7 + np.arange(len(live)) % 3
    b = Batch(oracle, inet_oracle, None, mtu, FCS, placed=(arena, poff[pick], pln[pick]),
              l2=np.random.default_rng(98).integers(0, 256, (3, 12), dtype=np.uint8)[rng.integers(0, 3, n)], seed=99)
    chunks = host_chunks(b.plan_first, b.ln, b.slot, k)
    assert [(e - i, bound) for i, e, _, bound in chunks] == [(C, "dgs"), (C, "dgs"), (3, "end")]
    assert [c[2] > 0 for c in chunks] == [True, False, True]
    assert np.flatnonzero(np.diff(b.plan_first.astype(np.int64))).tolist() == live
    b.check(dev)
