"""GPU tests of one-pass RX demultiplexing (include/nstack_dmx.h) through the C ABI. Every batch asserts
that the plan arrays, the whole canaried q (canary bytes in front of, between and behind the records
included), the final status words and qcounts are exactly what the model expects
(tests/dmx_model.py). Whole-q equality is also what shows a write outside a record's own range."""
import struct

import numpy as np
import pytest

import dmx_batch as db
import dmx_model as dm
import nstack_amd as na
import rxr_model as rr
import tso_model as tm
import txf_model as fm
from dmx_batch import A, B, BATCHES, DmxBatch, to_dev

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
MAC = bytes(range(0x20, 0x2C))
MTU = 1500
DROP = na.RXV_FCS_BAD | na.RXV_IP_BAD_HDR | na.RXV_IP_BAD_CSUM | na.RXV_L4_BAD_CSUM


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)
    na.load()
    return torch.device("cuda:0")


# ---- 1. the round trip ----
def tx_dev(dev, dgs, tso):
    """ip_tx_frame_l4_dev (or ip_tx_tso_dev at mss 1460) at mtu 1500 with the FCS: (arena, slot, flen with the FCS)."""
    flags = fm.F_FCS | fm.F_L2_ONE | ((tm.F_MSS_ONE) if tso else 0)
    arena = np.frombuffer(b"".join(dgs), dtype=np.uint8)
    ln = np.array([len(d) for d in dgs], dtype=np.uint32)
    off = np.zeros(len(dgs), dtype=np.uint64)
    off[1:] = np.cumsum(ln[:-1], dtype=np.uint64)
    n, slot = len(dgs), fm.min_slot(MTU, fm.F_FCS)
    d_arena, d_off, d_ln = (to_dev(x, dev) for x in (arena, off, ln))
    d_l2 = to_dev(np.frombuffer(MAC, dtype=np.uint8).reshape(1, 12), dev)
    d_mss = to_dev(np.array([1460], dtype=np.uint16).view(np.int16), dev)
    d_first = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    if tso:
        na.tx_tso_plan_dev(d_arena, arena.size, d_off, d_ln, d_mss, n, MTU, d_first, flags)
    else:
        na.tx_frame_plan_dev(d_arena, arena.size, d_off, d_ln, n, MTU, d_first, flags)
    torch.cuda.synchronize()
    slots = int(d_first.cpu().numpy().view(np.uint64)[n])
    d_out = torch.full((slots * slot + 16,), 0xEE, dtype=torch.uint8, device=dev)
    d_flen = torch.zeros(slots, dtype=torch.int32, device=dev)
    if tso:
        na.tx_tso_dev(d_arena, arena.size, d_off, d_ln, d_l2, d_mss, n, MTU, d_first, d_out, slot, slots, flags, d_flen)
    else:
        na.tx_frame_l4_dev(d_arena, arena.size, d_off, d_ln, d_l2, n, MTU, d_first, d_out, slot, slots, flags, d_flen)
    torch.cuda.synchronize()
    return d_out.cpu().numpy(), slot, d_flen.cpu().numpy().view(np.uint32) + 4


def rx_dev(dev, arena, off, ln, gro):
    """ether_rx_validate_dev, then the reassembly (or coalescing) plan and its L4 build: the device arrays
    they leave, and out_bytes."""
    n = len(off)
    d_arena, d_off, d_ln = to_dev(arena, dev), to_dev(off, dev), to_dev(ln, dev)
    d_v = torch.zeros(n, dtype=torch.int32, device=dev)
    na.rx_validate_dev(d_arena, arena.size, d_off, d_ln, d_v, n, na.RXV_F_TRAILER)
    i32 = lambda k: torch.zeros(k, dtype=torch.int32, device=dev)
    i64 = lambda k: torch.zeros(k, dtype=torch.int64, device=dev)
    t = dict(fstat=i32(n), dst=i64(n), dgi=i32(n), doff=i64(n + 1), dlen=i32(n), counts=i64(2), dverdict=i32(n))
    plan, build = (na.rx_gro_plan_dev, na.rx_gro_dev) if gro else (na.rx_reasm_plan_dev, na.rx_reasm_l4_dev)
    plan(d_arena, arena.size, d_off, d_ln, n, t["fstat"], t["dst"], t["dgi"], t["doff"], t["dlen"], None, t["counts"],
         flags=rr.F_TRAILER, verdict=d_v, drop_mask=DROP, align=4)
    torch.cuda.synchronize()
    out_bytes = int(t["counts"].cpu().numpy().view(np.uint64)[1])
    t["out"] = torch.full((out_bytes + 16,), 0xEE, dtype=torch.uint8, device=dev)
    build(d_arena, arena.size, d_off, d_ln, n, t["fstat"], t["dst"], t["dgi"], t["doff"], t["dlen"], t["counts"], t["out"], out_bytes,
          t["dverdict"], flags=rr.F_TRAILER)
    torch.cuda.synchronize()
    assert (d_v.cpu().numpy().view(np.uint32) & DROP == 0).all()
    return t, out_bytes, n


def demux_given(dev, t, out_bytes, n, bind, align):
    """The batch of what the RX calls left in device memory, run on those very arrays."""
    m = int(t["counts"].cpu().numpy().view(np.uint64)[0])
    out = t["out"].cpu().numpy()
    doff, dlen = t["doff"].cpu().numpy().view(np.uint64), t["dlen"].cpu().numpy().view(np.uint32)
    dv = t["dverdict"].cpu().numpy().view(np.uint32)
    dgs = [out[int(doff[k]):int(doff[k]) + int(dlen[k])].tobytes() for k in range(m)]
    b = DmxBatch(dgs, bind, align, starts=[int(x) for x in doff[:m]], dverdict=dv[:m], drop_mask=na.RXD_L4_BAD_CSUM, n=n,
                 out_bytes=out_bytes)
    r = b.run_dev(dev, given=t)
    b.check_dev(r)
    return b, r


@pytest.mark.parametrize("permuted", [False, True])
def test_round_trip_udp_through_framing_and_reassembly(dev, permuted):
    rng = np.random.default_rng(1)
    socks = [(17, 53, A), (17, 5353, A), (17, 53, B), (17, 9, B), (6, 53, A)]
    bind = [dm.key(*s) for s in socks]
    sent, dgs = [[] for _ in socks], []
    for k in range(60):
        s = int(rng.integers(0, 4))
        p = db.payload(rng, int(rng.choice([0, 1, 300, 1472, 1473, 4000])))
        sent[s].append((0x0A000001, 4000 + k, socks[s][2], socks[s][1], p))
        dgs.append(dm.udp(p, socks[s][1], sport=4000 + k, dst=socks[s][2], ident=k + 1))
    arena, slot, flen = tx_dev(dev, dgs, False)
    nf = len(flen)
    assert nf > len(dgs)                                                  # some were fragmented
    if permuted:                                                          # the frames lie in permuted slots, named in send order
        perm = np.random.default_rng(2).permutation(nf)
        moved = np.full_like(arena, 0xEE)
        for i in range(nf):
            moved[perm[i] * slot:perm[i] * slot + slot] = arena[i * slot:(i + 1) * slot]
        arena, off = moved, perm.astype(np.uint64) * np.uint64(slot)
    else:
        off = np.arange(nf, dtype=np.uint64) * np.uint64(slot)
    t, out_bytes, n = rx_dev(dev, arena, off, flen.astype(np.uint32), False)
    b, r = demux_given(dev, t, out_bytes, n, bind, 16)
    assert b.m == len(dgs) and n > b.m and int(b.plan["qcounts"][0]) == len(dgs)
    for s in range(len(socks)):                                           # every payload as sent, in send order per socket
        assert dm.queue_of(b.plan, r["q"][128:], s) == sent[s], s


def test_round_trip_tcp_through_segmentation_and_coalescing(dev, inet_oracle):
    from gro_batch import tso_datagrams
    dgs = tso_datagrams(inet_oracle, 1460)
    arena, slot, flen = tx_dev(dev, dgs, True)
    nf = len(flen)
    perm = np.random.default_rng(3).permutation(nf)
    t, out_bytes, n = rx_dev(dev, arena, perm.astype(np.uint64) * np.uint64(slot), flen[perm].astype(np.uint32), True)
    b, r = demux_given(dev, t, out_bytes, n, [dm.key(6, 0x50, 0x0A000002)], 8)
    assert b.m == len(dgs) and nf > 3 * b.m                               # a merged datagram is one record
    got = {(src, sport): p for src, sport, _, _, p in dm.queue_of(b.plan, r["q"][128:], 0)}
    assert len(got) == len(dgs)
    for d in dgs:
        hlen = (d[0] & 15) * 4
        thl = (d[hlen + 12] >> 4) * 4
        src, sport = struct.unpack_from(">I", d, 12)[0], struct.unpack_from(">H", d, hlen)[0]
        assert got[(src, sport)] == d[hlen + thl:]


# ---- 2-5. the batches of tests/dmx_batch.py: alignment and sizes, partition edges, every way to make no record ----
_GROUPS = {}
for _name in BATCHES:
    _GROUPS.setdefault(_name.split("-")[0] + ("-" + _name.split("-")[1] if _name.startswith("align") else ""), []).append(_name)


@pytest.mark.parametrize("group", sorted(_GROUPS))
def test_batches_equal_the_model(dev, group):
    for name in _GROUPS[group]:
        b = BATCHES[name]()
        b.check_dev(b.run_dev(dev))


# ---- 6. room and empty cases ----
def test_room_exact_short_and_none(dev):
    full = db.mixed(40, 5, align=16)
    last = max(full.plan["recs"], key=lambda k: int(full.plan["rec"][k]))
    for q_bytes, delivered in ((full.need, 40), (full.need - 1, 39), (0, 0)):
        b = db.mixed(40, 5, align=16, q_bytes=q_bytes)
        assert int(((b.fin & dm.DELIVERED) != 0).sum()) == delivered and int(((b.fin & dm.NO_ROOM) != 0).sum()) == 40 - delivered
        if q_bytes == full.need - 1:
            assert b.fin[last] & dm.NO_ROOM
        b.check_dev(b.run_dev(dev))


def test_no_datagrams_and_a_zero_count(dev):
    b = DmxBatch([], db.binds(3), 8)
    r = b.run_dev(dev)
    b.check_dev(r)
    assert r["qcounts"][:4].tolist() == [0, 0, 0, 0] and r["sbase"][:4].tolist() == [0] * 4
    b = DmxBatch([], db.binds(300), 8, n=1500)                            # counts[0] = 0 with n > 0
    b.check_dev(b.run_dev(dev))
    b = DmxBatch([], [], 8, n=5)
    b.check_dev(b.run_dev(dev))


def test_the_final_words_may_replace_the_plan_words(dev):
    b = db.no_record(16, n=40)
    b.check_dev(b.run_dev(dev, pstat_inplace=True), pstat_inplace=True)
    b.check_dev(b.run_dev(dev, build=False), build=False)                 # the plan alone touches no byte of q


# ---- 7. determinism ----
def test_determinism_at_scale(dev):
    b = db.mixed(20000, 300, seed=6, align=8)
    runs = [b.run_dev(dev) for _ in range(2)]
    b.check_dev(runs[0])
    for k in ("dstat", "dsock", "rec", "sbase", "scnt", "qcounts", "fin", "q"):
        assert np.array_equal(runs[0][k], runs[1][k]), k


# ---- 8. the host form ----
def test_host_form_equals_the_device_form(dev):
    for mk in (lambda: db.no_record(16), db.half_none, db.duplicate_keys, db.outside, lambda: db.alignment(5, 8), db.big_udp):
        b = mk()
        r = b.run_host()
        b.check_host(r)
        assert na.dmx_last_host_chunks() == [b.m]
        d = b.run_dev(dev)
        assert np.array_equal(d["q"], r["q"]) and np.array_equal(d["fin"][:b.m], r["dstat"][:b.m])
    b = DmxBatch([], db.binds(3), 8)
    b.check_host(b.run_host())
    assert na.dmx_last_host_chunks() == []


def test_host_form_across_a_chunk_cut(dev):
    """65537 small datagrams: kChunkDgs cuts them into two chunks; sockets' queues cross the cut."""
    import host_chunks as hc
    rng = np.random.default_rng(13)
    bind = db.binds(9)
    pool = [db.to_key(bind[s], rng, 1 + s) for s in range(9)] + [dm.ip_datagram(1, bytes(8))]
    m = (1 << 16) + 1
    b = DmxBatch([pool[k % 10] for k in range(m)], bind, 8)
    # what travels: a datagram without a record as zero bytes at the end of the one before, which in this
    # packed layout is its own offset
    glen = np.where((b.plan["dstat"][:m] & dm.QUEUED) != 0, b.dlen[:m], 0)
    cut = hc.host_chunks(b.doff[:m], glen, 32 << 20, 1 << 16, 0)
    assert [(c[0], c[1], c[2]) for c in cut] == [(0, 1 << 16, "pkts"), (1 << 16, m, "end")]
    r = b.run_host()
    assert na.dmx_last_host_chunks() == [1 << 16, 1]
    b.check_host(r)
    with pytest.raises(na.FcsError) as e:                                 # one byte short: -ENOSPC, nothing written
        short = DmxBatch([pool[k % 10] for k in range(20)], bind, 8)
        short.q_bytes -= 1
        short.run_host()
    assert e.value.rc == -28


# ---- 9. the launch name, and the arguments only the device can refuse ----
def test_launch_name_and_unaligned_q(dev):
    b = db.mixed(10, 3)
    b.check_dev(b.run_dev(dev))
    assert na.dmx_last_launch() == "demux"
    t = torch.zeros(1024, dtype=torch.uint8, device=dev)
    z = torch.zeros(16, dtype=torch.int64, device=dev)
    with pytest.raises(na.FcsError) as e:
        na.rx_demux_dev(t, 1024, z, z, z, 1, z, z, t.data_ptr() + 8, 512, 16)
    assert e.value.rc == -22 and "aligned" in str(e.value)
