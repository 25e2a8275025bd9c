"""GPU tests of one-pass TX multiplexing (include/nstack_mux.h) through the C ABI. Every batch asserts
that the plan arrays, counts, tnext, the whole canaried dgram (canary bytes in front of, between and
behind the datagrams included) and the final status words are exactly what the model expects
(tests/mux_model.py). Whole-arena equality is also what shows a write outside a datagram's own range.
The round trips run the TX chain and the RX chain on the very device arrays the calls leave."""
import struct

import numpy as np
import pytest

import dmx_model as dm
import mux_batch as mb
import mux_model as mm
import nstack_amd as na
import rxr_model as rr
import txf_model as fm
from dmx_batch import DmxBatch
from mux_batch import BATCHES, HOSTS, IF1, MuxBatch, to_dev

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
MTU = 1500
RXV_BAD = na.RXV_FCS_BAD | na.RXV_RUNT | na.RXV_IP_BAD_HDR | na.RXV_IP_BAD_CSUM | na.RXV_L4_BAD_CSUM | na.RXV_L4_SHORT
DROP = na.RXV_FCS_BAD | na.RXV_IP_BAD_HDR | na.RXV_IP_BAD_CSUM | na.RXV_L4_BAD_CSUM


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)
    na.load()
    return torch.device("cuda:0")


# ---- 1. the batches of tests/mux_batch.py: rows, plan blocks, the copy, the tables, the statuses ----
_GROUPS = {}
for _name in BATCHES:
    _GROUPS.setdefault(_name.split("-")[0] + ("-" + _name.split("-")[2] if _name.startswith("copy") else ""), []).append(_name)


@pytest.mark.parametrize("group", sorted(_GROUPS))
def test_batches_equal_the_model(dev, group):
    for name in _GROUPS[group]:
        b = BATCHES[name]()
        b.check_dev(b.run_dev(dev))


def test_the_copy_batches_reach_every_destination_phase():
    for al in (4, 8, 16, 128):
        for pr, hl in ((17, 28), (6, 40)):
            b = mb.copy(pr, al)
            phases = {(int(b.plan["off"][k]) + hl) % 16 for k in b.plan["dgs"]}
            assert phases == {(hl + x) % 16 for x in range(0, 16, min(al, 16))}, (al, pr)   # all four at align 4
            assert {int(r) % 16 for r in b.rec[:b.n]} == {0, 8}


# ---- 2. room, a plan alone, words in place ----
def test_room_exact_short_and_none(dev):
    full = mb.mixed(40, 5, align=16)
    planned = int(full.plan["counts"][0])
    last = max(full.plan["dgs"], key=lambda k: int(full.plan["off"][k]))
    end = int(full.plan["off"][last]) + int(full.plan["len"][last])
    for room, built in ((end, planned), (end - 1, planned - 1), (0, 0)):
        b = mb.mixed(40, 5, align=16, dgram_bytes=room)
        assert int(((b.fin & mm.BUILT) != 0).sum()) == built and int(((b.fin & mm.NO_ROOM) != 0).sum()) == planned - built
        if room == end - 1:
            assert b.fin[last] & mm.NO_ROOM
        b.check_dev(b.run_dev(dev))


def test_the_final_words_may_replace_the_plan_words(dev):
    b = mb.no_datagram()
    r = b.run_dev(dev, pstat_inplace=True)
    assert np.array_equal(r["fin"][:b.n], b.fin) and np.array_equal(r["dgram"], b.dgram)
    b.check_dev(b.run_dev(dev, build=False), build=False)                 # the plan alone touches no byte of dgram


def test_a_corrupted_plan_array_gives_no_room_and_no_write(dev):
    b = mb.mixed(60, 4, seed=21, align=16)
    ks = sorted(b.plan["dgs"])[3:40:12]
    assert len(ks) == 4

    def corrupt(t):
        t["len"].view(torch.int32)[ks[0]] += 1                            # a wrong len
        t["off"].view(torch.int64)[ks[1]] += 4                            # a misaligned off
        t["himg"][ks[2] * 40 + 9] = 1                                     # a protocol that is neither 6 nor 17
        t["rec"].view(torch.int64)[ks[3]] += 4                            # a record start that is no multiple of 8
    r = b.run_dev(dev, corrupt=corrupt)
    pl = dict(b.plan, dgs={k: d for k, d in b.plan["dgs"].items() if k not in ks})
    want = np.full(b.dgram.size, mb.CANARY, np.uint8)
    fin = mm.build(pl, want[128:], b.dgram_bytes)
    for k in ks:
        fin[k] |= mm.NO_ROOM
    assert np.array_equal(r["fin"][:b.n], fin) and np.array_equal(r["dgram"], want)


# ---- 3. determinism ----
def test_determinism_at_scale(dev):
    b = mb.mixed(20000, 300, seed=6, align=8)
    runs = [b.run_dev(dev) for _ in range(2)]
    b.check_dev(runs[0])
    for k in ("mstat", "off", "len", "l2", "himg", "tnext", "counts", "fin", "dgram"):
        assert np.array_equal(runs[0][k], runs[1][k]), k


# ---- 4. the round trips ----
def frame_dev(dev, r, b, tso):
    """ether_tx_frame_plan_dev + ip_tx_frame_l4_dev (or the TSO pair at mss 1460) at mtu 1500 with the FCS,
    on the device arrays the mux calls left: (the frame arena, slot, flen with the FCS, first, status)."""
    t, n = r["dev"], b.n
    dgram, flags = t["dgram"].data_ptr() + 128, fm.F_FCS | (na.TSO_F_MSS_ONE if tso else 0)
    slot = fm.min_slot(MTU, fm.F_FCS)
    d_first = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    d_stat = torch.zeros(n, dtype=torch.int32, device=dev)
    d_mss = to_dev(np.array([1460], dtype=np.uint16).view(np.int16), dev)
    if tso:
        na.tx_tso_plan_dev(dgram, b.need, t["off"], t["len"], d_mss, n, MTU, d_first, flags)
    else:
        na.tx_frame_plan_dev(dgram, b.need, t["off"], t["len"], n, MTU, d_first, flags)
    torch.cuda.synchronize()
    first = d_first.cpu().numpy().view(np.uint64)
    slots = int(first[n])
    d_out = torch.full((slots * slot + 16,), 0xEE, dtype=torch.uint8, device=dev)
    d_flen = torch.zeros(slots, dtype=torch.int32, device=dev)
    if tso:
        na.tx_tso_dev(dgram, b.need, t["off"], t["len"], t["l2"], d_mss, n, MTU, d_first, d_out, slot, slots, flags, d_flen, d_stat)
    else:
        na.tx_frame_l4_dev(dgram, b.need, t["off"], t["len"], t["l2"], n, MTU, d_first, d_out, slot, slots, flags, d_flen, d_stat)
    torch.cuda.synchronize()
    return d_out.cpu().numpy(), slot, d_flen.cpu().numpy().view(np.uint32) + 4, first, d_stat.cpu().numpy().view(np.uint32)


def rx_dev(dev, arena, off, ln, gro):
    """ether_rx_validate_dev, then the reassembly (or coalescing) plan and its L4 build."""
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
    return t, out_bytes, n, d_v.cpu().numpy().view(np.uint32)


def demux_given(dev, t, out_bytes, n, bind, align):
    m = int(t["counts"].cpu().numpy().view(np.uint64)[0])
    out = t["out"].cpu().numpy()
    doff, dlen = t["doff"].cpu().numpy().view(np.uint64), t["dlen"].cpu().numpy().view(np.uint32)
    dv = t["dverdict"].cpu().numpy().view(np.uint32)
    # every L4 verdict good: checked, or (coalescing) merged and built with a fresh checksum
    assert (dv[:m] & (na.RXD_NO_ROOM | na.RXD_L4_BAD_CSUM | na.RXD_L4_SHORT) == 0).all()
    assert (dv[:m] & (na.RXD_L4_CHECKED | na.GROD_MERGED) != 0).all()
    dgs = [out[int(doff[k]):int(doff[k]) + int(dlen[k])].tobytes() for k in range(m)]
    b = DmxBatch(dgs, bind, align, starts=[int(x) for x in doff[:m]], dverdict=dv[:m], drop_mask=na.RXD_L4_BAD_CSUM, n=n,
                 out_bytes=out_bytes)
    r = b.run_dev(dev, given=t)
    b.check_dev(r)
    return b, r


def test_round_trip_udp_through_framing_reassembly_and_demux(dev):
    rng = np.random.default_rng(1)
    dests = [(HOSTS[0], 53), (HOSTS[1], 5353), (HOSTS[21], 53), (HOSTS[21], 9)]
    ports = (4000, 4001, 4002)
    socks = [(mm.key(17, p, IF1), None, []) for p in ports]
    sent = [[] for _ in dests]
    rt, nb = mb.ROUTES[:2], mb.neigh(HOSTS[:30])
    nodg = 0
    for s in range(3):
        for i in range(20):
            P = int(rng.choice([1, 17, 300, 1472, 1473, 4000]))
            if i % 7 == 3:                                                # a record that makes no datagram
                d, dport, P = ((0x08080808, 53, P), (HOSTS[35], 53, P), (HOSTS[0], 53, 0))[(i // 7 + s) % 3]
                nodg += 1
            else:
                d, dport = dests[int(rng.integers(0, len(dests)))]
            p = mb.payload(rng, P)
            socks[s][2].append(mm.record(d, dport, p))
    b = MuxBatch(socks, rt, nb, 16, id0=0xFFF0)
    for k, d in sorted(b.plan["dgs"].items()):                            # what the destinations expect, in send order
        s = int(np.searchsorted(b.sfirst, k, side="right")) - 1
        dst, dport = struct.unpack_from(">I", d, 16)[0], struct.unpack_from(">H", d, 22)[0]
        src = mb.IF1 if dst >> 8 == mb.NET1 >> 8 else mb.IF2
        sent[dests.index((dst, dport))].append((src, ports[s], dst, dport, d[28:]))
    assert nodg >= 6 and int(b.plan["counts"][0]) == b.n - nodg
    r = b.run_dev(dev)
    b.check_dev(r)
    arena, slot, flen, first, stat = frame_dev(dev, r, b, False)
    for k in range(b.n):                                                  # no datagram: TXF_BAD_HDR and no frame
        if k in b.plan["dgs"]:
            assert stat[k] & (na.TXF_WHOLE | na.TXF_FRAGMENTED) and not stat[k] & (na.TXF_BAD_HDR | na.TXF_BAD_LEN) and first[k + 1] > first[k]
        else:
            assert stat[k] & na.TXF_BAD_HDR and first[k + 1] == first[k]
    nf = len(flen)
    assert nf > len(b.plan["dgs"])                                        # some were fragmented
    for k, d in b.plan["dgs"].items():                                    # the frames carry the plan's MAC pair
        at = int(first[k]) * slot
        assert arena[at:at + 12].tobytes() == b.plan["l2"][k].tobytes()
    off = np.arange(nf, dtype=np.uint64) * np.uint64(slot)
    t, out_bytes, n, v = rx_dev(dev, arena, off, flen.astype(np.uint32), False)
    assert (v & RXV_BAD == 0).all() and (v & na.RXV_IPV4 != 0).all()      # RXV_FRAG and RXV_IP_BAD_LEN (padding) are the documented ones
    bind = [dm.key(17, port, addr) for addr, port in dests]
    db_, rd_ = demux_given(dev, t, out_bytes, n, bind, 16)
    assert db_.m == len(b.plan["dgs"]) and int(db_.plan["qcounts"][0]) == db_.m
    for s in range(len(dests)):
        assert dm.queue_of(db_.plan, rd_["q"][128:], s) == sent[s], s


def test_round_trip_tcp_through_segmentation_coalescing_and_demux(dev):
    rng = np.random.default_rng(2)
    dests = [(HOSTS[0], 80), (HOSTS[1], 8080)]
    pay = [[mb.payload(rng, 32768) for _ in range(3)], [mb.payload(rng, 32768) for _ in range(2)]]
    socks = [(mm.key(6, 5000 + s, IF1), (0xFFFF8000 if s == 0 else 12345, 99, 502, mm.PSH_ACK),
              [mm.record(dests[s][0], dests[s][1], p) for p in pay[s]]) for s in range(2)]
    b = MuxBatch(socks, mb.ROUTES, mb.neigh(HOSTS), 16, id0=7)
    r = b.run_dev(dev)
    b.check_dev(r)
    dg = r["dgram"][128:]
    for s in range(2):                                                    # consecutive records carry consecutive sequence numbers
        seqs = [struct.unpack_from(">I", dg, int(b.plan["off"][k]) + 24)[0] for k in range(int(b.sfirst[s]), int(b.sfirst[s + 1]))]
        assert seqs == [(b.tcb[s][0] + 32768 * i) & 0xFFFFFFFF for i in range(len(seqs))]
        assert int(b.plan["tnext"][s]) == (b.tcb[s][0] + 32768 * len(seqs)) & 0xFFFFFFFF
    arena, slot, flen, first, stat = frame_dev(dev, r, b, True)
    nf = len(flen)
    assert (stat & na.TSO_SEGMENTED != 0).all() and nf == 5 * 23          # 32768 bytes in 1460-byte segments
    off = np.arange(nf, dtype=np.uint64) * np.uint64(slot)
    t, out_bytes, n, v = rx_dev(dev, arena, off, flen.astype(np.uint32), True)
    assert (v & (RXV_BAD | na.RXV_FRAG | na.RXV_IP_BAD_LEN) == 0).all()
    db_, rd_ = demux_given(dev, t, out_bytes, n, [dm.key(6, port, addr) for addr, port in dests], 8)
    for s in range(2):
        got = dm.queue_of(db_.plan, rd_["q"][128:], s)
        assert all(g[:4] == (IF1, 5000 + s, dests[s][0], dests[s][1]) for g in got)
        assert b"".join(g[4] for g in got) == b"".join(pay[s]), s


# ---- 5. the host form ----
def _counters():
    L = na.load()
    return (L.fcs_engine_host_batches(), L.fcs_engine_host_fallbacks())


def test_host_form_equals_the_model_and_the_device_form(dev):
    before = _counters()
    for mk in (mb.no_datagram, mb.wraps, lambda: mb.copy(17, 16), lambda: mb.copy(6, 4), lambda: mb.tables_neigh(257),
               lambda: mb.mixed(300, 9, align=128)):
        b = mk()
        r = b.run_host()
        b.check_host(r)
        assert na.mux_last_host_chunks() == [b.n]
        d = b.run_dev(dev)
        assert np.array_equal(d["dgram"], r["dgram"]) and np.array_equal(d["fin"][:b.n], r["mstat"][:b.n])
    b = mb.mixed(0, 3)
    b.check_host(b.run_host())
    assert na.mux_last_host_chunks() == []
    assert _counters() == before                                          # nothing was answered on the host


def test_host_form_across_a_chunk_cut(dev):
    """65537 small records: kChunkRecs cuts them into two chunks; a socket's queue crosses the cut."""
    import host_chunks as hc
    b = mb.mixed(65537, 300, seed=1, align=4, sizes=(1, 1))
    m = b.n
    planned = (b.plan["mstat"] & mm.PLANNED) != 0
    glen = np.where(planned, 25, 0)                                       # what travels: the 24-byte header and one byte
    goff, last = np.zeros(m, np.int64), 0
    for k in range(m):
        if planned[k]:
            goff[k], last = int(b.rec[k]), int(b.rec[k]) + 25
        else:
            goff[k] = last
    cut = hc.host_chunks(goff, glen, 32 << 20, 1 << 16, 0)
    assert [(c[0], c[1], c[2]) for c in cut] == [(0, 1 << 16, "pkts"), (1 << 16, m, "end")]
    r = b.run_host()
    assert na.mux_last_host_chunks() == [1 << 16, 1]
    b.check_host(r)
    with pytest.raises(na.FcsError) as e:                                 # one byte short: -ENOSPC, nothing written
        short = mb.mixed(20, 3)
        last = max(short.plan["dgs"], key=lambda k: int(short.plan["off"][k]))
        short.dgram_bytes = int(short.plan["off"][last]) + int(short.plan["len"][last]) - 1
        short.run_host()
    assert e.value.rc == -28


# ---- 6. the launch name, and the arguments only the device can refuse ----
def test_launch_name_and_misaligned_arrays(dev):
    b = mb.mixed(10, 3)
    b.check_dev(b.run_dev(dev))
    assert na.mux_last_launch() == "mux"
    t = torch.zeros(1024, dtype=torch.uint8, device=dev)
    z = torch.zeros(64, dtype=torch.int64, device=dev)
    for q_off, h_off, d_off, word in ((4, 0, 0, "q is"), (0, 2, 0, "himg"), (0, 0, 8, "dgram")):
        with pytest.raises(na.FcsError) as e:
            na.tx_mux_dev(t.data_ptr() + q_off, 512, z, 1, z, z, z, z.data_ptr() + h_off, t.data_ptr() + 512 + d_off, 256, 16)
        assert e.value.rc == -22 and word in str(e.value) and "aligned" in str(e.value)
