"""GPU tests of one-pass RX reassembly (include/nstack_rxr.h) through the C ABI. For every batch the
device form (ether_rx_reasm_dev after ether_rx_reasm_plan_dev) and the host form must leave
byte-identical output arenas, equal to the model's (tests/rxr_model.py: the header's rules with the
oracle's checksum) and, for the golden vectors, to the independently generated datagrams. The output
arena is canary bytes before, between (alignment gaps) and behind the datagrams and is compared as a
whole, so a write to any byte other than a delivered datagram's fails the test; every plan array and
the final status words are compared with the model's too."""
import struct
import threading

import numpy as np
import pytest

import nstack_amd as na
import rxr_model as rr
import txf_model as fm
from rxr_batch import RBatch, mg, to_dev

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)
    na.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def rxr_golden():
    return rr.load_golden()


# ---- 1. the golden vectors, at four arena start alignments ----
@pytest.mark.parametrize("align", [1, 16])
def test_golden_vectors(dev, inet_oracle, rxr_golden, align):
    for c in rxr_golden["cases"]:
        for lead in range(4):
            b = RBatch(inet_oracle, c["frames"], c["flags"], c["verdict"], c["drop_mask"], align, lead=lead, gap=lead,
                       out_base=(5 * lead) & 15, out_bytes=c["out_bytes"], seed=lead)
            if align == 1:   # the model's arena holds exactly the golden datagrams
                assert b.fstat.tolist() == c["fstat"], c["tag"]
                for k, (want, fits) in enumerate(zip(c["dgrams"], c["fits"])):
                    at = b.base + int(b.plan["doff"][k])
                    assert not fits or b.expect[at:at + len(want)].tobytes() == want, (c["tag"], k)
            b.check(dev, host=lead == 0)
    assert na.rxr_last_launch() == "general"


# ---- 2. alignment sweep ----
SWEEP_L = list(range(1, 201)) + [1536 + t for t in range(-4, 5)]
HLENS = (20, 24, 60)


@pytest.fixture(scope="module")
def sweep_frames():
    """Whole frames and three-fragment groups whose last payload is L, for every L of the sweep; the
    header lengths rotate so that each meets every residue of L mod 16."""
    rng = mg.random.Random(9)
    rb = lambda n: bytes(rng.randrange(256) for _ in range(n))
    frames, seen = [], set()
    for q, L in enumerate(SWEEP_L):
        hw, hh = HLENS[q % 3], HLENS[(q // 3 + q) % 3]
        seen |= {("w", hw, L % 16), ("g", hh, L % 16)}
        frames.append(mg.frame(mg.ip_packet(rb(L), hw, ident=q, rng=rng), bool(q & 1)) + (b"" if q & 1 else rb(4)))
        a, m = 8 * (1 + q % 5), 8 * (1 + q % 3)
        frames += mg.fragments(rng, rb(a + m + L), [a, a + m], True, hlen_head=hh, hlen_rest=HLENS[(q + 1) % 3], ident=0x4000 + q)
    assert seen == {(k, h, r) for k in "wg" for h in HLENS for r in range(16)}
    return frames


@pytest.mark.parametrize("start", [0, 1, 2, 3])
def test_alignment_sweep(dev, inet_oracle, sweep_frames, start):
    """Source start 0..3 x destination residue 0..15: align = 1 behind a first datagram of 20..35 bytes
    moves every datagram behind it through all sixteen residues; the frames abut in the arena, so their
    own starts take every residue too. Fragment payloads abut byte-exactly inside a datagram."""
    for first in range(20, 36):
        head = mg.frame(mg.ip_packet(bytes(first - 20), ident=0x3FFF), True)
        b = RBatch(inet_oracle, [head] + sweep_frames, rr.F_TRAILER, align=1, lead=start, out_base=first & 15, seed=first)
        assert int(b.plan["doff"][1]) == first and b.m == 1 + 2 * len(SWEEP_L)
        b.check(dev, host=first == 20 + start)


# ---- 3. borders ----
def test_borders_of_the_16_byte_lines_and_jumbo_datagrams(dev, inet_oracle):
    rng = mg.random.Random(3)
    rb = lambda n: bytes(rng.randrange(256) for _ in range(n))
    frames = []
    for k in (1, 2, 42):
        for t in range(-4, 5):
            frames.append(mg.frame(mg.ip_packet(rb(1536 * k + t - 20), ident=k * 16 + t + 4), False))
    frames += [mg.frame(mg.ip_packet(rb(65535 - hl), hl, ident=0x900 + hl, rng=rng), True) for hl in (20, 60)]
    for align, base in ((1, 0), (1, 7), (128, 3)):
        RBatch(inet_oracle, frames, 0, align=align, lead=base & 3, out_base=base).check(dev, host=align == 128)


def framed(dev, dgs, mtu, macs, seed=0):
    """ether_tx_frame_dev over the datagrams: (device arena of slots, slot, first[], flen[]) with the FCS."""
    arena = np.frombuffer(b"".join(dgs), dtype=np.uint8)
    ln = np.array([len(d) for d in dgs], dtype=np.uint32)
    n, slot = len(dgs), fm.min_slot(mtu, fm.F_FCS)
    off = np.zeros(n, dtype=np.uint64)
    off[1:] = np.cumsum(ln[:-1], dtype=np.uint64)
    d_arena, d_off, d_ln, d_l2 = (to_dev(x, dev) for x in (arena, off, ln, macs))
    d_first = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    na.tx_frame_plan_dev(d_arena, arena.size, d_off, d_ln, n, mtu, d_first, fm.F_FCS)
    torch.cuda.synchronize()
    first = d_first.cpu().numpy().view(np.uint64)
    slots = int(first[n])
    d_out = torch.full((slots * slot + 16,), 0xEE, dtype=torch.uint8, device=dev)
    d_flen = torch.zeros(slots, dtype=torch.int32, device=dev)
    na.tx_frame_dev(d_arena, arena.size, d_off, d_ln, d_l2, n, mtu, d_first, d_out, slot, slots, fm.F_FCS, d_flen)
    torch.cuda.synchronize()
    return d_out, slot, first, d_flen.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("tag,mtu,cnt", [("max_m76_h60", 76, 8185), ("max_m1500_h20", 1500, 45)])
def test_the_framers_largest_datagrams_come_back(dev, inet_oracle, tag, mtu, cnt):
    g = fm.load_golden()
    r = next(r for r in g["datagrams"] if r["tag"] == tag)
    dg = g["input_bytes"][r["off"]:r["off"] + r["len"]]
    d_out, slot, first, flen = framed(dev, [dg], mtu, np.zeros((1, 12), dtype=np.uint8))
    assert int(first[1]) == cnt and len(dg) == 65535
    perm = np.random.default_rng(cnt).permutation(cnt)
    arena = d_out.cpu().numpy()
    b = RBatch(inet_oracle, flags=rr.F_TRAILER, align=16, placed=(arena, perm.astype(np.uint64) * slot, flen[perm] + 4))
    assert b.m == 1 and int(b.plan["dlen"][0]) == 65535 and int(b.plan["dlead"][0]) == int(np.flatnonzero(perm == 0)[0])
    got = b.expect[b.base:b.base + 65535].tobytes()
    assert got[:6] == dg[:6] and got[6:8] == b"\x00\x00" and got[8:10] == dg[8:10] and got[12:] == dg[12:]
    b.check(dev)


# ---- 4. round trip on the device ----
@pytest.mark.parametrize("mtu", [76, 100, 576, 1500, 9000])
def test_round_trip_on_the_device(dev, mtu):
    """frame -> permute the slots -> reassemble -> frame again gives the same frames byte for byte."""
    g = fm.load_golden()
    a = g["input_bytes"]
    recs = [r for r in g["datagrams"] if r["mtu"] == mtu and r["flen"] and not r["tag"].endswith("_frag_fits")]
    dgs = [a[r["off"]:r["off"] + r["len"]] for r in recs]
    macs = np.array([list(bytes.fromhex(r["mac"])) for r in recs], dtype=np.uint8)
    d_fr, slot, first, flen = framed(dev, dgs, mtu, macs)
    slots, n = int(first[-1]), len(dgs)
    perm = np.random.default_rng(mtu).permutation(slots)
    owner = np.repeat(np.arange(n), np.diff(first.astype(np.int64)))     # the datagram of a slot
    d_off, d_ln = to_dev(perm.astype(np.uint64) * slot, dev), to_dev(flen[perm] + 4, dev)
    t = dict(fstat=torch.zeros(slots, dtype=torch.int32, device=dev), dst=torch.zeros(slots, dtype=torch.int64, device=dev),
             dgi=torch.zeros(slots, dtype=torch.int32, device=dev), doff=torch.zeros(slots + 1, dtype=torch.int64, device=dev),
             dlen=torch.zeros(slots, dtype=torch.int32, device=dev), dlead=torch.zeros(slots, dtype=torch.int32, device=dev),
             counts=torch.zeros(2, dtype=torch.int64, device=dev))
    na.rx_reasm_plan_dev(d_fr, slots * slot, d_off, d_ln, slots, t["fstat"], t["dst"], t["dgi"], t["doff"], t["dlen"], t["dlead"],
                         t["counts"], flags=rr.F_TRAILER, align=4)
    torch.cuda.synchronize()
    m, total = (int(x) for x in t["counts"].cpu().numpy())
    assert m == n                                                        # the keys of the fixtures are distinct
    d_dg = torch.full((total + 16,), 0xEE, dtype=torch.uint8, device=dev)
    na.rx_reasm_dev(d_fr, slots * slot, d_off, d_ln, slots, t["fstat"], t["dst"], t["dgi"], t["doff"], t["dlen"], d_dg, total,
                    flags=rr.F_TRAILER, fstat=t["fstat"])
    torch.cuda.synchronize()
    assert (t["fstat"].cpu().numpy().view(np.uint32) & rr.DELIVERED).all()
    lead = t["dlead"].cpu().numpy().view(np.uint32)[:m]
    back = owner[perm[lead]]                                             # datagram k came from input datagram back[k]
    assert sorted(back.tolist()) == list(range(n))
    assert (t["dlen"].cpu().numpy().view(np.uint32)[:m] == np.array([len(dgs[i]) for i in back])).all()
    # frame the reassembled datagrams again, where they lie, with their own MAC pairs
    d_first2 = torch.zeros(m + 1, dtype=torch.int64, device=dev)
    na.tx_frame_plan_dev(d_dg, total, t["doff"], t["dlen"], m, mtu, d_first2, fm.F_FCS)
    d_out2 = torch.full((slots * slot + 16,), 0xEE, dtype=torch.uint8, device=dev)
    na.tx_frame_dev(d_dg, total, t["doff"], t["dlen"], to_dev(macs[back], dev), m, mtu, d_first2, d_out2, slot, slots, fm.F_FCS)
    torch.cuda.synchronize()
    first2 = d_first2.cpu().numpy().view(np.uint64)
    assert int(first2[m]) == slots
    one, two = d_fr.cpu().numpy()[:slots * slot].reshape(slots, slot), d_out2.cpu().numpy()[:slots * slot].reshape(slots, slot)
    for k in range(m):
        i = int(back[k])
        c = int(first[i + 1] - first[i])
        assert int(first2[k + 1] - first2[k]) == c
        assert np.array_equal(two[int(first2[k]):int(first2[k]) + c], one[int(first[i]):int(first[i]) + c]), recs[i]["tag"]


# ---- 5. grouping at scale ----
def scale_batch(inet_oracle, n, seed):
    """n frames drawn from a small pool with restamped, sequential ids, the fragments of a group up to
    a few dozen frames apart; runs of 64 dropped frames."""
    rng = mg.random.Random(seed)
    rb = lambda k: bytes(rng.randrange(256) for _ in range(k))
    pool = [[mg.frame(mg.ip_packet(rb(k), hl, proto=40 + q, rng=rng), True)] for q, (k, hl) in enumerate(((0, 20), (33, 24), (100, 60)))]
    pool += [mg.fragments(rng, rb(k), cuts, True, hlen_head=hh, hlen_rest=20, proto=50 + q)
             for q, (k, cuts, hh) in enumerate(((9, [8], 20), (40, [16], 24), (100, [32, 64], 60), (31, [8, 16, 24], 20)))]
    lone = mg.fragments(rng, rb(64), [32], True, proto=60)
    pool += [lone[:1], lone[1:], [mg.frame(rb(40), True, etype=0x0806)]]
    frames, q = [], 0
    while len(frames) < n:
        t = pool[(q * 7 + q // 11) % len(pool)]
        ident = struct.pack(">H", q & 0xFFFF)
        frames += [f[:18] + ident + f[20:] if len(f) >= 34 and f[12:14] == b"\x08\x00" else f for f in t]
        q += 1
    frames = frames[:n]
    order = np.arange(n)
    prng = np.random.default_rng(seed)
    for s in range(0, n, 48):                                            # shuffle within windows of 48 frames
        order[s:s + 48] = prng.permutation(order[s:s + 48])
    frames = [frames[i] for i in order]
    verdict = np.zeros(n, dtype=np.uint32)
    for s in range(100, n, 1000):
        verdict[s:s + 64] = na.RXV_FCS_BAD
    return RBatch(inet_oracle, frames, rr.F_TRAILER, verdict, na.RXV_FCS_BAD, align=8, lead=1, seed=seed)


@pytest.mark.parametrize("n", [255, 256, 257, 65537, (1 << 18) + 77])
def test_grouping_at_scale(dev, inet_oracle, n):
    b = scale_batch(inet_oracle, n, n & 0xFFFF)
    assert b.m > n // 8 and (b.fstat & rr.INCOMPLETE).any() and (b.fstat & rr.DROPPED).sum() >= 64 * (n // 1000)
    runs = [b.run_dev(dev) for _ in range(3)]
    for r in runs:
        b.check_dev(r)
    for r in runs[1:]:                                                   # a function of the input alone
        for k, cnt in (("fstat", b.n), ("dst", b.n), ("dgi", b.n), ("doff", b.m + 1), ("dlen", b.m), ("dlead", b.m), ("counts", 2)):
            assert np.array_equal(r[k][:cnt], runs[0][k][:cnt]), k
    if n <= 65537:
        b.check_host()


# ---- 6. composition ----
def test_composition_with_the_validator_and_the_checksum_batches(dev, oracle, inet_oracle):
    """Verdicts from ether_rx_validate_dev drop one FCS-corrupted fragment of every third group: that
    group is RXR_INCOMPLETE and the rest is delivered; inet_csum_batch_dev over the reassembled UDP
    datagrams' segments equals the oracle's udp_checksum."""
    rng = mg.random.Random(6)
    rb = lambda k: bytes(rng.randrange(256) for _ in range(k))
    frames, bad = [], []
    for q in range(60):
        seg = rb(100 + 13 * q)
        fr = mg.fragments(rng, seg, [32, 72], True, hlen_head=(20, 28)[q & 1], ident=q, src=0x0A000000 + q)
        if q % 3 == 0:
            f = bytearray(fr[1])
            f[40] ^= 0x10
            fr[1] = bytes(f)
            bad.append(len(frames) + 1)
        frames += fr
    arena, off, ln = rr.layout(frames, lead=2)
    n = len(frames)
    d_arena, d_off, d_ln = to_dev(arena, dev), to_dev(off, dev), to_dev(ln, dev)
    d_v = torch.zeros(n, dtype=torch.int32, device=dev)
    na.rx_validate_dev(d_arena, arena.size, d_off, d_ln, d_v, n, flags=na.RXV_F_TRAILER)
    torch.cuda.synchronize()
    verdict = d_v.cpu().numpy().view(np.uint32)
    assert np.flatnonzero(verdict & na.RXV_FCS_BAD).tolist() == bad
    b = RBatch(inet_oracle, flags=rr.F_TRAILER, verdict=verdict, drop_mask=na.RXV_FCS_BAD, align=4, placed=(arena, off, ln))
    assert b.m == 40 and (b.fstat[bad] == rr.DROPPED).all() and ((b.fstat & rr.INCOMPLETE) != 0).sum() == 40
    t = b.launch_dev(dev)
    torch.cuda.synchronize()
    b.check_dev(b.collect(t))
    # the UDP segments of the reassembled datagrams, checked where they lie
    doff, dlen = b.plan["doff"][:b.m], b.plan["dlen"]
    hl = np.array([(int(b.expect[b.base + int(o)]) & 15) * 4 for o in doff], dtype=np.uint64)
    seg_off, seg_len = doff + hl, (dlen - hl.astype(np.uint32)).astype(np.uint32)
    out = b.expect[b.base:]
    addr = np.array([struct.unpack_from("<II", out, int(o) + 12) for o in doff], dtype=np.uint32)
    d_sum = torch.zeros(b.m, dtype=torch.int16, device=dev)
    na.inet_batch_dev("udp", t["out"].data_ptr() + b.base, b.need, to_dev(seg_off, dev), to_dev(seg_len, dev), to_dev(addr, dev),
                      d_sum, b.m)
    torch.cuda.synchronize()
    want = np.zeros(b.m, dtype=np.uint16)
    out = np.ascontiguousarray(out)
    inet_oracle.oracle_inet_batch(na.INET_MODES["udp"], out.ctypes.data, seg_off.ctypes.data, seg_len.ctypes.data,
                                  addr.ctypes.data, want.ctypes.data, b.m)
    assert np.array_equal(d_sum.cpu().numpy().view(np.uint16), want) and len(set(want.tolist())) > 30


# ---- 7. room and bounds ----
def small_batch(inet_oracle, **kw):
    rng = mg.random.Random(7)
    rb = lambda k: bytes(rng.randrange(256) for _ in range(k))
    frames = [mg.frame(mg.ip_packet(rb(40), ident=1), False)] + mg.fragments(rng, rb(100), [48], False, ident=2)[::-1] + \
             [mg.frame(mg.ip_packet(rb(7), 24, ident=3, rng=rng), False)]
    return RBatch(inet_oracle, frames, 0, **kw)


def test_room_exact_one_short_and_none(dev, inet_oracle):
    full = small_batch(inet_oracle)
    assert full.m == 3 and full.need == 60 + 120 + 31
    for out_bytes, delivered in ((full.need, 3), (full.need - 1, 2), (60 + 119, 1), (59, 0), (0, 0)):
        b = small_batch(inet_oracle, out_bytes=out_bytes, out_base=3)
        heads = b.fstat[b.plan["dlead"]]
        assert ((heads & rr.DELIVERED) != 0).sum() == delivered and ((heads & rr.NO_ROOM) != 0).sum() == 3 - delivered
        b.check(dev)
    with pytest.raises(na.FcsError) as e:
        small_batch(inet_oracle, out_bytes=full.need - 1).run_host()
    assert e.value.rc == -28                                             # -ENOSPC


def test_no_frames_and_null_optional_outputs(dev, inet_oracle):
    b = RBatch(inet_oracle, [], 0)
    r = b.run_dev(dev)
    assert r["counts"].tolist() == [0, 0] and int(r["doff"][0]) == 0 and np.array_equal(r["out"], b.expect)
    assert na.rx_reasm_host(b.arena, 0, b.off, b.ln, 0, b.out0, 0) == 0
    b = small_batch(inet_oracle, align=16)
    b.check_dev(b.run_dev(dev, dlead=False, counts=False, fstat=False), dlead=False, counts=False, fstat=False)
    b.check_dev(b.run_dev(dev, inplace=True))                            # fstat may be pstat itself
    out = b.out0.copy()
    assert na.rx_reasm_host(b.arena, b.arena.size, b.off, b.ln, b.n, out[b.base:], b.out_bytes, align=16) == 3
    assert np.array_equal(out, b.expect)


def test_one_frame_arenas_declared_exactly_as_long_as_the_frame(dev, inet_oracle):
    """The arena is the frame, at an aligned base + 0..3 with random bytes around: loads stay inside
    [floor4(arena), ceil4(end)) whatever the lengths say."""
    rng = mg.random.Random(8)
    rb = lambda k: bytes(rng.randrange(256) for _ in range(k))
    for front in range(4):
        for f in (mg.frame(mg.ip_packet(rb(0)), False, pad=0), mg.frame(mg.ip_packet(rb(1), 60, rng=rng), False, pad=0),
                  mg.frame(mg.ip_packet(rb(61 + front)), True, pad=0), mg.frame(mg.ip_packet(rb(29), foff=mg.MF), False, pad=0),
                  mg.frame(mg.ip_packet(rb(300), ip_len=400), False), rb(33), rb(14), rb(1), b""):
            arena = np.frombuffer(f, dtype=np.uint8) if f else np.zeros(0, dtype=np.uint8)
            for flags in (0, rr.F_TRAILER):
                b = RBatch(inet_oracle, flags=flags, align=1, out_base=front, front=16 + front, back=5,
                           placed=(arena, np.zeros(1, np.uint64), np.array([len(f)], np.uint32)))
                b.check(dev, host=front == 0)


def test_frames_outside_the_arena_are_planned_as_frames_of_no_bytes(dev, inet_oracle):
    """The device plan cannot return -EINVAL for what only a kernel sees: a frame that ends behind the
    arena, starts behind it, or whose off + len wraps is RXR_NOT_IPV4 and nothing of it is read; the
    frames around it are reassembled. The host calls refuse the same batch."""
    b0 = small_batch(inet_oracle)
    n = b0.n
    off = np.concatenate([b0.off, np.array([int(b0.off[1]), b0.arena.size + 1, 2**64 - 8, b0.arena.size], dtype=np.uint64)])
    ln = np.concatenate([b0.ln, np.array([b0.arena.size, 60, 60, 1], dtype=np.uint32)])
    b = RBatch(inet_oracle, flags=0, align=4, placed=(b0.arena, off, ln), front=8, back=4)
    assert b.m == 3 and (b.fstat[n:] == rr.NOT_IPV4).all() and (b.fstat[:n] & rr.DELIVERED).all()
    b.check_dev(b.run_dev(dev))
    with pytest.raises(na.FcsError) as e:
        b.run_host()
    assert e.value.rc == -22 and "frame %d " % n in str(e.value)


def test_two_threads(dev, inet_oracle):
    batches = [scale_batch(inet_oracle, 3000 + 17 * q, 40 + q) for q in range(2)]
    errs = []

    def work(b):
        try:
            torch.cuda.set_device(0)
            s = torch.cuda.Stream()
            for _ in range(4):
                b.check_dev(b.run_dev(dev, stream=s))
                b.check_host()
        except Exception as e:   # noqa: BLE001
            errs.append(e)

    th = [threading.Thread(target=work, args=(b,)) for b in batches]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs, errs
