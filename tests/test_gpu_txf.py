"""GPU tests of one-pass TX framing (include/nstack_txf.h) through the C ABI. For every batch the
device form (after ether_tx_frame_plan_dev) and the host form must leave byte-identical output
arenas, equal to the model's (tests/txf_model.py: the header's rules with the oracle's CRC and
checksum) and to the independently generated golden vectors. The output arena is canary bytes
before, between and behind the slots and is compared as a whole, so a write to any byte other than
a produced frame's fails the test; flen, fcs, status and first are compared with the model too."""
import struct
import threading

import numpy as np
import pytest

import nstack_amd as na
import rxv_model as rm
import txf_model as fm
from txf_batch import FCS, UNSET, Batch, datagram, frames_fn, to_dev

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
def txf_golden():
    return fm.load_golden()


# ---- the golden vectors, at datagram start alignments 0..3 and out base alignments 0..3 ----
@pytest.mark.parametrize("mtu", [76, 100, 576, 1500, 9000])
def test_golden_vectors(dev, oracle, inet_oracle, txf_golden, mtu):
    a = txf_golden["input_bytes"]
    for flags in (0, fm.F_HONOR_DF):
        recs = [r for r in txf_golden["datagrams"] if r["mtu"] == mtu and r["flags"] == flags]
        dgs = [a[r["off"]:r["off"] + r["len"]] for r in recs]
        l2 = np.array([list(bytes.fromhex(r["mac"])) for r in recs], dtype=np.uint8)
        want = txf_golden["frame_bytes"][mtu]
        for base in range(4):
            b = Batch(oracle, inet_oracle, dgs, mtu, FCS | flags, base=base, seed=10 + base, l2=l2,
                      aligns=[(i + base) & 3 for i in range(len(dgs))])
            # the model's arena holds exactly the golden frames
            for i, r in enumerate(recs):
                assert b.status[i] == r["status"], r["tag"]
                at, k = r["at"], int(b.plan_first[i])
                for q, F in enumerate(r["flen"]):
                    o = b.base + (k + q) * b.slot
                    assert b.expect[o:o + F + 4].tobytes() == want[at:at + F + 4], (r["tag"], q)
                    at += F + 4
            b.check(dev, host=base == 0)


# ---- alignment sweep ----
def sweep_lengths(mtu, hlen):
    mx = fm.frag_unit(mtu, hlen)
    top = 3 * mx + 9
    return list(range(0, top + 1)) if top < 400 else list(range(0, top + 1, 41)) + [mx - 1, mx, mx + 1, 2 * mx, top]


def alignment_sweep(dev, oracle, inet_oracle, mtu, extra, flags):
    rng = np.random.default_rng(100 + mtu)
    dgs, res = [], set()
    T = 4 if flags & FCS else 0
    for hlen in (20, 24, 60):
        for B in sweep_lengths(mtu, hlen):
            dgs.append(datagram(rng, hlen, B))
            for F in (len(f) - T for f in frames_fn(oracle, inet_oracle, dgs[-1], bytes(12), mtu, flags)[1]):
                res.add(F % 96)
    # every residue mod 96 of F (at mtu 100 every F there is: 70..114)
    assert res == (set(range(96)) if mtu == 1500 else {F % 96 for F in range(70, 115)})
    dgs += [datagram(rng, hlen, mtu - hlen) for hlen in (20, 24, 60)]      # whole frames of 14 + mtu, in a row
    b = Batch(oracle, inet_oracle, dgs, mtu, flags, slot=fm.min_slot(mtu, flags) + extra, seed=3)
    if extra:   # every source-to-destination distance mod 4 occurs within the batch
        dist = set()
        for i in range(b.n):
            dist.add((int(b.off[i]) - (b.base + int(b.plan_first[i]) * b.slot)) & 3)
        assert dist == {0, 1, 2, 3}
    if not T and not extra:   # full frames in consecutive slots: a frame's last byte abuts the next one's first
        full = b.flen[:b.total] == b.slot
        assert (full[:-1] & full[1:]).sum() >= 2
    b.check(dev, host=extra in (0, 3))


@pytest.mark.parametrize("extra", [0, 1, 2, 3])
@pytest.mark.parametrize("mtu", [100, 1500])
def test_alignment_sweep(dev, oracle, inet_oracle, mtu, extra):
    alignment_sweep(dev, oracle, inet_oracle, mtu, extra, FCS)


@pytest.mark.parametrize("extra", [0, 1, 2, 3])
@pytest.mark.parametrize("mtu", [100, 1500])
def test_alignment_sweep_without_fcs(dev, oracle, inet_oracle, mtu, extra):
    """txf_kernel<false>: the tail store is the up to three bytes behind the last whole dword alone."""
    alignment_sweep(dev, oracle, inet_oracle, mtu, extra, 0)


# ---- segment borders ----
BORDER_MTUS = list(range(1528, 1580, 4)) + [3072, 3100, 9000]


def segment_borders(dev, oracle, inet_oracle, mtu, flags):
    rng = np.random.default_rng(mtu)
    dgs = [datagram(rng, hlen, 2 * mtu + 5 - hlen) for hlen in (20, 24, 60)]
    dgs += [datagram(rng, 20, mtu - 20), datagram(rng, 28, mtu - 29)]      # whole frames of 14 + mtu and one less
    for slot_extra in (0, 1):
        Batch(oracle, inet_oracle, dgs, mtu, flags, slot=fm.min_slot(mtu, flags) + slot_extra, seed=mtu).check(dev)


@pytest.mark.parametrize("mtu", BORDER_MTUS)
def test_segment_borders(dev, oracle, inet_oracle, mtu):
    segment_borders(dev, oracle, inet_oracle, mtu, FCS)


@pytest.mark.parametrize("mtu", BORDER_MTUS)
def test_segment_borders_without_fcs(dev, oracle, inet_oracle, mtu):
    segment_borders(dev, oracle, inet_oracle, mtu, 0)


# ---- extremes ----
def test_largest_datagram_at_the_smallest_mtu(dev, oracle, inet_oracle):
    rng = np.random.default_rng(5)
    b = Batch(oracle, inet_oracle, [datagram(rng, 60, 65535 - 60)], 76, FCS, slot=95)
    assert b.total == 8185
    b.check(dev)


def test_largest_datagram_at_mtu_1500(dev, oracle, inet_oracle):
    rng = np.random.default_rng(6)
    b = Batch(oracle, inet_oracle, [datagram(rng, 20, 65535 - 20)], 1500, FCS, slot=1519)
    assert b.total == 45
    b.check(dev)


def test_load_imbalance_mix(dev, oracle, inet_oracle):
    rng = np.random.default_rng(7)
    dgs = []
    for i in range(70):
        dgs.append(datagram(rng, 20, 65535 - 20) if i % 23 == 5 else datagram(rng, 20, 0))
    Batch(oracle, inet_oracle, dgs, 1500, FCS, slot=1521).check(dev)


# ---- status ----
def status_batch(rng, mtu):
    good = lambda: datagram(rng, 20, int(rng.integers(0, 3 * mtu)))
    return [good(), rng.integers(0, 256, 19, dtype=np.uint8).tobytes(), good(), b"", good(),
            datagram(rng, 20, 40, vhl=0x05), good(), datagram(rng, 20, 40, vhl=0x44), good(),
            datagram(rng, 20, 4, vhl=0x4F, ip_len=24), good(), datagram(rng, 20, 40, ip_len=59), good(),
            datagram(rng, 20, mtu, foff=0x2000), good(), datagram(rng, 24, mtu, foff=0x0010), good(),
            datagram(rng, 20, mtu, foff=0x4000), good(), datagram(rng, 20, mtu, foff=0x4001), good(),
            datagram(rng, 20, 30, foff=0x4000), datagram(rng, 20, 30, foff=0x2007), datagram(rng, 28, mtu, foff=0x8000), good()]


@pytest.mark.parametrize("flags", [FCS, FCS | fm.F_HONOR_DF, 0, fm.F_HONOR_DF])
def test_status_classes_between_neighbours(dev, oracle, inet_oracle, flags):
    """Every status-only class between datagrams that become frames; TXF_F_HONOR_DF on and off; without
    TXF_F_FCS the four bytes behind each frame keep their canary (the whole arena is compared)."""
    rng = np.random.default_rng(8)
    b = Batch(oracle, inet_oracle, status_batch(rng, 1500), 1500, flags, slot=1521, spare=2)
    seen = int(np.bitwise_or.reduce(b.status))
    want = fm.WHOLE | fm.FRAGMENTED | fm.BAD_HDR | fm.BAD_LEN | fm.REFRAG | (fm.DF_DROP if flags & fm.F_HONOR_DF else 0)
    assert seen == want
    b.check(dev)


def test_no_room_for_the_last_datagram_only(dev, oracle, inet_oracle):
    rng = np.random.default_rng(9)
    dgs = [datagram(rng, 20, 3000), datagram(rng, 20, 100), datagram(rng, 24, 4000)]
    full = Batch(oracle, inet_oracle, dgs, 1500, FCS)
    b = Batch(oracle, inet_oracle, dgs, 1500, FCS, slots=full.total - 1)
    assert list(b.status) == [fm.FRAGMENTED, fm.WHOLE, fm.FRAGMENTED | fm.NO_ROOM]
    b.check(dev)
    with pytest.raises(na.FcsError) as e:
        b.run_host()
    assert "ENOSPC" in str(e.value)
    # a first[] that points past the slots
    b2 = Batch(oracle, inet_oracle, dgs, 1500, FCS, slots=4, first=[0, 3, 1 << 40], spare=0)
    assert list(b2.status) == [fm.FRAGMENTED, fm.WHOLE, fm.FRAGMENTED | fm.NO_ROOM]
    out, flen, fcs, st, _, _ = b2.run_dev(dev)
    assert (out == b2.expect).all() and (st == b2.status).all() and (flen == b2.flen).all()


def test_one_l2_record_for_the_batch(dev, oracle, inet_oracle):
    rng = np.random.default_rng(11)
    dgs = [datagram(rng, 20 + 4 * (i % 3), int(rng.integers(0, 4000))) for i in range(40)]
    per = Batch(oracle, inet_oracle, dgs, 1500, FCS, seed=4)
    one = Batch(oracle, inet_oracle, dgs, 1500, FCS | fm.F_L2_ONE, seed=4, l2=per.l2)
    same = Batch(oracle, inet_oracle, dgs, 1500, FCS, seed=4, l2=np.repeat(per.l2[:1], 40, axis=0))
    assert (one.expect == same.expect).all() and not (one.expect == per.expect).all()
    one.check(dev)
    per.check(dev)
    # a single record is all the one-record form may read
    one.l2 = per.l2[:1].copy()
    one.check(dev)


# ---- plan ----
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 65537])
def test_plan_prefix_sums(dev, n):
    rng = np.random.default_rng(n)
    D = rng.integers(20, 6000, n).astype(np.uint32)
    D[rng.integers(0, 10, n) == 0] = 7                       # refused ones in between
    off = np.arange(n, dtype=np.uint64) * 8                  # headers only, 8 bytes apart
    arena = np.zeros(8 * n + 8, dtype=np.uint8)
    for i in range(n):                                        # the 8 bytes the plan reads
        arena[8 * i:8 * i + 8] = np.frombuffer(struct.pack(">BBHHH", 0x45, 0, int(D[i]), 0, 0), dtype=np.uint8)
    cnt = np.array([na.tx_frame_count(int(d), 20, 1500) for d in D], dtype=np.uint64)
    want = np.zeros(n + 1, dtype=np.uint64)
    want[1:] = np.cumsum(cnt)
    d_first = torch.full((n + 1,), -1, dtype=torch.int64, device=dev)
    d_st = torch.full((max(n, 1),), -1, dtype=torch.int32, device=dev)
    # the arena is declared as large as the datagrams claim: only their first 8 bytes are read
    big = to_dev(np.concatenate([arena, np.zeros(6000, dtype=np.uint8)]), dev)
    na.tx_frame_plan_dev(big, big.numel(), to_dev(off, dev) if n else None, to_dev(D, dev) if n else None, n, 1500,
                         d_first, 0, d_st)
    torch.cuda.synchronize()
    assert (d_first.cpu().numpy().view(np.uint64) == want).all()
    st = d_st.cpu().numpy().view(np.uint32)[:n]
    assert (st == np.where(D < 20, fm.BAD_HDR, np.where(D <= 1500, fm.WHOLE, fm.FRAGMENTED))).all()


def test_hand_made_first_with_gaps(dev, oracle, inet_oracle):
    rng = np.random.default_rng(12)
    dgs = [datagram(rng, 20, 3000), datagram(rng, 20, 10), rng.integers(0, 256, 5, dtype=np.uint8).tobytes(),
           datagram(rng, 44, 1500)]
    # counts 3, 1, 0, 2: slots out of order, with unused slots between them
    b = Batch(oracle, inet_oracle, dgs, 1500, FCS, slot=1523, slots=12, first=[7, 1, 0, 3])
    assert (b.flen != UNSET).sum() == 6
    out, flen, fcs, st, _, pst = b.run_dev(dev)
    assert (out == b.expect).all() and (flen == b.flen).all() and (fcs == b.fcs).all() and (st == b.status).all()
    assert (pst == b.status).all()


# ---- composition with the other one-pass entry points ----
def test_built_frames_pass_the_validator_and_the_fcs_check(dev, oracle, inet_oracle):
    rng = np.random.default_rng(13)
    dgs = [datagram(rng, 20 + 4 * (i % 11), int(rng.integers(0, 5000))) for i in range(60)]
    dgs += [datagram(rng, 20, 1472 * 2 + t) for t in range(1, 9)]          # padded last fragments
    b = Batch(oracle, inet_oracle, dgs, 1500, FCS, slot=1525)
    out = b.run_dev(dev)[0]
    k = b.total
    off = np.arange(k, dtype=np.uint64) * b.slot + b.base
    ln = b.flen[:k] + 4
    d_out, d_off, d_ln = to_dev(out, dev), to_dev(off, dev), to_dev(ln, dev)
    d_v = torch.zeros(k, dtype=torch.int32, device=dev)
    na.rx_validate_dev(d_out, out.size, d_off, d_ln, d_v, k, na.RXV_F_TRAILER)
    d_ok = torch.zeros(k, dtype=torch.uint8, device=dev)
    d_bad = torch.ones(1, dtype=torch.int64, device=dev)
    na.verify_dev(d_out, out.size, d_off, d_ln, d_ok, d_bad, k)
    torch.cuda.synchronize()
    v = d_v.cpu().numpy().view(np.uint32)
    padded = 0
    for q in range(k):
        f = out[int(off[q]):int(off[q]) + int(ln[q])].tobytes()
        want = rm.IPV4 | (253 << rm.PROTO_SHIFT)
        if int.from_bytes(f[20:22], "big") & 0x3FFF:
            want |= rm.FRAG
        if int.from_bytes(f[16:18], "big") < 56:
            want |= rm.IP_BAD_LEN
            padded += 1
        assert v[q] == want, (q, hex(v[q]), hex(want))
    assert padded >= 8
    assert int(d_bad.item()) == 0 and bool(d_ok.all())


def test_sealing_whole_udp_frames_changes_nothing(dev, oracle, inet_oracle):
    """TXF_WHOLE frames of UDP datagrams whose checksum is in place: ether_tx_seal_dev finds the same
    IP checksum and FCS and leaves the arena as it is."""
    rng = np.random.default_rng(14)
    dgs = []
    for i in range(48):
        hlen, L = 20 + 4 * (i % 4), 8 + int(rng.integers(0, 1400))
        d = bytearray(datagram(rng, hlen, L, proto=17, foff=0x4000 if i & 1 else 0))
        d[hlen + 4:hlen + 6] = L.to_bytes(2, "big")
        d[hlen + 6:hlen + 8] = b"\x00\x00"
        src_raw, dst_raw = struct.unpack_from("<II", d, 12)
        c = inet_oracle.oracle_udp_checksum(bytes(d[hlen:]), L, src_raw, dst_raw) or 0xFFFF
        d[hlen + 6:hlen + 8] = struct.pack("<H", c)
        dgs.append(bytes(d))
    b = Batch(oracle, inet_oracle, dgs, 1500, FCS, slot=1520)
    assert (b.status == fm.WHOLE).all()
    out = b.run_dev(dev)[0]
    assert (out == b.expect).all()
    k = b.total
    d_out = to_dev(out, dev)
    d_off = to_dev(np.arange(k, dtype=np.uint64) * b.slot + b.base, dev)
    d_st = torch.zeros(k, dtype=torch.int32, device=dev)
    na.tx_seal_dev(d_out, out.size, d_off, to_dev(b.flen[:k], dev), k, na.TXS_F_FCS, status=d_st)
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy() == out).all()
    st = d_st.cpu().numpy().view(np.uint32)
    assert ((st & (na.TXS_IP_CSUM_SET | na.TXS_L4_CSUM_SET | na.TXS_FCS_SET)) ==
            (na.TXS_IP_CSUM_SET | na.TXS_L4_CSUM_SET | na.TXS_FCS_SET)).all()


# ---- calls ----
def test_optional_outputs_may_be_null_and_last_launch(dev, oracle, inet_oracle):
    rng = np.random.default_rng(15)
    dgs = [datagram(rng, 20, int(rng.integers(0, 4000))) for _ in range(20)]
    for flags, name in ((FCS, "general-fcs"), (0, "general")):
        b = Batch(oracle, inet_oracle, dgs, 1500, flags, slot=1522)
        out, flen, fcs, st, _, _ = b.run_dev(dev, flen=False, status=False, fcs=False)
        assert (out == b.expect).all()
        assert (flen == UNSET).all() and (fcs == UNSET).all() and (st == 0xFFFFFFFF).all()
        assert na.txf_last_launch() == name
        out, flen, fcs, st, _, _ = b.run_dev(dev, status=False)
        assert (out == b.expect).all() and (flen == b.flen).all() and (fcs == b.fcs).all()
    # n == 0: nothing to do, first[0] = 0
    d_first = torch.full((1,), -1, dtype=torch.int64, device=dev)
    na.tx_frame_plan_dev(None, 0, None, None, 0, 1500, d_first)
    na.tx_frame_dev(None, 0, None, None, None, 0, 1500, d_first, None, 1518, 0)
    torch.cuda.synchronize()
    assert int(d_first.item()) == 0
    assert na.tx_frame_host(None, 0, None, None, None, 0, 1500, None, 1518, 0) == 0


def test_two_threads_on_two_streams(dev, oracle, inet_oracle):
    rng = np.random.default_rng(16)
    batches = [Batch(oracle, inet_oracle, [datagram(rng, 20 + 4 * t, int(rng.integers(0, 6000))) for _ in range(64)],
                     1500 if t == 0 else 576, FCS, seed=20 + t) for t in range(2)]
    res, err = [None, None], []

    def work(t):
        try:
            torch.cuda.set_device(0)
            s = torch.cuda.Stream()
            for _ in range(3):
                res[t] = batches[t].run_dev(dev, stream=s)
        except Exception as e:   # noqa: BLE001
            err.append(e)

    th = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not err, err
    for t in range(2):
        out, flen, fcs, st, first, _ = res[t]
        assert (out == batches[t].expect).all() and (flen == batches[t].flen).all()
        assert (st == batches[t].status).all() and (first == batches[t].plan_first).all()
