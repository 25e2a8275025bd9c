"""Frame generator for the RX validator's tail-subtraction and LDS-DMA tests (CPU only, seeded and
deterministic). Built on tests/golden/make_rxv_golden.py (l4_frame, with_fcs, flip, expect).

The L4 sum of both kernels is total - [0, 14 + hlen) - [14 + ip_len, F); a wrong last term shows
only in a frame whose L4 checksum is valid, so `padded` puts non-zero bytes behind a good datagram
and `cut_sweep` moves the cut cl = 14 + ip_len through the frame, each cut with its two one-byte
witnesses. `mixed_fixed` is fixed-length traffic of every verdict class for the fixed-stride
kernels. Test infrastructure only."""
import importlib.util
import os
import random
import struct

import numpy as np

_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_rxv_golden", os.path.join(_GOLDEN, "make_rxv_golden.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

F_TRAILER = gen.F_TRAILER
FCS_BAD, RUNT, IPV4, IP_BAD_HDR, IP_BAD_LEN, IP_BAD_CSUM = 0x001, 0x002, 0x004, 0x008, 0x010, 0x020
FRAG, L4_CHECKED, L4_BAD_CSUM, L4_SHORT = 0x040, 0x080, 0x100, 0x200

KINDS = ("tcp", "udp", "icmp")
PROTO = {"tcp": 6, "udp": 17, "udp0": 17, "icmp": 1}
L4HDR = {"tcp": 20, "udp": 8, "udp0": 8, "icmp": 8}
HLENS = tuple(range(20, 64, 4))   # all eleven header lengths
SWEEP_HLENS = (20, 44)            # 44: the UDP checksum field lies wholly in the second header dword


def clean_verdict(kind, padding):
    """The verdict of a frame that holds a valid `kind` datagram followed by `padding` bytes."""
    return IPV4 | L4_CHECKED | (PROTO[kind] << 16) | (IP_BAD_LEN if padding else 0)


def max_payload(kind, hlen, F, trailer):
    """The longest payload a `kind` datagram with an hlen-byte header can carry in an F-byte frame (< 0: none)."""
    return F - (4 if trailer else 0) - 14 - hlen - L4HDR[kind]


def _nonzero(b):
    return bytes(x or 0xA7 for x in b)


def padded(kind, hlen, payload_len, F, trailer, rng, fill=None):
    """An F-byte frame: a datagram with valid checksums (payload_len payload bytes), then bytes up to
    the frame's end (in front of the FCS when `trailer`) that are random and never zero, or `fill`
    throughout payload and padding. The cut is cl = 14 + hlen + L4HDR[kind] + payload_len."""
    T = 4 if trailer else 0
    payload = rng.randbytes(payload_len) if fill is None else bytes([fill]) * payload_len
    body = gen.l4_frame(kind, payload, hlen, trailer=False, rng=rng)
    npad = F - T - len(body)
    if npad < 0:
        raise ValueError(f"{kind} hlen {hlen} payload {payload_len} does not fit {F} bytes")
    body += _nonzero(rng.randbytes(npad)) if fill is None else bytes([fill]) * npad
    fr = gen.with_fcs(body) if trailer else body
    assert len(fr) == F
    return fr


class Sweep:
    """Frames (bytes, all of one length for cut_sweep and the fixed generators), the verdict each
    must get, and info[i] = (kind, hlen, cl, which)."""

    def __init__(self):
        self.frames, self.expect, self.info = [], [], []

    def add(self, fr, exp, info):
        self.frames.append(fr)
        self.expect.append(exp)
        self.info.append(info)

    def done(self):
        self.expect = np.array(self.expect, dtype=np.uint32)
        return self

    def __len__(self):
        return len(self.frames)

    def matrix(self):
        """The frames as an (n, F) byte matrix (equal lengths only)."""
        F = len(self.frames[0])
        return np.frombuffer(b"".join(self.frames), dtype=np.uint8).reshape(len(self.frames), F)

    def count(self, which):
        return sum(1 for i in self.info if i[3] == which)


def all_payloads(kind, hlen, F, trailer):
    return range(0, max_payload(kind, hlen, F, trailer) + 1)


def cut_sweep(F, trailer, cuts, seed, kinds=KINDS):
    """For each kind, each hlen of SWEEP_HLENS and each payload length of cuts(kind, hlen) (or, when
    `cuts` is a set of frame positions, each cl in it that the kind and hlen admit): the clean padded
    frame, a copy with frame byte cl - 1 bent (the segment's last byte) and, when there is padding,
    a copy with frame byte cl bent (the first byte behind the segment), each with the verdict it
    must get by construction. A change inside one byte never leaves a one's-complement sum
    unchanged, so the two copies are the +-1-byte witnesses of the tail mask."""
    rng = random.Random(seed)
    fcs = FCS_BAD if trailer else 0
    T = 4 if trailer else 0
    out = Sweep()
    for kind in kinds:
        for hlen in SWEEP_HLENS:
            top = max_payload(kind, hlen, F, trailer)
            base = 14 + hlen + L4HDR[kind]
            if callable(cuts):
                pls = [n for n in cuts(kind, hlen) if 0 <= n <= top]
            else:
                pls = [cl - base for cl in sorted(cuts) if 0 <= cl - base <= top]
            for n in pls:
                cl = base + n
                while True:
                    fr = padded(kind, hlen, n, F, trailer, rng)
                    # without payload cl - 1 is the UDP checksum field's low byte: a field of 0x005A
                    # would be bent to zero, "none sent"
                    if not (kind == "udp" and n == 0 and fr[14 + hlen + 6] == 0 and fr[14 + hlen + 7] == 0x5A):
                        break
                pad = F - T - cl
                clean = clean_verdict(kind, pad)
                out.add(fr, clean, (kind, hlen, cl, "clean"))
                out.add(gen.flip(fr, cl - 1), clean | L4_BAD_CSUM | fcs, (kind, hlen, cl, "last"))
                if pad:
                    out.add(gen.flip(fr, cl), clean | fcs, (kind, hlen, cl, "behind"))
    return out.done()


def cut_positions(sweep):
    """The set of (kind, hlen, cl) a sweep holds."""
    return {(k, h, cl) for k, h, cl, _ in sweep.info}


def segment_cuts(F, seed, near=100, nrandom=500):
    """Cut positions for a multi-segment length: every cl within `near` bytes of each F - 1536 k
    (the segment borders, counted from the frame end as the kernels do), within `near` bytes of
    F - 96 j for j = 0..3 (the end lanes' chunk borders), and `nrandom` seeded random ones."""
    rng = random.Random(seed)
    cuts = set()
    for k in range((F + 1535) // 1536 + 1):
        cuts.update(range(F - 1536 * k - near, F - 1536 * k + near + 1))
    for j in range(4):
        cuts.update(range(F - 96 * j - near, F - 96 * j + near + 1))
    cuts.update(rng.randrange(0, F + 1) for _ in range(nrandom))
    return {c for c in cuts if 0 <= c <= F}


# The sweeps of tests/test_gpu_rxv_cuts.py (tests/test_rxv_traffic.py checks the same frames on the CPU).
DMA_LENGTHS = (1496, 1497, 1517, 1518, 1524)   # every cut through the LDS-DMA kernel
FULL_LENGTHS = (1518, 1497, 60, 64)            # every cut through the general kernel
SEG_LENGTHS = (1600, 3072, 3073, 9018)         # multi-segment: the cuts of segment_cuts()


def full_sweep(F, trailer):
    """Every cut an F-byte frame admits."""
    return cut_sweep(F, trailer, lambda kind, hlen: all_payloads(kind, hlen, F, trailer), seed=2 * F + trailer)


def seg_sweep(F, trailer, kind):
    """One kind's frames at the cuts of segment_cuts(F)."""
    return cut_sweep(F, trailer, segment_cuts(F, seed=F), seed=2 * F + trailer, kinds=(kind,))


def quirk_frames(F, trailer):
    """Valid datagrams whose payload and padding are 0x00 or 0xFF throughout (tail sums of 0 and of a
    non-zero multiple of 0xffff), and the all-zero ICMP message (the reference's 0xffff accumulator
    start accepts it) in front of both paddings."""
    rng = random.Random(0x51 + F + trailer)
    T = 4 if trailer else 0
    out = Sweep()
    for fill in (0x00, 0xFF):
        for kind in KINDS:
            for n in (0, 1, 2, 101, 700):
                if max_payload(kind, 20, F, trailer) < n:
                    continue
                cl = 34 + L4HDR[kind] + n
                out.add(padded(kind, 20, n, F, trailer, rng, fill=fill), clean_verdict(kind, F - T - cl),
                        (kind, 20, cl, f"fill{fill:02x}"))
        body = gen.frame(gen.ip_header(1, 8) + bytes(8), trailer=False)
        body += bytes([fill]) * (F - T - len(body))
        out.add(gen.with_fcs(body) if trailer else body, clean_verdict("icmp", F - T - 42), ("icmp", 20, 42, f"zeros{fill:02x}"))
    return out.done()


def variable_mix(n, trailer, seed):
    """n padded frames of seeded random lengths 60..1518 (5 %: 1537..9018), a random kind, hlen over
    all eleven values and a random cut, with their constructed verdicts."""
    rng = random.Random(seed)
    T = 4 if trailer else 0
    out = Sweep()
    for i in range(n):
        F = rng.randrange(1537, 9019) if rng.random() < 0.05 else rng.randrange(60, 1519)
        kind = rng.choice(KINDS)
        fits = [h for h in HLENS if max_payload(kind, h, F, trailer) >= 0]
        hlen = fits[i % len(fits)]
        top = max_payload(kind, hlen, F, trailer)
        r = rng.random()   # cuts near the frame's end as often as anywhere else
        pl = top - rng.randrange(0, min(top, 200) + 1) if r < 0.5 else rng.randrange(0, top + 1)
        cl = 14 + hlen + L4HDR[kind] + pl
        out.add(padded(kind, hlen, pl, F, trailer, rng), clean_verdict(kind, F - T - cl), (kind, hlen, cl, "clean"))
    return out.done()


# ---- fixed-length traffic of every verdict class ----
def _fit_hlen(kind, hlen, F, trailer):
    """The largest header length <= hlen whose `kind` datagram fits the frame; None when none does."""
    while hlen >= 20 and max_payload(kind, hlen, F, trailer) < 0:
        hlen -= 4
    return hlen if hlen >= 20 else None


def _forced_random(F, T, rng):
    """Random bytes with forced header fields (tests/test_gpu_rxv.py's random_frames), F bytes."""
    b = bytearray(rng.randbytes(F))
    if F >= 14 and rng.random() < 0.9:
        b[12:14] = b"\x08\x00"
    if F > 14:
        b[14] = rng.choice([0x45, 0x45, 0x46, 0x4A, 0x4F, 0x44, 0x35, 0x65])
    if F > 23:
        b[23] = rng.choice([6, 6, 17, 17, 1, 47])
    if F > 21 and rng.random() < 0.85:
        b[20:22] = bytes([rng.choice([0x00, 0x40]), 0])
    if F > 17:
        P = max(F - 14 - T, 0)
        hl = (b[14] & 15) * 4
        ipl = [P, P, P + 4, max(P - rng.randrange(0, 50), 0), hl, max(hl - 1, 0), hl + rng.randrange(0, 24),
               rng.randrange(0, 65536)][rng.randrange(0, 8)]
        b[16:18] = (ipl & 0xFFFF).to_bytes(2, "big")
    q = 14 + (b[14] & 15) * 4 + 6 if F > 14 else F
    if q + 2 <= F and rng.random() < 0.2:
        b[q:q + 2] = b"\x00\x00"
    return bytes(b)


def _mixed_body(cls, k, F, trailer, rng):
    """The body (F - T bytes, no FCS) of class `cls`, variant counter k; None when the class does
    not fit the length."""
    T = 4 if trailer else 0
    P = F - 14 - T
    kind = KINDS[(k + cls) % 3]
    full = lambda kd, h, **kw: gen.l4_frame(kd, rng.randbytes(max_payload(kd, h, F, trailer)), h, trailer=False,   # noqa: E731
                                            rng=rng, **kw)
    if cls in (0, 11):      # a valid datagram, a random cut, non-zero bytes behind it
        h = _fit_hlen(kind, HLENS[rng.randrange(11)], F, trailer)
        if h is None:
            return None
        return padded(kind, h, rng.randrange(0, max_payload(kind, h, F, trailer) + 1), F - T, False, rng)
    if cls == 1:            # a datagram that fills the frame, hlen over all eleven values
        h = _fit_hlen(kind, HLENS[k % 11], F, trailer)
        return None if h is None else full(kind, h)
    if cls == 2:            # UDP without a checksum
        h = _fit_hlen("udp0", HLENS[k % 11], F, trailer)
        return None if h is None else full("udp0", h)
    if cls in (3, 4):       # fragments (MF, a non-zero offset, both); DF only
        h = _fit_hlen(kind, 20 if k % 2 else 24, F, trailer)
        foff = 0x4000 if cls == 4 else (0x2000, 0x00B9, 0x2001, 0x5FFF)[k % 4]
        return None if h is None else full(kind, h, foff=foff)
    if cls == 5:            # not IPv4
        h = _fit_hlen(kind, 20, F, trailer)
        if h is None:
            return None
        b = bytearray(full(kind, h))
        b[12:14] = struct.pack(">H", (0x0806, 0x8100, 0x86DD)[k % 3])
        return bytes(b)
    if cls == 6:            # bad header shapes; hlen > P cannot happen at these lengths: hlen 60 over ip_len 59
        h = _fit_hlen(kind, 60 if k % 4 == 3 else 20, F, trailer)
        if h is None:
            return None
        if k % 4 == 3:
            return full(kind, h, ip_len=h - 1)
        b = bytearray(full(kind, h))
        b[14] = (0x35, 0x44, 0x4F)[k % 4]
        return bytes(b)
    if cls == 7:            # ip_len against P and hlen, for all three protocols
        h = _fit_hlen(kind, HLENS[(k // 3) % 11], F, trailer)
        if h is None:
            return None
        return full(kind, h, ip_len=(P + 1, h, h - 1, h + 3, 0)[(k // 3) % 5])
    if cls == 8:            # a protocol without an L4 checksum
        return gen.frame(gen.ip_header((47, 2, 132, 0, 255)[k % 5], P - 20, rng=rng) + rng.randbytes(P - 20), trailer=False,
                         rng=rng) if P >= 20 else None
    if cls == 9:            # one-byte corruptions, region by region (applied by the caller: the FCS comes first)
        h = _fit_hlen(kind, HLENS[k % 11], F, trailer)
        if h is None:
            return None
        top = max_payload(kind, h, F, trailer)
        return padded(kind, h, max(top - rng.randrange(0, 40), 0), F - T, False, rng)
    return _forced_random(F - T, 0, rng)   # cls 10


MIXED_CLASSES = 13   # odd: every class meets every i mod 4 within 52 frames


def mixed_fixed(F, n, trailer, seed):
    """n frames of exactly F bytes (F >= 38) that cycle through the verdict classes, each class at
    every i mod 4 (the LDS-DMA item's quarter). Expectations are the model's (rxv_model.verdicts)."""
    rng = random.Random(seed)
    T = 4 if trailer else 0
    start = rng.randrange(MIXED_CLASSES)
    frames = []
    for i in range(n):
        cls, k = (i + start) % MIXED_CLASSES, (i + start) // MIXED_CLASSES
        if cls == 12:       # random bytes with forced fields, trailer and all
            frames.append(_forced_random(F, T, rng))
            continue
        body = _mixed_body(cls, k, F, trailer, rng)
        bend = cls == 9 and body is not None
        if body is None:
            body = _forced_random(F - T, 0, rng)
        assert len(body) == F - T, (cls, k, len(body))
        fr = gen.with_fcs(body) if trailer else body
        if bend:
            hlen = (fr[14] & 15) * 4
            cl = 14 + ((fr[16] << 8) | fr[17])
            region = k % 7
            pos = (k % 12, 14 + k % hlen, 14 + hlen, (14 + hlen + cl) // 2, cl - 1,
                   F - 1 - k % 4, cl + k % max(F - T - cl, 1))[region]
            fr = gen.flip(fr, min(pos, F - 1))
        frames.append(fr)
    return frames


def tiny_fixed(F, n, seed):
    """n frames of F < 38 random bytes, the ethertype forced where it fits."""
    rng = random.Random(seed)
    frames = []
    for i in range(n):
        b = bytearray(rng.randbytes(F))
        if F >= 14 and i % 4 != 3:
            b[12:14] = b"\x08\x00"
        if F > 14 and i % 2:
            b[14] = 0x45
        frames.append(bytes(b))
    return frames
