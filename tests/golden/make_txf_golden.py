"""Generate the TX-framing fixtures (tests/golden/txf_vectors.json, txf_input.bin, txf_frames_<mtu>.bin).

    python tests/golden/make_txf_golden.py

IPv4 datagrams and the frames framing must make of them (include/nstack_txf.h), from an INDEPENDENT
formulation written only for this script: the fragments are cut by slicing, the header checksum is
RFC 1071 over big-endian 16-bit words (make_rxv_golden.py's be_sum / csum), the FCS is zlib.crc32.
It does not use the oracle or the model. tests/test_txf_model.py checks the model
(tests/txf_model.py, which takes its arithmetic from the oracle) against these vectors,
tests/test_gpu_txf.py the kernels.

txf_input.bin holds the datagrams back to back. Every datagram belongs to one mtu;
txf_frames_<mtu>.bin holds that mtu's frames back to back, each with its FCS (F + 4 bytes; without
TXF_F_FCS the first F bytes are what is written). A record: tag, off, len, mtu, flags (TXF_F_HONOR_DF
or 0), mac (hex), status, flen (the list of F), at (offset of its first frame in the frames file).
"""
import importlib.util
import json
import os
import random
import struct
import zlib

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_rxv_golden", os.path.join(HERE, "make_rxv_golden.py"))
rx = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rx)

F_HONOR_DF = 2
WHOLE, FRAGMENTED, BAD_HDR, BAD_LEN, REFRAG, DF_DROP = 0x001, 0x002, 0x004, 0x008, 0x010, 0x020
MTUS = (76, 100, 576, 1500, 9000)
HLENS = tuple(range(20, 64, 4))


def unit(mtu, hlen):
    """Payload bytes of a full fragment: the reference's mtu - hlen - 8, rounded UP to a multiple of 8."""
    u = mtu - hlen - 8
    return u if u % 8 == 0 else u + 8 - u % 8


def datagram(rng, hlen, B, foff=0, vhl=None, ip_len=None):
    D = hlen + B
    opts = bytes(rng.randrange(256) for _ in range(hlen - 20))
    h = struct.pack(">BBHHHBBHII", (0x40 | hlen // 4) if vhl is None else vhl, rng.randrange(256),
                    D if ip_len is None else ip_len, rng.getrandbits(16), foff, 64, 253,   # a protocol without L4 rules
                    rng.getrandbits(16),   # garbage in the checksum field: framing rewrites it
                    rng.getrandbits(32), rng.getrandbits(32)) + opts
    return h + rng.randbytes(B)


def expect(dg, mac, mtu, flags):
    """(status, [F + 4 frame bytes])."""
    D = len(dg)
    if D < 20:
        return BAD_HDR, []
    hlen = (dg[0] & 15) * 4
    if not dg[0] & 0x40 or hlen < 20 or hlen > D:
        return BAD_HDR, []
    if (dg[2] << 8 | dg[3]) != D:
        return BAD_LEN, []
    foff = dg[6] << 8 | dg[7]

    def frame(hdr, pay):
        hdr = bytearray(hdr)
        hdr[10:12] = b"\x00\x00"
        hdr[10:12] = struct.pack(">H", rx.csum(rx.be_sum(bytes(hdr))))
        ip = bytes(hdr) + pay
        if len(ip) < 56:
            ip += bytes(56 - len(ip))
        return rx.with_fcs(mac + b"\x08\x00" + ip)

    if D <= mtu:
        return WHOLE, [frame(dg[:hlen], dg[hlen:])]
    st = (REFRAG if foff & 0x3FFF else 0) | (DF_DROP if flags & F_HONOR_DF and foff & 0x4000 else 0)
    if st:
        return st, []
    u, pay, out, at = unit(mtu, hlen), dg[hlen:], [], 0
    while at < len(pay):
        piece = pay[at:at + u]
        more = at + len(piece) < len(pay)
        hdr = bytearray(dg[:hlen])
        hdr[2:4] = struct.pack(">H", hlen + len(piece))
        hdr[6:8] = struct.pack(">H", (0x2000 if more else 0) | at // 8)
        out.append(frame(hdr, piece))
        at += len(piece)
    return FRAGMENTED, out


def main():
    rng = random.Random(0x7F1A)
    recs, blob = [], bytearray()
    frames = {m: bytearray() for m in MTUS}

    def add(tag, dg, mtu, flags=0):
        mac = rng.randbytes(12)
        st, fr = expect(dg, mac, mtu, flags)
        blob.extend(rng.randbytes(rng.randrange(4)))        # any start alignment
        recs.append({"tag": tag, "off": len(blob), "len": len(dg), "mtu": mtu, "flags": flags, "mac": mac.hex(),
                     "status": st, "flen": [len(f) - 4 for f in fr], "at": len(frames[mtu])})
        blob.extend(dg)
        for f in fr:
            frames[mtu].extend(f)

    for mtu in MTUS:
        hlens = HLENS if mtu <= 576 else (20, 24, 60)
        for hlen in hlens:
            u = unit(mtu, hlen)
            for B in (0, 1, u - 1, u, u + 1, 2 * u, 2 * u + 1):
                add(f"m{mtu}_h{hlen}_B{B}", datagram(rng, hlen, B), mtu)
            for D in (mtu - 1, mtu, mtu + 1):
                add(f"m{mtu}_h{hlen}_D{D}", datagram(rng, hlen, D - hlen), mtu)
        for hlen in (20, 44):                               # last fragments of 1..8 bytes: padded frames
            u = unit(mtu, hlen)
            for t in range(1, 9):
                add(f"m{mtu}_h{hlen}_tail{t}", datagram(rng, hlen, u + t if u + t + hlen > mtu else 2 * u + t), mtu)
        # status-only classes
        add(f"m{mtu}_short", rng.randbytes(19), mtu)
        add(f"m{mtu}_empty", b"", mtu)
        add(f"m{mtu}_v6", datagram(rng, 20, 40, vhl=0x65), mtu)            # (vhl & 0x40) == 0x40: passes, the quirk
        add(f"m{mtu}_novers", datagram(rng, 20, 40, vhl=0x05), mtu)
        add(f"m{mtu}_hl16", datagram(rng, 20, 40, vhl=0x44), mtu)
        add(f"m{mtu}_hl_gt_D", datagram(rng, 20, 4, vhl=0x4F, ip_len=24), mtu)
        add(f"m{mtu}_badlen_lo", datagram(rng, 20, 40, ip_len=59), mtu)
        add(f"m{mtu}_badlen_hi", datagram(rng, 20, mtu, ip_len=61), mtu)
        add(f"m{mtu}_refrag_mf", datagram(rng, 20, mtu, foff=0x2000), mtu)
        add(f"m{mtu}_refrag_off", datagram(rng, 24, mtu, foff=0x0010), mtu)
        add(f"m{mtu}_frag_fits", datagram(rng, 20, 30, foff=0x2007), mtu)   # a fragment that fits: TXF_WHOLE, foff kept
        add(f"m{mtu}_df_frag", datagram(rng, 20, mtu, foff=0x4000), mtu)    # DF without the flag: fragmented, DF cleared
        add(f"m{mtu}_df_drop", datagram(rng, 20, mtu, foff=0x4000), mtu, F_HONOR_DF)
        add(f"m{mtu}_df_fits", datagram(rng, 20, 30, foff=0x4000), mtu, F_HONOR_DF)   # DF kept in a whole frame
        add(f"m{mtu}_df_refrag", datagram(rng, 20, mtu, foff=0x4001), mtu, F_HONOR_DF)
        add(f"m{mtu}_rsv_frag", datagram(rng, 28, mtu, foff=0x8000), mtu)   # the reserved bit is cleared too
    add("max_m76_h60", datagram(rng, 60, 65535 - 60), 76)                   # 8185 frames of 82 bytes
    add("max_m1500_h20", datagram(rng, 20, 65535 - 20), 1500)

    with open(os.path.join(HERE, "txf_input.bin"), "wb") as f:
        f.write(blob)
    for m in MTUS:
        with open(os.path.join(HERE, f"txf_frames_{m}.bin"), "wb") as f:
            f.write(frames[m])
    with open(os.path.join(HERE, "txf_vectors.json"), "w") as f:
        json.dump({"input": "txf_input.bin", "frames": {str(m): f"txf_frames_{m}.bin" for m in MTUS},
                   "datagrams": recs}, f, separators=(",", ":"))
    print(len(recs), "datagrams,", len(blob), "input bytes,", {m: len(frames[m]) for m in MTUS})


if __name__ == "__main__":
    main()
