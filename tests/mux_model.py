"""Expected-result model of one-pass TX multiplexing: the rule list of include/nstack_mux.h restated over
Python lists and `struct`. Sockets are (key, tcb, records); the model walks them in send order, as the
reference's nstack_udp_send / nstack_tcp_send -> ip_send would, one call per record. Test
infrastructure only."""
import json
import os
import struct

import numpy as np

BAD_REC, BAD_SIZE, NO_TCB, NO_ROUTE, NO_NEIGH, PLANNED, NO_ROOM, BUILT = 0x01, 0x02, 0x04, 0x08, 0x10, 0x20, 0x40, 0x80
REC_HDR, IMG = 24, 40
UDP_MAX, TCP_MAX = 65506, 65495
MAX_SOCKS, MAX_ROUTES, MAX_NEIGH = 65536, 256, 65536
PSH_ACK = 0x18


def key(proto: int, port: int, addr: int) -> int:
    return (proto << 48) | (port << 32) | addr


def key_valid(k: int) -> bool:
    return (k >> 48) in (6, 17)


def record(dst: int, dport: int, payload: bytes, src=0x7F000001, sport=0x7777, size=None) -> bytes:
    """struct nstack_dgram on LP64 (nstack_dmx.h rule 6). srcaddr is not used by any rule."""
    return struct.pack("<IiIiQ", src, sport, dst, dport, len(payload) if size is None else size) + payload


def route(network, netmask, iface, mac, gw=0):
    return dict(network=network, netmask=netmask, gw=gw, iface=iface, mac=bytes(mac))


def route_find(rt, dst):
    """ip_route_find_by_network (src/ip_route.c:132-166) over the table in the caller's order."""
    for i, r in enumerate(rt):
        if r["network"] == dst:
            return i
    for i, r in enumerate(rt):
        if r["network"] == (dst & r["netmask"]):
            return i
    for i, r in enumerate(rt):
        if r["network"] == 0:
            return i
    return None


def ip_checksum(hdr: bytes) -> int:
    s = sum(struct.unpack(f">{len(hdr) // 2}H", hdr))
    while s >> 16:
        s = (s & 0xFFFF) + (s >> 16)
    return ~s & 0xFFFF


def headers(proto, P, ident, src, dst, sport, dport, tcb=None, seq=0) -> bytes:
    """Rule 5: the finished IP and L4 header, the L4 checksum field left 0."""
    hl = 28 if proto == 17 else 40
    ip = struct.pack(">BBHHHBBHII", 0x45, 0, hl + P, ident & 0xFFFF, 0x4000, 64, proto, 0, src, dst)
    ip = ip[:10] + struct.pack(">H", ip_checksum(ip)) + ip[12:]
    if proto == 17:
        return ip + struct.pack(">HHHH", sport, dport, 8 + P, 0)
    return ip + struct.pack(">HHIIBBHHH", sport, dport, seq & 0xFFFFFFFF, tcb[1], 0x50, tcb[3], tcb[2], 0, 0)


def plan(q, q_bytes, rec, sfirst, bind, tcb, rt, nb, id0=0, align=16):
    """q: uint8 array; rec: offsets; sfirst: S + 1 entries; bind: keys; tcb: None or a list of
    (seq, ack, win, flags) per socket; rt: route() dicts; nb: (addr, mac, valid) tuples."""
    n, S = len(rec), len(bind)
    assert len(sfirst) == S + 1 and (S == 0 or (sfirst[0] == 0 and sfirst[S] == n)) and align in (4, 8, 16, 32, 64, 128)
    lowest = {}
    for i, (addr, mac, valid) in enumerate(nb):
        if valid:
            lowest.setdefault(addr, i)                                    # an address belongs to its lowest index
    mstat, off, ln = np.zeros(n, np.uint32), np.zeros(n, np.uint64), np.zeros(n, np.uint32)
    l2, himg = np.zeros((n, 12), np.uint8), np.zeros((n, IMG), np.uint8)
    tnext, dgs = np.zeros(S, np.uint32), {}
    at = planned = 0
    for s in range(S):
        k_ = int(bind[s])
        proto, sport = k_ >> 48, (k_ >> 32) & 0xFFFF
        tcp = key_valid(k_) and proto == 6
        sent = 0
        for k in range(int(sfirst[s]), int(sfirst[s + 1])):
            off[k] = at
            r = int(rec[k])
            if r % 8 or r + REC_HDR > q_bytes or not key_valid(k_):       # rule 1
                mstat[k] = BAD_REC
                continue
            _, _, dst, dport, P = struct.unpack_from("<IiIiQ", q, r)
            if r + REC_HDR + P > q_bytes or not 0 <= dport <= 0xFFFF:
                mstat[k] = BAD_REC
                continue
            st = 0                                                        # rule 2
            if (proto == 17 and not 0 < P < 65507) or (proto == 6 and P > TCP_MAX):
                st |= BAD_SIZE
            if tcp and tcb is None:
                st |= NO_TCB
            if st:
                mstat[k] = st
                continue
            ri = route_find(rt, dst)                                      # rule 3
            if ri is None:
                mstat[k] = NO_ROUTE
                continue
            ni = lowest.get(dst)                                          # rule 4
            if ni is None:
                mstat[k] = NO_NEIGH
                continue
            mstat[k] = PLANNED                                            # rule 5
            h = headers(proto, P, id0 + planned, rt[ri]["iface"], dst, sport, dport, tcb[s] if tcp else None,
                        (tcb[s][0] + sent) if tcp else 0)
            planned += 1
            if tcp:
                sent += P
            ln[k] = len(h) + P                                            # rule 6
            at += -(-int(ln[k]) // align) * align
            l2[k] = np.frombuffer(bytes(nb[ni][1]) + rt[ri]["mac"], np.uint8)
            himg[k, :len(h)] = np.frombuffer(h, np.uint8)                 # rule 7
            dgs[k] = h + bytes(q[r + REC_HDR:r + REC_HDR + P])
        if tcp and tcb is not None:
            tnext[s] = (tcb[s][0] + sent) & 0xFFFFFFFF
    counts = np.array([planned, at, int((mstat == NO_ROUTE).sum()), int((mstat == NO_NEIGH).sum())], np.uint64)
    return dict(n=n, S=S, align=align, mstat=mstat, off=off, len=ln, l2=l2, himg=himg, tnext=tnext, counts=counts, dgs=dgs)


def build(pl, dgram, dgram_bytes=None):
    """Rule 8: writes the datagrams that have room into the uint8 array dgram; returns the final words."""
    dgram_bytes = len(dgram) if dgram_bytes is None else dgram_bytes
    fin = pl["mstat"].copy()
    for k, d in pl["dgs"].items():
        at = int(pl["off"][k])
        if at + len(d) > dgram_bytes:
            fin[k] |= NO_ROOM
        else:
            dgram[at:at + len(d)] = np.frombuffer(d, np.uint8)
            fin[k] |= BUILT
    return fin


def load_golden():
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    with open(os.path.join(here, "mux_vectors.json")) as f:
        vec = json.load(f)
    blob = np.fromfile(os.path.join(here, vec["blob"]), dtype=np.uint8)
    return vec, blob
