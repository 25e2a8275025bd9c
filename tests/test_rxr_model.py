"""CPU tests of one-pass RX reassembly (include/nstack_rxr.h): the expected-result model
(tests/rxr_model.py: the header's rules with the oracle's arithmetic) against the independently
generated golden vectors (tests/golden/make_rxr_golden.py), the host plan (ether_rx_reasm_plan_host)
against the model on the vectors, on seeded permutations and on the framer's golden frames, the ABI,
the argument errors that need no GPU, and the stand-alone sanitizer check of the host planning header
(tests/c/rxr_plan_check.cpp)."""
import errno
import os
import random
import re
import struct
import subprocess

import numpy as np
import pytest

import nstack_amd as na
import rxr_model as rr
import txf_model as fm
from rxr_batch import mg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAN_KEYS = ("fstat", "dst", "dgi", "doff", "dlen", "dlead")


@pytest.fixture(scope="module")
def rxr_golden():
    return rr.load_golden()


def host_plan(frames, flags=0, verdict=None, drop_mask=0, align=1, lead=0, gap=0, order=None):
    """ether_rx_reasm_plan_host over the frames laid out in an arena of exactly their size."""
    arena, off, ln = rr.layout(frames, lead=lead, gap=gap, order=order)
    n = len(frames)
    v = None if verdict is None else np.asarray(verdict, dtype=np.uint32)
    o = dict(fstat=np.full(n, 0xDEADBEEF, np.uint32), dst=np.full(n, 0xDEADBEEF, np.uint64), dgi=np.full(n, 0xDEADBEEF, np.uint32),
             doff=np.full(n + 1, 0xDEADBEEF, np.uint64), dlen=np.full(n, 0xDEADBEEF, np.uint32),
             dlead=np.full(n, 0xDEADBEEF, np.uint32))
    m = na.rx_reasm_plan_host(arena, arena.size, off, ln, n, o["fstat"], o["dst"], o["dgi"], o["doff"], o["dlen"], o["dlead"],
                              flags=flags, verdict=v, drop_mask=drop_mask, align=align)
    assert (o["doff"][m + 1:] == 0xDEADBEEF).all() and (o["dlen"][m:] == 0xDEADBEEF).all() and (o["dlead"][m:] == 0xDEADBEEF).all()
    o["doff"], o["dlen"], o["dlead"], o["m"] = o["doff"][:m + 1], o["dlen"][:m], o["dlead"][:m], m
    return o


def same_plan(got, want, what):
    assert got["m"] == want["m"], what
    for k in PLAN_KEYS:
        assert np.array_equal(got[k], want[k]), (what, k)


def test_model_matches_golden(inet_oracle, rxr_golden):
    assert len(rxr_golden["cases"]) >= 19
    for c in rxr_golden["cases"]:
        pl = rr.plan(c["frames"], c["flags"], c["verdict"], c["drop_mask"])
        room = int(pl["doff"][-1]) if c["out_bytes"] is None else c["out_bytes"]
        before = np.full(int(pl["doff"][-1]) + 16, 0xA5, dtype=np.uint8)
        arena, fstat = rr.build(inet_oracle, c["frames"], pl, before, room)
        assert fstat.tolist() == c["fstat"], c["tag"]
        assert pl["dlead"].tolist() == c["dlead"] and pl["dlen"].tolist() == c["dlen"], c["tag"]
        for k, (want, fits) in enumerate(zip(c["dgrams"], c["fits"])):
            at = int(pl["doff"][k])
            got = arena[at:at + len(want)].tobytes()
            assert got == (want if fits else b"\xa5" * len(want)), (c["tag"], k)
        assert (arena[int(pl["doff"][-1]):] == 0xA5).all()


def test_golden_covers_what_the_issue_lists(rxr_golden):
    by = {c["tag"]: c for c in rxr_golden["cases"]}
    seen = 0
    for c in by.values():
        for s in c["fstat"]:
            seen |= s
    assert seen == 0xFFF
    for t in (0, 1):
        c = by[f"hlens_differ_t{t}"]
        heads = {(f[14] & 15) * 4 for f, s in zip(c["frames"], c["fstat"]) if s & rr.HEAD}
        rest = {(f[14] & 15) * 4 for f, s in zip(c["frames"], c["fstat"]) if s & rr.FRAG and not s & rr.HEAD}
        assert {20, 60} <= heads and {20, 60} <= rest and all(s & rr.DELIVERED for s in c["fstat"])
        assert {(f[14] & 15) * 4 for f in by[f"whole_hlens_t{t}"]["frames"]} == set(range(20, 64, 4))
        c = by[f"short_lasts_t{t}"]
        lasts = [f for f, s in zip(c["frames"], c["fstat"]) if s & rr.FRAG and not s & rr.HEAD]
        assert {int.from_bytes(f[16:18], "big") - 20 for f in lasts} == set(range(1, 9)) and all(len(f) == 60 + 4 * t for f in lasts)
        assert min(c["dlen"]) == 29                                      # total 9: the smallest group there is
        assert all(s & rr.INCOMPLETE or s & rr.WHOLE for s in by[f"incomplete_t{t}"]["fstat"][:-3])
        assert [s & rr.DELIVERED for s in by[f"incomplete_t{t}"]["fstat"][-3:]] == [rr.DELIVERED] * 3
        # the gap-and-overlap vector: one head, one last, distinct offsets, and the lengths add up to the total
        go = [f for f in by[f"incomplete_t{t}"]["frames"] if f[18:20] == b"\x04\x0a"]
        spans = sorted(((int.from_bytes(f[20:22], "big") & 0x1FFF) * 8, int.from_bytes(f[16:18], "big") - 20) for f in go)
        assert spans == [(0, 16), (8, 16), (32, 8)] and sum(L for _o, L in spans) == spans[-1][0] + spans[-1][1]
        assert len(by[f"same_id_t{t}"]["dlen"]) == 4
        assert by[f"status_bits_t{t}"]["fstat"].count(rr.NOT_IPV4) == 4 and by[f"status_bits_t{t}"]["fstat"].count(rr.BAD_HDR) == 4
    assert by["total_65515"]["dlen"] == [65535] and len(by["total_65515"]["flen"]) == 45
    assert {p for c in by.values() for p in c["dlen"]} >= {20, 21, 28}   # payloads of 0, 1 and 8 bytes
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "rxr_vectors.bin")) < 500_000


def test_host_plan_equals_the_model_on_the_vectors(rxr_golden):
    for c in rxr_golden["cases"]:
        for align in (1, 16, 128):
            want = rr.plan(c["frames"], c["flags"], c["verdict"], c["drop_mask"], align)
            got = host_plan(c["frames"], c["flags"], c["verdict"], c["drop_mask"], align, lead=align % 5, gap=align % 3)
            same_plan(got, want, (c["tag"], align))


def test_host_plan_on_seeded_permutations(inet_oracle, rxr_golden):
    """Permutations of the same fragments: the datagram set and bytes are unchanged, the order follows
    the head frames."""
    by = {c["tag"]: c for c in rxr_golden["cases"]}
    rng = random.Random(5)
    for tag in ("hlens_differ_t1", "short_lasts_t0", "interleaved_t1", "incomplete_t0", "same_id_t0", "status_bits_t1"):
        c = by[tag]
        base = sorted(c["dgrams"][k] for k in range(len(c["dgrams"])))
        for _ in range(6):
            perm = list(range(len(c["frames"])))
            rng.shuffle(perm)
            frames = [c["frames"][q] for q in perm]
            verdict = None if c["verdict"] is None else [c["verdict"][q] for q in perm]
            want = rr.plan(frames, c["flags"], verdict, c["drop_mask"], 4)
            same_plan(host_plan(frames, c["flags"], verdict, c["drop_mask"], 4, order=rng.sample(perm, len(perm))), want, tag)
            arena, _ = rr.build(inet_oracle, frames, want, np.zeros(int(want["doff"][-1]), dtype=np.uint8))
            assert sorted(rr.datagrams(arena, want)) == base, tag
            assert want["dlead"].tolist() == sorted(want["dlead"].tolist())
            heads = [i for i in range(len(frames)) if want["dgi"][i] != rr.NONE32 and want["dst"][i] == want["doff"][want["dgi"][i]]]
            assert heads == want["dlead"].tolist()


# ---- the framer's golden frames come back as its golden datagrams ----
def _calls_of(recs, key_of):
    """The records in calls without two equal keys in one call."""
    calls = []
    for r in recs:
        for c in calls:
            if key_of(r) not in c["keys"]:
                break
        else:
            c = dict(keys=set(), recs=[])
            calls.append(c)
        c["keys"].add(key_of(r))
        c["recs"].append(r)
    return calls


def test_the_framers_golden_frames_come_back(inet_oracle):
    g = fm.load_golden()
    a = g["input_bytes"]
    back = frag_fits = 0
    for mtu, blob in g["frame_bytes"].items():
        recs = [r for r in g["datagrams"] if r["mtu"] == mtu and r["flen"]]
        dg_of = lambda r: a[r["off"]:r["off"] + r["len"]]
        calls = _calls_of(recs, lambda r: (dg_of(r)[12:20], dg_of(r)[9], dg_of(r)[4:6]))
        assert sum(len(c["recs"]) for c in calls) == len(recs) and all(len(c["keys"]) == len(c["recs"]) for c in calls)
        for c in calls:
            frames, owner = [], []
            for q, r in enumerate(c["recs"]):
                at = r["at"]
                for F in r["flen"]:
                    frames.append(blob[at:at + F + 4])
                    owner.append(q)
                    at += F + 4
            want = rr.plan(frames, rr.F_TRAILER)
            same_plan(host_plan(frames, rr.F_TRAILER), want, mtu)
            arena, fstat = rr.build(inet_oracle, frames, want, np.zeros(int(want["doff"][-1]), dtype=np.uint8))
            got = dict(zip((owner[int(i)] for i in want["dlead"]), rr.datagrams(arena, want)))
            for q, r in enumerate(c["recs"]):
                dg = dg_of(r)
                if r["tag"].endswith("_frag_fits"):                      # a lone fragment
                    assert q not in got and fstat[owner.index(q)] == rr.FRAG | rr.INCOMPLETE, r["tag"]
                    frag_fits += 1
                    continue
                rd, hlen = got[q], (dg[0] & 15) * 4
                assert len(rd) == len(dg) and rd[:6] == dg[:6] and rd[8:10] == dg[8:10] and rd[12:] == dg[12:], r["tag"]
                assert rd[6:8] == (b"\x00\x00" if r["status"] & fm.FRAGMENTED else dg[6:8]), r["tag"]
                hdr = bytearray(rd[:hlen])
                hdr[10:12] = b"\x00\x00"
                assert rd[10:12] == struct.pack("<H", inet_oracle.oracle_ip_checksum(bytes(hdr), hlen)), r["tag"]
                back += 1
    assert back > 480 and frag_fits == 5


def test_model_constants_match_the_binding_and_the_header():
    names = ("F_TRAILER", "WHOLE", "FRAG", "HEAD", "DROPPED", "NOT_IPV4", "BAD_HDR", "BAD_LEN", "FRAG_BAD", "INCOMPLETE",
             "TOO_BIG", "NO_ROOM", "DELIVERED", "NONE32", "NONE64")
    for name in names:
        assert getattr(rr, name) == getattr(na, "RXR_" + name), name
    hdr = open(os.path.join(ROOT, "include", "nstack_rxr.h")).read()
    found = re.findall(r"#define\s+(RXR_\w+)\s+(0x[0-9a-fA-F]+|\d+)u", hdr)
    assert len(found) == 15
    for name, val in found:
        assert getattr(na, name) == int(val, 0), name


# ---- ABI ----
def _declared():
    hdr = open(os.path.join(ROOT, "include", "nstack_rxr.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return re.findall(r"\b((?:ether_rx_reasm|fcs_debug_rxr_)\w*)\s*\(", hdr)


def test_every_declared_function_is_exported_and_listed():
    decl = _declared()
    assert sorted(decl) == sorted(na.RXR_EXPORTS) and len(decl) == 6
    out = subprocess.run(["nm", "-D", "--defined-only", na.LIB_PATH], capture_output=True, text=True, check=True).stdout
    syms = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in decl:
        assert name in syms, name
        assert getattr(na.load(), name).argtypes is not None, name
    assert not set(na.RXR_EXPORTS) & (set(na.EXPORTS) | set(na.RXV_EXPORTS) | set(na.TXS_EXPORTS) | set(na.TXF_EXPORTS))


# ---- argument errors (no GPU needed: they are decided before any device call) ----
def _args(n=3):
    frames = mg.fragments(None, bytes(range(100)), [48], False) + [mg.frame(mg.ip_packet(bytes(30)), False)]
    arena, off, ln = rr.layout(frames[:n])
    return dict(arena=arena, off=off, ln=ln, fstat=np.full(n, 0xDEADBEEF, np.uint32), dst=np.full(n, 0xDEADBEEF, np.uint64),
                dgi=np.full(n, 0xDEADBEEF, np.uint32), doff=np.full(n + 1, 0xDEADBEEF, np.uint64),
                dlen=np.full(n, 0xDEADBEEF, np.uint32), dlead=np.full(n, 0xDEADBEEF, np.uint32),
                out=np.full(400, 0xA5, np.uint8), n=n)


def _calls(L, a, flags=0, align=1, null=None, n=None, plan=True, build=True, host=True):
    """The four entry points' returns; plan / build / host = False leaves those calls out (None in their place)."""
    p = lambda k: None if k == null else a[k].ctypes.data
    n = a["n"] if n is None else n
    return (L.ether_rx_reasm_plan_host(p("arena"), a["arena"].size, p("off"), p("ln"), n, flags, None, 0, align, p("fstat"),
                                       p("dst"), p("dgi"), p("doff"), p("dlen"), p("dlead")) if plan else None,
            L.ether_rx_reasm_plan_dev(p("arena"), a["arena"].size, p("off"), p("ln"), n, flags, None, 0, align, p("fstat"),
                                      p("dst"), p("dgi"), p("doff"), p("dlen"), p("dlead"), None, None) if plan else None,
            L.ether_rx_reasm_dev(p("arena"), a["arena"].size, p("off"), p("ln"), n, flags, p("fstat"), p("dst"), p("dgi"),
                                 p("doff"), p("dlen"), p("out"), a["out"].size, None, None) if build else None,
            L.ether_rx_reasm_host(p("arena"), a["arena"].size, p("off"), p("ln"), n, flags, None, 0, align, p("out"),
                                  a["out"].size, p("fstat"), p("doff"), p("dlen"), p("dlead")) if host else None)


def _untouched(a):
    return all((a[k] == 0xDEADBEEF).all() for k in PLAN_KEYS) and (a["out"] == 0xA5).all()


def test_bad_flags_align_and_nulls_are_einval():
    L = na.load()
    a = _args()
    E = -errno.EINVAL
    for flags, word in ((2, "flag"), (0x80000001, "flag")):
        assert _calls(L, a, flags=flags) == (E, E, E, E), flags
        assert word in L.fcs_last_error().decode()
    for align in (0, 3, 24, 129, 256, 1 << 31):
        r = _calls(L, a, align=align, build=False)                       # the build call takes no align
        assert (r[0], r[1], r[3]) == (E, E, E), align
        assert "align" in L.fcs_last_error().decode()
    for null in ("arena", "off", "ln", "fstat", "dst", "dgi", "doff", "dlen"):
        needed = null in ("arena", "off", "ln")                          # the host form's other arrays are optional
        r = _calls(L, a, null=null, host=needed)
        assert r[:3] == (E, E, E) and r[3] == (E if needed else None), null
    assert _calls(L, a, null="out", plan=False)[2:] == (E, E)
    assert _calls(L, a, n=1 << 30) == (E, E, E, E)
    with pytest.raises(na.FcsError):
        na.rx_reasm_plan_host(a["arena"], a["arena"].size, a["off"], a["ln"], 3, a["fstat"], a["dst"], a["dgi"], a["doff"],
                              a["dlen"], align=3)
    assert _untouched(a)


def test_host_forms_check_the_arena_and_the_capacity_before_any_work():
    L = na.load()
    a = _args()
    E = -errno.EINVAL
    p = lambda k: a[k].ctypes.data
    off2 = a["off"].copy()
    for bad in (a["arena"].size - int(a["ln"][1]) + 1, 2**64 - 20):    # one byte past the arena; off + len wraps
        off2[1] = bad
        assert L.ether_rx_reasm_plan_host(p("arena"), a["arena"].size, off2.ctypes.data, p("ln"), 3, 0, None, 0, 1, p("fstat"),
                                          p("dst"), p("dgi"), p("doff"), p("dlen"), p("dlead")) == E
        assert "frame 1 " in L.fcs_last_error().decode()
        assert L.ether_rx_reasm_host(p("arena"), a["arena"].size, off2.ctypes.data, p("ln"), 3, 0, None, 0, 1, p("out"),
                                     a["out"].size, p("fstat"), p("doff"), p("dlen"), p("dlead")) == E
        assert "frame 1 " in L.fcs_last_error().decode()
    # two datagrams of 120 and 50 bytes: 170 bytes hold them, 169 do not, and with align 128 the second ends at 178
    for out_bytes, align in ((169, 1), (0, 1), (177, 128)):
        assert L.ether_rx_reasm_host(p("arena"), a["arena"].size, p("off"), p("ln"), 3, 0, None, 0, align, p("out"), out_bytes,
                                     p("fstat"), p("doff"), p("dlen"), p("dlead")) == -errno.ENOSPC
    assert _untouched(a)
    assert L.ether_rx_reasm_plan_host(p("arena"), a["arena"].size, p("off"), p("ln"), 3, 0, None, 0, 128, p("fstat"), p("dst"),
                                      p("dgi"), p("doff"), p("dlen"), p("dlead")) == 2
    assert a["doff"][:3].tolist() == [0, 128, 256] and a["dlen"][:2].tolist() == [120, 50] and a["dlead"][:2].tolist() == [0, 2]
    # n = 0: the empty plan, whatever the other pointers are
    assert L.ether_rx_reasm_plan_host(None, 0, None, None, 0, 0, None, 0, 1, None, None, None, p("doff"), None, None) == 0
    assert a["doff"][0] == 0


def _no_gpu():
    try:
        import torch
        return not torch.cuda.is_available()
    except Exception:
        return True


@pytest.mark.skipif(not _no_gpu(), reason="a GPU is present")
def test_no_gpu_is_enodev_without_touching_the_host_counters():
    L = na.load()
    a = _args()
    before = (L.fcs_engine_host_batches(), L.fcs_engine_host_fallbacks())
    r = _calls(L, a)
    assert r[0] == 2 and r[1:] == (-errno.ENODEV,) * 3                   # the plan is host arithmetic
    assert (L.fcs_engine_host_batches(), L.fcs_engine_host_fallbacks()) == before
    assert (a["out"] == 0xA5).all()


# ---- the host planning header under the sanitizers (a stand-alone program: nothing is loaded into Python) ----
def test_plan_header_check_runs_clean_under_asan_and_ubsan():
    cdir = os.path.join(ROOT, "tests", "c")
    subprocess.run(["make", "-s", "-C", cdir, "-f", "rxr_plan_check.mk"], check=True)
    r = subprocess.run([os.path.join(cdir, "rxr_plan_check")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "rxr_plan_check: ok" in r.stdout and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr
