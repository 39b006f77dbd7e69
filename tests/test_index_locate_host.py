"""Positions, segments, depth (kbo_hip.h) on the host: the position table's rule (kbo_positions_from_ms_host), the segments and delta
of a walked batch (kbo_segments_from_ms_host), the argument errors of every new entry point that checks before its first HIP call, and
tools/index_locate_check.cpp under AddressSanitizer and UBSan.

The yardstick is brute force written here from the definitions: a dict from every k-mer of every indexed stretch of the sources to its
occurrences (REV through the reverse complement), the expected entry from it, and a chain builder over the dict for the segments.  The
library's side is fed by the oracle's matching statistics.  All comparisons are exact and cover every row, record and delta word.
No GPU.  tests/test_gpu_index_locate.py takes the worlds and the brute force from here."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import kbo_amd
from kbo_amd import _capi, locate
from oracle import binding as ora

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_EMPTY_QUERY, E_BAD_ARG, E_UNSUPPORTED = -1, -4, -8
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
COMP = np.arange(256, dtype=np.uint8)  # (lower case stays what it is: no base on either strand)
for _a, _b in zip(b"ACGT", b"TGCA"):
    COMP[_a] = _b
NONE, MULTI, REV, PMASK = 0xFFFFFFFF, 1 << 31, 1 << 30, (1 << 30) - 1
KS = [5, 31, 96]
BRIDGES = lambda k: [0, 1, k, 255]  # noqa: E731
NEW_SYMBOLS = ["kbo_index_add_positions", "kbo_index_has_positions", "kbo_index_positions_bytes", "kbo_index_positions", "kbo_index_source_offsets",
               "kbo_index_source_bases", "kbo_index_positions_to_device", "kbo_positions_from_ms_host", "kbo_segments_work_bytes", "kbo_segments_dev",
               "kbo_segments_from_ms_host", "kbo_depth_work_bytes", "kbo_depth_finish_dev", "kbo_segments_batch"]


def revcomp(a):
    return COMP[a[::-1]]


def _other(b):
    return ACGT[(int(np.searchsorted(ACGT, b)) + 1) % 4]


# ---- the worlds
LENS = (700, 300, 64, 4)


def sources(k, seed=11, lens=LENS):
    """sequences of 700, 300, 64 and 4 bases (or longer first two): an exact repeat of k + 20 bases inside the first (MULTI), k + 10 bases of the first reverse-
    complemented into the second (an inverted repeat), an N and a lower-case base in the second, and sequences shorter than k"""
    rng = np.random.default_rng(seed + k)
    s = [ACGT[rng.integers(0, 4, n)].copy() for n in lens]
    R, R2 = k + 20, k + 10
    s[0][400:400 + R] = s[0][50:50 + R]
    s[1][150:150 + R2] = revcomp(s[0][200:200 + R2])
    s[1][270] = ord("N")
    s[1][285] = ord("a")
    return s


def stretches(seq, k):
    """the indexed stretches of a sequence: maximal runs of A, C, G, T of at least k bases, as (begin, end)"""
    ok = np.isin(seq, ACGT)
    out, i, n = [], 0, len(seq)
    while i < n:
        if not ok[i]:
            i += 1
            continue
        j = i
        while j < n and ok[j]:
            j += 1
        if j - i >= k:
            out.append((i, j))
        i = j
    return out


def occurrences(srcs, k, add_revcomp):
    """k-mer -> [(rev, p)] over the sources, p in source coordinates"""
    occ, base = {}, 0
    for seq in srcs:
        for b, e in stretches(seq, k):
            for i in range(b, e - k + 1):
                w = seq[i:i + k]
                occ.setdefault(w.tobytes(), []).append((0, base + i))
                if add_revcomp:
                    occ.setdefault(revcomp(w).tobytes(), []).append((1, base + i))
        base += len(seq)
    return occ


def entry_of(occs):
    rev, p = min(occs)  # FWD before REV, then the smallest p
    return p | (REV if rev else 0) | (MULTI if len(occs) > 1 else 0)


def expected_table(oi, occ):
    """the entry of every row of the oracle's index, through the row's own k-mer"""
    out = np.full(oi.n_sets, NONE, dtype=np.uint32)
    for r in range(oi.n_sets):
        o = occ.get(oi.access_kmer(r))
        if o:
            out[r] = entry_of(o)
    return out


def walk(oi, seqs):
    """(d uint8, lo uint32, offsets) of the oracle's matching statistics, sequence by sequence; an empty sequence has none"""
    ds, los, off = [], [], [0]
    for q in seqs:
        if len(q):
            d, lo, _ = oi.matching_statistics(q)
            ds.append(d.astype(np.uint8))
            los.append(lo.astype(np.uint32))
        off.append(off[-1] + len(q))
    cat = lambda xs, t: np.concatenate(xs) if xs else np.zeros(0, dtype=t)  # noqa: E731
    return cat(ds, np.uint8), cat(los, np.uint32), np.array(off, dtype=np.uint64)


def src_offsets(srcs):
    return np.concatenate([[0], np.cumsum([len(s) for s in srcs])]).astype(np.uint64)


def queries(srcs, k):
    """name -> sequence: what the issue lists"""
    s0, s1 = srcs[0], srcs[1]
    R = k + 20
    q = {}
    q["exact"] = s0[100:100 + k + 60].copy()
    sub = s0[168:168 + 2 * k + 40].copy()  # (between the two copies of the repeat)
    sub[len(sub) // 2] = _other(sub[len(sub) // 2])
    q["substitution"] = sub
    base = s1[0:2 * k + 30]
    q["insertion"] = np.concatenate([base[:len(base) // 2], ACGT[:1], base[len(base) // 2:]])
    q["deletion"] = np.concatenate([base[:len(base) // 2], base[len(base) // 2 + 1:]])
    q["reverse"] = revcomp(s0[20:20 + k + 50])
    q["repeat_first"] = s0[55:50 + R + k + 10].copy()
    q["repeat_second"] = s0[405:400 + R + k + 10].copy()
    q["junction"] = np.concatenate([s0[len(s0) - (k + 10):], s1[:k + 10]])
    q["short"] = s0[300:300 + k - 1].copy()
    q["empty"] = np.zeros(0, dtype=np.uint8)
    q["tail"] = s0[560:700].copy()
    return q


# ---- brute force: the chain builder
def brute_segments(seqs, occ, k, bridge, strand):
    """records of the batch as tuples (seq, strand, q_first, q_last, pos_first, pos_last, flags), in (seq, q_first) order"""
    lists = []
    for q in seqs:
        ok = np.isin(q, ACGT)
        anchors = []
        for i in range(0, len(q) - k + 1):
            if ok[i:i + k].all():
                o = occ.get(q[i:i + k].tobytes())
                if o:
                    anchors.append((i, entry_of(o)))
        lists.append(anchors)
    return brute_chains(lists, bridge, strand)


def brute_chains(anchor_lists, bridge, strand):
    """the chain-building half of brute_segments: anchor_lists[s] holds the anchors of sequence s as (q, entry) by ascending q - from
    the occurrence dict as above, or synthetic"""
    out = []
    for s, anchors in enumerate(anchor_lists):
        chain = []
        for a in anchors:
            if chain:
                (qa, ea), (qb, eb) = chain[-1], a
                rev = bool(ea & REV)
                same_diag = ((ea & PMASK) + qa == (eb & PMASK) + qb) if rev else ((ea & PMASK) - qa == (eb & PMASK) - qb)
                if not (qb - qa <= 1 + bridge and bool(eb & REV) == rev and same_diag):
                    out.append((s, chain))
                    chain = []
            chain.append(a)
        if chain:
            out.append((s, chain))
    recs = []
    for s, chain in out:
        (qf, ef), (ql, el) = chain[0], chain[-1]
        recs.append((s, strand, qf, ql, ef & PMASK, el & PMASK, (1 if ef & REV else 0) | (4 if ef & MULTI else 0) | (8 if el & MULTI else 0)))
    return recs


def covered(rec, k):
    """the half-open range of source bases a record covers"""
    return (rec[5], rec[4] + k) if rec[6] & 1 else (rec[4], rec[5] + k)


def brute_delta(recs, k, n_bases):
    d = np.zeros(n_bases + 1, dtype=np.int64)
    for r in recs:
        a, b = covered(r, k)
        d[a] += 1
        d[b] -= 1
    return (d & 0xFFFFFFFF).astype(np.uint32)


def brute_depth(recs, k, n_bases):
    d = np.zeros(n_bases, dtype=np.uint32)
    for r in recs:
        a, b = covered(r, k)
        d[a:b] += 1
    return d


def as_tuples(segs):
    return [tuple(int(v) for v in r) for r in segs.tolist()]


_WORLDS = {}


def world(k, add_revcomp, lens=LENS):
    """the sources, the oracle's index over them, the occurrence dict and the expected table; made once per (k, add_revcomp, lens)"""
    key = (k, bool(add_revcomp), lens)
    if key not in _WORLDS:
        srcs = sources(k, lens=lens)
        oi = ora.Index.build([s.tobytes() for s in srcs], k=k, add_revcomp=bool(add_revcomp))
        occ = occurrences(srcs, k, add_revcomp)
        _WORLDS[key] = (srcs, oi, occ, expected_table(oi, occ))
    return _WORLDS[key]


# ---- the table
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("add_revcomp", [False, True])
def test_table_from_the_oracles_walk_equals_brute_force(k, add_revcomp):
    srcs, oi, occ, want = world(k, add_revcomp)
    assert len(occ) == oi.n_kmers
    n, soff = oi.n_sets, src_offsets(srcs)
    got = np.full(n, NONE, dtype=np.uint32)
    missing = []
    for rev in ([0, 1] if add_revcomp else [0]):
        seqs = [revcomp(s) for s in srcs] if rev else srcs
        d, lo, off = walk(oi, seqs)
        assert np.array_equal(off, soff)
        missing.append(locate.positions_from_ms_host(k, n, d, lo, off, soff, rev, got))
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:10]
    windows = sum(max(0, len(s) - k + 1) for s in srcs)
    indexed = sum(e - b - k + 1 for s in srcs for b, e in stretches(s, k))
    assert missing == [windows - indexed] * len(missing)
    # the planted cases occur
    ent = want[want != NONE]
    assert (ent & MULTI).any(), "the exact repeat gives MULTI"
    assert indexed < windows, "the N, the lower-case base and the short sequences leave windows out"
    assert any(len(s) < k for s in srcs)
    if add_revcomp:
        assert ((ent & REV) != 0).any(), "a k-mer with no forward occurrence: REV wins"
        both = [o for o in occ.values() if {r for r, _ in o} == {0, 1}]
        assert both and all(not (entry_of(o) & REV) for o in both), "the inverted repeat: FWD wins over REV"
    else:
        assert not (ent & REV).any()


# ---- segments and delta
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("add_revcomp", [False, True])
def test_segments_and_delta_equal_the_brute_force_chains(k, add_revcomp):
    srcs, oi, occ, table = world(k, add_revcomp)
    n_bases = int(src_offsets(srcs)[-1])
    qs = queries(srcs, k)
    names, seqs = list(qs), list(qs.values())
    d, lo, off = walk(oi, seqs)
    seen = {}
    for bridge in BRIDGES(k):
        want = brute_segments(seqs, occ, k, bridge, 1)
        delta = np.zeros(n_bases + 1, dtype=np.uint32)
        got, n = locate.segments_from_ms_host(table, k, d, lo, off, bridge, 1, len(want) + 5, n_bases, delta)
        assert n == len(want) and as_tuples(got) == want, (bridge, [(a, b) for a, b in zip(as_tuples(got), want) if a != b][:3])
        assert np.array_equal(delta, brute_delta(want, k, n_bases))
        assert np.array_equal(np.cumsum(delta[:-1], dtype=np.uint32), brute_depth(want, k, n_bases))
        seen[bridge] = {nm: [r for r in want if r[0] == i] for i, nm in enumerate(names)}
        # a capacity below the count: counted, and nothing written at or behind it
        few = max(0, len(want) - 3)
        got2, n2 = locate.segments_from_ms_host(table, k, d, lo, off, bridge, 2, few, n_bases)
        assert n2 == len(want) and as_tuples(got2) == [r[:1] + (2,) + r[2:] for r in want[:few]]
    # what each planted query is there for (k = 5: nearly every 5-mer occurs somewhere in 1 068 bases, so only the comparison above holds)
    if k < 31:
        return
    assert len(seen[0]["exact"]) == 1 and seen[0]["exact"][0][2:4] == (0, 60) and seen[0]["exact"][0][4] == 100
    assert len(seen[0]["substitution"]) == 2 and len(seen[k]["substitution"]) == 1
    for nm in ("insertion", "deletion"):
        assert len(seen[255][nm]) == 2, "an indel changes the diagonal: never joined"
    assert len(seen[255]["repeat_second"]) >= 2, "leaving the second copy of the repeat: the diagonal jumps"
    assert seen[255]["repeat_second"][0][6] & 4, "... and its first anchors are MULTI"
    assert len(seen[0]["junction"]) == 2, "no window spans two sources"
    assert len(seen[k]["junction"]) == 1, "... but the sources are adjacent in source coordinates: one diagonal, k windows apart"
    assert not seen[255]["short"] and not seen[255]["empty"]
    if add_revcomp:
        assert len(seen[0]["reverse"]) == 1 and seen[0]["reverse"][0][6] & 1 and seen[0]["reverse"][0][4] > seen[0]["reverse"][0][5]
    else:
        assert not seen[0]["reverse"]


def test_segment_source_names_the_sequence_and_the_offset():
    off = np.array([0, 700, 1000, 1064, 1068], dtype=np.uint64)
    segs = np.zeros(3, dtype=locate.SEGMENT_DTYPE)
    segs["pos_first"], segs["pos_last"], segs["flags"] = [5, 900, 1063], [50, 720, 1063], [0, 1, 0]
    src, at, rev = locate.segment_source(segs, off)
    assert src.tolist() == [0, 1, 2] and at.tolist() == [5, 20, 63] and rev.tolist() == [0, 1, 0]


# ---- errors
def _seqs(items):
    arr = (C.c_char_p * len(items))(*items)
    lens = (C.c_size_t * len(items))(*[len(s) for s in items])
    return arr, lens


def test_argument_errors_come_before_any_device_work():
    L = kbo_amd.lib()
    rust = open(os.path.join(ROOT, "bindings", "rust", "kbo-hip", "src", "lib.rs")).read()
    guide = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW_SYMBOLS:
        assert name in _capi.SYMBOLS and hasattr(L, name) and "pub fn %s(" % name in rust
    for name in ("kbo_index_add_positions", "kbo_segments_dev", "kbo_depth_finish_dev", "kbo_segments_batch"):
        assert "pub fn %s(" % name in guide
    g = b"ACGTTGCATGCATGCAAGTCGATCGATTTGACCATG" * 3
    sbwt, _ = kbo_amd.build([g], kbo_amd.BuildOpts(k=7))
    h = sbwt._h
    arr, lens = _seqs([g])
    P = 0x10000  # a pointer that is never followed: every check below comes first
    n, n64, nsz = C.c_uint64(0), C.c_uint64(0), C.c_size_t(0)
    # kbo_index_add_positions
    assert L.kbo_index_add_positions(None, arr, lens, 1, 0, -1) == E_BAD_ARG
    assert L.kbo_index_add_positions(h, None, lens, 1, 0, -1) == E_BAD_ARG
    assert L.kbo_index_add_positions(h, arr, None, 1, 0, -1) == E_BAD_ARG
    assert L.kbo_index_add_positions(h, arr, lens, 0, 0, -1) == E_BAD_ARG
    big = (C.c_size_t * 1)(1 << 30)
    assert L.kbo_index_add_positions(h, arr, big, 1, 0, -1) == E_UNSUPPORTED
    # a handle without positions
    assert L.kbo_index_has_positions(h) == 0 and L.kbo_index_has_positions(None) == 0
    assert L.kbo_index_positions_bytes(h) == 0 and L.kbo_index_source_bases(h) == 0 and L.kbo_depth_work_bytes(h) == 0
    assert L.kbo_index_positions(h, None, C.byref(nsz)) == E_BAD_ARG and L.kbo_index_positions(h, None, None) == E_BAD_ARG
    assert L.kbo_index_source_offsets(h, None, C.byref(nsz)) == E_BAD_ARG and L.kbo_index_source_offsets(None, None, C.byref(nsz)) == E_BAD_ARG
    assert L.kbo_index_positions_to_device(None, -1) == E_BAD_ARG and L.kbo_index_positions_to_device(h, -1) == E_BAD_ARG
    with pytest.raises(kbo_amd.KboError) as e:
        sbwt.positions()
    assert e.value.code == E_BAD_ARG
    # kbo_segments_dev, in its order: null, misaligned, bridge; empty; limits, sharded; no positions
    wb = L.kbo_segments_work_bytes(3, 1000)

    def seg(idx=h, ms=P, lo=P, off=P, n_seqs=3, total=1000, bridge=7, segs=P, cap=10, cnt=P, delta=None, work=P, wbytes=wb):
        return L.kbo_segments_dev(idx, ms, lo, off, n_seqs, total, bridge, 1, segs, cap, cnt, delta, work, wbytes, None)
    for kw in (dict(idx=None), dict(ms=None), dict(lo=None), dict(off=None), dict(cnt=None), dict(work=None), dict(segs=None)):
        assert seg(**kw) == E_BAD_ARG, kw
    for kw in (dict(lo=P + 2), dict(off=P + 4), dict(cnt=P + 4), dict(work=P + 8), dict(segs=P + 1), dict(delta=P + 2)):
        assert seg(n_seqs=0, **kw) == E_BAD_ARG, kw
    assert seg(bridge=256, n_seqs=0) == E_BAD_ARG
    assert seg(n_seqs=0, total=1 << 33) == E_EMPTY_QUERY
    assert seg(total=(1 << 32) - 15) == E_UNSUPPORTED and seg(n_seqs=1 << 28) == E_UNSUPPORTED
    assert seg(segs=None, cap=0) == E_BAD_ARG and "no positions" in L.kbo_last_error().decode()
    # kbo_depth_finish_dev
    assert L.kbo_depth_finish_dev(None, P, P, P, 16, None) == E_BAD_ARG and L.kbo_depth_finish_dev(h, None, P, P, 16, None) == E_BAD_ARG
    assert L.kbo_depth_finish_dev(h, P, P + 2, P, 16, None) == E_BAD_ARG and L.kbo_depth_finish_dev(h, P, P, P, 1 << 20, None) == E_BAD_ARG
    # kbo_segments_batch
    q = np.frombuffer(g, dtype=np.uint8)
    off = np.array([0, len(q)], dtype=np.uint64)
    out = C.c_void_p()

    def batch(idx=h, concat=q.ctypes.data, offsets=off.ctypes.data, n_seqs=1, bridge=7, strands=1, segs=C.byref(out), cnt=C.byref(n64)):
        return L.kbo_segments_batch(idx, concat, offsets, n_seqs, bridge, strands, segs, cnt, None)
    assert batch(strands=0) == E_BAD_ARG and batch(strands=4, idx=None) == E_BAD_ARG
    assert batch(idx=None) == E_BAD_ARG and batch(segs=None) == E_BAD_ARG and batch(cnt=None) == E_BAD_ARG
    assert batch(bridge=256) == E_BAD_ARG
    assert batch() == E_BAD_ARG and "no positions" in L.kbo_last_error().decode()
    with pytest.raises(kbo_amd.KboError) as e:
        kbo_amd.segments([g], sbwt)
    assert e.value.code == E_BAD_ARG
    # a sharded handle
    L.kbo_set_index_shards(2)
    try:
        sharded, _ = kbo_amd.build([g, g[::-1]], kbo_amd.BuildOpts(k=7))
    finally:
        L.kbo_set_index_shards(0)
    assert sharded.shards() == 2
    arr2, lens2 = _seqs([g, g[::-1]])
    assert L.kbo_index_add_positions(sharded._h, arr2, lens2, 2, 0, -1) == E_UNSUPPORTED
    assert L.kbo_index_add_positions(sharded._h, arr2, lens2, 0, 0, -1) == E_BAD_ARG
    assert seg(idx=sharded._h) == E_UNSUPPORTED and batch(idx=sharded._h) == E_UNSUPPORTED
    assert L.kbo_index_positions_to_device(sharded._h, -1) == E_UNSUPPORTED and L.kbo_index_has_positions(sharded._h) == 0
    # the host restatements
    ent = np.full(8, NONE, dtype=np.uint32)
    d, lo = np.zeros(4, dtype=np.uint8), np.zeros(4, dtype=np.uint32)
    o4 = np.array([0, 4], dtype=np.uint64)
    rec = np.zeros(4, dtype=locate.SEGMENT_DTYPE)

    def host_seg(entries=ent.ctypes.data, d_=d.ctypes.data, lo_=lo.ctypes.data, off_=o4.ctypes.data, n_seqs=1, bridge=0, segs=rec.ctypes.data, cap=4,
                 cnt=C.byref(n)):
        return L.kbo_segments_from_ms_host(entries, 8, 3, d_, lo_, off_, n_seqs, bridge, 1, segs, cap, cnt, None, 100)
    assert host_seg() == 0 and n.value == 0
    for kw in (dict(entries=None), dict(d_=None), dict(lo_=None), dict(off_=None), dict(cnt=None), dict(segs=None)):
        assert host_seg(**kw) == E_BAD_ARG, kw
    assert host_seg(segs=None, cap=0) == 0
    assert host_seg(bridge=256, n_seqs=0) == E_BAD_ARG and host_seg(n_seqs=0) == E_EMPTY_QUERY
    bad = np.array([0, 4, 2], dtype=np.uint64)
    assert host_seg(off_=bad.ctypes.data, n_seqs=2) == E_BAD_ARG
    assert L.kbo_positions_from_ms_host(3, 8, None, lo.ctypes.data, o4.ctypes.data, 1, o4.ctypes.data, 0, ent.ctypes.data, None) == E_BAD_ARG
    assert L.kbo_positions_from_ms_host(3, 8, d.ctypes.data, lo.ctypes.data, o4.ctypes.data, 0, o4.ctypes.data, 0, ent.ctypes.data, None) == E_BAD_ARG
    o5 = np.array([0, 5], dtype=np.uint64)
    assert L.kbo_positions_from_ms_host(3, 8, d.ctypes.data, lo.ctypes.data, o4.ctypes.data, 1, o5.ctypes.data, 0, ent.ctypes.data, None) == E_BAD_ARG
    assert L.kbo_positions_from_ms_host(3, 8, d.ctypes.data, lo.ctypes.data, o4.ctypes.data, 1, o4.ctypes.data, 0, ent.ctypes.data, None) == 0


def test_work_byte_figures_are_the_documented_ones():
    L = kbo_amd.lib()
    tile, halo, chunk = C.c_uint32(), C.c_uint32(), C.c_uint32()
    assert L.kbo_segments_geometry(C.byref(tile), C.byref(halo), C.byref(chunk)) == 0
    assert (tile.value, halo.value, chunk.value) == (2048, 256, 2048) and halo.value >= 256
    r16 = lambda v: (v + 15) // 16 * 16  # noqa: E731
    for n_seqs, total in ((1, 1), (3, 2048), (7, 2049), (100, 15000), (1 << 20, 150 << 20)):
        tiles = (total + tile.value - 1) // tile.value
        assert L.kbo_segments_work_bytes(n_seqs, total) == r16(total) + r16(8 * tiles) + r16(8 * ((tiles + chunk.value - 1) // chunk.value))
    assert L.kbo_segments_work_bytes(0, 100) == 0 and L.kbo_segments_work_bytes(1 << 28, 100) == 0
    assert L.kbo_segments_work_bytes(1, (1 << 32) - 15) == 0 and L.kbo_segments_work_bytes(1, (1 << 32) - 16) > 0


# ---- sanitizers
def test_locate_arithmetic_under_sanitizers(tmp_path):
    """tools/index_locate_check.cpp: the serial forms, the tile-and-halo decision and the three-pass scan of index_locate.hpp through
    accessors that check every index, against brute force of its own"""
    exe = str(tmp_path / "index_locate_check")
    subprocess.run(["c++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I",
                    os.path.join(ROOT, "kbo_amd", "csrc"), os.path.join(ROOT, "tools", "index_locate_check.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "in range" in run.stdout and "agree" in run.stdout
