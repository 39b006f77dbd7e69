"""Positions, segments, depth, placement and pileup (kbo_hip.h) at the sizes where their kernels take a loop a second time.

The other three GPU modules of this family run over two hand-planted worlds in which every grid-stride loop, every carry of a scan and
every wave's record loop is taken once.  Here each of those loops is taken at least twice, over synthetic arrays uploaded to the device
- records, MS bytes, rows, offsets, delta, pile - made with numpy so that the expected words follow from the definitions in kbo_hip.h
without a walk: a vectorised statement of the rule, which the CPU restatement (kbo_*_host) must equal as well and which the brute
force of the host modules confirms on a sample.  Every threshold below is derived from the launch code it names, and every test first
asserts that its input lies beyond it.  Every device buffer is at exactly its documented figure between guard bands.

Not covered: the 64-bit scan of the tiles' counts in kbo_segments_dev takes a second round of scan_sums_kernel only above
kThreads * kScanChunk tiles = 2^30 bases a batch, out of reach for a test of seconds."""
import numpy as np
import pytest

import kbo_amd
from kbo_amd import locate

from gpu_helpers import Guarded
from test_gpu_index_locate import _Batch, _dev, _geometry, _located
from test_gpu_index_pileup import _Piles, _Uploaded
from test_gpu_index_place import _Dev, _hand_handle
from test_index_locate_host import ACGT, LENS, MULTI, NONE, PMASK, REV, as_tuples, brute_chains, brute_delta, revcomp, src_offsets, world
from test_index_pileup_host import brute_pile, brute_sites, site_tuples
from test_index_place_host import FIELDS, K as PLACE_K, SRC_OFF, py_merge, py_place, same

pytestmark = pytest.mark.gpu

SEG, SITE = locate.SEGMENT_DTYPE.itemsize, locate.SITE_DTYPE.itemsize
# launch_pileup (pileup_kernels.hip): min(ceil(capacity / kWaves), 8192) workgroups of kWaves = 4 waves, a wave a record: the loop
# `r += n_waves` of pileup_kernel takes a second turn beyond 8192 * 4 records
PILEUP_TURN = 8192 * 4
# launch_place (place_kernels.hip): place_wave_kernel on min(capacity / (kLaneMax + 1), n_seqs, 4096) workgroups of one wave:
# `at += gridDim.x` takes a second turn beyond 4096 lists of more than kLaneMax segments
WAVE_TURN, LANE_MAX, WINDOW = 4096, locate.PLACE_LANE_MAX, locate.PLACE_WINDOW
# stride_blocks() (locate_kernels.hip) and place_range_kernel's grid (launch_place): at most 4096 workgroups of kThreads = 256 lanes:
# locate_mark_kernel, locate_entries_kernel, segment_clear_kernel and place_range_kernel stride beyond 4096 * 256 elements
STRIDE_TURN = 4096 * 256
# launch_scan3 / launch_pileup_sites: scan_sums_kernel and site_sums_kernel are ONE workgroup that takes the chunks' sums kThreads = 256
# at a time, a chunk kScanChunk = 2048 values: `run` is carried beyond 256 * 2048 source bases
SCAN_TURN = 256 * 2048
# tile_sequences (locate_kernels.hip): `s += kThreads` over the sequence starts inside the positions a tile looks at
STARTS_TURN = 256
CODE = np.full(256, 4, dtype=np.int64)
for _i, _b in enumerate(b"ACGT"):
    CODE[_b] = _i

K5 = 5


def _small(rc=True):
    """the small located handle of tests/test_gpu_index_locate.py at k = 5 and its table, which that module checks row by row"""
    sbwt = _located(K5, rc, LENS)
    table = world(K5, rc, LENS)[3]
    assert np.array_equal(sbwt.positions(), table)
    return sbwt, table, int(src_offsets(world(K5, rc, LENS)[0])[-1])


# ---- a. pileup over more than two turns of records
def pileup_world(k, n_bases, n, seed):
    """n records, one a sequence: anchors at windows pad and pad + g with none between them (g = k + 1: one bridged base, the substituted
    one; every 1 000th sequence g = 66 .. 90: a gap of more than 64 windows), `pad` bases in front of which some records take the last
    two windows in (a head no anchor covers); FWD and REV, MULTI at either end, N and lower-case bytes at the bridged base, positions
    drawn from the few source bases there are: many records add to the same word"""
    rng = np.random.default_rng(seed)
    r = np.arange(n)
    pad = np.where(rng.integers(0, 3, n) == 0, 0, rng.integers(0, 24, n))
    head = np.where((rng.integers(0, 4, n) == 0) & (pad >= 2), 2, 0)
    g = np.where(r % 1000 == 0, 66 + (r // 1000) % 25, k + 1)
    lens = pad + g + k
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    total = int(off[-1])
    cat = ACGT[rng.integers(0, 4, total)]
    mid = off[:-1].astype(np.int64) + pad + k  # the base behind the first anchor's window
    cat[mid[r % 97 == 3]] = ord("N")
    cat[mid[r % 97 == 5]] = ord("g")
    ms = rng.integers(0, k, total).astype(np.uint8)
    ms[off[:-1].astype(np.int64) + pad + k - 1] = k
    ms[off[:-1].astype(np.int64) + pad + g + k - 1] = k
    segs = np.zeros(n, dtype=locate.SEGMENT_DTYPE)
    rev = (r % 3 == 1).astype(np.int64)
    pf = np.where(r % 5 == 0, rng.integers(0, n_bases, n), rng.integers(300, 360, n))  # (most on 60 bases: contended words)
    segs["seq"], segs["strand"], segs["q_first"], segs["q_last"] = r, 1, pad - head, pad + g
    segs["pos_first"] = pf
    segs["pos_last"] = (np.where(rev == 1, pf - (g + head), pf + g + head) & 0xFFFFFFFF).astype(np.uint32)
    segs["flags"] = rev | np.where(r % 11 == 4, 4, 0) | np.where(r % 11 == 7, 8, 0)
    return dict(segs=segs, cat=cat, ms=ms, off=off, n_long=int((r % 1000 == 0).sum()))


def vector_pile(segs, cat, ms, off, k, n_bases, skip_multi):
    """(pile, bridged bases) of records that all hold something, from the definition: base x of [q_first, q_last + k) is bridged when
    no window of [max(q_first, x - k + 1), min(x, q_last)] is an anchor - a difference of the anchors' prefix counts"""
    take = np.flatnonzero((segs["flags"] & 12) == 0) if skip_multi else np.arange(len(segs))
    qf, ql, pf = (segs[f][take].astype(np.int64) for f in ("q_first", "q_last", "pos_first"))
    o = off[segs["seq"][take]].astype(np.int64)
    rev = (segs["flags"][take] & 1).astype(np.int64)
    span = ql + k - qf
    rec = np.repeat(np.arange(len(take)), span)
    x = qf[rec] + np.arange(len(rec)) - np.repeat(np.cumsum(span) - span, span)
    anchors = np.concatenate([[0], np.cumsum(ms[:len(cat)] == k)])
    first, last = np.maximum(qf[rec], x - k + 1), np.minimum(x, ql[rec])
    bridged = anchors[o[rec] + last + k] - anchors[o[rec] + first + k - 1] == 0
    code = CODE[cat[o[rec] + x]]
    col = np.where(rev[rec] == 1, 3 - code, code)
    j = np.where(rev[rec] == 1, pf[rec] + k - 1 - (x - qf[rec]), pf[rec] + (x - qf[rec]))
    ok = bridged & (code < 4) & (j >= 0) & (j < n_bases)
    pile = np.zeros((n_bases, 4), dtype=np.int64)
    np.add.at(pile, (j[ok], col[ok]), 1)
    return pile, int(bridged.sum())


def test_pileup_over_more_than_two_turns_of_records():
    import torch
    k = K5
    sbwt, _, n_bases = _small()
    n = 2 * PILEUP_TURN + 77 + 1000
    assert n > 2 * PILEUP_TURN + 76, "every wave takes a second record, the first 1 077 waves a third"
    w = pileup_world(k, n_bases, n, 5)
    segs, cat, ms, off = w["segs"], w["cat"], w["ms"], w["off"]
    assert w["n_long"] > 2 * PILEUP_TURN // 1000 and (segs["flags"] & 1).any() and (segs["flags"] & 4).any() and (segs["flags"] & 8).any()
    assert (segs["q_last"].astype(np.int64) + k <= np.diff(off.astype(np.int64))).all(), "every record holds something"
    seqs = np.split(cat, off[1:-1].astype(np.int64))
    # the brute force of the host module on a sample over all three turns, the long gaps among it
    pick = np.unique(np.concatenate([np.arange(0, n, 31), np.arange(0, n, 1000)]))
    assert len(pick) >= 2000 and set((pick // PILEUP_TURN).tolist()) == {0, 1, 2}
    h = dict(strand_seqs=[seqs], ms=[ms], off=off)
    stream = torch.cuda.Stream()
    for run, (skip_multi, cap, count) in enumerate(((False, n, n), (True, n, n), (False, PILEUP_TURN, n + 1000), (False, PILEUP_TURN + 1, n),
                                                    (True, 2 * PILEUP_TURN, 2 * PILEUP_TURN + 3))):
        want, bridged = vector_pile(segs[:cap], cat, ms, off, k, n_bases, skip_multi)
        sample = pick[pick < cap]
        bp, bb = brute_pile(segs[sample], seqs, ms, off, k, n_bases, skip_multi)
        vp, vb = vector_pile(segs[sample], cat, ms, off, k, n_bases, skip_multi)
        assert bb == vb and np.array_equal(bp, vp), "the vectorised statement is the definition's"
        host, hb = locate.pileup_from_segments_host(segs[:cap], cat, ms, off, k, n_bases, skip_multi=skip_multi)
        assert hb == bridged and np.array_equal(host, want)
        if run == 0:
            assert want.max() > 100 and bridged > n + 60 * w["n_long"], "contended words; the long gaps' bases"
            assert int(vector_pile(segs, cat, ms, off, k, n_bases, True)[0].sum()) < int(want.sum())
        p = _Piles(sbwt, 0, seed=run)
        _Uploaded(sbwt, h, segs, capacity=cap, count=count, seed=run).run(p, skip_multi, stream=stream)  # (checks the inputs' guard bands)
        p.pile.assert_intact("run %d" % run)
        got = p.pile.host().view(np.uint32).reshape(-1, 4)
        assert np.array_equal(got, want), (run, np.argwhere(got != want)[:5])


# ---- b. place over more than one turn of long lists
MAX_GAP, MAX_INDEL = 120, 40
GAPS = (1, 3, 9, 20, 45, MAX_GAP - 1, MAX_GAP, MAX_GAP + 1, MAX_GAP + 7)
SHIFTS = (0, 0, 0, 0, 2, -2, 7, -5, MAX_INDEL, -MAX_INDEL, MAX_INDEL + 1, -MAX_INDEL - 1)


def place_lists(seed, n_long):
    """records of a batch in (seq, q_first) order: n_long lists of 5 .. 8 segments (every 50th: 65 .. 130, more than the window), lists
    of 0 .. 4 and sequences without a record between them.  A list follows two tracks - a diagonal of source 0 and one of source 3,
    either FWD or REV - and every segment moves its track's diagonal by a shift on either side of max_indel, a gap on either side of
    max_gap behind the segment in front of it: chains that break, and a runner-up on the other track"""
    rng = np.random.default_rng(seed)
    k = PLACE_K
    rows, s, counts = [], 0, []

    def one_list(n):
        tracks = [[20000 + int(rng.integers(0, 50000)), int(rng.integers(0, 2))], [230000 + int(rng.integers(0, 40000)), int(rng.integers(0, 2))]]
        for t in tracks:  # [diagonal, rev]: p - q forward, p + q reverse
            t[0] += 20000 if t[1] else 0
        ql = int(rng.integers(0, 30)) - 1
        for _ in range(n):
            qf = ql + int(GAPS[rng.integers(0, len(GAPS))])
            span = int(rng.integers(0, 40))
            t = tracks[0 if rng.integers(0, 5) else 1]
            shift = int(SHIFTS[rng.integers(0, len(SHIFTS))])
            t[0] += -shift if t[1] else shift
            pf = t[0] - qf if t[1] else t[0] + qf
            flags = t[1] | (4 if rng.integers(0, 9) == 0 else 0) | (8 if rng.integers(0, 9) == 0 else 0)
            rows.append((s, 1, qf, qf + span, pf, pf - span if t[1] else pf + span, flags))
            ql = qf + span
        counts.append(n)

    for at in range(n_long):
        if at % 3 == 0:
            one_list(int(rng.integers(0, LANE_MAX + 1)))
            s += 1
        if at % 7 == 0:
            counts.append(0)
            s += 1
        one_list(int(rng.integers(WINDOW + 1, 2 * WINDOW + 3)) if at % 50 == 49 else int(rng.integers(LANE_MAX + 1, 9)))
        s += 1
    counts.append(0)
    return np.array(rows, dtype=locate.SEGMENT_DTYPE), s + 1, np.array(counts)


def _merged(into, recs):
    out = into.copy()
    for s in range(len(recs)):
        m = py_merge({f: int(into[s][f]) for f in FIELDS}, {f: int(recs[s][f]) for f in FIELDS})
        out[s] = tuple(m[f] for f in FIELDS)
    return out


def test_place_over_more_than_one_turn_of_long_lists():
    import torch
    sbwt = _hand_handle()
    segs, n_seqs, counts = place_lists(3, WAVE_TURN + 300)
    n_wave = int((counts > LANE_MAX).sum())
    assert n_wave >= WAVE_TURN + 300 and len(segs) // (LANE_MAX + 1) >= WAVE_TURN and n_seqs > WAVE_TURN, "a grid of 4 096 waves and a second turn"
    assert (counts > WINDOW).sum() >= 80 and counts.max() <= 2 * WINDOW + 2 and (counts == 0).sum() > 500
    assert ((counts >= 1) & (counts <= LANE_MAX)).sum() > 1000 and counts[0] <= LANE_MAX and counts[-1] == 0
    assert np.array_equal(np.bincount(segs["seq"], minlength=n_seqs), counts)
    want = py_place(segs, n_seqs, PLACE_K, SRC_OFF, MAX_GAP, MAX_INDEL)
    placed = want[want["source"] != 0xFFFFFFFF]
    assert set(placed["source"].tolist()) == {0, 3} and (placed["flags"] & 1).any() and not (placed["flags"] & 1).all()
    assert (placed["indel"] > 0).sum() > 1000 and (placed["second"] > 0).sum() > 1000 and (placed["n_multi"] > 0).any()
    long_ones = want[counts > LANE_MAX]
    assert (long_ones["n_segs"] < counts[counts > LANE_MAX]).sum() > 1000 and (long_ones["n_segs"] > 1).sum() > 1000, "chains that break, chains that hold"
    same(locate.place_from_segments_host(segs, n_seqs, SRC_OFF, PLACE_K, MAX_GAP, MAX_INDEL), want)
    stream = torch.cuda.Stream()
    d = _Dev(segs, n_seqs, seed=1)
    same(d.run(sbwt, stream=stream, max_gap=MAX_GAP, max_indel=MAX_INDEL), want)
    same(d.run(sbwt, stream=stream, max_gap=MAX_GAP, max_indel=MAX_INDEL), want)  # over what the first run left in d_work and d_place
    # merge: into another call's records (these, seven sequences on, as the '-' strand's), twice
    other = np.roll(want, 7)
    other["strand"][other["source"] != 0xFFFFFFFF] = 2
    once = _merged(other, want)
    twice = _merged(once, want)
    same(locate.place_from_segments_host(segs, n_seqs, SRC_OFF, PLACE_K, MAX_GAP, MAX_INDEL, merge_into=other), once)
    m = _Dev(segs, n_seqs, seed=2, place_data=other)
    same(m.run(sbwt, merge=True, stream=stream, max_gap=MAX_GAP, max_indel=MAX_INDEL), once)
    same(m.run(sbwt, merge=True, stream=stream, max_gap=MAX_GAP, max_indel=MAX_INDEL), twice)
    assert (once["strand"] == 2).any() and (once["strand"] == 1).any() and (twice["second"] != once["second"]).any()


# ---- c. more than 1 048 576 records
def _rows_by_position(table, n_bases):
    """(row of the FWD entry at position p or -1, the same for REV, the rows that have an entry)"""
    fwd, rv = np.full(n_bases + 2, -1, dtype=np.int64), np.full(n_bases + 2, -1, dtype=np.int64)
    rows = np.flatnonzero(table != NONE)
    e = table[rows]
    is_rev = (e & REV) != 0
    fwd[(e & PMASK)[~is_rev]] = rows[~is_rev]
    rv[(e & PMASK)[is_rev]] = rows[is_rev]
    return fwd, rv, rows


def vector_segments(table, d, lo, off, k, strand, n_bases):
    """(records, delta) at bridge 0 from the rule: an anchor starts a record unless the base in front of it is an anchor of its sequence
    on the same strand and diagonal, and ends one unless the base behind it is"""
    total = int(off[-1])
    seq = np.searchsorted(off, np.arange(total), side="right") - 1
    q = np.arange(total) - off[seq].astype(np.int64) - (k - 1)
    anchor = (d[:total] == k) & (q >= 0) & (lo < len(table))
    e = table[np.where(anchor, lo, 0)].astype(np.int64)
    p, rv = e & PMASK, (e & REV) != 0
    join = np.zeros(total, dtype=bool)  # join[i]: i - 1 and i are joined
    join[1:] = anchor[1:] & anchor[:-1] & (seq[1:] == seq[:-1]) & (rv[1:] == rv[:-1]) & (np.where(rv[1:], p[:-1] - p[1:], p[1:] - p[:-1]) == 1)
    starts = np.flatnonzero(anchor & ~join)
    ends = np.flatnonzero(anchor & ~np.concatenate([join[1:], [False]]))
    assert len(starts) == len(ends)
    recs = np.zeros(len(starts), dtype=locate.SEGMENT_DTYPE)
    recs["seq"], recs["strand"], recs["q_first"], recs["q_last"] = seq[starts], strand, q[starts], q[ends]
    recs["pos_first"], recs["pos_last"] = p[starts], p[ends]
    multi = (e & MULTI) != 0
    recs["flags"] = rv[starts].astype(np.int64) | 4 * multi[starts] | 8 * multi[ends]
    delta = np.zeros(n_bases + 1, dtype=np.int64)
    low = np.where(rv[starts], p[ends], p[starts])  # FWD covers [pos_first, pos_last + k), REV [pos_last, pos_first + k)
    high = np.where(rv[starts], p[starts], p[ends]) + k
    np.add.at(delta, low, 1)
    np.add.at(delta, high, -1)
    return recs, (delta & 0xFFFFFFFF).astype(np.uint32)


def dense_world(table, n_bases, k, n_seqs, seq_len, seed):
    """every position an anchor (d = k everywhere: the first k - 1 bases of a sequence are none all the same), rows drawn at random,
    every tenth one the row of the position one on from its neighbour's - a join at bridge 0"""
    rng = np.random.default_rng(seed)
    fwd, rv, rows = _rows_by_position(table, n_bases)
    total = n_seqs * seq_len
    lo = rows[rng.integers(0, len(rows), total)]
    e = table[lo].astype(np.int64)
    nxt = np.where((e & REV) != 0, rv[(e & PMASK) - 1], fwd[(e & PMASK) + 1])  # (position 0 - 1 reads the array's last word: -1)
    go = np.flatnonzero((rng.integers(0, 10, total - 1) == 0) & (nxt[:-1] >= 0)) + 1
    go = go[~np.isin(go - 1, go)]
    lo[go] = nxt[go - 1]
    off = (np.arange(n_seqs + 1) * seq_len).astype(np.uint64)
    return np.full(total, k, dtype=np.uint8), lo.astype(np.uint32), off


def test_more_than_a_stride_of_records_through_segments_and_place():
    import torch
    k = K5
    sbwt, table, n_bases = _small()
    soff = sbwt.source_offsets()
    n_seqs, seq_len = 160_000, 12
    d, lo, off = dense_world(table, n_bases, k, n_seqs, seq_len, 9)
    total = int(off[-1])
    want, want_delta = vector_segments(table, d, lo, off, k, 1, n_bases)
    n = len(want)
    assert n > STRIDE_TURN + 4096, "segment_clear_kernel and place_range_kernel stride"
    assert n < n_seqs * (seq_len - k + 1), "the draw joins some neighbours"
    assert (want["q_last"] > want["q_first"]).sum() > 10000 and (want["flags"] & 1).any() and (want["flags"] & 12).any()
    host_delta = np.zeros(n_bases + 1, dtype=np.uint32)
    host, hn = locate.segments_from_ms_host(table, k, d, lo, off, 0, 1, n, n_bases, host_delta)
    assert hn == n and np.array_equal(host, want) and np.array_equal(host_delta, want_delta)
    # the brute-force chain builder on the first sequences
    few = 300
    lists = [[(q, int(table[lo[s * seq_len + q + k - 1]])) for q in range(seq_len - k + 1)] for s in range(few)]
    assert as_tuples(want[want["seq"] < few]) == brute_chains(lists, 0, 1)
    dev = _dev()
    t_d = torch.from_numpy(np.concatenate([d, np.zeros(16, dtype=np.uint8)])).to(dev)
    t_lo = torch.from_numpy(lo.astype(np.int32)).to(dev)
    t_off = torch.from_numpy(off.astype(np.int64)).to(dev)
    sb = locate.segments_work_bytes(n_seqs, total)
    work, cnt = Guarded("d_work", sb, 1 << 16, dev, seed=1), Guarded("d_n_segs", 8, 4096, dev, seed=2)
    segs = Guarded("d_segs", SEG * n, 1 << 16, dev, seed=3)
    delta = Guarded("d_delta", 4 * (n_bases + 1), 1 << 16, dev, seed=4, data=np.zeros(4 * (n_bases + 1), dtype=np.uint8))
    pwb = locate.place_work_bytes(n_seqs, n)
    pwork = Guarded("d_work", pwb, 1 << 16, dev, seed=5)
    place = Guarded("d_place", locate.PLACE_DTYPE.itemsize * n_seqs, 1 << 16, dev, seed=6)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    locate.segments_dev(sbwt, t_d, t_lo, t_off, n_seqs, total, segs.ptr, n, cnt.ptr, work.ptr, sb, bridge=0, delta=delta.ptr, stream=stream)
    locate.place_dev(sbwt, segs.ptr, cnt.ptr, n, n_seqs, place.ptr, pwork.ptr, pwb, stream=stream)
    torch.cuda.synchronize()
    for g in (work, cnt, segs, delta, pwork, place):
        g.assert_intact()
    assert int(cnt.host().view(np.uint64)[0]) == n
    got = segs.host().view(locate.SEGMENT_DTYPE)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:5]
    assert np.array_equal(delta.host().view(np.uint32), want_delta)
    # place: the host form for every sequence, the chain builder on a sample with the sequences around record 1 048 576 in it
    placed = place.host().view(locate.PLACE_DTYPE)
    same(placed, locate.place_from_segments_host(want, n_seqs, soff, k))
    edge = int(want["seq"][STRIDE_TURN])
    pick = np.unique(np.concatenate([np.arange(0, n_seqs, 149), np.arange(edge - 3, edge + 4), [n_seqs - 1]]))
    assert len(pick) >= 1000 and int(want["seq"][STRIDE_TURN - 1]) in pick and edge in pick
    sub = want[np.isin(want["seq"], pick)].copy()
    sub["seq"] = np.searchsorted(pick, sub["seq"])
    chains = py_place(sub, len(pick), k, soff)
    same(placed[pick], chains)
    assert (chains["n_segs"] > 1).sum() > 50 and (chains["second"] > 0).sum() > 500 and (np.bincount(want["seq"]) > LANE_MAX).sum() > STRIDE_TURN // 16


# ---- d. a handle of more than 1 048 576 rows and source bases
BIG_K = 31
_big = {}


def big_sources(seed=17):
    """about 40 small sources - empty ones, ones shorter than k - around one of 1.1 M bases with an exact repeat, an inverted repeat and
    an N; those behind it lie beyond base 524 288"""
    rng = np.random.default_rng(seed)
    small = [0, 5, BIG_K - 1, BIG_K, 64, 200, 1000, 0, 333, BIG_K + 1]
    big = ACGT[rng.integers(0, 4, 1_100_000)]
    big[900_000:905_000] = big[100_000:105_000]
    big[700_000:703_000] = revcomp(big[200_000:203_000])
    big[550_000] = ord("N")
    return [ACGT[rng.integers(0, 4, small[i % 10])] for i in range(15)] + [big] + [ACGT[rng.integers(0, 4, small[(i + 3) % 10])] for i in range(25)]


def packed_kmers(cat, soff, k):
    """(forward k-mer, its reverse complement, valid) of the window that starts at every base: 2 bits a base in a uint64; valid: A, C, G
    and T alone, inside one source"""
    code = CODE[cat]
    m = len(cat) - k + 1
    c = (code & 3).astype(np.uint64)
    v, r = np.zeros(m, dtype=np.uint64), np.zeros(m, dtype=np.uint64)
    for j in range(k):
        v = (v << np.uint64(2)) | c[j:j + m]
        r |= (np.uint64(3) - c[j:j + m]) << np.uint64(2 * j)
    bad = np.concatenate([[0], np.cumsum(code == 4)])
    src = np.searchsorted(soff[1:], np.arange(len(cat)), side="right")
    return v, r, (bad[k:] - bad[:m] == 0) & (src[:m] == src[k - 1:])


def brute_entries(v, r, valid):
    """the entries of all distinct k-mers, sorted: by (k-mer, FWD before REV, p) the first of each group, MULTI when there are more"""
    p = np.flatnonzero(valid)
    kmer = np.concatenate([v[p], r[p]])
    rev = np.concatenate([np.zeros(len(p), dtype=np.int64), np.ones(len(p), dtype=np.int64)])
    pos = np.concatenate([p, p])
    order = np.lexsort((pos, rev, kmer))
    kmer, rev, pos = kmer[order], rev[order], pos[order]
    first = np.flatnonzero(np.concatenate([[True], kmer[1:] != kmer[:-1]]))
    size = np.diff(np.concatenate([first, [len(kmer)]]))
    return np.sort((pos[first] | np.where(rev[first] == 1, REV, 0) | np.where(size > 1, MULTI, 0)).astype(np.uint32))


def big_handle():
    if not _big:
        srcs = big_sources()
        sbwt = kbo_amd.build(srcs, kbo_amd.BuildOpts(k=BIG_K, add_revcomp=True, num_threads=4), device=-1)[0]
        kbo_amd.add_positions(sbwt, srcs, add_revcomp=True)
        _big["x"] = (sbwt, srcs, src_offsets(srcs))
    return _big["x"]


def test_table_of_more_than_a_stride_of_rows_against_packed_kmers():
    import torch
    k = BIG_K
    sbwt, srcs, soff = big_handle()
    n_bases, n_rows = int(soff[-1]), sbwt.n_sets()
    assert n_rows > STRIDE_TURN + 4096 and n_bases > STRIDE_TURN + 4096, "locate_entries_kernel and locate_mark_kernel stride"
    lens = np.diff(soff.astype(np.int64))
    assert (lens == 0).sum() >= 4 and ((lens > 0) & (lens < k)).sum() >= 4 and (soff[:-1][lens > 0] > SCAN_TURN).sum() >= 10
    # the packed brute force itself first: on the small world it gives the entries the oracle spells row by row
    small, _, _, spelled = world(k, True, LENS)
    assert np.array_equal(brute_entries(*packed_kmers(np.concatenate(small), src_offsets(small), k)), np.sort(spelled[spelled != NONE]))
    cat = np.concatenate(srcs)
    v, r, valid = packed_kmers(cat, soff, k)
    want = brute_entries(v, r, valid)
    assert (want & MULTI).sum() > 5000 and ((want & REV) != 0).sum() > len(want) // 3 and (~valid).sum() > k
    table = sbwt.positions()
    assert len(table) == n_rows
    has = table != NONE
    assert int((~has).sum()) == n_rows - len(want), "a row without an entry is no k-mer of the sources"
    assert np.array_equal(np.sort(table[has]), want)
    assert (table[STRIDE_TURN:] & MULTI)[has[STRIDE_TURN:]].any(), "MULTI rows in the second turn of locate_entries_kernel"
    # every base of the sources walked at depth k: the entry of its row names an occurrence of the window that ends there
    b = _Batch(sbwt, [s for s in srcs if len(s)], 1, seed=3)
    stream = torch.cuda.Stream()
    b.walk(1, stream)
    torch.cuda.synchronize()
    ms, lo = b.ms.cpu().numpy()[:n_bases], b.lo.cpu().numpy().view(np.uint32)[:n_bases]
    ends = np.flatnonzero(valid) + k - 1
    assert (ms[ends] == k).all() and int((ms == k).sum()) == len(ends), "the windows of the sources, and no other, reach depth k"
    e = table[lo[ends]]
    assert (e != NONE).all()
    p = (e & PMASK).astype(np.int64)
    assert valid[p].all() and np.array_equal(np.where((e & REV) != 0, r[p], v[p]), v[ends - k + 1])
    assert np.array_equal((e & REV) == 0, np.isin(v[ends - k + 1], v[valid])), "FWD before REV"
    # the same table from slabs cut at 600 000 bases
    L = kbo_amd.lib()
    L.kbo_set_positions_slab_bases(600_000)
    try:
        kbo_amd.add_positions(sbwt, srcs, add_revcomp=True)
    finally:
        L.kbo_set_positions_slab_bases(0)
    assert np.array_equal(sbwt.positions(), table)


def test_depth_and_sites_carry_across_the_rounds_of_the_sums():
    import torch
    sbwt, srcs, soff = big_handle()
    n = int(soff[-1])
    assert n > 2 * SCAN_TURN + 2048 and n % 2048, "scan_sums_kernel and site_sums_kernel take a third round, the last chunk is partial"
    rng = np.random.default_rng(23)
    # a sparse delta: entries in the first chunk, beyond every round of the sums, in the last chunk; sums that wrap
    delta = np.zeros(n + 1, dtype=np.uint32)
    at = np.unique(np.concatenate([rng.integers(0, n, 5000), [0, 1, 2047, 2048, SCAN_TURN - 1, SCAN_TURN, SCAN_TURN + 1, 2 * SCAN_TURN, n - 1, n - 5]]))
    delta[at] = rng.integers(0, 1 << 32, len(at), dtype=np.uint64).astype(np.uint32)
    delta[at[::3]] = 1
    depth_want = np.cumsum(delta[:-1], dtype=np.uint32)
    assert delta[:2048].any() and delta[n // 2048 * 2048:n].any() and delta[SCAN_TURN:].any()
    # a sparse pile over depths of 0 .. 12: counts at the thresholds and one below
    pile = np.zeros((n, 4), dtype=np.uint32)
    rows = np.unique(np.concatenate([rng.integers(0, n, 6000), [0, 2047, 2048, SCAN_TURN - 1, SCAN_TURN, 2 * SCAN_TURN - 1, 2 * SCAN_TURN, n - 1]]))
    pile[rows] = rng.integers(0, 7, (len(rows), 4)) * (rng.integers(0, 3, (len(rows), 4)) == 0)
    depth = np.zeros(n, dtype=np.uint32)
    depth[rows] = rng.integers(0, 13, len(rows))
    lens = np.diff(soff.astype(np.int64))
    edges = np.unique(np.concatenate([soff[:-1].astype(np.int64)[lens > 0], soff[1:].astype(np.int64)[lens > 0] - 1]))
    pile[edges], depth[edges] = [0, 5, 0, 1], 9  # the first and the last base of every source: sites
    nz = np.flatnonzero(pile.any(axis=1))
    t = (3, 1, 2)
    want = brute_sites(pile, depth, soff, *t, rows=nz.tolist())  # (a row of zeros is no site: min_count >= 1)
    top = pile[nz].max(axis=1).astype(np.int64)
    dd = depth[nz].astype(np.int64)
    assert ((top == 3) & (2 * top >= dd)).any() and ((top == 2) & (dd == 0)).any() and ((top >= 3) & (2 * top == dd)).any() and ((top >= 3) & (2 * top == dd - 1)).any()
    srcs_hit = {s[1] for s in want}
    assert len(srcs_hit) >= 30 and min(srcs_hit) < 15 < max(srcs_hit), "sites in the small sources on both sides of the long one"
    assert sum(s[0] >= 2 * SCAN_TURN for s in want) > 20 and sum(s[0] < SCAN_TURN for s in want) > 100 and len(want) > 1000
    host, hn = locate.pileup_sites_host(pile, depth, soff, min_count=t[0], frac_num=t[1], frac_den=t[2])
    assert hn == len(want) and site_tuples(host) == want
    p = _Piles(sbwt, len(want), seed=1)
    p.pile.data, p.delta.data = pile.view(np.uint8).ravel(), delta.view(np.uint8)
    p.pile.fill(2)
    p.delta.fill(3)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    locate.depth_finish_dev(sbwt, p.delta.ptr, p.depth.ptr, p.dwork.ptr, p.dwb, stream=stream)
    torch.cuda.synchronize()
    for g in (p.delta, p.depth, p.dwork):
        g.assert_intact()
    got = p.depth.host().view(np.uint32)
    assert np.array_equal(got, depth_want), np.flatnonzero(got != depth_want)[:5]
    assert not p.delta.changed(), "d_delta is read only"
    # the sites of the uploaded pile against the uploaded depth, at capacities exact, below and 0
    p.depth.data = depth.view(np.uint8)
    p.depth.fill(4)
    for cap in (len(want), len(want) // 2, 0):
        p.site_cap = cap
        p.sites = Guarded("d_sites", SITE * cap, 1 << 16, p.dev, seed=5 + cap)
        p.cnt.fill(6)
        p.twork.fill(7)
        torch.cuda.synchronize()
        p.finish(t, stream, depth=False)
        torch.cuda.synchronize()
        _, _, sites, cnt = p.results("capacity %d" % cap)
        assert cnt == len(want) and np.array_equal(sites, host[:cap])
        assert not p.pile.changed() and not p.depth.changed(), "d_pile and d_depth are read only"


# ---- e. more than 256 sequence starts in one tile
CYCLE = (0, 0, 5, 6, 9, 1, 12, 0, 4, 7, 0, 13, 2, 5)


def tiny_lengths(tile, halo):
    """lengths that cycle through 0, 0, 5, 6, 9, 1, 12, 0, ... over more than three tiles, the first and the last sequence empty, with
    runs of empty sequences where a tile begins, where the positions the next tile looks at begin, and inside a tile"""
    lens, total = [], 0

    def cycle_until(stop):
        nonlocal total
        while total < stop:
            n = min(CYCLE[len(lens) % len(CYCLE)], stop - total)
            lens.append(n)
            total += n

    cycle_until(tile)
    lens += [0] * 330          # all at base `tile`: where tile 1 begins
    cycle_until(2 * tile - halo)
    lens += [0] * 700          # where the positions tile 2 looks at begin
    cycle_until(2 * tile + 900)
    lens += [0] * 1500
    cycle_until(3 * tile + 100)
    lens += [0] * 600
    cycle_until(3 * tile + 411)
    lens.append(0)
    return lens


def tiny_world(table, n_bases, k, lens, seed):
    """(d, lo, off, anchor lists): d = k at four positions of five - at the first k - 1 of a sequence too, where it makes no anchor -
    rows along a diagonal of the sequence's own (FWD or REV) where the table has them, a random row at every sixth position and where
    it has none; a few rows beyond the table: no anchors"""
    rng = np.random.default_rng(seed)
    fwd, rv, rows = _rows_by_position(table, n_bases)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    total = int(off[-1])
    seq = np.searchsorted(off, np.arange(total), side="right") - 1
    q = np.arange(total) - off[seq].astype(np.int64) - (k - 1)
    d = np.where(rng.integers(0, 5, total) == 0, rng.integers(0, k, total), k).astype(np.uint8)
    blank = np.flatnonzero((np.asarray(lens) >= 12) & (np.arange(len(lens)) % 4 == 0))  # anchors at the first and the last window alone
    d[np.isin(seq, blank) & (q > 0) & (np.arange(total) + 1 < off[seq + 1].astype(np.int64))] = 0
    p0, dirs = rng.integers(0, n_bases, len(lens)), rng.integers(0, 2, len(lens))
    want_p = np.clip(np.where(dirs[seq] == 1, p0[seq] - q, p0[seq] + q), 0, n_bases + 1)
    lo = np.where(dirs[seq] == 1, rv[want_p], fwd[want_p])
    rand = rows[rng.integers(0, len(rows), total)]
    lo = np.where((lo < 0) | (rng.integers(0, 6, total) == 0), rand, lo)
    wild = rng.integers(0, 40, total) == 0
    lo[wild] = np.where(rng.integers(0, 2, int(wild.sum())) == 0, len(table), 0xFFFFFFFF)
    lists = [[] for _ in lens]
    for i in np.flatnonzero((d == k) & (q >= 0) & (lo < len(table))).tolist():
        lists[seq[i]].append((int(q[i]), int(table[lo[i]])))
    return d, lo.astype(np.uint32), off, lists


def test_more_than_a_turn_of_sequence_starts_in_one_tile():
    import torch
    k = K5
    sbwt, table, n_bases = _small()
    tile, halo = _geometry()
    lens = tiny_lengths(tile, halo)
    d, lo, off, lists = tiny_world(table, n_bases, k, lens, 13)
    n_seqs, total = len(lens), int(off[-1])
    assert lens[0] == 0 and lens[-1] == 0 and n_seqs > 3000 and total > 3 * tile
    for t in range((total + tile - 1) // tile):  # the starts tile_sequences strides over: every sequence that begins inside the positions tile t looks at
        ext_lo, ext_hi = max(0, t * tile - halo), min(total, (t + 1) * tile + halo)
        assert ((off[:-1] > ext_lo) & (off[:-1] < ext_hi)).sum() > 2 * STARTS_TURN, t
    assert (off[:-1] == tile).sum() > 300 and (off[:-1] == 2 * tile - halo).sum() > 300
    dev = _dev()
    t_d = torch.from_numpy(np.concatenate([d, np.zeros(16, dtype=np.uint8)])).to(dev)
    t_lo = torch.from_numpy(lo.astype(np.int32)).to(dev)
    t_off = torch.from_numpy(off.astype(np.int64)).to(dev)
    sb = locate.segments_work_bytes(n_seqs, total)
    seen = {}
    for bridge in (0, k, 255):
        want = brute_chains(lists, bridge, 1)
        seen[bridge] = len(want)
        want_delta = brute_delta(want, k, n_bases)
        host_delta = np.zeros(n_bases + 1, dtype=np.uint32)
        host, hn = locate.segments_from_ms_host(table, k, d, lo, off, bridge, 1, len(want), n_bases, host_delta)
        assert hn == len(want) and as_tuples(host) == want and np.array_equal(host_delta, want_delta)
        work, cnt = Guarded("d_work", sb, 1 << 16, dev, seed=bridge), Guarded("d_n_segs", 8, 4096, dev, seed=1)
        segs = Guarded("d_segs", SEG * len(want), 1 << 16, dev, seed=2)
        delta = Guarded("d_delta", 4 * (n_bases + 1), 1 << 16, dev, seed=3, data=np.zeros(4 * (n_bases + 1), dtype=np.uint8))
        torch.cuda.synchronize()
        locate.segments_dev(sbwt, t_d, t_lo, t_off, n_seqs, total, segs.ptr, len(want), cnt.ptr, work.ptr, sb, bridge=bridge, delta=delta.ptr)
        torch.cuda.synchronize()
        for g in (work, cnt, segs, delta):
            g.assert_intact("bridge %d" % bridge)
        assert int(cnt.host().view(np.uint64)[0]) == len(want)
        got = segs.host().view(locate.SEGMENT_DTYPE)
        assert np.array_equal(got, host), (bridge, np.flatnonzero(got != host)[:5])
        assert np.array_equal(delta.host().view(np.uint32), want_delta)
    assert seen[0] > seen[k] > seen[255] > 500, "joins across one hole and across several"
