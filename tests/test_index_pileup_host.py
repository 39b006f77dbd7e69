"""Pileup (kbo_hip.h) on the host: kbo_pileup_from_segments_host and kbo_pileup_sites_host word for word against brute force written
here from the definitions - for every record the set of bases its anchors' windows cover, subtracted from its extent, projected and
counted; for every base the threshold rule in Python integers - on worlds in the style of tests/test_index_locate_host.py (three
sources of 2 - 4 kbp, k = 5, 31 and 96, indexes with and without add_revcomp, MS bytes through the oracle's walk) at bridge 0, k, k + 5
and 255, with every planted case asserted to occur; the sites' thresholds at equality and one below it; capacities below the count;
the argument errors and their order; pileup_snps end to end on a tiled sample; tools/index_pileup_check.cpp plain and under ASan +
UBSan.  No GPU.  tests/test_gpu_index_pileup.py takes the batches and the brute force from here."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import kbo_amd
from kbo_amd import _capi, locate

from test_index_locate_host import ACGT, COMP, _other, brute_depth, brute_segments, as_tuples, revcomp, src_offsets, walk, world

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_EMPTY_QUERY, E_BAD_ARG, E_UNSUPPORTED = -1, -4, -8
LENS = (4000, 3000, 2000)
KS = [5, 31, 96]
BRIDGES = lambda k: [0, k, k + 5, 255]  # noqa: E731
NEW_SYMBOLS = ["kbo_pileup_dev", "kbo_pileup_sites_work_bytes", "kbo_pileup_sites_dev", "kbo_pileup_from_segments_host", "kbo_pileup_sites_host",
               "kbo_pileup_batch"]
SAME = 70  # reads with one and the same substitution


# ---- brute force from the definitions
def brute_pile(segs, seqs, ms, off, k, n_bases, skip_multi, pile=None):
    """(pile int64[n_bases, 4], bridged bases) of records given as tuples or a SEGMENT_DTYPE array over the batch `seqs` with its MS bytes"""
    pile = np.zeros((n_bases, 4), dtype=np.int64) if pile is None else pile
    concat = np.concatenate([np.asarray(s, dtype=np.uint8) for s in seqs] + [np.zeros(0, dtype=np.uint8)])
    bridged = 0
    for seq, _, qf, ql, pf, _, flags in (segs if isinstance(segs, list) else as_tuples(segs)):
        if seq >= len(seqs) or qf > ql or (skip_multi and flags & 12):
            continue
        o, e = int(off[seq]), int(off[seq + 1])
        if not (o <= e <= len(concat)) or o + ql + k > e:
            continue
        covered = set()
        for w in range(qf, ql + 1):
            if ms[o + w + k - 1] == k:
                covered.update(range(w, w + k))
        for x in sorted(set(range(qf, ql + k)) - covered):
            bridged += 1
            byte = int(concat[o + x])
            j = pf + k - 1 - (x - qf) if flags & 1 else pf + (x - qf)
            col = b"ACGT".find(bytes([int(COMP[byte]) if flags & 1 else byte]))
            if col >= 0 and 0 <= j < n_bases:
                pile[j, col] += 1
    return pile, bridged


def brute_sites(pile, depth, soff, min_count, num, den, rows=None):
    """rows: the bases looked at, ascending (None: every one)"""
    out = []
    for j in (range(len(depth)) if rows is None else rows):
        d = int(depth[j])
        if any(int(c) >= min_count and int(c) * den >= num * d for c in pile[j]):
            src = max(s for s in range(len(soff) - 1) if int(soff[s]) <= j)
            out.append((j, src, d, tuple(int(c) for c in pile[j]), 0))
    return out


def site_tuples(sites):
    return [(int(s["pos"]), int(s["source"]), int(s["depth"]), tuple(int(c) for c in s["count"]), int(s["reserved"])) for s in sites]


# ---- the planted cases
def _with(seq, edits):
    q = seq.copy()
    for at, b in edits:
        q[at] = _other(q[at]) if b is None else b
    return q


def planted(srcs, k):
    """name -> (sequence, what it is there for); every read but the named ones comes from a stretch of the first source behind its
    planted repeats"""
    s0, s1 = srcs[0], srcs[1]
    q = {}
    n = 3 * k + 20
    q["lone"] = _with(s0[1000:1000 + n], [(n // 2, None)])
    for d in (5, 6):  # the anchors around two substitutions d <= k apart are d + k + 1 apart: joined iff d <= bridge - k
        q["pair%d" % d] = _with(s0[1200:1200 + n + d], [(n // 2, None), (n // 2 + d, None)])
    at = max(67, k + 4)  # (behind a first window; the k windows that hold it are no anchors: 63 and 64 among them)
    q["straddle63"] = _with(s0[1400:1400 + at + k + 30], [(at, None)])
    q["straddle127"] = _with(s0[1700:1700 + 131 + k + 30], [(131, None)])  # ... 127 and 128
    subs = list(range(k + 9, k + 9 + 71, k - 1))  # windows 10 .. the last substitution hold one: more than 64 of them
    q["long_gap"] = _with(s0[2000:2000 + subs[-1] + k + 20], [(p, None) for p in subs])
    q["reverse"] = revcomp(_with(s0[2400:2400 + n], [(n // 2, None)]))
    q["n_base"] = _with(s0[2600:2600 + n], [(n // 2, ord("N"))])
    lower = s0[2800:2800 + n].copy()
    lower[n // 2] = ord(chr(lower[n // 2]).lower())
    q["lower"] = lower
    base = s0[3000:3000 + 2 * k + 30]
    q["insertion"] = np.concatenate([base[:len(base) // 2], ACGT[:1], base[len(base) // 2:]])
    q["deletion"] = np.concatenate([base[:len(base) // 2], base[len(base) // 2 + 1:]])
    q["multi"] = _with(s0[55:55 + n + 20], [(2 * k + 20, None)])  # begins inside the first copy of the exact repeat
    q["junction"] = _with(np.concatenate([s0[len(s0) - (k + 10):], s1[:k + 10]]), [(k + 7, None)])  # 3 bases in front of the junction
    q["short"] = s0[300:300 + k - 1].copy()
    q["empty"] = np.zeros(0, dtype=np.uint8)
    same = _with(s0[3300:3300 + n], [(n // 2, None)])
    for r in range(SAME):
        q["same%d" % r] = same
    return q


_PILES = {}


def host_piles(k, rc, bridge, skip_multi):
    """the planted batch piled up on the host for '+' then '-' into one pile and one delta, checked against brute force on the way:
    -> dict(names, seqs, segs [per strand], ms [per strand], off, pile, depth, bridged, srcs, soff)"""
    key = (k, rc, bridge, skip_multi)
    if key in _PILES:
        return _PILES[key]
    srcs, oi, occ, table = world(k, rc, LENS)
    soff = src_offsets(srcs)
    n_bases = int(soff[-1])
    qs = planted(srcs, k)
    names, seqs = list(qs), list(qs.values())
    delta = np.zeros(n_bases + 1, dtype=np.uint32)
    pile = np.zeros((n_bases, 4), dtype=np.uint32)
    want = np.zeros((n_bases, 4), dtype=np.int64)
    want_depth = np.zeros(n_bases, dtype=np.uint32)
    out = dict(names=names, seqs=seqs, segs=[], ms=[], strand_seqs=[], bridged=[], srcs=srcs, soff=soff, n_bases=n_bases)
    for strand in (1, 2):
        ss = [revcomp(s) for s in seqs] if strand == 2 else seqs
        d, lo, off = walk(oi, ss)
        recs = brute_segments(ss, occ, k, bridge, strand)
        segs, n = locate.segments_from_ms_host(table, k, d, lo, off, bridge, strand, len(recs) + 3, n_bases, delta)
        assert n == len(recs) and as_tuples(segs) == recs
        _, got_bridged = locate.pileup_from_segments_host(segs, np.concatenate(ss), d, off, k, n_bases, skip_multi=skip_multi, pile=pile)
        _, want_bridged = brute_pile(recs, ss, d, off, k, n_bases, skip_multi, want)
        assert got_bridged == want_bridged, (strand, got_bridged, want_bridged)
        assert np.array_equal(pile, want), (strand, np.argwhere(pile != want)[:5])
        want_depth += brute_depth(recs, k, n_bases)
        out["segs"].append(segs)
        out["ms"].append(d)
        out["strand_seqs"].append(ss)
        out["bridged"].append(got_bridged)
        out["off"] = off
    out["pile"] = pile
    out["depth"] = np.cumsum(delta[:-1], dtype=np.uint32)
    assert np.array_equal(out["depth"], want_depth)
    _PILES[key] = out
    return out


def _recs_of(h, strand, name):
    i = h["names"].index(name)
    return [r for r in as_tuples(h["segs"][strand - 1]) if r[0] == i]


def _non_anchor_windows(h, strand, rec, k):
    o = int(h["off"][rec[0]])
    return [w - rec[2] for w in range(rec[2], rec[3] + 1) if h["ms"][strand - 1][o + w + k - 1] != k]


def _one_pile(h, strand, name, k, skip_multi=False):
    """the pile of one sequence's records alone, by brute force"""
    return brute_pile(_recs_of(h, strand, name), h["strand_seqs"][strand - 1], h["ms"][strand - 1], h["off"], k, h["n_bases"], skip_multi)


# ---- the pile
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("rc", [False, True])
def test_pile_and_sites_equal_brute_force_from_the_definitions(k, rc):
    for bridge in BRIDGES(k):
        for skip_multi in (False, True):
            h = host_piles(k, rc, bridge, skip_multi)  # (every word of the pile against brute force, strand by strand)
            pile, depth = h["pile"], h["depth"]
            assert (pile.sum(axis=1) <= depth).all(), "a bridged base lies inside its segment's extent"
            if bridge == 0:
                assert not pile.any() and h["bridged"] == [0, 0], "adjacent windows leave no base uncovered"
            for min_count, num, den in ((1, 0, 1), (3, 1, 2), (2, 1, 1), (SAME, 1, 1), (1, 2, 1)):
                want = brute_sites(pile, depth, h["soff"], min_count, num, den)
                got, n = locate.pileup_sites_host(pile, depth, h["soff"], min_count=min_count, frac_num=num, frac_den=den)
                assert n == len(want) and site_tuples(got) == want, (bridge, min_count, num, den)
                few, n2 = locate.pileup_sites_host(pile, depth, h["soff"], capacity=len(want) // 2, min_count=min_count, frac_num=num, frac_den=den)
                assert n2 == n and site_tuples(few) == want[:len(want) // 2]
                none, n3 = locate.pileup_sites_host(pile, depth, h["soff"], capacity=0, min_count=min_count, frac_num=num, frac_den=den)
                assert n3 == n and len(none) == 0


@pytest.mark.parametrize("k", [31, 96])
@pytest.mark.parametrize("rc", [False, True])
def test_every_planted_case_occurs(k, rc):
    """(k = 5 is left to the comparison above: nearly every 5-mer occurs somewhere in 9 000 bases)"""
    at_k, at_k5, at_255 = (host_piles(k, rc, b, False) for b in (k, k + 5, 255))
    n = 3 * k + 20
    # a lone substitution mid-read: one bridged base, one count in the column of the read's base at its source coordinate
    (rec,) = _recs_of(at_k, 1, "lone")
    p, b = _one_pile(at_k, 1, "lone", k)
    assert b == 1 and p.sum() == 1 and p[1000 + n // 2].sum() == 1
    assert p[1000 + n // 2, b"ACGT".find(bytes([int(at_k["seqs"][at_k["names"].index("lone")][n // 2])]))] == 1
    # two substitutions d apart: joined iff d <= bridge - k
    assert len(_recs_of(at_k5, 1, "pair5")) == 1 and _one_pile(at_k5, 1, "pair5", k)[1] == 6
    assert len(_recs_of(at_k5, 1, "pair6")) == 2 and _one_pile(at_k5, 1, "pair6", k)[1] == 0
    assert len(_recs_of(at_k, 1, "pair5")) == 2 and _one_pile(at_255, 1, "pair6", k)[1] == 7
    # gaps across the rounds of 64 windows
    for name, edge in (("straddle63", 63), ("straddle127", 127)):
        (rec,) = _recs_of(at_k, 1, name)
        gap = _non_anchor_windows(at_k, 1, rec, k)
        assert edge in gap and edge + 1 in gap and _one_pile(at_k, 1, name, k)[1] == 1
    (rec,) = _recs_of(at_255, 1, "long_gap")
    gap = _non_anchor_windows(at_255, 1, rec, k)
    assert len(gap) > 64 and gap == list(range(gap[0], gap[0] + len(gap))), "ONE gap of more than 64 windows"
    assert _one_pile(at_255, 1, "long_gap", k)[1] == len(gap) - k + 1
    # a REV-strand read: with add_revcomp the '+' walk finds it on the reverse strand and counts the complement
    fwd_read = revcomp(at_k["seqs"][at_k["names"].index("reverse")])
    col = b"ACGT".find(bytes([int(fwd_read[n // 2])]))
    if rc:
        (rec,) = _recs_of(at_k, 1, "reverse")
        assert rec[6] & 1 and _one_pile(at_k, 1, "reverse", k)[0][2400 + n // 2, col] == 1
    else:
        assert not _recs_of(at_k, 1, "reverse")
    assert _one_pile(at_k, 2, "reverse", k)[0][2400 + n // 2, col] == 1, "... and the '-' walk finds it forward"
    # an N and a lower-case byte at a bridged base: bridged, counted in no column
    for name in ("n_base", "lower"):
        p, b = _one_pile(at_k, 1, name, k)
        assert len(_recs_of(at_k, 1, name)) == 1 and b == 1 and p.sum() == 0
    # an insertion and a deletion: two segments, nothing bridged between them
    for name in ("insertion", "deletion"):
        assert len(_recs_of(at_255, 1, name)) == 2 and _one_pile(at_255, 1, name, k)[1] == 0
    # a MULTI segment
    (rec,) = _recs_of(at_k, 1, "multi")
    assert rec[6] & 4 and _one_pile(at_k, 1, "multi", k, False)[1] == 1 and _one_pile(at_k, 1, "multi", k, True)[1] == 0
    skipping = host_piles(k, rc, k, True)
    assert skipping["pile"].sum() < at_k["pile"].sum() and skipping["bridged"][0] < at_k["bridged"][0]
    assert np.array_equal(skipping["depth"], at_k["depth"]), "DEPTH counts the MULTI segments whatever the pile leaves out"
    # 70 reads with the same substitution: one word incremented 70 times
    assert at_k["pile"][3300 + n // 2].max() == SAME * (2 if rc else 1) and skipping["pile"][3300 + n // 2].max() == SAME * (2 if rc else 1)
    # a read across a source junction: bridged bases up to the last base of the first source
    (rec,) = _recs_of(at_255, 1, "junction")
    p, b = _one_pile(at_255, 1, "junction", k)
    end0 = int(at_255["soff"][1])
    assert b == 3 and rec[4] < end0 <= rec[5] and p[end0 - 3:end0].sum() == 3 and p[end0:].sum() == 0
    sites, _ = locate.pileup_sites_host(at_255["pile"], at_255["depth"], at_255["soff"], min_count=1, frac_num=0, frac_den=1)
    assert {0} == set(sites["source"][sites["pos"] < end0].tolist()) and sites["source"][sites["pos"] == end0 - 1].tolist() == [0]
    # sequences shorter than k
    assert not _recs_of(at_255, 1, "short") and not _recs_of(at_255, 1, "empty")


def wild_records(h, k, seed):
    """the '+' records of a planted batch with fields that hold anything: sequences that do not exist or are not the record's, extents
    past the sequence's end or empty, heads and tails that no anchor covers, positions at and beyond the ends of the sources, flipped
    strands, random words"""
    segs, ss = h["segs"][0], h["strand_seqs"][0]
    rng = np.random.default_rng(seed)
    wild = segs.copy()
    same = np.flatnonzero(segs["seq"] >= h["names"].index("same0"))
    hit = rng.choice(np.setdiff1d(np.arange(len(wild)), same[:10]), 60, replace=False)
    wild["seq"][hit[:10]] = [0xFFFFFFFF, len(ss)] * 5
    wild["seq"][hit[10:20]] = rng.integers(0, len(ss), 10)
    wild["q_last"][hit[20:25]] += 1          # past the sequence's end for a read mapped up to its last window
    wild["q_first"][hit[25:30]] = wild["q_last"][hit[25:30]] + 1
    wild["pos_first"][hit[35:40]] = [0, 1, h["n_bases"] - 1, h["n_bases"], 0x3FFFFFFF]
    wild["flags"][hit[40:50]] ^= 1
    for f in ("q_first", "q_last", "pos_first", "flags"):
        wild[f][hit[50:]] = rng.integers(0, 1 << 32, 10, dtype=np.uint64).astype(np.uint32)
    n = 3 * k + 20
    wild["q_first"][same[:5]] = n // 2 - 5   # windows that hold the substitution: the record no longer starts with an anchor ...
    wild["q_last"][same[5:10]] = n // 2 - 5  # ... or no longer ends with one: head and tail are bridged
    return wild, same[:10]


def test_records_that_hold_anything_are_skipped_or_stay_in_bounds():
    k = 31
    h = host_piles(k, False, 255, False)
    ss, ms, off = h["strand_seqs"][0], h["ms"][0], h["off"]
    wild, edge = wild_records(h, k, 5)
    for skip_multi in (False, True):
        got, b = locate.pileup_from_segments_host(wild, np.concatenate(ss), ms, off, k, h["n_bases"], skip_multi=skip_multi)
        want, wb = brute_pile(wild, ss, ms, off, k, h["n_bases"], skip_multi)
        assert b == wb and np.array_equal(got, want)
    for x in edge[:5]:   # the bases from q_first to the substitution: 6 where the whole record bridges 1
        assert brute_pile(wild[x:x + 1], ss, ms, off, k, h["n_bases"], False)[1] == 6
    for x in edge[5:]:   # from the substitution, where the last anchor's window ends, to q_last + k
        assert brute_pile(wild[x:x + 1], ss, ms, off, k, h["n_bases"], False)[1] == k - 5
    # and the sequence ends: offsets that descend or end beyond the batch
    bad = off.copy()
    bad[3] = bad[-1] + 7
    got, b = locate.pileup_from_segments_host(h["segs"][0], np.concatenate(ss), ms, bad, k, h["n_bases"], skip_multi=False)
    want, wb = brute_pile(h["segs"][0], ss, ms, bad, k, h["n_bases"], False)
    assert b == wb and np.array_equal(got, want) and 0 < b < h["bridged"][0]


# ---- sites
def test_site_thresholds_at_equality_and_one_below():
    soff = np.array([0, 4, 4, 9], dtype=np.uint64)
    pile = np.zeros((9, 4), dtype=np.uint32)
    depth = np.zeros(9, dtype=np.uint32)
    pile[0, 1], depth[0] = 3, 6   # 3 * 2 == 1 * 6
    pile[1, 2], depth[1] = 3, 7   # 6 < 7
    pile[2, 3], depth[2] = 2, 2   # below min_count
    pile[3, 0], depth[3] = 4, 8   # equality again, the last base of source 0
    pile[4] = [1, 1, 3, 1]        # the first base of source 2 (source 1 is empty)
    depth[4] = 6
    pile[8, 0], depth[8] = 3, 0   # a depth of zero: any count qualifies
    got, n = locate.pileup_sites_host(pile, depth, soff, min_count=3, frac_num=1, frac_den=2)
    assert n == 4 and got["pos"].tolist() == [0, 3, 4, 8] and got["source"].tolist() == [0, 0, 2, 2]
    assert got["depth"].tolist() == [6, 8, 6, 0] and got["count"][2].tolist() == [1, 1, 3, 1] and not got["reserved"].any()
    assert site_tuples(got) == brute_sites(pile, depth, soff, 3, 1, 2)
    # the products are 64-bit
    pile[:], depth[:] = 0, 0
    pile[5, 0], depth[5] = 0x80000000, 0x80000000
    pile[6, 0], depth[6] = 0x80000000, 0x80000001
    pile[7, 1], depth[7] = 0xFFFFFFFF, 0xFFFFFFFF
    got, n = locate.pileup_sites_host(pile, depth, soff, min_count=1, frac_num=0xFFFFFFFF, frac_den=0xFFFFFFFF)
    assert n == 2 and got["pos"].tolist() == [5, 7]
    got, n = locate.pileup_sites_host(pile, depth, soff, min_count=0x80000001, frac_num=0, frac_den=1)
    assert n == 1 and got["pos"].tolist() == [7]


# ---- end to end
def sample_and_reads(srcs, k):
    """a sample with a substitution every 211 bases of every source - from base 2 k + 48, which keeps clear of the world's planted
    repeats, none within 2 k of a source end - and its reads of 150 bases tiled every 7 on both strands; -> (reads, planted set of
    (source, position, ref, alt))"""
    reads, want = [], set()
    for s, src in enumerate(srcs):
        sample = src.copy()
        for p in range(2 * k + 48, len(src) - 2 * k, 211):
            assert src[p] in ACGT
            sample[p] = _other(src[p])
            want.add((s, p, int(src[p]), int(sample[p])))
        for at in range(0, len(sample) - 150 + 1, 7):
            reads.append(sample[at:at + 150].copy())
            reads.append(revcomp(sample[at:at + 150]))
    return reads, want


def snp_set(snps):
    return {(int(r["source"]), int(r["pos"]), int(r["ref"]), int(r["alt"])) for r in snps}


@pytest.mark.parametrize("rc", [False, True])
def test_tiled_reads_give_exactly_the_planted_substitutions(rc):
    """Why exact: a read bridges a substitution that lies at least k bases from both its ends, and a read that does not ends or
    starts its segment next to it and adds nothing to DEPTH there, so at a planted base the alt column IS the depth but for the few
    reads skip_multi leaves out, while every other base is covered by exact windows alone: its pile is zero."""
    k = 31
    srcs, oi, occ, table = world(k, rc, LENS)
    soff = src_offsets(srcs)
    n_bases = int(soff[-1])
    reads, want = sample_and_reads(srcs, k)
    assert len(want) >= 3 * 8 and {s for s, _, _, _ in want} == {0, 1, 2}
    delta = np.zeros(n_bases + 1, dtype=np.uint32)
    pile = np.zeros((n_bases, 4), dtype=np.uint32)
    for strand in (1, 2):
        ss = [revcomp(s) for s in reads] if strand == 2 else reads
        d, lo, off = walk(oi, ss)
        segs, n = locate.segments_from_ms_host(table, k, d, lo, off, k, strand, 3 * len(ss), n_bases, delta)
        assert n == len(segs)
        locate.pileup_from_segments_host(segs, np.concatenate(ss), d, off, k, n_bases, skip_multi=True, pile=pile)
    depth = np.cumsum(delta[:-1], dtype=np.uint32)
    sites, n = locate.pileup_sites_host(pile, depth, soff, min_count=3, frac_num=1, frac_den=2)
    snps = locate.pileup_snps(sites, srcs, min_count=3, frac_num=1, frac_den=2)
    assert snp_set(snps) == want and len(snps) == len(want)
    assert (snps["count"] >= 3).all() and (2 * snps["count"] >= snps["depth"]).all()


def test_pileup_snps_drops_the_source_column():
    srcs = [b"ACGTACGT", b"", b"TTTT"]
    sites = np.zeros(4, dtype=locate.SITE_DTYPE)
    sites["pos"], sites["source"], sites["depth"] = [1, 2, 9, 11], [0, 0, 2, 2], [10, 10, 10, 10]
    sites["count"] = [[0, 9, 0, 0],   # the source base alone: between two nearby substitutions
                      [0, 0, 4, 6],   # G is the source's: T remains
                      [5, 5, 0, 0],   # two columns qualify: no single alt
                      [0, 2, 0, 0]]   # below min_count
    snps = locate.pileup_snps(sites, srcs, min_count=3, frac_num=1, frac_den=2)
    assert [tuple(int(v) for v in r) for r in snps.tolist()] == [(0, 2, ord("G"), ord("T"), 6, 10)]


# ---- errors
def test_argument_errors_come_before_any_device_work_and_in_order():
    L = kbo_amd.lib()
    rust = open(os.path.join(ROOT, "bindings", "rust", "kbo-hip", "src", "lib.rs")).read()
    guide = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW_SYMBOLS:
        assert name in _capi.SYMBOLS and hasattr(L, name) and "pub fn %s(" % name in rust
    for name in ("kbo_pileup_dev", "kbo_pileup_sites_dev", "kbo_pileup_batch"):
        assert "pub fn %s(" % name in guide
    for name in ("pileup", "pileup_dev", "pileup_sites_dev", "pileup_sites_work_bytes", "pileup_from_segments_host", "pileup_sites_host", "pileup_snps"):
        assert hasattr(kbo_amd, name)
    g = b"ACGTTGCATGCATGCAAGTCGATCGATTTGACCATG" * 3
    sbwt, _ = kbo_amd.build([g], kbo_amd.BuildOpts(k=7))
    h = sbwt._h
    P = 0x10000  # a pointer that is never followed: every check below comes first
    n64 = C.c_uint64(0)
    L.kbo_set_index_shards(2)
    try:
        sharded, _ = kbo_amd.build([g, g[::-1]], kbo_amd.BuildOpts(k=7))
    finally:
        L.kbo_set_index_shards(0)
    assert sharded.shards() == 2

    # kbo_pileup_dev: null, misaligned; empty; limits, sharded; no positions
    def pile(idx=h, concat=P, ms=P, off=P, n_seqs=3, total=1000, segs=P, cnt=P, cap=10, out=P):
        return L.kbo_pileup_dev(idx, concat, ms, off, n_seqs, total, segs, cnt, cap, 1, out, None)
    for kw in (dict(idx=None), dict(concat=None), dict(ms=None), dict(off=None), dict(cnt=None), dict(out=None), dict(segs=None)):
        assert pile(**kw) == E_BAD_ARG, kw
    for kw in (dict(segs=P + 2), dict(off=P + 4), dict(cnt=P + 4), dict(out=P + 8)):
        assert pile(n_seqs=0, **kw) == E_BAD_ARG, kw
    assert pile(n_seqs=0, total=1 << 33) == E_EMPTY_QUERY
    assert pile(total=(1 << 32) - 15) == E_UNSUPPORTED and pile(n_seqs=1 << 28) == E_UNSUPPORTED and pile(cap=0xFFFFFFFF) == E_UNSUPPORTED
    assert pile(idx=sharded._h) == E_UNSUPPORTED
    assert pile(segs=None, cap=0) == E_BAD_ARG and "no positions" in L.kbo_last_error().decode()

    # kbo_pileup_sites_dev: null, misaligned, thresholds; sharded; no positions
    assert L.kbo_pileup_sites_work_bytes(h) == 0 and L.kbo_pileup_sites_work_bytes(None) == 0

    def sites(idx=h, pl=P, depth=P, min_count=3, num=1, den=2, out=P, cap=10, cnt=P, work=P, wb=1 << 20):
        return L.kbo_pileup_sites_dev(idx, pl, depth, min_count, num, den, out, cap, cnt, work, wb, None)
    for kw in (dict(idx=None), dict(pl=None), dict(depth=None), dict(cnt=None), dict(work=None), dict(out=None)):
        assert sites(**kw) == E_BAD_ARG, kw
    for kw in (dict(pl=P + 4), dict(depth=P + 2), dict(out=P + 8), dict(cnt=P + 4), dict(work=P + 8), dict(min_count=0), dict(den=0)):
        assert sites(idx=sharded._h, **kw) == E_BAD_ARG, kw
    assert sites(idx=sharded._h) == E_UNSUPPORTED
    assert sites(out=None, cap=0) == E_BAD_ARG and "no positions" in L.kbo_last_error().decode()

    # kbo_pileup_batch: as kbo_segments_batch, the thresholds behind the bridge
    q = np.frombuffer(g, dtype=np.uint8)
    off = np.array([0, len(q)], dtype=np.uint64)
    out = C.c_void_p()

    def batch(idx=h, concat=q.ctypes.data, offsets=off.ctypes.data, n_seqs=1, bridge=7, strands=1, min_count=3, den=2, sites_=C.byref(out), cnt=C.byref(n64)):
        return L.kbo_pileup_batch(idx, concat, offsets, n_seqs, bridge, strands, 1, min_count, 1, den, sites_, cnt, None, None)
    assert batch(strands=0) == E_BAD_ARG and batch(strands=4, idx=None) == E_BAD_ARG
    assert batch(idx=None) == E_BAD_ARG and batch(sites_=None) == E_BAD_ARG and batch(cnt=None) == E_BAD_ARG
    assert batch(bridge=256, idx=sharded._h) == E_BAD_ARG and batch(min_count=0, idx=sharded._h) == E_BAD_ARG and batch(den=0, idx=sharded._h) == E_BAD_ARG
    assert batch(idx=sharded._h) == E_UNSUPPORTED
    assert batch() == E_BAD_ARG and "no positions" in L.kbo_last_error().decode()
    with pytest.raises(kbo_amd.KboError) as e:
        kbo_amd.pileup([g], sbwt)
    assert e.value.code == E_BAD_ARG

    # the host restatements
    rec = np.zeros(2, dtype=locate.SEGMENT_DTYPE)
    cat, ms = np.frombuffer(b"ACGTACGT", dtype=np.uint8), np.zeros(8, dtype=np.uint8)
    o8 = np.array([0, 8], dtype=np.uint64)
    pl = np.zeros((5, 4), dtype=np.uint32)

    def host(segs=rec.ctypes.data, n=2, concat=cat.ctypes.data, ms_=ms.ctypes.data, off_=o8.ctypes.data, n_seqs=1, total=8, k=3, out=pl.ctypes.data, bases=5):
        return L.kbo_pileup_from_segments_host(segs, n, concat, ms_, off_, n_seqs, total, k, 0, out, bases, None)
    assert host() == 0 and pl.sum() == 6, "two records of one window over MS bytes of zero: no anchor, three bases bridged each"
    for kw in (dict(segs=None), dict(concat=None), dict(ms_=None), dict(off_=None), dict(out=None), dict(k=0)):
        assert host(**kw) == E_BAD_ARG, kw
    assert host(segs=None, n=0) == 0
    assert host(n_seqs=0, k=0) == E_BAD_ARG and host(n_seqs=0) == E_EMPTY_QUERY
    assert host(total=(1 << 32) - 15) == E_UNSUPPORTED and host(bases=1 << 30) == E_UNSUPPORTED
    depth = np.zeros(5, dtype=np.uint32)
    so = np.array([0, 5], dtype=np.uint64)
    st = np.zeros(5, dtype=locate.SITE_DTYPE)

    def host_sites(pl_=pl.ctypes.data, depth_=depth.ctypes.data, bases=5, so_=so.ctypes.data, n_src=1, min_count=1, den=1, out=st.ctypes.data, cap=5, cnt=C.byref(n64)):
        return L.kbo_pileup_sites_host(pl_, depth_, bases, so_, n_src, min_count, 0, den, out, cap, cnt)
    assert host_sites() == 0 and n64.value == 3
    for kw in (dict(pl_=None), dict(depth_=None), dict(so_=None), dict(cnt=None), dict(out=None), dict(n_src=0), dict(min_count=0), dict(den=0)):
        assert host_sites(**kw) == E_BAD_ARG, kw
    assert host_sites(out=None, cap=0) == 0 and n64.value == 3
    assert host_sites(bases=1 << 30, min_count=0) == E_BAD_ARG and host_sites(bases=1 << 30) == E_UNSUPPORTED
    bad = np.array([0, 4, 2], dtype=np.uint64)
    assert host_sites(so_=bad.ctypes.data, n_src=2) == E_BAD_ARG


# ---- sanitizers
@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]], ids=["plain", "sanitizers"])
def test_pileup_arithmetic_through_checked_accessors(tmp_path, flags):
    """tools/index_pileup_check.cpp: pileup_serial, the rounds of 64 windows as a wave takes them and sites_serial of index_pileup.hpp
    through accessors that check every index, on randomized and wild records, against brute force of its own"""
    exe = str(tmp_path / "index_pileup_check")
    subprocess.run(["c++", "-std=c++17", "-O1", "-g"] + flags + ["-I", os.path.join(ROOT, "kbo_amd", "csrc"),
                    os.path.join(ROOT, "tools", "index_pileup_check.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "in range" in run.stdout and "agree" in run.stdout
