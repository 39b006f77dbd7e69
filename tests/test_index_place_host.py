"""Placement (kbo_hip.h) on the host: kbo_place_from_segments_host byte for byte against a chain builder written here from the
header's definitions, on hand-made segment lists with every planted case asserted to occur and on the segments of the oracle's walk
of reads and of a 5 000-base sequence; the argument errors and their order; tools/index_place_check.cpp plain and under ASan + UBSan.

The yardstick is py_place(): the recurrence over the definitions in Python integers.  On top of it, for every sequence with at most
12 segments, every ascending subsequence whose consecutive pairs may follow each other is enumerated: with n <= W the recurrence is
exact, so `score` must be the maximum the definition allows.  No GPU.  tests/test_gpu_index_place.py takes the lists and the builder
from here."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

import kbo_amd
from kbo_amd import _capi, locate

from test_index_locate_host import _other, revcomp, src_offsets, walk, world

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_EMPTY_QUERY, E_BAD_ARG, E_UNSUPPORTED = -1, -4, -8
W, LANE_MAX, NONE = 64, 4, 0xFFFFFFFF
K, MAX_GAP, MAX_INDEL = 31, 1000, 100
SRC_OFF = np.array([0, 100000, 100000, 200000, 300000], dtype=np.uint64)  # (source 1 is empty)
NEW_SYMBOLS = ["kbo_place_work_bytes", "kbo_place_dev", "kbo_place_from_segments_host", "kbo_place_batch"]
FIELDS = locate.PLACE_DTYPE.names


# ---- the yardstick: the definitions in Python integers
def _src(src_off, pos):
    return int(np.searchsorted(np.asarray(src_off, dtype=np.uint64), np.uint64(pos), side="right")) - 1


class _S:
    def __init__(self, rec, k, src_off):
        self.seq, self.strand, self.qf, self.ql, self.pf, self.pl, self.flags = (int(v) for v in rec)
        self.len = self.ql - self.qf + k
        self.rev = self.flags & 1
        self.diag = self.pf + self.qf if self.rev else self.pf - self.qf
        self.src = _src(src_off, self.pf)
        self.multi = 1 if self.flags & 12 else 0


def may_precede(a, b, j, i, max_gap, max_indel):
    """(allowed, shift) for s_j = a before s_i = b"""
    if not (i - W <= j < i) or a.rev != b.rev or a.src != b.src:
        return False, 0
    g = b.qf - a.ql
    shift = a.diag - b.diag if b.rev else b.diag - a.diag
    return g <= max_gap and abs(shift) <= max_indel and g + shift >= 1, shift


def gain(a, b):
    return min(b.len, b.ql - a.ql)


def py_chains(recs, k, src_off, max_gap, max_indel):
    """the segments of ONE sequence in list order -> (segments, f, pred, root, n_segs, indel, n_multi)"""
    S = [_S(r, k, src_off) for r in recs]
    n = len(S)
    f, pred, root, ns, ind, nm = [0] * n, [None] * n, [0] * n, [0] * n, [0] * n, [0] * n
    for i in range(n):
        best, best_j, best_shift = None, None, 0
        for j in range(max(0, i - W), i):
            ok, shift = may_precede(S[j], S[i], j, i, max_gap, max_indel)
            if ok and (best is None or f[j] + gain(S[j], S[i]) >= best):  # (ties to the larger j)
                best, best_j, best_shift = f[j] + gain(S[j], S[i]), j, shift
        if best is not None and best > S[i].len:
            f[i], pred[i], root[i], ns[i], ind[i], nm[i] = best, best_j, root[best_j], ns[best_j] + 1, ind[best_j] + abs(best_shift), nm[best_j] + S[i].multi
        else:
            f[i], root[i], ns[i], ind[i], nm[i] = S[i].len, i, 1, 0, S[i].multi
    return S, f, pred, root, ns, ind, nm


def py_record(recs, k, src_off, max_gap, max_indel):
    """the record of ONE sequence as a dict"""
    zero = dict.fromkeys(FIELDS, 0)
    if not len(recs):
        return dict(zero, source=NONE)
    S, f, pred, root, ns, ind, nm = py_chains(recs, k, src_off, max_gap, max_indel)
    e = max(range(len(S)), key=lambda i: (f[i], -i))  # (ties to the smaller i)
    r = root[e]
    rev = S[e].rev
    pos_start, pos_end = (S[e].pl, S[r].pf + k) if rev else (S[r].pf, S[e].pl + k)
    spills = 2 if pos_end > int(src_off[S[r].src + 1]) else 0
    second = max([f[i] for i in range(len(S)) if root[i] != r], default=0)
    return dict(zero, source=S[r].src, strand=S[e].strand, flags=rev | spills, q_start=S[r].qf, q_end=S[e].ql + k, pos_start=pos_start, pos_end=pos_end,
                score=f[e], n_segs=ns[e], indel=ind[e], n_multi=nm[e], second=second)


def py_merge(a, b):
    if b["source"] == NONE or (a["source"] != NONE and (a["score"], -a["strand"]) >= (b["score"], -b["strand"])):
        w, l = a, b
    else:
        w, l = b, a
    return dict(w, second=max(w["second"], l["second"], l["score"]))


def py_place(segs, n_seqs, k, src_off, max_gap=MAX_GAP, max_indel=MAX_INDEL, merge_into=None):
    """records of a batch in (seq, q_first) order -> PLACE_DTYPE[n_seqs]"""
    out = np.zeros(n_seqs, dtype=locate.PLACE_DTYPE)
    by_seq = {}
    for r in segs.tolist():  # (one pass: the records of a sequence in list order, wherever they lie)
        by_seq.setdefault(int(r[0]), []).append(tuple(int(v) for v in r))
    for s in range(n_seqs):
        rec = py_record(by_seq.get(s, []), k, src_off, max_gap, max_indel)
        if merge_into is not None:
            rec = py_merge({n: int(merge_into[s][n]) for n in FIELDS}, rec)
        out[s] = tuple(rec[n] for n in FIELDS)
    return out


def exhaustive_best(recs, k, src_off, max_gap, max_indel):
    """the largest score of any chain the rule allows, by enumeration (n <= 12)"""
    S = [_S(r, k, src_off) for r in recs]
    n = len(S)
    assert n <= 12
    ok = {(j, i): may_precede(S[j], S[i], j, i, max_gap, max_indel)[0] for i in range(n) for j in range(i)}
    best = 0
    for size in range(1, n + 1):
        for sub in itertools.combinations(range(n), size):
            if all(ok[(a, b)] for a, b in zip(sub, sub[1:])):
                best = max(best, S[sub[0]].len + sum(gain(S[a], S[b]) for a, b in zip(sub, sub[1:])))
    return best


# ---- hand-made lists
def seg(qf, ql, pf, rev=0, multi=0, strand=1):
    """a record without its seq: windows qf .. ql on one diagonal from pf"""
    return (strand, qf, ql, pf, pf - (ql - qf) if rev else pf + (ql - qf), rev | multi)


def line(n, base, step=100, span=30, strand=1):
    """n collinear FWD segments, a lone substitution apart: one chain"""
    return [seg(step * i, step * i + span, base + step * i, strand=strand) for i in range(n)]


def far(n, back):
    """n segments: one on a diagonal of source 0 at index n - 1 - back, noise that chains with nothing (a diagonal of its own each, far
    beyond max_indel, in source 3), and a last one on the first's diagonal: a chain of two iff back <= W"""
    at = n - 1 - back
    out = []
    for i in range(n - 1):
        out.append(seg(10 + 2 * i, 10 + 2 * i, 5000 + 10 + 2 * i) if i == at else seg(10 + 2 * i, 10 + 2 * i, 200000 + 700 * i))
    q = 10 + 2 * (n - 1) + 40
    out.append(seg(q, q + 20, 5000 + q))
    return out


def hand_made():
    """name -> the segments of one sequence (without seq); an empty list: a sequence without segments"""
    c = {}
    c["none_first"] = []
    c["one"] = [seg(3, 40, 7000)]
    c["four"] = line(4, 20000)
    c["none_between"] = []
    c["five"] = line(5, 30000)
    for n in (63, 64, 65, 66, 130):
        c["line%d" % n] = line(n, 1000, step=40, span=5)
        for back in (W, W + 1):
            if n - 1 - back >= 0:
                c["far%d_%d" % (n, back)] = far(n, back)
    c["far63_62"], c["far64_63"] = far(63, 62), far(64, 63)
    c["gap_at"] = [seg(0, 30, 40000), seg(30 + MAX_GAP, 60 + MAX_GAP, 40000 + 30 + MAX_GAP)]
    c["gap_over"] = [seg(0, 30, 40000), seg(31 + MAX_GAP, 61 + MAX_GAP, 40000 + 31 + MAX_GAP)]
    for name, sh in (("del_at", MAX_INDEL), ("del_over", MAX_INDEL + 1), ("ins_at", -MAX_INDEL), ("ins_over", -MAX_INDEL - 1)):
        c[name] = [seg(0, 30, 50000), seg(230, 260, 50000 + 230 + sh)]
        c[name + "_rev"] = [seg(0, 30, 60000, rev=1), seg(230, 260, 60000 - 230 - sh, rev=1)]
    c["advance_1"] = [seg(0, 30, 70000), seg(70, 90, 70000 + 70 - 39)]   # g = 40, shift = -39
    c["advance_0"] = [seg(0, 30, 70000), seg(70, 90, 70000 + 70 - 40)]   # g = 40, shift = -40: the source stands still
    c["both_strands"] = [seg(0, 30, 80000), seg(50, 90, 90000, rev=1), seg(100, 140, 80100), seg(150, 170, 89900, rev=1)]
    c["junction"] = [seg(0, 30, 199900), seg(100, 130, 200000)]          # one diagonal, sources 2 and 3
    c["empty_source"] = [seg(0, 30, 100000)]                             # src_off[1] == src_off[2] == 100000: source 2
    c["spills"] = [seg(0, 50, 199990)]                                   # ends at 200071, behind source 2
    c["spills_rev"] = [seg(0, 50, 199990, rev=1)]                        # rev: pos_end = pos_first + k = 200021
    c["rev_down"] = [seg(0, 50, 200020, rev=1)]                          # rev, running down out of source 3: not what SPILLS is defined as
    # two predecessors of equal value: 60 bases to either side of the third's diagonal, too far from each other
    c["tie_pred"] = [seg(0, 10, 110000 - 60), seg(20, 30, 110020 + 60), seg(200, 200, 110200)]
    c["tie_ends"] = [seg(0, 10, 120000), seg(50, 60, 250000)]            # equal f, two sources: the smaller i
    # a branch: 2 and 3 both follow 1 and not each other; the end at 3 shares the root with the best and must not be `second`
    c["runner_inside"] = [seg(0, 30, 130000), seg(100, 130, 130100), seg(200, 260, 130200 + 90), seg(400, 440, 130400 - 90), seg(500, 500, 260000)]
    c["runner_outside"] = [seg(0, 30, 140000), seg(100, 130, 140100), seg(200, 245, 270000)]
    c["multi"] = [seg(0, 30, 150000, multi=4), seg(100, 130, 150100), seg(200, 230, 150200, multi=8), seg(300, 330, 150300, multi=12)]
    c["none_last"] = []
    return c


def as_batch(cases, strand=None):
    """(records SEGMENT_DTYPE in (seq, q_first) order, names)"""
    rows = []
    for s, name in enumerate(cases):
        for r in cases[name]:
            rows.append((s, r[0] if strand is None else strand) + tuple(r[1:]))
    return np.array(rows, dtype=locate.SEGMENT_DTYPE), list(cases)


_HAND = {}


def hand_batch():
    """the hand-made batch and its expected records, made once"""
    if not _HAND:
        segs, names = as_batch(hand_made())
        _HAND["x"] = (segs, names, py_place(segs, len(names), K, SRC_OFF))
    return _HAND["x"]


def same(got, want):
    assert got.tobytes() == want.tobytes(), [(s, got[s], want[s]) for s in np.flatnonzero(got != want)[:3]]


# ---- the tests
def test_hand_made_lists_equal_the_definitions_byte_for_byte():
    segs, names, want = hand_batch()
    got = locate.place_from_segments_host(segs, len(names), SRC_OFF, K, MAX_GAP, MAX_INDEL)
    same(got, want)
    assert not want["reserved"].any() and locate.PLACE_DTYPE.itemsize == 48
    # a sequence count beyond the last record's, and no record at all
    same(locate.place_from_segments_host(segs[:0], 3, SRC_OFF, K), py_place(segs[:0], 3, K, SRC_OFF))
    r = dict(zip(names, want))
    count = {n: len(v) for n, v in hand_made().items()}
    # every planted case occurs
    for n in ("none_first", "none_between", "none_last"):
        assert r[n]["source"] == NONE and not any(int(r[n][f]) for f in FIELDS[1:])
    assert names[0] == "none_first" and names[-1] == "none_last" and 0 < names.index("none_between") < len(names) - 1
    assert count["one"] == 1 and r["one"]["n_segs"] == 1 and r["one"]["score"] == 40 - 3 + K and r["one"]["second"] == 0
    assert (count["four"], count["five"]) == (LANE_MAX, LANE_MAX + 1) and r["four"]["n_segs"] == 4 and r["five"]["n_segs"] == 5
    assert r["five"]["score"] == 61 + 4 * 61 and r["five"]["q_start"] == 0 and r["five"]["q_end"] == 430 + K
    for n in (63, 64, 65, 66, 130):
        assert count["line%d" % n] == n and r["line%d" % n]["n_segs"] == n and r["line%d" % n]["score"] == 36 + 36 * (n - 1)
    for name in ("far63_62", "far64_63", "far65_64", "far66_64", "far130_64"):
        assert r[name]["n_segs"] == 2 and r[name]["source"] == 0, name  # the best predecessor lies at most W back
    for name in ("far66_65", "far130_65"):
        assert r[name]["n_segs"] == 1 and r[name]["source"] == 0 and r[name]["score"] == 20 + K, name  # W + 1 back: not looked at
    assert r["gap_at"]["n_segs"] == 2 and r["gap_over"]["n_segs"] == 1
    for sfx in ("", "_rev"):
        assert r["del_at" + sfx]["n_segs"] == 2 and r["del_at" + sfx]["indel"] == MAX_INDEL and r["del_over" + sfx]["n_segs"] == 1
        assert r["ins_at" + sfx]["n_segs"] == 2 and r["ins_at" + sfx]["indel"] == MAX_INDEL and r["ins_over" + sfx]["n_segs"] == 1
        assert (r["del_at" + sfx]["flags"] & 1) == (1 if sfx else 0)
    assert r["del_at"]["pos_end"] - r["del_at"]["pos_start"] == 260 + K + MAX_INDEL  # a deletion in the sequence: the source runs ahead
    assert r["del_at_rev"]["pos_end"] - r["del_at_rev"]["pos_start"] == 260 + K + MAX_INDEL
    assert r["advance_1"]["n_segs"] == 2 and r["advance_1"]["indel"] == 39 and r["advance_0"]["n_segs"] == 1
    b = r["both_strands"]
    assert b["n_segs"] == 2 and b["flags"] == 0 and b["score"] == 61 + 71 and b["second"] == 71 + 51  # (the REV chain is the runner-up)
    assert r["junction"]["n_segs"] == 1 and r["junction"]["second"] == 30 + K
    ignoring = py_record([(0,) + s for s in hand_made()["junction"]], K, [0, 300000], MAX_GAP, MAX_INDEL)
    assert ignoring["n_segs"] == 2, "with the sources ignored the two would join"
    assert r["empty_source"]["source"] == 2 and r["empty_source"]["pos_start"] == 100000
    assert r["spills"]["flags"] == 2 and r["spills"]["source"] == 2 and r["spills"]["pos_end"] > 200000
    assert r["spills_rev"]["flags"] == 3 and r["spills_rev"]["source"] == 2 and r["spills_rev"]["pos_end"] == 200021
    assert r["rev_down"]["flags"] == 1 and r["rev_down"]["source"] == 3 and r["rev_down"]["pos_start"] < 200000
    assert not (want["flags"][[names.index(n) for n in ("one", "five", "junction")]] & 2).any()
    t = r["tie_pred"]
    assert t["n_segs"] == 2 and t["q_start"] == 20 and t["indel"] == 60, "equal values: the larger j"
    S, f, *_ = py_chains([(0,) + s for s in hand_made()["tie_pred"]], K, SRC_OFF, MAX_GAP, MAX_INDEL)
    assert f[0] + gain(S[0], S[2]) == f[1] + gain(S[1], S[2]) > S[2].len and f[1] == S[1].len
    e = r["tie_ends"]
    assert e["source"] == 2 and e["pos_start"] == 120000 and e["score"] == e["second"] == 10 + K, "equal f: the smaller i, and the other is the runner-up"
    ri = r["runner_inside"]
    S, f, pred, root, *_ = py_chains([(0,) + s for s in hand_made()["runner_inside"]], K, SRC_OFF, MAX_GAP, MAX_INDEL)
    assert root[:4] == [0, 0, 0, 0] and pred[2] == 1 and pred[3] == 1 and f[2] > f[3] > f[4] and root[4] == 4
    assert ri["score"] == f[2] and ri["second"] == f[4] == K, "an end of the best chain's tree is no second placement"
    ro = r["runner_outside"]
    assert ro["n_segs"] == 2 and ro["second"] == 45 + K and ro["source"] == 2
    assert r["multi"]["n_segs"] == 4 and r["multi"]["n_multi"] == 3


def test_score_is_the_maximum_over_every_chain_the_rule_allows():
    segs, names, want = hand_batch()
    rows = [tuple(int(v) for v in r) for r in segs.tolist()]
    tried = 0
    for s, name in enumerate(names):
        mine = [r for r in rows if r[0] == s]
        if 0 < len(mine) <= 12:
            assert int(want[s]["score"]) == exhaustive_best(mine, K, SRC_OFF, MAX_GAP, MAX_INDEL), name
            tried += 1
    assert tried >= 25
    # random lists of 12 segments near one diagonal: many chains to choose from
    rng = np.random.default_rng(5)
    for trial in range(20):
        q, mine = 0, []
        for i in range(12):
            q += int(rng.integers(1, 80))
            span = int(rng.integers(0, 40))
            rev = int(rng.integers(0, 4) == 0)
            jit = int(rng.integers(-70, 71))
            mine.append((0,) + seg(q, q + span, (60000 - q if rev else 50000 + q) + jit, rev=rev))
            q += span
        arr = np.array(mine, dtype=locate.SEGMENT_DTYPE)
        got = locate.place_from_segments_host(arr, 1, SRC_OFF, K, 150, 60)
        same(got, py_place(arr, 1, K, SRC_OFF, 150, 60))
        assert int(got[0]["score"]) == exhaustive_best(mine, K, SRC_OFF, 150, 60), trial


def strand_lists():
    """two calls over four sequences: '-' wins, '+' wins, equal scores (the smaller strand wins), '+' alone, neither"""
    fwd = {"rev_wins": line(2, 1000), "fwd_wins": line(5, 2000), "equal": line(3, 3000), "fwd_only": line(1, 4000), "neither": []}
    rev = {"rev_wins": line(4, 110000, strand=2), "fwd_wins": line(2, 120000, strand=2), "equal": line(3, 130000, strand=2), "fwd_only": [], "neither": []}
    return as_batch(fwd)[0], as_batch(rev)[0], list(fwd)


def test_merge_of_two_strands_in_both_orders_gives_the_same_bytes():
    a, b, names = strand_lists()
    n = len(names)
    pa, pb = py_place(a, n, K, SRC_OFF), py_place(b, n, K, SRC_OFF)
    want = py_place(b, n, K, SRC_OFF, merge_into=pa)
    same(py_place(a, n, K, SRC_OFF, merge_into=pb), want)
    ha = locate.place_from_segments_host(a, n, SRC_OFF, K)
    hb = locate.place_from_segments_host(b, n, SRC_OFF, K)
    same(ha, pa)
    same(hb, pb)
    ab = locate.place_from_segments_host(b, n, SRC_OFF, K, merge_into=ha)
    ba = locate.place_from_segments_host(a, n, SRC_OFF, K, merge_into=hb)
    same(ab, want)
    same(ba, want)
    r = dict(zip(names, want))
    assert r["rev_wins"]["strand"] == 2 and r["rev_wins"]["second"] == pa[0]["score"]
    assert r["fwd_wins"]["strand"] == 1 and r["fwd_wins"]["second"] == pb[1]["score"]
    assert r["equal"]["strand"] == 1 and r["equal"]["second"] == r["equal"]["score"]
    assert r["fwd_only"]["strand"] == 1 and r["fwd_only"]["second"] == 0 and r["neither"]["source"] == NONE
    # the record is its own reduction state: a third call, in any grouping
    c = as_batch({"rev_wins": line(3, 210000, strand=3), "fwd_wins": [], "equal": line(4, 220000, strand=3), "fwd_only": line(1, 230000, strand=3), "neither": []})[0]
    hc = locate.place_from_segments_host(c, n, SRC_OFF, K)
    left = locate.place_from_segments_host(c, n, SRC_OFF, K, merge_into=ab)
    right = locate.place_from_segments_host(a, n, SRC_OFF, K, merge_into=locate.place_from_segments_host(b, n, SRC_OFF, K, merge_into=hc))
    same(left, right)


# ---- through real data
def _edit(seq, at, kind):
    if kind == "sub":
        out = seq.copy()
        out[at] = _other(out[at])
        return out
    if kind == "ins":
        return np.concatenate([seq[:at], np.frombuffer(b"ACG", dtype=np.uint8), seq[at:]])
    return np.concatenate([seq[:at], seq[at + 3:]])


def real_reads(srcs, rng):
    """(sequences, truth): 150-base reads of the first source with nothing, a substitution, two, a 3-base insertion, a 3-base deletion"""
    s0 = srcs[0]
    seqs, truth = [], []
    for r in range(40):
        at = int(rng.integers(1000, len(s0) - 400))
        kind = ("exact", "sub", "sub2", "ins", "del")[r % 5]
        q = s0[at:at + 150].copy()
        if kind == "sub":
            q = _edit(q, 75, "sub")
        elif kind == "sub2":
            q = _edit(_edit(q, 50, "sub"), 100, "sub")
        elif kind in ("ins", "del"):
            q = _edit(s0[at:at + 153].copy(), 75, kind)
        seqs.append(q)
        truth.append((at, kind))
    return seqs, truth


def long_sequence(srcs):
    """5 000 bases of the first source with an edit every 97: substitutions, every fifth a base dropped"""
    q = srcs[0][1000:6000].copy()
    keep = np.ones(len(q), dtype=bool)
    for n, i in enumerate(range(50, 5000, 97)):
        if n % 5 == 4:
            keep[i] = False
        else:
            q[i] = _other(q[i])
    return q[keep]


LONG = (9000, 2500, 64, 4)


def real_segments(k, rc, seqs, bridge, strand=1):
    srcs, oi, occ, table = world(k, rc, LONG)
    d, lo, off = walk(oi, [revcomp(s) for s in seqs] if strand == 2 else seqs)
    n_bases = int(src_offsets(srcs)[-1])
    cap = sum(max(0, len(s) - k + 1) for s in seqs)
    segs, n = locate.segments_from_ms_host(table, k, d, lo, off, bridge, strand, cap, n_bases)
    assert n == len(segs)
    return segs


def test_reads_with_planted_edits_are_placed_where_they_come_from():
    k = 31
    srcs = world(k, False, LONG)[0]
    soff = src_offsets(srcs)
    seqs, truth = real_reads(srcs, np.random.default_rng(3))
    for bridge in (0, k):
        segs = real_segments(k, False, seqs, bridge)
        got = locate.place_from_segments_host(segs, len(seqs), soff, k)
        same(got, py_place(segs, len(seqs), k, soff))
        rows = [tuple(int(v) for v in r) for r in segs.tolist()]
        for s, (at, kind) in enumerate(truth):
            r = got[s]
            mine = [x for x in rows if x[0] == s]
            assert int(r["score"]) == exhaustive_best(mine, k, soff, MAX_GAP, MAX_INDEL)
            assert r["source"] == 0 and r["flags"] == 0 and r["pos_start"] == at and r["q_start"] == 0, (s, kind, r)
            assert r["q_end"] == len(seqs[s]) and r["pos_end"] == at + (153 if kind in ("ins", "del") else 150)
            want_segs = {"exact": 1, "sub": 2 if bridge == 0 else 1, "sub2": 3 if bridge == 0 else 1, "ins": 2, "del": 2}[kind]
            assert r["n_segs"] == want_segs and r["indel"] == (3 if kind in ("ins", "del") else 0), (s, kind, r)
        src, start, end, rev = locate.place_local(got, soff)
        assert src.tolist() == [0] * len(seqs) and start.tolist() == [t[0] for t in truth] and not rev.any()


@pytest.mark.parametrize("k", [31, 96])
def test_a_long_sequence_with_an_edit_every_97_bases_is_one_chain(k):
    srcs = world(k, False, LONG)[0]
    soff = src_offsets(srcs)
    q = long_sequence(srcs)
    segs = real_segments(k, False, [q], 0)
    assert len(segs) > LANE_MAX and (k == 31 or len(segs) >= 40), "a list for the wave route"
    got = locate.place_from_segments_host(segs, 1, soff, k)
    same(got, py_place(segs, 1, k, soff))
    r = got[0]
    assert r["source"] == 0 and r["n_segs"] == len(segs) and r["second"] == 0 and r["indel"] == 10
    assert 1000 <= r["pos_start"] <= 1000 + 97 and 6000 - 97 <= r["pos_end"] <= 6000 and r["q_end"] - r["q_start"] >= len(q) - 2 * 97
    # the reverse complement's walk over an index with both strands: the same stretch, REV
    if k == 31:
        srcs2 = world(k, True, LONG)[0]
        seg2 = real_segments(k, True, [revcomp(q)], 0)
        got2 = locate.place_from_segments_host(seg2, 1, src_offsets(srcs2), k)
        same(got2, py_place(seg2, 1, k, src_offsets(srcs2)))
        assert got2[0]["flags"] == 1 and got2[0]["n_segs"] == len(seg2) and (got2[0]["pos_start"], got2[0]["pos_end"]) == (r["pos_start"], r["pos_end"])


def test_place_local_gives_the_sources_own_coordinates():
    rec = np.zeros(3, dtype=locate.PLACE_DTYPE)
    rec["source"], rec["pos_start"], rec["pos_end"], rec["flags"] = [0, 3, NONE], [5, 200020, 0], [50, 200100, 0], [0, 1, 0]
    src, start, end, rev = locate.place_local(rec, SRC_OFF)
    assert src.tolist() == [0, 3, NONE] and start.tolist() == [5, 20, 0] and end.tolist() == [50, 100, 0] and rev.tolist() == [0, 1, 0]


# ---- errors
def test_argument_errors_come_before_any_device_work_and_in_order():
    L = kbo_amd.lib()
    rust = open(os.path.join(ROOT, "bindings", "rust", "kbo-hip", "src", "lib.rs")).read()
    guide = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW_SYMBOLS:
        assert name in _capi.SYMBOLS and hasattr(L, name) and "pub fn %s(" % name in rust
    for name in ("kbo_place_dev", "kbo_place_batch"):
        assert "pub fn %s(" % name in guide
    g = b"ACGTTGCATGCATGCAAGTCGATCGATTTGACCATG" * 3
    sbwt, _ = kbo_amd.build([g], kbo_amd.BuildOpts(k=7))
    h = sbwt._h
    P = 0x10000  # a pointer that is never followed: every check below comes first
    wb = L.kbo_place_work_bytes(3, 10)
    r16 = lambda v: (v + 15) // 16 * 16  # noqa: E731
    for n_seqs, cap in ((1, 0), (3, 10), (5, 4), (1000, 77), (1 << 20, 1100000)):
        assert L.kbo_place_work_bytes(n_seqs, cap) == 3 * r16(4 * n_seqs) + 16 + r16(4 * cap)
    assert L.kbo_place_work_bytes(0, 10) == 0 and L.kbo_place_work_bytes(1 << 28, 10) == 0 and L.kbo_place_work_bytes(1, (1 << 32) - 1) == 0
    assert L.kbo_place_work_bytes((1 << 28) - 1, (1 << 32) - 2) > 0

    def dev(idx=h, segs=P, cnt=P, cap=10, n_seqs=3, place=P, work=P, wbytes=wb):
        return L.kbo_place_dev(idx, segs, cnt, cap, n_seqs, MAX_GAP, MAX_INDEL, 0, place, work, wbytes, None)
    # null, misaligned; empty; limits, sharded; no positions; (a short d_work comes last: tests/test_gpu_index_place.py)
    for kw in (dict(idx=None), dict(segs=None), dict(cnt=None), dict(place=None), dict(work=None)):
        assert dev(n_seqs=0, **kw) == E_BAD_ARG, kw
    for kw in (dict(segs=P + 2), dict(cnt=P + 4), dict(place=P + 8), dict(work=P + 4)):
        assert dev(n_seqs=0, **kw) == E_BAD_ARG, kw
    assert dev(n_seqs=0, cap=1 << 33) == E_EMPTY_QUERY
    assert dev(n_seqs=1 << 28) == E_UNSUPPORTED and dev(cap=(1 << 32) - 1) == E_UNSUPPORTED
    assert dev(wbytes=0) == E_BAD_ARG and "no positions" in L.kbo_last_error().decode()
    assert dev(segs=None, cap=0) == E_BAD_ARG and "no positions" in L.kbo_last_error().decode()
    L.kbo_set_index_shards(2)
    try:
        sharded, _ = kbo_amd.build([g, g[::-1]], kbo_amd.BuildOpts(k=7))
    finally:
        L.kbo_set_index_shards(0)
    assert sharded.shards() == 2 and dev(idx=sharded._h, wbytes=0) == E_UNSUPPORTED and dev(idx=sharded._h, n_seqs=1 << 28) == E_UNSUPPORTED
    # kbo_place_batch: as kbo_segments_batch
    q = np.frombuffer(g, dtype=np.uint8)
    off = np.array([0, len(q)], dtype=np.uint64)
    out = np.zeros(1, dtype=locate.PLACE_DTYPE)

    def batch(idx=h, concat=q.ctypes.data, offsets=off.ctypes.data, n_seqs=1, bridge=7, strands=1, place=out.ctypes.data):
        return L.kbo_place_batch(idx, concat, offsets, n_seqs, bridge, strands, MAX_GAP, MAX_INDEL, place)
    assert batch(strands=0) == E_BAD_ARG and batch(strands=4, idx=None) == E_BAD_ARG
    assert batch(idx=None) == E_BAD_ARG and batch(place=None) == E_BAD_ARG and batch(bridge=256) == E_BAD_ARG
    assert batch(idx=sharded._h) == E_UNSUPPORTED
    assert batch() == E_BAD_ARG and "no positions" in L.kbo_last_error().decode()
    with pytest.raises(kbo_amd.KboError) as e:
        kbo_amd.place([g], sbwt)
    assert e.value.code == E_BAD_ARG
    # the host restatement
    segs = np.array([(0,) + seg(0, 5, 10)], dtype=locate.SEGMENT_DTYPE)
    so = np.array([0, 100], dtype=np.uint64)
    rec = np.zeros(2, dtype=locate.PLACE_DTYPE)

    def host(segs_=segs.ctypes.data, n=1, n_seqs=2, so_=so.ctypes.data, n_src=1, k=7, place=rec.ctypes.data):
        return L.kbo_place_from_segments_host(segs_, n, n_seqs, so_, n_src, k, MAX_GAP, MAX_INDEL, 0, place)
    assert host() == 0 and rec[0]["score"] == 12 and rec[1]["source"] == NONE
    for kw in (dict(segs_=None), dict(so_=None), dict(place=None), dict(k=0), dict(n_src=0)):
        assert host(n_seqs=0, **kw) == E_BAD_ARG, kw
    assert host(segs_=None, n=0) == 0 and rec[0]["source"] == NONE
    assert host(n_seqs=0) == E_EMPTY_QUERY
    assert host(n_seqs=1 << 28) == E_UNSUPPORTED and host(n=(1 << 32) - 1) == E_UNSUPPORTED
    bad = np.array([0, 100, 50], dtype=np.uint64)
    assert host(so_=bad.ctypes.data, n_src=2) == E_BAD_ARG
    one = np.array([1, 100], dtype=np.uint64)
    assert host(so_=one.ctypes.data) == E_BAD_ARG


def test_lists_that_are_not_in_order_stay_in_bounds_on_the_host():
    """records whose seq is out of range or not its range's are skipped; whatever else they hold, the call returns"""
    segs, names, want = hand_batch()
    rng = np.random.default_rng(9)
    wild = segs.copy()
    hit = rng.choice(len(wild), 60, replace=False)
    wild["seq"][hit[:20]] = 0xFFFFFFFF
    wild["seq"][hit[20:40]] = rng.integers(0, len(names), 20)
    for f in ("q_first", "q_last", "pos_first", "pos_last", "flags"):
        wild[f][hit[40:]] = rng.integers(0, 1 << 32, 20, dtype=np.uint64).astype(np.uint32)
    got = locate.place_from_segments_host(wild, len(names), SRC_OFF, K)
    assert len(got) == len(names) and not got["reserved"].any()
    untouched = [s for s, n in enumerate(names) if not np.isin(np.flatnonzero(segs["seq"] == s), hit).any() and not (wild["seq"][hit[20:40]] == s).any()]
    assert len(untouched) >= 5
    same(got[untouched], want[untouched])


# ---- sanitizers
@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]], ids=["plain", "sanitizers"])
def test_place_arithmetic_through_checked_accessors(tmp_path, flags):
    """tools/index_place_check.cpp: place_serial, the wave's form of a step and the merge of index_place.hpp through accessors that
    check every index, against a chain builder of its own"""
    exe = str(tmp_path / "index_place_check")
    subprocess.run(["c++", "-std=c++17", "-O1", "-g"] + flags + ["-I", os.path.join(ROOT, "kbo_amd", "csrc"),
                    os.path.join(ROOT, "tools", "index_place_check.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "in range" in run.stdout and "agree" in run.stdout
