"""Indels (kbo_hip.h) on the host: kbo_indels_from_segments_host and kbo_indel_sites_host field for field against brute force written
here from the definitions - the intervals of a pair of records, the left-aligned pos, the inserted string by slicing and revcomp, the
sites with a dict counter, all in Python integers - on a world in the style of tests/test_index_locate_host.py with a homopolymer
planted into the first source (k = 5, 31 and 96, indexes with and without add_revcomp, MS bytes through the oracle's walk), strands 1
then 2 into one list, at bridge 0, k and 255, skip_multi on and off, max_indel 1, 16, 17 and 100, with every planted case asserted to
occur at k = 31 and 96; thresholds at equality and one below; capacities below the counts; wild records and events; a tiled sample end
to end through indel_variants; the argument errors and their order; tools/index_indel_check.cpp plain and under ASan + UBSan.
No GPU.  tests/test_gpu_index_indel.py takes the batches and the brute force from here."""
import ctypes as C
import os
import subprocess
from collections import Counter

import numpy as np
import pytest

import kbo_amd
from kbo_amd import _capi, locate
from oracle import binding as ora

from test_index_locate_host import ACGT, _other, as_tuples, brute_segments, expected_table, occurrences, revcomp, sources, src_offsets, walk
from test_index_pileup_host import SAME, planted, wild_records

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_EMPTY_QUERY, E_BAD_ARG, E_UNSUPPORTED = -1, -4, -8
LENS = (4000, 3000, 2000)
KS = [5, 31, 96]
MAX_INDELS = [1, 16, 17, 100]
INS, LONG, LEN_MASK = 1 << 31, 1 << 30, (1 << 30) - 1
HP_AT, HP_LEN = 3500, 9  # the homopolymer planted into the first source
NEW_SYMBOLS = ["kbo_indels_work_bytes", "kbo_indels_dev", "kbo_indel_sites_work_bytes", "kbo_indel_sites_dev", "kbo_indels_from_segments_host",
               "kbo_indel_sites_host", "kbo_indels_batch"]


def _b(s):
    return np.frombuffer(s, dtype=np.uint8)


# ---- brute force from the definitions
def brute_events(recs, seqs, off, k, soff, skip_multi, max_indel, out, capacity):
    """appends the events of the records (tuples or a SEGMENT_DTYPE array) of one call over the batch `seqs` to the list `out` as
    (pos, kind_len, code, flags), counting beyond `capacity` without writing; -> (the list's full count grows by, complex junctions)"""
    recs = recs if isinstance(recs, list) else as_tuples(recs)
    concat = np.concatenate([np.asarray(s, dtype=np.uint8) for s in seqs] + [np.zeros(0, dtype=np.uint8)])
    total, n_src, bases = len(concat), len(soff) - 1, int(soff[-1])
    lim = min(int(max_indel), LEN_MASK)

    def holds(r):
        seq, _, qf, ql, _, _, flags = r
        if seq >= len(seqs) or qf > ql or (skip_multi and flags & 12):
            return False
        o, e = int(off[seq]), int(off[seq + 1])
        return o <= e <= total and ql + k <= e - o

    def S(r):
        return (r[5], r[4] + k) if r[6] & 1 else (r[4], r[5] + k)

    def source_of(x):
        return max(s for s in range(n_src) if int(soff[s]) <= x)

    made = n_complex = 0
    for x in range(1, len(recs)):
        A, B = recs[x - 1], recs[x]
        if not (holds(A) and holds(B)) or A[0] != B[0] or (A[6] ^ B[6]) & 1 or not A[3] < B[2]:
            continue
        rev = A[6] & 1
        lower, upper = (B, A) if rev else (A, B)
        gq = B[2] - (A[3] + k)
        gs = S(upper)[0] - S(lower)[1]
        shift = gs - gq
        if shift == 0 or abs(shift) > lim:
            continue
        if gq > 0 and gs > 0:
            n_complex += 1
            continue
        o, e = int(off[A[0]]), int(off[A[0] + 1])
        seq = concat[o:e]
        if shift > 0:
            assert gq <= 0
            ln, pos, code, kind = shift, S(upper)[0] - shift, 0, 0
            if pos < 0 or pos + ln > bases:
                continue
        else:
            assert gs <= 0
            ln, pos, kind = -shift, S(upper)[0], INS
            if pos > bases:
                continue
            if rev:
                if A[3] + k + ln > len(seq):
                    continue
                ins = revcomp(seq[A[3] + k:A[3] + k + ln])
            else:
                if B[2] - ln < 0:
                    continue
                ins = seq[B[2] - ln:B[2]]
            if not np.isin(ins, ACGT).all():
                continue
            code = sum(b"ACGT".index(int(c)) << (2 * i) for i, c in enumerate(ins)) if ln <= 16 else 0
            kind |= LONG if ln > 16 else 0
        if source_of(S(upper)[0]) != source_of(S(lower)[1] - 1):
            continue
        minus = 1 if bool(rev) != (B[1] == 2) else 0
        if len(out) < capacity:
            out.append((pos, ln | kind, code, minus))
        made += 1
    return made, n_complex


def event_holds(ev, bases):
    pos, kl, code, flags = ev
    ln = kl & LEN_MASK
    if flags > 1 or ln == 0 or pos > bases:
        return False
    if kl & INS:
        return bool(kl & LONG) == (ln > 16) and not (kl & LONG and code) and not (ln < 16 and code >> (2 * ln))
    return not (kl & LONG) and code == 0 and pos + ln <= bases


def brute_sites(events, depth, soff, min_count, num, den):
    """the sites of a list of (pos, kind_len, code, flags) as tuples of the record's eight fields"""
    bases = int(soff[-1])
    count, minus = Counter(), Counter()
    for ev in events:
        if event_holds(ev, bases):
            count[ev[:3]] += 1
            minus[ev[:3]] += ev[3]
    out = []
    for key in sorted(count):
        pos, c = key[0], count[key]
        d = int(depth[pos - 1 if pos else 0]) if bases else 0
        if c >= min_count and c * den >= num * d:
            out.append((pos, max(s for s in range(len(soff) - 1) if int(soff[s]) <= pos), key[1], key[2], c, minus[key], d, 0))
    return out


def event_tuples(ev):
    return [tuple(int(v) for v in r) for r in ev.tolist()]


site_tuples = event_tuples


# ---- the world: the sources of tests/test_index_locate_host.py with a homopolymer of 9 T in the first
_WORLDS = {}


def indel_world(k, rc):
    key = (k, bool(rc))
    if key not in _WORLDS:
        srcs = [s.copy() for s in sources(k, lens=LENS)]
        srcs[0][HP_AT - 1] = ord("C")
        srcs[0][HP_AT:HP_AT + HP_LEN] = ord("T")
        srcs[0][HP_AT + HP_LEN] = ord("G")
        oi = ora.Index.build([s.tobytes() for s in srcs], k=k, add_revcomp=bool(rc))
        occ = occurrences(srcs, k, rc)
        _WORLDS[key] = (srcs, oi, occ, expected_table(oi, occ))
    return _WORLDS[key]


def del_read(src, p, ln, m):
    return np.concatenate([src[p - m:p], src[p + ln:p + ln + m]])


def ins_read(src, p, bases, m):
    return np.concatenate([src[p - m:p], np.asarray(bases, dtype=np.uint8), src[p:p + m]])


def left_del(src, p, ln):
    """the left-aligned (pos, deleted bytes) of the deletion of src[p:p + ln]"""
    while p > 0 and src[p - 1] == src[p + ln - 1]:
        p -= 1
    return p, src[p:p + ln].tobytes()


def left_ins(src, p, bases):
    """the left-aligned (pos, inserted bytes) of `bases` inserted in front of src[p]"""
    bases = bytes(bases)
    while p > 0 and src[p - 1] == bases[-1]:
        bases = bases[-1:] + bases[:-1]
        p -= 1
    return p, bases


INS16 = _b(b"TGCATGGATCCAGTCT")
INS17 = _b(b"TGCATGGATCCAGTCTA")


def planted_indels(srcs, k):
    """the pileup tests' batch and, behind it, the reads this file plants; -> name -> sequence"""
    s0, s1 = srcs[0], srcs[1]
    m = k + 15
    q = dict(planted(srcs, k))
    q["hp_del"] = del_read(s0, HP_AT + 3, 3, m)                      # the same read wherever the three T are taken from
    q["hp_del_rc"] = revcomp(q["hp_del"])
    q["hp_ins"] = ins_read(s0, HP_AT + 4, _b(b"T"), m)
    q["hp_ins_rc"] = revcomp(q["hp_ins"])
    q["ins16"] = ins_read(s0, 2200, INS16, m)
    q["ins17"] = ins_read(s0, 2300, INS17, m)
    q["ins_n"] = ins_read(s0, 2450, _b(b"ACNGT"), m)
    cx = del_read(s0, 2700, 2, m)
    cx[m + 3] = _other(cx[m + 3])                                     # a substitution three bases beside the junction
    q["complex"] = cx
    ln = next(x for x in range(1, 9) if s1[x] != s1[0])              # (no slip: the lower segment ends with the first source)
    q["across"] = np.concatenate([s0[len(s0) - m:], s1[ln:ln + m]])  # a deletion of the second source's first bases
    one = ins_read(s0, 3700, _b(b"GA"), m)
    for r in range(SAME):
        q["same_ins%d" % r] = one
    return q


_LISTS = {}


def host_lists(k, rc, bridge, skip_multi, max_indel):
    """the planted batch through the host form for '+' then '-' into one list and one delta, every field checked against brute
    force on the way: -> dict(names, seqs, segs, ms, lo, strand_seqs [per strand], off, events, n_events, n_complex, depth, srcs, soff)"""
    key = (k, rc, bridge, skip_multi, max_indel)
    if key in _LISTS:
        return _LISTS[key]
    srcs, oi, occ, table = indel_world(k, rc)
    soff = src_offsets(srcs)
    n_bases = int(soff[-1])
    qs = planted_indels(srcs, k)
    names, seqs = list(qs), list(qs.values())
    delta = np.zeros(n_bases + 1, dtype=np.uint32)
    want, events, n_events, n_complex = [], None, 0, 0
    out = dict(names=names, seqs=seqs, segs=[], ms=[], lo=[], strand_seqs=[], srcs=srcs, soff=soff, n_bases=n_bases, table=table, per_strand=[])
    for strand in (1, 2):
        ss = [revcomp(s) for s in seqs] if strand == 2 else seqs
        d, lo, off = walk(oi, ss)
        recs = brute_segments(ss, occ, k, bridge, strand)
        segs, n = locate.segments_from_ms_host(table, k, d, lo, off, bridge, strand, len(recs) + 3, n_bases, delta)
        assert n == len(recs) and as_tuples(segs) == recs
        if events is None:
            events = np.zeros(4 * len(recs), dtype=locate.INDEL_EVENT_DTYPE)
        _, n_events, cx = locate.indels_from_segments_host(segs, np.concatenate(ss), off, k, soff, skip_multi=skip_multi, max_indel=max_indel,
                                                           events=events, n_events=n_events)
        made, want_cx = brute_events(recs, ss, off, k, soff, skip_multi, max_indel, want, len(events))
        assert n_events == len(want) and cx == want_cx, (strand, n_events, len(want), cx, want_cx)
        n_complex += cx
        out["segs"].append(segs)
        out["ms"].append(d)
        out["lo"].append(lo)
        out["strand_seqs"].append(ss)
        out["per_strand"].append(made)
        out["off"] = off
    assert event_tuples(events[:n_events]) == want
    assert not events[n_events:].view(np.uint32).any(), "nothing behind the count is written"
    out.update(events=events[:n_events].copy(), n_events=n_events, n_complex=n_complex, depth=np.cumsum(delta[:-1], dtype=np.uint32))
    _LISTS[key] = out
    return out


def events_of(h, strand, name, k, skip_multi=False, max_indel=100, soff=None):
    """(events, complex junctions) of one sequence's records alone, through the host form"""
    i = h["names"].index(name)
    segs = h["segs"][strand - 1]
    ev, n, cx = locate.indels_from_segments_host(segs[segs["seq"] == i], np.concatenate(h["strand_seqs"][strand - 1]), h["off"], k,
                                                 h["soff"] if soff is None else soff, skip_multi=skip_multi, max_indel=max_indel)
    return event_tuples(ev[:n]), cx


# ---- events and sites against brute force
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("rc", [False, True])
def test_events_and_sites_equal_brute_force_from_the_definitions(k, rc):
    some = 0
    for bridge in (0, k, 255):
        for skip_multi in (False, True):
            for max_indel in MAX_INDELS:
                h = host_lists(k, rc, bridge, skip_multi, max_indel)  # (every field of every event against brute force, strand by strand)
                ev, depth, soff = h["events"], h["depth"], h["soff"]
                some += len(ev)
                for min_count, num, den in ((1, 0, 1), (3, 1, 2), (2, 1, 1), (SAME, 1, 1), (1, 2, 1)):
                    want = brute_sites(event_tuples(ev), depth, soff, min_count, num, den)
                    got, n = locate.indel_sites_host(ev, len(ev), depth, soff, min_count=min_count, frac_num=num, frac_den=den)
                    assert n == len(want) and site_tuples(got) == want, (bridge, skip_multi, max_indel, min_count, num, den)
                    few, n2 = locate.indel_sites_host(ev, len(ev), depth, soff, capacity=len(want) // 2, min_count=min_count, frac_num=num, frac_den=den)
                    assert n2 == n and site_tuples(few) == want[:len(want) // 2]
                    none, n3 = locate.indel_sites_host(ev, len(ev), depth, soff, capacity=0, min_count=min_count, frac_num=num, frac_den=den)
                    assert n3 == n and len(none) == 0
    assert some


@pytest.mark.parametrize("k", [31, 96])
@pytest.mark.parametrize("rc", [False, True])
def test_every_planted_case_occurs(k, rc):
    h = host_lists(k, rc, k, False, 100)
    s0, s1 = h["srcs"][0], h["srcs"][1]
    m = k + 15
    # the pileup tests' insertion and deletion reads: one event each, at the planted place left-aligned against the source
    base_at, half = 3000, (2 * k + 30) // 2
    pos, ins = left_ins(s0, base_at + half, b"A")
    assert events_of(h, 1, "insertion", k) == ([(pos, 1 | INS, b"ACGT".index(ins[0]), 0)], 0)
    pos, _ = left_del(s0, base_at + half, 1)
    assert events_of(h, 1, "deletion", k) == ([(pos, 1, 0, 0)], 0)
    # inside the homopolymer: one key at its left end, whichever way the junction slips - the '+' read's upper segment is its second
    # record, the reverse complement's (REV records on the '+' walk of an index with add_revcomp) its first
    for name, key in (("hp_del", (HP_AT, 3, 0)), ("hp_ins", (HP_AT, 1 | INS, 3))):
        fwd, _ = events_of(h, 1, name, k)
        assert fwd == [key + (0,)], name
        back, _ = events_of(h, 2, name + "_rc", k)  # the '-' read walked as its reverse complement: the '+' read itself, MINUS
        assert back == [key + (1,)]
        flip, _ = events_of(h, 1, name + "_rc", k)
        seg = h["segs"][0][h["segs"][0]["seq"] == h["names"].index(name + "_rc")]
        if rc:
            assert len(seg) == 2 and (seg["flags"] & 1).all() and flip == [key + (1,)], "REV records: the same key, MINUS"
            assert seg["q_last"][0] + k > seg["q_first"][1], "the windows of the two segments overlap inside the homopolymer"
        else:
            assert len(seg) == 0 and flip == []
    # 16 bases use every bit of the code, 17 are LONG, an N gives nothing
    pos, ins = left_ins(s0, 2200, INS16.tobytes())
    code = sum(b"ACGT".index(c) << (2 * i) for i, c in enumerate(ins))
    assert events_of(h, 1, "ins16", k) == ([(pos, 16 | INS, code, 0)], 0) and code >> 30 and code & 3
    pos, _ = left_ins(s0, 2300, INS17.tobytes())
    assert events_of(h, 1, "ins17", k) == ([(pos, 17 | INS | LONG, 0, 0)], 0)
    assert len(h["segs"][0][h["segs"][0]["seq"] == h["names"].index("ins_n")]) == 2 and events_of(h, 1, "ins_n", k) == ([], 0)
    # |shift| == max_indel is taken, one more is not
    assert len(events_of(h, 1, "hp_del", k, max_indel=3)[0]) == 1 and events_of(h, 1, "hp_del", k, max_indel=2) == ([], 0)
    assert len(events_of(h, 1, "ins16", k, max_indel=16)[0]) == 1 and events_of(h, 1, "ins16", k, max_indel=15) == ([], 0)
    # an indel with a substitution three bases beside it: complex, no event; beyond max_indel it is not even that
    assert events_of(h, 1, "complex", k) == ([], 1) and events_of(h, 1, "complex", k, max_indel=1) == ([], 0)
    assert h["n_complex"] >= 1
    # two segments on one diagonal further than the bridge apart
    h0 = host_lists(k, rc, 0, False, 100)
    assert len(h0["segs"][0][h0["segs"][0]["seq"] == h0["names"].index("lone")]) == 2 and events_of(h0, 1, "lone", k) == ([], 0)
    # a pair across a source junction: an event only when the junction is not there
    one_source = np.array([0, 0, 0, h["n_bases"]], dtype=np.uint64)
    assert events_of(h, 1, "across", k) == ([], 0) and len(events_of(h, 1, "across", k, soff=one_source)[0]) == 1
    # a pair of different sequences
    i = h["names"].index("hp_del")
    pair = h["segs"][0][h["segs"][0]["seq"] == i].copy()
    cat = np.concatenate(h["strand_seqs"][0])
    assert locate.indels_from_segments_host(pair, cat, h["off"], k, h["soff"], max_indel=100)[1] == 1
    pair["seq"][1] = i + 1
    assert locate.indels_from_segments_host(pair, cat, h["off"], k, h["soff"], max_indel=100)[1] == 0
    # 70 reads with one insertion: one site of count 70 (found on both walks with add_revcomp)
    pos, ins = left_ins(s0, 3700, b"GA")
    sites, _ = locate.indel_sites_host(h["events"], h["n_events"], h["depth"], h["soff"], min_count=SAME, frac_num=0, frac_den=1)
    assert site_tuples(sites)[-1][:6] == (pos, 0, 2 | INS, b"ACGT".index(ins[0]) | b"ACGT".index(ins[1]) << 2, SAME * (2 if rc else 1), 0)
    assert len(sites) == 1
    assert locate.indel_variants(sites, h["srcs"]) == [(0, pos, b"", ins, SAME * (2 if rc else 1), int(h["depth"][pos - 1]))]


def test_two_calls_append_and_capacities_cut():
    k = 31
    h = host_lists(k, True, k, False, 100)
    want, n = event_tuples(h["events"]), h["n_events"]
    a, b = h["per_strand"]
    assert a > 2 and b > 2 and a + b == n
    for cap in (0, 1, a - 1, a, a + 1, n - 1, n, n + 5):
        ev = np.zeros(cap, dtype=locate.INDEL_EVENT_DTYPE)
        cnt = 0
        for strand in (1, 2):
            _, cnt, _ = locate.indels_from_segments_host(h["segs"][strand - 1], np.concatenate(h["strand_seqs"][strand - 1]), h["off"], k, h["soff"],
                                                         skip_multi=False, max_indel=100, events=ev, n_events=cnt)
        assert cnt == n and event_tuples(ev[:min(cap, n)]) == want[:cap] and not ev[n:].view(np.uint32).any()
        # ... and the sites look at the first min(n, capacity) events
        got, ns = locate.indel_sites_host(ev, cnt, h["depth"], h["soff"], min_count=1, frac_num=0, frac_den=1)
        assert site_tuples(got) == brute_sites(want[:cap], h["depth"], h["soff"], 1, 0, 1) and ns == len(got)


def test_a_shuffled_list_gives_the_same_sites():
    k = 31
    h = host_lists(k, True, k, False, 100)
    ev = h["events"]
    want, n = locate.indel_sites_host(ev, len(ev), h["depth"], h["soff"], min_count=1, frac_num=0, frac_den=1)
    assert n >= 6 and (want["n_minus"] > 0).any() and (want["n_minus"] < want["count"]).any()
    rng = np.random.default_rng(3)
    for _ in range(3):
        got, n2 = locate.indel_sites_host(ev[rng.permutation(len(ev))], len(ev), h["depth"], h["soff"], min_count=1, frac_num=0, frac_den=1)
        assert n2 == n and got.tobytes() == want.tobytes()


# ---- wild records and events
def wild_events(h, seed, n=600):
    """events of random words, and the list's own events with one field each replaced: positions at and beyond the end of the sources,
    lengths of zero and beyond a code's, codes where none belongs, flags beyond the MINUS bit"""
    rng = np.random.default_rng(seed)
    ev = np.zeros(n, dtype=locate.INDEL_EVENT_DTYPE)
    ev.view(np.uint32)[:] = rng.integers(0, 1 << 32, 4 * n, dtype=np.uint64).astype(np.uint32)
    own = h["events"][rng.integers(0, len(h["events"]), n // 2)]
    ev[:n // 2] = own
    for i in range(0, n // 2, 3):
        f = ("pos", "kind_len", "code", "flags")[(i // 3) % 4]
        ev[f][i] = rng.choice([0, 1, 2, 16, 17, h["n_bases"] - 1, h["n_bases"], h["n_bases"] + 1, INS | 1, INS | 16, INS | LONG | 17, INS | LONG | 3, LONG | 2,
                               INS, 0xFFFFFFFF, int(rng.integers(0, 1 << 32))])
    return ev[rng.permutation(n)]


def test_records_and_events_that_hold_anything_are_skipped_or_stay_in_bounds():
    k = 31
    h = host_lists(k, False, 255, False, 100)
    ss, off, soff = h["strand_seqs"][0], h["off"], h["soff"]
    wild, _ = wild_records(h, k, 5)
    for skip_multi in (False, True):
        for max_indel in (16, 0xFFFFFFFF):
            ev, n, cx = locate.indels_from_segments_host(wild, np.concatenate(ss), off, k, soff, skip_multi=skip_multi, max_indel=max_indel)
            want = []
            made, wcx = brute_events(wild, ss, off, k, soff, skip_multi, max_indel, want, len(ev))
            assert n == made and cx == wcx and event_tuples(ev[:n]) == want
    bad = off.copy()
    bad[h["names"].index("insertion") + 1] = bad[-1] + 7  # offsets that descend or end beyond the batch: the insertion and the deletion read
    ev, n, cx = locate.indels_from_segments_host(h["segs"][0], np.concatenate(ss), bad, k, soff, skip_multi=False, max_indel=100)
    want = []
    made, wcx = brute_events(h["segs"][0], ss, bad, k, soff, False, 100, want, len(ev))
    assert n == made and cx == wcx and event_tuples(ev[:n]) == want and 0 < n < h["per_strand"][0]
    we = wild_events(h, 9)
    held = [e for e in event_tuples(we) if event_holds(e, h["n_bases"])]
    assert 100 < len(held) < len(we)
    for min_count in (1, 2):
        got, n = locate.indel_sites_host(we, len(we), h["depth"], soff, min_count=min_count, frac_num=0, frac_den=1)
        assert site_tuples(got) == brute_sites(event_tuples(we), h["depth"], soff, min_count, 0, 1) and n == len(got) and n > 0


# ---- sites
def _events(rows):
    ev = np.zeros(len(rows), dtype=locate.INDEL_EVENT_DTYPE)
    for i, r in enumerate(rows):
        ev[i] = r
    return ev


def test_site_thresholds_at_equality_and_one_below():
    soff = np.array([0, 4, 4, 9], dtype=np.uint64)
    depth = np.array([6, 7, 2, 8, 6, 1, 1, 1, 0], dtype=np.uint32)
    rows = [(1, 2, 0, 0)] * 3          # depth[0] = 6: 3 * 2 == 1 * 6
    rows += [(2, 1 | INS, 2, 1)] * 3   # depth[1] = 7: 6 < 7
    rows += [(3, 1, 0, 0)] * 2         # below min_count
    rows += [(4, 1 | INS, 1, 0)] * 2 + [(4, 1 | INS, 1, 1)] * 2  # depth[3] = 8: equality; the first base of source 2 (source 1 is empty)
    rows += [(0, 1, 0, 1)] * 3         # pos 0 reads DEPTH[0]
    rows += [(9, 1 | INS, 0, 0)] * 3   # an insertion behind the last base: depth[8] = 0, any count qualifies
    rows += [(9, 1, 0, 0)] * 3         # a deletion there would leave the sources: skipped
    ev = _events(rows)
    got, n = locate.indel_sites_host(ev, len(ev), depth, soff, min_count=3, frac_num=1, frac_den=2)
    assert site_tuples(got) == [(0, 0, 1, 0, 3, 3, 6, 0), (1, 0, 2, 0, 3, 0, 6, 0), (4, 2, 1 | INS, 1, 4, 2, 8, 0), (9, 2, 1 | INS, 0, 3, 0, 0, 0)] and n == 4
    assert site_tuples(got) == brute_sites(event_tuples(ev), depth, soff, 3, 1, 2)
    # the products are 64-bit
    depth[:] = 0
    depth[0], depth[1] = 0xFFFFFFFF, 2
    ev = _events([(1, 1, 0, 0)] * 2 + [(2, 1, 0, 0)])
    got, n = locate.indel_sites_host(ev, 3, depth, soff, min_count=1, frac_num=1, frac_den=0x80000000)
    assert [s[0] for s in site_tuples(got)] == [1, 2], "2 * 2^31 >= 2^32 - 1, which 32 bits would not see"
    got, n = locate.indel_sites_host(ev, 3, depth, soff, min_count=1, frac_num=0x80000000, frac_den=1)
    assert n == 0, "1 < 2^31 * 2, which 32 bits would not see"
    # equal positions: deletions before insertions, shorter before longer, then the code
    ev = _events([(5, 2 | INS, 7, 0), (5, 2 | INS, 4, 0), (5, 3, 0, 0), (5, 1 | INS, 3, 0), (5, 1, 0, 0), (5, 17 | INS | LONG, 0, 0)])
    got, n = locate.indel_sites_host(ev, 6, depth, soff, min_count=1, frac_num=0, frac_den=1)
    assert [(s[2], s[3]) for s in site_tuples(got)] == [(1, 0), (3, 0), (1 | INS, 3), (2 | INS, 4), (2 | INS, 7), (17 | INS | LONG, 0)]
    assert [v[2:4] for v in locate.indel_variants(got, [b"ACGT", b"", b"ACGTA"])] == [(b"C", b""), (b"CGT", b""), (b"", b"T"), (b"", b"AC"), (b"", b"TC"),
                                                                                      (b"", b"")]


# ---- end to end
def sample_and_reads(srcs, k):
    """a sample with alternating deletions and insertions of 1 - 5 bases every 211 bases of every source - from base 2 k + 48, none
    within 2 k of a source end - and its reads of 150 bases tiled every 7 on both strands; -> (reads, the planted set of (source,
    position, ref, alt), left-aligned against the source)"""
    rng = np.random.default_rng(17)
    reads, want = [], set()
    for s, src in enumerate(srcs):
        parts, at = [], 0
        for i, p in enumerate(range(2 * k + 48, len(src) - 2 * k, 211)):
            ln = 1 + i % 5
            parts.append(src[at:p])
            if i % 2 == 0:
                pos, ref = left_del(src, p, ln)
                want.add((s, pos, ref, b""))
                at = p + ln
            else:
                ins = ACGT[rng.integers(0, 4, ln)]
                pos, alt = left_ins(src, p, ins.tobytes())
                want.add((s, pos, b"", alt))
                parts.append(ins)
                at = p
        parts.append(src[at:])
        sample = np.concatenate(parts)
        for a in range(0, len(sample) - 150 + 1, 7):
            reads.append(sample[a:a + 150].copy())
            reads.append(revcomp(sample[a:a + 150]))
    return reads, want


def variant_set(v):
    return {r[:4] for r in v}


@pytest.mark.parametrize("rc", [False, True])
def test_tiled_reads_give_exactly_the_planted_indels(rc):
    """Why exact: a read whose indel lies at least k bases from both its ends gives two segments and one clean event, any other read
    one segment and none - about 88 of the 119 reads that cover the base in front carry the event, the others cover it without one."""
    k = 31
    srcs, oi, occ, table = indel_world(k, rc)
    soff = src_offsets(srcs)
    n_bases = int(soff[-1])
    reads, want = sample_and_reads(srcs, k)
    assert len(want) >= 3 * 8 and {s for s, _, _, _ in want} == {0, 1, 2}
    assert {len(r) for _, _, r, a in want if not a} == {1, 2, 3, 4, 5} == {len(a) for _, _, r, a in want if not r}
    delta = np.zeros(n_bases + 1, dtype=np.uint32)
    events, n_events, complex_ = np.zeros(2 * len(reads), dtype=locate.INDEL_EVENT_DTYPE), 0, 0
    for strand in (1, 2):
        ss = [revcomp(s) for s in reads] if strand == 2 else reads
        d, lo, off = walk(oi, ss)
        segs, n = locate.segments_from_ms_host(table, k, d, lo, off, k, strand, 3 * len(ss), n_bases, delta)
        assert n == len(segs)
        _, n_events, cx = locate.indels_from_segments_host(segs, np.concatenate(ss), off, k, soff, skip_multi=True, max_indel=16, events=events,
                                                           n_events=n_events)
        complex_ += cx
    assert complex_ == 0, "the spacing leaves no junction with a mismatch next to it"
    depth = np.cumsum(delta[:-1], dtype=np.uint32)
    sites, n = locate.indel_sites_host(events, n_events, depth, soff, min_count=3, frac_num=1, frac_den=2)
    got = locate.indel_variants(sites, srcs)
    assert variant_set(got) == want and len(got) == len(want)
    assert all(c >= 3 and 2 * c >= d for _, _, _, _, c, d in got)
    assert (sites["n_minus"] * 2 == sites["count"]).all(), "every read is there on both strands"


# ---- errors
def test_argument_errors_come_before_any_device_work_and_in_order():
    L = kbo_amd.lib()
    rust = open(os.path.join(ROOT, "bindings", "rust", "kbo-hip", "src", "lib.rs")).read()
    guide = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW_SYMBOLS:
        assert name in _capi.SYMBOLS and hasattr(L, name) and "pub fn %s(" % name in rust
    for name in ("kbo_indels_dev", "kbo_indel_sites_dev", "kbo_indels_batch"):
        assert "pub fn %s(" % name in guide
    for name in ("INDEL_EVENT_DTYPE", "INDEL_SITE_DTYPE", "indels", "indels_dev", "indels_work_bytes", "indel_sites_dev", "indel_sites_work_bytes",
                 "indels_from_segments_host", "indel_sites_host", "indel_variants"):
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

    # the work sizes are exact figures of the capacity alone
    r16 = lambda v: (v + 15) // 16 * 16  # noqa: E731
    for cap in (0, 1, 2047, 2048, 2049, 4096, 4097, 1 << 20):
        assert L.kbo_indels_work_bytes(cap) == r16((cap + 2047) // 2048 * 4) + 16
        tiles = (cap + 4095) // 4096
        assert L.kbo_indel_sites_work_bytes(cap) == 2 * r16(16 * cap) + r16(1024 * tiles) + r16((256 * tiles // 1024 + 2) * 4) + r16(8 * (cap + 1)) + \
            r16((cap + 1 + 2047) // 2048 * 8) + r16((cap + 2047) // 2048 * 4) + 16
    assert L.kbo_indels_work_bytes(0xFFFFFFFF) == 0 and L.kbo_indel_sites_work_bytes(0xFFFFFFFF) == 0

    # kbo_indels_dev: null, misaligned, max_indel; empty; limits, sharded; no positions
    def events(idx=h, concat=P, off=P, n_seqs=3, total=1000, segs=P, cnt=P, cap=10, max_indel=16, out=P, ecap=10, ecnt=P, work=P, wb=1 << 20):
        return L.kbo_indels_dev(idx, concat, off, n_seqs, total, segs, cnt, cap, 1, max_indel, out, ecap, ecnt, work, wb, None)
    for kw in (dict(idx=None), dict(concat=None), dict(off=None), dict(cnt=None), dict(ecnt=None), dict(work=None), dict(segs=None), dict(out=None)):
        assert events(**kw) == E_BAD_ARG, kw
    for kw in (dict(segs=P + 2), dict(off=P + 4), dict(cnt=P + 4), dict(ecnt=P + 4), dict(out=P + 8), dict(work=P + 8), dict(max_indel=0)):
        assert events(n_seqs=0, **kw) == E_BAD_ARG, kw
    assert events(n_seqs=0, total=1 << 33) == E_EMPTY_QUERY
    assert events(total=(1 << 32) - 15) == E_UNSUPPORTED and events(n_seqs=1 << 28) == E_UNSUPPORTED and events(cap=0xFFFFFFFF) == E_UNSUPPORTED
    assert events(ecap=0xFFFFFFFF) == E_UNSUPPORTED and events(idx=sharded._h) == E_UNSUPPORTED
    assert events(segs=None, cap=0, out=None, ecap=0, wb=0) == E_BAD_ARG and "no positions" in L.kbo_last_error().decode()

    # kbo_indel_sites_dev: null, misaligned, thresholds; limits, sharded; no positions
    def sites(idx=h, ev=P, ecnt=P, ecap=10, depth=P, min_count=3, num=1, den=2, out=P, cap=10, cnt=P, work=P, wb=1 << 20):
        return L.kbo_indel_sites_dev(idx, ev, ecnt, ecap, depth, min_count, num, den, out, cap, cnt, work, wb, None)
    for kw in (dict(idx=None), dict(ev=None), dict(ecnt=None), dict(depth=None), dict(cnt=None), dict(work=None), dict(out=None)):
        assert sites(**kw) == E_BAD_ARG, kw
    for kw in (dict(ev=P + 8), dict(ecnt=P + 4), dict(depth=P + 2), dict(out=P + 8), dict(cnt=P + 4), dict(work=P + 8), dict(min_count=0), dict(den=0)):
        assert sites(idx=sharded._h, ecap=0xFFFFFFFF, **kw) == E_BAD_ARG, kw
    assert sites(idx=sharded._h) == E_UNSUPPORTED and sites(ecap=0xFFFFFFFF) == E_UNSUPPORTED
    assert sites(ev=None, ecap=0, out=None, cap=0, wb=0) == E_BAD_ARG and "no positions" in L.kbo_last_error().decode()

    # kbo_indels_batch: as kbo_pileup_batch, max_indel beside the thresholds
    q = np.frombuffer(g, dtype=np.uint8)
    off = np.array([0, len(q)], dtype=np.uint64)
    out = C.c_void_p()

    def batch(idx=h, concat=q.ctypes.data, offsets=off.ctypes.data, n_seqs=1, bridge=7, strands=1, max_indel=16, min_count=3, den=2, sites_=C.byref(out),
              cnt=C.byref(n64)):
        return L.kbo_indels_batch(idx, concat, offsets, n_seqs, bridge, strands, 1, max_indel, min_count, 1, den, sites_, cnt, None)
    assert batch(strands=0) == E_BAD_ARG and batch(strands=4, idx=None) == E_BAD_ARG
    assert batch(idx=None) == E_BAD_ARG and batch(sites_=None) == E_BAD_ARG and batch(cnt=None) == E_BAD_ARG
    for kw in (dict(bridge=256), dict(max_indel=0), dict(min_count=0), dict(den=0)):
        assert batch(idx=sharded._h, **kw) == E_BAD_ARG, kw
    assert batch(idx=sharded._h) == E_UNSUPPORTED
    assert batch() == E_BAD_ARG and "no positions" in L.kbo_last_error().decode()
    with pytest.raises(kbo_amd.KboError) as e:
        kbo_amd.indels([g], sbwt)
    assert e.value.code == E_BAD_ARG

    # the host restatements
    rec = np.zeros(2, dtype=locate.SEGMENT_DTYPE)
    rec[0] = (0, 1, 0, 1, 0, 1, 0)  # windows 0 .. 1 at 0 .. 1, then window 4 at 6: two source bases more than query bases
    rec[1] = (0, 1, 4, 4, 6, 6, 0)
    cat = np.frombuffer(b"ACGTACGT", dtype=np.uint8)
    o8 = np.array([0, 8], dtype=np.uint64)
    so = np.array([0, 12], dtype=np.uint64)
    ev = np.zeros(4, dtype=locate.INDEL_EVENT_DTYPE)

    def host(segs=rec.ctypes.data, n=2, concat=cat.ctypes.data, off_=o8.ctypes.data, n_seqs=1, total=8, k=3, max_indel=16, so_=so.ctypes.data, n_src=1,
             out=ev.ctypes.data, cap=4, cnt=C.byref(n64), cx=None):
        return L.kbo_indels_from_segments_host(segs, n, concat, off_, n_seqs, total, k, 0, max_indel, so_, n_src, out, cap, cnt, cx)
    n64.value = 1
    assert host() == 0 and n64.value == 2 and event_tuples(ev) == [(0, 0, 0, 0), (4, 2, 0, 0), (0, 0, 0, 0), (0, 0, 0, 0)], "appended behind the one there"
    n64.value = 0
    for kw in (dict(segs=None), dict(concat=None), dict(off_=None), dict(so_=None), dict(out=None), dict(cnt=None), dict(k=0), dict(n_src=0), dict(max_indel=0)):
        assert host(**kw) == E_BAD_ARG, kw
    assert host(segs=None, n=0) == 0 and n64.value == 0 and host(out=None, cap=0) == 0 and n64.value == 1
    assert host(n_seqs=0, max_indel=0) == E_BAD_ARG and host(n_seqs=0) == E_EMPTY_QUERY
    assert host(total=(1 << 32) - 15) == E_UNSUPPORTED and host(cap=0xFFFFFFFF) == E_UNSUPPORTED
    big, bad = np.array([0, 1 << 30], dtype=np.uint64), np.array([0, 4, 2], dtype=np.uint64)
    assert host(so_=big.ctypes.data) == E_UNSUPPORTED and host(so_=bad.ctypes.data, n_src=2) == E_BAD_ARG
    depth = np.zeros(12, dtype=np.uint32)
    st = np.zeros(4, dtype=locate.INDEL_SITE_DTYPE)

    def host_sites(ev_=ev.ctypes.data, n=2, ecap=4, depth_=depth.ctypes.data, so_=so.ctypes.data, n_src=1, min_count=1, den=1, out=st.ctypes.data, cap=4,
                   cnt=C.byref(n64)):
        return L.kbo_indel_sites_host(ev_, n, ecap, depth_, so_, n_src, min_count, 0, den, out, cap, cnt)
    assert host_sites() == 0 and n64.value == 1 and site_tuples(st)[0] == (4, 0, 2, 0, 1, 0, 0, 0), "the zero words in front hold no event"
    for kw in (dict(ev_=None), dict(depth_=None), dict(so_=None), dict(cnt=None), dict(out=None), dict(n_src=0), dict(min_count=0), dict(den=0)):
        assert host_sites(**kw) == E_BAD_ARG, kw
    assert host_sites(out=None, cap=0) == 0 and n64.value == 1 and host_sites(ev_=None, ecap=0) == 0 and n64.value == 0
    assert host_sites(ecap=0xFFFFFFFF, min_count=0) == E_BAD_ARG and host_sites(ecap=0xFFFFFFFF) == E_UNSUPPORTED
    assert host_sites(so_=big.ctypes.data) == E_UNSUPPORTED and host_sites(so_=bad.ctypes.data, n_src=2) == E_BAD_ARG


# ---- sanitizers
@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]], ids=["plain", "sanitizers"])
def test_indel_arithmetic_through_checked_accessors(tmp_path, flags):
    """tools/index_indel_check.cpp: the pair rule, the code packing both ways, the key order and the grouping from a shuffled list of
    index_indel.hpp through accessors that check every index, on randomized and wild records and events, against brute force of its own"""
    exe = str(tmp_path / "index_indel_check")
    subprocess.run(["c++", "-std=c++17", "-O1", "-g"] + flags + ["-I", os.path.join(ROOT, "kbo_amd", "csrc"),
                    os.path.join(ROOT, "tools", "index_indel_check.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "in range" in run.stdout and "agree" in run.stdout
