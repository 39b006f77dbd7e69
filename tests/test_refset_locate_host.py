"""The locus of a run (kbo_hip.h "The LOCUS of a run") on the host: kbo_refset_opts.positions, the position table, and
kbo_locate_refset_host - the CPU restatement of refset_locate_kernel over kbo_amd/csrc/refset_locate.hpp - and the argument errors.

The yardstick is brute force written here, independent of the library's walk: a dict from every k-mer of every indexed stretch of a
reference (and of the stretches' reverse complements when add_revcomp is set) to its occurrence list.  From the dict come the expected
table entry - FWD before REV, then the smallest p, MULTI for more than one occurrence - and, by scanning [start, end - k], the expected
first and last anchors of a run.  All comparisons are exact and cover every record.  The runs come from kbo_refset_ms_host plus the
oracle's derandomize, translate and run lengths, or are made by hand.  tools/refset_locate_check.cpp runs the look-up through
accessors that check every index, as a stand-alone program under AddressSanitizer and UBSan.  No GPU.
tests/test_gpu_refset_locate.py takes world() and the brute force from here."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import kbo_amd
from kbo_amd import _capi, refset
from oracle import binding as ora

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_EMPTY_QUERY, E_LEN_LE_2, E_BAD_ARG, E_UNSUPPORTED = -1, -2, -4, -8
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
COMP = np.arange(256, dtype=np.uint8)  # (lower case stays what it is: no base on either strand)
for _a, _b in zip(b"ACGT", b"TGCA"):
    COMP[_a] = _b
NONE, MULTI, REV = 0xFFFFFFFF, 1 << 31, 1 << 30
WINDOW = 64
WITH_N, WITH_GAP, REPEAT, RC_TWIN, WIDE, SHORT = 2, 3, 4, 5, 12, 13
WIDE_ROWS = 1 << 17
GAP = 5  # max_gap_len of the runs
NEW_SYMBOLS = ["kbo_refset_has_positions", "kbo_refset_positions_bytes", "kbo_refset_positions", "kbo_refset_ref_len", "kbo_locate_refset",
               "kbo_locate_refset_dev", "kbo_locate_refset_host"]


def _rnd(rng, n):
    return ACGT[rng.integers(0, 4, n)].copy()


def _other(base):
    return ACGT[(int(np.searchsorted(ACGT, base)) + 1) % 4]


def _not(*bases):
    """one base that is none of `bases`"""
    return [b for b in ACGT if b not in bases][:1]


def _sub(a, at):
    """a copy of `a` with substitutions at the offsets `at`"""
    a = a.copy()
    for i in at:
        a[i] = _other(a[i])
    return a


def revcomp(a):
    return COMP[a[::-1]]


def threshold(k, n_kmers, prob=1e-7):
    t = C.c_size_t()
    kbo_amd.check(kbo_amd.lib().kbo_random_match_threshold(k, n_kmers, 4, prob, C.byref(t)))
    return t.value


# ---- brute force
def stretches(ref, k):
    """the indexed stretches: maximal runs of A, C, G, T of at least k bases, as (begin, end)"""
    ok = np.isin(ref, ACGT)
    out, i, n = [], 0, len(ref)
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


def occurrences(ref, k, rc):
    """k-mer (bytes) -> [(0 for FWD / 1 for REV, p)], every occurrence"""
    d = {}
    for a, b in stretches(ref, k):
        for p in range(a, b - k + 1):
            w = ref[p:p + k]
            d.setdefault(w.tobytes(), []).append((0, p))
            if rc:
                d.setdefault(revcomp(w).tobytes(), []).append((1, p))
    return d


def entry_of(occ):
    strand, p = min(occ)
    return p | (REV if strand else 0) | (MULTI if len(occ) > 1 else 0)


def strand_seq(q, strand):
    return q if strand == 1 else revcomp(q)


def expected_locus(d, k, q, strand, start, end):
    """(q_first, ref_first, q_last, ref_last, flags) of the run [start, end) of q on `strand` against the reference of dict d"""
    s = strand_seq(q, strand)
    hits = [i for i in range(start, end - k + 1) if s[i:i + k].tobytes() in d]
    if not hits:
        return (NONE, NONE, NONE, NONE, 0)
    e0, e1 = entry_of(d[s[hits[0]:hits[0] + k].tobytes()]), entry_of(d[s[hits[-1]:hits[-1] + k].tobytes()])
    flags = (1 if e0 & REV else 0) | (2 if e1 & REV else 0) | (4 if e0 & MULTI else 0) | (8 if e1 & MULTI else 0)
    return (hits[0], e0 & (REV - 1), hits[-1], e1 & (REV - 1), flags)


def expected_tested(k, start, end, locus):
    """n_tested by the contract: windows handed out 64 at a time from the front until a group holds the first anchor, then from the back"""
    starts = end - start - k + 1
    if starts <= 0:
        return 0
    if locus[0] == NONE:
        return starts
    def upto(at):  # windows handed out when the hit is window number `at` of its direction
        return min(starts, (at // WINDOW + 1) * WINDOW)
    return upto(locus[0] - start) + upto(end - k - locus[2])


# ---- the set and the batch of the GPU test, and smaller things for this file
def make_refs(k, seed):
    rng = np.random.default_rng(seed)
    refs = [_rnd(rng, n) for n in (300, 400, 520, 640, 777, 900, 1000, 1100, 1300, 1500, 1800, 2000)]
    refs[WITH_N][260] = ord("N")
    refs[WITH_GAP][300] = refs[WITH_GAP][300 + k] = ord("N")      # a stretch of k - 1 bases: not indexed
    rep = k + 60
    refs[REPEAT][500:500 + rep] = refs[REPEAT][100:100 + rep]       # an exact repeat: MULTI
    refs[RC_TWIN][600:600 + rep] = revcomp(refs[RC_TWIN][100:100 + rep])  # the only other occurrence is on the other strand
    refs.append(_rnd(rng, 20000))                                   # wide
    refs.append(_rnd(rng, k - 1))                                   # no k-mer: a status
    return refs


FIRST_OFFSETS = (0, 63, 64, 65, 130)  # where the first k-mer hit lies behind run.start: the lane and window boundaries
BLOCK = 19  # matching bases that are a hit of their own: above every threshold of these references at 1e-7 (15 .. 18, kbo_hip.h)


def _lead_subs(d, k):
    """substitutions in a copy so that its first k-mer hit starts d bases in AND the run starts at its first base: the last one at
    d - 1, the others s apart with blocks of at least BLOCK matching bases between them and in front of the first - every block a hit
    of its own and shorter than k"""
    if d == 0:
        return []
    for t in range(0, d):
        for s in range(BLOCK + 1, k):
            p0 = d - 1 - t * s
            if BLOCK <= p0 <= k - 1:
                return [p0 + j * s for j in range(t + 1)]
    raise AssertionError("no such pattern for d = %d" % d)


def _lead(ref, at, d, k, tail=30):
    """a copy of d + k + tail bases of ref whose first k-mer that is one of the reference's starts d bases into the copy"""
    return _sub(ref[at:at + d + k + tail], _lead_subs(d, k))


def make_seqs(k, refs, seed):
    rng = np.random.default_rng(seed)
    gap = lambda n=40: _rnd(rng, n)
    first, last = [gap()], [gap()]
    plants = [(j, d) for j, d in enumerate(FIRST_OFFSETS * 3)]  # (each offset from three references: a chance match next to one shifts it)
    for j, d in plants:
        src = refs[6 + j % 6]
        at = 20 + 37 * (j // 6)
        first += [_lead(src, at, d, k), gap()]
    # the same offsets measured back from the end: the mirror image of _lead
    for j, d in plants:
        src = refs[6 + j % 6]
        at = 420 + 37 * (j // 6)
        n = d + k + 30
        piece = src[at:at + n]
        last += [_sub(piece, [n - 1 - i for i in _lead_subs(d, k)]), gap()]
    rep = k + 60
    short = 25 if k <= 40 else 40
    exact = refs[9][700:700 + k].copy()
    strands = [gap(), revcomp(refs[8][200:500]), gap(), refs[9][100:400], gap(),
               np.concatenate([[_other(refs[9][699])], exact, [_other(refs[9][700 + k])]]).astype(np.uint8), gap(),
               refs[10][900:900 + short], gap(),
               # (the repeat alone, between bases that continue neither copy: both anchors are MULTI)
               _not(refs[REPEAT][99], refs[REPEAT][499]), refs[REPEAT][100:100 + rep], _not(refs[REPEAT][100 + rep], refs[REPEAT][500 + rep]), gap(),
               _not(refs[RC_TWIN][99], COMP[refs[RC_TWIN][600 + rep]]), refs[RC_TWIN][100:100 + rep],
               _not(refs[RC_TWIN][100 + rep], COMP[refs[RC_TWIN][599]]), gap(),
               _sub(refs[WIDE][5000:5600], range(50, 600, 97)), gap(), revcomp(refs[WIDE][9000:9400]), gap()]
    every20 = _sub(refs[10][100:700], range(7, 600, 20))
    half = _sub(refs[11][100:500], range(7, 250, 20))
    back = _sub(refs[11][700:1100], range(157, 400, 20))
    dense = [gap(), every20, gap(), half, gap(), back, gap()]
    with_n = refs[1][50:350].copy()
    with_n[100] = ord("N")
    with_n[200] |= 0x20
    # (a mismatch on a contig's first base, the copy from its second: translate.rs gives position 0 an 'X', the one way a run of
    # find starts ONE base in front of its first k-mer hit; behind a run's last hit a lone 'X' cannot stand - it needs an 'M' after it)
    gaps = [[_other(refs[8][599])], refs[8][600:760], gap(), refs[7][100:250], _rnd(rng, 4), refs[7][250:400], gap(), refs[6][100:250], refs[6][254:400], gap(), with_n, gap(),
            refs[7][500:640], _rnd(rng, 3), refs[7][643:800], gap()]
    tail = [_rnd(rng, 1000), refs[WITH_GAP][350:640]]  # ends at the last base of the last contig
    return [np.concatenate(x).astype(np.uint8) for x in (first, last, strands, dense, gaps, tail)]


class World:
    def __init__(self, k, rc, prefilter=False):
        self.k, self.rc = k, rc
        self.refs = make_refs(k, 7000 + k)
        self.seqs = make_seqs(k, self.refs, 7100 + k)
        opts = kbo_amd.BuildOpts(k=k, add_revcomp=rc, num_threads=4)
        self.rs = refset.RefSet.build(self.refs, opts, wide_rows=WIDE_ROWS, positions=True, prefilter=prefilter)
        self.dicts = [occurrences(ref, k, rc) for ref in self.refs]
        self.queryable = [r for r in range(len(self.refs)) if self.rs.status(r) == 0]
        self.offsets = np.zeros(len(self.seqs) + 1, dtype=np.uint64)
        self.offsets[1:] = np.cumsum([len(s) for s in self.seqs])
        self._runs = None

    def cpu_runs(self):
        """kbo::find of every (reference, sequence, strand) on the CPU: the set's own matching statistics (kbo_refset_ms_host), then
        the oracle's derandomize, translate and run lengths (max_gap_len = GAP) -> REF_RUN records in find_refset's order"""
        if self._runs is None:
            out = []
            for r in self.queryable:
                thr = threshold(self.k, self.rs.n_kmers(r))
                for s, q in enumerate(self.seqs):
                    for strand in (1, 2):
                        ms = self.rs.ms_host(r, strand_seq(q, strand))
                        if not ((ms > thr).any() or (ms == self.k).any()):  # (every character is '-': kbo_hip.h, the prefilter)
                            continue
                        aln = ora.translate_ms_vec(ora.derandomize_ms_vec(ms, self.k, thr), self.k, thr)
                        out += [(r, s, strand) + tuple(t) for t in ora.run_lengths_gapped(aln, GAP)]
            self._runs = np.array(out, dtype=refset.REF_RUN)
        return self._runs

    def expected(self, runs):
        """brute force for every record: (q_first, ref_first, q_last, ref_last, flags, n_tested)"""
        out = np.zeros(len(runs), dtype=refset.REF_LOCUS)
        for x, w in enumerate(runs):
            loc = expected_locus(self.dicts[w["ref"]], self.k, self.seqs[w["seq"]], int(w["strand"]), int(w["start"]), int(w["end"]))
            out[x] = loc + (expected_tested(self.k, int(w["start"]), int(w["end"]), loc),)
        return out


_worlds = {}


def world(k, rc, prefilter=False):
    if (k, rc, prefilter) not in _worlds:
        _worlds[k, rc, prefilter] = World(k, rc, prefilter)
    return _worlds[k, rc, prefilter]


def reached(k, runs, loci):
    """how often each planted case occurs in a call's records"""
    start, end = runs["start"].astype(np.int64), runs["end"].astype(np.int64)
    has = loci["q_first"] != NONE
    lead = np.where(has, loci["q_first"].astype(np.int64) - start, -1)
    trail = np.where(has, end - k - loci["q_last"].astype(np.int64), -1)
    c = {"rev": int(((loci["flags"] & 3) != 0).sum()), "multi": int(((loci["flags"] & 12) != 0).sum()), "none": int((~has).sum()),
         "lead>=64": int((lead >= 64).sum()), "trail>=64": int((trail >= 64).sum()), "wide": int((runs["ref"] == WIDE).sum()),
         "exactly k": int((has & (end - start == k)).sum()), "shorter than k": int((end - start < k).sum()),
         "gap": int((runs["gap_bases"] > 0).sum()), "strand 1": int((runs["strand"] == 1).sum()), "strand 2": int((runs["strand"] == 2).sum()),
         "no anchor over windows": int((~has & (end - start - k + 1 > 2 * WINDOW)).sum())}
    for d in (0, 1, 63, 64, 65):
        c["lead=%d" % d] = int((lead == d).sum())
        c["trail=%d" % d] = int((trail == d).sum())
    c["lead~130"] = int(((lead >= 128) & (lead <= 135)).sum())
    c["trail~130"] = int(((trail >= 128) & (trail <= 135)).sum())
    return c


def assert_reached(k, rc, runs, loci):
    """every planted case occurs.  Not among them: a last anchor that ends ONE base in front of run.end.  A run of find ends on a
    character that is no gap; behind the last k-mer hit that is an 'M' or 'R' of a further match of more than `threshold` bases, or an
    'X', which translate.rs:199 writes only in front of an 'M' - so the distance is 0 or more than the threshold.  (In front of the
    first hit the same holds, except on a sequence's first two positions, where translate.rs:277 takes the previous value as k: the
    one 'X' that begins a run.)  tests/test_gpu_refset_locate.py reaches that distance with runs made by hand."""
    c = reached(k, runs, loci)
    need = [n for n in c if n not in ("rev", "trail=1")] + (["rev"] if rc else [])
    missing = [n for n in need if c[n] == 0]
    assert not missing, (missing, c)
    if not rc:
        assert c["rev"] == 0


# ---- the tests
def test_symbols_are_exported_and_declared():
    L = kbo_amd.lib()
    hdr = open(os.path.join(ROOT, "include", "kbo_hip.h")).read()
    rust = open(os.path.join(ROOT, "bindings", "rust", "kbo-hip", "src", "lib.rs")).read()
    for name in NEW_SYMBOLS:
        assert getattr(L, name) is not None and name in _capi.SYMBOLS
        assert re.search(r"\b%s\(" % name, hdr), name
        assert re.search(r"pub fn %s\(" % name, rust), name
    assert re.search(r"uint32_t n_tested;[^}]*\} kbo_ref_locus;", hdr) and "#define KBO_LOCUS_NONE 0xFFFFFFFFu" in hdr
    assert "#define KBO_POS_NONE 0xFFFFFFFFu" in hdr and "#define KBO_LOCUS_MULTI 0x80000000u" in hdr
    assert re.search(r"int32_t positions;", hdr) and re.search(r"pub positions: i32", rust)
    assert C.sizeof(_capi.RefLocus) == 24 == refset.REF_LOCUS.itemsize
    for fn in (refset.locate_refset, refset.locate_refset_dev, refset.locus_interval, refset.RefSet.has_positions, refset.RefSet.positions,
               refset.RefSet.ref_len):
        assert callable(fn)


def test_the_options_struct_keeps_its_size_and_its_default():
    assert C.sizeof(_capi.RefsetOpts) == C.sizeof(C.c_size_t) + 8 == 16  # what { size_t, int32_t } took, padding included
    o = _capi.RefsetOpts(1, 7, 7)
    kbo_amd.lib().kbo_refset_opts_default(C.byref(o))
    assert (o.max_wide_rows, o.prefilter, o.positions) == (refset.MAX_ROWS, 0, 0)


def _build(refs, k, rc, wide_rows, prefilter, positions):
    raw = [r.tobytes() for r in refs]
    arr = (C.c_char_p * len(raw))(*raw)
    lens = (C.c_size_t * len(raw))(*[len(s) for s in raw])
    co = kbo_amd.BuildOpts(k=k, add_revcomp=rc, num_threads=2)._to_c()
    ro = _capi.RefsetOpts(wide_rows, prefilter, positions)
    h = C.c_void_p()
    return kbo_amd.lib().kbo_refset_build_opts(arr, lens, len(raw), C.byref(co), C.byref(ro), C.byref(h)), h


def test_positions_0_is_the_set_as_it_was_and_other_values_are_refused():
    L = kbo_amd.lib()
    refs = make_refs(31, 5)
    for bad in (2, -1, 1 << 20):
        code, h = _build(refs, 31, False, WIDE_ROWS, 0, bad)
        assert code == E_BAD_ARG and not h.value
    plain = refset.RefSet.build(refs, kbo_amd.BuildOpts(k=31), wide_rows=WIDE_ROWS)
    code, h = _build(refs, 31, False, WIDE_ROWS, 0, 0)
    assert code == 0
    zero, one = refset.RefSet(h), refset.RefSet.build(refs, kbo_amd.BuildOpts(k=31), wide_rows=WIDE_ROWS, positions=True)
    assert not plain.has_positions() and not zero.has_positions() and one.has_positions()
    assert plain.positions_bytes() == zero.positions_bytes() == 0 < one.positions_bytes()
    n = C.c_size_t()
    assert L.kbo_refset_positions(zero._h, 0, None, C.byref(n)) == E_BAD_ARG
    for r in range(len(refs)):
        assert plain.ref_len(r) == zero.ref_len(r) == one.ref_len(r) == len(refs[r])
        assert plain.route(r) == zero.route(r) == one.route(r) and plain.n_kmers(r) == zero.n_kmers(r) == one.n_kmers(r)
        if plain.route(r) != refset.ROUTE_NONE:
            assert np.array_equal(plain.form(r), zero.form(r)) and np.array_equal(plain.form(r), one.form(r))
    assert plain.ref_len(len(refs)) == 0
    for args in ((3, 5000, 3, 100, 2), (8, 40000, 1, 10, 0)):
        for fn in (L.kbo_find_refset_dev_work_bytes, L.kbo_summary_refset_dev_work_bytes):
            assert fn(plain._h, *args) == fn(zero._h, *args) == fn(one._h, *args) > 0
        assert L.kbo_best_refset_dev_work_bytes(plain._h, *args[:3], args[4]) == L.kbo_best_refset_dev_work_bytes(one._h, *args[:3], args[4]) > 0
    total_rows = sum(len(one.positions(r)) for r in range(len(refs)))
    assert one.positions_bytes() == 4 * total_rows + 8 * (len(refs) + 1)


def _check_table(refs, k, rc, wide_rows):
    rs = refset.RefSet.build(refs, kbo_amd.BuildOpts(k=k, add_revcomp=rc, num_threads=2), wide_rows=wide_rows, positions=True)
    L = kbo_amd.lib()
    seen_multi = seen_rev = seen_cross = 0
    for r, ref in enumerate(refs):
        pos = rs.positions(r)
        if rs.route(r) in (refset.ROUTE_NONE, refset.ROUTE_INDEX):
            assert len(pos) == 0
            continue
        d = occurrences(ref, k, rc)
        rows = np.frombuffer(rs.form(r), dtype=np.uint8)
        assert len(pos) * 2 <= len(rows)  # (2 bytes a row and the padding of the form)
        # every full k-mer row has an entry, every other row none: as many entries as distinct k-mers
        assert int((pos != NONE).sum()) == len(d) == rs.n_kmers(r)
        # the entry of every k-mer, through the look-up: a run of exactly the k-mer on the '+' strand of a batch of one sequence
        kmers = sorted(d)
        batch = np.frombuffer(b"".join(kmers), dtype=np.uint8)
        offsets = np.array([0, len(batch)], dtype=np.uint64)
        runs = np.zeros(len(kmers), dtype=refset.REF_RUN)
        runs["ref"], runs["seq"], runs["strand"] = r, 0, 1
        runs["start"] = np.arange(len(kmers)) * k
        runs["end"] = runs["start"] + k
        loci = np.zeros(len(kmers), dtype=refset.REF_LOCUS)
        kbo_amd.check(L.kbo_locate_refset_host(rs._h, batch.ctypes.data, offsets.ctypes.data, 1, runs.ctypes.data, len(runs), loci.ctypes.data))
        e = np.array([entry_of(d[km]) for km in kmers], dtype=np.uint32)
        want = np.zeros(len(kmers), dtype=refset.REF_LOCUS)
        want["q_first"] = want["q_last"] = runs["start"]
        want["ref_first"] = want["ref_last"] = e & np.uint32(REV - 1)
        want["flags"] = np.where(e & np.uint32(REV), 3, 0) | np.where(e & np.uint32(MULTI), 12, 0)
        want["n_tested"] = 2
        bad = np.flatnonzero(loci != want)
        assert len(bad) == 0, (r, len(bad), kmers[bad[0]], d[kmers[bad[0]]], loci[bad[0]])
        # ... and the table as a whole: the multiset of its entries is the multiset of the expected entries
        exp = np.sort(np.array([entry_of(o) for o in d.values()], dtype=np.uint32))
        assert np.array_equal(np.sort(pos[pos != NONE]), exp)
        seen_multi += int((exp & MULTI != 0).sum())
        seen_rev += int((exp & REV != 0).sum())
        seen_cross += sum(1 for o in d.values() if len(o) == 2 and {s for s, _ in o} == {0, 1})
    return rs, seen_multi, seen_rev, seen_cross


@pytest.mark.parametrize("rc", [False, True])
@pytest.mark.parametrize("k", [5, 31, 96])
def test_the_position_table_against_brute_force(k, rc):
    refs = make_refs(k, 300 + k)
    if k == 5:
        refs = [r[:400] for r in refs[:6]] + [refs[WIDE][:3000], refs[SHORT]]  # (4^5 k-mers: every reference is full of repeats)
    rs, multi, rev, cross = _check_table(refs, k, rc, WIDE_ROWS)
    assert multi > 0 and (rev > 0) == rc and (cross > 0) == rc
    if k != 5:
        assert rs.route(WIDE) == refset.ROUTE_WIDE and rs.route(SHORT) == refset.ROUTE_NONE and rs.status(SHORT) != 0
        # the planted repeat and the twin on the other strand
        d = occurrences(refs[REPEAT], k, rc)
        assert [o for o in d.values() if (0, 100) in o and (0, 500) in o]
        if rc:
            d = occurrences(refs[RC_TWIN], k, rc)
            assert [o for o in d.values() if len(o) == 2 and o[0][0] != o[1][0]]
        # a stretch shorter than k and an N inside: no entry covers them
        for r, cut in ((WITH_N, 260), (WITH_GAP, 300)):
            p = rs.positions(r)
            p = p[p != NONE] & (REV - 1)
            assert not ((p <= cut) & (p + k > cut)).any()
        p = rs.positions(WITH_GAP)
        p = p[p != NONE] & (REV - 1)
        assert not ((p > 300) & (p < 300 + k)).any()


def test_a_single_index_reference_has_no_entries():
    refs = make_refs(31, 9)
    rs, _, _, _ = _check_table(refs, 31, False, refset.MAX_ROWS)  # wide_rows at its minimum: 20 kbp takes the single-index route
    assert rs.route(WIDE) == refset.ROUTE_INDEX and len(rs.positions(WIDE)) == 0 and len(rs.positions(0)) > 0
    runs = np.zeros(1, dtype=refset.REF_RUN)
    runs["ref"], runs["strand"], runs["end"] = WIDE, 1, 100
    with pytest.raises(kbo_amd.KboError) as e:
        refset.locate_refset([refs[0]], rs, runs, host=True)
    assert e.value.code == E_BAD_ARG


def test_a_reference_of_2_to_the_30_bases_is_refused_before_any_work():
    L = kbo_amd.lib()
    a = np.frombuffer(b"ACGTACGTAC", dtype=np.uint8)
    arr = (C.c_char_p * 2)(a.tobytes(), a.tobytes())
    lens = (C.c_size_t * 2)(len(a), 1 << 30)  # (a length the call must refuse before it reads a base)
    co = kbo_amd.BuildOpts(k=5)._to_c()
    ro = _capi.RefsetOpts(refset.MAX_ROWS, 0, 1)
    h = C.c_void_p()
    assert L.kbo_refset_build_opts(arr, lens, 2, C.byref(co), C.byref(ro), C.byref(h)) == E_UNSUPPORTED and not h.value


@pytest.mark.parametrize("rc", [False, True])
@pytest.mark.parametrize("k", [31, 96])
def test_locate_host_against_brute_force_and_every_planted_case(k, rc):
    """the fixtures of the GPU test, on the CPU first: every record against brute force, and every planted case occurs"""
    w = world(k, rc)
    runs = w.cpu_runs()
    assert len(runs) > 40
    loci = refset.locate_refset(w.seqs, w.rs, runs, host=True)
    exp = w.expected(runs)
    bad = [x for x in range(len(runs)) if tuple(loci[x]) != tuple(exp[x])]
    assert not bad, (bad[:5], [(runs[x], loci[x], exp[x]) for x in bad[:3]])
    assert_reached(k, rc, runs, loci)
    last = len(w.seqs) - 1
    assert [x for x in range(len(runs)) if runs["seq"][x] == last and runs["strand"][x] == 1 and runs["end"][x] == len(w.seqs[last])]


def test_hand_made_runs():
    w = world(31, True)
    q = w.seqs[2]
    runs = np.zeros(6, dtype=refset.REF_RUN)
    runs["ref"], runs["seq"] = 9, 2
    runs["strand"] = [1, 1, 2, 1, 1, 2]
    runs["start"] = [0, 0, 0, 100, len(q), len(q) - 40]
    runs["end"] = [len(q), 30, len(q), 100, len(q), len(q)]
    loci = refset.locate_refset(w.seqs, w.rs, runs, host=True)
    assert [tuple(v) for v in loci] == [tuple(v) for v in w.expected(runs)]
    assert loci["q_first"][0] != NONE and loci["q_first"][2] != NONE and tuple(loci[1]) == (NONE,) * 4 + (0, 0) == tuple(loci[3]) == tuple(loci[4])
    assert len(refset.locate_refset(w.seqs, w.rs, runs[:0], host=True)) == 0


def test_argument_errors_and_their_order_need_no_device():
    L = kbo_amd.lib()
    w = world(31, False)
    plain = refset.RefSet.build(w.refs, kbo_amd.BuildOpts(k=31), wide_rows=WIDE_ROWS)
    concat = np.concatenate(w.seqs)
    off = w.offsets.copy()
    good = np.zeros(2, dtype=refset.REF_RUN)
    good["ref"], good["seq"], good["strand"], good["start"], good["end"] = [0, 12], [0, 5], [1, 2], [5, 0], [200, len(w.seqs[5])]
    loci = np.zeros(2, dtype=refset.REF_LOCUS)
    Q, OFF, RUNS, CNT, LOCI = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000  # device pointers that nothing ever follows

    for fn in (L.kbo_locate_refset_host, L.kbo_locate_refset):
        def call(h=w.rs._h, q=concat.ctypes.data, o=off, n_seqs=len(w.seqs), runs=good, n=None, out=loci.ctypes.data):
            n = len(runs) if n is None and runs is not None else (n or 0)
            return fn(h, q, None if o is None else o.ctypes.data, n_seqs, None if runs is None else runs.ctypes.data, n, out)
        if fn is L.kbo_locate_refset_host:
            assert call() == 0
        assert call(n=0) == 0 and call(runs=None, n=0, out=None) == 0  # nothing to do: nothing touched, a device included
        for kw in (dict(h=None), dict(q=None), dict(o=None), dict(runs=None, n=2), dict(out=None)):
            assert call(**kw) == E_BAD_ARG, kw
        assert call(h=plain._h) == E_BAD_ARG and call(h=plain._h, n_seqs=0) == E_BAD_ARG  # no positions: before the batch
        assert call(n_seqs=0) == E_EMPTY_QUERY
        o2 = off.copy()
        o2[2] = o2[1] + 2
        assert call(o=o2) == E_LEN_LE_2
        o2[2] = o2[1] - 1
        assert call(o=o2) == E_BAD_ARG
        o2 = off.copy()
        o2[0] = 1
        assert call(o=o2) == E_BAD_ARG
        # the records bit 4 describes, after the batch: an unusable record AND a bad batch reports the batch
        for field, value in (("ref", len(w.refs)), ("ref", SHORT), ("seq", len(w.seqs)), ("strand", 0), ("strand", 3), ("start", 201),
                             ("end", len(w.seqs[0]) + 1), ("ref", 0xFFFFFFFF)):
            bad = good.copy()
            bad[field][0] = value
            assert call(runs=bad) == E_BAD_ARG, (field, value)
            assert call(runs=bad, n_seqs=0) == E_EMPTY_QUERY
        edge = good.copy()
        edge["start"][0] = edge["end"][0] = len(w.seqs[0])  # start == end == len is a run of nothing, not an error
        if fn is L.kbo_locate_refset_host:
            assert call(runs=edge) == 0

    # (a set of its own: world()'s sets are shared with the GPU tests, which give them a device copy, and these pointers are fake)
    fresh = refset.RefSet.build(w.refs[:3], kbo_amd.BuildOpts(k=31), positions=True)

    def dev(h=fresh._h, q=Q, o=OFF, n_seqs=6, total=int(off[-1]), runs=RUNS, cnt=CNT, cap=10, out=LOCI):
        return L.kbo_locate_refset_dev(h, q, o, n_seqs, total, runs, cnt, cap, out, None)
    for kw in (dict(h=None), dict(q=None), dict(o=None), dict(cnt=None), dict(runs=None), dict(out=None), dict(q=Q + 8), dict(o=OFF + 4),
               dict(cnt=CNT + 4), dict(runs=RUNS + 2), dict(out=LOCI + 1), dict(h=plain._h), dict(h=plain._h, n_seqs=0)):
        assert dev(**kw) == E_BAD_ARG, kw
    assert dev(n_seqs=0) == E_EMPTY_QUERY
    assert dev() == E_BAD_ARG  # a set without a copy on the current device: nothing is enqueued


def test_locate_arithmetic_under_sanitizers(tmp_path):
    """tools/refset_locate_check.cpp: the look-up, the strand's bases and the serial search of refset_locate.hpp through accessors
    that check every index, against brute force of its own, over a form and a table written here"""
    w = world(31, True)
    exe = str(tmp_path / "refset_locate_check")
    subprocess.run(["c++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I",
                    os.path.join(ROOT, "kbo_amd", "csrc"), os.path.join(ROOT, "tools", "refset_locate_check.cpp"), "-o", exe], check=True)
    for r in (REPEAT, RC_TWIN, WITH_N):
        pos = w.rs.positions(r)
        files = {}
        for name, data in (("form", w.rs.form(r)), ("pos", pos.view(np.uint8)), ("ref", w.refs[r]), ("query", w.seqs[2])):
            files[name] = str(tmp_path / ("%s_%d" % (name, r)))
            data.tofile(files[name])
        run = subprocess.run([exe, files["form"], files["pos"], files["ref"], files["query"], str(len(pos)), "31", "1"], capture_output=True, text=True)
        assert run.returncode == 0, run.stdout + run.stderr
        assert "in range" in run.stdout and "agree" in run.stdout


def test_locus_interval_on_planted_substitution_only_inserts():
    w = world(31, True)
    k, rng = 31, np.random.default_rng(11)
    cases = [(9, 100, 400, False), (8, 200, 500, True), (10, 0, 300, False), (11, 1700, 2000, True), (WIDE, 7000, 7500, False)]
    seqs, exp = [], []
    for r, lo, hi, flip in cases:
        piece = _sub(w.refs[r][lo:hi], range(40, hi - lo - 40, 53))  # substitutions only: the diagonal holds
        seqs.append(np.concatenate([_rnd(rng, 200), revcomp(piece) if flip else piece, _rnd(rng, 150)]))
        exp.append((r, lo, hi, 2 if flip else 1))
    runs = np.zeros(len(cases), dtype=refset.REF_RUN)
    for x, (r, lo, hi, flip) in enumerate(cases):
        runs[x] = (r, x, 1, 200, 200 + hi - lo, 0, 0, 0, 0, 0)
    loci = refset.locate_refset(seqs, w.rs, runs, host=True)
    ref_lens = [w.rs.ref_len(r) for r in range(len(w.refs))]
    lo, hi, orient = refset.locus_interval(runs, loci, k, ref_lens)
    assert [(int(runs["ref"][x]), int(lo[x]), int(hi[x]), int(orient[x])) for x in range(len(cases))] == exp
    # the same inserts seen from the '-' strand of the sequence: the other orientation, the same interval
    runs2 = runs.copy()
    runs2["strand"] = 2
    runs2["start"], runs2["end"] = 150, 150 + (runs["end"] - runs["start"])
    loci2 = refset.locate_refset(seqs, w.rs, runs2, host=True)
    lo2, hi2, orient2 = refset.locus_interval(runs2, loci2, k, ref_lens)
    assert np.array_equal(lo2, lo) and np.array_equal(hi2, hi) and np.array_equal(orient2, 3 - orient)
    # a run that sticks out of the reference is clipped; a run without an anchor gives -1
    runs3 = runs[:2].copy()
    runs3[0] = (10, 2, 1, 150, 500, 0, 0, 0, 0, 0)      # 50 bases in front of the reference's first base
    runs3[1] = (9, 0, 1, 0, 150, 0, 0, 0, 0, 0)         # random bases only
    loci3 = refset.locate_refset(seqs, w.rs, runs3, host=True)
    lo3, hi3, orient3 = refset.locus_interval(runs3, loci3, k, ref_lens)
    assert (int(lo3[0]), int(hi3[0]), int(orient3[0])) == (0, 300, 1) and (int(lo3[1]), int(hi3[1]), int(orient3[1])) == (-1, -1, -1)
