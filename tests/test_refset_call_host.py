"""The variants of a pair (kbo_hip.h "The VARIANTS of a pair") on the host: kbo_call_refset_host - the CPU restatement of
refset_call_kernels.hip over kbo_amd/csrc/refset_call.hpp, with the second pass kbo_call_refset shares - the spelling of a row off
the packed form, and the argument errors.

Yardstick 1 is the oracle's literal kbo::call: oracle.Index.build([reference], k, add_revcomp).call(sequence or its reverse
complement, k, p) for every (reference, sequence, strand) whose oracle matches() holds a character other than '-' - the pairs
kbo_summary_refset has a record for.  Every field and character of every record is compared.  The oracle's call does not model
add_revcomp of the sequence's own index, so that setting is only compared with itself here; tests/test_gpu_refset_call.py compares it
with kbo_amd.call on one index per reference.  The planted cases are asserted to occur, from the oracle's variants and from the sites
(i, j, row) of the first pass restated here over the oracle's matching statistics.  tools/refset_call_check.cpp runs the scan, the
match and the spelling through accessors that check every index, with the slabs' offsets given explicitly, as a stand-alone program
with and without AddressSanitizer and UBSan.  No GPU.
tests/test_gpu_refset_call.py takes world() from here."""
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
E_EMPTY_QUERY, E_LEN_LE_2, E_BAD_ARG, E_K_MISMATCH, E_UNSUPPORTED = -1, -2, -4, -6, -8
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
COMP = np.arange(256, dtype=np.uint8)  # (lower case stays what it is: no base on either strand)
for _a, _b in zip(b"ACGT", b"TGCA"):
    COMP[_a] = _b
WIDE_ROWS = 1 << 17
ALLELE_A, MOVED, WIDE, ALLELE_B, SHORT = 6, 1, 12, 13, 14
KS, PROBS = (31, 41, 63, 96), (1e-7, 1e-4)
NEW_SYMBOLS = ["kbo_call_refset", "kbo_call_refset_host", "kbo_ref_calls_free", "kbo_refset_last_call", "kbo_refset_spell_row"]


def _rnd(rng, n):
    return ACGT[rng.integers(0, 4, n)].copy()


def _other(base, step=1):
    return ACGT[(int(np.searchsorted(ACGT, base)) + step) % 4]


def _sub(a, at, width=1):
    """a copy of `a` with substitutions of `width` bases at the offsets `at`"""
    a = a.copy()
    for i in at:
        for j in range(i, i + width):
            a[j] = _other(a[j])
    return a


def revcomp(a):
    return COMP[a[::-1]]


def strand_seq(q, strand):
    return q if strand == 1 else revcomp(q)


def threshold(k, n_kmers, prob=1e-7):
    t = C.c_size_t()
    kbo_amd.check(kbo_amd.lib().kbo_random_match_threshold(k, n_kmers, 4, prob, C.byref(t)))
    return t.value


def call_opts(k, prob=1e-7, add_revcomp=False):
    return kbo_amd.CallOpts(max_error_prob=prob, sbwt_build_opts=kbo_amd.BuildOpts(k=k, add_revcomp=add_revcomp, build_select=True))


# ---- the set and the batch
def make_refs(k, seed):
    rng = np.random.default_rng(seed)
    refs = [_rnd(rng, n) for n in (300, 400, 520, 640, 777, 900, 1000, 1100, 1300, 1500, 1800, 2000)]
    refs.append(_rnd(rng, 20000))                                 # WIDE
    refs.append(_sub(refs[ALLELE_A], (200, 420, 640, 860)))        # ALLELE_B: a few substitutions from ALLELE_A
    refs.append(_rnd(rng, k - 1))                                 # SHORT: no k-mer, a status
    return refs


def make_seqs(k, refs, thr, seed):
    """thr[p][r]: reference r's threshold at max_error_prob p.  Returns the contigs and a dict of where the planted cases lie"""
    rng = np.random.default_rng(seed)
    gap = lambda n=300: _rnd(rng, n)
    at = {}
    # substitution, multi-base substitution; insertion, deletion; two variants fewer than k bases apart
    ins = np.concatenate([refs[8][:400], _rnd(rng, 2), refs[8][400:800], refs[8][803:]])
    c0 = [gap(500), _sub(_sub(refs[7], [300]), [600], 3), gap(), ins, gap(400), _sub(refs[9], (700, 720)), gap(500)]
    at["substitution"] = (7, 0, 500 + 300)
    at["multi-base"] = (7, 0, 500 + 600)
    at["insertion"] = (8, 0, 500 + 1100 + 300 + 400)
    at["deletion"] = (8, 0, 500 + 1100 + 300 + 802)
    at["close pair"] = (9, 0, 500 + 1100 + 300 + len(ins) + 400 + 700)
    # a copy from a contig's first base with a variant whose match lies in its first k - 1 bases; a variant so near a reference's
    # first base that the matched row is no full k-mer
    t3, t4 = thr[1e-7][3], thr[1e-7][4]
    c1 = [_sub(refs[3][100:600], [t3 + 3]), gap(), _sub(refs[4], [t4 + 3]), gap(1200)]
    at["j < k - 1"] = (3, 1, t3 + 3)
    at["'$' in the row"] = (4, 1, 500 + 300 + t4 + 3)
    # copies that end at a contig's last base, with the match of their last variant at it: one for each max_error_prob
    tails = []
    for p, r in ((1e-7, 5), (1e-4, 2)):
        body = refs[r][100:500]
        tails.append([gap(1700), _sub(body, [len(body) - 1 - thr[p][r]])])
        at["j = len - 1", p] = (r, 2 if p == 1e-7 else 3, 1700 + len(body) - 1 - thr[p][r])
    with_n = _sub(refs[10], [1200])
    with_n[900] = ord("N")
    c4 = [gap(), with_n, gap(200)]
    at["N"] = (10, 4, 300 + 900)
    minus = np.concatenate([refs[11][:1200], refs[11][1203:]])
    c5 = [gap(400), revcomp(_sub(minus, [500])), gap()]
    at["'-' only"] = 11
    # a reference's end inside a contig; one allele whole, to be called against the other; a rearranged reference: at the joint the
    # k-mers of both sides match up to the joint, so query_overlap == ref_overlap (variant_calling.rs:175)
    # (neither side may go on matching across the joint by chance: the base behind either piece is not the one the other side has)
    m = refs[MOVED]
    e = 330
    while m[e] == m[160]:
        e += 1
    c6 = [gap(), refs[2][200:], gap(400), refs[ALLELE_A], gap(), m[60:160], [_other(m[160])], _rnd(rng, 49), m[e - 100:e], m[160:], gap(200)]
    at["reference end"] = (2, 6, 300 + 320)
    at["joint"] = (MOVED, 6, 300 + 320 + 400 + 1000 + 300 + 100 + 50 + 100)
    # many sites: substitutions 37 apart over 9 000 bases of the wide reference - i mod 64 takes every value
    c7 = [gap(500), _sub(refs[WIDE][10000:19000], range(40, 8990, 37)), gap(500)]
    seqs = [np.concatenate(x).astype(np.uint8) for x in [c0, c1] + tails + [c4, c5, c6, c7]]
    return seqs, at


class World:
    def __init__(self, k, rc, prefilter=False):
        self.k, self.rc = k, rc
        self.refs = make_refs(k, 9000 + k)
        opts = kbo_amd.BuildOpts(k=k, add_revcomp=rc, num_threads=4)
        self.rs = refset.RefSet.build(self.refs, opts, wide_rows=WIDE_ROWS, prefilter=prefilter)
        self.queryable = [r for r in range(len(self.refs)) if self.rs.status(r) == 0]
        self.thr = {p: [threshold(k, self.rs.n_kmers(r), p) if r in self.queryable else 0 for r in range(len(self.refs))] for p in PROBS}
        self.seqs, self.at = make_seqs(k, self.refs, self.thr, 9100 + k)
        self._index, self._own, self._oracle = {}, {}, {}

    def index(self, r):
        if r not in self._index:
            self._index[r] = ora.Index.build([self.refs[r]], self.k, add_revcomp=self.rc)
        return self._index[r]

    def oracle(self, prob):
        """{(r, s, strand): the oracle's variants} for the pairs with a hit, and the number of variants in the pairs without one"""
        if prob not in self._oracle:
            kept, dropped = {}, 0
            for r in self.queryable:
                ix = self.index(r)
                ms_floor = self.thr[prob][r]
                for s, q in enumerate(self.seqs):
                    for strand in (1, 2):
                        seq = strand_seq(q, strand)
                        hit = bool(re.search(b"[^-]", ix.matches(seq, prob)))
                        # (a pair without a depth of the threshold has no site: the oracle's call of it is empty, and is not made)
                        if not hit and int(ix.matching_statistics(seq)[0].max()) < ms_floor:
                            continue
                        calls = [(pos, qc.encode(), rf.encode()) for pos, qc, rf in ix.call(seq, self.k, prob)[0]]
                        if hit:
                            kept[r, s, strand] = calls
                        else:
                            dropped += len(calls)
            self._oracle[prob] = (kept, dropped)
        return self._oracle[prob]

    def expected(self, prob, strands):
        """the records of kbo_call_refset by yardstick 1, as tuples (ref, seq, strand, pos, query_chars, ref_chars) in its order"""
        kept, _ = self.oracle(prob)
        return [(r, s, strand) + v for (r, s, strand), calls in sorted(kept.items()) if strands & strand for v in calls]

    def sites(self, prob, r, s, strand):
        """the first pass over the oracle's matching statistics: [(i, j or None, row or None)] of one pair"""
        d, lo, hi = self.index(r).matching_statistics(strand_seq(self.seqs[s], strand))
        d, t, out = d.astype(np.int64), self.thr[prob][r], []
        for i in np.flatnonzero((d[1:] < d[:-1]) & (d[:-1] >= t) & (d[1:] < t)) + 1:
            found = (int(i), None, None)
            for j in range(i + 1, min(i + self.k + 1, len(d))):
                if d[j] >= t and hi[j] - lo[j] == 1:
                    found = (int(i), j, int(lo[j]))
                    break
            out.append(found)
        return out

    def own_index(self, s, strand):
        if (s, strand) not in self._own:
            self._own[s, strand] = ora.Index.build([strand_seq(self.seqs[s], strand)], self.k)
        return self._own[s, strand]

    def resolve(self, prob, r, s, strand, site):
        """resolve_variant (variant_calling.rs:139-201) of one site: 'ok', 'no peak' or 'equal overlaps'"""
        k, t, (i, j, row) = self.k, self.thr[prob][r], site
        seq = strand_seq(self.seqs[s], strand)
        qk = b"$" * max(0, k - 1 - j) + seq[max(0, j + 1 - k):j + 1].tobytes()
        rk = self.index(r).access_kmer(row)
        vs_ref = self.index(r).matching_statistics(np.frombuffer(qk, dtype=np.uint8))[0]
        vs_query = self.own_index(s, strand).matching_statistics(np.frombuffer(rk, dtype=np.uint8))[0]

        def peak(ms):
            for x in range(k - 2, -1, -1):
                if ms[x] >= t and ms[x] > ms[x + 1]:
                    return x
            return None
        csl = 0
        while csl < k and qk[k - 1 - csl] == rk[k - 1 - csl]:
            csl += 1
        qp, rp = peak(vs_ref), peak(vs_query)
        if qp is None or rp is None:
            return "no peak"
        qgap, rgap = k - csl - qp - 1, k - csl - rp - 1
        return "ok" if (qgap > 0 and rgap > 0) or qgap != rgap else "equal overlaps"

    def assert_reached(self, prob=1e-7):
        """every planted case occurs, in the oracle's variants or in the sites of the first pass"""
        k, kept = self.k, self.oracle(prob)[0]
        useful = k >= 41  # (k >= 2 t or so: below it the reference resolves little but deletions; kbo_hip.h)

        def near(name, what=None):
            r, s, pos = self.at[name]
            got = [v for v in kept.get((r, s, 1), []) if pos - 3 <= v[0] <= pos + 3]
            assert got and (what is None or what(got[0])), (name, got)
            return got[0]
        if useful:
            near("deletion", lambda v: v[1] == b"" and len(v[2]) == 3)
            near("substitution", lambda v: len(v[1]) == 1 == len(v[2]) and v[1] != v[2])
            near("multi-base", lambda v: len(v[1]) == 3 == len(v[2]))
            near("insertion", lambda v: len(v[1]) == 2 and v[2] == b"")
            near("N", lambda v: b"N" in v[1])
            r, s, pos = self.at["close pair"]
            pair = [v[0] for v in kept[r, s, 1] if pos - 3 <= v[0] <= pos + 23]
            assert len(pair) == 2 and 0 < pair[1] - pair[0] < k, pair
            assert len(kept[ALLELE_B, 6, 1]) == 4 and kept[ALLELE_A, 6, 1] == []  # the allele against the other one, and against itself
            r = self.at["'-' only"]
            assert len(kept[r, 5, 2]) == 2 and (self.rc or prob != 1e-7 or (r, 5, 1) not in kept)
        if prob != 1e-7:
            r, s, pos = self.at["j = len - 1", prob]
            assert (pos, len(self.seqs[s]) - 1) in [(i, j) for i, j, _ in self.sites(prob, r, s, 1)]
            return
        r, s, pos = self.at["j = len - 1", prob]
        assert (pos, len(self.seqs[s]) - 1) in [(i, j) for i, j, _ in self.sites(prob, r, s, 1)]
        if useful:
            r, s, pos = self.at["j < k - 1"]
            first = self.sites(prob, r, s, 1)[0]
            assert first[0] == pos and first[1] < k - 1 and near("j < k - 1")
            r, s, pos = self.at["'$' in the row"]
            site = [x for x in self.sites(prob, r, s, 1) if x[0] == pos][0]
            assert self.index(r).access_kmer(site[2]).startswith(b"$") and near("'$' in the row")
        r, s, pos = self.at["reference end"]
        assert (pos, None, None) in self.sites(prob, r, s, 1)
        r, s, pos = self.at["joint"]
        joint = [x for x in self.sites(prob, r, s, 1) if pos <= x[0] <= pos + 3 and x[1] is not None]  # (the joint may match a base on by chance)
        assert joint
        if useful:
            assert self.resolve(prob, r, s, 1, joint[0]) == "equal overlaps" and not [v for v in kept[r, s, 1] if v[0] == joint[0][0]]
        every = [x for x in self.sites(prob, WIDE, 7, 1) if x[1] is not None]
        assert len(every) >= 200 and len({i % 64 for i, _, _ in every}) == 64


_worlds = {}


def world(k, rc, prefilter=False):
    if (k, rc, prefilter) not in _worlds:
        _worlds[k, rc, prefilter] = World(k, rc, prefilter)
    return _worlds[k, rc, prefilter]


def as_tuples(variants, chars):
    return [(int(v["ref"]), int(v["seq"]), int(v["strand"]), int(v["pos"])) + refset.variant_chars(v, chars) for v in variants]


# ---- the tests
def test_symbols_are_exported_and_declared():
    L = kbo_amd.lib()
    hdr = open(os.path.join(ROOT, "include", "kbo_hip.h")).read() + open(os.path.join(ROOT, "include", "kbo_hip_tuning.h")).read()
    rust = open(os.path.join(ROOT, "bindings", "rust", "kbo-hip", "src", "lib.rs")).read()
    for name in NEW_SYMBOLS:
        assert getattr(L, name) is not None and name in (_capi.TUNING_SYMBOLS if "last_call" in name or "spell" in name else _capi.SYMBOLS)
        assert re.search(r"\b%s\(" % name, hdr), name
        assert re.search(r"pub fn %s\(" % name, rust), name
    assert re.search(r"uint16_t query_len, ref_len;[^}]*\} kbo_ref_variant;", hdr) and "pub struct RefVariant" in rust and "pub struct RefCalls" in rust
    assert refset.REF_VARIANT.itemsize == 24 and C.sizeof(_capi.RefCalls) == 32
    for fn in (refset.call_refset, refset.variant_chars, refset.last_call, kbo_amd.call_refset, refset.RefSet.spell_row):
        assert callable(fn)


def test_the_world_is_what_the_issue_asks_for():
    w = world(41, False)
    lens = [len(r) for r in w.refs]
    assert sum(300 <= n <= 2000 for n in lens) >= 12 and w.rs.route(WIDE) == refset.ROUTE_WIDE and w.rs.status(SHORT) != 0 and w.rs.packed_only()
    assert 0 < int((w.refs[ALLELE_A] != w.refs[ALLELE_B]).sum()) <= 4
    assert len(w.seqs) == 8 and all(2000 <= len(s) <= 30000 for s in w.seqs) and sum(len(s) for s in w.seqs) <= 10**5
    assert all(15 <= w.thr[1e-7][r] <= 18 for r in w.queryable)
    assert w.rs.spell_row(0, 0) == b"$" * 41 and refset.REF_VARIANT.itemsize == 24  # (row 0 is the root)


@pytest.mark.parametrize("prob", PROBS)
@pytest.mark.parametrize("rc", [False, True])
@pytest.mark.parametrize("k", KS)
def test_call_host_against_the_oracle(k, rc, prob):
    """yardstick 1: every field and character of every record, on both strands, each strand alone, and the order"""
    w = world(k, rc)
    kept, dropped = w.oracle(prob)
    print("k %d rc %d p %g: %d pairs with a hit, %d variants, %d variants of the oracle in pairs without a hit" %
          (k, rc, prob, len(kept), sum(len(v) for v in kept.values()), dropped))
    if prob == 1e-7:
        assert dropped == 0
    for strands in (3, 1, 2):
        variants, chars = refset.call_refset(w.seqs, w.rs, call_opts(k, prob), strands, host=True)
        got, exp = as_tuples(variants, chars), w.expected(prob, strands)
        assert got == exp, [x for x in zip(got, exp) if x[0] != x[1]][:3]
        stats = refset.last_call()
        assert stats[3] == len(exp) and stats[0] > 0 and stats[1] >= stats[2] >= stats[3]
        if len(variants):
            assert int(variants["chars"][-1]) + int(variants["query_len"][-1]) + int(variants["ref_len"][-1]) == len(chars)
        if strands == 3:
            assert k < 41 or (len(exp) > 150 and {1, 2} <= {x[2] for x in exp})  # (below k = 2 t or so little is resolved)
    w.assert_reached(prob)


@pytest.mark.parametrize("k", [41, 96])
def test_the_sequences_own_index_with_reverse_complements_changes_nothing_here(k):
    """no contig holds a stretch and its reverse complement: add_revcomp of the call's options, which the oracle's call does not
    model, leaves every record as it is.  (tests/test_gpu_refset_call.py compares that setting with kbo_amd.call.)"""
    w = world(k, True)
    a = refset.call_refset(w.seqs, w.rs, call_opts(k), host=True)
    b = refset.call_refset(w.seqs, w.rs, call_opts(k, add_revcomp=True), host=True)
    assert len(a[0]) > 150 and a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


@pytest.mark.parametrize("k", [5, 31, 96])
def test_spelling_every_row(k):
    """kbo_refset_spell_row against the oracle's access_kmer for every row of every reference"""
    rng = np.random.default_rng(k)
    refs = [_rnd(rng, n) for n in (k, k + 1, 300, 777, 2000)] + [_rnd(rng, 20000), _rnd(rng, max(1, k - 1))]
    refs[3][400] = ord("N")
    for rc in (False, True):
        rs = refset.RefSet.build(refs, kbo_amd.BuildOpts(k=k, add_revcomp=rc, num_threads=2), wide_rows=WIDE_ROWS)
        rows = 0
        for r, ref in enumerate(refs[:-1]):
            ix = ora.Index.build([ref], k, add_revcomp=rc)
            n = ix.n_sets
            assert rs.route(r) in (refset.ROUTE_LDS, refset.ROUTE_WIDE)
            for row in range(n):
                assert rs.spell_row(r, row) == ix.access_kmer(row), (k, rc, r, row)
                rows += 1
            out = np.zeros(k, dtype=np.uint8)
            assert kbo_amd.lib().kbo_refset_spell_row(rs._h, r, n, out.ctypes.data) == E_BAD_ARG
        assert rows > 2000 or k == 5
        out = np.zeros(k, dtype=np.uint8)
        L = kbo_amd.lib()
        assert L.kbo_refset_spell_row(rs._h, len(refs) - 1, 0, out.ctypes.data) == E_BAD_ARG  # a reference with a status
        assert L.kbo_refset_spell_row(rs._h, len(refs), 0, out.ctypes.data) == E_BAD_ARG
        assert L.kbo_refset_spell_row(rs._h, 0, 0, None) == E_BAD_ARG and L.kbo_refset_spell_row(None, 0, 0, out.ctypes.data) == E_BAD_ARG


def test_argument_errors_and_their_order_need_no_device():
    L = kbo_amd.lib()
    k = 41
    w = world(k, False)
    concat = np.concatenate(w.seqs)
    off = np.zeros(len(w.seqs) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(s) for s in w.seqs])
    single = refset.RefSet.build(w.refs, kbo_amd.BuildOpts(k=k))  # (without wide_rows the long reference takes the single-index route)
    assert not single.packed_only()
    for fn in (L.kbo_call_refset_host, L.kbo_call_refset):
        res = _capi.RefCalls(7, 7, 0x1000, 0x1000)

        def call(h=w.rs._h, q=concat.ctypes.data, o=off, n_seqs=len(w.seqs), kk=k, prob=1e-7, strands=3, out=res, opts=True):
            o_c = _capi.CallOpts(prob, kbo_amd.BuildOpts(k=kk, build_select=True)._to_c())
            return fn(h, q, None if o is None else o.ctypes.data, n_seqs, C.byref(o_c) if opts else None, strands, None if out is None else C.byref(out))
        for kw in (dict(strands=0), dict(strands=4), dict(strands=0, h=None)):
            assert call(**kw) == E_BAD_ARG, kw
        assert (res.n_variants, res.variants) == (7, 0x1000)  # (out is cleared only once it is known to be one)
        assert call(h=None) == E_BAD_ARG and call(out=None) == E_BAD_ARG and call(out=None, kk=31) == E_BAD_ARG
        # k of the options, then the routes, then what kbo_summary_refset checks, in its order
        assert call(kk=31) == E_K_MISMATCH and call(kk=31, h=single._h) == E_K_MISMATCH and call(kk=31, prob=2.0, n_seqs=0) == E_K_MISMATCH
        assert (res.n_variants, res.n_chars, res.variants, res.chars) == (0, 0, None, None)
        assert call(opts=False) == E_K_MISMATCH  # (the defaults have k = 31)
        assert call(h=single._h) == E_UNSUPPORTED and call(h=single._h, prob=2.0) == E_UNSUPPORTED and call(h=single._h, q=None) == E_UNSUPPORTED
        assert call(prob=2.0) == E_BAD_ARG and call(prob=0.0, n_seqs=0) == E_BAD_ARG and call(prob=2.0, q=None) == E_BAD_ARG
        assert call(q=None) == E_BAD_ARG and call(o=None) == E_BAD_ARG
        assert call(n_seqs=0) == E_EMPTY_QUERY
        o2 = off.copy()
        o2[2] = o2[1] + 2
        assert call(o=o2) == E_LEN_LE_2
        o2[2] = o2[1] - 1
        assert call(o=o2) == E_BAD_ARG
        o2 = off.copy()
        o2[0] = 1
        assert call(o=o2) == E_BAD_ARG
    L.kbo_ref_calls_free(None)
    empty = _capi.RefCalls()
    L.kbo_ref_calls_free(C.byref(empty))
    out = (C.c_uint64 * 4)()
    assert L.kbo_refset_last_call(None) == E_BAD_ARG and L.kbo_refset_last_call(out) == 0
    # a reference with a status contributes nothing, and unrelated contigs give nothing at all
    rng = np.random.default_rng(4)
    variants, chars = refset.call_refset([_rnd(rng, 3000), _rnd(rng, 500)], w.rs, call_opts(k), host=True)
    assert len(variants) == 0 == len(chars) and refset.last_call()[2:] == (0, 0)
    full = refset.call_refset(w.seqs, w.rs, call_opts(k), host=True)[0]
    assert SHORT not in set(full["ref"]) and len(full) > 150


def _check_tool(tmp_path, sanitize):
    exe = str(tmp_path / ("refset_call_check" + ("_san" if sanitize else "")))
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else []
    subprocess.run(["c++", "-std=c++17", "-O1", "-g"] + flags + ["-I", os.path.join(ROOT, "kbo_amd", "csrc"),
                    os.path.join(ROOT, "tools", "refset_call_check.cpp"), "-o", exe], check=True)
    return exe


def _run_tool(exe, tmp_path, k, rc, r, s, cut=None):
    w = world(k, rc)
    seq = w.seqs[s][:cut]
    form, ms = w.rs.form(r), w.rs.ms_host(r, seq)
    paths = [str(tmp_path / ("%s_%d_%d_%d" % (name, k, rc, r))) for name in ("form", "seq", "ms")]
    for path, a in zip(paths, (form, seq, ms)):
        a.tofile(path)
    run = subprocess.run([exe] + paths + [str(w.index(r).n_sets), str(k), str(w.thr[1e-7][r])], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "agree with the definition" in run.stdout and "in range" in run.stdout
    m = re.search(r"(\d+) candidates and (\d+) sites .* lanes 0/63 of a wave (\d+)/(\d+), 0/255 of a workgroup (\d+)/(\d+)", run.stdout)
    return [int(v) for v in m.groups()]


def test_scan_and_match_at_their_boundaries(tmp_path):
    """the header's scan and match over slabs whose offsets put every site on the first and the last lane of a wave and of a workgroup
    of 256, a candidate at i = 1, pairs that were not kept, a boundary between pairs that would be a candidate, and windows of j cut
    by the sequence end - tools/refset_call_check.cpp, against the definition written out there"""
    exe = _check_tool(tmp_path, False)
    for k, rc, r, s in ((41, False, 7, 0), (31, True, 8, 0), (96, False, 9, 0), (63, True, 3, 1)):
        cands, sites, w0, w63, g0, g255 = _run_tool(exe, tmp_path, k, rc, r, s)
        assert cands > sites > 10 and min(w0, w63, g0, g255) > 0, (k, rc, r, s, cands, sites, w0, w63, g0, g255)


def test_call_arithmetic_under_sanitizers(tmp_path):
    """the same program under AddressSanitizer and UBSan, over an LDS reference and the wide one"""
    exe = _check_tool(tmp_path, True)
    for k, rc, r, s, cut in ((41, False, 8, 0, None), (63, True, WIDE, 7, 1600)):  # (the first 1 600 bases of the wide copy: ~30 sites)
        cands, sites = _run_tool(exe, tmp_path, k, rc, r, s, cut)[:2]
        assert cands >= sites > 2
