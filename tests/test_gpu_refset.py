"""kbo_find_refset (kbo_hip.h "find against a set of references") against the oracle.

Expected value of every (reference r, sequence s, strand): oracle.run_lengths_gapped(oracle.Index.build([ref_r], k, rc).matches(seq_s
or its reverse complement, made by numpy here), max_gap_len) - one oracle index PER REFERENCE, as the reference crate's callers
build them; nothing comes from the library under test.  Compared as one list, field by field, so the order of the records -
(ref, seq, strand with '+' first, start) - is part of every comparison.

Shapes: references of k - 1 bases (no k-mer: status set, no record), k, 40, 300, 1 500, one with an N in the middle, two
identical ones, a spread of other lengths, one of 16 300 bases (the largest LDS form) and one of 16 400 bases whose index has
16 401 rows, just over KBO_REFSET_MAX_ROWS = 16 384: it takes the single-index pipeline.  Queries: a 30 kbp contig with copies of
references at 0 / 1 / 3 % substitutions, one with a 2-base deletion, one as its reverse complement, and a copy across each of the
first three chunk cuts (every max(KBO_REFSET_CHUNK, 4 k) bases); a 40-base and a 3-base contig; a contig with Ns; an unrelated
one."""
import numpy as np
import pytest

import kbo_amd
from kbo_amd import batch, refset
from oracle import binding as ora

pytestmark = pytest.mark.gpu

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
COMP = np.arange(256, dtype=np.uint8)
for _a, _b in zip(b"ACGT", b"TGCA"):
    COMP[_a] = _b
CHUNK, MAX_ROWS = 256, 16384  # KBO_REFSET_CHUNK, KBO_REFSET_MAX_ROWS (tests/test_refset_host.py pins them to the header)
DEFAULT_SLAB = 16 << 20
UNRELATED_REF, UNRELATED_SEQ = 9, 4


def _rnd(rng, n):
    return ACGT[rng.integers(0, 4, n)].copy()


def _mutate(rng, a, rate):
    a = a.copy()
    pos = np.flatnonzero(rng.random(len(a)) < rate)
    a[pos] = ACGT[(np.searchsorted(ACGT, a[pos]) + rng.integers(1, 4, len(pos))) % 4]
    return a


def _shapes(k):
    rng = np.random.default_rng(1000 + k)
    lens = [k - 1, k, 40, 300, 1500, 200, 300, 300, 97, 333, 700, 1000, 2000, 3000, 5000, 64, 128, 257, 511, 1200, 800, 450, 999, 2500,
            16300, 16400]
    refs = [_rnd(rng, n) for n in lens]
    refs[5][100] = ord("N")
    refs[7] = refs[6].copy()
    cut = max(CHUNK, 4 * k)
    big = _rnd(rng, 30000)

    def put(at, a):
        big[at:at + len(a)] = a
    for i, r in enumerate((3, 9, 10)):  # across the first three chunk cuts
        put((i + 1) * cut - 75, refs[r][:150])
    put(5000, refs[4])
    put(8000, _mutate(rng, refs[11], 0.01))
    put(10000, _mutate(rng, refs[12], 0.03))
    put(13000, np.delete(refs[13], [1500, 1501]))
    put(17000, COMP[refs[19][::-1]])
    put(19000, _mutate(rng, refs[25][:5000], 0.01))
    put(25000, refs[24][2000:5000])
    with_n = _mutate(rng, refs[4], 0.01)
    with_n[[200, 201, 900]] = ord("N")
    seqs = [big, refs[2].copy(), _rnd(rng, 3), np.concatenate([_rnd(rng, 300), with_n, _rnd(rng, 200)]), _rnd(rng, 500)]
    return refs, seqs


_cache = {}


def _world(k, rc=False):
    """references, query sequences, the set under test and the oracle's alignment of every pair - made once per (k, rc)"""
    if (k, rc) not in _cache:
        refs, seqs = _shapes(k)
        rs = refset.RefSet.build(refs, kbo_amd.BuildOpts(k=k, add_revcomp=rc, num_threads=4))
        aln, n_fit, n_own = {}, 0, 0
        for r, ref in enumerate(refs):
            oi = ora.Index.build([ref.tobytes()], k=k, add_revcomp=rc)
            assert rs.n_kmers(r) == oi.n_kmers
            if oi.n_kmers == 0:
                assert rs.status(r) != 0
                continue
            assert rs.status(r) == 0
            n_fit += oi.n_sets <= MAX_ROWS
            n_own += oi.n_sets > MAX_ROWS
            for s, q in enumerate(seqs):
                aln[r, s, 1] = oi.matches(q.tobytes(), 1e-7)
                aln[r, s, 2] = oi.matches(COMP[q[::-1]].tobytes(), 1e-7)
        _cache[k, rc] = (refs, seqs, rs, aln, n_fit, n_own)
    return _cache[k, rc]


def _expected(k, rc, gap, strands):
    refs, seqs, _, aln, _, _ = _world(k, rc)
    out = []
    for r in range(len(refs)):
        for s in range(len(seqs)):
            for strand in (1, 2):
                if strands & strand and (r, s, strand) in aln:
                    out += [(r, s, strand) + t for t in ora.run_lengths_gapped(aln[r, s, strand], gap)]
    return out


def _tuples(rec):
    return [tuple(int(v) for v in row) for row in rec.tolist()]


def _find(k, rc, gap, strands):
    _, seqs, rs, _, _, _ = _world(k, rc)
    return refset.find_refset(seqs, rs, kbo_amd.FindOpts(max_gap_len=gap), strands=strands)


@pytest.mark.parametrize("strands", [1, 2, 3])
@pytest.mark.parametrize("gap", [0, 5])
@pytest.mark.parametrize("k", [31, 96])
def test_find_refset_equals_one_oracle_index_per_reference(k, gap, strands):
    refs, seqs, rs, aln, n_fit, n_own = _world(k)
    got = _tuples(_find(k, False, gap, strands))
    exp = _expected(k, False, gap, strands)
    # (the comparison is not of two empty lists: ten copies lie on the '+' strand, the reverse-complemented one on the '-' strand)
    assert len(exp) >= (10 if strands & 1 else 0) + (1 if strands & 2 else 0)
    assert got == exp
    n_strands = 2 if strands == 3 else 1
    routes = refset.last_routes()
    assert routes[:3] == (n_fit, n_own, (n_fit + n_own) * len(seqs) * n_strands) and n_own == 1 and n_fit >= 22
    # no record of a reference without a k-mer, none of an unrelated pair; the neighbours of both have theirs
    assert rs.status(0) != 0 and not [t for t in got if t[0] == 0]
    assert not [t for t in got if t[0] == UNRELATED_REF and t[1] == UNRELATED_SEQ]
    assert [t for t in got if t[0] == 1 or t[0] == 3] == [t for t in exp if t[0] == 1 or t[0] == 3]


def test_find_refset_with_reverse_complements_in_the_indexes():
    got = _tuples(_find(31, True, 0, 3))
    assert got == _expected(31, True, 0, 3) and len(got) > 20
    _, _, _, _, n_fit, n_own = _world(31, True)
    assert refset.last_routes()[:2] == (n_fit, n_own) and n_own == 2  # (twice the rows: the 16 300-base reference no longer fits)


def test_record_buffer_grows_from_one_record():
    base = _find(31, False, 5, 3)
    L = kbo_amd.lib()
    L.kbo_set_refset_record_capacity(1)
    try:
        again = _find(31, False, 5, 3)
    finally:
        L.kbo_set_refset_record_capacity(1 << 16)
    assert len(base) > 20 and np.array_equal(base, again)


def test_slabs_of_the_smallest_budget():
    """64 KiB of pair bytes a slab: a 30 kbp contig in both strands fills one, so every reference's pairs spread over several"""
    base = _find(31, False, 0, 3)
    one = refset.last_routes()[3]
    L = kbo_amd.lib()
    L.kbo_set_slab_bytes(1 << 16)
    try:
        again = _find(31, False, 0, 3)
        many = refset.last_routes()[3]
    finally:
        L.kbo_set_slab_bytes(DEFAULT_SLAB)
    assert np.array_equal(base, again)
    assert many >= 20 and many > one


def test_against_find_batch_strands_on_single_handles():
    """without the oracle: kbo_find_batch_strands on a handle kbo_index_build made of that reference alone"""
    refs, seqs, rs, _, _, _ = _world(31)
    got = _tuples(_find(31, False, 5, 3))
    concat = np.concatenate(seqs)
    offsets = np.zeros(len(seqs) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(s) for s in seqs])
    for r in (4, 13, 25):
        sbwt, _ = kbo_amd.build([refs[r]], kbo_amd.BuildOpts(k=31))
        rles, ro = batch.find_batch_strands(sbwt, concat, offsets, kbo_amd.FindOpts(max_gap_len=5), strands=3)
        exp = []
        for s in range(len(seqs)):
            for strand in (1, 2):
                a, b = int(ro[2 * s + strand - 1]), int(ro[2 * s + strand])
                exp += [(r, s, strand) + tuple(int(v) for v in row) for row in rles[a:b].tolist()]
        assert exp and [t for t in got if t[0] == r] == exp


def test_both_routes_were_reached():
    """the LDS kernel for every reference that fits its form, the single-index pipeline for the one that does not"""
    for k in (31, 96):
        refs, seqs, rs, _, n_fit, n_own = _world(k)
        _find(k, False, 0, 1)
        lds, own, pairs, slabs = refset.last_routes()
        assert lds == n_fit and own == n_own == 1 and lds + own == sum(rs.status(r) == 0 for r in range(len(refs)))
        assert pairs == (lds + own) * len(seqs) and slabs >= 1


def test_a_contig_of_more_than_65536_bases():
    """the derandomize / translate stage takes a sequence above 65 536 bases with its chunked scan, one chain of launches per pair:
    a 70 kbp contig with copies in front of, across and behind that length, both strands"""
    rng = np.random.default_rng(77)
    refs = [_rnd(rng, n) for n in (300, 1500, 2500)]
    big = _rnd(rng, 70000)
    big[100:400] = refs[0]
    big[40000:41500] = _mutate(rng, refs[1], 0.01)
    big[64500:67000] = refs[2]
    big[68000:68300] = COMP[refs[0][::-1]]
    seqs = [big, _rnd(rng, 200)]
    rs = refset.RefSet.build(refs, kbo_amd.BuildOpts(k=31))
    got = _tuples(refset.find_refset(seqs, rs, kbo_amd.FindOpts(max_gap_len=5), strands=3))
    exp = []
    for r, ref in enumerate(refs):
        oi = ora.Index.build([ref.tobytes()], k=31)
        for s, q in enumerate(seqs):
            for strand, text in ((1, q), (2, COMP[q[::-1]])):
                exp += [(r, s, strand) + t for t in ora.run_lengths_gapped(oi.matches(text.tobytes(), 1e-7), 5)]
    assert len(exp) >= 4 and got == exp
    assert refset.last_routes()[:3] == (3, 0, 12)
