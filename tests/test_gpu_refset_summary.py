"""kbo_summary_refset (kbo_hip.h "find against a set of references": its summary form) against the oracle.

Expected record of every (reference r, sequence s, strand): the fold, in numpy here, of oracle.Index.build([ref_r], k, rc).matches(seq_s
or its reverse complement, made by numpy here) - one oracle index PER REFERENCE; pairs whose characters are all '-' are dropped.
Nothing comes from the library under test.  Compared as one list, so the order of the records - (ref, seq, strand with '+' first) -
is part of every comparison.

The world is that of tests/test_gpu_refset.py, restated: references of k - 1 bases (no k-mer: status set, no record), k, 40, 300,
1 500, one with an N in the middle, two identical ones, a spread of other lengths, one of 16 300 bases (the largest LDS form) and
one of 16 400 bases whose index has 16 401 rows, just over KBO_REFSET_MAX_ROWS = 16 384: it takes the single-index pipeline.
Queries: a 30 kbp contig with copies of references at 0 / 1 / 3 % substitutions, one with a 2-base deletion, one as its reverse
complement, and a copy across each of the first three chunk cuts (every max(KBO_REFSET_CHUNK, 4 k) bases); a 40-base and a 3-base
contig; a contig with Ns; an unrelated one."""
import numpy as np
import pytest

import kbo_amd
from kbo_amd import refset
from oracle import binding as ora

pytestmark = pytest.mark.gpu

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
COMP = np.arange(256, dtype=np.uint8)
for _a, _b in zip(b"ACGT", b"TGCA"):
    COMP[_a] = _b
CHUNK, MAX_ROWS = 256, 16384  # KBO_REFSET_CHUNK, KBO_REFSET_MAX_ROWS (tests/test_refset_host.py pins them to the header)
DEFAULT_SLAB = 16 << 20
BIG_REF = 25  # the 16 400-base reference


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


def fold(text):
    """kbo_aln_extent of one pair's characters"""
    chars = np.frombuffer(text.encode() if isinstance(text, str) else bytes(text), dtype=np.uint8)
    hit = chars != ord("-")
    starts = hit & ~np.concatenate([[False], hit[:-1]])
    at = np.flatnonzero(hit)
    return (int((chars == ord("M")).sum()), int((chars == ord("X")).sum()), int((chars == ord("R")).sum()), int(starts.sum()),
            int(at[0]) if len(at) else 0, int(at[-1]) + 1 if len(at) else 0)


_cache = {}


def _world(k, rc=False):
    """references, query sequences, the set under test and the fold of the oracle's alignment of every pair - made once per (k, rc)"""
    if (k, rc) not in _cache:
        refs, seqs = _shapes(k)
        rs = refset.RefSet.build(refs, kbo_amd.BuildOpts(k=k, add_revcomp=rc, num_threads=4))
        ext, n_fit, n_own = {}, 0, 0
        for r, ref in enumerate(refs):
            oi = ora.Index.build([ref.tobytes()], k=k, add_revcomp=rc)
            if oi.n_kmers == 0:
                assert rs.status(r) != 0
                continue
            assert rs.status(r) == 0
            n_fit += oi.n_sets <= MAX_ROWS
            n_own += oi.n_sets > MAX_ROWS
            for s, q in enumerate(seqs):
                ext[r, s, 1] = fold(oi.matches(q.tobytes(), 1e-7))
                ext[r, s, 2] = fold(oi.matches(COMP[q[::-1]].tobytes(), 1e-7))
        _cache[k, rc] = (refs, seqs, rs, ext, n_fit, n_own)
    return _cache[k, rc]


def _expected(k, rc, strands):
    refs, seqs, _, ext, _, _ = _world(k, rc)
    out = []
    for r in range(len(refs)):
        for s in range(len(seqs)):
            for strand in (1, 2):
                if strands & strand and (r, s, strand) in ext and ext[r, s, strand][3] > 0:
                    out.append((r, s, strand) + ext[r, s, strand])
    return out


def _tuples(rec):
    return [tuple(int(v) for v in row) for row in rec.tolist()]


def _summary(k, rc, strands):
    _, seqs, rs, _, _, _ = _world(k, rc)
    got = refset.summary_refset(seqs, rs, strands=strands)
    assert got.dtype == refset.REF_SUMMARY
    return got


@pytest.mark.parametrize("strands", [1, 2, 3])
@pytest.mark.parametrize("k", [31, 96])
def test_summary_refset_equals_one_oracle_index_per_reference(k, strands):
    refs, seqs, rs, ext, n_fit, n_own = _world(k)
    exp = _expected(k, False, strands)
    for strand in (1, 2):  # the comparison is of lists that hold records on every strand asked for, and of the reference that does not fit
        assert not strands & strand or [t for t in exp if t[2] == strand]
    assert not strands & 1 or [t for t in exp if t[0] == BIG_REF]  # (its copy lies on the '+' strand)
    got = _tuples(_summary(k, False, strands))
    assert got == exp
    n_strands = 2 if strands == 3 else 1
    routes = refset.last_routes()
    assert routes[:3] == (n_fit, n_own, (n_fit + n_own) * len(seqs) * n_strands) and n_own == 1 and n_fit >= 22 and routes[3] >= 1
    assert rs.status(0) != 0 and not [t for t in got if t[0] == 0]


def test_summary_refset_with_reverse_complements_in_the_indexes():
    exp = _expected(31, True, 3)
    got = _tuples(_summary(31, True, 3))
    assert got == exp and len(got) > 10
    _, _, _, _, n_fit, n_own = _world(31, True)
    assert refset.last_routes()[:2] == (n_fit, n_own) and n_own == 2  # (twice the rows: the 16 300-base reference no longer fits)


@pytest.mark.parametrize("k", [31, 96])
def test_against_find_refset_without_gaps(k):
    """the returned records of both calls, grouped by pair: with max_gap_len = 0 a run is a maximal stretch without '-'"""
    _, seqs, rs, _, _, _ = _world(k)
    summ = _summary(k, False, 3)
    runs = refset.find_refset(seqs, rs, kbo_amd.FindOpts(max_gap_len=0), strands=3)
    by_pair = {}
    for t in runs.tolist():
        by_pair.setdefault(tuple(t[:3]), []).append(t[3:])
    assert len(summ) > 10 and sorted(by_pair) == [tuple(t[:3]) for t in summ.tolist()]
    for rec in summ:
        mine = by_pair[int(rec["ref"]), int(rec["seq"]), int(rec["strand"])]  # (start, end, matches, mismatches, jumps, ...)
        assert int(rec["n_runs"]) == len(mine)
        assert int(rec["n_match"]) + int(rec["n_jump"]) == sum(m[2] for m in mine)
        assert int(rec["n_mismatch"]) == sum(m[3] for m in mine)
        assert int(rec["start"]) == mine[0][0] and int(rec["end"]) == mine[-1][1]


def test_slabs_of_the_smallest_budget():
    """64 KiB of pair bytes a slab: a 30 kbp contig in both strands fills one, so every reference's pairs spread over several"""
    base = _summary(31, False, 3)
    one = refset.last_routes()[3]
    L = kbo_amd.lib()
    L.kbo_set_slab_bytes(1 << 16)
    try:
        again = _summary(31, False, 3)
        many = refset.last_routes()[3]
    finally:
        L.kbo_set_slab_bytes(DEFAULT_SLAB)
    assert len(base) > 10 and np.array_equal(base, again)
    assert many >= 20 and many > one >= 1


def test_unrelated_queries_give_no_record():
    _, _, rs, _, _, _ = _world(31)
    rng = np.random.default_rng(5)
    got = refset.summary_refset([_rnd(rng, 2000), _rnd(rng, 300), _rnd(rng, 3)], rs, strands=3)
    assert len(got) == 0 and got.dtype == refset.REF_SUMMARY


def test_a_copy_of_every_reference():
    refs, _, rs, _, _, _ = _world(31)
    got = refset.summary_refset([np.concatenate(refs)], rs, strands=1)
    buildable = [r for r in range(len(refs)) if rs.status(r) == 0]
    assert len(buildable) >= 24 and sorted(set(got["ref"].tolist())) == buildable
    assert (got["n_runs"] > 0).all() and (got["strand"] == 1).all() and (got["seq"] == 0).all()
