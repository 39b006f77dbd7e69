"""kbo_best_refset / kbo_best_refset_dev (kbo_hip.h "find against a set of references": the best reference per sequence) against the
oracle.

Expected record of every sequence: the fold, in numpy here, of oracle.Index.build([ref_r], k, rc).matches(seq_s or its reverse
complement, made by numpy here) for every reference r - one oracle index PER REFERENCE - reduced in Python by SORTING the pairs with a
hit by (larger n_match, smaller ref, '+' first): the first pair, the number of pairs, the first pair of another reference.  Nothing
comes from the library under test, and not from summary_refset either; one test ties the two calls together.

The world is that of tests/test_gpu_refset_summary.py, restated (its _shapes, fold and _world), with two sequences behind its five: a
copy of reference 6, which reference 7 is identical to - a tie across references - and the reverse complement of reference 19 - a
best pair on the '-' strand.  26 references of k - 1 to 16 400 bases (one with a status, one with an N, one of the single-index
route); a 30 kbp contig with planted copies across chunk cuts, a 40-base copy, a 3-base sequence, a contig with Ns, an unrelated
one.  Seven sequences are fewer than 64: refset_best_kernel runs a workgroup per sequence.  A second world - 200 sequences of 40 to
300 bases against 8 references - runs a wave per sequence."""
import numpy as np
import pytest

import kbo_amd
from kbo_amd import refset
from oracle import binding as ora

from gpu_helpers import Guarded

pytestmark = pytest.mark.gpu

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
COMP = np.arange(256, dtype=np.uint8)
for _a, _b in zip(b"ACGT", b"TGCA"):
    COMP[_a] = _b
CHUNK, MAX_ROWS = 256, 16384  # KBO_REFSET_CHUNK, KBO_REFSET_MAX_ROWS (tests/test_refset_host.py pins them to the header)
DEFAULT_SLAB = 16 << 20
BIG_REF = 25  # the 16 400-base reference
NONE = 0xFFFFFFFF
E_BAD_ARG = -4
TWIN_SEQ, REV_SEQ, SHORT_SEQ, UNRELATED_SEQ = 5, 6, 2, 4
ALL = 0  # refs_per_slab: as many as a slab may hold


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
    seqs += [refs[6].copy(), COMP[refs[19][::-1]].copy()]  # (behind the five: the draws above are the summary test's)
    return refs, seqs


def fold(text):
    """kbo_aln_extent of one pair's characters"""
    chars = np.frombuffer(text.encode() if isinstance(text, str) else bytes(text), dtype=np.uint8)
    hit = chars != ord("-")
    starts = hit & ~np.concatenate([[False], hit[:-1]])
    at = np.flatnonzero(hit)
    return (int((chars == ord("M")).sum()), int((chars == ord("X")).sum()), int((chars == ord("R")).sum()), int(starts.sum()),
            int(at[0]) if len(at) else 0, int(at[-1]) + 1 if len(at) else 0)


def _extents(refs, seqs, k, rc, rs):
    """(r, s, strand) -> the fold of the oracle's alignment, for every reference with a k-mer; rows of every such reference"""
    ext, rows = {}, {}
    for r, ref in enumerate(refs):
        oi = ora.Index.build([ref.tobytes()], k=k, add_revcomp=rc)
        if oi.n_kmers == 0:
            assert rs.status(r) != 0
            continue
        assert rs.status(r) == 0
        rows[r] = oi.n_sets
        for s, q in enumerate(seqs):
            ext[r, s, 1] = fold(oi.matches(q.tobytes(), 1e-7))
            ext[r, s, 2] = fold(oi.matches(COMP[q[::-1]].tobytes(), 1e-7))
    return ext, rows


_cache = {}


def _world(k, rc=False):
    """references, query sequences, the set under test and the fold of the oracle's alignment of every pair - made once per (k, rc)"""
    if (k, rc) not in _cache:
        refs, seqs = _shapes(k)
        rs = refset.RefSet.build(refs, kbo_amd.BuildOpts(k=k, add_revcomp=rc, num_threads=4))
        ext, rows = _extents(refs, seqs, k, rc, rs)
        n_fit = sum(1 for n in rows.values() if n <= MAX_ROWS)
        _cache[k, rc] = (refs, seqs, rs, ext, n_fit, len(rows) - n_fit)
    return _cache[k, rc]


def _pairs_with_a_hit(ext, n_refs, n_seqs, strands):
    """summary_refset's records, from the oracle: (ref, seq, strand) + extent of every pair with a run, in its order"""
    out = []
    for r in range(n_refs):
        for s in range(n_seqs):
            for strand in (1, 2):
                if strands & strand and (r, s, strand) in ext and ext[r, s, strand][3] > 0:
                    out.append((r, s, strand) + ext[r, s, strand])
    return out


def reduce_best(n_seqs, records):
    """kbo_ref_best of every sequence from records (ref, seq, strand, n_match, n_mismatch, n_jump, n_runs, start, end), by sorting"""
    out = []
    for s in range(n_seqs):
        mine = sorted((t for t in records if t[1] == s), key=lambda t: (-t[3], t[0], t[2]))
        if not mine:
            out.append((s, NONE, 0, 0, 0, 0, 0, 0, 0, 0, NONE, 0))
            continue
        first = mine[0]
        others = [t for t in mine if t[0] != first[0]]
        out.append((s, first[0], first[2]) + tuple(first[3:9]) + (len(mine), others[0][0] if others else NONE, others[0][3] if others else 0))
    return out


def _expected(k, rc, strands):
    refs, seqs, _, ext, _, _ = _world(k, rc)
    return reduce_best(len(seqs), _pairs_with_a_hit(ext, len(refs), len(seqs), strands))


def _tuples(rec):
    return [tuple(int(v) for v in row) for row in rec.tolist()]


def _best(seqs, rs, strands):
    got = refset.best_refset(seqs, rs, strands=strands)
    assert got.dtype == refset.REF_BEST and len(got) == len(seqs)
    return got


def _check_the_expectation(exp, strands):
    """what the comparison must hold, asserted on the oracle's side: a change of shapes cannot empty the test"""
    REF, STRAND, MATCH, HITS, SECOND, SECOND_MATCH = 1, 2, 3, 9, 10, 11
    for s in (SHORT_SEQ, UNRELATED_SEQ):
        assert exp[s] == (s, NONE, 0, 0, 0, 0, 0, 0, 0, 0, NONE, 0)
    if strands & 1:  # the copy of references 6 = 7: the lower one wins, the other one ties
        twin = exp[TWIN_SEQ]
        assert twin[REF] == 6 and twin[STRAND] == 1 and twin[SECOND] == 7 and twin[SECOND_MATCH] == twin[MATCH] > 0
        assert [t for t in exp if BIG_REF in (t[REF], t[SECOND])], "the reference of the single-index route is merged on the host"
    if strands & 2:
        assert exp[REV_SEQ][REF] == 19 and exp[REV_SEQ][STRAND] == 2 and exp[REV_SEQ][MATCH] > 0
    if strands & 1:  # (on the '-' strand alone the contig meets one reference)
        assert [t for t in exp if t[SECOND] != NONE and t[SECOND_MATCH] < t[MATCH]]
    assert [t for t in exp if t[REF] != NONE and t[SECOND] == NONE and t[SECOND_MATCH] == 0], "only one reference hit"
    if strands == 3:
        assert [t for t in exp if t[HITS] > 2] and exp[REV_SEQ][STRAND] == 2 and exp[0][STRAND] == 1


@pytest.mark.parametrize("strands", [1, 2, 3])
@pytest.mark.parametrize("k", [31, 96])
def test_best_refset_equals_the_sorted_pairs_of_one_oracle_index_per_reference(k, strands):
    refs, seqs, rs, ext, n_fit, n_own = _world(k)
    exp = _expected(k, False, strands)
    _check_the_expectation(exp, strands)
    got = _tuples(_best(seqs, rs, strands))
    assert got == exp
    n_strands = 2 if strands == 3 else 1
    routes = refset.last_routes()
    assert routes[:3] == (n_fit, n_own, (n_fit + n_own) * len(seqs) * n_strands) and n_own == 1 and n_fit >= 22 and routes[3] >= 1
    assert refset.last_best() == (0, routes[3])  # fewer than 64 sequences: a workgroup per sequence, one launch a slab


def test_best_refset_with_reverse_complements_in_the_indexes():
    refs, seqs, rs, _, n_fit, n_own = _world(31, True)
    exp = _expected(31, True, 3)
    assert exp[TWIN_SEQ][1] == 6 and exp[TWIN_SEQ][10] == 7 and exp[REV_SEQ][1] == 19 and exp[REV_SEQ][2] == 1  # (both strands in the index: '+' first)
    assert _tuples(_best(seqs, rs, 3)) == exp
    assert refset.last_routes()[:2] == (n_fit, n_own) and n_own == 2  # (twice the rows: the 16 300-base reference no longer fits)


def test_slabs_of_the_smallest_budget():
    """64 KiB of pair bytes a slab: a 30 kbp contig in both strands fills one, so slabs begin and end in the middle of a reference"""
    _, seqs, rs, _, _, _ = _world(31)
    base = _best(seqs, rs, 3)
    one = refset.last_routes()[3]
    L = kbo_amd.lib()
    L.kbo_set_slab_bytes(1 << 16)
    try:
        again = _best(seqs, rs, 3)
        many = refset.last_routes()[3]
        launches = refset.last_best()
    finally:
        L.kbo_set_slab_bytes(DEFAULT_SLAB)
    assert _tuples(base) == _expected(31, False, 3)
    assert base.tobytes() == again.tobytes()
    assert many >= 20 and many > one >= 1 and launches == (0, many)


@pytest.mark.parametrize("strands", [1, 3])
def test_best_refset_is_the_reduction_of_summary_refsets_records(strands):
    _, seqs, rs, _, _, _ = _world(31)
    summ = refset.summary_refset(seqs, rs, strands=strands)
    assert len(summ) > 10
    assert _tuples(_best(seqs, rs, strands)) == reduce_best(len(seqs), _tuples(summ))


# ---- the device-resident form: the same references in a packed-only set - the 16 400-base one takes the wide route there


class Packed:
    def __init__(self, refs, seqs, k):
        import torch
        self.seqs = seqs
        self.rs = refset.RefSet.build(refs, kbo_amd.BuildOpts(k=k, num_threads=4), wide_rows=1 << 20).to_device()
        self.n_seqs = len(seqs)
        self.offsets = np.zeros(self.n_seqs + 1, dtype=np.uint64)
        self.offsets[1:] = np.cumsum([len(s) for s in seqs])
        self.total = int(self.offsets[-1])
        self.device = torch.device("cuda", torch.cuda.current_device())
        q = np.zeros(self.total + 16, dtype=np.uint8)
        q[:self.total] = np.concatenate(seqs)
        self.d_q = torch.from_numpy(q).to(self.device)
        self.d_off = torch.from_numpy(self.offsets.astype(np.int64)).to(self.device)
        self._host, self.routes = {}, {}

    def host(self, strands):
        """best_refset on the same set, made once; what the call reported: (references through the single-index pipeline, references
        walked by the wide kernel)"""
        if strands not in self._host:
            self._host[strands] = _best(self.seqs, self.rs, strands)
            self.routes[strands] = (refset.last_routes()[1], refset.last_wide()[0])
        return self._host[strands]

    def work_bytes(self, strands, refs_per_slab):
        return int(kbo_amd.lib().kbo_best_refset_dev_work_bytes(self.rs._h, self.n_seqs, self.total, strands, refs_per_slab))

    def enqueue(self, strands, work_ptr, work_bytes, out_ptr):
        import torch
        s = torch.cuda.current_stream(self.device)
        return kbo_amd.lib().kbo_best_refset_dev(self.rs._h, self.d_q.data_ptr(), self.d_off.data_ptr(), self.n_seqs, self.total, 1e-7, strands,
                                                 work_ptr, work_bytes, out_ptr, s.cuda_stream)

    def run_guarded(self, strands, refs_per_slab):
        """d_work of exactly the figure and d_out of exactly n_seqs records, each between guard bands -> the table as bytes"""
        import torch
        wb = self.work_bytes(strands, refs_per_slab)
        assert wb > 0 and wb % 16 == 0
        work = Guarded("d_work", wb, 4 << 20, self.device, seed=refs_per_slab)
        out = Guarded("d_out", self.n_seqs * 48, 1 << 20, self.device, seed=7)
        kbo_amd.check(self.enqueue(strands, work.ptr, wb, out.ptr))
        torch.cuda.synchronize()
        work.assert_intact("best")
        out.assert_intact("best")
        return out.host().tobytes()


def _packed(k=31):
    if ("packed", k) not in _cache:
        refs, seqs, _, _, _, _ = _world(k)
        _cache["packed", k] = Packed(refs, seqs, k)
    return _cache["packed", k]


@pytest.mark.parametrize("refs_per_slab", [1, 3, ALL])
@pytest.mark.parametrize("strands", [1, 3])
def test_best_refset_dev_equals_best_refset_on_a_packed_only_set(strands, refs_per_slab):
    p = _packed()
    routes = [p.rs.route(r) for r in range(len(p.rs))]
    assert p.rs.packed_only() and refset.ROUTE_LDS in routes and routes[BIG_REF] == refset.ROUTE_WIDE
    host = p.host(strands)
    assert _tuples(host) == _expected(31, False, strands)  # (the routes do not show in the records)
    assert p.routes[strands] == (0, 1)
    if refs_per_slab:
        assert p.work_bytes(strands, refs_per_slab) < p.work_bytes(strands, refs_per_slab + 1)  # (so the call cannot take a larger slab)
    assert p.run_guarded(strands, refs_per_slab) == host.tobytes()
    slabs = -(-25 // refs_per_slab) if refs_per_slab else 1  # (25 references can be queried)
    assert refset.last_best() == (0, slabs)


def test_work_one_byte_short_of_one_reference_a_slab_is_refused():
    import torch
    p = _packed()
    wb = p.work_bytes(3, 1)
    work = torch.empty(wb // 8 + 2, dtype=torch.int64, device=p.device)
    out = torch.full((p.n_seqs, 12), 77, dtype=torch.int32, device=p.device)
    assert p.enqueue(3, work.data_ptr(), wb - 1, out.data_ptr()) == E_BAD_ARG
    torch.cuda.synchronize()
    assert bool((out == 77).all())  # nothing was enqueued


def test_the_python_wrapper():
    import torch
    p = _packed()
    table = refset.best_refset_dev(p.d_q, p.d_off, p.rs, refs_per_slab=4)
    torch.cuda.synchronize()
    assert table.shape == (p.n_seqs, 12) and table.dtype == torch.int32
    assert table.cpu().numpy().tobytes() == p.host(3).tobytes()
    # the defaults, a batch tensor without slack behind its last base, one strand
    table = refset.best_refset_dev(p.d_q[:p.total], p.d_off, p.rs, strands=refset.STRAND_FWD)
    torch.cuda.synchronize()
    assert table.cpu().numpy().tobytes() == p.host(1).tobytes()


# ---- many short sequences: a wave per sequence


def _many():
    """200 sequences of 40 to 300 bases - stretches of the references as they are, with substitutions, reverse-complemented, and
    unrelated ones - against 8 references, two of them identical"""
    if "many" not in _cache:
        k = 31
        rng = np.random.default_rng(77)
        refs = [_rnd(rng, n) for n in (400, 650, 900, 1300, 2000, 400, 3000, 512)]
        refs[5] = refs[0].copy()
        seqs = []
        for i in range(200):
            n = int(rng.integers(40, 301))
            ref = refs[int(rng.integers(0, len(refs)))]
            at = int(rng.integers(0, len(ref) - n + 1))
            piece = ref[at:at + n]
            seqs.append([piece.copy(), _mutate(rng, piece, 0.02), COMP[piece[::-1]].copy(), _rnd(rng, n)][i % 4])
        rs = refset.RefSet.build(refs, kbo_amd.BuildOpts(k=k, num_threads=4))
        ext, rows = _extents(refs, seqs, k, False, rs)
        assert len(rows) == 8
        exp = reduce_best(len(seqs), _pairs_with_a_hit(ext, len(refs), len(seqs), 3))
        _cache["many"] = (refs, seqs, rs, exp)
    return _cache["many"]


def test_a_wave_per_sequence_for_many_short_sequences():
    refs, seqs, rs, exp = _many()
    assert len(seqs) == 200 and min(len(s) for s in seqs) >= 40 and max(len(s) for s in seqs) <= 300
    hit = [t for t in exp if t[1] != NONE]
    assert len(hit) >= 100 and len(exp) - len(hit) >= 20
    assert [t for t in hit if t[2] == 2] and [t for t in hit if t[1] == 0 and t[10] == 5 and t[11] == t[3]]  # '-' bests; the twins tie
    assert _tuples(_best(seqs, rs, 3)) == exp
    slabs = refset.last_routes()[3]
    assert refset.last_best() == (slabs, 0) and slabs >= 1
    # ... and with slabs that begin in the middle of a reference: 200 sequences on both strands are more than 64 KiB
    assert 2 * sum(len(s) for s in seqs) > (1 << 16)
    L = kbo_amd.lib()
    L.kbo_set_slab_bytes(1 << 16)
    try:
        again = _tuples(_best(seqs, rs, 3))
        cut = refset.last_best()
    finally:
        L.kbo_set_slab_bytes(DEFAULT_SLAB)
    assert again == exp and cut[0] >= 8 and cut[1] == 0
    # the device form takes the same mapping
    p = Packed(refs, seqs, 31)
    host = p.host(3).tobytes()
    assert p.run_guarded(3, 3) == host
    assert refset.last_best() == (3, 0)  # (8 references, 3 a slab)
