"""The wide route of a reference set (kbo_refset_build_wide, kbo_hip.h "find against a set of references"): references of more than
KBO_REFSET_MAX_ROWS rows walked from memory by refset_wide_kernels.hip, in the same slabs as the references of the LDS kernel -
through kbo_find_refset / kbo_summary_refset and through their device-resident forms - against the oracle.

Expected value of every (reference r, sequence s, strand): oracle.run_lengths_gapped(oracle.Index.build([ref_r], k, rc).matches(seq_s
or its reverse complement, made by numpy here), max_gap_len), and for the summary form the fold of those characters
(tests/test_gpu_refset_summary.py's, imported with the device helpers of tests/test_gpu_refset_dev.py) - one oracle index PER
REFERENCE; nothing comes from the library under test.  Compared as one list, so the order of the records is part of every comparison.

References, in this order so that the kinds alternate in every slab (L: LDS, W: wide): 1 200 bases (L), 16 384 bases = 16 385 rows
(W, the smallest), 300 (L), a length whose rows are a multiple of 32 (W), one whose rows + 1 are a multiple of 16 (L), 40 000 bases (W,
a form over 64 KiB), 70 000 bases (W, rows over 65 536), 20 bases (no k-mer: a status), 5 000 (L), one with N and lower-case
stretches (W), one over the letters A and T only (W: deep LCS structure, long scans).  The set is built with max_wide_rows = the rows
of the 70 000-base reference; for the host calls a second set holds a reference one base longer behind them, which takes the
single-index route.  A third world has add_revcomp = 1 and a reference of 8 200 bases: 16 401 rows, so wide.
Queries: a 30 kbp contig with copies of stretches of the references - substitutions, a deletion, an insertion, reverse complements,
one across a chunk cut; a 70 kbp contig that holds the whole 40 000-base reference - more than 256 chunks, so a reference has two
tasks and more, and a run across many chunk cuts with the depth at k; sequences of 3, 40, 257 and 511 bases; for the device form
sequences of 0, 1 and 2 bases in the middle as well (the host calls refuse those: they get the batch without them)."""
import numpy as np
import pytest

import kbo_amd
from kbo_amd import refset
from oracle import binding as ora

import test_gpu_refset_dev as dev
from gpu_helpers import Guarded
from test_gpu_refset_dev import ACGT, COMP, _as_words, _mutate, _rnd, _tuples

pytestmark = pytest.mark.gpu

CHUNK, MAX_ROWS = 256, 16384  # KBO_REFSET_CHUNK, KBO_REFSET_MAX_ROWS (tests/test_refset_host.py pins them to the header)
L_, W_, I_, NONE_ = refset.ROUTE_LDS, refset.ROUTE_WIDE, refset.ROUTE_INDEX, refset.ROUTE_NONE
KINDS = [L_, W_, L_, W_, L_, W_, W_, NONE_, L_, W_, W_]
ALL = 0  # refs_per_slab: as many as a slab may hold


def _shapes(k):
    rng = np.random.default_rng(3000 + k)
    lens = [1200, 16384, 300, 20479, 4094, 40000, 70000, 20, 5000, 25000]
    refs = [_rnd(rng, n) for n in lens]
    refs[9][8000:8003] = ord("N")
    refs[9][15000:15050] += 32  # lower case: no bases
    refs[9][20000] = ord("N")
    refs.append(ACGT[[0, 3]][rng.integers(0, 2, 30000)].copy())
    refs.append(np.concatenate([refs[6], _rnd(rng, 1)]))  # one base longer than the largest wide one: the single-index route
    cut = max(CHUNK, 4 * k)
    big = _rnd(rng, 30000)

    def put(a, at, seq):
        a[at:at + len(seq)] = seq
    put(big, cut - 75, refs[2][:150])                                      # across the first chunk cut
    put(big, 1500, _mutate(rng, refs[1][2000:4000], 0.01))
    put(big, 4000, np.delete(refs[5][5000:7000], [700, 701]))
    put(big, 6500, np.insert(refs[6][10000:11500], 600, ACGT[[1, 2, 3]]))
    put(big, 8500, COMP[refs[6][66000:68000][::-1]])                       # rows over 65 536 are reached on the '-' strand too
    put(big, 11000, _mutate(rng, refs[0], 0.03))
    put(big, 12500, COMP[refs[3][100:1600][::-1]])
    put(big, 14500, refs[9][7000:9000])                                    # across the Ns of the reference
    put(big, 16800, refs[9][14500:15500])                                  # ... and its lower-case stretch
    put(big, 18000, _mutate(rng, refs[10][1000:3000], 0.01))
    put(big, 20500, refs[8][1000:3000])
    put(big, 23000, _mutate(rng, refs[4][500:2500], 0.01))
    put(big, 25500, refs[3][-1500:])
    put(big, 27500, COMP[refs[10][20000:21500][::-1]])
    put(big, 29000, COMP[refs[8][3000:3900][::-1]])
    big[26000] = ord("N")
    big[28000:28004] = np.frombuffer(b"acgt", dtype=np.uint8)
    huge = _rnd(rng, 70000)
    put(huge, 15000, refs[5])                                              # the whole 40 000-base reference: one run at depth k
    put(huge, 60000, COMP[refs[1][:3000][::-1]])
    put(huge, 64000, refs[6][-2500:])                                      # across 65 536
    seqs = [big, huge, refs[2][100:140].copy(), _rnd(rng, 0), _rnd(rng, 1), _rnd(rng, 2), _rnd(rng, 3), refs[6][500:757].copy(),
            _mutate(rng, refs[9][3000:3511], 0.01)]
    assert [len(s) for s in seqs] == [30000, 70000, 40, 0, 1, 2, 3, 257, 511]
    return refs, seqs


class WideWorld(dev.World):
    """tests/test_gpu_refset_dev.py's World - the batch on the device, the calls, the host calls with `seq` mapped back - over the
    references above.  rs: the packed-only set; rs_all: the same references and the one of the single-index route behind them"""

    def __init__(self, k, rc=False):
        self.k, self.rc = k, rc
        if rc:
            rng = np.random.default_rng(3500 + k)
            self.refs = [_rnd(rng, 300), _rnd(rng, 8200), _rnd(rng, 1200)]
            big = _rnd(rng, 6000)
            big[500:2500] = _mutate(rng, self.refs[1][3000:5000], 0.01)
            big[3000:4000] = COMP[self.refs[1][6000:7000][::-1]]
            big[4500:4800] = self.refs[0]
            self.seqs = [big, self.refs[2][200:240].copy(), _rnd(rng, 3)]
            self.kinds = [L_, W_, L_]
            cap = refset.WIDE_MAX_ROWS
        else:
            self.refs, self.seqs = _shapes(k)
            self.kinds = KINDS + [I_]
        self.aln, self.queryable, rows = {}, [], []
        for r, ref in enumerate(self.refs):
            oi = ora.Index.build([ref.tobytes()], k=k, add_revcomp=rc)
            rows.append(oi.n_sets)
            if oi.n_kmers == 0:
                continue
            self.queryable.append(r)
            seen = {}
            for s, q in enumerate(self.seqs):
                if len(q) < 3:  # no alignment (derandomize.rs:274-276): no record
                    continue
                for strand, text in ((1, q.tobytes()), (2, COMP[q[::-1]].tobytes())):
                    if text not in seen:
                        seen[text] = oi.matches(text, 1e-7)
                    self.aln[r, s, strand] = seen[text]
        self.rows = rows
        opts = kbo_amd.BuildOpts(k=k, add_revcomp=rc, num_threads=4)
        if rc:
            assert rows[1] == 16401
            self.n_packed = len(self.refs)
            self.rs = self.rs_all = refset.RefSet.build(self.refs, opts, wide_rows=cap)
        else:
            assert rows[1] == MAX_ROWS + 1 and rows[3] % 32 == 0 and rows[3] > MAX_ROWS and (rows[4] + 1) % 16 == 0 and rows[4] <= MAX_ROWS
            assert rows[5] * 2 > (1 << 16) and rows[6] > (1 << 16) and rows[11] == rows[6] + 1
            assert all(rows[r] > MAX_ROWS for r in (9, 10)) and all(rows[r] <= MAX_ROWS for r in (0, 2, 8))
            cap = rows[6]
            self.n_packed = len(self.refs) - 1
            self.rs = refset.RefSet.build(self.refs[:self.n_packed], opts, wide_rows=cap)
            self.rs_all = refset.RefSet.build(self.refs, opts, wide_rows=cap)
        for r, ref in enumerate(self.refs):
            assert self.rs_all.route(r) == self.kinds[r], r
            assert self.rs_all.status(r) == (0 if r in self.queryable else -4)
        assert [self.rs.route(r) for r in range(self.n_packed)] == self.kinds[:self.n_packed]
        assert self.rs.packed_only() and not self.rs.lds_only() and self.rs_all.packed_only() == bool(rc)
        self.n_seqs = len(self.seqs)
        self.offsets = np.zeros(self.n_seqs + 1, dtype=np.uint64)
        self.offsets[1:] = np.cumsum([len(s) for s in self.seqs])
        self.total = int(self.offsets[-1])
        self.kept = [s for s in range(self.n_seqs) if len(self.seqs[s]) >= 3]  # what the host calls accept
        self._exp, self._host = {}, {}
        self.device = None

    def expected(self, form, gap, strands, every=False):
        """the records of the packed-only set; every: those of the reference of the single-index route behind them as well"""
        base = dev.World.expected(self, form, gap, strands)
        return base if every else [t for t in base if t[0] < self.n_packed]

    def host(self, form, gap, strands, rs=None):
        rs = self.rs if rs is None else rs
        seqs = [self.seqs[s] for s in self.kept]
        if form == "find":
            rec = refset.find_refset(seqs, rs, kbo_amd.FindOpts(max_gap_len=gap), strands=strands)
        else:
            rec = refset.summary_refset(seqs, rs, strands=strands)
        rec["seq"] = np.asarray(self.kept, dtype=np.uint32)[rec["seq"]]
        return rec

    def host_packed(self, form, gap, strands):
        """the host call on the packed-only set, made once"""
        key = (form, gap, strands)
        if key not in self._host:
            self._host[key] = self.host(form, gap, strands)
        return self._host[key]

    def kind_count(self, kind, every):
        return sum(1 for r in self.queryable if self.kinds[r] == kind and (every or r < self.n_packed))


_cache = {}


def _oracle_world(k, rc=False):
    if (k, rc) not in _cache:
        _cache[k, rc] = WideWorld(k, rc)
    return _cache[k, rc]


def _world(k, rc=False):
    return _oracle_world(k, rc).on_device()


def test_the_fixtures_on_the_oracle_side():
    """no comparison below is of empty lists, the planted copies show, and the batch has the geometry the tasks were chosen for"""
    for k in (31, 96):
        w = _oracle_world(k)
        exp = w.expected("find", 0, 3, every=True)
        for r in w.queryable:
            assert [t for t in exp if t[0] == r], r
        for strand in (1, 2):
            assert [t for t in exp if t[2] == strand and w.kinds[t[0]] == W_] and [t for t in exp if t[2] == strand and w.kinds[t[0]] == L_]
        # the whole 40 000-base reference is ONE run of the 70 kbp contig, across more than a hundred chunk cuts
        assert [t for t in exp if t[:3] == (5, 1, 1) and t[3] <= 15000 and t[4] >= 55000 - 1]
        assert [t for t in exp if t[:3] == (6, 0, 2)] and [t for t in exp if t[:3] == (6, 1, 1) and t[3] < 65536 < t[4]]
        assert {t[1] for t in exp} >= ({0, 1, 2, 7, 8} if k == 31 else {0, 1, 7}) and not [t for t in exp if len(w.seqs[t[1]]) < 3]
        cut = max(CHUNK, 4 * k)
        if k == 31:
            assert sum(-(-len(s) // cut) for s in w.seqs) > 256, "a second task per reference"
        assert w.expected("summary", 0, 3) and len(w.expected("summary", 0, 3)) < len(w.expected("find", 0, 3))
    w = _oracle_world(31, True)
    assert [t for t in w.expected("find", 0, 3) if t[0] == 1 and t[2] == 1] and [t for t in w.expected("find", 0, 3) if t[0] == 1 and t[2] == 2]


def _planted(strands):
    """pairs with a planted copy, so records at least: ten references have one on the '+' strand, five (1, 3, 6, 8, 10) on the '-'"""
    return (10 if strands & 1 else 0) + (5 if strands & 2 else 0)


def _assert_routes(w, strands, every):
    n_strands = 2 if strands == 3 else 1
    n_lds, n_wide, n_own = w.kind_count(L_, every), w.kind_count(W_, every), w.kind_count(I_, every)
    routes, wide = refset.last_routes(), refset.last_wide()
    assert routes[:3] == (n_lds, n_own, (n_lds + n_wide + n_own) * len(w.kept) * n_strands) and routes[3] >= 1
    assert wide[0] == n_wide  # (the tasks, wide[1], are pinned for the one-slab call in test_all_three_routes_were_reached)
    return n_lds, n_wide, n_own


@pytest.mark.parametrize("strands", [1, 2, 3])
@pytest.mark.parametrize("gap", [0, 5])
@pytest.mark.parametrize("k", [31, 96])
def test_find_refset_equals_one_oracle_index_per_reference(k, gap, strands):
    w = _world(k)
    exp = w.expected("find", gap, strands, every=True)
    got = _tuples(w.host("find", gap, strands, w.rs_all))
    assert len(exp) >= _planted(strands) and got == exp
    assert _assert_routes(w, strands, True) == (4, 6, 1)
    # the packed-only set: the same records without the last reference's
    assert _tuples(w.host("find", gap, strands)) == w.expected("find", gap, strands)
    assert _assert_routes(w, strands, False) == (4, 6, 0)


@pytest.mark.parametrize("strands", [1, 2, 3])
@pytest.mark.parametrize("k", [31, 96])
def test_summary_refset_equals_the_fold_of_the_oracles_characters(k, strands):
    w = _world(k)
    exp = w.expected("summary", 0, strands, every=True)
    got = _tuples(w.host("summary", 0, strands, w.rs_all))
    assert len(exp) >= _planted(strands) and got == exp and all(t[6] > 0 for t in got)
    assert _assert_routes(w, strands, True) == (4, 6, 1)
    assert _tuples(w.host("summary", 0, strands)) == w.expected("summary", 0, strands)


@pytest.mark.parametrize("form", ["find", "summary"])
def test_a_set_with_reverse_complements_in_the_indexes(form):
    w = _world(31, True)
    exp = w.expected(form, 0, 3)
    assert len(exp) >= 4 and _tuples(w.host(form, 0, 3)) == exp
    assert refset.last_routes()[:2] == (2, 0) and refset.last_wide()[0] == 1
    n, got = w.run(form, 0, 3, ALL, len(exp) + 5)
    assert n == len(exp) and _tuples(got) == exp


@pytest.mark.parametrize("k", [31, 96])
def test_the_wide_walk_against_the_single_index_route(k):
    """the same references built by kbo_refset_build: every one of more than KBO_REFSET_MAX_ROWS rows goes through the single-index
    pipeline there - the records are the same bytes"""
    w = _world(k)
    plain = refset.RefSet.build(w.refs, kbo_amd.BuildOpts(k=k, num_threads=4))
    assert [plain.route(r) for r in range(len(w.refs))] == [I_ if kind == W_ else kind for kind in w.kinds]
    for form, gap in (("find", 5), ("summary", 0)):
        a = w.host(form, gap, 3, plain)
        assert refset.last_routes()[:2] == (4, 7) and refset.last_wide() == (0, 0)
        b = w.host(form, gap, 3, w.rs_all)
        assert len(a) >= _planted(3) and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def test_slabs_of_the_smallest_budget_mix_the_kinds():
    """64 KiB of pair bytes a slab: every reference's pairs spread over several slabs, and a slab holds the end of one reference's
    pairs and the start of the next one's - an LDS and a wide reference next to each other"""
    w = _world(31)
    base = w.host("find", 5, 3)
    one = refset.last_routes()[3]
    L = kbo_amd.lib()
    L.kbo_set_slab_bytes(1 << 16)
    try:
        again = w.host("find", 5, 3)
        many = refset.last_routes()[3]
        assert refset.last_routes()[0] == 4 and refset.last_wide()[0] == 6
    finally:
        L.kbo_set_slab_bytes(16 << 20)
    assert len(base) >= _planted(3) and np.array_equal(base, again)
    assert many >= 20 and many > one


def _run_guarded(w, form, gap, strands, refs_per_slab, capacity):
    """the device call twice, over differently patterned scratch and output: d_work of exactly the figure and the records of exactly
    `capacity` between guard bands that stay intact -> (count, the first min(count, capacity) records as an (n, words) uint32 array)"""
    import torch
    words = 10 if form == "find" else 9
    wb = w.work_bytes(form, strands, capacity, refs_per_slab)
    assert wb > 0
    work = Guarded("d_work", wb, 1 << 20, w.device, seed=1)
    out = Guarded("records", capacity * words * 4, 1 << 16, w.device, seed=2)
    count = torch.full((1,), -1, dtype=torch.int64, device=w.device)
    s = torch.cuda.current_stream(w.device)
    res = []
    for seed in (3, 4):
        kbo_amd.check(w.enqueue(form, gap, strands, work.ptr, wb, out.ptr if capacity else None, capacity, count.data_ptr(), s.cuda_stream))
        torch.cuda.synchronize()
        work.assert_intact(form)
        out.assert_intact(form)
        n = int(count.item())
        res.append((n, out.host().view(np.uint32).reshape(capacity, words)[:min(n, capacity)].copy()))
        work.fill(seed)
        out.fill(seed + 10)
        count.fill_(seed)
    assert res[0][0] == res[1][0] and np.array_equal(res[0][1], res[1][1])
    return res[0]


@pytest.mark.parametrize("refs_per_slab", [1, 3, ALL])
@pytest.mark.parametrize("gap,strands", [(5, 1), (5, 2), (5, 3), (0, 3)])
@pytest.mark.parametrize("k", [31, 96])
def test_find_refset_dev_on_a_packed_only_set(k, gap, strands, refs_per_slab):
    """1 a slab: all-LDS and all-wide slabs; 3 a slab: (L W L) (W L W) (W L W) (W); all: one mixed slab"""
    w = _world(k)
    exp = w.expected("find", gap, strands)
    n, got = _run_guarded(w, "find", gap, strands, refs_per_slab, len(exp))  # capacity: exactly the records there are
    assert n == len(exp) >= _planted(strands) and _tuples(got) == exp
    assert np.array_equal(got, _as_words(w.host_packed("find", gap, strands)))


@pytest.mark.parametrize("refs_per_slab", [1, 3, ALL])
@pytest.mark.parametrize("strands", [1, 2, 3])
@pytest.mark.parametrize("k", [31, 96])
def test_summary_refset_dev_on_a_packed_only_set(k, strands, refs_per_slab):
    w = _world(k)
    exp = w.expected("summary", 0, strands)
    n, got = _run_guarded(w, "summary", 0, strands, refs_per_slab, len(exp))
    assert n == len(exp) >= _planted(strands) and _tuples(got) == exp
    assert np.array_equal(got, _as_words(w.host_packed("summary", 0, strands)))


@pytest.mark.parametrize("form", ["find", "summary"])
def test_capacity_one_below_the_records(form):
    """the count is the full number, the written prefix is exact, nothing is written at or behind element `capacity`"""
    w = _world(31)
    exp = w.expected(form, 5, 3)
    n, got = _run_guarded(w, form, 5, 3, 3, len(exp) - 1)
    assert n == len(exp) and _tuples(got) == exp[:-1]


@pytest.mark.parametrize("form", ["find", "summary"])
def test_the_device_form_still_refuses_the_single_index_route(form):
    import torch
    w = _world(31)
    w.rs_all.to_device()
    assert w.work_bytes(form, 3, 100, 1) > 0
    L = kbo_amd.lib()
    wb_fn = L.kbo_find_refset_dev_work_bytes if form == "find" else L.kbo_summary_refset_dev_work_bytes
    assert wb_fn(w.rs_all._h, w.n_seqs, w.total, 3, 100, 1) == 0
    rs, w.rs = w.rs, w.rs_all
    try:
        work = torch.empty(1 << 20, dtype=torch.int64, device=w.device)
        out = torch.empty((100, 10), dtype=torch.int32, device=w.device)
        count = torch.full((1,), 77, dtype=torch.int64, device=w.device)
        s = torch.cuda.current_stream(w.device)
        assert w.enqueue(form, 0, 3, work.data_ptr(), 8 << 20, out.data_ptr(), 100, count.data_ptr(), s.cuda_stream) == -8
        torch.cuda.synchronize()
        assert int(count.item()) == 77  # nothing was enqueued
    finally:
        w.rs = rs


def test_the_python_wrappers():
    import torch
    w = _world(31)
    exp = w.expected("find", 5, 3)
    rec, count = refset.find_refset_dev(w.d_q, w.d_off, w.rs, kbo_amd.FindOpts(max_gap_len=5), capacity=len(exp) + 10, refs_per_slab=4)
    torch.cuda.synchronize()
    assert int(count.item()) == len(exp) and _tuples(rec[:len(exp)].cpu().numpy().view(np.uint32)) == exp
    exp = w.expected("summary", 0, 2)
    rec, count = refset.summary_refset_dev(w.d_q, w.d_off, w.rs, strands=refset.STRAND_REV)
    torch.cuda.synchronize()
    assert int(count.item()) == len(exp) and _tuples(rec[:len(exp)].cpu().numpy().view(np.uint32)) == exp


def test_all_three_routes_were_reached():
    """the LDS kernel, the wide kernel and the single-index pipeline in one call, each for exactly its references"""
    for k in (31, 96):
        w = _world(k)
        w.host("find", 0, 1, w.rs_all)
        lds, own, pairs, slabs = refset.last_routes()
        wide, tasks = refset.last_wide()
        assert (lds, wide, own) == (4, 6, 1) and lds + wide + own == len(w.queryable)
        assert pairs == len(w.queryable) * len(w.kept)
        # one slab holds every pair of this call (about 1 MB of the 16 MiB a slab may hold), so the wide kernel was launched once, with
        # the slab's whole task list: a task per 256 chunks of each walked reference, the LDS references' included
        cut = max(CHUNK, 4 * k)
        chunks = sum(-(-len(w.seqs[s]) // cut) for s in w.kept)
        assert slabs == 1 and tasks == (lds + wide) * -(-chunks // 256)
        assert [w.rs_all.route(r) for r in range(len(w.refs))] == w.kinds
