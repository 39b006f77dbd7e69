"""kbo_find_refset_dev / kbo_summary_refset_dev (kbo_hip.h "find against a set of references", the device-resident form) against the
oracle.

Expected value of every (reference r, sequence s, strand): oracle.run_lengths_gapped(oracle.Index.build([ref_r], k, rc).matches(seq_s
or its reverse complement, made by numpy here), max_gap_len), and for the summary form the fold, in numpy here, of those characters -
one oracle index PER REFERENCE; nothing comes from the library under test.  Compared as one list, so the order of the records -
(ref, seq, strand with '+' first, start) - is part of every comparison.  One cross-check per case asserts byte equality with
refset.find_refset / summary_refset on the same inputs; those refuse a batch with a sequence of fewer than 3 bases, so they get the
batch without them and their `seq` is mapped back.

Set: tests/test_gpu_refset.py's reference lengths without the 16 400-base one (the device form refuses the single-index route), the
references without a k-mer (k - 1 bases; 40 and 64 bases too at k = 96) in the middle, behind six that can be queried: a slab cut
falls beside them at 1, 2 and 3 references a slab.  Batch, chosen for the cuts the planner makes: a contig of 70 000 bases - more
than 256 chunks of max(256, 4 k) bases at k = 31, so a second task per reference - with copies of references across the first three
chunk cuts, across position 8 192 and multiples of 128 (the group and the chunk of the stages behind the walk) and across 65 536, a
1 % and a 3 % mutated copy, one with a deletion, one reverse-complemented; contigs of 40, 257 and 511 bases, so that pair offsets are
unaligned; contigs of 0, 1, 2 and 3 bases in the middle; 300 contigs of 5 bases at the end, behind 300 empty ones: the host's bound
of the chunks, total / chunk + n_seqs, counts a slot per sequence and every contig with a base fills one, so it is the empty contigs
that make the bound exceed the chunks by more than a task's worth - tasks without an item exist."""
import ctypes as C

import numpy as np
import pytest

import kbo_amd
from kbo_amd import _capi, refset
from oracle import binding as ora

from gpu_helpers import Guarded

pytestmark = pytest.mark.gpu

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
COMP = np.arange(256, dtype=np.uint8)
for _a, _b in zip(b"ACGT", b"TGCA"):
    COMP[_a] = _b
CHUNK = 256  # KBO_REFSET_CHUNK (tests/test_refset_host.py pins it to the header)
E_BAD_ARG = -4
N_BEFORE_STATUS = 6  # references that can be queried in front of the first one that cannot


def _rnd(rng, n):
    return ACGT[rng.integers(0, 4, n)].copy()


def _mutate(rng, a, rate):
    a = a.copy()
    pos = np.flatnonzero(rng.random(len(a)) < rate)
    a[pos] = ACGT[(np.searchsorted(ACGT, a[pos]) + rng.integers(1, 4, len(pos))) % 4]
    return a


def _shapes(k, rc):
    rng = np.random.default_rng(2000 + k)
    lens = [k, 300, 1500, 200, 300, 300, k - 1, 40, 64, 97, 333, 700, 1000, 2000, 3000, 5000, 128, 257, 511, 1200, 800, 450, 999, 2500, 16300]
    if rc:  # (twice the rows: the 16 300-base reference would take the single-index route)
        lens = lens[:-1]
    refs = [_rnd(rng, n) for n in lens]
    refs[3][100] = ord("N")
    refs[5] = refs[4].copy()
    cut = max(CHUNK, 4 * k)
    big = _rnd(rng, 70000)

    def put(at, a):
        big[at:at + len(a)] = a
    for i, r in enumerate((1, 10, 11)):  # across the first three chunk cuts
        put((i + 1) * cut - 75, refs[r][:150])
    put(7500, refs[2])                               # an exact copy across 8 192 and eleven multiples of 128
    put(12000, _mutate(rng, refs[12], 0.01))
    put(14000, _mutate(rng, refs[13], 0.03))
    put(17000, np.delete(refs[14], [1500, 1501]))
    put(21000, COMP[refs[19][::-1]])
    if not rc:
        put(25000, refs[24][2000:5000])
    put(40000, refs[15])
    put(64500, refs[23])                             # across 65 536
    with_n = _mutate(rng, refs[18], 0.01)
    with_n[[200, 201]] = ord("N")
    seqs = [big, refs[7].copy(), refs[17].copy(), _rnd(rng, 0), _rnd(rng, 1), _rnd(rng, 2), _rnd(rng, 3), with_n]
    seqs += [_rnd(rng, 0) for _ in range(300)]  # (a contig of 5 bases is a chunk AND a slot of the bound: only the empty ones leave slots over)
    seqs += [_rnd(rng, 5) for _ in range(300)]
    assert [len(s) for s in seqs[:8]] == [70000, 40, 257, 0, 1, 2, 3, 511]
    return refs, seqs


def fold(text):
    """kbo_aln_extent of one pair's characters"""
    chars = np.frombuffer(text.encode() if isinstance(text, str) else bytes(text), dtype=np.uint8)
    hit = chars != ord("-")
    starts = hit & ~np.concatenate([[False], hit[:-1]])
    at = np.flatnonzero(hit)
    return (int((chars == ord("M")).sum()), int((chars == ord("X")).sum()), int((chars == ord("R")).sum()), int(starts.sum()),
            int(at[0]) if len(at) else 0, int(at[-1]) + 1 if len(at) else 0)


class World:
    """references, the batch on the host and on the device, the set under test and the oracle's alignment of every pair"""

    def __init__(self, k, rc):
        self.k, self.rc = k, rc
        self.refs, self.seqs = _shapes(k, rc)
        self.rs = refset.RefSet.build(self.refs, kbo_amd.BuildOpts(k=k, add_revcomp=rc, num_threads=4))
        assert self.rs.lds_only()
        self.aln, self.queryable = {}, []
        for r, ref in enumerate(self.refs):
            oi = ora.Index.build([ref.tobytes()], k=k, add_revcomp=rc)
            assert self.rs.n_kmers(r) == oi.n_kmers
            if oi.n_kmers == 0:
                assert self.rs.status(r) != 0
                continue
            assert self.rs.status(r) == 0
            self.queryable.append(r)
            seen = {}
            for s, q in enumerate(self.seqs):
                if len(q) < 3:  # no alignment (derandomize.rs:274-276): no record
                    continue
                for strand, text in ((1, q.tobytes()), (2, COMP[q[::-1]].tobytes())):
                    if text not in seen:
                        seen[text] = oi.matches(text, 1e-7)
                    self.aln[r, s, strand] = seen[text]
        # the references that cannot be queried lie in the middle, behind six that can: a cut beside them at 1, 2 and 3 a slab
        status = [r for r in range(len(self.refs)) if r not in self.queryable]
        assert status[0] == N_BEFORE_STATUS and status[-1] < len(self.refs) - 1 and self.queryable[:N_BEFORE_STATUS] == list(range(N_BEFORE_STATUS))
        self.n_seqs = len(self.seqs)
        self.offsets = np.zeros(self.n_seqs + 1, dtype=np.uint64)
        self.offsets[1:] = np.cumsum([len(s) for s in self.seqs])
        self.total = int(self.offsets[-1])
        self.kept = [s for s in range(self.n_seqs) if len(self.seqs[s]) >= 3]  # what the host calls accept
        self._exp, self._host = {}, {}
        self.device = None

    def on_device(self):
        """the set's copy and the batch on the current device, once (the oracle side above needs none)"""
        import torch
        if self.device is None:
            self.rs.to_device()
            self.device = torch.device("cuda", torch.cuda.current_device())
            q = np.zeros(self.total + 16, dtype=np.uint8)
            q[:self.total] = np.concatenate(self.seqs)
            self.d_q = torch.from_numpy(q).to(self.device)
            self.d_off = torch.from_numpy(self.offsets.astype(np.int64)).to(self.device)
        return self

    def expected(self, form, gap, strands):
        key = (form, gap, strands)
        if key not in self._exp:
            out = []
            for r in self.queryable:
                for s in range(self.n_seqs):
                    for strand in (1, 2):
                        if not (strands & strand and (r, s, strand) in self.aln):
                            continue
                        if form == "find":
                            out += [(r, s, strand) + t for t in ora.run_lengths_gapped(self.aln[r, s, strand], gap)]
                        else:
                            e = fold(self.aln[r, s, strand])
                            if e[3] > 0:
                                out.append((r, s, strand) + e)
            self._exp[key] = out
        return self._exp[key]

    def host(self, form, gap, strands):
        """the host call on the batch without the sequences it refuses, `seq` mapped back: a structured array"""
        key = (form, gap, strands)
        if key not in self._host:
            seqs = [self.seqs[s] for s in self.kept]
            if form == "find":
                rec = refset.find_refset(seqs, self.rs, kbo_amd.FindOpts(max_gap_len=gap), strands=strands)
            else:
                rec = refset.summary_refset(seqs, self.rs, strands=strands)
            rec["seq"] = np.asarray(self.kept, dtype=np.uint32)[rec["seq"]]
            self._host[key] = rec
        return self._host[key]

    def work_bytes(self, form, strands, capacity, refs_per_slab):
        L = kbo_amd.lib()
        fn = L.kbo_find_refset_dev_work_bytes if form == "find" else L.kbo_summary_refset_dev_work_bytes
        return int(fn(self.rs._h, self.n_seqs, self.total, strands, capacity, refs_per_slab))

    def enqueue(self, form, gap, strands, work_ptr, work_bytes, out_ptr, capacity, count_ptr, stream, prob=1e-7):
        L = kbo_amd.lib()
        if form == "find":
            o = _capi.FindOpts(prob, gap)
            return L.kbo_find_refset_dev(self.rs._h, self.d_q.data_ptr(), self.d_off.data_ptr(), self.n_seqs, self.total, C.byref(o), strands,
                                         work_ptr, work_bytes, out_ptr, capacity, count_ptr, stream)
        return L.kbo_summary_refset_dev(self.rs._h, self.d_q.data_ptr(), self.d_off.data_ptr(), self.n_seqs, self.total, prob, strands,
                                        work_ptr, work_bytes, out_ptr, capacity, count_ptr, stream)

    def run(self, form, gap, strands, refs_per_slab, capacity):
        """one call with buffers of its own -> (count, the first min(count, capacity) records as an (n, words) uint32 array)"""
        import torch
        words = 10 if form == "find" else 9
        wb = self.work_bytes(form, strands, capacity, refs_per_slab)
        work = torch.empty(wb // 8 + 2, dtype=torch.int64, device=self.device)
        out = torch.empty((max(capacity, 1), words), dtype=torch.int32, device=self.device)
        count = torch.full((1,), -1, dtype=torch.int64, device=self.device)  # (the call does not need it zeroed)
        s = torch.cuda.current_stream(self.device)
        kbo_amd.check(self.enqueue(form, gap, strands, work.data_ptr(), wb, out.data_ptr(), capacity, count.data_ptr(), s.cuda_stream))
        torch.cuda.synchronize()
        n = int(count.item())
        return n, out[:min(n, capacity)].cpu().numpy().view(np.uint32)


_cache = {}


def _oracle_world(k, rc=False):
    if (k, rc) not in _cache:
        _cache[k, rc] = World(k, rc)
    return _cache[k, rc]


def _world(k, rc=False):
    return _oracle_world(k, rc).on_device()


def _tuples(rec):
    return [tuple(int(v) for v in row) for row in rec.tolist()]


def _as_words(rec):
    return np.ascontiguousarray(rec).view(np.uint32).reshape(len(rec), -1)


ALL = 0  # refs_per_slab: as many as a slab may hold


def test_the_fixtures_on_the_oracle_side():
    """at capacity = number of records no case may leave records out: every strand has records, some reference that can be queried
    has none, the planted copies show, and the geometry is the one the planner's cuts were chosen for"""
    for k in (31, 96):
        w = _oracle_world(k)
        for gap in (0, 5):
            for strands in (1, 2, 3):
                exp = w.expected("find", gap, strands)
                for strand in (1, 2):
                    assert bool([t for t in exp if t[2] == strand]) == bool(strands & strand)
                with_records = {t[0] for t in exp}
                assert with_records < set(w.queryable) and len(with_records) >= (10 if strands & 1 else 1)
                assert not [t for t in exp if len(w.seqs[t[1]]) < 3]
        exp = w.expected("find", 0, 3)
        # the exact copy of reference 2 is one run across position 8 192; reference 23's crosses 65 536; the reverse-complemented copy
        assert [t for t in exp if t[:3] == (2, 0, 1) and t[3] <= 7600 and t[4] >= 8900]
        assert [t for t in exp if t[:3] == (23, 0, 1) and t[3] < 65536 < t[4]]
        assert [t for t in exp if t[:3] == (19, 0, 2)]
        assert [t for t in exp if t[1] in (1, 2, 7)] and len({t[1] for t in exp}) >= 3
        cut = max(CHUNK, 4 * k)
        chunks = sum(-(-len(s) // cut) for s in w.seqs)
        assert w.total // cut + w.n_seqs - chunks > 256, "tasks without an item"
        if k == 31:
            assert chunks > 256, "a second task per reference"
        assert int(w.offsets[2]) % 16 and int(w.offsets[3]) % 16 and int(w.offsets[7]) % 4
        assert w.expected("summary", 0, 3) and len(w.expected("summary", 0, 3)) < len(exp)


@pytest.mark.parametrize("refs_per_slab", [1, 3, ALL])
@pytest.mark.parametrize("strands", [1, 2, 3])
@pytest.mark.parametrize("gap", [0, 5])
@pytest.mark.parametrize("k", [31, 96])
def test_find_refset_dev_equals_one_oracle_index_per_reference(k, gap, strands, refs_per_slab):
    w = _world(k)
    exp = w.expected("find", gap, strands)
    n, got = w.run("find", gap, strands, refs_per_slab, len(exp) + 50)
    assert n == len(exp) and _tuples(got) == exp
    assert np.array_equal(got, _as_words(w.host("find", gap, strands)))


@pytest.mark.parametrize("refs_per_slab", [1, 3, ALL])
@pytest.mark.parametrize("strands", [1, 2, 3])
@pytest.mark.parametrize("k", [31, 96])
def test_summary_refset_dev_equals_the_fold_of_the_oracles_characters(k, strands, refs_per_slab):
    w = _world(k)
    exp = w.expected("summary", 0, strands)
    n, got = w.run("summary", 0, strands, refs_per_slab, len(exp) + 50)
    assert n == len(exp) and _tuples(got) == exp  # every field of every record, and records only for the pairs with a run
    assert all(t[6] > 0 for t in _tuples(got))
    assert np.array_equal(got, _as_words(w.host("summary", 0, strands)))
    # aln.n_runs is the number of find records of the pair at max_gap_len = 0
    runs = {}
    for t in w.expected("find", 0, strands):
        runs[t[:3]] = runs.get(t[:3], 0) + 1
    assert {t[:3]: t[6] for t in _tuples(got)} == runs


@pytest.mark.parametrize("form", ["find", "summary"])
def test_a_set_with_reverse_complements_in_the_indexes(form):
    w = _world(31, True)
    exp = w.expected(form, 0, 3)
    n, got = w.run(form, 0, 3, 3, len(exp) + 50)
    assert n == len(exp) > 20 and _tuples(got) == exp
    assert np.array_equal(got, _as_words(w.host(form, 0, 3)))


@pytest.mark.parametrize("short", [0, 1, "none"])
@pytest.mark.parametrize("form", ["find", "summary"])
def test_capacity(form, short):
    """capacity equal to the number of records, one less, and 0 with a NULL output: the count is the full number, the written prefix
    is exact, the bytes behind element `capacity` are as they were"""
    import torch
    w = _world(31)
    gap, strands, words = 5, 3, 10 if form == "find" else 9
    exp = w.expected(form, gap, strands)
    capacity = 0 if short == "none" else len(exp) - short
    wb = w.work_bytes(form, strands, capacity, 3)
    work = torch.empty(wb // 8 + 2, dtype=torch.int64, device=w.device)
    out = Guarded("records", capacity * words * 4, 1 << 20, w.device, seed=3)
    count = torch.full((1,), 12345, dtype=torch.int64, device=w.device)
    s = torch.cuda.current_stream(w.device)
    kbo_amd.check(w.enqueue(form, gap, strands, work.data_ptr(), wb, out.ptr if capacity else None, capacity, count.data_ptr(), s.cuda_stream))
    torch.cuda.synchronize()
    assert int(count.item()) == len(exp)
    out.assert_intact(form)
    got = out.host().view(np.uint32).reshape(capacity, words)
    assert _tuples(got) == exp[:capacity]
    if capacity == 0:
        assert not out.changed()


@pytest.mark.parametrize("refs_per_slab", [1, 3])
@pytest.mark.parametrize("form", ["find", "summary"])
def test_work_of_exactly_the_figure_between_guard_bands(form, refs_per_slab):
    import torch
    w = _world(31)
    gap, strands, words = 5, 3, 10 if form == "find" else 9
    exp = w.expected(form, gap, strands)
    capacity = len(exp) + 7
    wb = w.work_bytes(form, strands, capacity, refs_per_slab)
    assert wb < w.work_bytes(form, strands, capacity, refs_per_slab + 1)  # (so the call cannot take a larger slab than asked for)
    work = Guarded("d_work", wb, 4 << 20, w.device, seed=refs_per_slab)
    out = torch.empty((capacity, words), dtype=torch.int32, device=w.device)
    count = torch.zeros(1, dtype=torch.int64, device=w.device)
    s = torch.cuda.current_stream(w.device)
    kbo_amd.check(w.enqueue(form, gap, strands, work.ptr, wb, out.data_ptr(), capacity, count.data_ptr(), s.cuda_stream))
    torch.cuda.synchronize()
    work.assert_intact(form)
    assert int(count.item()) == len(exp) and _tuples(out[:len(exp)].cpu().numpy().view(np.uint32)) == exp


@pytest.mark.parametrize("form", ["find", "summary"])
def test_work_one_byte_short_of_one_reference_a_slab_is_refused(form):
    import torch
    w = _world(31)
    wb = w.work_bytes(form, 3, 100, 1)
    work = torch.empty(wb // 8 + 2, dtype=torch.int64, device=w.device)
    out = torch.empty((100, 10), dtype=torch.int32, device=w.device)
    count = torch.full((1,), 77, dtype=torch.int64, device=w.device)
    s = torch.cuda.current_stream(w.device)
    assert w.enqueue(form, 0, 3, work.data_ptr(), wb - 1, out.data_ptr(), 100, count.data_ptr(), s.cuda_stream) == E_BAD_ARG
    torch.cuda.synchronize()
    assert int(count.item()) == 77  # nothing was enqueued


def test_two_calls_on_two_streams():
    import torch
    w = _world(31)
    jobs = [("find", 5, 3, 3), ("summary", 0, 3, 1)]
    held = []
    for form, gap, strands, refs_per_slab in jobs:
        words = 10 if form == "find" else 9
        exp = w.expected(form, gap, strands)
        capacity = len(exp) + 5
        wb = w.work_bytes(form, strands, capacity, refs_per_slab)
        work = torch.empty(wb // 8 + 2, dtype=torch.int64, device=w.device)
        out = torch.empty((capacity, words), dtype=torch.int32, device=w.device)
        count = torch.zeros(1, dtype=torch.int64, device=w.device)
        held.append((exp, work, wb, out, capacity, count, torch.cuda.Stream(device=w.device)))
    torch.cuda.synchronize()
    for (form, gap, strands, _), (exp, work, wb, out, capacity, count, s) in zip(jobs, held):
        kbo_amd.check(w.enqueue(form, gap, strands, work.data_ptr(), wb, out.data_ptr(), capacity, count.data_ptr(), s.cuda_stream))
    torch.cuda.synchronize()
    for exp, work, wb, out, capacity, count, s in held:
        assert int(count.item()) == len(exp) and _tuples(out[:len(exp)].cpu().numpy().view(np.uint32)) == exp


def test_the_python_wrappers():
    import torch
    w = _world(31)
    exp = w.expected("find", 5, 3)
    rec, count = refset.find_refset_dev(w.d_q, w.d_off, w.rs, kbo_amd.FindOpts(max_gap_len=5), capacity=len(exp) + 10, refs_per_slab=4)
    torch.cuda.synchronize()
    assert rec.shape == (len(exp) + 10, 10) and int(count.item()) == len(exp)
    assert _tuples(rec[:len(exp)].cpu().numpy().view(np.uint32)) == exp
    # the defaults; a batch tensor without slack behind its last base; one strand
    exp = w.expected("summary", 0, 2)
    rec, count = refset.summary_refset_dev(w.d_q[:w.total], w.d_off, w.rs, strands=refset.STRAND_REV)
    torch.cuda.synchronize()
    assert rec.shape == (1 << 16, 9) and int(count.item()) == len(exp)
    assert _tuples(rec[:len(exp)].cpu().numpy().view(np.uint32)) == exp
    rec, count = refset.find_refset_dev(w.d_q, w.d_off, w.rs, strands=refset.STRAND_FWD, capacity=0, refs_per_slab=0)
    torch.cuda.synchronize()
    assert rec.shape == (0, 10) and int(count.item()) == len(w.expected("find", 0, 1))
