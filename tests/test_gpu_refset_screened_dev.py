"""kbo_refset_candidates_dev and kbo_find / summary / best_refset_screened_dev (kbo_hip.h "The SCREENED device forms";
kbo_amd/csrc/refset_cand_kernels.hip) over the world of tests/test_refset_screen_host.py: 19 references, a wide one among them, and 21
sequences of 3 to 20 000 bases.

  - the bitmap is kbo_refset_candidates_host's bit for bit, and the statistics are numpy's sums over it;
  - with caps that hold every candidate the records are byte for byte those of the host forms on the same set, d_work sized at exactly
    its figure and the records at exactly their number, both behind guard bands;
  - with tight caps the walked pairs are the prefix numpy computes from the host's bitmap and the lengths, the records the host's
    restricted to those pairs, and the best table the host's fold of the restricted summary, done here by sorting;
  - no candidate; a batch of thousands of short sequences, where the bitmap spans several scan blocks and, at 1e-3, the references
    that cannot be screened own more than 256 items each; two calls back to back on one stream.
Every reference of this world can be screened at 1e-7 and at 1e-4, so 1e-3 runs next to them wherever references that cannot be
screened matter: their pairs are all candidates, the 3-base sequence's included."""
import ctypes as C

import numpy as np
import pytest

import kbo_amd
from kbo_amd import _capi, refset

from gpu_helpers import Guarded
from test_refset_screen_host import N_UNRELATED, PROBS, SEED_MIN, seed_len, world

pytestmark = pytest.mark.gpu

WORDS = {"find": 10, "summary": 9}
DTYPE = {"find": refset.REF_RUN, "summary": refset.REF_SUMMARY}
# At 1e-7 and 1e-4 every reference of the world can be screened (m_r >= 11).  At 1e-3 most cannot (m_r = 9 or 10) and a few can (11,
# 13): all pairs of the former are candidates, the latter are screened - both kinds in one bitmap.  At 0.5 none can.
MIXED_PROB = 1e-3


class Batch:
    """a batch of a world on the device, the host's bitmap and the host forms' records of it"""
    _cache = {}

    def __init__(self, w, seqs):
        import torch
        self.w, self.seqs, self.n_seqs = w, seqs, len(seqs)
        self.lens = np.asarray([len(s) for s in seqs], dtype=np.int64)
        self.offsets = np.zeros(self.n_seqs + 1, dtype=np.int64)
        self.offsets[1:] = np.cumsum(self.lens)
        self.total = int(self.offsets[-1])
        w.rs.to_device()
        self.device = torch.device("cuda", torch.cuda.current_device())
        q = np.zeros(self.total + 16, dtype=np.uint8)
        q[:self.total] = np.concatenate(seqs)
        self.d_q = torch.from_numpy(q).to(self.device)
        self.d_off = torch.from_numpy(self.offsets).to(self.device)
        self._bits, self._host = {}, {}

    @classmethod
    def of(cls, k, rc=False, which="world"):
        key = (k, rc, which)
        if key not in cls._cache:
            w = world(k, rc)
            if which == "world":
                seqs = w.seqs
            elif which == "unrelated":
                seqs = w.seqs[:N_UNRELATED]
            else:  # thousands of short sequences in front of the world's planted contigs
                rng = np.random.default_rng(77)
                acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
                seqs = [acgt[rng.integers(0, 4, 40)].copy() for _ in range(3000)] + w.seqs[N_UNRELATED:]
            cls._cache[key] = cls(w, seqs)
        return cls._cache[key]

    def bits(self, prob, strands):
        """the host's bitmap [n_refs, n_seqs, 2]"""
        if (prob, strands) not in self._bits:
            self._bits[prob, strands] = self.w.rs.candidates(self.seqs, prob, strands, host=True)
        return self._bits[prob, strands]

    def candidates(self, prob, strands):
        """(the set bits in ascending order, their pairs' lengths)"""
        order = np.flatnonzero(self.bits(prob, strands).ravel())
        return order, self.lens[(order >> 1) % self.n_seqs]

    def walked(self, prob, strands, max_pairs, max_bases):
        """the prefix of the candidates within both caps: its length"""
        order, lens = self.candidates(prob, strands)
        within = np.cumsum(lens)[:max_pairs] <= max_bases
        return int(within.sum()) if within.all() else int(np.argmin(within))

    def host(self, form, prob, strands, gap=0):
        key = (form, prob, strands, gap)
        if key not in self._host:
            if form == "find":
                self._host[key] = refset.find_refset(self.seqs, self.w.rs, kbo_amd.FindOpts(max_error_prob=prob, max_gap_len=gap), strands)
            elif form == "summary":
                self._host[key] = refset.summary_refset(self.seqs, self.w.rs, prob, strands)
            else:
                self._host[key] = refset.best_refset(self.seqs, self.w.rs, prob, strands)
        return self._host[key]

    def restricted(self, form, prob, strands, gap, n_walked):
        """the host's records of the first n_walked candidates"""
        rec = self.host(form, prob, strands, gap)
        order, _ = self.candidates(prob, strands)
        bit = (rec["ref"].astype(np.int64) * self.n_seqs + rec["seq"]) * 2 + rec["strand"] - 1
        return rec[np.isin(bit, order[:n_walked])]

    def run(self, form, prob, strands, max_pairs, max_bases, gap=0, capacity=None, work=None, seed=1, sync=True):
        """one call, d_work at exactly its figure and the output at exactly `capacity` records (n_seqs for best), behind guards"""
        import torch
        L = kbo_amd.lib()
        h, s = self.w.rs._h, torch.cuda.current_stream(self.device)
        stats = torch.full((4,), -1, dtype=torch.int64, device=self.device)
        if form == "best":
            wb = int(L.kbo_best_refset_screened_dev_work_bytes(h, self.n_seqs, self.total, strands, max_pairs, max_bases))
            out = Guarded("table", self.n_seqs * 48, 1 << 16, self.device, seed=seed)
        else:
            fn = L.kbo_find_refset_screened_dev_work_bytes if form == "find" else L.kbo_summary_refset_screened_dev_work_bytes
            wb = int(fn(h, self.n_seqs, self.total, strands, capacity, max_pairs, max_bases))
            out = Guarded("records", capacity * WORDS[form] * 4, 1 << 16, self.device, seed=seed)
        assert wb > 0
        if work is None:
            work = Guarded("d_work", wb, 1 << 20, self.device, seed=seed + 1)
        assert work.n >= wb
        count = torch.full((1,), 12345, dtype=torch.int64, device=self.device)
        args = (h, self.d_q.data_ptr(), self.d_off.data_ptr(), self.n_seqs, self.total)
        tail = (max_pairs, max_bases, stats.data_ptr(), s.cuda_stream)
        if form == "best":
            rc = L.kbo_best_refset_screened_dev(*args, prob, strands, work.ptr, wb, out.ptr, *tail)
        elif form == "find":
            o = _capi.FindOpts(prob, gap)
            rc = L.kbo_find_refset_screened_dev(*args, C.byref(o), strands, work.ptr, wb, out.ptr if capacity else None, capacity, count.data_ptr(), *tail)
        else:
            rc = L.kbo_summary_refset_screened_dev(*args, prob, strands, work.ptr, wb, out.ptr if capacity else None, capacity, count.data_ptr(), *tail)
        kbo_amd.check(rc)
        res = dict(form=form, work=work, out=out, count=count, stats=stats, capacity=capacity)
        return self.finish(res) if sync else res

    def finish(self, res):
        import torch
        torch.cuda.synchronize()
        res["work"].assert_intact(res["form"])
        res["out"].assert_intact(res["form"])
        res["stats"] = tuple(int(v) for v in res["stats"].cpu().numpy())
        if res["form"] == "best":
            res["records"] = np.frombuffer(res["out"].host().tobytes(), dtype=refset.REF_BEST)
        else:
            res["count"] = int(res["count"].item())
            n = min(res["count"], res["capacity"])
            res["records"] = np.frombuffer(res["out"].host().tobytes(), dtype=DTYPE[res["form"]])[:n]
        return res


def fold_best(summary, n_seqs):
    """kbo_best_refset's table of these summary records, by sorting: (larger n_match, smaller ref, '+' first)"""
    out = np.zeros(n_seqs, dtype=refset.REF_BEST)
    out["seq"] = np.arange(n_seqs)
    out["ref"] = out["second_ref"] = refset.REF_NONE
    srt = summary[np.lexsort((summary["strand"], summary["ref"], -summary["n_match"].astype(np.int64), summary["seq"]))]
    for s in np.unique(srt["seq"]):
        rows = srt[srt["seq"] == s]
        for f in ("ref", "strand", "n_match", "n_mismatch", "n_jump", "n_runs", "start", "end"):
            out[f][s] = rows[0][f]
        out["n_hits"][s] = len(rows)
        others = rows[rows["ref"] != rows[0]["ref"]]
        if len(others):
            out["second_ref"][s], out["second_match"][s] = others[0]["ref"], others[0]["n_match"]
    return out


@pytest.mark.parametrize("k,rc", [(31, False), (31, True), (96, False)])
def test_candidates_dev_is_the_cpu_screen(k, rc):
    import torch
    b = Batch.of(k, rc)
    n_bits = len(b.w.refs) * b.n_seqs * 2
    for prob in PROBS:
        for strands in (3, 1, 2):
            host = b.bits(prob, strands)
            bits, stats = b.w.rs.candidates_dev(b.d_q, b.d_off, prob, strands)
            torch.cuda.synchronize()
            got = np.unpackbits(bits.cpu().numpy().view(np.uint8), bitorder="little")[:n_bits].astype(bool).reshape(host.shape)
            assert np.array_equal(got, host), (prob, strands, np.argwhere(got != host)[:10])
            order, lens = b.candidates(prob, strands)
            assert tuple(int(v) for v in stats.cpu().numpy()) == (len(order), int(lens.sum()), 0, 0), (prob, strands)
    assert all(m < SEED_MIN for m in b.w.m[0.5]), "at 0.5 no reference can be screened: all pairs of the packed ones are candidates"


def test_candidates_dev_work_is_exactly_its_figure():
    import torch
    b = Batch.of(31)
    L = kbo_amd.lib()
    for strands in (1, 2, 3):
        wb = int(L.kbo_refset_candidates_dev_work_bytes(b.w.rs._h, b.n_seqs, b.total, strands))
        work = Guarded("d_work", wb, 1 << 20, b.device, seed=strands)
        words = (len(b.w.refs) * b.n_seqs * 2 + 31) // 32
        bits = Guarded("d_bits", words * 4, 1 << 16, b.device, seed=9)
        stats = torch.zeros(4, dtype=torch.int64, device=b.device)
        kbo_amd.check(L.kbo_refset_candidates_dev(b.w.rs._h, b.d_q.data_ptr(), b.d_off.data_ptr(), b.n_seqs, b.total, 1e-4, strands, work.ptr, wb,
                                                  bits.ptr, stats.data_ptr(), torch.cuda.current_stream(b.device).cuda_stream))
        torch.cuda.synchronize()
        work.assert_intact("candidates")
        bits.assert_intact("candidates")
        got = np.unpackbits(bits.host(), bitorder="little")[:len(b.w.refs) * b.n_seqs * 2].astype(bool)
        assert np.array_equal(got, b.bits(1e-4, strands).ravel())


@pytest.mark.parametrize("prob", [1e-7, 1e-4, MIXED_PROB])
@pytest.mark.parametrize("strands", [1, 2, 3])
@pytest.mark.parametrize("k", [31, 96])
def test_ample_caps_give_the_host_forms_records(k, strands, prob):
    b = Batch.of(k)
    order, lens = b.candidates(prob, strands)
    n_cand, bases = len(order), int(lens.sum())
    assert n_cand > 0
    if prob == MIXED_PROB:  # the references that cannot be screened: every pair, the 3-base sequence's included
        assert int(b.lens.min()) == 3 and b.bits(prob, strands)[:, int(np.argmin(b.lens))].any() and not b.bits(prob, strands)[b.w.packed].all()
    full = (n_cand, bases, n_cand, bases)
    for form, gap in (("find", 0), ("find", 5), ("summary", 0)):
        host = b.host(form, prob, strands, gap)
        assert len(host) > 0
        got = b.run(form, prob, strands, n_cand, bases, gap, capacity=len(host))
        assert got["stats"] == full and got["count"] == len(host), (form, gap, got["stats"], got["count"])
        assert got["records"].tobytes() == host.tobytes(), (form, gap)
    got = b.run("best", prob, strands, n_cand, bases)
    assert got["stats"] == full
    assert got["records"].tobytes() == b.host("best", prob, strands).tobytes()
    assert got["records"].tobytes() == fold_best(b.host("summary", prob, strands), b.n_seqs).tobytes()


TIGHT = ["pairs", "bases", "below_first"]


@pytest.mark.parametrize("cap", TIGHT)
def test_tight_caps_walk_the_prefix(cap):
    b = Batch.of(31)
    prob, strands = 1e-4, 3
    order, lens = b.candidates(prob, strands)
    n_cand, bases = len(order), int(lens.sum())
    assert n_cand > 8
    if cap == "pairs":
        max_pairs, max_bases = n_cand - 1, bases
        n_walked = n_cand - 1
    elif cap == "bases":  # one base short of the first `mid` pairs' total
        mid = n_cand // 2
        max_pairs, max_bases = n_cand, int(lens[:mid].sum()) - 1
        n_walked = b.walked(prob, strands, max_pairs, max_bases)
        assert 0 < n_walked < mid
    else:
        max_pairs, max_bases = n_cand, int(lens[0]) - 1
        n_walked = 0
    assert b.walked(prob, strands, max_pairs, max_bases) == n_walked
    stats = (n_cand, bases, n_walked, int(lens[:n_walked].sum()))
    for form, gap in (("find", 5), ("summary", 0)):
        exp = b.restricted(form, prob, strands, gap, n_walked)
        assert len(exp) <= len(b.host(form, prob, strands, gap)) and (n_walked > 0 or len(exp) == 0)
        got = b.run(form, prob, strands, max_pairs, max_bases, gap, capacity=len(exp))
        assert got["stats"] == stats and got["count"] == len(exp), (form, got["stats"], stats, got["count"], len(exp))
        assert got["records"].tobytes() == exp.tobytes(), form
    got = b.run("best", prob, strands, max_pairs, max_bases)
    assert got["stats"] == stats
    assert got["records"].tobytes() == fold_best(b.restricted("summary", prob, strands, 0, n_walked), b.n_seqs).tobytes()
    if n_walked == 0:
        assert (got["records"]["ref"] == refset.REF_NONE).all() and not got["records"]["n_hits"].any()


@pytest.mark.parametrize("form,gap", [("find", 5), ("summary", 0)])
def test_records_beyond_capacity_are_counted_and_not_written(form, gap):
    b = Batch.of(31)
    prob, strands = 1e-7, 3
    order, lens = b.candidates(prob, strands)
    host = b.host(form, prob, strands, gap)
    for capacity in (len(host) - 3, 1, 0):
        got = b.run(form, prob, strands, len(order), int(lens.sum()), gap, capacity=capacity)  # (run() checks the guard behind the records)
        assert got["count"] == len(host) and got["stats"][2] == len(order)
        assert got["records"].tobytes() == host[:capacity].tobytes()


def test_no_candidate():
    b = Batch.of(31, which="unrelated")
    assert not b.bits(1e-7, 3).any()
    for form in ("find", "summary"):
        got = b.run(form, 1e-7, 3, 16, 1000, 5, capacity=4)
        assert got["stats"] == (0, 0, 0, 0) and got["count"] == 0
    got = b.run("best", 1e-7, 3, 16, 1000)
    assert got["stats"] == (0, 0, 0, 0)
    assert got["records"].tobytes() == fold_best(np.zeros(0, dtype=refset.REF_SUMMARY), b.n_seqs).tobytes()


@pytest.mark.parametrize("prob", [1e-4, MIXED_PROB])
def test_many_words_and_several_tasks_a_reference(prob):
    b = Batch.of(31, which="many")
    strands = 3
    n_bits = len(b.w.refs) * b.n_seqs * 2
    order, lens = b.candidates(prob, strands)
    chunk = 256
    items_of_ref = np.bincount(order // (2 * b.n_seqs), weights=-(-lens // chunk), minlength=len(b.w.refs))
    assert n_bits // 32 > 3 * 1024 and len(order) > 0
    if prob == MIXED_PROB:  # thousands of candidates a reference that cannot be screened: several tasks each, several blocks of pairs
        assert any(0 < m < SEED_MIN for m in b.w.m.get(prob, [seed_len(b.w.k, n, prob) if n else 0 for n in b.w.n_kmers]))
        assert len(order) > 4096 and items_of_ref.max() > 2 * 256
    host = b.host("summary", prob, strands)
    got = b.run("summary", prob, strands, len(order), int(lens.sum()), capacity=len(host))
    assert got["stats"] == (len(order), int(lens.sum()), len(order), int(lens.sum())) and got["count"] == len(host) > 0
    assert got["records"].tobytes() == host.tobytes()
    got = b.run("best", prob, strands, len(order), int(lens.sum()))
    assert got["records"].tobytes() == b.host("best", prob, strands).tobytes()


def test_two_calls_back_to_back_on_one_stream():
    b = Batch.of(31)
    L = kbo_amd.lib()
    o3, l3 = b.candidates(1e-4, 3)
    o1, l1 = b.candidates(1e-7, 1)
    h3, h1 = b.host("summary", 1e-4, 3), b.host("find", 1e-7, 1, 5)
    wb = max(int(L.kbo_summary_refset_screened_dev_work_bytes(b.w.rs._h, b.n_seqs, b.total, 3, len(h3), len(o3), int(l3.sum()))),
             int(L.kbo_find_refset_screened_dev_work_bytes(b.w.rs._h, b.n_seqs, b.total, 1, len(h1), len(o1), int(l1.sum()))))
    work = Guarded("d_work", wb, 1 << 20, b.device, seed=5)  # ONE scratch for both: the second call runs over what the first left
    first = b.run("summary", 1e-4, 3, len(o3), int(l3.sum()), capacity=len(h3), work=work, sync=False)
    second = b.run("find", 1e-7, 1, len(o1), int(l1.sum()), 5, capacity=len(h1), work=work, sync=False)
    first, second = b.finish(first), b.finish(second)
    assert first["count"] == len(h3) and first["records"].tobytes() == h3.tobytes()
    assert second["count"] == len(h1) and second["records"].tobytes() == h1.tobytes()
    assert first["stats"][2] == len(o3) and second["stats"][2] == len(o1)
