"""kbo_cover_refset / kbo_cover_refset_dev (kbo_hip.h "The COVER of a reference") on the GPU against brute force.

The yardstick is tests/test_refset_cover_host.py's: the occurrence dicts of tests/test_refset_locate_host.py, every window of every
run looked up in them, H, D and every field of the record from the header's definitions with numpy - nothing from the library's
walk.  All comparisons are exact: every field of every record and every word of the profile, and the bytes of kbo_cover_refset_host.
The set - twelve references of 300 to 2 000 bases, one of 20 kbp on the wide route, one without a k-mer - and the contigs are that
file's world(); the planted cases are test_refset_cover_host.planted(), run again here and counted in what the GPU returned."""
import numpy as np
import pytest

import kbo_amd
from kbo_amd import refset

from gpu_helpers import Guarded
from test_refset_cover_host import NO_ENTRIES, assert_identities, assert_same, brute_cover, planted, world_entries
from test_refset_locate_host import GAP, SHORT, WIDE, make_refs, world

pytestmark = pytest.mark.gpu

CASES = [(31, False), (31, True), (96, False), (96, True)]
BACK = 1 << 16


def _opts():
    return kbo_amd.FindOpts(max_gap_len=GAP)


def _words(a):
    return np.ascontiguousarray(a).view(np.uint32).reshape(len(a), -1)


_device = {}


def _on_device(key, rs, seqs):
    """the set's copy and the batch on the current device, once per world"""
    import torch
    if key not in _device:
        rs.to_device()
        dev = torch.device("cuda", torch.cuda.current_device())
        total = sum(len(s) for s in seqs)
        q = np.zeros(total + 16, dtype=np.uint8)
        q[:total] = np.concatenate(seqs)
        off = np.zeros(len(seqs) + 1, dtype=np.int64)
        off[1:] = np.cumsum([len(s) for s in seqs])
        _device[key] = (torch.from_numpy(q).to(dev), torch.from_numpy(off).to(dev), dev, total)
    return _device[key]


_expected = {}


def _brute(w, k, strands, runs):
    """brute force over find's runs of a world, shared among the tests (the prefilter changes no record)"""
    key = (k, w.rc, strands)
    if key not in _expected:
        _expected[key] = (brute_cover(w.refs, w.dicts, world_entries(w), k, w.seqs, runs), _words(runs).copy())
    exp, same = _expected[key]
    assert np.array_equal(_words(runs), same)
    return exp


@pytest.mark.parametrize("prefilter", [False, True])
@pytest.mark.parametrize("k,rc", CASES)
def test_cover_over_find_equals_brute_force_and_the_host_form(k, rc, prefilter):
    w = world(k, rc, prefilter)
    assert w.rs.has_positions() and w.rs.has_prefilter == prefilter and w.rs.packed_only()
    for strands in (1, 2, 3):
        runs = refset.find_refset(w.seqs, w.rs, _opts(), strands=strands)
        assert len(runs) > (40 if strands & 1 or rc else 2)
        got = refset.cover_refset(w.seqs, w.rs, runs, depth=True)
        assert_same(got, _brute(w, k, strands, runs), "strands %d" % strands)
        assert_identities(k, *got)
        host = refset.cover_refset(w.seqs, w.rs, runs, depth=True, host=True)
        assert got[0].tobytes() == host[0].tobytes() and got[1].tobytes() == host[1].tobytes()
        assert refset.cover_refset(w.seqs, w.rs, runs).tobytes() == got[0].tobytes()  # without the profile: the same records
        if strands == 3:
            assert np.array_equal(_words(runs), _words(w.cpu_runs()))  # the runs the CPU checks of the fixtures went by
            c = got[0]
            assert c["covered"][WIDE] > 0 and w.rs.route(WIDE) == refset.ROUTE_WIDE and c["flags"][SHORT] == NO_ENTRIES == c["flags"].sum()
            assert c["n_multi"].sum() > 0 and c["n_segments"].max() > 1
    none = refset.cover_refset(w.seqs, w.rs, runs[:0], depth=True)
    assert not none[0]["n_runs"].any() and not none[1].any() and np.array_equal(none[0]["ref_len"], [len(r) for r in w.refs])


@pytest.mark.parametrize("k,rc", CASES)
def test_the_planted_cases_on_the_gpu(k, rc):
    p = planted(k, rc)
    got = refset.cover_refset(p.seqs, p.rs, p.runs, depth=True)
    assert_same(got, p.expected())
    assert_identities(k, *got)
    p.assert_reached(*got)
    host = refset.cover_refset(p.seqs, p.rs, p.runs, depth=True, host=True)
    assert got[0].tobytes() == host[0].tobytes() and got[1].tobytes() == host[1].tobytes()


class _Out:
    """d_covers, d_depth and d_work at exactly their sizes, each between guard bands"""

    def __init__(self, rs, dev, seed, depth=True):
        self.n, self.bases, self.wb = len(rs), rs.cover_bases(), rs.cover_work_bytes()
        self.covers = Guarded("d_covers", self.n * 48, BACK, dev, seed=seed)
        self.depth = Guarded("d_depth", self.bases * 4, BACK, dev, seed=seed + 1) if depth else None
        self.work = Guarded("d_work", self.wb, BACK, dev, seed=seed + 2)

    def call(self, rs, d_q, d_off, n_seqs, total, runs_ptr, count_ptr, capacity, stream):
        kbo_amd.check(kbo_amd.lib().kbo_cover_refset_dev(rs._h, d_q.data_ptr(), d_off.data_ptr(), n_seqs, total, runs_ptr, count_ptr, capacity,
                                                         self.covers.ptr, self.depth.ptr if self.depth else None, self.work.ptr, self.wb,
                                                         stream))

    def result(self):
        for g in (self.covers, self.depth, self.work):
            if g is not None:
                g.assert_intact("cover")
        covers = self.covers.host().view(refset.REF_COVER).copy()
        return covers, (self.depth.host().view(np.uint32).copy() if self.depth else None)


@pytest.mark.parametrize("short", [False, True])
@pytest.mark.parametrize("screened", [False, True])
@pytest.mark.parametrize("k,rc", CASES)
def test_find_dev_then_cover_dev_on_one_stream(k, rc, screened, short):
    """kbo_find_refset_dev / kbo_find_refset_screened_dev and kbo_cover_refset_dev enqueued back to back, nothing read in between, with
    and without d_depth: records and profile are the host form's over the first min(n, capacity) runs, and the bytes around d_covers,
    d_depth and d_work are as they were"""
    import torch
    w = world(k, rc, screened)
    d_q, d_off, dev, total = _on_device(id(w), w.rs, w.seqs)
    runs = refset.find_refset(w.seqs, w.rs, _opts())
    capacity = len(runs) - 7 if short else len(runs) + 9
    n = min(len(runs), capacity)
    host = refset.cover_refset(w.seqs, w.rs, runs[:n], depth=True, host=True)
    s = torch.cuda.Stream(device=dev)
    with_depth, without = _Out(w.rs, dev, k + capacity), _Out(w.rs, dev, k + capacity + 5, depth=False)
    torch.cuda.synchronize()
    if screened:
        rec, count, stats = refset.find_refset_dev(d_q, d_off, w.rs, _opts(), capacity=capacity, stream=s, screened=True, max_pairs=4096,
                                                   max_pair_bases=1 << 22)
    else:
        rec, count = refset.find_refset_dev(d_q, d_off, w.rs, _opts(), capacity=capacity, stream=s)
    for out in (with_depth, without):
        out.call(w.rs, d_q, d_off, len(w.seqs), total, rec.data_ptr(), count.data_ptr(), capacity, s.cuda_stream)
    torch.cuda.synchronize()
    assert int(count.item()) == len(runs)
    if screened:
        assert int(stats[2]) == int(stats[0]) > 0  # every candidate pair was walked: the records are complete
    assert np.array_equal(rec[:n].cpu().numpy().view(np.uint32), _words(runs)[:n])
    covers, depth = with_depth.result()
    assert covers.tobytes() == host[0].tobytes() and depth.tobytes() == host[1].tobytes()
    covers2, none = without.result()
    assert none is None and covers2.tobytes() == covers.tobytes()
    if short:
        assert covers.tobytes() != refset.cover_refset(w.seqs, w.rs, runs, host=True).tobytes()  # (the runs left out do count)


def _cover_dev(key, rs, seqs, runs, n_seqs=None, count=None, capacity=None, seed=0):
    """kbo_cover_refset_dev over hand-made records -> (covers, profile)"""
    import torch
    d_q, d_off, dev, total = _on_device(key, rs, seqs)
    d_runs = torch.from_numpy(_words(runs).view(np.int32).copy()).to(dev)
    d_n = torch.tensor([len(runs) if count is None else count], dtype=torch.int64, device=dev)
    out = _Out(rs, dev, len(runs) + seed)
    s = torch.cuda.current_stream(dev)
    out.call(rs, d_q, d_off, len(seqs) if n_seqs is None else n_seqs, total, d_runs.data_ptr(), d_n.data_ptr(),
             len(runs) if capacity is None else capacity, s.cuda_stream)
    torch.cuda.synchronize()
    return out.result()


def test_unusable_records_are_skipped_and_leave_the_others_alone():
    """records the contract defines as unusable, one per condition, among good ones: the result is that of the good ones alone"""
    w = world(31, True)
    found = refset.find_refset(w.seqs, w.rs, _opts())
    good = np.concatenate([found[:36], found[found["ref"] == WIDE][:4]])  # (some on the wide reference, for the last part)
    assert len(good) == 40
    runs = good.copy()
    lens = [len(s) for s in w.seqs]
    bad = {3: ("ref", len(w.refs)), 7: ("ref", SHORT), 11: ("seq", len(w.seqs)), 14: ("strand", 0), 18: ("strand", 3), 22: ("ref", 0xFFFFFFFF),
           26: ("seq", 0xFFFFFFFF), 30: ("strand", 0xFFFFFFFF)}
    for x, (field, value) in bad.items():
        runs[field][x] = value
    runs["start"][33] = runs["end"][33] + 1                      # start > end
    runs["end"][36] = lens[runs["seq"][36]] + 1                  # end beyond the sequence
    runs["start"][38], runs["end"][38] = 0xFFFFFFF0, 0xFFFFFFFF  # both far beyond it
    unusable = sorted(list(bad) + [33, 36, 38])
    kept = good[[x for x in range(len(good)) if x not in unusable]]
    host = refset.cover_refset(w.seqs, w.rs, kept, depth=True, host=True)
    covers, depth = _cover_dev(id(w), w.rs, w.seqs, runs)
    assert covers.tobytes() == host[0].tobytes() and depth.tobytes() == host[1].tobytes()
    assert covers["n_runs"].sum() == len(kept) and covers["n_anchors"].sum() > 0
    # a count beyond the capacity reads `capacity` records; a count of 0 none; capacity 0 none and no d_runs
    all_good = refset.cover_refset(w.seqs, w.rs, good, depth=True, host=True)
    covers, depth = _cover_dev(id(w), w.rs, w.seqs, good, count=1 << 40)
    assert covers.tobytes() == all_good[0].tobytes() and depth.tobytes() == all_good[1].tobytes()
    nothing = refset.cover_refset(w.seqs, w.rs, good[:0], depth=True, host=True)
    for kw in (dict(count=0), dict(capacity=0)):
        covers, depth = _cover_dev(id(w), w.rs, w.seqs, good, seed=3, **kw)
        assert covers.tobytes() == nothing[0].tobytes() and not depth.any()
    # the batch seen with fewer sequences: the records of the others are unusable
    covers, depth = _cover_dev(id(w), w.rs, w.seqs, good, n_seqs=2)
    fewer = refset.cover_refset(w.seqs, w.rs, good[good["seq"] < 2], depth=True, host=True)
    assert (good["seq"] >= 2).any() and covers.tobytes() == fewer[0].tobytes() and depth.tobytes() == fewer[1].tobytes()
    # a reference of the single-index route: its runs are skipped, its record has bit 0 and it owns no base of the profile
    refs = make_refs(31, 7031)
    mixed = refset.RefSet.build(refs, kbo_amd.BuildOpts(k=31, add_revcomp=True, num_threads=4), wide_rows=refset.MAX_ROWS, positions=True)
    assert mixed.route(WIDE) == refset.ROUTE_INDEX
    on_wide = good["ref"] == WIDE
    assert on_wide.any() and not on_wide.all()
    covers, depth = _cover_dev("mixed", mixed, w.seqs, good)
    rest = refset.cover_refset(w.seqs, mixed, good[~on_wide], depth=True, host=True)
    assert covers.tobytes() == rest[0].tobytes() and depth.tobytes() == rest[1].tobytes()
    assert covers["flags"][WIDE] == NO_ENTRIES and len(depth) == mixed.cover_bases() == w.rs.cover_bases() - len(refs[WIDE])


def test_the_same_inputs_twice_give_the_same_bytes():
    """the adds are integer atomics: their order changes nothing.  Many runs on few bases, so that waves do meet on a word"""
    w = world(31, True)
    found = refset.find_refset(w.seqs, w.rs, _opts())
    runs = np.concatenate([found] * 8)[np.random.default_rng(5).permutation(len(found) * 8)]
    a = _cover_dev(id(w), w.rs, w.seqs, runs, seed=1)
    b = _cover_dev(id(w), w.rs, w.seqs, runs, seed=2)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    once = refset.cover_refset(w.seqs, w.rs, found, depth=True, host=True)
    assert np.array_equal(a[1], once[1] * 8) and np.array_equal(a[0]["n_anchors"], once[0]["n_anchors"] * 8)
    assert np.array_equal(a[0]["covered"], once[0]["covered"]) and np.array_equal(a[0]["n_segments"], once[0]["n_segments"])
    c, d, _ = refset.cover_refset(w.seqs, w.rs, runs, depth=True)
    assert c.tobytes() == a[0].tobytes() and d.tobytes() == a[1].tobytes()


def test_the_python_wrapper_and_capacity_0():
    import torch
    w = world(31, True)
    d_q, d_off, dev, total = _on_device(id(w), w.rs, w.seqs)
    runs = refset.find_refset(w.seqs, w.rs, _opts())
    host = refset.cover_refset(w.seqs, w.rs, runs, depth=True, host=True)
    rec, count = refset.find_refset_dev(d_q, d_off, w.rs, _opts(), capacity=len(runs) + 3)
    covers, depth = refset.cover_refset_dev(d_q[:total], d_off, w.rs, rec, count, len(runs) + 3, depth=True)  # (a batch tensor without slack)
    only, none = refset.cover_refset_dev(d_q, d_off, w.rs, rec, count, len(runs) + 3)
    torch.cuda.synchronize()
    assert covers.shape == (len(w.refs), 12) and none is None
    assert covers.cpu().numpy().tobytes() == host[0].tobytes() == only.cpu().numpy().tobytes() and depth.cpu().numpy().tobytes() == host[1].tobytes()
    zero, _ = refset.cover_refset_dev(d_q, d_off, w.rs, rec, count, 0)
    torch.cuda.synchronize()
    assert zero.cpu().numpy().tobytes() == refset.cover_refset(w.seqs, w.rs, runs[:0], host=True).tobytes()
