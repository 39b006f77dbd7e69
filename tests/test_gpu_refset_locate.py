"""kbo_locate_refset / kbo_locate_refset_dev (kbo_hip.h "The LOCUS of a run") on the GPU against brute force.

The yardstick is tests/test_refset_locate_host.py's: a dict from every k-mer of every indexed stretch of a reference (and of the
reverse complements when add_revcomp is set) to its occurrences, and a scan of [start, end - k] of every run for its first and last
anchor - nothing from the library's walk.  All comparisons are exact and cover every record.  The set - twelve references of 300 to
2 000 bases, one of 20 kbp on the wide route, one without a k-mer - the contigs and every planted case are that file's world(), which
its own tests check on the CPU first (kbo_locate_refset_host against the same brute force, and that every case occurs); the last test
here counts the cases again in what the GPU returned."""
import numpy as np
import pytest

import kbo_amd
from kbo_amd import refset

from gpu_helpers import Guarded
from test_refset_locate_host import GAP, NONE, SHORT, WIDE, assert_reached, make_refs, world

pytestmark = pytest.mark.gpu

UNUSABLE = 16
CASES = [(31, False), (31, True), (96, False), (96, True)]


def _opts():
    return kbo_amd.FindOpts(max_gap_len=GAP)


def _words(a):
    return np.ascontiguousarray(a).view(np.uint32).reshape(len(a), -1)


def _no_tested(loci):
    return [tuple(v)[:5] for v in loci]


_device = {}


def _on_device(w):
    """the set's copy and the batch on the current device, once per world"""
    import torch
    if id(w) not in _device:
        w.rs.to_device()
        dev = torch.device("cuda", torch.cuda.current_device())
        total = int(w.offsets[-1])
        q = np.zeros(total + 16, dtype=np.uint8)
        q[:total] = np.concatenate(w.seqs)
        _device[id(w)] = (torch.from_numpy(q).to(dev), torch.from_numpy(w.offsets.astype(np.int64)).to(dev), dev)
    return _device[id(w)]


@pytest.mark.parametrize("prefilter", [False, True])
@pytest.mark.parametrize("k,rc", CASES)
def test_locate_over_find_equals_brute_force_and_the_host_form(k, rc, prefilter):
    w = world(k, rc, prefilter)
    assert w.rs.has_positions() and w.rs.has_prefilter == prefilter and w.rs.packed_only()
    for strands in (1, 2, 3):
        runs = refset.find_refset(w.seqs, w.rs, _opts(), strands=strands)
        assert len(runs) > (40 if strands & 1 or rc else 2)
        loci = refset.locate_refset(w.seqs, w.rs, runs)
        exp = w.expected(runs)
        assert _no_tested(loci) == _no_tested(exp)  # every field of every record but the work count
        host = refset.locate_refset(w.seqs, w.rs, runs, host=True)
        assert np.array_equal(_words(loci), _words(host))  # ... and that one too: the serial form hands out the same windows
        assert not (loci["flags"] & UNUSABLE).any()
        if strands == 3:
            assert np.array_equal(_words(runs), _words(w.cpu_runs()))  # the runs the CPU checks of the fixtures went by
            runs2, loci2 = refset.find_refset(w.seqs, w.rs, _opts(), locate=True)
            assert np.array_equal(_words(runs2), _words(runs)) and np.array_equal(_words(loci2), _words(loci))
    assert len(refset.locate_refset(w.seqs, w.rs, runs[:0])) == 0


@pytest.mark.parametrize("short", [False, True])
@pytest.mark.parametrize("screened", [False, True])
@pytest.mark.parametrize("k,rc", CASES)
def test_find_dev_then_locate_dev_on_one_stream(k, rc, screened, short):
    """kbo_find_refset_dev / kbo_find_refset_screened_dev and kbo_locate_refset_dev enqueued back to back, nothing read in between:
    the loci are the host form's, only the first `capacity` are written, and the bytes around d_loci are as they were"""
    import torch
    w = world(k, rc, screened)
    d_q, d_off, dev = _on_device(w)
    runs = refset.find_refset(w.seqs, w.rs, _opts())
    host = refset.locate_refset(w.seqs, w.rs, runs, host=True)
    capacity = len(runs) - 7 if short else len(runs) + 9
    s = torch.cuda.Stream(device=dev)
    loci = Guarded("d_loci", capacity * 24, 1 << 16, dev, seed=k + capacity)
    torch.cuda.synchronize()
    if screened:
        rec, count, stats = refset.find_refset_dev(d_q, d_off, w.rs, _opts(), capacity=capacity, stream=s, screened=True, max_pairs=4096,
                                                   max_pair_bases=1 << 22)
    else:
        rec, count = refset.find_refset_dev(d_q, d_off, w.rs, _opts(), capacity=capacity, stream=s)
    kbo_amd.check(kbo_amd.lib().kbo_locate_refset_dev(w.rs._h, d_q.data_ptr(), d_off.data_ptr(), len(w.seqs), int(w.offsets[-1]), rec.data_ptr(),
                                                      count.data_ptr(), capacity, loci.ptr, s.cuda_stream))
    torch.cuda.synchronize()
    n = min(len(runs), capacity)
    assert int(count.item()) == len(runs)
    if screened:
        assert int(stats[2]) == int(stats[0]) > 0  # every candidate pair was walked: the records are complete
    assert np.array_equal(rec[:n].cpu().numpy().view(np.uint32), _words(runs)[:n])
    loci.assert_intact("locate")
    got = loci.host().view(np.uint32).reshape(capacity, 6)
    assert np.array_equal(got[:n], _words(host)[:n])
    if not short:  # nothing behind the count either
        assert np.array_equal(loci.buf[n * 24:].cpu().numpy(), loci.image[loci.front + n * 24:loci.front + loci.n].cpu().numpy())


def test_the_python_wrapper_and_capacity_0():
    import torch
    w = world(31, True)
    d_q, d_off, dev = _on_device(w)
    runs = refset.find_refset(w.seqs, w.rs, _opts())
    host = refset.locate_refset(w.seqs, w.rs, runs, host=True)
    rec, count = refset.find_refset_dev(d_q, d_off, w.rs, _opts(), capacity=len(runs) + 3)
    loci = refset.locate_refset_dev(d_q[:int(w.offsets[-1])], d_off, w.rs, rec, count, len(runs) + 3)  # (a batch tensor without slack)
    torch.cuda.synchronize()
    assert loci.shape == (len(runs) + 3, 6) and np.array_equal(loci[:len(runs)].cpu().numpy().view(np.uint32), _words(host))
    none = refset.locate_refset_dev(d_q, d_off, w.rs, rec, count, 0)
    torch.cuda.synchronize()
    assert none.shape == (0, 6)


def _locate_dev(w, rs, runs, n_seqs=None, count=None):
    """kbo_locate_refset_dev over hand-made records -> the loci"""
    import torch
    d_q, d_off, dev = _on_device(w)
    d_runs = torch.from_numpy(_words(runs).view(np.int32).copy()).to(dev)
    d_n = torch.tensor([len(runs) if count is None else count], dtype=torch.int64, device=dev)
    loci = Guarded("d_loci", len(runs) * 24, 1 << 16, dev, seed=len(runs))
    s = torch.cuda.current_stream(dev)
    kbo_amd.check(kbo_amd.lib().kbo_locate_refset_dev(rs._h, d_q.data_ptr(), d_off.data_ptr(), len(w.seqs) if n_seqs is None else n_seqs,
                                                      int(w.offsets[-1]), d_runs.data_ptr(), d_n.data_ptr(), len(runs), loci.ptr, s.cuda_stream))
    torch.cuda.synchronize()
    loci.assert_intact("locate")
    return loci.host().view(refset.REF_LOCUS).copy()


def test_unusable_records_get_bit_4_and_leave_the_others_alone():
    """records the contract defines as unusable, one per condition, among good ones: bit 4 and NONE for them, the good ones as ever"""
    w = world(31, True)
    found = refset.find_refset(w.seqs, w.rs, _opts())
    good = np.concatenate([found[:36], found[found["ref"] == WIDE][:4]])  # (some on the wide reference, for the last part)
    assert len(good) == 40
    host = refset.locate_refset(w.seqs, w.rs, good, host=True)
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
    got = _locate_dev(w, w.rs, runs)
    for x in range(len(runs)):
        if x in unusable:
            assert tuple(got[x]) == (NONE, NONE, NONE, NONE, UNUSABLE, 0), (x, got[x])
        else:
            assert tuple(got[x]) == tuple(host[x]), x
    # a count beyond the capacity writes `capacity` records; a count of 0 none
    assert np.array_equal(_words(_locate_dev(w, w.rs, good, count=1 << 40)), _words(host))
    # the batch seen with fewer sequences: the records of the others are unusable
    fewer = _locate_dev(w, w.rs, good, n_seqs=2)
    for x in range(len(good)):
        assert tuple(fewer[x]) == (tuple(host[x]) if good["seq"][x] < 2 else (NONE, NONE, NONE, NONE, UNUSABLE, 0))
    # a reference of the single-index route
    refs = make_refs(31, 7031)
    mixed = refset.RefSet.build(refs, kbo_amd.BuildOpts(k=31, add_revcomp=True, num_threads=4), wide_rows=refset.MAX_ROWS, positions=True)
    assert mixed.route(WIDE) == refset.ROUTE_INDEX
    mixed.to_device()
    got = _locate_dev(w, mixed, good)
    on_wide = good["ref"] == WIDE
    assert on_wide.any() and not on_wide.all()
    for x in range(len(good)):
        assert tuple(got[x]) == ((NONE, NONE, NONE, NONE, UNUSABLE, 0) if on_wide[x] else tuple(host[x]))


@pytest.mark.parametrize("k,rc", [(31, True), (96, False)])
def test_hand_made_runs_at_the_lane_and_window_boundaries(k, rc):
    """runs laid by hand around planted copies so that the first anchor lies 0, 1, 63, 64, 65, 127, 128, 129 and 130 windows behind
    run.start and the last as many in front of run.end - k - and every pair of them - through both forms, against brute force"""
    w = world(k, rc)
    found = refset.find_refset(w.seqs, w.rs, _opts())
    loci = refset.locate_refset(w.seqs, w.rs, found, host=True)
    clean = [x for x in range(len(found)) if loci["q_first"][x] == found["start"][x] and loci["q_last"][x] + k == found["end"][x]]
    steps = (0, 1, 63, 64, 65, 127, 128, 129, 130)
    made = []
    for x in clean[:12]:
        n = len(w.seqs[found["seq"][x]])
        for a in steps:
            for b in steps:
                if found["start"][x] >= a and found["end"][x] + b <= n:
                    made.append((found["ref"][x], found["seq"][x], found["strand"][x], found["start"][x] - a, found["end"][x] + b, 0, 0, 0, 0, 0))
    runs = np.array(made, dtype=refset.REF_RUN)
    assert len(runs) > 500
    exp = w.expected(runs)
    lead = exp["q_first"].astype(np.int64) - runs["start"]
    trail = runs["end"].astype(np.int64) - k - exp["q_last"]
    for d in steps:  # (a chance k-mer in front of a copy would shorten one: each distance still occurs)
        assert (lead == d).any() and (trail == d).any(), d
    got = refset.locate_refset(w.seqs, w.rs, runs)
    assert np.array_equal(_words(got), _words(exp))
    assert np.array_equal(_words(got), _words(refset.locate_refset(w.seqs, w.rs, runs, host=True)))


@pytest.mark.parametrize("k,rc", CASES)
def test_the_planted_cases_were_really_reached(k, rc):
    """REV and MULTI anchors, runs without an anchor, first and last anchors beyond the first group of 64 windows, runs on the wide
    reference and the rest of test_refset_locate_host.reached(): counted in what the GPU returned"""
    w = world(k, rc)
    runs = refset.find_refset(w.seqs, w.rs, _opts())
    loci = refset.locate_refset(w.seqs, w.rs, runs)
    assert_reached(k, rc, runs, loci)
    last = len(w.seqs) - 1
    assert ((runs["seq"] == last) & (runs["strand"] == 1) & (runs["end"] == len(w.seqs[last]))).any()  # the slack bytes
    assert (runs["ref"] == WIDE).any() and w.rs.route(WIDE) == refset.ROUTE_WIDE
