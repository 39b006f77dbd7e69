"""The seed screen of a reference set on the device (kbo_hip.h "A set with a PREFILTER"; kbo_amd/csrc/refset_screen_kernels.hip).

  - kbo_refset_candidates is bit for bit kbo_refset_candidates_host - and, at the default max_error_prob, the contract by brute force -
    over the world of tests/test_refset_screen_host.py: one contig holds exactly m_r bases of a reference across the boundary between
    two workgroups of the kernel, and exactly m_r bases of another across the boundary between two lanes, so those two bits are set
    only by a lane that reads behind its own positions;
  - kbo_find_refset, kbo_summary_refset and kbo_best_refset return the same bytes from the set with the prefilter and from the set
    without it, over several slabs, and the counters say that only the candidates were walked;
  - a batch without a candidate, the fall-back above the bitmap's cap, and the device forms, which ignore the prefilter."""
import numpy as np
import pytest

import kbo_amd
from kbo_amd import refset

from test_refset_screen_host import BIG, BIG_AT, N_UNRELATED, PROBS, WIDE_A, WIDE_B, expected, lane_run, lane_threads, world

pytestmark = pytest.mark.gpu

DEFAULT_SLAB = 16 << 20
SMALL_SLAB = 1 << 16  # the least kbo_set_slab_bytes takes: the ten candidate pairs of the 16 kbp contig alone are more than two of it
MIXED_ROWS = 20000  # between the rows of the two long references: one is wide, the other takes the single-index route


def _calls(rs, seqs, prob, strands):
    """the records of the four calls as bytes, and the prefilter's counters and the slabs of each"""
    out, counters = {}, {}
    for name, f in (("find0", lambda: refset.find_refset(seqs, rs, kbo_amd.FindOpts(max_error_prob=prob, max_gap_len=0), strands)),
                    ("find5", lambda: refset.find_refset(seqs, rs, kbo_amd.FindOpts(max_error_prob=prob, max_gap_len=5), strands)),
                    ("summary", lambda: refset.summary_refset(seqs, rs, prob, strands)),
                    ("best", lambda: refset.best_refset(seqs, rs, prob, strands))):
        rec = f()
        out[name] = rec
        counters[name] = (refset.last_prefilter(), refset.last_routes())
    return out, counters


@pytest.mark.parametrize("k,rc", [(31, False), (31, True), (96, False)])
def test_the_bitmap_is_the_hosts(k, rc):
    w = world(k, rc)
    run, group = lane_run(), lane_run() * lane_threads()
    # where the two planted seeds lie: across a workgroup's boundary, and across a lane's inside a workgroup
    for r, cut in ((0, (BIG_AT // group + 1) * group), (1, ((BIG_AT + 3000) // run + 1) * run)):
        m = w.m[1e-7][r]
        at = cut - m // 2 - BIG_AT
        assert np.array_equal(w.seqs[BIG][at:at + m], w.refs[r][100:100 + m]) and at + BIG_AT < cut < at + BIG_AT + m
        assert cut % run == 0 and (cut % group == 0) == (r == 0)
    w.rs.to_device()
    for prob in PROBS:
        for strands in (3, 1, 2):
            host = w.rs.candidates(w.seqs, prob, strands, host=True)
            got = w.rs.candidates(w.seqs, prob, strands)
            assert np.array_equal(got, host), (prob, strands, np.argwhere(got != host)[:10])
    got = w.rs.candidates(w.seqs, 1e-7)
    assert np.array_equal(got, expected(w, 1e-7)) and got[0, BIG, 0] and got[1, BIG, 0] and not got[:, :N_UNRELATED].any()


@pytest.mark.parametrize("k,rc,wide_rows,strands", [(31, False, MIXED_ROWS, 3), (31, True, refset.WIDE_MAX_ROWS, 3),
                                                    (96, False, refset.WIDE_MAX_ROWS, 3), (31, False, MIXED_ROWS, 1)])
def test_records_are_the_same_and_only_candidates_are_walked(k, rc, wide_rows, strands):
    w = world(k, rc, wide_rows)
    routes = [w.rs.route(r) for r in range(len(w.refs))]
    assert refset.ROUTE_LDS in routes and refset.ROUTE_WIDE in routes
    assert (refset.ROUTE_INDEX in routes) == (wide_rows == MIXED_ROWS) and routes[WIDE_A] == refset.ROUTE_WIDE
    L = kbo_amd.lib()
    L.kbo_set_slab_bytes(SMALL_SLAB)
    try:
        plain, plain_counters = _calls(w.plain, w.seqs, 1e-7, strands)
        screened, counters = _calls(w.rs, w.seqs, 1e-7, strands)
    finally:
        L.kbo_set_slab_bytes(DEFAULT_SLAB)
    bits = w.rs.candidates(w.seqs, 1e-7, strands)
    n_packed = len(w.packed) * len(w.seqs) * (2 if strands == 3 else 1)
    for name in plain:
        assert len(plain[name]) > 0 and screened[name].tobytes() == plain[name].tobytes(), name
        pre, routes_of = counters[name]
        assert pre[3] == 1 and pre[2] == pre[1] == int(bits.sum()) < pre[0] == n_packed, (name, pre)
        assert routes_of[3] >= 3, "at least three slabs"
        assert plain_counters[name][0] == (n_packed, 0, n_packed, 0)
        # (every reference of the single-index route goes through its pipeline as before)
        assert routes_of[1] == plain_counters[name][1][1] == routes.count(refset.ROUTE_INDEX)
    # every pair with a record has its bit set
    for name in ("find0", "find5", "summary"):
        rec = screened[name]
        packed = np.isin(rec["ref"], w.packed)
        assert packed.any() and bits[rec["ref"][packed], rec["seq"][packed], rec["strand"][packed] - 1].all()
    best = screened["best"]
    hit = (best["ref"] != refset.REF_NONE) & np.isin(best["ref"], w.packed)
    assert hit.any() and bits[best["ref"][hit], best["seq"][hit], best["strand"][hit] - 1].all()
    if wide_rows == MIXED_ROWS:  # the single-index reference has records, and no bit
        assert (screened["summary"]["ref"] == WIDE_B).any() and not bits[WIDE_B].any()


def test_a_batch_without_a_candidate_runs_no_slab():
    w = world(31, False)
    seqs = w.seqs[:N_UNRELATED]
    plain, _ = _calls(w.plain, seqs, 1e-7, 3)
    screened, counters = _calls(w.rs, seqs, 1e-7, 3)
    for name in plain:
        assert screened[name].tobytes() == plain[name].tobytes(), name
        pre, routes = counters[name]
        assert pre == (len(w.packed) * N_UNRELATED * 2, 0, 0, 1) and routes == (0, 0, 0, 0), (name, pre, routes)
    assert len(screened["find0"]) == len(screened["find5"]) == len(screened["summary"]) == 0
    assert len(screened["best"]) == N_UNRELATED and (screened["best"]["ref"] == refset.REF_NONE).all()


def test_above_the_cap_the_call_runs_unscreened():
    w = world(31, False)
    n_packed = len(w.packed) * len(w.seqs) * 2
    plain, _ = _calls(w.plain, w.seqs, 1e-7, 3)
    assert len(w.refs) * len(w.seqs) * 2 > 64
    refset.set_prefilter_max_bits(64)
    try:
        capped, counters = _calls(w.rs, w.seqs, 1e-7, 3)
    finally:
        refset.set_prefilter_max_bits(0)
    for name in plain:
        assert capped[name].tobytes() == plain[name].tobytes(), name
        assert counters[name][0] == (n_packed, 0, n_packed, 0)
    again = refset.summary_refset(w.seqs, w.rs)
    assert again.tobytes() == plain["summary"].tobytes() and refset.last_prefilter()[3] == 1


def test_the_device_forms_ignore_the_prefilter():
    import torch
    w = world(31, False)
    assert w.rs.packed_only() and w.plain.packed_only()
    concat = np.concatenate(w.seqs)
    offsets = np.zeros(len(w.seqs) + 1, dtype=np.int64)
    offsets[1:] = np.cumsum([len(s) for s in w.seqs])
    d_q = torch.zeros(len(concat) + 16, dtype=torch.uint8, device="cuda:0")
    d_q[:len(concat)] = torch.from_numpy(concat).to("cuda:0")
    d_off = torch.from_numpy(offsets).to("cuda:0")
    got = {}
    for name, rs in (("plain", w.plain), ("prefilter", w.rs)):
        rs.to_device()
        found, n_found = refset.find_refset_dev(d_q, d_off, rs, kbo_amd.FindOpts(max_gap_len=5), capacity=4096)
        summary, n_summary = refset.summary_refset_dev(d_q, d_off, rs, capacity=4096)
        best = refset.best_refset_dev(d_q, d_off, rs)
        torch.cuda.synchronize()
        assert 0 < int(n_found.item()) <= 4096 and 0 < int(n_summary.item()) <= 4096
        got[name] = (found[:int(n_found.item())].cpu().numpy().tobytes(), summary[:int(n_summary.item())].cpu().numpy().tobytes(),
                     best.cpu().numpy().tobytes())
    assert got["plain"] == got["prefilter"]
    host = refset.summary_refset(w.seqs, w.rs)
    assert got["prefilter"][1] == host.tobytes()
