"""kbo_refset_candidates_dev and kbo_find / summary / best_refset_screened_dev (kbo_hip.h "The SCREENED device forms") on the host:
the symbols, the scratch figures and every documented argument error - all of which come back before the first HIP call, so the device
pointers are dummy integers, suitably aligned, that nothing ever follows.  The planner's index arithmetic
(kbo_amd/csrc/refset_cand.hpp) runs as a stand-alone program under AddressSanitizer and UBSan next to the host's own plan over the
candidate pairs and next to brute force (tools/refset_cand_check.cpp).  No GPU."""
import ctypes as C
import os
import re
import subprocess

import pytest

import kbo_amd
from kbo_amd import _capi, refset

from test_refset_screen_host import world

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_EMPTY_QUERY, E_THRESHOLD_LE_1, E_BAD_ARG, E_UNSUPPORTED = -1, -3, -4, -8
Q, OFF, WORK, OUT, CNT, BITS, STATS = 0x10000, 0x20000, 0x30000, 0x50000, 0x60000, 0x70000, 0x80000
MIXED_ROWS = 20000  # between the rows of the two long references: one is wide, the other takes the single-index route
FORMS = ("find", "summary", "best")
NEW_SYMBOLS = ["kbo_refset_candidates_dev_work_bytes", "kbo_refset_candidates_dev"]
NEW_SYMBOLS += ["kbo_%s_refset_screened_dev%s" % (f, t) for f in FORMS for t in ("", "_work_bytes")]


@pytest.fixture(scope="module")
def w():
    return world(31, False)


def test_symbols_are_exported_and_declared():
    L = kbo_amd.lib()
    hdr = open(os.path.join(ROOT, "include", "kbo_hip.h")).read()
    rust = open(os.path.join(ROOT, "bindings", "rust", "kbo-hip", "src", "lib.rs")).read()
    for name in NEW_SYMBOLS:
        assert getattr(L, name) is not None and name in _capi.SYMBOLS
        assert re.search(r"\b%s\(" % name, hdr), name
        assert re.search(r"pub fn %s\(" % name, rust), name
    assert re.search(r"uint64_t n_candidates, candidate_bases, n_walked, walked_bases;\s*\} kbo_refset_screen_stats;", hdr)
    assert callable(refset.RefSet.candidates_dev)


def _wb(L, form, h, n_seqs, total, strands, capacity, max_pairs, max_bases):
    if form == "best":
        return int(L.kbo_best_refset_screened_dev_work_bytes(h, n_seqs, total, strands, max_pairs, max_bases))
    fn = L.kbo_find_refset_screened_dev_work_bytes if form == "find" else L.kbo_summary_refset_screened_dev_work_bytes
    return int(fn(h, n_seqs, total, strands, capacity, max_pairs, max_bases))


@pytest.mark.parametrize("form", FORMS)
def test_work_bytes_are_exactly_monotonic_and_zero_for_what_is_refused(w, form):
    L = kbo_amd.lib()
    h = w.rs._h
    for n_seqs, total in ((1, 3), (21, 70000), (300, 1500), (2, 0)):
        for strands in (1, 2, 3):
            by_pairs = [_wb(L, form, h, n_seqs, total, strands, 1000, mp, 50000) for mp in (1, 2, 17, 1024, 1025, 100000, (1 << 28) - 1)]
            assert by_pairs[0] > 0 and all(v % 16 == 0 for v in by_pairs)
            assert all(a <= b for a, b in zip(by_pairs, by_pairs[1:]))
            strict = strands != 2  # ('-' alone lies at least a strand's bytes into d_work: small scratch in front of it is padded)
            assert not strict or all(a < b for a, b in zip(by_pairs, by_pairs[1:])), "more pairs, more scratch"
            by_bases = [_wb(L, form, h, n_seqs, total, strands, 1000, 100, mb) for mb in (0, 1, 300, 5000, 1 << 20, (1 << 32) - 17)]
            assert all(a <= b for a, b in zip(by_bases, by_bases[1:])) and by_bases[3] < by_bases[4] < by_bases[5]
            assert not strict or by_bases[0] < by_bases[2] < by_bases[3]
            by_cap = [_wb(L, form, h, n_seqs, total, strands, c, 100, 5000) for c in (0, 1, 10, 1000, 1 << 20, 1 << 40)]
            assert all(a <= b for a, b in zip(by_cap, by_cap[1:]))
            if form == "find" and strict:
                assert by_cap[0] < by_cap[1] < by_cap[2] < by_cap[3]
            cand = int(L.kbo_refset_candidates_dev_work_bytes(h, n_seqs, total, strands))
            assert 0 < cand <= by_pairs[0] and cand % 16 == 0
        assert _wb(L, form, h, n_seqs, total, 3, 10, 5, 500) >= _wb(L, form, h, n_seqs, total, 1, 10, 5, 500)
    # what the call refuses has no figure
    ok = dict(h=h, n_seqs=21, total=70000, strands=3, capacity=10, max_pairs=5, max_bases=500)

    def wb(**kw):
        a = dict(ok, **kw)
        return _wb(L, form, a["h"], a["n_seqs"], a["total"], a["strands"], a["capacity"], a["max_pairs"], a["max_bases"])
    assert wb() > 0
    assert wb(h=None) == 0 and wb(h=w.plain._h) == 0 and wb(h=world(31, False, MIXED_ROWS).rs._h) == 0
    assert wb(n_seqs=0, total=0) == 0 and wb(strands=0) == 0 and wb(strands=4) == 0
    assert wb(max_pairs=0) == 0 and wb(max_pairs=1 << 28) == 0 and wb(max_bases=(1 << 32) - 16) == 0
    assert wb(n_seqs=1 << 26, total=1 << 26, strands=1) == 0  # a bitmap of 19 x 2^26 x 2 bits
    assert wb(total=1 << 31, strands=1) == 0 and wb(total=(1 << 31) - 8, strands=3) == 0
    L2 = L.kbo_refset_candidates_dev_work_bytes
    assert L2(None, 21, 70000, 3) == 0 and L2(w.plain._h, 21, 70000, 3) == 0 and L2(h, 0, 0, 3) == 0 and L2(h, 21, 70000, 5) == 0
    assert L2(h, 1 << 26, 1 << 26, 1) == 0


def _caller(L, form, h, n_seqs=21, total=70000, capacity=100, max_pairs=50, max_bases=20000):
    """the entry point of `form` with dummy device pointers; its figure"""
    if form == "candidates":
        wb1 = int(L.kbo_refset_candidates_dev_work_bytes(h, n_seqs, total, 3))
    else:
        wb1 = _wb(L, form, h, n_seqs, total, 3, capacity, max_pairs, max_bases)

    def call(h=h, q=Q, off=OFF, n_seqs=n_seqs, total=total, prob=1e-7, strands=3, work=WORK, work_bytes=wb1, out=OUT, capacity=capacity, cnt=CNT,
             max_pairs=max_pairs, max_bases=max_bases, stats=STATS):
        if form == "candidates":
            return L.kbo_refset_candidates_dev(h, q, off, n_seqs, total, prob, strands, work, work_bytes, out, stats, None)
        if form == "find":
            o = _capi.FindOpts(prob, 0)
            return L.kbo_find_refset_screened_dev(h, q, off, n_seqs, total, C.byref(o), strands, work, work_bytes, out, capacity, cnt, max_pairs,
                                                  max_bases, stats, None)
        if form == "summary":
            return L.kbo_summary_refset_screened_dev(h, q, off, n_seqs, total, prob, strands, work, work_bytes, out, capacity, cnt, max_pairs,
                                                     max_bases, stats, None)
        return L.kbo_best_refset_screened_dev(h, q, off, n_seqs, total, prob, strands, work, work_bytes, out, max_pairs, max_bases, stats, None)
    return call, wb1


@pytest.mark.parametrize("form", ("candidates",) + FORMS)
def test_argument_errors_and_their_order_need_no_device(w, form):
    L = kbo_amd.lib()
    records = form in ("find", "summary")
    call, wb1 = _caller(L, form, w.rs._h)
    assert wb1 > 0
    # those of the unscreened device forms
    for null in ("h", "q", "off", "work", "stats", "out") + (("cnt",) if records else ()):
        assert call(**{null: None}) == E_BAD_ARG, null
    aligned = [("q", Q, 8), ("q", Q, 1), ("off", OFF, 4), ("work", WORK, 8), ("stats", STATS, 4), ("out", OUT, 2)]
    for name, base, step in aligned + ([("cnt", CNT, 4)] if records else []):
        assert call(**{name: base + step}) == E_BAD_ARG, (name, step)
    for strands in (0, 4, -1):
        assert call(strands=strands) == E_BAD_ARG
    for prob in (0.0, 1.5, -1e-7):
        assert call(prob=prob) == E_BAD_ARG
    assert call(n_seqs=0) == E_EMPTY_QUERY
    assert call(prob=1.0) == E_THRESHOLD_LE_1
    if records:
        assert call(out=None, capacity=1) == E_BAD_ARG  # a NULL output is an error only with room asked for
    # the screened forms' own
    plain, _ = _caller(L, form, w.plain._h)
    assert plain(work_bytes=1 << 40) == E_BAD_ARG                      # a set without a prefilter
    assert call(work_bytes=wb1 - 1) == E_BAD_ARG and call(work_bytes=0) == E_BAD_ARG
    mixed, _ = _caller(L, form, world(31, False, MIXED_ROWS).rs._h)
    assert mixed(work_bytes=1 << 40) == E_UNSUPPORTED                  # a reference of the single-index route
    assert call(n_seqs=1 << 26, total=1 << 26, strands=1, work_bytes=1 << 60) == E_UNSUPPORTED  # a bitmap of more than 2^31 bits
    assert call(total=1 << 31, strands=1, work_bytes=1 << 60) == E_UNSUPPORTED
    assert call(total=(1 << 31) - 8, strands=3, work_bytes=1 << 60) == E_UNSUPPORTED
    if form != "candidates":
        assert call(max_pairs=0, work_bytes=1 << 60) == E_BAD_ARG
        assert call(max_pairs=1 << 28, work_bytes=1 << 60) == E_UNSUPPORTED
        assert call(max_bases=(1 << 32) - 16, work_bytes=1 << 60) == E_UNSUPPORTED
        assert call(max_pairs=51) == E_BAD_ARG and call(max_bases=1 << 20) == E_BAD_ARG  # (the figure is for 50 pairs and 20 000 bases)
        assert mixed(max_pairs=0, work_bytes=1 << 40) == E_BAD_ARG     # max_pairs == 0 before the set's routes
    # the order: strands, then the empty batch, then the prefilter, then the thresholds, then the routes, the bitmap and the caps,
    # and work_bytes last
    assert plain(strands=0, n_seqs=0) == E_BAD_ARG and plain(n_seqs=0) == E_EMPTY_QUERY
    plain_mixed, _ = _caller(L, form, world(31, False, MIXED_ROWS).plain._h)
    assert plain_mixed(work_bytes=1 << 40) == E_BAD_ARG
    assert plain(prob=1.0) == E_BAD_ARG and mixed(prob=1.0) == E_THRESHOLD_LE_1
    assert call(n_seqs=1 << 26, total=1 << 26, strands=1, work_bytes=0) == E_UNSUPPORTED
    assert mixed(work_bytes=0) == E_UNSUPPORTED


def test_cand_arithmetic_under_sanitizers(tmp_path):
    """tools/refset_cand_check.cpp: rank, the cut by the caps, item to pair and task to reference from refset_cand.hpp against
    run_slabs / add_pair's loop over the candidate pairs and against brute force"""
    exe = str(tmp_path / "refset_cand_check")
    subprocess.run(["c++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I",
                    os.path.join(ROOT, "kbo_amd", "csrc"), os.path.join(ROOT, "tools", "refset_cand_check.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "calls agree" in run.stdout
