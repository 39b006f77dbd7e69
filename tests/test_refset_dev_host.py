"""kbo_find_refset_dev / kbo_summary_refset_dev, their *_work_bytes and kbo_refset_lds_only (kbo_hip.h) on the host: the symbols, the
scratch figures and every documented argument error - all of which come back before the first HIP call, so the device pointers are
dummy integers, suitably aligned, that nothing ever follows.  The planner's index arithmetic (kbo_amd/csrc/refset_plan.hpp) runs as a
stand-alone program under AddressSanitizer and UBSan next to the host's own plan (tools/refset_plan_check.cpp)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import kbo_amd
from kbo_amd import _capi, refset

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_EMPTY_QUERY, E_THRESHOLD_LE_1, E_BAD_ARG, E_UNSUPPORTED = -1, -3, -4, -8
Q, OFF, WORK, OUT, CNT = 0x10000, 0x20000, 0x30000, 0x50000, 0x60000
NEW_SYMBOLS = ["kbo_refset_lds_only", "kbo_find_refset_dev_work_bytes", "kbo_find_refset_dev", "kbo_summary_refset_dev_work_bytes",
               "kbo_summary_refset_dev"]
K = 31


def _rnd(rng, n):
    return np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)].tobytes()


@pytest.fixture(scope="module")
def rs():
    rng = np.random.default_rng(5)
    return refset.RefSet.build([_rnd(rng, n) for n in (K, K - 1, 40, 300, 1500)], kbo_amd.BuildOpts(k=K))


@pytest.fixture(scope="module")
def rs_own():
    """one reference of 16 400 bases: 16 401 rows, over KBO_REFSET_MAX_ROWS - the single-index route"""
    rng = np.random.default_rng(6)
    return refset.RefSet.build([_rnd(rng, 300), _rnd(rng, 16400)], kbo_amd.BuildOpts(k=K))


def test_symbols_are_exported_and_declared():
    L = kbo_amd.lib()
    hdr = open(os.path.join(ROOT, "include", "kbo_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert getattr(L, name) is not None and name in _capi.SYMBOLS
        assert re.search(r"\b%s\(" % name, hdr), name
    assert kbo_amd.find_refset_dev is refset.find_refset_dev and kbo_amd.summary_refset_dev is refset.summary_refset_dev


def test_lds_only(rs, rs_own):
    assert rs.lds_only() is True and rs_own.lds_only() is False
    assert kbo_amd.lib().kbo_refset_lds_only(None) == 0


@pytest.mark.parametrize("form", ["find", "summary"])
def test_work_bytes_are_monotonic(rs, form):
    L = kbo_amd.lib()
    wb = L.kbo_find_refset_dev_work_bytes if form == "find" else L.kbo_summary_refset_dev_work_bytes
    n_q = 4  # (the reference of k - 1 bases cannot be queried)
    for n_seqs, total in ((1, 3), (7, 70000), (300, 1500), (2, 0)):
        for strands in (1, 2, 3):
            by_refs = [int(wb(rs._h, n_seqs, total, strands, 1000, r)) for r in range(1, n_q + 3)]
            assert by_refs[0] > 0 and all(v % 16 == 0 for v in by_refs)
            assert all(a <= b for a, b in zip(by_refs, by_refs[1:]))
            if total:
                assert all(a < b for a, b in zip(by_refs[:n_q - 1], by_refs[1:n_q])), "a slab of more references holds more bytes"
            # beyond the queryable references a slab cannot grow, and 0 asks for as many as there are
            assert by_refs[n_q - 1] == by_refs[n_q] == by_refs[n_q + 1] == int(wb(rs._h, n_seqs, total, strands, 1000, 0))
            by_cap = [int(wb(rs._h, n_seqs, total, strands, c, 2)) for c in (0, 1, 10, 1000, 1 << 20, 1 << 40)]
            assert all(a <= b for a, b in zip(by_cap, by_cap[1:]))
            if form == "find" and total > 100:
                assert by_cap[0] < by_cap[1] < by_cap[2] < by_cap[3]
        assert wb(rs._h, n_seqs, total, 3, 10, 1) >= wb(rs._h, n_seqs, total, 1, 10, 1)
    # what the call refuses has no figure
    assert wb(None, 1, 3, 3, 10, 1) == 0 and wb(rs._h, 0, 0, 3, 10, 1) == 0
    assert wb(rs._h, 1, 3, 0, 10, 1) == 0 and wb(rs._h, 1, 3, 4, 10, 1) == 0
    assert wb(rs._h, 1 << 27, 1 << 27, 3, 10, 1) == 0 and wb(rs._h, 1 << 28, 1 << 28, 1, 10, 1) == 0
    assert wb(rs._h, 1, (1 << 32) - 16, 1, 10, 1) == 0 and wb(rs._h, 1, (1 << 31) - 8, 3, 10, 1) == 0


def _caller(L, form, h, n_seqs, total, capacity=100):
    """the entry point of `form` with dummy device pointers; its figure for one reference a slab"""
    find = form == "find"
    wb_fn = L.kbo_find_refset_dev_work_bytes if find else L.kbo_summary_refset_dev_work_bytes
    wb1 = int(wb_fn(h, n_seqs, total, 3, capacity, 1))

    def call(h=h, q=Q, off=OFF, n_seqs=n_seqs, total=total, prob=1e-7, strands=3, work=WORK, work_bytes=wb1, out=OUT, capacity=capacity, cnt=CNT):
        if find:
            o = _capi.FindOpts(prob, 0)
            return L.kbo_find_refset_dev(h, q, off, n_seqs, total, C.byref(o), strands, work, work_bytes, out, capacity, cnt, None)
        return L.kbo_summary_refset_dev(h, q, off, n_seqs, total, prob, strands, work, work_bytes, out, capacity, cnt, None)
    return call, wb1


@pytest.mark.parametrize("form", ["find", "summary"])
def test_argument_errors_need_no_device(rs, rs_own, form):
    L = kbo_amd.lib()
    call, wb1 = _caller(L, form, rs._h, 4, 1000)
    assert wb1 > 0
    for null in ("h", "q", "off", "work", "cnt", "out"):
        assert call(**{null: None}) == E_BAD_ARG, null
    for name, base, step in (("q", Q, 8), ("q", Q, 1), ("off", OFF, 4), ("work", WORK, 8), ("cnt", CNT, 4), ("out", OUT, 2)):
        assert call(**{name: base + step}) == E_BAD_ARG, (name, step)
    for strands in (0, 4, -1):
        assert call(strands=strands) == E_BAD_ARG
    for prob in (0.0, 1.5, -1e-7):
        assert call(prob=prob) == E_BAD_ARG
    assert call(n_seqs=0) == E_EMPTY_QUERY
    assert call(prob=1.0) == E_THRESHOLD_LE_1  # (every string is a random match then: the host calls fail so)
    assert call(work_bytes=wb1 - 1) == E_BAD_ARG and call(work_bytes=0) == E_BAD_ARG
    assert call(strands=3, work_bytes=_caller(L, form, rs._h, 4, 1000)[1] - 16) == E_BAD_ARG
    # the limits: a slab of one reference of 2^32 - 16 bytes or more, 2^28 (sequence, strand) pairs or more
    assert call(total=(1 << 32) - 16, strands=1, work_bytes=1 << 60) == E_UNSUPPORTED
    assert call(total=(1 << 31) - 8, strands=3, work_bytes=1 << 60) == E_UNSUPPORTED
    assert call(n_seqs=1 << 28, total=1 << 28, strands=1, work_bytes=1 << 60) == E_UNSUPPORTED
    assert call(n_seqs=1 << 27, total=1 << 27, strands=3, work_bytes=1 << 60) == E_UNSUPPORTED
    # a set with a reference of the single-index route, whatever else is right
    own, wb_own = _caller(L, form, rs_own._h, 4, 1000)
    assert own(work_bytes=1 << 30) == E_UNSUPPORTED
    # a NULL output is an error only with room asked for
    assert call(out=None, capacity=1) == E_BAD_ARG


def test_plan_arithmetic_under_sanitizers(tmp_path):
    """tools/refset_plan_check.cpp: pairs, items and tasks from refset_plan.hpp's closed forms against SlabWalker::add_pair's loop"""
    exe = str(tmp_path / "refset_plan_check")
    subprocess.run(["c++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I",
                    os.path.join(ROOT, "kbo_amd", "csrc"), os.path.join(ROOT, "tools", "refset_plan_check.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "slabs agree" in run.stdout
