"""kbo_refset_build_wide and the wide route (kbo_hip.h "find against a set of references") on the host: the symbols, the routes at
both boundaries - the rows are the oracle's n_sets, asserted - the answers of kbo_refset_lds_only / kbo_refset_packed_only, the
device-resident calls' figures and refusals with dummy pointers, and the step the wide kernel runs (kbo_amd/csrc/refset_step.hpp)
restated on the CPU: kbo_refset_ms_host against the oracle's matching statistics over an oracle index of that reference alone, and
tools/refset_step_check.cpp, a stand-alone program under AddressSanitizer and UBSan whose accessor checks every index.  No GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import kbo_amd
from kbo_amd import _capi, refset
from oracle import binding as ora

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_BAD_ARG, E_UNSUPPORTED = -4, -8
MAX_ROWS, WIDE_MAX_ROWS = 16384, 1 << 20
Q, OFF, WORK, OUT, CNT = 0x10000, 0x20000, 0x30000, 0x50000, 0x60000
API = ["kbo_refset_build_wide", "kbo_refset_route", "kbo_refset_packed_only"]
HOOKS = ["kbo_refset_last_wide", "kbo_refset_form", "kbo_refset_ms_host"]
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
K = 31


def _rnd(rng, n):
    return ACGT[rng.integers(0, 4, n)].copy()


def _rows(ref, k=K, rc=False):
    return ora.Index.build([ref.tobytes()], k=k, add_revcomp=rc).n_sets


@pytest.fixture(scope="module")
def refs():
    """name -> sequence: 16 384 and 16 385 rows, 40 001 and 40 002 rows (the second boundary), small ones, one without a k-mer"""
    rng = np.random.default_rng(41)
    out = {"small": _rnd(rng, 300), "lds_max": _rnd(rng, 16383), "wide_min": _rnd(rng, 16384), "at_cap": _rnd(rng, 40000),
           "over_cap": _rnd(rng, 40001), "none": _rnd(rng, K - 1), "mid": _rnd(rng, 1500)}
    assert _rows(out["lds_max"]) == MAX_ROWS and _rows(out["wide_min"]) == MAX_ROWS + 1
    assert _rows(out["at_cap"]) == 40001 and _rows(out["over_cap"]) == 40002
    return out


ORDER = ["small", "lds_max", "wide_min", "none", "at_cap", "over_cap", "mid"]


def _build(refs, names, wide_rows, k=K, rc=False):
    return refset.RefSet.build([refs[n] for n in names], kbo_amd.BuildOpts(k=k, add_revcomp=rc, num_threads=3), wide_rows=wide_rows)


def test_symbols_are_exported_and_declared():
    L = kbo_amd.lib()
    api = open(os.path.join(ROOT, "include", "kbo_hip.h")).read()
    tuning = open(os.path.join(ROOT, "include", "kbo_hip_tuning.h")).read()
    for name in API:
        assert getattr(L, name) is not None and name in _capi.SYMBOLS
        assert re.search(r"\b%s\(" % name, api), name
    for name in HOOKS:
        assert getattr(L, name) is not None and name in _capi.TUNING_SYMBOLS
        assert re.search(r"\b%s\(" % name, tuning), name
    for method in ("route", "packed_only"):
        assert callable(getattr(refset.RefSet, method))
    assert callable(refset.last_wide)


def test_header_constants_are_the_kernels():
    api = open(os.path.join(ROOT, "include", "kbo_hip.h")).read()
    kern = open(os.path.join(ROOT, "kbo_amd", "csrc", "kernels.hpp")).read()
    assert re.search(r"#define KBO_REFSET_WIDE_MAX_ROWS \(1u << 20\)", api)
    assert re.search(r"constexpr uint32_t kRefsetWideMaxRows = 1u << 20;", kern)
    assert refset.WIDE_MAX_ROWS == WIDE_MAX_ROWS and refset.MAX_ROWS == MAX_ROWS
    routes = re.search(r"constexpr uint32_t kRefsetRouteLds = (\d+), kRefsetRouteIndex = (\d+), kRefsetRouteWide = (\d+);", kern)
    assert routes
    for name, value, py in zip(("LDS", "INDEX", "WIDE"), routes.groups(), (refset.ROUTE_LDS, refset.ROUTE_INDEX, refset.ROUTE_WIDE)):
        assert int(re.search(r"#define KBO_REFSET_ROUTE_%s (\d+)" % name, api).group(1)) == int(value) == py
    assert re.search(r"#define KBO_REFSET_ROUTE_NONE \(-1\)", api) and refset.ROUTE_NONE == -1


def test_max_wide_rows_outside_its_range_is_refused():
    L = kbo_amd.lib()
    seq = (C.c_char_p * 1)(b"ACGT" * 20)
    lens = (C.c_size_t * 1)(80)
    for bad in (0, 1, MAX_ROWS - 1, WIDE_MAX_ROWS + 1, 1 << 40):
        h = C.c_void_p(1)
        assert L.kbo_refset_build_wide(seq, lens, 1, None, bad, C.byref(h)) == E_BAD_ARG and not h.value, bad
    for good in (MAX_ROWS, MAX_ROWS + 1, WIDE_MAX_ROWS):
        h = C.c_void_p()
        assert L.kbo_refset_build_wide(seq, lens, 1, None, good, C.byref(h)) == 0 and h.value
        assert L.kbo_refset_route(h, 0) == refset.ROUTE_LDS
        L.kbo_refset_free(h)
    # the other whole-call errors are kbo_refset_build's
    h = C.c_void_p()
    assert L.kbo_refset_build_wide(None, lens, 1, None, MAX_ROWS, C.byref(h)) == E_BAD_ARG
    assert L.kbo_refset_build_wide(seq, lens, 0, None, MAX_ROWS, C.byref(h)) == E_BAD_ARG
    assert L.kbo_refset_build_wide(seq, lens, 1, None, MAX_ROWS, None) == E_BAD_ARG


def test_routes_by_rows_at_both_boundaries(refs):
    cap = _rows(refs["at_cap"])
    rs = _build(refs, ORDER, cap)
    want = {"small": refset.ROUTE_LDS, "lds_max": refset.ROUTE_LDS, "wide_min": refset.ROUTE_WIDE, "none": refset.ROUTE_NONE,
            "at_cap": refset.ROUTE_WIDE, "over_cap": refset.ROUTE_INDEX, "mid": refset.ROUTE_LDS}
    assert [rs.route(r) for r in range(len(ORDER))] == [want[n] for n in ORDER]
    assert rs.status(ORDER.index("none")) == E_BAD_ARG and all(rs.status(r) == 0 for r, n in enumerate(ORDER) if n != "none")
    for r, n in enumerate(ORDER):  # the indexes are what kbo_refset_build makes of them
        assert rs.n_kmers(r) == ora.Index.build([refs[n].tobytes()], k=K).n_kmers
    L = kbo_amd.lib()
    assert L.kbo_refset_route(rs._h, len(ORDER)) == E_BAD_ARG and L.kbo_refset_route(None, 0) == E_BAD_ARG
    # one row more of room: the reference over the cap is wide too
    rs2 = _build(refs, ORDER, cap + 1)
    assert rs2.route(ORDER.index("over_cap")) == refset.ROUTE_WIDE and rs2.packed_only()


def test_build_wide_at_the_lds_limit_is_build(refs):
    a, b = _build(refs, ORDER, None), _build(refs, ORDER, MAX_ROWS)
    routes = [a.route(r) for r in range(len(ORDER))]
    assert routes == [b.route(r) for r in range(len(ORDER))]
    assert routes == [refset.ROUTE_LDS, refset.ROUTE_LDS, refset.ROUTE_INDEX, refset.ROUTE_NONE, refset.ROUTE_INDEX, refset.ROUTE_INDEX,
                      refset.ROUTE_LDS]
    assert [a.n_kmers(r) for r in range(len(ORDER))] == [b.n_kmers(r) for r in range(len(ORDER))]
    assert a.lds_only() == b.lds_only() is False and a.packed_only() == b.packed_only() is False


def test_lds_only_and_packed_only_for_each_kind_of_set(refs):
    lds = _build(refs, ["small", "none", "lds_max"], WIDE_MAX_ROWS)
    wide = _build(refs, ["small", "none", "wide_min", "at_cap"], WIDE_MAX_ROWS)
    own = _build(refs, ["small", "wide_min", "over_cap"], _rows(refs["at_cap"]))
    assert (lds.lds_only(), lds.packed_only()) == (True, True)
    assert (wide.lds_only(), wide.packed_only()) == (False, True)
    assert (own.lds_only(), own.packed_only()) == (False, False)
    assert kbo_amd.lib().kbo_refset_packed_only(None) == 0
    # the hooks of the packed form refuse what has none
    n = C.c_size_t()
    L = kbo_amd.lib()
    assert L.kbo_refset_form(own._h, 2, None, C.byref(n)) == E_BAD_ARG and L.kbo_refset_form(lds._h, 1, None, C.byref(n)) == E_BAD_ARG
    assert L.kbo_refset_form(lds._h, 3, None, C.byref(n)) == E_BAD_ARG and L.kbo_refset_form(lds._h, 0, None, None) == E_BAD_ARG
    assert L.kbo_refset_ms_host(own._h, 2, None, 0, None) == E_BAD_ARG and L.kbo_refset_ms_host(wide._h, 2, None, 5, None) == E_BAD_ARG
    assert L.kbo_refset_last_wide(None) == E_BAD_ARG


def _dev_call(L, form, h, n_seqs, total, work_bytes, capacity=100):
    if form == "find":
        o = _capi.FindOpts(1e-7, 0)
        return L.kbo_find_refset_dev(h, Q, OFF, n_seqs, total, C.byref(o), 3, WORK, work_bytes, OUT, capacity, CNT, None)
    return L.kbo_summary_refset_dev(h, Q, OFF, n_seqs, total, 1e-7, 3, WORK, work_bytes, OUT, capacity, CNT, None)


@pytest.mark.parametrize("form", ["find", "summary"])
def test_dev_work_bytes_do_not_depend_on_the_routes(refs, form):
    L = kbo_amd.lib()
    wb = L.kbo_find_refset_dev_work_bytes if form == "find" else L.kbo_summary_refset_dev_work_bytes
    # three references that can be queried and one that cannot, in both sets
    lds = _build(refs, ["small", "none", "mid", "lds_max"], WIDE_MAX_ROWS)
    wide = _build(refs, ["small", "none", "wide_min", "at_cap"], WIDE_MAX_ROWS)
    assert lds.lds_only() and wide.packed_only() and not wide.lds_only()
    for n_seqs, total in ((1, 3), (7, 70000), (300, 1500)):
        for strands in (1, 2, 3):
            for capacity in (0, 1000):
                for per_slab in (0, 1, 2, 3, 5):
                    a = int(wb(wide._h, n_seqs, total, strands, capacity, per_slab))
                    assert a > 0 and a == int(wb(lds._h, n_seqs, total, strands, capacity, per_slab))


@pytest.mark.parametrize("form", ["find", "summary"])
def test_a_set_with_a_reference_of_the_single_index_route_is_still_refused(refs, form):
    L = kbo_amd.lib()
    wb = L.kbo_find_refset_dev_work_bytes if form == "find" else L.kbo_summary_refset_dev_work_bytes
    own = _build(refs, ["small", "wide_min", "over_cap"], _rows(refs["at_cap"]))
    plain = _build(refs, ["small", "wide_min"], None)  # kbo_refset_build: 16 385 rows take the single-index route
    for rs in (own, plain):
        assert not rs.packed_only()
        for per_slab in (0, 1, 2):
            assert wb(rs._h, 4, 1000, 3, 100, per_slab) == 0
        assert _dev_call(L, form, rs._h, 4, 1000, 1 << 30) == E_UNSUPPORTED
    # ... and the same references with room for both are taken: the figure is there, and only the missing device copy stops the call
    ok = _build(refs, ["small", "wide_min", "over_cap"], WIDE_MAX_ROWS)
    assert ok.packed_only() and wb(ok._h, 4, 1000, 3, 100, 1) > 0


def _queries(rng, ref):
    """N, lower case, stretches absent from the reference, copies with substitutions and an indel, the reference's two ends"""
    n = len(ref)
    a, b = ref[n // 3:n // 3 + 400].copy(), ref[n // 2:n // 2 + 300].copy()
    at = [50, 51, len(a) // 2 + 40]
    a[at] = ACGT[(np.searchsorted(ACGT, a[at]) + 1) % 4]
    low = ref[10:60].copy() + 32  # lower case: no base
    parts = [_rnd(rng, 200), a, np.frombuffer(b"NNN", dtype=np.uint8), np.delete(b, [len(b) // 2, len(b) // 2 + 1]), low, _rnd(rng, 150), ref[:120], ref[-120:],
             np.frombuffer(b"acgtN", dtype=np.uint8), ref[n // 4:n // 4 + 250]]
    return np.concatenate(parts)


@pytest.mark.parametrize("rc", [False, True])
@pytest.mark.parametrize("k", [3, 31, 96])
def test_ms_host_equals_the_oracles_matching_statistics(k, rc):
    """LDS and wide references (at k = 3 no index has more than 86 rows, so every reference there is an LDS one); the ATAT reference
    has long contraction scans"""
    rng = np.random.default_rng(500 + k + rc)
    seqs = [_rnd(rng, 300), _rnd(rng, 5000), _rnd(rng, 16500), _rnd(rng, 40000), ACGT[[0, 3]][rng.integers(0, 2, 20000)].copy()]
    with_n = _rnd(rng, 20000)
    with_n[5000:5003] = ord("N")
    with_n[9000:9040] += 32
    seqs.append(with_n)
    rs = refset.RefSet.build(seqs, kbo_amd.BuildOpts(k=k, add_revcomp=rc, num_threads=3), wide_rows=WIDE_MAX_ROWS)
    kinds = set()
    for r, ref in enumerate(seqs):
        oi = ora.Index.build([ref.tobytes()], k=k, add_revcomp=rc)
        assert rs.route(r) == (refset.ROUTE_LDS if oi.n_sets <= MAX_ROWS else refset.ROUTE_WIDE)
        kinds.add(rs.route(r))
        for own, q in ((True, _queries(rng, ref)), (False, _queries(rng, seqs[(r + 1) % len(seqs)]))):
            d, _, _ = oi.matching_statistics(q)
            got = rs.ms_host(r, q)
            assert got.dtype == np.uint8 and np.array_equal(got, d.astype(np.uint8)), (k, rc, r)
            assert not own or (int(d.max()) == k and int(d.min()) == 0)  # (whole k-mers of the copies, nothing at an N)
        assert len(rs.form(r)) == 16 * (2 * (oi.n_sets // 32 + 1) + (oi.n_sets + 16) // 16)
    assert kinds == ({refset.ROUTE_LDS} if k == 3 else {refset.ROUTE_LDS, refset.ROUTE_WIDE})


def test_the_step_under_sanitizers_with_checked_indexes(tmp_path):
    """tools/refset_step_check.cpp over forms from kbo_refset_form: a 16 385-row reference, one of 40 000 bases (a form over 64 KiB)
    and one of 70 000 bases (rows over 65 536); its depths are kbo_refset_ms_host's and the oracle's, and no index is out of range"""
    exe = str(tmp_path / "refset_step_check")
    subprocess.run(["c++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I",
                    os.path.join(ROOT, "kbo_amd", "csrc"), os.path.join(ROOT, "tools", "refset_step_check.cpp"), "-o", exe], check=True)
    rng = np.random.default_rng(77)
    seqs = [_rnd(rng, 16384), _rnd(rng, 40000), _rnd(rng, 70000)]
    rs = refset.RefSet.build(seqs, kbo_amd.BuildOpts(k=K, num_threads=3), wide_rows=WIDE_MAX_ROWS)
    for r, ref in enumerate(seqs):
        oi = ora.Index.build([ref.tobytes()], k=K)
        assert rs.route(r) == refset.ROUTE_WIDE and oi.n_sets == len(ref) + 1
        form = rs.form(r)
        assert len(form) > (1 << 16 if r else 0)
        q = _queries(rng, ref)
        form.tofile(str(tmp_path / "form"))
        q.tofile(str(tmp_path / "query"))
        run = subprocess.run([exe, str(tmp_path / "form"), str(tmp_path / "query"), str(oi.n_sets), str(K), str(tmp_path / "depths")],
                             capture_output=True, text=True)
        assert run.returncode == 0, run.stdout + run.stderr
        assert "in range" in run.stdout
        got = np.fromfile(str(tmp_path / "depths"), dtype=np.uint8)
        d, _, _ = oi.matching_statistics(q)
        assert np.array_equal(got, d.astype(np.uint8)) and np.array_equal(got, rs.ms_host(r, q))
    # a form that is not the one of the rows it is said to have is refused, not walked
    run = subprocess.run([exe, str(tmp_path / "form"), str(tmp_path / "query"), "123", str(K), str(tmp_path / "depths")],
                         capture_output=True, text=True)
    assert run.returncode == 2
