"""kbo_best_refset, kbo_best_refset_dev and kbo_best_refset_dev_work_bytes (kbo_hip.h "find against a set of references": the best
reference per sequence) on the host: the symbols, the record's layout against the header's struct, the scratch figure, every
documented argument error - all of which come back before the first HIP call, so the device pointers are dummy integers, suitably
aligned, that nothing ever follows - and the record's merge (kbo_amd/csrc/refset_best.hpp) by brute force in
tools/refset_best_check.cpp, a stand-alone program under AddressSanitizer and UBSan.  No GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import kbo_amd
from kbo_amd import _capi, refset

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_EMPTY_QUERY, E_LEN_LE_2, E_THRESHOLD_LE_1, E_BAD_ARG, E_UNSUPPORTED = -1, -2, -3, -4, -8
Q, OFF, WORK, OUT = 0x10000, 0x20000, 0x30000, 0x50000
API = ["kbo_best_refset", "kbo_best_refset_dev_work_bytes", "kbo_best_refset_dev"]
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
    api = open(os.path.join(ROOT, "include", "kbo_hip.h")).read()
    tuning = open(os.path.join(ROOT, "include", "kbo_hip_tuning.h")).read()
    for name in API:
        assert getattr(L, name) is not None and name in _capi.SYMBOLS
        assert re.search(r"\b%s\(" % name, api), name
    assert getattr(L, "kbo_refset_last_best") is not None and "kbo_refset_last_best" in _capi.TUNING_SYMBOLS
    assert re.search(r"\bkbo_refset_last_best\(", tuning)
    assert kbo_amd.best_refset is refset.best_refset and kbo_amd.best_refset_dev is refset.best_refset_dev
    assert callable(refset.last_best) and L.kbo_refset_last_best(None) == E_BAD_ARG


def test_the_dtype_is_the_headers_struct():
    d = refset.REF_BEST
    assert d.itemsize == 48 and len(d.names) == 12 and all(d[n] == np.uint32 for n in d.names)
    assert [d.fields[n][1] for n in d.names] == list(range(0, 48, 4))
    hdr = open(os.path.join(ROOT, "include", "kbo_hip.h")).read()
    m = re.search(r"typedef struct \{\s*uint32_t ([a-z_, ]+);[^\n]*\n\s*kbo_aln_extent aln;\s*uint32_t ([a-z_, ]+);\s*\}\s*kbo_ref_best; /\* 48 bytes \*/", hdr)
    assert m, "kbo_ref_best in kbo_hip.h"
    ext = re.search(r"uint32_t ([a-z_, ]+);\s*\}\s*kbo_aln_extent;", hdr).group(1)
    names = [n.strip() for n in (m.group(1) + "," + ext + "," + m.group(2)).split(",")]
    assert tuple(names) == d.names
    # ... and the words of refset_best.hpp, which the kernel and the host merge by
    hpp = open(os.path.join(ROOT, "kbo_amd", "csrc", "refset_best.hpp")).read()
    words = re.search(r"struct Best \{[^\n]*\n\s*uint32_t ([a-z_, ]+);", hpp).group(1)
    assert tuple(n.strip() for n in words.split(",")) == d.names
    assert re.search(r"#define KBO_REF_NONE 0xFFFFFFFFu", hdr) and refset.REF_NONE == 0xFFFFFFFF
    assert re.search(r"constexpr uint32_t kNone = 0xFFFFFFFFu;", hpp)


def test_work_bytes_are_monotonic_and_aligned(rs, rs_own):
    L = kbo_amd.lib()
    wb = L.kbo_best_refset_dev_work_bytes
    n_q = 4  # (the reference of k - 1 bases cannot be queried)
    shapes = ((1, 3), (2, 0), (7, 1500), (7, 70000), (300, 70000), (5000, 70000))
    for n_seqs, total in shapes:
        for strands in (1, 2, 3):
            by_refs = [int(wb(rs._h, n_seqs, total, strands, r)) for r in range(1, n_q + 3)]
            assert by_refs[0] > 0 and all(v % 16 == 0 for v in by_refs)
            assert all(a <= b for a, b in zip(by_refs, by_refs[1:]))
            if total:
                assert all(a < b for a, b in zip(by_refs[:n_q - 1], by_refs[1:n_q])), "a slab of more references holds more bytes"
            # beyond the queryable references a slab cannot grow, and 0 asks for as many as there are
            assert by_refs[n_q - 1] == by_refs[n_q] == by_refs[n_q + 1] == int(wb(rs._h, n_seqs, total, strands, 0))
            # no more than the summary form's figure without room for a record: its scan and its kept list are not there
            assert by_refs[1] < int(L.kbo_summary_refset_dev_work_bytes(rs._h, n_seqs, total, strands, 0, 2))
    for per_slab in (1, 2, 0):
        for strands in (1, 2, 3):  # non-decreasing in the sequences and in the bases
            by_seqs = [int(wb(rs._h, n, 70000, strands, per_slab)) for n in (1, 7, 300, 5000)]
            by_bases = [int(wb(rs._h, 7, t, strands, per_slab)) for t in (0, 3, 1500, 70000, 1 << 20)]
            assert all(a <= b for a, b in zip(by_seqs, by_seqs[1:])) and all(a <= b for a, b in zip(by_bases, by_bases[1:]))
        by_strands = [int(wb(rs._h, 7, 70000, s, per_slab)) for s in (1, 2, 3)]
        assert by_strands[0] <= by_strands[1] <= by_strands[2]
    # what the call refuses has no figure
    assert wb(None, 1, 3, 3, 1) == 0 and wb(rs._h, 0, 0, 3, 1) == 0
    assert wb(rs._h, 1, 3, 0, 1) == 0 and wb(rs._h, 1, 3, 4, 1) == 0
    assert wb(rs._h, 1 << 27, 1 << 27, 3, 1) == 0 and wb(rs._h, 1 << 28, 1 << 28, 1, 1) == 0
    assert wb(rs._h, 1, (1 << 32) - 16, 1, 1) == 0 and wb(rs._h, 1, (1 << 31) - 8, 3, 1) == 0
    assert wb(rs_own._h, 4, 1000, 3, 1) == 0 and not rs_own.packed_only()


def test_device_form_argument_errors_need_no_device(rs, rs_own):
    L = kbo_amd.lib()
    wb1 = int(L.kbo_best_refset_dev_work_bytes(rs._h, 4, 1000, 3, 1))
    assert wb1 > 0

    def call(h=rs._h, q=Q, off=OFF, n_seqs=4, total=1000, prob=1e-7, strands=3, work=WORK, work_bytes=wb1, out=OUT):
        return L.kbo_best_refset_dev(h, q, off, n_seqs, total, prob, strands, work, work_bytes, out, None)
    for null in ("h", "q", "off", "work", "out"):
        assert call(**{null: None}) == E_BAD_ARG, null
    for name, base, step in (("q", Q, 8), ("q", Q, 1), ("off", OFF, 4), ("work", WORK, 8), ("out", OUT, 2)):
        assert call(**{name: base + step}) == E_BAD_ARG, (name, step)
    for strands in (0, 4, -1):
        assert call(strands=strands) == E_BAD_ARG
    for prob in (0.0, 1.5, -1e-7):
        assert call(prob=prob) == E_BAD_ARG
    assert call(n_seqs=0) == E_EMPTY_QUERY
    assert call(prob=1.0) == E_THRESHOLD_LE_1
    assert call(work_bytes=wb1 - 1) == E_BAD_ARG and call(work_bytes=0) == E_BAD_ARG
    assert call(total=(1 << 32) - 16, strands=1, work_bytes=1 << 60) == E_UNSUPPORTED
    assert call(n_seqs=1 << 28, total=1 << 28, strands=1, work_bytes=1 << 60) == E_UNSUPPORTED
    # a set that is not packed-only, whatever else is right
    assert call(h=rs_own._h, work_bytes=1 << 30) == E_UNSUPPORTED


def test_host_form_argument_errors_need_no_device(rs):
    L = kbo_amd.lib()
    q = np.frombuffer(b"ACGTACGTACGTAC", dtype=np.uint8).copy()
    off = np.array([0, 10, 14], dtype=np.uint64)
    p = C.c_void_p()

    def call(h=rs._h, concat=q.ctypes.data, offsets=off, n_seqs=2, prob=1e-7, strands=3, out=C.byref(p)):
        return L.kbo_best_refset(h, concat, offsets.ctypes.data if offsets is not None else None, n_seqs, prob, strands, out)
    assert call(h=None) == E_BAD_ARG
    assert call(concat=None) == E_BAD_ARG
    assert call(offsets=None) == E_BAD_ARG
    assert call(out=None) == E_BAD_ARG
    for strands in (0, 4, -1):
        assert call(strands=strands) == E_BAD_ARG
    for prob in (0.0, 1.5, -1e-7):
        assert call(prob=prob) == E_BAD_ARG
    assert call(offsets=np.array([0, 12, 14], dtype=np.uint64)) == E_LEN_LE_2  # a 2-base sequence refuses the batch
    assert call(offsets=np.array([0, 12, 8], dtype=np.uint64)) == E_BAD_ARG    # offsets that do not ascend
    assert call(prob=1.0) == E_THRESHOLD_LE_1
    big = np.array([0, 1 << 31], dtype=np.uint64)
    assert call(offsets=big, n_seqs=1) == E_UNSUPPORTED  # a batch of 2^31 bases (nothing is read before the check)
    assert not p.value


def test_the_merge_by_brute_force_under_sanitizers(tmp_path):
    """tools/refset_best_check.cpp: every list of pairs over 3 references x 2 strands, every cut into up to 3 slabs, both merge orders,
    against the record made by sorting - all twelve words"""
    exe = str(tmp_path / "refset_best_check")
    subprocess.run(["c++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I",
                    os.path.join(ROOT, "kbo_amd", "csrc"), os.path.join(ROOT, "tools", "refset_best_check.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    m = re.search(r"(\d+) lists, (\d+) cases agree", run.stdout)
    assert m and int(m.group(1)) == 4 ** 6 >= 3 ** 6 and int(m.group(2)) == 4 ** 6 * 28 * 8
