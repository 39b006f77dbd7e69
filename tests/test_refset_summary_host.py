"""kbo_summary_refset, kbo_derand_summary_seq_dev and kbo_derand_summary_seq_work_bytes (kbo_hip.h) on the host: the symbols, the
record sizes, the scratch figure and every documented argument error - all of which come back before the first HIP call, so the
device pointers are dummy integers, suitably aligned, that nothing ever follows."""
import ctypes as C
import os
import re

import numpy as np

import kbo_amd
from kbo_amd import _capi, refset

E_EMPTY_QUERY, E_LEN_LE_2, E_THRESHOLD_LE_1, E_BAD_ARG, E_UNSUPPORTED = -1, -2, -3, -4, -8
MS, OFF, THR, OUT, WORK = 0x10000, 0x20000, 0x30000, 0x50000, 0x60000
NEW_SYMBOLS = ["kbo_derand_summary_seq_work_bytes", "kbo_derand_summary_seq_dev", "kbo_summary_refset"]


def test_symbols_are_exported_and_declared():
    L = kbo_amd.lib()
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "kbo_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert getattr(L, name) is not None and name in _capi.SYMBOLS
        assert re.search(r"\b%s\(" % name, hdr), name
    assert "kbo_aln_extent" in hdr and "kbo_ref_summary" in hdr
    assert kbo_amd.summary_refset is refset.summary_refset


def test_record_sizes():
    assert refset.REF_SUMMARY.itemsize == 36 and len(refset.REF_SUMMARY.names) == 9
    assert all(refset.REF_SUMMARY[n] == np.uint32 for n in refset.REF_SUMMARY.names)
    assert refset.REF_SUMMARY.names[:3] == ("ref", "seq", "strand")
    extent = refset.REF_SUMMARY.names[3:]
    assert extent == ("n_match", "n_mismatch", "n_jump", "n_runs", "start", "end") and 4 * len(extent) == 24
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "kbo_hip.h")).read()
    assert re.search(r"uint32_t n_match, n_mismatch, n_jump, n_runs, start, end;\s*\}\s*kbo_aln_extent;", hdr)
    assert re.search(r"uint32_t ref, seq, strand;[^}]*kbo_aln_extent aln;\s*\}\s*kbo_ref_summary;", hdr)


def test_work_bytes_follow_the_character_form():
    L = kbo_amd.lib()
    wb, wb_chars = L.kbo_derand_summary_seq_work_bytes, L.kbo_derand_seq_work_bytes
    assert wb(1, 3, 31, 14) > 0 and wb(1, 0, 3, 2) > 0 and wb(1000, 1 << 24, 255, 2) > 0
    for args in ((0, 0, 31, 14), (1, 3, 31, 14), (1000, 1 << 20, 96, 20), (7, 12345, 255, 2), (5, 100, 0, 0), (5, 100, 31, 40),
                 (1 << 28, 1 << 33, 300, 1)):
        # zero for the inputs the character form's figure is zero for; otherwise enough for the shared passes
        assert (wb(*args) == 0) == (wb_chars(*args) == 0), args
        assert wb(*args) >= wb_chars(*args), args
    assert wb(1000, 1 << 24, 31, 14) % 16 == 0


def test_stage_argument_errors_need_no_device():
    L = kbo_amd.lib()
    n, total, k, t = 4, 1000, 31, 14
    wb = int(L.kbo_derand_summary_seq_work_bytes(n, total, k, t))

    def call(ms=MS, off=OFF, n_seqs=n, total_bases=total, k=k, thr=THR, min_thr=t, out=OUT, work=WORK, work_bytes=wb):
        return L.kbo_derand_summary_seq_dev(ms, off, n_seqs, total_bases, k, thr, min_thr, out, work, work_bytes, None)
    for null in ("ms", "off", "thr", "out", "work"):
        assert call(**{null: None}) == E_BAD_ARG, null
    for bad_k in (0, 256):
        assert call(k=bad_k, min_thr=2) == E_BAD_ARG
    assert call(min_thr=k + 1) == E_BAD_ARG
    for low in (0, 1):
        assert call(min_thr=low, work_bytes=1 << 40) == E_THRESHOLD_LE_1
    assert call(n_seqs=0) == E_EMPTY_QUERY
    for step in (4, 8):
        assert call(work=WORK + step) == E_BAD_ARG, "a misaligned d_work"
    for name, base, step in (("ms", MS, 2), ("out", OUT, 3)):
        assert call(**{name: base + step}) == E_BAD_ARG, name
    assert call(work_bytes=wb - 1) == E_BAD_ARG and call(work_bytes=0) == E_BAD_ARG
    assert call(min_thr=2) == E_BAD_ARG, "a lower bound needs more scratch than a higher one's figure"
    assert call(total_bases=(1 << 32) - 15, work_bytes=1 << 60) == E_UNSUPPORTED
    assert call(n_seqs=1 << 28, work_bytes=1 << 60) == E_UNSUPPORTED


def _refs(k, seed):
    rng = np.random.default_rng(seed)

    def rnd(n):
        return np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)].tobytes()
    return [rnd(k - 1), rnd(k), rnd(40), rnd(300), rnd(1500)]


def test_summary_refset_argument_errors_need_no_device():
    L = kbo_amd.lib()
    rs = refset.RefSet.build(_refs(31, 5), kbo_amd.BuildOpts(k=31))
    q = np.frombuffer(b"ACGTACGTACGTAC", dtype=np.uint8).copy()
    off = np.array([0, 10, 14], dtype=np.uint64)
    p, n = C.c_void_p(), C.c_uint64()

    def call(h=rs._h, concat=q.ctypes.data, offsets=off, n_seqs=2, prob=1e-7, strands=3, records=C.byref(p), n_records=C.byref(n)):
        return L.kbo_summary_refset(h, concat, offsets.ctypes.data if offsets is not None else None, n_seqs, prob, strands, records, n_records)
    assert call(h=None) == E_BAD_ARG
    assert call(concat=None) == E_BAD_ARG
    assert call(offsets=None) == E_BAD_ARG
    assert call(records=None) == E_BAD_ARG
    assert call(n_records=None) == E_BAD_ARG
    for strands in (0, 4, -1):
        assert call(strands=strands) == E_BAD_ARG
    for prob in (0.0, 1.5, -1e-7):
        assert call(prob=prob) == E_BAD_ARG
    assert call(offsets=np.array([0, 12, 14], dtype=np.uint64)) == E_LEN_LE_2  # a 2-base sequence refuses the batch
    assert call(offsets=np.array([0, 12, 8], dtype=np.uint64)) == E_BAD_ARG    # offsets that do not ascend
    assert call(offsets=np.array([1, 10, 14], dtype=np.uint64)) == E_BAD_ARG   # ... or do not start at 0
    assert call(prob=1.0) == E_THRESHOLD_LE_1  # (every string is a random match then: kbo_find on such a handle fails so)
    assert not p.value and n.value == 0
