"""kbo_map_batch_opts / kbo_fill_gaps_batch without a GPU: the symbols, MapOpts through ctypes, the whole-call errors that come
before any device work, the loud failure where there is no device, and the rule gap_starts_kernel (kbo_amd/csrc/gap_kernels.hip)
rests on - that the starts of the reference's sequential gap scan (gap_filling.rs:466-521, refine.cpp kbo::fill_gaps) can be
decided per position - checked against that scan on random and adversarial translations."""
import ctypes as C

import numpy as np
import pytest

import kbo_amd
from kbo_amd import _capi, batch

E_EMPTY, E_BAD_ARG, E_K_MISMATCH, E_HIP = -1, -4, -6, -7


def _batch(seqs):
    off = np.zeros(len(seqs) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    return np.frombuffer(b"".join(seqs), dtype=np.uint8).copy(), off


def test_symbols_and_map_opts_through_ctypes():
    L = kbo_amd.lib()
    for name in ("kbo_map_batch_opts", "kbo_fill_gaps_batch", "kbo_fill_gaps_stats", "kbo_map_batch_opts_phases"):
        assert hasattr(L, name), name
    assert "kbo_map_batch_opts" in _capi.SYMBOLS and "kbo_fill_gaps_batch" in _capi.SYMBOLS
    assert "kbo_fill_gaps_stats" in _capi.TUNING_SYMBOLS
    o = _capi.MapOpts()
    L.kbo_map_opts_default(C.byref(o))
    d = kbo_amd.MapOpts()
    assert (o.max_error_prob, o.fill_gaps, o.call_variants, o.format, o.sbwt_build_opts.k) == \
        (d.max_error_prob, int(d.fill_gaps), int(d.call_variants), int(d.format), d.sbwt_build_opts.k)
    st = (C.c_uint64 * 4)()
    assert L.kbo_fill_gaps_stats(st) == 0
    assert L.kbo_fill_gaps_stats(None) == E_BAD_ARG


def test_null_arguments():
    L = kbo_amd.lib()
    sbwt, _ = kbo_amd.build([b"ACGTACGTTGCAGGATCCA"], kbo_amd.BuildOpts(k=5))
    concat, off = _batch([b"ACGTACGTTG"])
    out = np.zeros(16, dtype=np.uint8)
    status = np.zeros(1, dtype=np.int32)
    o = _capi.MapOpts()
    L.kbo_map_opts_default(C.byref(o))
    o.sbwt_build_opts.k = 5
    args = [sbwt._h, concat.ctypes.data, off.ctypes.data, 1, C.byref(o), out.ctypes.data, status.ctypes.data]
    for i in (0, 1, 2, 5, 6):
        a = list(args)
        a[i] = None
        assert L.kbo_map_batch_opts(*a) == E_BAD_ARG, i
    fargs = [sbwt._h, concat.ctypes.data, off.ctypes.data, 1, 3, 1e-7, out.ctypes.data, status.ctypes.data]
    for i in (0, 1, 2, 6, 7):
        a = list(fargs)
        a[i] = None
        assert L.kbo_fill_gaps_batch(*a) == E_BAD_ARG, i
    assert L.kbo_fill_gaps_batch(*(fargs[:4] + [1] + fargs[5:])) == -3  # threshold > 1


def test_k_mismatch_comes_before_device_work():
    sbwt, _ = kbo_amd.build([b"ACGTACGTTGCAGGATCCA"], kbo_amd.BuildOpts(k=5))
    concat, off = _batch([b"ACGTACGTTGCA", b"GGATCCAACGT"])
    with pytest.raises(kbo_amd.KboError) as e:
        batch.map_batch_opts(sbwt, concat, off, kbo_amd.MapOpts())  # sbwt_build_opts.k = 31
    assert e.value.code == E_K_MISMATCH


def test_fails_loudly_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    sbwt, _ = kbo_amd.build([b"ACGTACGTTGCAGGATCCAATTGCCA"], kbo_amd.BuildOpts(k=5))
    concat, off = _batch([b"ACGTACGTTGCAGGATCCA", b"TTGCCAACGTACGTAGGA"])
    mo = kbo_amd.MapOpts(sbwt_build_opts=kbo_amd.BuildOpts(k=5, build_select=True))
    for call in (lambda: batch.map_batch_opts(sbwt, concat, off, mo),
                 lambda: batch.fill_gaps_batch(sbwt, concat, off, 3, 1e-7)):
        with pytest.raises(kbo_amd.KboError) as e:
            call()
        assert e.value.code == E_HIP


# ---- the gap-start rule

def sequential_gaps(tr, t):
    """The scan of gap_filling.rs:466-521 (refine.cpp kbo::fill_gaps) without the fills: (start, end) of every gap it visits.
    A fill writes only [start, end) and never '-', and nothing after it reads those positions, so the fills do not matter."""
    n = len(tr)
    gaps = []
    i = t + 1
    while i < n - t:
        if tr[i - 1] in b"-X":
            start = i - 1
            while i < n and tr[i] == ord("-"):
                i += 1
            gaps.append((start, min(i, n - t)))
        i += 1
    return gaps


def parallel_gaps(tr, t):
    """gap_starts_kernel's rule, one position at a time, and the end gap_fill_kernel finds for each start"""
    n = len(tr)
    gaps = []
    for s in range(n):
        c = tr[s]
        if not (t <= s and s + t + 1 < n and c in b"-X"):
            continue
        if c == ord("-") and s - 1 >= t and tr[s - 1] in b"-X":
            continue
        e = s + 1
        while e < n - t and tr[e] == ord("-"):
            e += 1
        gaps.append((s, min(e, n - t)))
    return gaps


def test_gap_start_rule_equals_the_sequential_scan_random():
    rng = np.random.default_rng(17)
    alphabet = np.frombuffer(b"M-XRACGT", dtype=np.uint8)
    weights = np.array([0.35, 0.3, 0.12, 0.05, 0.045, 0.045, 0.045, 0.045])
    n_gaps = 0
    for it in range(100_000):
        n = int(rng.integers(1, 48))
        t = int(rng.integers(2, 9))
        tr = alphabet[rng.choice(8, size=n, p=weights)].tobytes()
        a, b = sequential_gaps(tr, t), parallel_gaps(tr, t)
        assert a == b, (tr, t, a, b)
        n_gaps += len(a)
    assert n_gaps > 50_000


@pytest.mark.parametrize("t", [2, 3, 5])
def test_gap_start_rule_adversarial(t):
    cases = [b"-" * 40, b"X" * 40, b"X-X--X" * 8, b"-X" * 20, b"X-" * 20, b"M" * 40]
    for n in range(2 * t, 2 * t + 12):
        for a in range(n):
            for L in range(1, n - a + 1):
                cases.append(b"M" * a + b"-" * L + b"M" * (n - a - L))      # runs touching t and n - t
                cases.append(b"M" * a + b"X" + b"-" * (L - 1) + b"M" * (n - a - L))
    for tr in cases:
        assert sequential_gaps(tr, t) == parallel_gaps(tr, t), (tr, t)
