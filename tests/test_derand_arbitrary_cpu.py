"""The inputs of tests/test_gpu_derand_arbitrary.py reach the branches they are meant to reach - checked without a GPU, by a numpy
model of the piece rule of derand_translate_piece_lds_kernel (gpu_helpers.piece_gives_up): a piece that ends at c1 < len gives up, and
its sequence is redone by one lane in a second launch, when neither a k nor the sequence's last position lies in [c1, c1 + 1023].
Also here: the hook's symbol, and the argument error for a call in place, which comes back before anything is enqueued."""
import ctypes as C

import numpy as np
import pytest

import kbo_amd
from kbo_amd import _capi
import gpu_helpers as gh

KS = [3, 31, 96, 255]
E_BAD_ARG = -4


def _redone(k, t, kind, order, reach=gh.DT_REACH):
    """per sequence of the piece batch: length, and how many of its pieces give up (one is enough for the sequence to be redone)"""
    lens = gh.piece_lengths(order, 100 + order)
    off, ms, *_ = gh.derand_world(None, lens, k, t, kind, gh.DT_PIECE, 7)
    out = []
    for s, n in enumerate(lens):
        a = int(off[s])
        out.append((n, int(gh.piece_gives_up(ms[a:a + n], k, reach)[2].sum()) if n >= 3 else 0))  # (pieces that give up)
    return out


@pytest.mark.parametrize("k", KS)
def test_sparse_k_and_below_have_redone_and_finished_sequences_in_one_batch(k):
    for order in (0, 1, 2):
        for t in gh.derand_thresholds(k):
            r = _redone(k, t, "sparse_k", order)
            assert any(g for n, g in r) and any(not g for n, g in r if n > 2000), (k, t, order)
            assert not any(g for n, g in r if n <= 1024 + gh.DT_PIECE)  # the last position is in reach of every piece
            # with a reach of 1024 instead of 1023 fewer pieces give up: the inputs tell the two apart
            assert sum(g for n, g in _redone(k, t, "sparse_k", order, reach=gh.DT_REACH + 1)) < sum(g for n, g in r)
            if t < k:  # below: values 0 .. t, no k at all - exactly the sequences whose last position is out of piece 0's reach
                assert [g > 0 for n, g in _redone(k, t, "below", order)] == [n > 1024 + gh.DT_PIECE for n, g in r]
    # the distances from a piece's end to the nearest k, just inside and just outside the reach, all occur
    lens = gh.piece_lengths(0, 100)
    off, ms, *_ = gh.derand_world(None, lens, k, 2, "sparse_k", gh.DT_PIECE, 7)
    seen = set()
    for s, n in enumerate(lens):
        if n >= 3:
            seen |= set(gh.piece_gives_up(ms[int(off[s]):int(off[s]) + n], k)[1].tolist())
    assert {1022, 1023, 1024, 1025} <= seen


@pytest.mark.parametrize("k", KS)
def test_walk_like_bytes_never_reach_the_redo_launch(k):
    """what the rest of the suite feeds these kernels: a full-length match is never far away.  (k = 255 is the exception that this
    content has by construction: its ramps of 255 values start at most 199 positions apart, so no value reaches k behind the first
    ramp, which starts inside the first piece, and every sequence whose end is beyond that piece's reach is redone.)"""
    for order in (0, 1, 2):
        r = _redone(k, (k + 1) // 2, "walk", order)
        if k < 255:
            assert not any(g for n, g in r)
        else:
            assert [g > 0 for n, g in r] == [n > 1024 + gh.DT_PIECE for n, g in r]


def test_batches_have_the_shapes_their_routes_need():
    P = gh.DT_PIECE
    for order in (0, 1, 2):
        lens = gh.piece_lengths(order, 100 + order)
        assert {P - 1, P, P + 1, 2 * P, 2 * P + 1, 481, 64 * P - 1, 64 * P, 64 * P + 1, 1024 + P - 1, 1024 + P + 1, 20_000, 70_000} <= set(lens)
        assert {0, 1, 2} <= set(lens) and sum(lens) <= 200_000 and max(lens) == 70_000
    first = gh.piece_lengths(0, 100)
    assert all(n < 3 for n in first[:5]) and 0 < sum(first[:5]) < 16 and first[5] >= 3  # the first real sequence starts inside 16 bytes
    assert gh.piece_lengths(1, 101)[0] == 70_000 and gh.piece_lengths(2, 102)[-1] == 70_000
    assert {gh.lds_waves_per_workgroup(mx) for mx in gh.LDS_MAX_LENS} == {2, 3, 4}
    n_waves = (gh.LDS_SEQS + 63) // 64
    assert gh.LDS_SEQS % 64 and all(n_waves % w for w in (2, 3, 4))
    for mx in gh.LDS_MAX_LENS:
        for variant, mod in ((0, 0), (1, 7)):
            lens = gh.lds_lengths(mx, variant, 5)
            assert len(lens) == gh.LDS_SEQS and max(lens) == mx and sum(lens) % 16 == mod
            assert set(lens[gh.LDS_FULL_WAVE[0]:gh.LDS_FULL_WAVE[1]]) == {mx}
            assert (lens[0], lens[-1]) == ((1, mx) if variant == 0 else (mx, 2))
            assert {0, 1, 2, 3} <= set(lens)


def test_thresholds():
    assert gh.derand_thresholds(3) == [2, 3] and gh.derand_thresholds(31) == [2, 3, 16, 30, 31]
    assert gh.derand_thresholds(96) == [2, 3, 48, 95, 96] and gh.derand_thresholds(255) == [2, 3, 128, 254, 255]


def test_hook_is_declared_and_exported():
    assert "kbo_derand_translate_host" in _capi.TUNING_SYMBOLS and "kbo_derand_translate_host" not in _capi.SYMBOLS
    assert hasattr(C.CDLL(_capi.LIB_PATH), "kbo_derand_translate_host")
    assert kbo_amd.lib().kbo_derand_translate_host.argtypes is not None


def test_in_place_is_refused_before_anything_is_enqueued():
    """kbo_derand_translate_dev (kbo_hip.h): d_chars_out must not be d_ms.  The pointers are dummy integers that nothing follows."""
    L = kbo_amd.lib()
    MS, OFF, REF, WORK = 0x10000, 0x20000, 0x40000, 0x60000
    for max_len, work, wb in ((150, None, 0), (0, None, 0), (0, WORK, int(L.kbo_derand_work_bytes(4, 1000)))):
        for ref in (None, REF):
            assert L.kbo_derand_translate_dev(MS, OFF, 4, 1000, 31, 14, ref, MS, max_len, work, wb, None) == E_BAD_ARG
    assert b"in place" in L.kbo_last_error()
