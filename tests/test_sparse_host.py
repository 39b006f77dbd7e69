"""The sparse form of kbo::matches on the host side (no GPU): kbo_sparse_expand over hand-made records - runs at a sequence's first
and last base, both output forms - its argument checks, and the host entry point's argument checks, which must come before any
device work."""
import ctypes as C

import numpy as np
import pytest

import kbo_amd
from kbo_amd import batch, synth

BAD_ARG, UNSUPPORTED, EMPTY_QUERY, LEN_LE_2 = -4, -8, -1, -2


def runs_of(recs):
    out = np.zeros(len(recs), dtype=batch.SPARSE_DTYPE)
    for i, (s, st, ln, code) in enumerate(recs):
        out[i] = (s, st, ln, code)
    return out


def sparse_from_chars(chars, offsets):
    """the expected records, in numpy: maximal runs of one character other than 'M' inside each sequence"""
    recs = []
    code = {ord("-"): 1, ord("X"): 2, ord("R"): 3}
    for s in range(len(offsets) - 1):
        a, b = int(offsets[s]), int(offsets[s + 1])
        i = a
        while i < b:
            c = int(chars[i])
            if c == ord("M"):
                i += 1
                continue
            j = i
            while j < b and chars[j] == c:
                j += 1
            recs.append((s, i - a, j - i, code[c]))
            i = j
    return runs_of(recs)


OFFSETS = np.array([0, 5, 8, 28], dtype=np.uint64)  # sequences of 5, 3 and 20 bases
HAND = runs_of([(0, 0, 1, 2), (0, 3, 2, 1), (2, 0, 2, 1), (2, 2, 1, 2), (2, 19, 1, 3)])
HAND_CHARS = b"XMM--" + b"MMM" + b"--X" + b"M" * 16 + b"R"


def test_expand_hand_made_records():
    got = batch.expand_sparse(HAND, OFFSETS)
    assert got.tobytes() == HAND_CHARS
    ref = np.frombuffer(b"ACGTA" + b"CCG" + b"TTGACGTACGTACGTACGTG", dtype=np.uint8)
    rel = batch.expand_sparse(HAND, OFFSETS, ref=ref)
    # format::relative_to_ref (format.rs:270-286): the read's base for 'M' and 'R', '-' for 'X' and '-'
    exp = bytes(ref[i] if HAND_CHARS[i] in b"MR" else ord("-") for i in range(len(ref)))
    assert rel.tobytes() == exp


def test_expand_without_records_is_all_matches():
    got = batch.expand_sparse(runs_of([]), OFFSETS)
    assert got.tobytes() == b"M" * 28


def test_expand_round_trip_random_characters():
    rng = np.random.default_rng(5)
    lens = rng.integers(1, 300, 2000)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    # mostly 'M', with runs of each of the three other characters
    chars = np.full(int(offsets[-1]), ord("M"), dtype=np.uint8)
    for _ in range(4000):
        p = int(rng.integers(0, len(chars)))
        chars[p:p + int(rng.integers(1, 40))] = rng.choice(list(b"-XR"))
    runs = sparse_from_chars(chars, offsets)
    assert len(runs) > 1000
    assert np.array_equal(batch.expand_sparse(runs, offsets), chars)
    ref = np.frombuffer(synth.genome(len(chars), seed=3).tobytes(), dtype=np.uint8)
    exp = np.where((chars == ord("M")) | (chars == ord("R")), ref, np.uint8(ord("-")))
    assert np.array_equal(batch.expand_sparse(runs, offsets, ref=ref), exp)


@pytest.mark.parametrize("recs", [
    [(0, 3, 2, 1), (0, 0, 1, 2)],      # out of order inside a sequence
    [(2, 0, 1, 1), (0, 0, 1, 2)],      # out of order across sequences
    [(0, 0, 3, 1), (0, 2, 1, 2)],      # overlapping
    [(0, 4, 2, 1)],                    # past the sequence's end
    [(1, 0, 4, 1)],                    # longer than the sequence
    [(3, 0, 1, 1)],                    # no such sequence
    [(0, 1, 0, 1)],                    # length 0
    [(0, 1, 1, 0)],                    # code 0 ('M')
])
def test_expand_rejects_bad_records(recs):
    with pytest.raises(kbo_amd.KboError) as e:
        batch.expand_sparse(runs_of(recs), OFFSETS)
    assert e.value.code == BAD_ARG


def test_expand_null_arguments():
    L = kbo_amd.lib()
    out = np.zeros(28, dtype=np.uint8)
    raw = batch._sparse_to_raw(HAND)
    assert L.kbo_sparse_expand(None, 5, OFFSETS.ctypes.data, 3, None, out.ctypes.data) == BAD_ARG
    assert L.kbo_sparse_expand(raw.ctypes.data, 5, None, 3, None, out.ctypes.data) == BAD_ARG
    assert L.kbo_sparse_expand(raw.ctypes.data, 5, OFFSETS.ctypes.data, 3, None, None) == BAD_ARG
    assert L.kbo_sparse_expand(None, 0, OFFSETS.ctypes.data, 3, None, out.ctypes.data) == 0
    assert out.tobytes() == b"M" * 28


def test_sparse_entry_point_checks_before_any_device_work():
    """kbo_matches_batch_sparse takes kbo_matches_batch_packed's checks and error codes (plus the 30-bit length field); all of
    them are decided on the host"""
    L = kbo_amd.lib()
    g = synth.genome(20_000, seed=9)
    sbwt, _ = kbo_amd.build([g], kbo_amd.BuildOpts(k=31, num_threads=2))
    words = np.zeros(64, dtype=np.uint32)
    p, n = C.c_void_p(), C.c_uint64(0)

    def call(offsets, exc_pos=None, exc_byte=None, n_exc=0, runs=True):
        o = np.asarray(offsets, dtype=np.uint64)
        return L.kbo_matches_batch_sparse(sbwt._h, words.ctypes.data, o.ctypes.data, len(o) - 1,
                                          exc_pos.ctypes.data if exc_pos is not None else None,
                                          exc_byte.ctypes.data if exc_byte is not None else None, n_exc, 1e-7,
                                          C.byref(p) if runs else None, C.byref(n))
    assert call([0, 150], runs=False) == BAD_ARG
    assert call([0]) == EMPTY_QUERY
    assert call([1, 150]) == BAD_ARG
    assert call([0, 150, 100]) == BAD_ARG
    assert call([0, 150, 150]) == EMPTY_QUERY
    assert call([0, 150, 152]) == LEN_LE_2
    assert call([0, 150], np.array([5, 5], dtype=np.uint64), np.array([78, 78], dtype=np.uint8), 2) == BAD_ARG
    assert call([0, 150], np.array([150], dtype=np.uint64), np.array([78], dtype=np.uint8), 1) == BAD_ARG
    assert call([0, 150], None, None, 1) == BAD_ARG
    assert call([0, 1 << 30]) == UNSUPPORTED
    assert L.kbo_matches_batch_sparse(None, words.ctypes.data, np.array([0, 150], dtype=np.uint64).ctypes.data, 1, None, None, 0, 1e-7,
                                      C.byref(p), C.byref(n)) == BAD_ARG


def test_sparse_work_bytes():
    L = kbo_amd.lib()
    assert L.kbo_sparse_runs_work_bytes(0, 0) == 0
    assert L.kbo_sparse_runs_work_bytes(1000, 1 << 33) == 0
    a, b = L.kbo_sparse_runs_work_bytes(1000, 10_000), L.kbo_sparse_runs_work_bytes(1_000_000, 10_000_000)
    assert a > 0 and b > a and a % 16 == 0 and b % 16 == 0


def test_sparse_dev_workgroups():
    """kbo_sparse_runs_dev's grid: bounded by the longest sequence, the most workgroups when the length is unknown (0), and no
    bound that wraps round to a single workgroup"""
    L = kbo_amd.lib()
    assert L.kbo_sparse_runs_blocks(1, 0) == 2048
    assert L.kbo_sparse_runs_blocks(10_000_000, 0) == 2048
    assert L.kbo_sparse_runs_blocks(1, 1) == 1
    assert L.kbo_sparse_runs_blocks(1000, 150) == 40           # 10 000 words in chunks of 256
    assert L.kbo_sparse_runs_blocks(1_000_000, 150) == 2048
    assert L.kbo_sparse_runs_blocks((1 << 31) - 1, (1 << 30) - 1) == 2048
    assert L.kbo_sparse_runs_blocks(0, 150) == 0
    assert L.kbo_sparse_runs_blocks(1000, 1 << 30) == 0
