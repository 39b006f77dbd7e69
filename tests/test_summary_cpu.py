"""Per-sequence alignment summaries (kbo_hip.h kbo_aln_summary), the parts that need no GPU: batch.summary_of_chars - the plain-numpy
restatement the device entry points are tested against (tests/test_gpu_summary.py) - on the golden alignments and on hand-made edge
strings, and the new symbols of the library."""
import ctypes as C
import os

import numpy as np

import kbo_amd
from kbo_amd import _capi, batch

NEW_SYMBOLS = ["kbo_summary_batch", "kbo_summary_batch_packed", "kbo_summary_work_bytes", "kbo_summary_batch_dev", "kbo_summary_dev",
               "kbo_summary_words_work_bytes", "kbo_summary_words_dev", "kbo_map_stream_submit_summary"]


def _by_hand(s):
    """the record of one alignment string, counted the slow way"""
    if len(s) < 3:
        return [0, 0, 0, 0]
    return [s.count("M"), s.count("X"), s.count("R"), len([r for r in s.split("-") if r])]


def _summ(strings):
    chars = np.frombuffer("".join(strings).encode(), dtype=np.uint8)
    offsets = np.concatenate([[0], np.cumsum([len(s) for s in strings])]).astype(np.uint64)
    return batch.summary_of_chars(chars, offsets)


def _strings_of(obj, out):
    """every alignment string (only M - X R, at least one character) anywhere in the golden file"""
    if isinstance(obj, str):
        if obj and set(obj) <= set("M-XR"):
            out.append(obj)
    elif isinstance(obj, dict):
        for v in obj.values():
            _strings_of(v, out)
    elif isinstance(obj, list):
        for v in obj:
            _strings_of(v, out)


def test_summary_of_chars_on_the_golden_alignments(golden):
    strings = []
    _strings_of(golden, strings)
    assert len(strings) >= 3 and any("-" in s for s in strings) and any("X" in s or "R" in s for s in strings)
    got = _summ(strings)
    assert got.dtype == np.uint32 and got.shape == (len(strings), 4)
    assert got.tolist() == [_by_hand(s) for s in strings]
    # one at a time: no count leaks across a boundary
    for s in strings:
        assert _summ([s]).tolist() == [_by_hand(s)]


def test_summary_of_chars_edge_strings():
    cases = {
        "-----": [0, 0, 0, 0],                  # all '-': no run
        "MMMMM": [5, 0, 0, 1],                  # a run touching both ends
        "M-M": [2, 0, 0, 2],
        "-M-": [1, 0, 0, 1],
        "MMRR": [2, 0, 2, 1],
        "RRMM": [2, 0, 2, 1],
        "MMXMM--MRRM-": [6, 1, 2, 2],
        "X--": [0, 1, 0, 1],
        "": [0, 0, 0, 0],
        "M": [0, 0, 0, 0],                      # fewer than 3 bases: no alignment, whatever the characters
        "MM": [0, 0, 0, 0],
        "RX": [0, 0, 0, 0],
    }
    for s, want in cases.items():
        assert _by_hand(s) == want, s
        assert _summ([s]).tolist() == [want], s
    # 'R','R' at a boundary; runs that touch a boundary from both sides are two runs; short and empty sequences in between
    strings = ["MMMR", "RMMM", "MMM", "", "MMM", "MM", "---", "M", "--M", "M--", "MMMMMMMMMMMMMMMM", "-MMMMMMMMMMMMMMM-"]
    assert _summ(strings).tolist() == [_by_hand(s) for s in strings]
    assert _summ([]).shape == (0, 4)
    # the characters of a sequence of fewer than 3 bases are unspecified: pre-filled with 'M' they still count for nothing
    assert _summ(["MM", "MMM", "M", "M-M"]).tolist() == [[0, 0, 0, 0], [3, 0, 0, 1], [0, 0, 0, 0], [2, 0, 0, 2]]
    # bytes input
    assert batch.summary_of_chars(b"MM-XR", [0, 5]).tolist() == [[2, 1, 1, 2]]


def test_summary_of_chars_random_against_the_slow_count():
    rng = np.random.default_rng(5)
    alphabet = np.frombuffer(b"MMMM--XR", dtype=np.uint8)
    for _ in range(50):
        lens = rng.integers(0, 40, int(rng.integers(1, 30)))
        strings = [alphabet[rng.integers(0, len(alphabet), int(l))].tobytes().decode() for l in lens]
        assert _summ(strings).tolist() == [_by_hand(s) for s in strings]


def test_new_symbols_are_declared_and_exported():
    for name in NEW_SYMBOLS:
        assert name in _capi.SYMBOLS, name
    raw = C.CDLL(_capi.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(raw, name), name
    L = kbo_amd.lib()
    for name in NEW_SYMBOLS:
        assert getattr(L, name).argtypes is not None, name
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "kbo_hip.h")) as f:
        header = f.read()
    for name in NEW_SYMBOLS:
        assert name + "(" in header, name
    assert "kbo_aln_summary" in header
