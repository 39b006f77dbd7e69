"""kbo_run_lengths_seq_dev (kbo_hip.h): format::run_lengths_gapped of a batch at any sequence length, a chunk per lane, against the oracle.

Expected: oracle.run_lengths_batch of the same bytes - every record and every d_first entry.  One batch holds all the lengths, shuffled
by a fixed seed: 0, 1, 2, 3, 4, C - 1, C, C + 1, 2 C + 1, G - 1, G, G + 1, 2 G + 1, 65 536, 65 537 and one of 300 000 characters
(C = KBO_RLE_SEG_CHUNK = 128, G = KBO_RLE_SEG_GROUP = 8 192): every length at which a chunk or a group begins or ends, and one whose
owner loops over 37 groups.  Contents: (a) kbo::matches-like M - X R with 1 % 'X'; (b) all 'M' - one run across every group; (c) all
'-'; (d) stretches of '-' of exactly g, g + 1 and g + 2 (g = max_gap_len) that start at, end at and straddle chunk and group
boundaries, behind a ' ', the sequence's start and an 'M' (for g = 2^32 - 1, which no stretch reaches, of C - 1, C + 1 and G + 1); (e) the
whole alphabet with ' ', 'D', 'I' and arbitrary bytes, sequences that end in 'D' behind an earlier gap of their last run and ones
that end in '-'.  max_gap_len: 0, 1, 3, C - 1, C, C + 1, 2 G + 5, 2^32 - 1.  Every buffer sits behind guard bands at exactly its
documented size."""
import numpy as np
import pytest

import kbo_amd
from gpu_helpers import PER_BASE_GUARD, Guarded
from oracle import binding as ora

pytestmark = pytest.mark.gpu

C_, G_ = 128, 8192  # KBO_RLE_SEG_CHUNK, KBO_RLE_SEG_GROUP (tests/test_rle_seg_cpu.py pins them to the header)
GAPS = [0, 1, 3, C_ - 1, C_, C_ + 1, 2 * G_ + 5, 2**32 - 1]
CONTENTS = ["matches", "all_m", "all_dash", "stretches", "alphabet"]
LENS = [0, 1, 2, 3, 4, C_ - 1, C_, C_ + 1, 2 * C_ + 1, G_ - 1, G_, G_ + 1, 2 * G_ + 1, 65536, 65537, 300_000]
LENS = [LENS[i] for i in np.random.default_rng(77).permutation(len(LENS))]
OFF = np.zeros(len(LENS) + 1, dtype=np.uint64)
OFF[1:] = np.cumsum(LENS)
OFF.setflags(write=False)
TOTAL = int(OFF[-1])


def _stretches(rng, n, gap):
    """'M' (1 % 'X') with stretches of '-' placed against the chunk and group boundaries"""
    a = np.where(rng.random(n) < 0.01, ord("X"), ord("M")).astype(np.uint8)
    sizes = (gap, gap + 1, gap + 2) if gap < 2**31 else (C_ - 1, C_ + 1, G_ + 1)
    sizes = [s for s in sizes if s >= 1]
    cursor, i = 0, int(rng.integers(0, 24))
    if n > 4 and i % 5 == 0:  # behind the sequence's start
        m = min(sizes[i % len(sizes)], n - 2)
        a[:m] = ord("-")
        cursor = m
    while True:
        size, mode = sizes[i % len(sizes)], i % 3
        unit = G_ if (i // 3) % 8 == 7 else C_
        back = 0 if mode == 0 else size if mode == 1 else max(1, size // 2)  # starts at / ends at / straddles the boundary
        b = (cursor + 2 + back + unit - 1) // unit * unit
        start = b - back
        if start + size > n:
            break
        a[start:start + size] = ord("-")
        a[start - 1] = ord(" ") if (i // 2) % 2 else ord("M")
        cursor = start + size
        i += 1
    if n - cursor > 3 and i % 2:  # the sequence ends in a stretch
        a[cursor + 2:] = ord("-")
    return a


def _content(kind, rng, n, gap, s):
    if kind == "all_m":
        return np.full(n, ord("M"), dtype=np.uint8)
    if kind == "all_dash":
        return np.full(n, ord("-"), dtype=np.uint8)
    if kind == "stretches":
        return _stretches(rng, n, gap)
    if kind == "matches":
        a = np.where(rng.random(n) < 0.01, ord("X"), ord("M")).astype(np.uint8)
        p = int(rng.integers(0, 2000))
        while p < n:  # a stretch of '-' about every 2 kbp, an 'R' 'R' behind some
            m = int(rng.integers(1, 40))
            a[p:p + m] = ord("-")
            if p + m + 2 <= n and m % 3 == 0:
                a[p + m:p + m + 2] = ord("R")
            p += m + int(rng.integers(1000, 3000))
        return a
    letters = np.frombuffer(b"M-XR DI", dtype=np.uint8)
    a = rng.choice(letters, n, p=[0.55, 0.15, 0.04, 0.06, 0.04, 0.08, 0.08])
    hit = rng.random(n) < 0.05
    a[hit] = rng.integers(0, 256, int(hit.sum()))
    tail = (b"MM-MMDD", b"MXM--", b"")[s % 3]
    if n >= 8 and tail:
        a[n - len(tail):] = np.frombuffer(tail, dtype=np.uint8)
    return a.astype(np.uint8)


_cache = {}


def _world(kind, gap):
    """the batch's characters and the oracle's records and first-run indices - made once, never changed"""
    ckey = (kind, gap if kind == "stretches" else 0)
    if ("chars",) + ckey not in _cache:
        rng = np.random.default_rng(CONTENTS.index(kind) * 1000 + (gap % 9973 if kind == "stretches" else 0))
        chars = np.concatenate([_content(kind, rng, n, gap, s) for s, n in enumerate(LENS)])
        chars.setflags(write=False)
        _cache[("chars",) + ckey] = chars
    chars = _cache[("chars",) + ckey]
    if (kind, gap) not in _cache:
        recs, first = ora.run_lengths_batch(chars, OFF, gap)
        recs.setflags(write=False)
        first.setflags(write=False)
        _cache[kind, gap] = (recs, first)
    return (chars,) + _cache[kind, gap]


class _Call:
    """one call's buffers on the device, every one behind guard bands at exactly its documented size"""

    def __init__(self, chars, off, capacity, seed=0):
        import torch
        self.torch = torch
        dev = torch.device("cuda", 0)
        self.n, self.total, self.capacity = len(off) - 1, int(off[-1]), int(capacity)
        self.wb = int(kbo_amd.lib().kbo_run_lengths_seq_work_bytes(self.n, self.total))
        self.chars = Guarded("d_chars", self.total + 16, PER_BASE_GUARD, dev, seed=seed + 1, data=chars)
        self.off = Guarded("d_offsets", 8 * (self.n + 1), 4096, dev, seed=seed + 2, data=off.view(np.uint8))
        self.work = Guarded("d_work", self.wb, 1 << 20, dev, seed=seed + 3)
        self.recs = Guarded("d_records", 28 * self.capacity, 1 << 20, dev, seed=seed + 4)
        self.first = Guarded("d_first", 4 * (self.n + 1), 4096, dev, seed=seed + 5)

    def launch(self, gap, stream=None):
        s = stream if stream is not None else self.torch.cuda.current_stream()
        kbo_amd.check(kbo_amd.lib().kbo_run_lengths_seq_dev(self.chars.ptr, self.off.ptr, self.n, self.total, gap, self.work.ptr, self.wb,
                                                            self.recs.ptr, self.capacity, self.first.ptr, s.cuda_stream))

    def result(self):
        """(records written (min(capacity, runs), 7), first (n + 1)) as u64"""
        self.torch.cuda.synchronize()
        for b in (self.chars, self.off, self.work, self.recs, self.first):
            b.assert_intact()
        for b in (self.chars, self.off):  # inputs are not written
            assert not b.changed(), b.name
        first = self.first.host().view(np.uint32).astype(np.uint64)
        recs = self.recs.host().view(np.uint32).reshape(-1, 7).astype(np.uint64)
        return recs[:min(self.capacity, int(first[-1]))], first


def _seg_calls():
    import ctypes as C
    c, e = C.c_uint64(), C.c_uint64()
    kbo_amd.check(kbo_amd.lib().kbo_run_lengths_seg_calls(C.byref(c), C.byref(e)))
    return c.value, e.value


def _compare(got, exp, what):
    recs, first = got
    exp_recs, exp_first = exp
    bad = np.flatnonzero(first != exp_first)
    assert not len(bad), "%s: d_first differs, first at sequence %d (%d characters): got %d, expected %d" % (
        what, bad[0], LENS[min(int(bad[0]), len(LENS) - 1)], first[bad[0]], exp_first[bad[0]])
    assert recs.shape == exp_recs.shape, what
    rows = np.flatnonzero((recs != exp_recs).any(axis=1))
    if len(rows):
        r = int(rows[0])
        s = int(np.searchsorted(exp_first, r, side="right") - 1)
        raise AssertionError("%s: %d records differ, first is record %d (sequence %d, %d characters): got %s, expected %s" % (
            what, len(rows), r, s, LENS[s], recs[r].tolist(), exp_recs[r].tolist()))


@pytest.mark.parametrize("kind", CONTENTS)
def test_every_record_against_the_oracle(kind):
    call = None
    for gap in GAPS:
        chars, exp_recs, exp_first = _world(kind, gap)
        if call is None or kind == "stretches" or len(exp_recs) > call.capacity:
            call = _Call(chars, OFF, max(len(exp_recs), 1))
        call.recs.fill(gap % 1000 + 7)
        call.first.fill(gap % 1000 + 8)
        call.launch(gap)
        recs, first = call.result()
        _compare((recs, first), (exp_recs, exp_first), "%s max_gap_len %d" % (kind, gap))


@pytest.mark.parametrize("kind", ["matches", "alphabet"])
def test_capacity_bounds_the_records_written(kind):
    gap = 1
    chars, exp_recs, exp_first = _world(kind, gap)
    runs = len(exp_recs)
    assert runs > 100
    for capacity in (runs, runs - 1, 0):  # (the buffer is exactly 28 * capacity bytes: a record too many lands in its guard)
        call = _Call(chars, OFF, capacity, seed=capacity % 100)
        call.launch(gap)
        recs, first = call.result()
        _compare((recs, first), (exp_recs[:capacity], exp_first), "%s capacity %d of %d" % (kind, capacity, runs))


def test_two_streams_with_their_own_buffers():
    import torch
    worlds = [_world("matches", 3), _world("alphabet", C_)]
    calls = [_Call(w[0], OFF, len(w[1]), seed=10 * i) for i, w in enumerate(worlds)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    before = _seg_calls()
    for c, s, gap in zip(calls, streams, (3, C_)):
        c.launch(gap, s)
    assert _seg_calls() == (before[0] + 2, before[1] + 2), "kbo_run_lengths_seg_calls counts a count and an emit a call"
    for c, w in zip(calls, worlds):
        _compare(c.result(), w[1:], "two streams")


def test_python_wrapper():
    import torch
    from kbo_amd import batch
    dev = torch.device("cuda", 0)
    chars, exp_recs, exp_first = _world("alphabet", 3)
    d_off = torch.from_numpy(OFF.astype(np.int64)).to(dev)
    recs, first = batch.run_lengths_seq(torch.from_numpy(chars.copy()).to(dev), d_off, max_gap_len=3)
    assert recs.shape == (len(exp_recs), 7) and first.numel() == len(LENS) + 1
    got = (recs.cpu().numpy().view(np.uint32).astype(np.uint64), first.cpu().numpy().view(np.uint32).astype(np.uint64))
    _compare(got, (exp_recs, exp_first), "wrapper")
    # more runs than the room the wrapper guesses (a run per 64 characters): it sizes the records from the count and runs again
    dense = np.tile(np.frombuffer(b"M-", dtype=np.uint8), 10_000)
    off = np.array([0, 7, 7, len(dense)], dtype=np.uint64)
    exp = ora.run_lengths_batch(dense, off, 0)
    assert len(exp[0]) > 2 * 3 + len(dense) // 64
    recs, first = batch.run_lengths_seq(torch.from_numpy(dense).to(dev), torch.from_numpy(off.astype(np.int64)).to(dev), stream=torch.cuda.Stream())
    torch.cuda.synchronize()
    assert np.array_equal(recs.cpu().numpy().view(np.uint32).astype(np.uint64), exp[0])
    assert np.array_equal(first.cpu().numpy().view(np.uint32).astype(np.uint64), exp[1])
