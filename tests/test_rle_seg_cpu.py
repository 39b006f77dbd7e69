"""The segmented run-length stage on the host (kbo_hip.h kbo_run_lengths_seq_dev, kbo_hip_tuning.h kbo_run_lengths_seq_host): the algebra
the kernels run - chunk summaries and their combines, kbo_amd/csrc/rle_seg.hpp - restated on the CPU at chunk sizes at which every
boundary case is a few bytes long, against the oracle's literal loop; the scratch figure; the argument errors, which come back before
anything is enqueued (the pointers are dummy integers, suitably aligned, that nothing ever follows)."""
import itertools
import os
import re
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import kbo_amd
from oracle import binding as ora

E_EMPTY_QUERY, E_BAD_ARG, E_UNSUPPORTED = -1, -4, -8
CHUNK, GROUP = 128, 8192  # KBO_RLE_SEG_CHUNK, _GROUP (tests/test_gpu_rle_seg.py builds its shapes from them)
ALPHABET = b"M-XR DI"
GAPS = (0, 1, 2, 3, 2**32 - 1)
SHAPES = ((1, 1), (1, 2), (2, 4), (3, 3), (3, 6), (128, 8192))  # (chunk, group)
CHARS, OFF, WORK, RECS, FIRST = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000


def test_tuning_constants_are_the_headers():
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "kbo_hip_tuning.h")).read()
    assert int(re.search(r"#define KBO_RLE_SEG_CHUNK (\d+)", hdr).group(1)) == CHUNK
    assert int(re.search(r"#define KBO_RLE_SEG_GROUP (\d+)", hdr).group(1)) == GROUP
    assert GROUP % CHUNK == 0


def host_runs(aln, off, gap, chunk, group, min_len, capacity=None, each=False):
    """kbo_run_lengths_seq_host -> (records (n, 7) u32, first (n_seqs + 1) u32); capacity None: twice a call, the second with room for all.
    each: every sequence as a batch of its own (kbo_run_lengths_seq_host_each)"""
    aln = np.ascontiguousarray(aln, dtype=np.uint8)
    off = np.ascontiguousarray(off, dtype=np.uint64)
    n = len(off) - 1
    first = np.zeros(n + 1, dtype=np.uint32)
    buf = aln if len(aln) else np.zeros(1, dtype=np.uint8)
    cap = 0 if capacity is None else capacity
    recs = np.full((max(cap, 1) + 1, 7), 0xEEEEEEEE, dtype=np.uint32)
    fn = kbo_amd.lib().kbo_run_lengths_seq_host_each if each else kbo_amd.lib().kbo_run_lengths_seq_host
    kbo_amd.check(fn(buf.ctypes.data, off.ctypes.data, n, gap, chunk, group, min_len, recs.ctypes.data, cap, first.ctypes.data))
    if capacity is None:
        return host_runs(aln, off, gap, chunk, group, min_len, int(first[n]), each)
    assert (recs[cap:] == 0xEEEEEEEE).all(), "a record behind the capacity was written"
    return recs[:min(cap, int(first[n]))], first


def expected(aln, off, gap, min_len):
    """the oracle's records and first-run indices; a sequence shorter than min_len has no run"""
    recs, ro = ora.run_lengths_batch(aln, off, gap)
    if min_len:
        lens = np.diff(np.asarray(off, dtype=np.uint64))
        per = np.diff(ro).astype(np.int64)
        keep = np.repeat(lens >= min_len, per)
        recs = recs[keep]
        ro = np.concatenate(([0], np.cumsum(np.where(lens >= min_len, per, 0)))).astype(np.uint64)
    return recs, ro


def check(aln, off, gap, chunk, group, min_len, exp=None, each=False):
    exp_recs, exp_first = exp if exp is not None else expected(aln, off, gap, min_len)
    recs, first = host_runs(aln, off, gap, chunk, group, min_len, each=each)
    assert np.array_equal(first.astype(np.uint64), exp_first), (gap, chunk, group, min_len)
    assert np.array_equal(recs.astype(np.uint64), exp_recs), (gap, chunk, group, min_len)


@pytest.fixture(scope="module")
def every_string():
    """every string over ALPHABET of length 0 .. 7, packed into one batch in slices: [(aln, offsets)]"""
    strings = [np.zeros((1, 0), dtype=np.uint8)]
    letters = np.frombuffer(ALPHABET, dtype=np.uint8)
    for n in range(1, 8):
        idx = np.indices((len(letters),) * n).reshape(n, -1).T
        strings.append(letters[idx])
    slices = []
    for block in strings:
        n, width = block.shape
        for a in range(0, n, 1 << 17):
            part = block[a:a + (1 << 17)]
            slices.append((part.reshape(-1).copy(), (np.arange(len(part) + 1, dtype=np.uint64) * width)))
    return slices


EXPECTED = {}  # (slice, max_gap_len, min_len) -> the oracle's (records, first): computed once, shared, never changed


def _expect(every_string):
    if not EXPECTED:
        for i, (aln, off) in enumerate(every_string):
            for gap in GAPS:
                for min_len in (0, 3):
                    EXPECTED[i, gap, min_len] = expected(aln, off, gap, min_len)


def test_every_short_string_in_batches(every_string):
    """exhaustive: 960 800 strings as the sequences of packed batches (the neighbours' bytes right next to them), every max_gap_len,
    chunk and group shape and min_len"""
    _expect(every_string)
    exp = EXPECTED
    assert sum(len(off) - 1 for _, off in every_string) == sum(7 ** n for n in range(8))
    assert sum(len(exp[i, 0, 0][0]) for i in range(len(every_string))) > 10 ** 6

    def one(task):
        i, gap, (chunk, group), min_len = task
        aln, off = every_string[i]
        check(aln, off, gap, chunk, group, min_len, exp[i, gap, min_len])
    with ThreadPoolExecutor(8) as pool:
        list(pool.map(one, itertools.product(range(len(every_string)), GAPS, SHAPES, (0, 3))))


def test_every_short_string_alone(every_string):
    """exhaustive again, every string of length 0 .. 7 as a batch of ONE sequence in a buffer of exactly its length - nothing in front
    of it and nothing behind, n_seqs == 1 over up to seven chunks - for every max_gap_len, shape and min_len.  The loop over the
    960 800 calls is native (kbo_run_lengths_seq_host_each); a few hundred go through Python one by one as well"""
    def one(task):
        i, gap, (chunk, group), min_len = task
        aln, off = every_string[i]
        check(aln, off, gap, chunk, group, min_len, EXPECTED[i, gap, min_len], each=True)
    _expect(every_string)
    with ThreadPoolExecutor(8) as pool:
        list(pool.map(one, itertools.product(range(len(every_string)), GAPS, SHAPES, (0, 3))))
    rng = np.random.default_rng(3)
    for n in (0, 1, 2, 6, 7):
        for _ in range(1 if n == 0 else 12):
            s = bytes(rng.choice(np.frombuffer(ALPHABET, dtype=np.uint8), n))
            for gap in GAPS:
                for chunk, group in SHAPES:
                    recs, first = host_runs(np.frombuffer(s, dtype=np.uint8), [0, n], gap, chunk, group, 0)
                    assert [tuple(r) for r in recs.tolist()] == [tuple(x) for x in ora.run_lengths_gapped(s, gap)], (s, gap, chunk, group)
                    assert first.tolist() == [0, len(recs)]


def test_random_strings_with_arbitrary_bytes():
    rng = np.random.default_rng(20240611)
    letters = np.frombuffer(ALPHABET, dtype=np.uint8)
    seqs = []
    for i in range(600):
        n = int(rng.integers(1, 401))
        kind = i % 4
        if kind == 0:    # the alphabet, '-' and 'M' heavy
            a = rng.choice(letters, n, p=[0.3, 0.4, 0.05, 0.05, 0.1, 0.05, 0.05])
        elif kind == 1:  # long stretches
            a = np.repeat(rng.choice(letters, n, p=[0.3, 0.4, 0.05, 0.05, 0.1, 0.05, 0.05]), rng.integers(1, 30, n))[:n]
        elif kind == 2:  # any byte
            a = rng.integers(0, 256, n).astype(np.uint8)
        else:            # any byte among stretches of '-'
            a = np.where(rng.random(n) < 0.6, ord("-"), rng.integers(0, 256, n)).astype(np.uint8)
        seqs.append(a.astype(np.uint8))
    aln = np.concatenate(seqs)
    off = np.concatenate(([0], np.cumsum([len(s) for s in seqs]))).astype(np.uint64)
    for gap in GAPS + (5, 17, 40, 399):
        for min_len in (0, 3):
            exp = expected(aln, off, gap, min_len)
            for chunk, group in ((3, 6), (7, 28), (3, 3), (7, 7)):
                check(aln, off, gap, chunk, group, min_len, exp)


def test_capacity_and_bad_shapes():
    aln = np.frombuffer(b"MM-MM MX--M-", dtype=np.uint8)
    off = np.array([0, 6, 12], dtype=np.uint64)
    exp_recs, exp_first = expected(aln, off, 0, 0)
    for cap in (0, 1, len(exp_recs) - 1, len(exp_recs)):
        recs, first = host_runs(aln, off, 0, 2, 4, 0, capacity=cap)
        assert np.array_equal(first.astype(np.uint64), exp_first) and np.array_equal(recs.astype(np.uint64), exp_recs[:cap])
    L = kbo_amd.lib()
    first = np.zeros(3, dtype=np.uint32)
    for chunk, group in ((0, 0), (2, 3), (2, 0), (4, 2)):
        assert L.kbo_run_lengths_seq_host(aln.ctypes.data, off.ctypes.data, 2, 0, chunk, group, 0, None, 0, first.ctypes.data) == E_BAD_ARG


def header_formula(n_seqs, total):
    return total * 77 // 128 + n_seqs * 158


def test_work_bytes_positive_monotone_and_the_headers_formula():
    wb = kbo_amd.lib().kbo_run_lengths_seq_work_bytes
    assert wb(1, 0) > 0 and wb(1, 3) > 0
    seqs = [wb(n, 1 << 20) for n in (1, 2, 3, 100, 1023, 1024, 1025, 100_000, 10_000_000)]
    assert seqs == sorted(seqs) and len(set(seqs)) == len(seqs)
    bases = [wb(1000, b) for b in (0, 3000, 3001, 127_999, 128_000, 128_001, 1 << 20, (1 << 20) + 1, 1 << 30, (1 << 32) - 16)]
    assert bases == sorted(bases) and bases[-1] > bases[0]
    for n, total in ((1, 0), (7, 12345), (1000, 1 << 24), (167, 1 << 24), (1 << 20, 1 << 27), (100_000, 1 << 30)):
        assert wb(n, total) % 16 == 0
    for n, total in ((1000, 1 << 24), (167, 1 << 24), (1 << 20, 1 << 27), (100_000, 1 << 30), (1 << 16, 1 << 20)):
        assert abs(wb(n, total) - header_formula(n, total)) < 0.02 * wb(n, total), (n, total)


def test_argument_errors_need_no_device():
    L = kbo_amd.lib()
    n, total = 4, 1000
    wb = int(L.kbo_run_lengths_seq_work_bytes(n, total))

    def call(chars=CHARS, off=OFF, n_seqs=n, total_bases=total, gap=0, work=WORK, work_bytes=wb, recs=RECS, capacity=16, first=FIRST):
        return L.kbo_run_lengths_seq_dev(chars, off, n_seqs, total_bases, gap, work, work_bytes, recs, capacity, first, None)
    for null in ("chars", "off", "work", "recs", "first"):
        assert call(**{null: None}) == E_BAD_ARG, null
    assert call(work_bytes=wb - 1) == E_BAD_ARG and call(work_bytes=0) == E_BAD_ARG
    assert call(n_seqs=n + 1) == E_BAD_ARG, "a sequence more needs more scratch"
    assert call(total_bases=total + 4096) == E_BAD_ARG, "more bases need more scratch"
    for name, base, step in (("off", OFF, 4), ("recs", RECS, 2), ("first", FIRST, 1), ("work", WORK, 4), ("work", WORK, 8)):
        assert call(**{name: base + step}) == E_BAD_ARG, name
    assert call(n_seqs=0) == E_EMPTY_QUERY
    assert call(total_bases=(1 << 32) - 15, work_bytes=1 << 60) == E_UNSUPPORTED
    assert call(total_bases=1 << 40, work_bytes=1 << 60) == E_UNSUPPORTED
    assert call(n_seqs=1 << 28, work_bytes=1 << 60) == E_UNSUPPORTED
