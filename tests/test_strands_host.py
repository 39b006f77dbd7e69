"""Both strands, host side (no GPU): kbo_revcomp_batch against a numpy restatement of its definition, and the argument checks of
the strand entry points, which run before any HIP call."""
import ctypes as C

import numpy as np
import pytest

import kbo_amd
from kbo_amd import batch, synth

BAD_ARG = -4
COMP = np.arange(256, dtype=np.uint8)
for _a, _b in zip(b"ACGTacgt", b"TGCAtgca"):
    COMP[_a] = _b


def np_revcomp(concat, offsets):
    """per sequence: output base i = complement of input base len - 1 - i; only A C G T a c g t change"""
    out = np.empty_like(concat)
    for s in range(len(offsets) - 1):
        a, b = int(offsets[s]), int(offsets[s + 1])
        out[a:b] = COMP[concat[a:b][::-1]]
    return out


def random_batch(rng, lens):
    """ACGT with N, lower case and bytes >= 0x80 strewn in"""
    total = int(np.sum(lens))
    q = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, total)].copy()
    r = rng.random(total)
    q[r < 0.03] = ord("N")
    low = (r >= 0.03) & (r < 0.10)
    q[low] |= 0x20
    high = (r >= 0.10) & (r < 0.13)
    q[high] = rng.integers(0x80, 0x100, int(high.sum()), dtype=np.uint8)
    other = (r >= 0.13) & (r < 0.15)
    q[other] = rng.integers(0, 0x80, int(other.sum()), dtype=np.uint8)
    return q, np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_revcomp_batch_equals_numpy(seed):
    rng = np.random.default_rng(seed)
    lens = np.concatenate([[0, 1, 0, 0, 1, 2, 3], rng.integers(0, 400, 3000), [0, 700_000, 1, 0]])
    rng.shuffle(lens[7:-4])
    concat, offsets = random_batch(rng, lens)
    got = batch.revcomp_batch(concat, offsets)
    assert np.array_equal(got, np_revcomp(concat, offsets))
    assert np.array_equal(batch.revcomp_batch(got, offsets), concat), "applied twice: the input again"


def test_revcomp_batch_every_byte_value():
    concat = np.arange(256, dtype=np.uint8)
    offsets = np.array([0, 256], dtype=np.uint64)
    got = batch.revcomp_batch(concat, offsets)
    assert np.array_equal(got, COMP[concat[::-1]])
    changed = np.flatnonzero(COMP != np.arange(256))
    assert sorted(changed.tolist()) == sorted(b"ACGTacgt")


def test_revcomp_batch_bad_arguments():
    L = kbo_amd.lib()
    concat = np.frombuffer(b"ACGTACGTAC", dtype=np.uint8).copy()
    offsets = np.array([0, 4, 10], dtype=np.uint64)
    out = np.zeros(10, dtype=np.uint8)
    c, o, d = concat.ctypes.data, offsets.ctypes.data, out.ctypes.data
    assert L.kbo_revcomp_batch(None, o, 2, d) == BAD_ARG
    assert L.kbo_revcomp_batch(c, None, 2, d) == BAD_ARG
    assert L.kbo_revcomp_batch(c, o, 2, None) == BAD_ARG
    assert L.kbo_revcomp_batch(c, o, 2, c) == BAD_ARG, "in place"
    assert L.kbo_revcomp_batch(c, o, 2, c + 9) == BAD_ARG, "one byte of overlap"
    assert L.kbo_revcomp_batch(c + 5, np.array([0, 5], dtype=np.uint64).ctypes.data, 1, c) == 0, "adjacent is not overlapping"
    bad = np.array([0, 6, 4], dtype=np.uint64)
    assert L.kbo_revcomp_batch(c, bad.ctypes.data, 2, d) == BAD_ARG, "offsets not monotone"


def test_device_entry_points_check_arguments_before_any_hip_call():
    L = kbo_amd.lib()
    buf = (C.c_uint8 * 4096)()
    base = (C.addressof(buf) + 255) // 256 * 256  # host memory stands in for device memory: the checks never touch it
    a, b, off, scr = base, base + 1024, base + 2048, base + 3072
    assert L.kbo_revcomp_batch_dev(None, off, 1, 100, 0, b, None) == BAD_ARG
    assert L.kbo_revcomp_batch_dev(a, None, 1, 100, 0, b, None) == BAD_ARG
    assert L.kbo_revcomp_batch_dev(a, off, 1, 100, 0, None, None) == BAD_ARG
    assert L.kbo_revcomp_batch_dev(a, off, 1, 100, 0, a, None) == BAD_ARG, "in place"
    assert L.kbo_revcomp_batch_dev(a, off, 1, 100, 0, a + 96, None) == BAD_ARG, "overlapping"
    assert L.kbo_revcomp_batch_dev(a + 4, off, 1, 100, 0, b, None) == BAD_ARG, "d_concat not 16-byte aligned"
    assert L.kbo_revcomp_packed_dev(None, off, 1, 7, None, None, 0, b, None, None, scr, None) == BAD_ARG
    assert L.kbo_revcomp_packed_dev(a, off, 1, 7, None, None, 0, None, None, None, scr, None) == BAD_ARG
    assert L.kbo_revcomp_packed_dev(a, off, 1, 7, None, None, 0, b, None, None, None, None) == BAD_ARG
    assert L.kbo_revcomp_packed_dev(a, off, 1, 7, None, None, 3, b, None, None, scr, None) == BAD_ARG, "a list without its arrays"
    assert L.kbo_revcomp_packed_dev(a, off, 1, 7, None, None, 0, a + 24, None, None, scr, None) == BAD_ARG, "overlapping words"
    assert L.kbo_revcomp_packed_scratch_bytes(0) == 0 and L.kbo_revcomp_packed_scratch_bytes(1000) % 16 == 0


def test_strand_entry_points_refuse_bad_arguments_without_a_gpu():
    L = kbo_amd.lib()
    g = synth.genome(5000, seed=3)
    sbwt, _ = kbo_amd.build([g], kbo_amd.BuildOpts(k=31, num_threads=2))
    concat = g[:300].copy()
    offsets = np.array([0, 150, 300], dtype=np.uint64)
    fwd, rev = np.zeros(300, dtype=np.uint8), np.zeros(300, dtype=np.uint8)
    words, epos, ebyt = batch.pack_reads(concat, offsets)
    wf, wr = np.zeros(len(words), dtype=np.uint32), np.zeros(len(words), dtype=np.uint32)
    ro = np.zeros(5, dtype=np.uint64)
    p = C.POINTER(kbo_amd._capi.RLE)()
    vp = C.c_void_p()
    h, c, o = sbwt._h, concat.ctypes.data, offsets.ctypes.data
    for strands in (0, 4, -1):
        assert L.kbo_matches_batch_strands(h, c, o, 2, 1e-7, 0, strands, fwd.ctypes.data, rev.ctypes.data) == BAD_ARG
        assert L.kbo_find_batch_strands(h, c, o, 2, None, strands, C.byref(p), ro.ctypes.data) == BAD_ARG
        assert L.kbo_matches_batch_packed_strands(h, words.ctypes.data, o, 2, None, None, 0, 1e-7, strands, wf.ctypes.data,
                                                  wr.ctypes.data) == BAD_ARG
        assert L.kbo_find_batch_packed_strands(h, words.ctypes.data, o, 2, None, None, 0, None, strands, C.byref(vp),
                                               ro.ctypes.data) == BAD_ARG
    # null arguments; the output of a strand that is asked for
    assert L.kbo_matches_batch_strands(None, c, o, 2, 1e-7, 0, 3, fwd.ctypes.data, rev.ctypes.data) == BAD_ARG
    assert L.kbo_matches_batch_strands(h, None, o, 2, 1e-7, 0, 3, fwd.ctypes.data, rev.ctypes.data) == BAD_ARG
    assert L.kbo_matches_batch_strands(h, c, None, 2, 1e-7, 0, 3, fwd.ctypes.data, rev.ctypes.data) == BAD_ARG
    assert L.kbo_matches_batch_strands(h, c, o, 2, 1e-7, 0, 3, fwd.ctypes.data, None) == BAD_ARG
    assert L.kbo_matches_batch_strands(h, c, o, 2, 1e-7, 0, 3, None, rev.ctypes.data) == BAD_ARG
    assert L.kbo_matches_batch_strands(h, c, o, 2, 1e-7, 0, 1, None, rev.ctypes.data) == BAD_ARG
    assert L.kbo_matches_batch_strands(h, c, o, 2, 1e-7, 0, 2, fwd.ctypes.data, None) == BAD_ARG
    assert L.kbo_find_batch_strands(h, c, o, 2, None, 3, None, ro.ctypes.data) == BAD_ARG
    assert L.kbo_find_batch_strands(h, c, o, 2, None, 3, C.byref(p), None) == BAD_ARG
    assert L.kbo_find_batch_strands(h, None, o, 2, None, 3, C.byref(p), ro.ctypes.data) == BAD_ARG
    assert L.kbo_matches_batch_packed_strands(h, None, o, 2, None, None, 0, 1e-7, 3, wf.ctypes.data, wr.ctypes.data) == BAD_ARG
    assert L.kbo_matches_batch_packed_strands(h, words.ctypes.data, o, 2, None, None, 0, 1e-7, 3, wf.ctypes.data, None) == BAD_ARG
    assert L.kbo_matches_batch_packed_strands(h, words.ctypes.data, None, 2, None, None, 0, 1e-7, 3, wf.ctypes.data, wr.ctypes.data) == BAD_ARG
    assert L.kbo_find_batch_packed_strands(h, words.ctypes.data, o, 2, None, None, 0, None, 3, None, ro.ctypes.data) == BAD_ARG
    assert L.kbo_find_batch_packed_strands(h, None, o, 2, None, None, 0, None, 3, C.byref(vp), ro.ctypes.data) == BAD_ARG
    assert L.kbo_last_batch_staged_bytes() >= 0
