"""map_reads_kernel's direct forms with bytes out (kbo_amd/csrc/map_kernels.hip), every output byte: stage 0 reads the batch's bases
with streaming loads, stage 5 expands each 16-byte block of 2-bit codes and stores it - whole blocks as streaming 16-byte stores, the
wave's first and last block byte by byte inside [first byte, last byte) of its reads.  Up to three writers touch one output byte: the
wave that holds it, a neighbouring wave whose partial block shares its 16 bytes, and the second pass (finish_reads_kernel, a later
launch) over the reads the kernel leaves.

The cases were laid out for a form of stage 5 that stores a block's default characters early and expands only the blocks that differ,
listed across the wave (measured and not kept: LABNOTES round 7) - waves with no, with 63 .. 192 and with all 600 blocks holding a
character other than 'M', read counts around a wave, lengths that put read boundaries inside blocks.  They are what any form of that
stage has to get right, so they stay.

Every case goes through kbo_map_batch_dev / kbo_find_batch_dev with d_concat, d_offsets, d_ms, d_chars_out and d_work at exactly their
documented sizes between guard bands (gpu_helpers.Guarded), asserts the one-kernel route, compares EVERY specified output byte with
the oracle (matches_batch, then relative_to_ref where the format is on) and asserts every guard intact.  The index is built as in
test_gpu_map_reads.py::test_read_shapes_and_contents (300 kbp, k = 31: a copy with a depth table).  In the cases that are to exercise
the kernel's own stage 5 (0 - 1 % substitutions, planted substitutions) at most a tenth of the reads may be left to the second pass
(kbo_plan_flags_dev, as test_how_many_reads_the_kernel_leaves_to_the_second_pass reads them): it would rewrite their bytes.

offsets[0] is 0 by contract, so a batch's first wave starts 16-aligned; a first read of 5 bases in front of reads of 150 puts the
first byte of every LATER wave at 1 mod 16 - both its first and its last block are partial.  The packed-in / bytes-out form (IO = 1)
has no device-resident entry point: it is reached through the host calls kbo_matches_batch_sparse and kbo_find_batch_packed, which
report no route and, like the reference, refuse sequences of fewer than 3 bases: those cases compare the characters and the runs alone."""
import ctypes as C

import numpy as np
import pytest

import kbo_amd
from kbo_amd import batch, synth
from gpu_helpers import PER_BASE_GUARD, Guarded, scratch_guard_bytes, threads

pytestmark = pytest.mark.gpu

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
K = 31
WAVE = 64           # reads a wave
MANY = 256          # of a wave's 600 blocks: "most of them"
PLANT_AT = (40, 75, 110)  # bases of a 150-base read: more than k apart and more than k from either end - one 'X' each, nothing else


def _dev():
    import torch
    return torch.device("cuda:0")


def _substitute(rng, r, rate):
    """substitutions that always change the base"""
    r = r.copy()
    hit = np.flatnonzero(rng.random(len(r)) < rate)
    r[hit] = ACGT[(np.searchsorted(ACGT, r[hit]) + rng.integers(1, 4, len(hit))) % 4]
    return r


def _take(rng, g, n, length):
    lens = np.full(n, length) if np.isscalar(length) else rng.choice(length, n)
    return [g[a:a + int(l)].copy() for a, l in zip(rng.integers(0, len(g) - 200, n), lens)]


def _plant(rng, g, counts):
    """a wave of 64 reads of 150 bases per entry of `counts`, with exactly that many substitutions, each in a block of its own"""
    reads = []
    for n_sub in counts:
        wave = _take(rng, g, WAVE, 150)
        slots = [(r, p) for p in PLANT_AT for r in range(WAVE)][:n_sub]
        assert len(slots) == n_sub
        for r, p in slots:
            wave[r][p] = ACGT[(int(np.searchsorted(ACGT, wave[r][p])) + 1 + (r + p) % 3) % 4]
        reads += wave
    return reads


PLANTED = (63, 64, 65, 0, 127, 128, 129, 191, 192)  # dirty blocks of the batch's waves: either side of 64, 128 and 192 (a round of the wave's lanes)


def _cases(g, other):
    """name -> (reads, stage-5 case: at most a tenth of the reads may go to the second pass)"""
    rng = np.random.default_rng(20_26)
    c = {}
    for n in (1, 63, 64, 65, 129):  # the last wave is partial
        c["reads_%d" % n] = ([_substitute(rng, r, 0.01) for r in _take(rng, g, n, 150)], True)
    for length in (150, 149, 33, 17, 16, 3):  # not multiples of 16: a read boundary inside a block
        c["len_%d" % length] = ([_substitute(rng, r, 0.01) for r in _take(rng, g, 200, length)], True)
    c["len_mixed"] = ([_substitute(rng, r, 0.01) for r in _take(rng, g, 300, [150, 149, 33, 17, 16, 3, 160, 100, 48])], True)
    # every wave but the first starts at 1 mod 16 (module docstring)
    c["unaligned_waves"] = ([g[1000:1005].copy()] + [_substitute(rng, r, 0.01) for r in _take(rng, g, 200, 150)], True)
    c["clean"] = (_take(rng, g, 200, 150), True)  # no dirty block
    c["planted"] = (_plant(rng, g, PLANTED), True)
    # most blocks dirty: reads of another genome (all '-': 600 dirty blocks a wave), 5 - 10 % substitutions
    unrelated = [other[a:a + 150].copy() for a in rng.integers(0, len(other) - 150, 2 * WAVE)]
    c["unrelated"] = (unrelated, False)
    c["sub_5_to_10"] = ([_substitute(rng, r, rate) for rate in (0.05, 0.07, 0.10) for r in _take(rng, g, WAVE, 150)], False)
    mix = []
    for w in range(6):  # whole waves in turn: all '-', clean, 8 % substitutions, ...
        mix += (unrelated[:WAVE], _take(rng, g, WAVE, 150), [_substitute(rng, r, 0.08) for r in _take(rng, g, WAVE, 150)])[w % 3]
    c["dense_mixed_with_clean"] = (mix + _take(rng, g, 7, 150), False)
    # three writers on one byte
    nn = _take(rng, g, 120, 150)  # (150 = 6 mod 16: every read boundary lies inside a block)
    for i in range(1, 119, 4):
        nn[i][-1 if i % 8 == 1 else 0] = ord("N")  # the block it shares with a clean neighbour
    c["non_acgt_next_to_clean"] = (nn, False)
    fl = _take(rng, g, 128, 150)
    for i in range(0, 128, 2):
        fl[i] = _substitute(rng, fl[i], 0.12)  # (18 mismatches: its list holds 13 - the second pass's; its neighbours are finished here)
    c["flagged_next_to_finished"] = (fl, False)
    tiny = []
    for i, r in enumerate(_take(rng, g, 150, 150)):
        tiny.append(_substitute(rng, r, 0.01))
        tiny.append(ACGT[rng.integers(0, 4, i % 3)])  # 0, 1 and 2 bases
    c["empty_and_tiny_between"] = (tiny, True)
    return c


CASE_NAMES = ["reads_1", "reads_63", "reads_64", "reads_65", "reads_129", "len_150", "len_149", "len_33", "len_17", "len_16", "len_3",
              "len_mixed", "unaligned_waves", "clean", "planted", "unrelated", "sub_5_to_10", "dense_mixed_with_clean",
              "non_acgt_next_to_clean", "flagged_next_to_finished", "empty_and_tiny_between"]


class Expected:
    """a case's batch and what the oracle says about it, computed once"""

    def __init__(self, oracle, ora, reads, stage5):
        self.stage5 = stage5
        self.concat = np.concatenate(reads)
        self.lens = np.array([len(r) for r in reads], dtype=np.int64)
        self.offsets = np.concatenate([[0], np.cumsum(self.lens)]).astype(np.uint64)
        self.n, self.total, self.max_len = len(reads), int(self.offsets[-1]), int(self.lens.max())
        # (sequences of fewer than 3 bases: their bytes are unspecified, and the oracle, like the reference, refuses them)
        self.keep = np.repeat(self.lens >= 3, self.lens)
        self.big_off = np.concatenate([[0], np.cumsum(self.lens[self.lens >= 3])]).astype(np.uint64)
        self.chars = np.zeros(self.total, dtype=np.uint8)
        self.chars[self.keep] = ora.matches_batch(self.concat[self.keep], self.big_off, 1e-7, n_threads=threads())
        self.map = np.frombuffer(oracle.relative_to_ref(self.concat, self.chars), dtype=np.uint8)
        recs, first_big = oracle.run_lengths_batch(self.chars[self.keep], self.big_off, 0)
        before = np.concatenate([[0], np.cumsum(self.lens >= 3)])
        self.runs, self.first = recs, np.asarray(first_big, dtype=np.uint64)[before]
        for v in (self.concat, self.offsets, self.keep, self.chars, self.map, self.runs, self.first):
            v.setflags(write=False)

    def dirty_blocks(self, wave):
        """16-byte blocks of the wave's stretch that hold a character other than 'M'"""
        a, b = int(self.offsets[WAVE * wave]), int(self.offsets[min(WAVE * (wave + 1), self.n)])
        at = np.flatnonzero(self.chars[a:b] != ord("M")) + a
        return len(np.unique(at // 16))


@pytest.fixture(scope="module")
def world(oracle):
    g = synth.genome(300_000, seed=931)
    sbwt, _ = kbo_amd.build([g], kbo_amd.BuildOpts(k=K, num_threads=threads()))
    ora = oracle.Index.build([g.tobytes()], k=K)
    sbwt.to_device(-1)
    assert sbwt.depth_table_order() > 0
    cases = _cases(g, synth.genome(50_000, seed=77))
    assert sorted(cases) == sorted(CASE_NAMES)
    return {"sbwt": sbwt, "ora": ora, "oracle": oracle, "cases": cases, "expected": {}}


def _expected(world, name):
    if name not in world["expected"]:
        reads, stage5 = world["cases"][name]
        world["expected"][name] = Expected(world["oracle"], world["ora"], reads, stage5)
    return world["expected"][name]


def _first_difference(got, want, keep, offsets, what):
    bad = np.flatnonzero((got != want) & keep)
    if len(bad):
        s = int(np.searchsorted(offsets, bad[0], side="right")) - 1
        a, b = int(offsets[s]), int(offsets[s + 1])
        raise AssertionError("%s: %d bytes differ from the oracle, the first in read %d (%d bases, wave %d) at base %d (byte %d of the batch)\n got  %s\n want %s" % (
            what, len(bad), s, b - a, s // WAVE, int(bad[0]) - a, int(bad[0]), got[a:b].tobytes(), want[a:b].tobytes()))


def _run(world, name, fmt, find):
    """the case through kbo_map_batch_dev (find: kbo_find_batch_dev, max_gap_len = 0) -> the share of the reads left to the second pass"""
    import torch
    L, sbwt, e = kbo_amd.lib(), world["sbwt"], _expected(world, name)
    dev = _dev()
    what = "%s, %s" % (name, "find" if find else "relative_to_ref" if fmt else "matches")
    q = Guarded("d_concat", e.total + 16, PER_BASE_GUARD, dev, data=e.concat)
    off = Guarded("d_offsets", 8 * (e.n + 1), PER_BASE_GUARD, dev, data=e.offsets.view(np.uint8))
    ms = Guarded("d_ms", e.total + 16, PER_BASE_GUARD, dev, seed=1)
    chars = Guarded("d_chars_out", e.total + 16, PER_BASE_GUARD, dev, seed=3)
    wb = int(L.kbo_index_work_bytes(sbwt._h, e.n, e.total, e.max_len))
    work = Guarded("d_work", wb, scratch_guard_bytes(e.n, e.total, K), dev, seed=2)
    bufs = [q, off, ms, chars, work]
    s = torch.cuda.current_stream(dev).cuda_stream
    fused = C.c_int(-1)
    L.kbo_set_plan(1, 0, 0)  # (a batch that left most of its reads holds the copy off: clear it)
    if find:
        rle = Guarded("d_rle_work", int(L.kbo_run_lengths_work_bytes(e.n)), scratch_guard_bytes(e.n, e.total, K), dev, seed=4)
        recs = Guarded("d_records", 28 * len(e.runs), PER_BASE_GUARD, dev, seed=6)
        bufs += [rle, recs]
        kbo_amd.check(L.kbo_find_batch_dev(sbwt._h, q.ptr, off.ptr, e.n, e.total, e.max_len, 1e-7, 0, ms.ptr, chars.ptr, work.ptr, wb,
                                           rle.ptr, recs.ptr, len(e.runs), s, s, C.byref(fused)))
    else:
        kbo_amd.check(L.kbo_map_batch_dev(sbwt._h, q.ptr, off.ptr, e.n, e.total, e.max_len, 1e-7, int(fmt), 0, ms.ptr, chars.ptr, work.ptr,
                                          wb, s, C.byref(fused)))
    torch.cuda.synchronize()
    assert fused.value == 1, "%s: not the one kernel (fused = %d)" % (what, fused.value)
    _first_difference(chars.host()[:e.total], e.map if fmt else e.chars, e.keep, e.offsets, what)
    if find:
        w = rle.host().view(np.uint32)
        words = e.n + 1 + (e.n + 1 + 1023) // 1024
        assert int(w[words]) == len(e.runs), "%s: %d runs counted, %d expected" % (what, int(w[words]), len(e.runs))
        first = w[e.n + 1 + np.arange(e.n + 1) // 1024].astype(np.uint64) + w[:e.n + 1]
        assert np.array_equal(first, e.first), what + ": first-run indices"
        assert np.array_equal(recs.host().view(np.uint32).reshape(-1, 7).astype(np.uint64), e.runs), what + ": run records"
    for x in bufs:
        x.assert_intact(what)
    flags = np.zeros(e.n, dtype=np.uint8)
    kbo_amd.check(L.kbo_plan_flags_dev(e.n, e.total, e.max_len, K, work.ptr, flags.ctypes.data, s))
    share = float((flags != 0).mean())
    print("%s: %d reads, %.2f %% left to the second pass" % (what, e.n, 100.0 * share))
    if e.stage5:
        assert share <= 0.10, "%s: %.1f %% of the reads went to the second pass, which would rewrite what stage 5 stored" % (what, 100.0 * share)
    return share


def test_the_planted_waves_hold_the_dirty_blocks_they_are_named_for(world):
    """the oracle's characters of the planted batch: wave w has PLANTED[w] blocks with a character other than 'M' (one 'X' each); the
    clean batch has none; every wave of the other batches that is not clean has more than MANY"""
    e = _expected(world, "planted")
    assert [e.dirty_blocks(w) for w in range(len(PLANTED))] == list(PLANTED)
    assert int((e.chars != ord("M")).sum()) == sum(PLANTED) and int((e.chars == ord("X")).sum()) == sum(PLANTED)
    c = _expected(world, "clean")
    assert bool((c.chars == ord("M")).all())
    u = _expected(world, "unrelated")
    assert min(u.dirty_blocks(w) for w in range(2)) > MANY
    m = _expected(world, "dense_mixed_with_clean")
    counts = [m.dirty_blocks(w) for w in range(6)]
    assert all(n == 0 for n in counts[1::3]) and all(n > MANY for n in counts[0::3] + counts[2::3]), counts
    s = _expected(world, "sub_5_to_10")
    assert s.dirty_blocks(0) > 64 and s.dirty_blocks(2) > MANY


@pytest.mark.parametrize("fmt", [False, True], ids=["matches", "relative_to_ref"])
@pytest.mark.parametrize("name", CASE_NAMES)
def test_every_byte_against_the_oracle(world, name, fmt):
    _run(world, name, fmt, find=False)


@pytest.mark.parametrize("name", ["reads_129", "len_mixed", "unaligned_waves", "planted", "dense_mixed_with_clean",
                                  "flagged_next_to_finished", "empty_and_tiny_between"])
def test_find_characters_and_runs(world, name):
    """kbo_find_batch_dev with max_gap_len = 0: the kernel counts the runs off its codes, the characters leave as above"""
    _run(world, name, False, find=True)


@pytest.mark.parametrize("name", ["reads_129", "len_mixed", "planted", "dense_mixed_with_clean", "non_acgt_next_to_clean"])
def test_packed_in_bytes_out(world, name):
    """the reads as 2-bit words in, the characters as bytes out (IO = 1), through the host calls that need bytes on the device: the
    sparse records (made from those bytes; expanded, they are every character) and kbo::find's runs"""
    e = _expected(world, name)
    words, pos, byt = batch.pack_reads(e.concat, e.offsets)
    kbo_amd.lib().kbo_set_plan(1, 0, 0)
    runs = batch.matches_batch_sparse(world["sbwt"], words, e.offsets, pos, byt)
    _first_difference(batch.expand_sparse(runs, e.offsets), e.chars, e.keep, e.offsets, name + ", sparse, expanded")
    _first_difference(batch.expand_sparse(runs, e.offsets, ref=e.concat), e.map, e.keep, e.offsets, name + ", sparse, expanded with the reads")
    kbo_amd.lib().kbo_set_plan(1, 0, 0)
    recs, first = batch.find_batch_packed(world["sbwt"], words, e.offsets, pos, byt)
    assert np.array_equal(np.asarray(first, dtype=np.uint64), e.first), name + ": first-run indices"
    assert np.array_equal(recs, e.runs), name + ": run records"
