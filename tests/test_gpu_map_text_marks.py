"""map_reads_kernel's compare step over the text without its marks (kbo_amd/csrc/map_text.hpp: pc_t, the summary bits pc_mu, the coarse
summary pc_mc; the marks themselves from pc_tm only for a window that has any), every output byte against the oracle, on an index
whose path-cover text has several path starts: 12 contigs of 300 - 500 bases and one of 300 kbp, k = 31.

Method as in test_gpu_map_default_line.py (its _run and Expected are used as they are): kbo_map_batch_dev / kbo_find_batch_dev with
every buffer at exactly its documented size between guard bands, the one-kernel route asserted, EVERY specified output byte compared
with the oracle, every guard intact.  The same batches then go through the kernel's other instantiations: want_ms (the MS bytes equal
to the oracle's) and kbo_summary_batch_dev.

Cases:
  substitutions      1 % substitutions, starts at each of 16 consecutive offsets (every alignment of the window in its unit) of a short
                     contig and of the long one, lengths 1, 3, 15, 16, 17, 31, 149, 150, 160; at most a tenth of the reads may be left to
                     the second pass (kbo_plan_flags_dev): it would rewrite what the kernel made of them
  path_start_inside  for every ordered pair (a, b) of short contigs and every split s in SPLITS: the last s bases of a, then the first
                     150 - s of b.  Whichever pairs are neighbours in the path-cover text match their diagonal ACROSS the path start:
                     only the mark makes the break the oracle reports
  text_ends          the first 100 bases of every contig behind 50 random bases, the last 100 in front of 50 random bases
  marks_beyond       reads of 17 and 33 bases that end 1, 16 and 17 bases in front of a contig's end: a mark lies inside the loaded window
                     but beyond the read
  whole_contigs      reads that are a whole short contig.  They are 300 - 500 bases, more than the one kernel takes (160): this batch
                     goes to the kernel for sequences of any length, which reads the interleaved text that pack_text_kernel still makes,
                     so the one-kernel route is not asserted for it; every byte is compared all the same"""
import ctypes as C

import numpy as np
import pytest

import kbo_amd
from kbo_amd import synth
from gpu_helpers import PER_BASE_GUARD, Guarded, round16, scratch_guard_bytes, threads
from test_gpu_map_default_line import Expected, _dev, _first_difference, _run, _substitute
from test_gpu_summary import _assert_records, _oracle_summary

pytestmark = pytest.mark.gpu

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
K = 31
N_SHORT = 12
LENGTHS = (1, 3, 15, 16, 17, 31, 149, 150, 160)
SPLITS = (1, 15, 16, 17, 31, 75, 133, 134, 135, 149)
ONE_KERNEL = ["substitutions", "path_start_inside", "text_ends", "marks_beyond"]


def _contigs():
    rng = np.random.default_rng(8_2026)
    short = [synth.genome(int(n), seed=500 + i) for i, n in enumerate(rng.integers(300, 501, N_SHORT))]
    return short + [synth.genome(300_000, seed=931)]


def _cases(contigs):
    """name -> (reads, whether at most a tenth of them may be left to the second pass)"""
    rng = np.random.default_rng(20_27)
    short, long_ = contigs[:N_SHORT], contigs[N_SHORT]
    c = {}
    subs = []
    for g, base in ((short[3], 50), (long_, 123_457)):
        for length in LENGTHS:
            subs += [_substitute(rng, g[base + o:base + o + length].copy(), 0.01) for o in range(16)]
    c["substitutions"] = (subs, True)
    c["path_start_inside"] = ([np.concatenate([a[len(a) - s:], b[:150 - s]]) for ia, a in enumerate(short) for ib, b in enumerate(short) if ia != ib
                               for s in SPLITS], False)
    ends = []
    for g in contigs:
        ends.append(np.concatenate([ACGT[rng.integers(0, 4, 50)], g[:100]]))
        ends.append(np.concatenate([g[-100:], ACGT[rng.integers(0, 4, 50)]]))
    c["text_ends"] = (ends, False)
    c["marks_beyond"] = ([g[len(g) - gap - length:len(g) - gap].copy() for g in contigs for length in (17, 33) for gap in (1, 16, 17)], False)
    c["whole_contigs"] = ([g.copy() for g in short], False)
    return c


@pytest.fixture(scope="module")
def world(oracle):
    contigs = _contigs()
    sbwt, _ = kbo_amd.build(contigs, kbo_amd.BuildOpts(k=K, num_threads=threads()))
    ora = oracle.Index.build([g.tobytes() for g in contigs], k=K)
    sbwt.to_device(-1)
    assert sbwt.depth_table_order() > 0
    return {"sbwt": sbwt, "ora": ora, "oracle": oracle, "cases": _cases(contigs), "expected": {}}


def _expected(world, name):
    if name not in world["expected"]:
        reads, stage5 = world["cases"][name]
        world["expected"][name] = Expected(world["oracle"], world["ora"], reads, stage5)
    return world["expected"][name]


def test_the_cases_are_what_they_are_named_for(world):
    """the oracle's characters: reads across two contigs break at the junction whether or not the contigs are neighbours in the text, and
    the text-end reads are half matched"""
    e = _expected(world, "path_start_inside")
    assert e.n == N_SHORT * (N_SHORT - 1) * len(SPLITS) and bool((e.lens == 150).all())
    chars = e.chars.reshape(e.n, 150)
    for i, s in enumerate(SPLITS * (N_SHORT * (N_SHORT - 1))):
        if K <= s <= 150 - K:  # both sides hold a k-mer of their contig; the k-mers across the junction are in no contig
            assert bool((chars[i] != ord("M")).any()), "read %d (split %d) matches across a path start" % (i, s)
    t = _expected(world, "text_ends")
    assert t.n == 2 * (N_SHORT + 1) and bool((t.chars == ord("M")).any()) and bool((t.chars == ord("-")).any())
    assert _expected(world, "marks_beyond").n == (N_SHORT + 1) * 6
    assert _expected(world, "substitutions").n == 2 * 16 * len(LENGTHS)


@pytest.mark.parametrize("fmt", [False, True], ids=["matches", "relative_to_ref"])
@pytest.mark.parametrize("name", ONE_KERNEL)
def test_every_byte_against_the_oracle(world, name, fmt):
    _expected(world, name)
    _run(world, name, fmt, find=False)


@pytest.mark.parametrize("name", ONE_KERNEL)
def test_find_characters_and_runs(world, name):
    _expected(world, name)
    _run(world, name, False, find=True)


@pytest.mark.parametrize("name", ONE_KERNEL)
def test_ms_bytes_against_the_oracle(world, name):
    """want_ms: the kernel's MS-emitting form (the same compare step), characters and MS bytes"""
    import torch
    L, sbwt, e = kbo_amd.lib(), world["sbwt"], _expected(world, name)
    dev = _dev()
    want_d = np.zeros(e.total, dtype=np.uint8)
    want_d[e.keep] = world["ora"].matches_batch(e.concat[e.keep], e.big_off, 1e-7, n_threads=threads(), want_d=True)[1]
    q = Guarded("d_concat", e.total + 16, PER_BASE_GUARD, dev, data=e.concat)
    off = Guarded("d_offsets", 8 * (e.n + 1), PER_BASE_GUARD, dev, data=e.offsets.view(np.uint8))
    ms = Guarded("d_ms", e.total + 16, PER_BASE_GUARD, dev, seed=1)
    chars = Guarded("d_chars_out", e.total + 16, PER_BASE_GUARD, dev, seed=3)
    wb = int(L.kbo_index_work_bytes(sbwt._h, e.n, e.total, e.max_len))
    work = Guarded("d_work", wb, scratch_guard_bytes(e.n, e.total, K), dev, seed=2)
    s = torch.cuda.current_stream(dev).cuda_stream
    fused = C.c_int(-1)
    L.kbo_set_plan(1, 0, 0)
    kbo_amd.check(L.kbo_map_batch_dev(sbwt._h, q.ptr, off.ptr, e.n, e.total, e.max_len, 1e-7, 0, 1, ms.ptr, chars.ptr, work.ptr, wb, s, C.byref(fused)))
    torch.cuda.synchronize()
    assert fused.value == 1, "%s, want_ms: not the one kernel (fused = %d)" % (name, fused.value)
    _first_difference(chars.host()[:e.total], e.chars, e.keep, e.offsets, name + ", want_ms, characters")
    _first_difference(ms.host()[:e.total], want_d, e.keep, e.offsets, name + ", want_ms, MS bytes")
    for x in (q, off, ms, chars, work):
        x.assert_intact(name + ", want_ms")


@pytest.mark.parametrize("name", ONE_KERNEL)
def test_summaries_against_the_oracle(world, name):
    """kbo_summary_batch_dev: the kernel's summary form (the same compare step), a record per read"""
    import torch
    L, sbwt, e = kbo_amd.lib(), world["sbwt"], _expected(world, name)
    dev = _dev()
    wb = int(L.kbo_summary_work_bytes(sbwt._h, e.n, e.total, e.max_len))
    q = Guarded("concat", round16(e.total) + 16, 4096, dev, data=e.concat)
    off = Guarded("d_offsets", 8 * (e.n + 1), PER_BASE_GUARD, dev, data=e.offsets.view(np.uint8))
    msb = Guarded("ms", round16(e.total) + 16, 65536, dev)
    work = Guarded("work", wb, scratch_guard_bytes(e.n, e.total, K) + round16(e.total) + 4096, dev)
    out = Guarded("summary", 16 * e.n, 65536, dev)
    s = torch.cuda.current_stream(dev).cuda_stream
    fused = C.c_int(-1)
    L.kbo_set_plan(1, 0, 0)
    kbo_amd.check(L.kbo_summary_batch_dev(sbwt._h, q.ptr, off.ptr, e.n, e.total, e.max_len, 1e-7, msb.ptr, out.ptr, work.ptr, wb, s, s, C.byref(fused)))
    torch.cuda.synchronize()
    assert fused.value == 1, "%s, summary: not the one kernel (fused = %d)" % (name, fused.value)
    for x in (q, off, msb, work, out):
        x.assert_intact(name + ", summary")
    _assert_records(out.host().view(np.uint32).reshape(e.n, 4), _oracle_summary(world["ora"], e.concat, e.offsets, 1e-7), e.offsets, name + ", summary")


@pytest.mark.parametrize("fmt", [False, True], ids=["matches", "relative_to_ref"])
def test_whole_short_contigs(world, fmt):
    """300 - 500 bases a read: the kernel for sequences of any length, over the interleaved text this change still makes"""
    import torch
    L, sbwt, e = kbo_amd.lib(), world["sbwt"], _expected(world, "whole_contigs")
    assert e.max_len > 160
    dev = _dev()
    q = Guarded("d_concat", e.total + 16, PER_BASE_GUARD, dev, data=e.concat)
    off = Guarded("d_offsets", 8 * (e.n + 1), PER_BASE_GUARD, dev, data=e.offsets.view(np.uint8))
    ms = Guarded("d_ms", e.total + 16, PER_BASE_GUARD, dev, seed=1)
    chars = Guarded("d_chars_out", e.total + 16, PER_BASE_GUARD, dev, seed=3)
    wb = int(L.kbo_index_work_bytes(sbwt._h, e.n, e.total, e.max_len))
    work = Guarded("d_work", wb, scratch_guard_bytes(e.n, e.total, K), dev, seed=2)
    s = torch.cuda.current_stream(dev).cuda_stream
    L.kbo_set_plan(1, 0, 0)
    kbo_amd.check(L.kbo_map_batch_dev(sbwt._h, q.ptr, off.ptr, e.n, e.total, e.max_len, 1e-7, int(fmt), 0, ms.ptr, chars.ptr, work.ptr, wb, s, None))
    torch.cuda.synchronize()
    _first_difference(chars.host()[:e.total], e.map if fmt else e.chars, e.keep, e.offsets, "whole contigs")
    assert bool((e.chars == ord("M")).all()), "a whole contig matches itself"
    for x in (q, off, ms, chars, work):
        x.assert_intact("whole contigs")
