"""kbo_derand_translate_dev (kbo_hip.h) and the host batches' router behind it (kbo_hip_tuning.h kbo_derand_translate_host): derandomize +
translate with ONE threshold per call, every character of every route of derand_kernels.hip against the oracle, on MS bytes made by
numpy - no index, no walk - so arbitrary bytes <= k.

Expected value of every sequence of 3 bases or more: oracle.translate_ms_vec(oracle.derandomize_ms_vec(ms_s, k, t), k, t), and
oracle.relative_to_ref of it where a reference is given; sequences of 0, 1 and 2 bases lie in between and their bytes are unspecified.
k = 3, 31, 96, 255; one call per threshold of {2, 3, ceil(k / 2), k - 1, k}.  Contents (gpu_helpers.derand_content): the seven kinds of
tests/test_gpu_derand_seq.py - k_last / k_first with the period of the route's granule: 16 (a 16-byte block), 132 (a piece), 128 (a
chunk of the dl_* scan) - and sparse_k: single k's 1000 .. 1160 positions apart, the nearest one 1022, 1023 (inside) or 1024, 1025
(outside the reach) positions above a piece's end.  tests/test_derand_arbitrary_cpu.py shows with a numpy model of the piece rule that
sparse_k and below hold redone and finished sequences in one batch, and walk none.

Which case reaches which route of launch_derand_translate:
  test_lds_route         derand_translate_lds_kernel: max_seq_len = 3, 31, 150, 479 the flat image, 32, 256, 480 the skewed one; 2 (479,
                         480), 3 (256) and 4 waves a workgroup; 391 sequences = 7 waves, the last of 7 sequences, the last workgroup
                         never full (the 327 sequences of 6 waves would fill it at 2 and 3 waves); sequences 128 .. 191 all of the
                         maximal length - the largest span the image holds
  test_piece_route       d_work given: derand_translate_piece_lds_kernel + the redo launch (derand_translate_kernel over the flagged
                         sequences: sparse_k, below, anchors and, beyond 1156 bases, every content without a k), max_seq_len = 0 and exact;
                         d_work NULL, and work_bytes one byte short: derand_translate_kernel, one lane per sequence (dt_step_mid in the
                         interior blocks, dt_step in the first and the topmost one); orders: tiny sequences first (the first wave
                         stages nothing below its span and the first real sequence starts at byte 6.  The kernel's byte-by-byte copy-out
                         needs a wave whose first piece starts at byte 1 .. 15, that is 64 pieces inside 15 bytes: no batch whose
                         offsets start at 0 has one), the longest first, the longest last (the look-ahead capped by total_bases)
  test_two_streams       the piece route, two calls with disjoint buffers
  test_host_router       derand_translate_host_offsets as the slab pipeline calls it: reads alone -> the LDS kernel; a mixed batch ->
                         pieces up to 65 536 bases (longer sequences skipped) and dl_* - dl_emit_kernel's characters - for 65 537 and
                         81 921 bases (4 and 5 groups of 16 384 positions and one position more)
Every device buffer sits behind guard bands at exactly its documented size (d_ms, d_ref, d_chars_out: total_bases + 16 bytes; d_work:
kbo_derand_work_bytes()), inputs are asserted unchanged, and every call runs twice with differently patterned scratch and output."""
import numpy as np
import pytest

import kbo_amd
import gpu_helpers as gh
from gpu_helpers import PER_BASE_GUARD, Guarded, compare_chars
from oracle import binding as ora

pytestmark = pytest.mark.gpu

KS = [3, 31, 96, 255]
CONTENTS = gh.DERAND_CONTENTS + ["sparse_k"]
LONG_SEQ, DL_GROUP = 65536, 16384  # kLongSeq; kDlChunk * kDlGroup (derand_kernels.hip)


class _Call:
    """one kbo_derand_translate_dev call's buffers on the device, every one behind guard bands at exactly its documented size.
    work: "full" = kbo_derand_work_bytes(), "short" = the same buffer declared one byte short, None = no d_work"""

    def __init__(self, k, t, off, ms, ref, max_len, work, seed=0):
        import torch
        self.torch = torch
        dev = torch.device("cuda", 0)
        self.k, self.t, self.n, self.total, self.max_len = k, t, len(off) - 1, int(off[-1]), max_len
        wb = int(kbo_amd.lib().kbo_derand_work_bytes(self.n, self.total))
        self.ms = Guarded("d_ms", self.total + 16, PER_BASE_GUARD, dev, seed=seed + 1, data=ms)
        self.ref = Guarded("d_ref", self.total + 16, PER_BASE_GUARD, dev, seed=seed + 2, data=ref) if ref is not None else None
        self.out = Guarded("d_chars_out", self.total + 16, PER_BASE_GUARD, dev, seed=seed + 3)
        self.off = Guarded("d_offsets", 8 * (self.n + 1), 4096, dev, seed=seed + 4, data=off.view(np.uint8))
        self.work = Guarded("d_work", wb, 1 << 20, dev, seed=seed + 6) if work else None
        self.work_bytes = wb - (work == "short") if work else 0
        self.lane_route = work != "full" and not 0 < max_len <= 480

    def launch(self, stream=None):
        s = stream if stream is not None else self.torch.cuda.current_stream()
        kbo_amd.check(kbo_amd.lib().kbo_derand_translate_dev(
            self.ms.ptr, self.off.ptr, self.n, self.total, self.k, self.t, self.ref.ptr if self.ref else None, self.out.ptr, self.max_len,
            self.work.ptr if self.work else None, self.work_bytes, s.cuda_stream))

    def result(self):
        self.torch.cuda.synchronize()
        for b in (self.ms, self.ref, self.out, self.off, self.work):
            if b is not None:
                b.assert_intact()
        for b in (self.ms, self.ref, self.off):  # inputs are not written
            assert b is None or not b.changed(), b.name
        if self.work is not None and self.lane_route:  # a d_work that is too small is not touched
            assert not self.work.changed(), "d_work"
        return self.out.host()[:self.total]

    def refill(self):
        """scratch and output with another pattern"""
        for b in (self.out, self.work):
            if b is not None:
                b.fill(77)


def _twice(c, exp, keep, off, what):
    c.launch()
    first = c.result()
    compare_chars(first, exp, keep, off, what)
    c.refill()
    c.launch()
    second = c.result()
    compare_chars(second, exp, keep, off, what + " (second run, other scratch pattern)")
    assert np.array_equal(first[keep], second[keep])


@pytest.mark.parametrize("kind", CONTENTS)
@pytest.mark.parametrize("k", KS)
def test_lds_route(k, kind):
    for ti, t in enumerate(gh.derand_thresholds(k)):
        for mi, mx in enumerate(gh.LDS_MAX_LENS):
            variant = (ti + mi) % 2  # every maximal length and every threshold with both (first / last sequence, total mod 16)
            lens = gh.lds_lengths(mx, variant, 1000 * mx + variant)
            off, ms, ref, plain, rel, keep = gh.derand_world(ora, lens, k, t, kind, 16, k * 1000 + CONTENTS.index(kind) * 10 + mi)
            for with_ref in (False, True):
                c = _Call(k, t, off, ms, ref if with_ref else None, mx, None)
                _twice(c, rel if with_ref else plain, keep, off,
                       "LDS route, k %d t %d %s max_seq_len %d variant %d%s" % (k, t, kind, mx, variant, " ref" if with_ref else ""))


# (d_work, max_seq_len exact, reference) of the four calls over one batch: every route with and without d_ref, every order with both
_PIECE_CALLS = ((("full", False, False), ("full", True, True), (None, False, True), ("short", True, False)),
                (("full", False, True), ("full", True, False), (None, True, False), ("short", False, True)))


def _piece_world(k, t, kind, order, period):
    return gh.derand_world(ora, gh.piece_lengths(order, 100 + order), k, t, kind, period, k * 1000 + CONTENTS.index(kind) * 10 + order)


@pytest.mark.parametrize("kind", CONTENTS)
@pytest.mark.parametrize("k", KS)
def test_piece_route(k, kind):
    for ti, t in enumerate(gh.derand_thresholds(k)):
        for order in (0, 1, 2):
            worlds = {}
            for work, exact, with_ref in _PIECE_CALLS[(order + ti) % 2]:
                period = gh.DT_PIECE if work == "full" or kind not in ("k_last", "k_first") else 16  # the granule of the route
                if period not in worlds:
                    worlds[period] = _piece_world(k, t, kind, order, period)
                off, ms, ref, plain, rel, keep = worlds[period]
                c = _Call(k, t, off, ms, ref if with_ref else None, 70_000 if exact else 0, work)
                _twice(c, rel if with_ref else plain, keep, off, "%s, k %d t %d %s order %d max_seq_len %s%s" % (
                    {"full": "pieces", "short": "one lane per sequence (d_work one byte short)", None: "one lane per sequence"}[work],
                    k, t, kind, order, "exact" if exact else "0", " ref" if with_ref else ""))


def test_two_streams_with_disjoint_buffers():
    import torch
    k, t = 31, 16
    w1, w2 = _piece_world(k, t, "sparse_k", 0, gh.DT_PIECE), _piece_world(k, t, "uniform", 2, gh.DT_PIECE)
    calls = [_Call(k, t, w[0], w[1], w[2] if i else None, 0, "full", seed=10 * i) for i, w in enumerate((w1, w2))]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    for c, s in zip(calls, streams):
        c.launch(s)
    for i, (c, w) in enumerate(zip(calls, (w1, w2))):
        compare_chars(c.result(), w[4] if i else w[3], w[5], w[0], "two streams, call %d" % i)


def _host_lengths(seed):
    rng = np.random.default_rng(seed)
    lens = [150, 37, 480, 100, 3, 20_000, LONG_SEQ, LONG_SEQ + 1, 5 * DL_GROUP + 1, 1, 2, 2, 1]
    return [lens[i] for i in rng.permutation(len(lens))]


@pytest.mark.parametrize("kind", ["uniform", "below", "anchors", "k_last", "k_first", "sparse_k"])
@pytest.mark.parametrize("k", [3, 31, 255])
def test_host_router(k, kind):
    L = kbo_amd.lib()
    reads = [int(n) for n in np.random.default_rng(k).choice([1, 2, 3, 4, 17, 100, 150, 151, 480], 130)] + [480]
    for ti, t in enumerate(sorted({2, (k + 1) // 2, k})):
        for lens, name in ((_host_lengths(k + ti), "mixed batch"), (reads, "reads")):
            off, ms, ref, plain, rel, keep = gh.derand_world(ora, lens, k, t, kind, 128, k * 1000 + ti)
            for with_ref in (False, True):
                got = np.full(int(off[-1]), 0xEE, dtype=np.uint8)
                kbo_amd.check(L.kbo_derand_translate_host(ms.ctypes.data, off.ctypes.data, len(lens), k, t,
                                                          ref.ctypes.data if with_ref else None, got.ctypes.data))
                compare_chars(got, rel if with_ref else plain, keep, off,
                              "host router, %s, k %d t %d %s%s" % (name, k, t, kind, " ref" if with_ref else ""))
