"""kbo_derand_summary_seq_dev (kbo_hip.h): counts, runs and extent per sequence (kbo_aln_extent) with a threshold per sequence, at
any length, against the oracle.

Expected record of every sequence: the fold, in numpy here, of oracle.translate_ms_vec(oracle.derandomize_ms_vec(ms_s, k, t_s), k, t_s)
- the numbers of 'M', 'X' and 'R', the maximal stretches without '-', the first character other than '-' and one past the last.
Nothing comes from the library under test.  The MS bytes are made by numpy - no index, no walk - so they are arbitrary bytes <= k.

Shapes, thresholds and contents are those of tests/test_gpu_derand_seq.py, restated: one batch of 3, 4, C - 1, C, C + 1, 2 C + 1,
G - 1, G, G + 1, 2 G + 1, 65 536, 65 537 and 300 000 bases (70 000 at k = 255) with 1- and 2-base sequences in between, shuffled by a
fixed seed; C = KBO_DERAND_SEQ_CHUNK = 128, G = KBO_DERAND_SEQ_GROUP = 8 192.  Two threshold assignments, adjacent sequences always
different, each run with the true minimum as min_threshold and with the loose bound 2.  Buffers sit behind guard bands at exactly
their documented sizes: d_ms at total + 16, d_out at 24 n_seqs, d_work at kbo_derand_summary_seq_work_bytes()."""
import numpy as np
import pytest

import kbo_amd
from gpu_helpers import DERAND_CONTENTS as CONTENTS, PER_BASE_GUARD, Guarded, compare_chars, derand_content
from oracle import binding as ora

pytestmark = pytest.mark.gpu

C_, G_ = 128, 8192  # KBO_DERAND_SEQ_CHUNK, KBO_DERAND_SEQ_GROUP (tests/test_derand_seq_cpu.py pins them to the header)
KS = [3, 31, 96, 255]
FIELDS = ("n_match", "n_mismatch", "n_jump", "n_runs", "start", "end")


def fold(chars):
    """kbo_aln_extent of one sequence's characters (a uint8 array)"""
    hit = chars != ord("-")
    starts = hit & ~np.concatenate([[False], hit[:-1]])
    at = np.flatnonzero(hit)
    return [int((chars == ord("M")).sum()), int((chars == ord("X")).sum()), int((chars == ord("R")).sum()), int(starts.sum()),
            int(at[0]) if len(at) else 0, int(at[-1]) + 1 if len(at) else 0]


def test_fold_on_strings():
    def f(s):
        return fold(np.frombuffer(s, dtype=np.uint8))
    assert f(b"-----") == [0, 0, 0, 0, 0, 0]
    assert f(b"MMMMM") == [5, 0, 0, 1, 0, 5]
    assert f(b"--MXM--RR-M-") == [3, 1, 2, 3, 2, 11]
    assert f(b"M--") == [1, 0, 0, 1, 0, 1] and f(b"--R") == [0, 0, 1, 1, 2, 3]


def _lengths(k):
    rng = np.random.default_rng(4000 + k)
    big = 70_000 if k == 255 else 300_000
    lens = [3, 4, C_ - 1, C_, C_ + 1, 2 * C_ + 1, G_ - 1, G_, G_ + 1, 2 * G_ + 1, 65536, 65537, big]
    lens += [1, 2, 1, 2, 2, 1]
    return [lens[i] for i in rng.permutation(len(lens))]


def _thresholds(k, n, high):
    t_mid = max(2, (k + 1) // 2)
    cand = sorted(set([t_mid, k - 1, k] if high else [2, 3, t_mid, k - 1, k]) - {0, 1} - set(range(k + 1, 300)))
    assert len(cand) >= 2
    return np.array([cand[s % len(cand)] for s in range(n)], dtype=np.int32)


def _oracle_chars(ms, k, t):
    return np.frombuffer(ora.translate_ms_vec(ora.derandomize_ms_vec(ms, k, t), k, t).encode(), dtype=np.uint8)


_cache = {}


def _world(k, kind, high):
    """the batch, its thresholds, the oracle's characters and their fold - made once, never changed"""
    key = (k, kind, high)
    if key not in _cache:
        lens = _lengths(k)
        thr = _thresholds(k, len(lens), high)
        assert all(thr[i] != thr[i + 1] for i in range(len(lens) - 1))
        rng = np.random.default_rng(k * 1000 + CONTENTS.index(kind) * 10 + int(high))
        off = np.zeros(len(lens) + 1, dtype=np.uint64)
        off[1:] = np.cumsum(lens)
        total = int(off[-1])
        ms = np.concatenate([derand_content(kind, rng, n, k, int(t)) for n, t in zip(lens, thr)])
        plain = np.zeros(total, dtype=np.uint8)
        keep = np.zeros(total, dtype=bool)
        want = np.zeros((len(lens), 6), dtype=np.uint32)
        for s, n in enumerate(lens):
            if n < 3:
                continue  # (no alignment: an all-zero record)
            a, b = int(off[s]), int(off[s + 1])
            plain[a:b] = _oracle_chars(ms[a:b], k, int(thr[s]))
            keep[a:b] = True
            want[s] = fold(plain[a:b])
        for v in (ms, plain, keep, off, thr, want):
            v.setflags(write=False)
        _cache[key] = (lens, off, thr, ms, plain, keep, want)
    return _cache[key]


class _Call:
    """one call's buffers on the device, every one behind guard bands at exactly its documented size"""

    def __init__(self, k, off, thr, ms, min_thr, seed=0):
        import torch
        self.torch = torch
        dev = torch.device("cuda", 0)
        L = kbo_amd.lib()
        self.k, self.n, self.total, self.min_thr = k, len(thr), int(off[-1]), int(min_thr)
        self.wb = int(L.kbo_derand_summary_seq_work_bytes(self.n, self.total, k, self.min_thr))
        self.ms = Guarded("d_ms", self.total + 16, PER_BASE_GUARD, dev, seed=seed + 1, data=ms)
        self.out = Guarded("d_out", 24 * self.n, 4096, dev, seed=seed + 3)  # (filled with a pattern without a zero byte)
        self.off = Guarded("d_offsets", 8 * (self.n + 1), 4096, dev, seed=seed + 4, data=off.view(np.uint8))
        self.thr = Guarded("d_thresholds", 4 * self.n, 4096, dev, seed=seed + 5, data=thr.view(np.uint8))
        self.work = Guarded("d_work", self.wb, 1 << 20, dev, seed=seed + 6)

    def launch(self, stream=None):
        s = stream if stream is not None else self.torch.cuda.current_stream()
        kbo_amd.check(kbo_amd.lib().kbo_derand_summary_seq_dev(self.ms.ptr, self.off.ptr, self.n, self.total, self.k, self.thr.ptr, self.min_thr,
                                                               self.out.ptr, self.work.ptr, self.wb, s.cuda_stream))

    def result(self):
        self.torch.cuda.synchronize()
        for b in (self.ms, self.out, self.off, self.thr, self.work):
            b.assert_intact()
        for b in (self.ms, self.off, self.thr):  # inputs are not written
            assert not b.changed(), b.name
        return self.out.host().view(np.uint32).reshape(self.n, 6)


def _assert_records(got, want, lens, what):
    bad = np.flatnonzero((got != want).any(axis=1))
    if len(bad):
        s = int(bad[0])
        raise AssertionError("%s: %d records differ, first sequence %d (%d bases): got %s, expected %s" % (
            what, len(bad), s, lens[s], dict(zip(FIELDS, got[s].tolist())), dict(zip(FIELDS, want[s].tolist()))))


@pytest.mark.parametrize("kind", CONTENTS)
@pytest.mark.parametrize("k", KS)
def test_every_record_against_the_oracle(k, kind):
    for high in (False, True):
        lens, off, thr, ms, plain, keep, want = _world(k, kind, high)
        true_min = int(thr.min())
        assert len(set(thr.tolist())) >= 2 and (true_min == 2) == (not high or k == 3)
        short = [s for s, n in enumerate(lens) if n < 3]
        assert len(short) == 6 and not want[short].any()
        if kind == "all_k":  # one run over the whole sequence: a run counted twice across chunks, waves or groups shows here
            for s, n in enumerate(lens):  # (t = k: the last position's rule, a > t, does not fire - that one character is a '-')
                m = n - int(thr[s] == k)
                assert n < 3 or want[s].tolist() == [m, 0, 0, 1, 0, m]
            assert (thr < k).sum() >= len(lens) // 2
        if kind == "below":  # nothing fires: zeros (a sequence with t = k draws k itself among its bytes <= t, and k always fires)
            assert not want[thr < k].any() and (thr < k).sum() >= len(lens) // 2
        for min_thr in sorted({true_min, 2}):  # a loose bound must not change a record
            c = _Call(k, off, thr, ms, min_thr)
            c.launch()
            got = c.result()
            _assert_records(got, want, lens, "k %d %s thresholds %s min_threshold %d" % (k, kind, "high" if high else "all", min_thr))
            assert not got[short].any(), "records of 1- and 2-base sequences are written as zeros"


def _hand_made(k, cut_zeros):
    """3 C bases of k with two stretches of two zeros and the ramp 1, 2, ... k a walk leaves behind a mismatch: one stretch at
    `cut_zeros`, one at 2 C - 1 .. 2 C"""
    ms = np.full(3 * C_, k, dtype=np.uint8)
    for z in (cut_zeros, 2 * C_ - 1):
        ms[z:z + 2] = 0
        ms[z + 2:z + 2 + k] = np.arange(1, k + 1)
    return ms


def test_hand_made_runs_at_the_chunk_cuts():
    """A run that ends with the last position of a chunk, a run that starts with the first position of a chunk, and a '-' stretch
    over a chunk cut (2 C - 1 .. 2 C), each verified on the oracle's characters before any GPU call.  The first two cannot meet at
    one cut: a run that ends at C - 1 and one that starts at C would be one run, and a single '-' between two other characters does
    not exist - x[p] <= 0 < x[p + 1] makes x[p + 1] = 1, and then c[p] is 'X' unless x[p - 1] <= 0, which makes c[p - 1] a '-' as
    well.  So there are two sequences of 3 C bases, one per condition, and both carry the stretch over the second cut."""
    k, t = 31, 14
    a, b = _hand_made(k, C_), _hand_made(k, C_ - 2)
    ca, cb = _oracle_chars(a, k, t), _oracle_chars(b, k, t)
    dash = ord("-")
    assert ca[C_ - 1] != dash and ca[C_] == dash                      # a run ends exactly at position C - 1
    assert cb[C_ - 1] == dash and cb[C_] != dash                      # another run starts exactly at C
    for c in (ca, cb):
        assert c[2 * C_ - 1] == dash and c[2 * C_] == dash            # a '-' stretch covers 2 C - 1 .. 2 C
        assert c[2 * C_ - 2] != dash and c[2 * C_ + 1] != dash and fold(c)[3] == 3
    ms = np.concatenate([a, b])
    off = np.array([0, 3 * C_, 6 * C_], dtype=np.uint64)
    thr = np.array([t, t], dtype=np.int32)
    want = np.array([fold(ca), fold(cb)], dtype=np.uint32)
    c = _Call(k, off, thr, ms, t)
    c.launch()
    _assert_records(c.result(), want, [3 * C_, 3 * C_], "hand-made")


def test_two_streams_with_disjoint_buffers():
    import torch
    k = 31
    w1, w2 = _world(k, "uniform", False), _world(k, "walk", True)
    calls = [_Call(k, w[1], w[2], w[3], int(w[2].min()), seed=10 * i) for i, w in enumerate((w1, w2))]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    for c, s in zip(calls, streams):
        c.launch(s)
    for c, w in zip(calls, (w1, w2)):
        _assert_records(c.result(), w[6], w[0], "two streams")


def test_python_wrapper():
    import torch
    from kbo_amd import batch
    k = 31
    lens, off, thr, ms, plain, keep, want = _world(k, "walk", False)
    dev = torch.device("cuda", 0)
    d_ms = torch.from_numpy(ms.copy()).to(dev)
    d_off = torch.from_numpy(off.astype(np.int64)).to(dev)
    d_thr = torch.from_numpy(thr.copy()).to(dev)
    got = batch.derand_summary_seq(d_ms, d_off, k, d_thr)
    assert got.dtype == torch.int32 and tuple(got.shape) == (len(lens), 6)
    torch.cuda.synchronize()
    _assert_records(got.cpu().numpy().view(np.uint32), want, lens, "wrapper")
    got = batch.derand_summary_seq(d_ms, d_off, k, d_thr, stream=torch.cuda.Stream(), min_threshold=2)
    torch.cuda.synchronize()
    _assert_records(got.cpu().numpy().view(np.uint32), want, lens, "wrapper, its own stream")


def test_character_form_unchanged():
    """kbo_derand_translate_seq_dev on the same batch still gives the oracle's characters"""
    import torch
    k = 31
    lens, off, thr, ms, plain, keep, want = _world(k, "uniform", False)
    dev = torch.device("cuda", 0)
    L = kbo_amd.lib()
    n, total, min_thr = len(lens), int(off[-1]), int(thr.min())
    wb = int(L.kbo_derand_seq_work_bytes(n, total, k, min_thr))
    d_ms = Guarded("d_ms", total + 16, PER_BASE_GUARD, dev, seed=1, data=ms)
    d_out = Guarded("d_chars_out", total + 16, PER_BASE_GUARD, dev, seed=2)
    d_off = Guarded("d_offsets", 8 * (n + 1), 4096, dev, seed=3, data=off.view(np.uint8))
    d_thr = Guarded("d_thresholds", 4 * n, 4096, dev, seed=4, data=thr.view(np.uint8))
    d_work = Guarded("d_work", wb, 1 << 20, dev, seed=5)
    kbo_amd.check(L.kbo_derand_translate_seq_dev(d_ms.ptr, d_off.ptr, n, total, k, d_thr.ptr, min_thr, None, d_out.ptr, d_work.ptr, wb,
                                                 torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    for b in (d_ms, d_out, d_off, d_thr, d_work):
        b.assert_intact()
    compare_chars(d_out.host()[:total], plain, keep, off, "character form")
