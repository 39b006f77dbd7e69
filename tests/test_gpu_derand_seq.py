"""kbo_derand_translate_seq_dev (kbo_hip.h): derandomize + translate with a threshold per sequence, at any length, against the oracle.

Expected value of every sequence: oracle.translate_ms_vec(oracle.derandomize_ms_vec(ms_s, k, t_s), k, t_s), and relative_to_ref of
it where a reference is given.  The MS bytes are made by numpy - no index, no walk - so they are arbitrary bytes <= k.

Shapes (one batch holds all of them, shuffled by a fixed seed, with 1- and 2-base sequences in between): 3, 4, C - 1, C, C + 1,
2 C + 1, G - 1, G, G + 1, 2 G + 1, 65 536, 65 537 and one of 300 000 bases (70 000 at k = 255), C = KBO_DERAND_SEQ_CHUNK = 128 and
G = KBO_DERAND_SEQ_GROUP = 8 192: every length at which a chunk or a group begins or ends, and one whose owner loops over 37 groups.
Thresholds: two assignments, adjacent sequences always different - from {2, 3, t_mid, k - 1, k} (minimum 2), and from
{t_mid, k - 1, k}, run with min_threshold = t_mid and again with the loose bound 2.  Buffers sit behind guard bands at exactly
their documented sizes."""
import numpy as np
import pytest

import kbo_amd
from gpu_helpers import ACGT, DERAND_CONTENTS as CONTENTS, PER_BASE_GUARD, Guarded, compare_chars as _compare, derand_content as _content
from oracle import binding as ora

pytestmark = pytest.mark.gpu

C_, G_ = 128, 8192  # KBO_DERAND_SEQ_CHUNK, KBO_DERAND_SEQ_GROUP (tests/test_derand_seq_cpu.py pins them to the header)
KS = [3, 31, 96, 255]


def _lengths(k):
    rng = np.random.default_rng(4000 + k)
    big = 70_000 if k == 255 else 300_000
    lens = [3, 4, C_ - 1, C_, C_ + 1, 2 * C_ + 1, G_ - 1, G_, G_ + 1, 2 * G_ + 1, 65536, 65537, big]
    lens += [1, 2, 1, 2, 2, 1]
    lens = [lens[i] for i in rng.permutation(len(lens))]
    return lens


def _thresholds(k, n, high):
    t_mid = max(2, (k + 1) // 2)
    cand = sorted(set([t_mid, k - 1, k] if high else [2, 3, t_mid, k - 1, k]) - {0, 1} - set(range(k + 1, 300)))
    assert len(cand) >= 2
    return np.array([cand[s % len(cand)] for s in range(n)], dtype=np.int32)


_cache = {}


def _world(k, kind, high):
    """the batch, its thresholds and the oracle's characters (plain and relative to a reference) - made once, never changed"""
    key = (k, kind, high)
    if key not in _cache:
        lens = _lengths(k)
        thr = _thresholds(k, len(lens), high)
        assert all(thr[i] != thr[i + 1] for i in range(len(lens) - 1))
        rng = np.random.default_rng(k * 1000 + CONTENTS.index(kind) * 10 + int(high))
        off = np.zeros(len(lens) + 1, dtype=np.uint64)
        off[1:] = np.cumsum(lens)
        total = int(off[-1])
        ms = np.concatenate([_content(kind, rng, n, k, int(t)) for n, t in zip(lens, thr)])
        ref = ACGT[rng.integers(0, 4, total)]
        plain, rel = np.zeros(total, dtype=np.uint8), np.zeros(total, dtype=np.uint8)
        keep = np.zeros(total, dtype=bool)
        for s, n in enumerate(lens):
            if n < 3:
                continue
            a, b, t = int(off[s]), int(off[s + 1]), int(thr[s])
            ch = ora.translate_ms_vec(ora.derandomize_ms_vec(ms[a:b], k, t), k, t).encode()
            plain[a:b] = np.frombuffer(ch, dtype=np.uint8)
            rel[a:b] = np.frombuffer(ora.relative_to_ref(ref[a:b].tobytes(), ch), dtype=np.uint8)
            keep[a:b] = True
        for v in (ms, ref, plain, rel, keep, off, thr):
            v.setflags(write=False)
        _cache[key] = (lens, off, thr, ms, ref, plain, rel, keep)
    return _cache[key]


class _Call:
    """one call's buffers on the device, every one behind guard bands at exactly its documented size"""

    def __init__(self, k, off, thr, ms, ref, min_thr, seed=0):
        import torch
        self.torch = torch
        dev = torch.device("cuda", 0)
        L = kbo_amd.lib()
        self.k, self.n, self.total, self.min_thr = k, len(thr), int(off[-1]), int(min_thr)
        self.wb = int(L.kbo_derand_seq_work_bytes(self.n, self.total, k, self.min_thr))
        g = PER_BASE_GUARD
        self.ms = Guarded("d_ms", self.total + 16, g, dev, seed=seed + 1, data=ms)
        self.ref = Guarded("d_ref", self.total + 16, g, dev, seed=seed + 2, data=ref) if ref is not None else None
        self.out = Guarded("d_chars_out", self.total + 16, g, dev, seed=seed + 3)
        self.off = Guarded("d_offsets", 8 * (self.n + 1), 4096, dev, seed=seed + 4, data=off.view(np.uint8))
        self.thr = Guarded("d_thresholds", 4 * self.n, 4096, dev, seed=seed + 5, data=thr.view(np.uint8))
        self.work = Guarded("d_work", self.wb, 1 << 20, dev, seed=seed + 6)

    def launch(self, stream=None):
        s = stream if stream is not None else self.torch.cuda.current_stream()
        kbo_amd.check(kbo_amd.lib().kbo_derand_translate_seq_dev(
            self.ms.ptr, self.off.ptr, self.n, self.total, self.k, self.thr.ptr, self.min_thr, self.ref.ptr if self.ref else None,
            self.out.ptr, self.work.ptr, self.wb, s.cuda_stream))

    def result(self):
        self.torch.cuda.synchronize()
        for b in (self.ms, self.ref, self.out, self.off, self.thr, self.work):
            if b is not None:
                b.assert_intact()
        for b in (self.ms, self.ref, self.off, self.thr):  # inputs are not written, d_ms included (the call is not in place)
            assert b is None or not b.changed(), b.name
        return self.out.host()[:self.total]


@pytest.mark.parametrize("kind", CONTENTS)
@pytest.mark.parametrize("k", KS)
def test_every_character_against_the_oracle(k, kind):
    for high in (False, True):
        lens, off, thr, ms, ref, plain, rel, keep = _world(k, kind, high)
        true_min = int(thr.min())
        assert len(set(thr.tolist())) >= 2 and (true_min == 2) == (not high or k == 3)
        for min_thr in sorted({true_min, 2}):  # a loose bound must not change a character
            for with_ref in (False, True):
                c = _Call(k, off, thr, ms, ref if with_ref else None, min_thr)
                c.launch()
                _compare(c.result(), rel if with_ref else plain, keep, off,
                         "k %d %s thresholds %s min_threshold %d%s" % (k, kind, "high" if high else "all", min_thr, " ref" if with_ref else ""))


def test_golden_vector_of_the_reference(golden):
    """derandomize.rs:262-266 (k = 3, t = 2), alone and between two other sequences with other thresholds"""
    g = golden["derandomize_ms_vec"][0]
    k, t = g["k"], g["threshold"]
    v = np.array(g["noisy_ms"], dtype=np.uint8)
    assert ora.derandomize_ms_vec(v, k, t).tolist() == g["expected"]
    exp = np.frombuffer(ora.translate_ms_vec(g["expected"], k, t).encode(), dtype=np.uint8)
    for ms, off, thr, a in ((v, [0, len(v)], [t], 0), (np.concatenate([v[:5], v, v[:7]]), [0, 5, 5 + len(v), 12 + len(v)], [3, t, 3], 5)):
        c = _Call(k, np.array(off, dtype=np.uint64), np.array(thr, dtype=np.int32), ms, None, 2)
        c.launch()
        assert np.array_equal(c.result()[a:a + len(v)], exp)


def test_two_streams_with_disjoint_buffers():
    import torch
    k = 31
    w1, w2 = _world(k, "uniform", False), _world(k, "walk", True)
    calls = [_Call(k, w[1], w[2], w[3], None, int(w[2].min()), seed=10 * i) for i, w in enumerate((w1, w2))]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    for c, s in zip(calls, streams):
        c.launch(s)
    for c, w in zip(calls, (w1, w2)):
        _compare(c.result(), w[5], w[7], w[1], "two streams")


def test_python_wrapper():
    import torch
    from kbo_amd import batch
    k = 31
    lens, off, thr, ms, ref, plain, rel, keep = _world(k, "walk", False)
    dev = torch.device("cuda", 0)
    d_ms, d_ref = torch.from_numpy(ms.copy()).to(dev), torch.from_numpy(ref.copy()).to(dev)
    d_off = torch.from_numpy(off.astype(np.int64)).to(dev)
    d_thr = torch.from_numpy(thr.copy()).to(dev)
    got = batch.derand_translate_seq(d_ms, d_off, k, d_thr)
    assert got.dtype == torch.uint8 and got.numel() == int(off[-1])
    _compare(got.cpu().numpy(), plain, keep, off, "wrapper")
    torch.cuda.synchronize()
    got = batch.derand_translate_seq(d_ms, d_off, k, d_thr, ref=d_ref, stream=torch.cuda.Stream(), min_threshold=2)
    torch.cuda.synchronize()
    _compare(got.cpu().numpy(), rel, keep, off, "wrapper, ref")
