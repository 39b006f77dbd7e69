"""kbo_derand_translate_seq_dev / kbo_derand_seq_work_bytes (kbo_hip.h) on the host: the scratch figure and the argument errors,
which come back before anything is enqueued - the pointers are dummy integers, suitably aligned, that nothing ever follows."""
import os
import re

import kbo_amd

E_EMPTY_QUERY, E_THRESHOLD_LE_1, E_BAD_ARG, E_UNSUPPORTED = -1, -3, -4, -8
CHUNK, GROUP = 128, 8192  # KBO_DERAND_SEQ_CHUNK, KBO_DERAND_SEQ_GROUP (tests/test_gpu_derand_seq.py builds its shapes from them)
MS, OFF, THR, REF, OUT, WORK = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000


def test_tuning_constants_are_the_headers():
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "kbo_hip_tuning.h")).read()
    assert int(re.search(r"#define KBO_DERAND_SEQ_CHUNK (\d+)", hdr).group(1)) == CHUNK
    assert int(re.search(r"#define KBO_DERAND_SEQ_GROUP (\d+)", hdr).group(1)) == GROUP
    assert GROUP % CHUNK == 0


def test_work_bytes_positive_and_monotone():
    wb = kbo_amd.lib().kbo_derand_seq_work_bytes
    assert wb(1, 3, 31, 14) > 0 and wb(1, 0, 3, 2) > 0
    for k, t in ((3, 2), (31, 14), (96, 20), (255, 2), (255, 255)):
        seqs = [wb(n, 1 << 20, k, t) for n in (1, 2, 3, 100, 1023, 1024, 1025, 100_000, 10_000_000)]
        assert seqs == sorted(seqs) and seqs[0] > 0 and seqs[-1] > seqs[0]
        bases = [wb(1000, b, k, t) for b in (3000, 3001, 127_999, 128_000, 128_001, 1 << 20, (1 << 20) + 1, 1 << 30, (1 << 32) - 16)]
        assert bases == sorted(bases) and bases[-1] > bases[0]
    for k in (31, 255):
        states = [wb(1000, 1 << 24, k, t) for t in range(k, 1, -1)]  # k - min_threshold = 0, 1, ...
        assert states == sorted(states) and len(set(states)) == len(states)
    assert wb(1000, 1 << 24, 31, 14) % 16 == 0
    # the figure the header gives: about total * (k - t + 6) / 32 + n_seqs * (8 (k - t) + 64) bytes
    n, total, k, t = 1000, 1 << 24, 31, 14
    assert abs(wb(n, total, k, t) - (total * (k - t + 6) // 32 + n * (8 * (k - t) + 64))) < 0.02 * wb(n, total, k, t)


def test_argument_errors_need_no_device():
    L = kbo_amd.lib()
    n, total, k, t = 4, 1000, 31, 14
    wb = int(L.kbo_derand_seq_work_bytes(n, total, k, t))

    def call(ms=MS, off=OFF, n_seqs=n, total_bases=total, k=k, thr=THR, min_thr=t, ref=REF, out=OUT, work=WORK, work_bytes=wb):
        return L.kbo_derand_translate_seq_dev(ms, off, n_seqs, total_bases, k, thr, min_thr, ref, out, work, work_bytes, None)
    for null in ("ms", "off", "thr", "out", "work"):
        assert call(**{null: None}) == E_BAD_ARG, null
    for bad_k in (0, 256, 1000):
        assert call(k=bad_k, min_thr=2) == E_BAD_ARG
    assert call(min_thr=k + 1) == E_BAD_ARG
    assert call(work_bytes=wb - 1) == E_BAD_ARG and call(work_bytes=0) == E_BAD_ARG
    assert call(min_thr=2) == E_BAD_ARG, "a lower bound needs more scratch than a higher one's figure"
    for name, base, step in (("ms", MS, 2), ("ref", REF, 1), ("out", OUT, 3), ("work", WORK, 4), ("work", WORK, 8)):
        assert call(**{name: base + step}) == E_BAD_ARG, name
    assert call(out=MS) == E_BAD_ARG, "in place"
    assert call(n_seqs=0) == E_EMPTY_QUERY
    for low in (0, 1):
        assert call(min_thr=low, work_bytes=1 << 40) == E_THRESHOLD_LE_1
    big = (1 << 32) - 15
    assert call(total_bases=big, work_bytes=1 << 60) == E_UNSUPPORTED
    assert call(total_bases=1 << 40, work_bytes=1 << 60) == E_UNSUPPORTED
