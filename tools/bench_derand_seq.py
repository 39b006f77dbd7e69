#!/usr/bin/env python3
"""The derandomize / translate stage alone: kbo_derand_translate_seq_dev (a threshold per sequence) against kbo_derand_translate_dev
(one threshold a call) on the same bytes.  16 MiB of walk-like MS bytes - k, with ramps 0, 1, 2, ... behind a mismatch every about
100 bases - as 256 sequences of 64 KiB and as 16 sequences of 1 MiB, k = 31, t = 14.  Timed with device events over CALLS calls
behind WARMUP calls; prints one JSON line per shape with the milliseconds a call and whether the two stages' characters are equal.
The summary form of the stage (kbo_derand_summary_seq_dev: counts, runs and extent per sequence, no characters) is timed in the same
run, next to the composition it replaces - kbo_derand_translate_seq_dev followed by kbo_summary_dev on its output - and its counts are
compared with that composition's.
Usage: tools/bench_derand_seq.py   (environment: CALLS=20 WARMUP=3)"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import kbo_amd  # noqa: E402

import torch  # noqa: E402
assert torch.cuda.is_available(), "this measures the GPU path: no device, no number"

CALLS, WARMUP = int(os.environ.get("CALLS", 20)), int(os.environ.get("WARMUP", 3))
K, T, TOTAL = 31, 14, 16 << 20
L = kbo_amd.lib()
dev = torch.device("cuda", 0)
rng = np.random.default_rng(31)
ms = np.full(TOTAL, K, dtype=np.uint8)
p = 50
while p + K < TOTAL:
    ms[p:p + K] = np.arange(K)
    p += int(rng.integers(K + 1, 170))


def timed(fn):
    for _ in range(WARMUP):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(CALLS):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / CALLS


for n_seqs in (256, 16):
    length = TOTAL // n_seqs
    d_ms = torch.zeros(TOTAL + 16, dtype=torch.uint8, device=dev)
    d_ms[:TOTAL] = torch.from_numpy(ms).to(dev)
    d_off = torch.arange(n_seqs + 1, dtype=torch.int64, device=dev) * length
    d_thr = torch.full((n_seqs,), T, dtype=torch.int32, device=dev)
    out_seq = torch.zeros(TOTAL + 16, dtype=torch.uint8, device=dev)
    out_one = torch.zeros(TOTAL + 16, dtype=torch.uint8, device=dev)
    wb_seq = int(L.kbo_derand_seq_work_bytes(n_seqs, TOTAL, K, T))
    wb_one = int(L.kbo_derand_work_bytes(n_seqs, TOTAL))
    w_seq = torch.zeros(wb_seq // 8 + 2, dtype=torch.int64, device=dev)
    w_one = torch.zeros(wb_one // 8 + 2, dtype=torch.int64, device=dev)
    s = torch.cuda.current_stream().cuda_stream

    def seq():
        kbo_amd.check(L.kbo_derand_translate_seq_dev(d_ms.data_ptr(), d_off.data_ptr(), n_seqs, TOTAL, K, d_thr.data_ptr(), T, None,
                                                     out_seq.data_ptr(), w_seq.data_ptr(), wb_seq, s))

    def one():
        kbo_amd.check(L.kbo_derand_translate_dev(d_ms.data_ptr(), d_off.data_ptr(), n_seqs, TOTAL, K, T, None, out_one.data_ptr(), length,
                                                 w_one.data_ptr(), wb_one, s))
    wb_sum = int(L.kbo_derand_summary_seq_work_bytes(n_seqs, TOTAL, K, T))
    w_sum = torch.zeros(wb_sum // 8 + 2, dtype=torch.int64, device=dev)
    ext = torch.zeros((n_seqs, 6), dtype=torch.int32, device=dev)
    summ = torch.zeros((n_seqs, 4), dtype=torch.int32, device=dev)

    def summary():
        kbo_amd.check(L.kbo_derand_summary_seq_dev(d_ms.data_ptr(), d_off.data_ptr(), n_seqs, TOTAL, K, d_thr.data_ptr(), T, ext.data_ptr(),
                                                   w_sum.data_ptr(), wb_sum, s))

    def composed():
        seq()
        kbo_amd.check(L.kbo_summary_dev(out_seq.data_ptr(), d_off.data_ptr(), n_seqs, length, summ.data_ptr(), s))
    ms_seq, ms_one = timed(seq), timed(one)
    ms_sum, ms_comp = timed(summary), timed(composed)
    print(json.dumps({"n_seqs": n_seqs, "seq_len": length, "k": K, "t": T, "calls": CALLS, "derand_translate_seq_ms": round(ms_seq, 4),
                      "derand_translate_ms": round(ms_one, 4), "seq_scratch_bytes": wb_seq,
                      "derand_summary_seq_ms": round(ms_sum, 4), "derand_translate_seq_then_summary_ms": round(ms_comp, 4),
                      "summary_counts_equal": bool(torch.equal(ext[:, :4], summ)),
                      "equal": bool(torch.equal(out_seq[:TOTAL], out_one[:TOTAL]))}))
