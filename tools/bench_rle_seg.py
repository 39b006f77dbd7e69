#!/usr/bin/env python3
"""The run-length stage alone: kbo_run_lengths_seq_dev (a chunk per lane) against kbo_run_lengths_dev (one lane per sequence for
everything longer than a read) on the same bytes.  16 MiB of kbo::matches-like characters - 'M' with 1 % 'X' and a stretch of '-'
about every 2 kbp - cut into sequences of 512, 1 Ki, 2 Ki, ... 1 Mi characters.  Timed with device events behind WARMUP calls, over
up to CALLS calls (fewer where a call takes long: about BUDGET_MS of device time a figure); prints one JSON line per length and
max_gap_len with the milliseconds a call and whether the two stages' records are equal.  The smallest of these lengths from which
the new call wins at every longer one is where the library's own callers should start to take it (they do not yet).
Usage: tools/bench_rle_seg.py   (environment: CALLS=20 WARMUP=2 BUDGET_MS=300 GAPS=0,5)"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import kbo_amd  # noqa: E402

import torch  # noqa: E402
assert torch.cuda.is_available(), "this measures the GPU path: no device, no number"

CALLS, WARMUP = int(os.environ.get("CALLS", 20)), int(os.environ.get("WARMUP", 2))
BUDGET_MS = float(os.environ.get("BUDGET_MS", 300))
GAPS = [int(g) for g in os.environ.get("GAPS", "0,5").split(",")]
TOTAL = 16 << 20
L = kbo_amd.lib()
dev = torch.device("cuda", 0)
rng = np.random.default_rng(17)
chars = np.where(rng.random(TOTAL) < 0.01, ord("X"), ord("M")).astype(np.uint8)
p = 700
while p < TOTAL:
    m = int(rng.integers(1, 40))
    chars[p:p + m] = ord("-")
    p += m + int(rng.integers(1000, 3000))
d_chars = torch.zeros(TOTAL + 16, dtype=torch.uint8, device=dev)
d_chars[:TOTAL] = torch.from_numpy(chars).to(dev)


def interval(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def timed(fn):
    for _ in range(WARMUP):
        fn()
    once = interval(fn, 1)
    return interval(fn, max(1, min(CALLS, int(BUDGET_MS / max(once, 1e-3)))))


for length in [512 << i for i in range(12)]:
    n_seqs = TOTAL // length
    d_off = torch.arange(n_seqs + 1, dtype=torch.int64, device=dev) * length
    capacity = n_seqs + TOTAL // 500 + 1024
    rec_seq = torch.zeros((capacity, 7), dtype=torch.int32, device=dev)
    rec_one = torch.zeros((capacity, 7), dtype=torch.int32, device=dev)
    first = torch.zeros(n_seqs + 1, dtype=torch.int32, device=dev)
    wb_seq = int(L.kbo_run_lengths_seq_work_bytes(n_seqs, TOTAL))
    wb_one = int(L.kbo_run_lengths_work_bytes(n_seqs))
    w_seq = torch.zeros(wb_seq // 8 + 2, dtype=torch.int64, device=dev)
    w_one = torch.zeros(wb_one // 4 + 4, dtype=torch.int32, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    for gap in GAPS:
        def seq():
            kbo_amd.check(L.kbo_run_lengths_seq_dev(d_chars.data_ptr(), d_off.data_ptr(), n_seqs, TOTAL, gap, w_seq.data_ptr(), wb_seq,
                                                    rec_seq.data_ptr(), capacity, first.data_ptr(), s))

        def one():
            kbo_amd.check(L.kbo_run_lengths_dev(d_chars.data_ptr(), d_off.data_ptr(), n_seqs, length, gap, w_one.data_ptr(), rec_one.data_ptr(),
                                                capacity, s))
        ms_seq, ms_one = timed(seq), timed(one)
        runs = int(first[-1].item())
        w = w_one.cpu().numpy().view(np.uint32)
        first_one = w[:n_seqs + 1].astype(np.int64) + w[n_seqs + 1 + np.arange(n_seqs + 1) // 1024]
        equal = runs <= capacity and int(first_one[n_seqs]) == runs and bool(torch.equal(rec_seq[:runs], rec_one[:runs])) and \
            np.array_equal(first_one, first.cpu().numpy().astype(np.int64))
        print(json.dumps({"seq_len": length, "n_seqs": n_seqs, "max_gap_len": gap, "runs": runs, "run_lengths_seq_ms": round(ms_seq, 4),
                          "run_lengths_ms": round(ms_one, 4), "speedup": round(ms_one / ms_seq, 2), "seq_scratch_bytes": wb_seq, "equal": equal}),
              flush=True)
