#!/usr/bin/env python3
"""Characters against per-sequence summaries (kbo_aln_summary) on the C2 workload - 5 Mbp index, 1 M reads of 150 bases, 1 %
substitutions: device-resident batches through kbo_map_stream_* with two pipelines and one batch at a time (kbo_map_batch_dev /
kbo_summary_batch_dev), then host to host, bytes and packed (beside tools/bench_host.py's figures).  Prints one JSON line; every
rate is bases over wall time around a device synchronise.  Not the bench.py metric.
LEGS (environment, comma-separated, default all): two_pipelines_chars, two_pipelines_summary, one_at_a_time_chars,
one_at_a_time_summary, host - one leg alone is what a kernel trace is taken of (rocprofv3 --kernel-trace --stats -- python
tools/bench_summary.py: a process's statistics do not tell the legs apart).  The hardware queues are the environment's
(GPU_MAX_HW_QUEUES, HIP's default 4): two pipelines are four streams, and the line says how many queues they had."""
import os
import json
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import kbo_amd  # noqa: E402
from kbo_amd import batch, synth  # noqa: E402

import torch  # noqa: E402

G, R = int(os.environ.get("G", 5_000_000)), int(os.environ.get("R", 1_000_000))
STEPS, REPS = int(os.environ.get("STEPS", 100)), int(os.environ.get("REPS", 3))
HOST_R = int(os.environ.get("HOST_R", 4_000_000))
HAVE = hasattr(batch, "summary_batch")  # (a library without the summaries - the commit before them - times the character legs only)
assert torch.cuda.is_available(), "bench_summary.py needs a GPU"
dv = torch.device("cuda:0")
g = synth.genome(G)
sbwt, _ = kbo_amd.build([g], kbo_amd.BuildOpts(k=31, num_threads=16))
sbwt.to_device()
concat, offsets = synth.reads(g, R, 150, 0.01)
N_BATCH = 4
devs = [batch.DeviceBatch(sbwt, concat, offsets, device=dv, format=False, want_ms=False) for _ in range(N_BATCH)]
LEGS = [x for x in os.environ.get("LEGS", "").split(",") if x]
res = {"bench": "summary", "genome": G, "reads": R, "steps": STEPS, "have_summary": HAVE,
       "hw_queues": os.environ.get("GPU_MAX_HW_QUEUES", "unset (HIP's default: 4)")}


def wanted(name):
    return not LEGS or name in LEGS


def timed(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn(steps)
    torch.cuda.synchronize()
    return steps * len(concat) / (time.perf_counter() - t0) / 1e9  # Gbp/s


def stream_leg(summary):
    ms = batch.MapStream(sbwt, devs[0].n_seqs, devs[0].total, devs[0].max_len, pipelines=2)

    def run(steps):
        for i in range(steps):
            d = devs[i % N_BATCH]
            (ms.submit_summary if summary else ms.submit)(d)
        ms.sync()
    try:
        run(8)
        return [round(timed(run, STEPS), 1) for _ in range(REPS)]
    finally:
        ms.close()


def single_leg(summary):
    def run(steps):
        for i in range(steps):
            d = devs[i % N_BATCH]
            d.run_summary() if summary else d.run()
    run(8)
    return [round(timed(run, STEPS), 1) for _ in range(REPS)]


for rep_name, leg in (("two_pipelines", stream_leg), ("one_at_a_time", single_leg)):
    if wanted(rep_name + "_chars"):
        res[rep_name + "_chars_gbps"] = leg(False)
    if HAVE and wanted(rep_name + "_summary"):
        res[rep_name + "_summary_gbps"] = leg(True)
if not wanted("host"):
    print(json.dumps(res))
    sys.exit(0)

# host to host
hc, ho = synth.reads(g, HOST_R, 150, 0.01)
words, epos, ebyt = batch.pack_reads(hc, ho)


def host_leg(fn):
    fn()
    out = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        fn()
        out.append(round(len(hc) / (time.perf_counter() - t0) / 1e9, 1))
    return out


res["host_bytes_chars_gbps"] = host_leg(lambda: batch.matches_batch(sbwt, hc, ho))
res["host_packed_chars_gbps"] = host_leg(lambda: batch.matches_batch_packed(sbwt, words, ho, epos, ebyt))
if HAVE:
    L = kbo_amd.lib()
    out = np.zeros((HOST_R, 4), dtype=np.uint32)
    res["host_bytes_summary_gbps"] = host_leg(lambda: kbo_amd.check(L.kbo_summary_batch(sbwt._h, hc.ctypes.data, ho.ctypes.data, HOST_R, 1e-7, out.ctypes.data)))
    res["host_packed_summary_gbps"] = host_leg(lambda: kbo_amd.check(L.kbo_summary_batch_packed(
        sbwt._h, words.ctypes.data, ho.ctypes.data, HOST_R, epos.ctypes.data if len(epos) else None, ebyt.ctypes.data if len(ebyt) else None,
        len(epos), 1e-7, out.ctypes.data)))
print(json.dumps(res))
