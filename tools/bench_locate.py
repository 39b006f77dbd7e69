#!/usr/bin/env python3
"""Positions, segments, depth at the headline shape: a 5 Mbp source, 1 M x 150 bp reads with 1 % substitutions, k = 31, bridge = k,
inputs resident.  One session times, as medians of REPS (3) runs:
  walk            kbo_ms_batch_dev with intervals alone (the floor)
  walk+segments   ... plus kbo_segments_dev without delta
  walk+seg+delta  ... with delta
  depth_finish    kbo_depth_finish_dev
  add_positions   kbo_index_add_positions (a build step: host work, uploads and a wait included)
and prints one JSON line with them, the segment count and a CRC of the records.  GENOME, READS, K in the environment change the shape."""
import json
import os
import statistics
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("GPU_MAX_HW_QUEUES", "4")

import torch  # noqa: E402

import kbo_amd  # noqa: E402
from kbo_amd import locate, synth  # noqa: E402


def main():
    G, R, k, reps = int(os.environ.get("GENOME", 5_000_000)), int(os.environ.get("READS", 1_000_000)), int(os.environ.get("K", 31)), \
        int(os.environ.get("REPS", 3))
    L = kbo_amd.lib()
    dev = torch.device("cuda", 0)
    g = synth.genome(G)
    sbwt, _ = kbo_amd.build([g], kbo_amd.BuildOpts(k=k, num_threads=16))
    sbwt.to_device()
    t_add = []
    for _ in range(reps):
        t0 = time.perf_counter()
        kbo_amd.add_positions(sbwt, [g])
        t_add.append(time.perf_counter() - t0)
    concat, offsets = synth.reads(g, R, 150, 0.01)
    n, total = R, int(offsets[-1])
    q = torch.zeros(total + 64, dtype=torch.uint8, device=dev)
    q[:total] = torch.from_numpy(concat).to(dev)
    off = torch.from_numpy(offsets.astype(np.int64)).to(dev)
    ms = torch.zeros(total + 64, dtype=torch.uint8, device=dev)
    lo = torch.zeros(total, dtype=torch.int32, device=dev)
    hi = torch.zeros(total, dtype=torch.int32, device=dev)
    wb = int(L.kbo_ms_work_bytes(n, total, 150, k))
    work = torch.zeros(wb // 8 + 2, dtype=torch.int64, device=dev)
    sb = locate.segments_work_bytes(n, total)
    swork = torch.zeros(sb // 8 + 2, dtype=torch.int64, device=dev)
    cap = 4 * n
    segs = torch.zeros(cap * 7, dtype=torch.int32, device=dev)
    cnt = torch.zeros(1, dtype=torch.int64, device=dev)
    delta = torch.zeros(G + 1, dtype=torch.int32, device=dev)
    depth = torch.zeros(G, dtype=torch.int32, device=dev)
    dwb = locate.depth_work_bytes(sbwt)
    dwork = torch.zeros(dwb // 8 + 2, dtype=torch.int64, device=dev)
    s = torch.cuda.current_stream(dev)

    def walk():
        kbo_amd.check(L.kbo_ms_batch_dev(sbwt._h, q.data_ptr(), off.data_ptr(), n, total, 150, ms.data_ptr(), lo.data_ptr(), hi.data_ptr(),
                                         work.data_ptr(), wb, s.cuda_stream))

    def seg(with_delta):
        locate.segments_dev(sbwt, ms, lo, off, n, total, segs, cap, cnt, swork, sb, bridge=k, strand=1, delta=delta if with_delta else None, stream=s)

    def timed(f):
        out = []
        for _ in range(reps + 1):  # (the first run warms up and is dropped)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(s)
            f()
            b.record(s)
            b.synchronize()
            out.append(a.elapsed_time(b) * 1e-3)
        return statistics.median(out[1:])

    res = {"genome": G, "reads": R, "k": k, "bridge": k, "reps": reps}
    res["walk_s"] = timed(walk)
    res["walk_segments_s"] = timed(lambda: (walk(), seg(False)))
    delta.zero_()
    res["walk_segments_delta_s"] = timed(lambda: (walk(), seg(True)))
    res["segments_alone_s"] = timed(lambda: seg(False))
    res["depth_finish_s"] = timed(lambda: locate.depth_finish_dev(sbwt, delta, depth, dwork, dwb, stream=s))
    res["add_positions_s"] = statistics.median(t_add)
    torch.cuda.synchronize()
    n_segs = int(cnt.cpu().numpy()[0])
    res["n_segments"] = n_segs
    res["records_crc32"] = zlib.crc32(segs[:min(n_segs, cap) * 7].cpu().numpy().tobytes())
    res["gbp_per_s_walk"] = total / res["walk_s"] / 1e9
    res["gbp_per_s_walk_segments"] = total / res["walk_segments_s"] / 1e9
    res["positions_bytes"] = int(L.kbo_index_positions_bytes(sbwt._h))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
