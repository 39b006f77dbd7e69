#!/usr/bin/env python3
"""Placement at tools/bench_locate.py's shape: a 5 Mbp source, 1 M x 150 bp reads with 1 % substitutions, k = 31, bridge = k, inputs
resident; then the same bases as 10 kbp reads at bridge 0, where the wave route carries the load.  One session times, as medians of
REPS (3) runs behind a warm-up:
  walk_segments        kbo_ms_batch_dev with intervals + kbo_segments_dev (the floor: what the parent commit runs)
  walk_segments_place  ... plus kbo_place_dev on the same stream
  place_alone          the place launches alone, over the segments the run before left
and prints one JSON line a shape with them, the segment count, the sequences of either route and a CRC of the records, which must be
the host form's (kbo_place_from_segments_host over the downloaded segments).  GENOME, READS, K, LONG_LEN in the environment change
the shapes."""
import json
import os
import statistics
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("GPU_MAX_HW_QUEUES", "4")

import torch  # noqa: E402

import kbo_amd  # noqa: E402
from kbo_amd import locate, synth  # noqa: E402


def shape(sbwt, g, n, length, k, bridge, reps, name):
    L = kbo_amd.lib()
    dev = torch.device("cuda", 0)
    concat, offsets = synth.reads(g, n, length, 0.01)
    total = int(offsets[-1])
    q = torch.zeros(total + 64, dtype=torch.uint8, device=dev)
    q[:total] = torch.from_numpy(concat).to(dev)
    off = torch.from_numpy(offsets.astype(np.int64)).to(dev)
    ms = torch.zeros(total + 64, dtype=torch.uint8, device=dev)
    lo = torch.zeros(total, dtype=torch.int32, device=dev)
    hi = torch.zeros(total, dtype=torch.int32, device=dev)
    wb = int(L.kbo_ms_work_bytes(n, total, length, k))
    work = torch.zeros(wb // 8 + 2, dtype=torch.int64, device=dev)
    sb = locate.segments_work_bytes(n, total)
    swork = torch.zeros(sb // 8 + 2, dtype=torch.int64, device=dev)
    cap = max(4 * n, total // 40)
    segs = torch.zeros(cap * 7, dtype=torch.int32, device=dev)
    cnt = torch.zeros(1, dtype=torch.int64, device=dev)
    pb = locate.place_work_bytes(n, cap)
    pwork = torch.zeros(pb // 8 + 2, dtype=torch.int64, device=dev)
    place = torch.zeros(n * 12, dtype=torch.int32, device=dev)
    s = torch.cuda.current_stream(dev)

    def walk_seg():
        kbo_amd.check(L.kbo_ms_batch_dev(sbwt._h, q.data_ptr(), off.data_ptr(), n, total, length, ms.data_ptr(), lo.data_ptr(), hi.data_ptr(),
                                         work.data_ptr(), wb, s.cuda_stream))
        locate.segments_dev(sbwt, ms, lo, off, n, total, segs, cap, cnt, swork, sb, bridge=bridge, strand=1, stream=s)

    def do_place():
        locate.place_dev(sbwt, segs, cnt, cap, n, place, pwork, pb, stream=s)

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

    res = {"shape": name, "reads": n, "length": length, "k": k, "bridge": bridge, "reps": reps}
    res["walk_segments_s"] = timed(walk_seg)
    res["walk_segments_place_s"] = timed(lambda: (walk_seg(), do_place()))
    res["place_alone_s"] = timed(do_place)
    torch.cuda.synchronize()
    n_segs = int(cnt.cpu().numpy()[0])
    assert n_segs <= cap, "the segments did not fit: raise cap"
    recs = place.cpu().numpy().view(locate.PLACE_DTYPE)
    host_segs = segs[:n_segs * 7].cpu().numpy().view(locate.SEGMENT_DTYPE)
    per_seq = np.bincount(host_segs["seq"], minlength=n)
    host = locate.place_from_segments_host(host_segs, n, sbwt.source_offsets(), k)
    res["n_segments"] = n_segs
    res["seqs_lane_route"] = int(((per_seq > 0) & (per_seq <= locate.PLACE_LANE_MAX)).sum())
    res["seqs_wave_route"] = int((per_seq > locate.PLACE_LANE_MAX).sum())
    res["seqs_placed"] = int((recs["source"] != locate.PLACE_NONE).sum())
    res["records_crc32"] = zlib.crc32(recs.tobytes())
    res["host_crc32"] = zlib.crc32(host.tobytes())
    res["equal_to_host"] = bool(res["records_crc32"] == res["host_crc32"])
    res["gbp_per_s_walk_segments_place"] = total / res["walk_segments_place_s"] / 1e9
    print(json.dumps(res), flush=True)
    return res


def main():
    G, R, k, reps = int(os.environ.get("GENOME", 5_000_000)), int(os.environ.get("READS", 1_000_000)), int(os.environ.get("K", 31)), \
        int(os.environ.get("REPS", 3))
    long_len = int(os.environ.get("LONG_LEN", 10_000))
    g = synth.genome(G)
    sbwt, _ = kbo_amd.build([g], kbo_amd.BuildOpts(k=k, num_threads=16))
    sbwt.to_device()
    kbo_amd.add_positions(sbwt, [g])
    a = shape(sbwt, g, R, 150, k, k, reps, "reads")
    b = shape(sbwt, g, max(1, R * 150 // long_len), long_len, k, 0, reps, "long")
    assert a["equal_to_host"] and b["equal_to_host"], "the device's records differ from the host form's"


if __name__ == "__main__":
    main()
