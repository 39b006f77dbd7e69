#!/usr/bin/env python3
"""Pileup at tools/bench_locate.py's shape: a 5 Mbp source, 1 M x 150 bp reads with 1 % substitutions, k = 31, bridge = k, inputs
resident; then the same bases as 10 kbp reads.  One session times, as medians of REPS (3) runs behind a warm-up:
  walk_segments         kbo_ms_batch_dev with intervals + kbo_segments_dev with delta (the floor: what the parent commit runs)
  walk_segments_pileup  ... plus kbo_pileup_dev, kbo_depth_finish_dev and kbo_pileup_sites_dev on the same stream
  pileup_alone, depth_finish_alone, sites_alone   each of the three alone, over what the run before left
and prints one JSON line a shape with them, the segments, the bridged bases, the sites and a CRC of the sites, which must be the host
form's (kbo_pileup_from_segments_host and kbo_pileup_sites_host over the downloaded segments and MS bytes).  GENOME, READS, K,
LONG_LEN in the environment change the shapes."""
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

# the reads' substitutions are independent, so no base has a true variant: two reads that agree and a sixteenth of the depth give some
# ten thousand sites to write and to compare (min_count 3 and one half would give about none)
MIN_COUNT, FRAC_DEN = 2, 16


def shape(sbwt, g, n, length, k, bridge, reps, name):
    L = kbo_amd.lib()
    dev = torch.device("cuda", 0)
    concat, offsets = synth.reads(g, n, length, 0.01)
    total, bases = int(offsets[-1]), len(g)
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
    delta = torch.zeros(bases + 1, dtype=torch.int32, device=dev)
    depth = torch.zeros(bases, dtype=torch.int32, device=dev)
    pile = torch.zeros(bases * 4, dtype=torch.int32, device=dev)
    db, tb = locate.depth_work_bytes(sbwt), locate.pileup_sites_work_bytes(sbwt)
    dwork = torch.zeros(db // 8 + 2, dtype=torch.int64, device=dev)
    twork = torch.zeros(tb // 8 + 2, dtype=torch.int64, device=dev)
    site_cap = bases // 16
    sites = torch.zeros(site_cap * 8, dtype=torch.int32, device=dev)
    n_sites = torch.zeros(1, dtype=torch.int64, device=dev)
    s = torch.cuda.current_stream(dev)

    def walk_seg():
        kbo_amd.check(L.kbo_ms_batch_dev(sbwt._h, q.data_ptr(), off.data_ptr(), n, total, length, ms.data_ptr(), lo.data_ptr(), hi.data_ptr(),
                                         work.data_ptr(), wb, s.cuda_stream))
        locate.segments_dev(sbwt, ms, lo, off, n, total, segs, cap, cnt, swork, sb, bridge=bridge, strand=1, delta=delta, stream=s)

    def do_pile():
        locate.pileup_dev(sbwt, q, ms, off, n, total, segs, cnt, cap, pile, skip_multi=True, stream=s)

    def do_depth():
        locate.depth_finish_dev(sbwt, delta, depth, dwork, db, stream=s)

    def do_sites():
        locate.pileup_sites_dev(sbwt, pile, depth, sites, site_cap, n_sites, twork, tb, min_count=MIN_COUNT, frac_num=1, frac_den=FRAC_DEN, stream=s)

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

    res = {"shape": name, "reads": n, "length": length, "k": k, "bridge": bridge, "reps": reps, "source_bases": bases}
    res["walk_segments_s"] = timed(walk_seg)
    res["walk_segments_pileup_s"] = timed(lambda: (walk_seg(), do_pile(), do_depth(), do_sites()))
    res["pileup_alone_s"] = timed(do_pile)
    res["depth_finish_alone_s"] = timed(do_depth)
    res["sites_alone_s"] = timed(do_sites)
    # one run from zeroed accumulators, checked against the host form
    delta.zero_()
    pile.zero_()
    walk_seg(), do_pile(), do_depth(), do_sites()
    torch.cuda.synchronize()
    n_segs, ns = int(cnt.cpu().numpy()[0]), int(n_sites.cpu().numpy()[0])
    assert n_segs <= cap and ns <= site_cap, "the segments or the sites did not fit: raise cap"
    host_segs = segs[:n_segs * 7].cpu().numpy().view(locate.SEGMENT_DTYPE)
    got = sites[:ns * 8].cpu().numpy().view(locate.SITE_DTYPE)
    hp, bridged = locate.pileup_from_segments_host(host_segs, concat, ms[:total].cpu().numpy(), offsets, k, bases, skip_multi=True)
    host, hn = locate.pileup_sites_host(hp, depth.cpu().numpy().view(np.uint32), sbwt.source_offsets(), min_count=MIN_COUNT, frac_num=1, frac_den=FRAC_DEN)
    res["n_segments"] = n_segs
    res["bridged_bases"] = bridged
    res["pile_sum"] = int(pile.cpu().numpy().view(np.uint32).sum(dtype=np.uint64))
    res["n_sites"] = ns
    res["sites_crc32"] = zlib.crc32(got.tobytes())
    res["host_crc32"] = zlib.crc32(host.tobytes())
    res["equal_to_host"] = bool(hn == ns and res["sites_crc32"] == res["host_crc32"] and np.array_equal(pile.cpu().numpy().view(np.uint32).reshape(-1, 4), hp))
    res["gbp_per_s_walk_segments_pileup"] = total / res["walk_segments_pileup_s"] / 1e9
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
    b = shape(sbwt, g, max(1, R * 150 // long_len), long_len, k, k, reps, "long")
    assert a["equal_to_host"] and b["equal_to_host"], "the device's pile or sites differ from the host form's"


if __name__ == "__main__":
    main()
