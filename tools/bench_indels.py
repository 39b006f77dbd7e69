#!/usr/bin/env python3
"""Indels at tools/bench_pileup.py's shape: a 5 Mbp source, 1 M x 150 bp reads with 1 % substitutions and 0.2 % insertions and
deletions of 1 - 5 bases, k = 31, bridge = k, inputs resident; then the same bases as 10 kbp reads.  One session times, as medians of
REPS (3) runs behind a warm-up:
  chain                 kbo_ms_batch_dev with intervals + kbo_segments_dev with delta + kbo_pileup_dev + kbo_depth_finish_dev +
                        kbo_pileup_sites_dev (what the parent commit runs)
  chain_indels          ... plus kbo_indels_dev behind the pileup and kbo_indel_sites_dev behind the pileup's sites, on the same stream
  indels_alone, indel_sites_alone   each of the two alone, over what the run before left
  download_host         the only way without them: the records and the batch downloaded, kbo_indels_from_segments_host and
                        kbo_indel_sites_host over them (the depth downloaded too)
and prints one JSON line a shape with them, EVENT_CAPACITY (the sort's size), the events, the sites and a CRC of the sites, which must
be the host form's.  GENOME, READS, K, LONG_LEN, EVENT_CAPACITY in the environment change the shapes."""
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

# the reads' indels are independent, so no place has a true variant: one read and a sixty-fourth of the depth make nearly every event
# a site to write and to compare (min_count 3 and one half would give about none)
MIN_COUNT, FRAC_DEN, MAX_INDEL = 1, 64, 16
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def reads_with_indels(g, n, length, sub, indel, seed=1, chunk=1 << 16):
    """n reads of `length` bases off g: a column starts a deletion or an insertion of 1 - 5 bases with probability `indel`, then every
    base is substituted with probability `sub`; -> (concat, offsets)"""
    rng = np.random.default_rng(seed)
    out = np.empty(n * length, dtype=np.uint8)
    for a in range(0, n, chunk):
        m = min(chunk, n - a)
        start = rng.integers(0, len(g) - length - 6 * (2 + int(length * indel * 4)), m)
        adv = np.ones((m, length), dtype=np.int32)  # source bases a column takes
        ins = np.zeros((m, length), dtype=bool)
        ev = rng.random((m, length)) < indel
        ev[:, 0] = False
        kind = rng.random((m, length)) < 0.5
        ln = rng.integers(1, 6, (m, length))
        adv[ev & kind] += ln[ev & kind]  # a deletion in front of the column
        r, c = np.nonzero(ev & ~kind)
        for j in range(5):  # an insertion: its columns take no source base
            keep = (ln[r, c] > j) & (c + j < length)
            ins[r[keep], c[keep] + j] = True
        adv[ins] = 0
        idx = start[:, None] + np.cumsum(adv, axis=1) - 1
        q = g[np.minimum(idx, len(g) - 1)]
        q[ins] = ACGT[rng.integers(0, 4, int(ins.sum()))]
        hit = rng.random((m, length)) < sub
        q[hit] = ACGT[(np.searchsorted(ACGT, q[hit]) + rng.integers(1, 4, int(hit.sum()))) % 4]
        out[a * length:(a + m) * length] = q.ravel()
    return out, np.arange(n + 1, dtype=np.uint64) * np.uint64(length)


def shape(sbwt, g, n, length, k, bridge, reps, name, event_cap):
    L = kbo_amd.lib()
    dev = torch.device("cuda", 0)
    concat, offsets = reads_with_indels(g, n, length, 0.01, 0.002)
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
    eb, ib = locate.indels_work_bytes(cap), locate.indel_sites_work_bytes(event_cap)
    ework = torch.zeros(eb // 8 + 2, dtype=torch.int64, device=dev)
    iwork = torch.zeros(ib // 8 + 2, dtype=torch.int64, device=dev)
    events = torch.zeros(event_cap * 4, dtype=torch.int32, device=dev)
    n_events = torch.zeros(1, dtype=torch.int64, device=dev)
    isites = torch.zeros(event_cap * 8, dtype=torch.int32, device=dev)
    n_isites = torch.zeros(1, dtype=torch.int64, device=dev)
    s = torch.cuda.current_stream(dev)
    soff = sbwt.source_offsets()

    def walk_seg():
        kbo_amd.check(L.kbo_ms_batch_dev(sbwt._h, q.data_ptr(), off.data_ptr(), n, total, length, ms.data_ptr(), lo.data_ptr(), hi.data_ptr(),
                                         work.data_ptr(), wb, s.cuda_stream))
        locate.segments_dev(sbwt, ms, lo, off, n, total, segs, cap, cnt, swork, sb, bridge=bridge, strand=1, delta=delta, stream=s)

    def do_pile():
        locate.pileup_dev(sbwt, q, ms, off, n, total, segs, cnt, cap, pile, skip_multi=True, stream=s)

    def do_events():
        n_events.zero_()
        locate.indels_dev(sbwt, q, off, n, total, segs, cnt, cap, events, event_cap, n_events, ework, eb, skip_multi=True, max_indel=MAX_INDEL, stream=s)

    def do_depth_sites():
        locate.depth_finish_dev(sbwt, delta, depth, dwork, db, stream=s)
        locate.pileup_sites_dev(sbwt, pile, depth, sites, site_cap, n_sites, twork, tb, min_count=2, frac_num=1, frac_den=16, stream=s)

    def do_isites():
        locate.indel_sites_dev(sbwt, events, n_events, event_cap, depth, isites, event_cap, n_isites, iwork, ib, min_count=MIN_COUNT, frac_num=1,
                               frac_den=FRAC_DEN, stream=s)

    def host_way():
        n_segs = int(cnt.cpu().numpy()[0])
        recs = segs[:n_segs * 7].cpu().numpy().view(locate.SEGMENT_DTYPE)
        batch, d = q[:total].cpu().numpy(), depth.cpu().numpy().view(np.uint32)
        ev, ne, cx = locate.indels_from_segments_host(recs, batch, offsets, k, soff, skip_multi=True, max_indel=MAX_INDEL, capacity=event_cap)
        st, ns = locate.indel_sites_host(ev, ne, d, soff, min_count=MIN_COUNT, frac_num=1, frac_den=FRAC_DEN)
        return ev, ne, cx, st, ns

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

    def timed_host(f):
        out = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            out.append(time.perf_counter() - t0)
        return statistics.median(out)

    res = {"shape": name, "reads": n, "length": length, "k": k, "bridge": bridge, "reps": reps, "source_bases": bases, "event_capacity": event_cap,
           "max_indel": MAX_INDEL}
    res["chain_s"] = timed(lambda: (walk_seg(), do_pile(), do_depth_sites()))
    res["chain_indels_s"] = timed(lambda: (walk_seg(), do_pile(), do_events(), do_depth_sites(), do_isites()))
    res["indels_alone_s"] = timed(do_events)
    res["indel_sites_alone_s"] = timed(do_isites)
    # one run from zeroed accumulators, checked against the host form, which is timed with its downloads
    delta.zero_()
    pile.zero_()
    walk_seg(), do_pile(), do_events(), do_depth_sites(), do_isites()
    torch.cuda.synchronize()
    res["download_host_s"] = timed_host(host_way)
    ev, ne, cx, host, hn = host_way()
    n_segs, n_ev, ns = int(cnt.cpu().numpy()[0]), int(n_events.cpu().numpy()[0]), int(n_isites.cpu().numpy()[0])
    assert n_segs <= cap and n_ev <= event_cap, "the segments or the events did not fit: raise cap or EVENT_CAPACITY"
    got = isites[:ns * 8].cpu().numpy().view(locate.INDEL_SITE_DTYPE)
    res["n_segments"] = n_segs
    res["n_events"] = n_ev
    res["n_complex_host"] = cx
    res["n_sites"] = ns
    res["sites_crc32"] = zlib.crc32(got.tobytes())
    res["host_crc32"] = zlib.crc32(host.tobytes())
    res["equal_to_host"] = bool(hn == ns and ne == n_ev and res["sites_crc32"] == res["host_crc32"] and
                                events[:n_ev * 4].cpu().numpy().tobytes() == ev[:ne].tobytes())
    res["device_vs_download_host"] = res["download_host_s"] / (res["indels_alone_s"] + res["indel_sites_alone_s"])
    print(json.dumps(res), flush=True)
    return res


def main():
    G, R, k, reps = int(os.environ.get("GENOME", 5_000_000)), int(os.environ.get("READS", 1_000_000)), int(os.environ.get("K", 31)), \
        int(os.environ.get("REPS", 3))
    long_len, event_cap = int(os.environ.get("LONG_LEN", 10_000)), int(os.environ.get("EVENT_CAPACITY", 1 << 18))
    g = synth.genome(G)
    sbwt, _ = kbo_amd.build([g], kbo_amd.BuildOpts(k=k, num_threads=16))
    sbwt.to_device()
    kbo_amd.add_positions(sbwt, [g])
    a = shape(sbwt, g, R, 150, k, k, reps, "reads", event_cap)
    b = shape(sbwt, g, max(1, R * 150 // long_len), long_len, k, k, reps, "long", event_cap)
    assert a["equal_to_host"] and b["equal_to_host"], "the device's events or sites differ from the host form's"


if __name__ == "__main__":
    main()
