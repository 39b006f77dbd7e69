#!/usr/bin/env python3
"""kbo::find against a set of references: kbo_refset_build + kbo_refset_to_device and kbo_find_refset, against the only way there was
before - one kbo_index_build + kbo_index_to_device + kbo_find_batch_strands per reference.  Prints one JSON line: seconds of the
set's build + upload, seconds of the find (median of REPEATS calls behind one warm-up call, with their spread), the pair-bases per
second that is, the per-reference seconds of the loop (timed over LOOP references behind two warm-up references, and scaled to all
of them), the ratio, and whether the set's records equal the loop's for the references the loop took.
Workload: REFS random references of REF_BP bases at k = 31 against a query of QUERY_BP bases in CONTIGS contigs, both strands; a
copy of every 40th reference with 1 % substitutions lies in the query, so that there are runs to report.
Usage: tools/bench_refset.py   (environment: REFS=2000 REF_BP=1000 QUERY_BP=5000000 CONTIGS=50 LOOP=50 REPEATS=3; CONTIGS=100 makes
the contigs 50 kbp, below the 65 536 bases at which the single-index stage changes kernels; records_crc32 compares two builds)
SUMMARY=1 times kbo_summary_refset on the same workload instead (one record per pair with a hit; the CRC is of those records) and
checks, for the references the loop takes - or, with LOOP=0, for all of them against one kbo_find_refset(max_gap_len = 0) call that
is not timed - that every pair's n_runs is its number of run records.
DEV=1 adds the device-resident form on the same workload - refset.find_refset_dev, with SUMMARY=1 refset.summary_refset_dev: the batch
is uploaded once outside the timed region, a timed call ends when its records are on the host (REFS_PER_SLAB=64 references a slab,
DEV_CAPACITY=1048576 records of room), and its records_crc32 is printed next to the host call's.
WIDE=1 is a leg of its own: WIDE_REFS=300 references of WIDE_BP=50000 bases - plasmid-sized, over KBO_REFSET_MAX_ROWS rows each - built
twice in one process, by kbo_refset_build (every reference through the single-index pipeline, one at a time) and by
kbo_refset_build_wide (the packed form walked from memory, refset_wide_kernels.hip), and run against the same contigs on both strands:
both builds' and both calls' seconds, records_crc32 of both (they must be equal) and the wide kernel's share of the references and
pairs of its call.  SUMMARY=1 and REPEATS apply; nothing else of the above runs.
BEST=1 is a leg of its own on the first workload: kbo_best_refset - one record per contig, reduced on the device - against what a
caller did before it: kbo_summary_refset plus the fold of its records in numpy (sort by (seq, most matches, ref, strand), the first
record of every contig, the first of another reference).  Both in one session, median of REPEATS behind a warm-up; the seconds of
each, of the fold alone, the records the summary sent, and the CRC of the best records next to the CRC of the folded summary records
(they must be equal).  LOOP, SUMMARY and DEV do not apply.
PREFILTER=1 is a leg of its own: the same call on the same references built without and with the seed table (RefSet.build(...,
prefilter=True)), in one session: kbo_find_refset, with SUMMARY=1 kbo_summary_refset, with BEST=1 kbo_best_refset, on the first
workload or, with WIDE=1, on the wide leg's references as a set of the wide route.  Median of REPEATS behind a warm-up for both sets;
the seconds of both, whether the records' CRCs are equal, kbo_refset_last_prefilter's counters (pairs of packed references, with
their bit set, walked, whether the screen ran), and the table's bytes and the seconds its build added.  LOOP and DEV do not apply.
The screen kernel's own time: run this under a kernel trace and read refset_screen_kernel's row.
DEV=1 PREFILTER=1 is a leg of its own on the first workload, one set built with the seed table, one session: the screened
device-resident form (refset.find_refset_dev(..., screened=True), with SUMMARY=1 / BEST=1 the summary / best form; the caps come from
one read-back of RefSet.candidates_dev's figures outside the timed region), next to the unscreened device-resident form on the same
set (REFS_PER_SLAB, DEV_CAPACITY as above) and next to the host form, which screens.  The batch is uploaded once outside the timed
regions; a timed device call ends when its records are on the host.  Median of REPEATS behind a warm-up for each; records_crc32 of
each, the statistics the screened call left on the device, and the ratios.
LOCATE=1 is a leg of its own on the first workload, one session: two sets, without and with the position table
(RefSet.build(..., positions=True); with PREFILTER=1 both carry the seed table, so the find in front of the locate screens), and on
the second one kbo_find_refset, kbo_find_refset followed by kbo_locate_refset (find_refset(..., locate=True)), and kbo_locate_refset
alone over the runs of the find.  Median of REPEATS behind a warm-up for each; the seconds of the three, the table's bytes and both
sets' build seconds, the sum of n_tested and a CRC of the loci (it compares two builds; the host form's CRC, made once outside the
timed regions, stands next to it).  LOOP, SUMMARY, DEV, WIDE and BEST do not apply.
COVER=1 is a leg of its own next to LOCATE=1, on the same set with the position table, one session: kbo_find_refset, kbo_locate_refset
and kbo_cover_refset (with and without the depth profile) over the runs of the find, median of REPEATS behind a warm-up for each; a
CRC of the records and of the profile, the host form's next to them (made once outside the timed regions), and the sums of the
records' fields.  For breadth alone on an assembly there is an older way with another definition - an index of the QUERY
(kbo_index_build_device) and kbo_summary_batch with the references as the batch: its seconds stand next to the cover's, the time only.
CALL=1 is a leg of its own on the first workload, one session (K=63 for it: useful calls need k of about twice the threshold or more;
PREFILTER=1 builds the set with the seed table): kbo_call_refset next to kbo_summary_refset on the same set - the floor: the same
walk - and next to the only way there was before, one kbo_index_build + kbo_index_to_device + kbo_call_batch per reference over the
contigs and their reverse complements, for LOOP references (LOOP=0: every reference), scaled to all of them.  Median of REPEATS
behind a warm-up for the set's calls; the seconds, kbo_refset_last_call's counters (pairs, candidates, sites, variants), and a CRC of
the variants of the references the loop took from both routes - the loop's filtered to the pairs with a summary record, as the call
is defined - which must be equal.
CALL=1 DEV=1 is a leg of its own on the same workload, one set, one session: kbo_call_refset next to the device-resident form - with
PREFILTER=1 kbo_call_refset_screened_dev with caps from kbo_refset_candidates_dev's figures, else kbo_call_refset_dev (REFS_PER_SLAB) -
and next to the floor, the summary's device form on the same set.  The batch is uploaded once outside the timed regions; a timed
device call ends when its records, characters and stats are on the host.  Median of REPEATS behind a warm-up for each; variants_crc32
of both calls (they must be equal) and the device form's stats.  MAX_SITES=65536 sizes its lists.  LOOP does not apply.
The LDS kernel's own rate: run this under a kernel trace with LOOP=0 REPEATS=1 and divide the pair-bases by refset_walk_kernel's time."""
import json
import os
import statistics
import sys
import time
import zlib

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import kbo_amd  # noqa: E402
from kbo_amd import batch, refset  # noqa: E402

REFS, REF_BP, QUERY_BP, CONTIGS, LOOP, REPEATS, SUMMARY = (int(os.environ.get(n, d)) for n, d in (
    ("REFS", 2000), ("REF_BP", 1000), ("QUERY_BP", 5_000_000), ("CONTIGS", 50), ("LOOP", 50), ("REPEATS", 3), ("SUMMARY", 0)))
DEV, REFS_PER_SLAB, DEV_CAPACITY = (int(os.environ.get(n, d)) for n, d in (("DEV", 0), ("REFS_PER_SLAB", 64), ("DEV_CAPACITY", 1 << 20)))
WIDE, WIDE_REFS, WIDE_BP = (int(os.environ.get(n, d)) for n, d in (("WIDE", 0), ("WIDE_REFS", 300), ("WIDE_BP", 50_000)))
BEST = int(os.environ.get("BEST", 0))
PREFILTER = int(os.environ.get("PREFILTER", 0))
LOCATE = int(os.environ.get("LOCATE", 0))
COVER = int(os.environ.get("COVER", 0))
CALL = int(os.environ.get("CALL", 0))
K, THREADS = int(os.environ.get("K", 31)), 16
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
rng = np.random.default_rng(2024)
refs = [ACGT[rng.integers(0, 4, REF_BP)] for _ in range(REFS)]
per = QUERY_BP // CONTIGS
contigs = [ACGT[rng.integers(0, 4, per)] for _ in range(CONTIGS)]
for i, r in enumerate(range(0, REFS, 40)):
    c = contigs[i % CONTIGS]
    at = int(rng.integers(0, per - REF_BP))
    copy = refs[r].copy()
    pos = np.flatnonzero(rng.random(REF_BP) < 0.01)
    copy[pos] = ACGT[(np.searchsorted(ACGT, copy[pos]) + 1) % 4]
    c[at:at + REF_BP] = copy
concat = np.concatenate(contigs)
offsets = (np.arange(CONTIGS + 1, dtype=np.uint64) * np.uint64(per))
opts = kbo_amd.BuildOpts(k=K, num_threads=THREADS)
fopts = kbo_amd.FindOpts()
pair_bases = REFS * 2 * int(offsets[-1])

import torch  # noqa: E402
assert torch.cuda.is_available(), "this measures the GPU path: no device, no number"


def wide_refs():
    """the wide leg's references.  (It plants its copies in the module's `contigs` AFTER `concat` was made of them: a leg that takes
    them passes `contigs` to its calls and exits, no other leg runs behind it)"""
    big = [ACGT[rng.integers(0, 4, WIDE_BP)] for _ in range(WIDE_REFS)]
    for i, r in enumerate(range(0, WIDE_REFS, 10)):  # a stretch of every 10th reference with 1 % substitutions lies in the query
        c = contigs[i % CONTIGS]
        n = min(5000, WIDE_BP, per)
        at = int(rng.integers(0, per - n + 1))
        copy = big[r][:n].copy()
        pos = np.flatnonzero(rng.random(n) < 0.01)
        copy[pos] = ACGT[(np.searchsorted(ACGT, copy[pos]) + 1) % 4]
        c[at:at + n] = copy
    return big


def prefilter_leg():
    """the same call on the same references, built without and with the prefilter"""
    the_refs, rows = (wide_refs(), refset.WIDE_MAX_ROWS) if WIDE else (refs, None)
    form = "best_refset" if BEST else "summary_refset" if SUMMARY else "find_refset"
    total = len(the_refs) * 2 * int(offsets[-1])
    out = {"workload": {"refs": len(the_refs), "ref_bp": len(the_refs[0]), "query_bp": int(offsets[-1]), "contigs": CONTIGS, "k": K, "strands": 2,
                        "pair_bases": total}, "form": form}
    for label, pre in (("plain", False), ("prefilter", True)):
        a = time.perf_counter()
        s = refset.RefSet.build(the_refs, opts, wide_rows=rows, prefilter=pre)
        b = time.perf_counter()
        s.to_device()
        torch.cuda.synchronize()
        c = time.perf_counter()

        def call():
            if BEST:
                return refset.best_refset(contigs, s, fopts.max_error_prob, strands=3)
            if SUMMARY:
                return refset.summary_refset(contigs, s, fopts.max_error_prob, strands=3)
            return refset.find_refset(contigs, s, fopts, strands=3)
        got = call()  # warm-up: code objects, the call's buffers
        ts = []
        for _ in range(REPEATS):
            t = time.perf_counter()
            got = call()
            ts.append(time.perf_counter() - t)
        out[label] = {"build_s": round(b - a, 4), "to_device_s": round(c - b, 4), "call_s": round(statistics.median(ts), 4),
                      "call_s_all": [round(t, 4) for t in ts], "gbp_per_s": round(total / statistics.median(ts) / 1e9, 2),
                      "records": int(len(got)), "records_crc32": zlib.crc32(got.tobytes()), "routes": refset.last_routes(),
                      "prefilter_counters": refset.last_prefilter(), "prefilter_bytes": s.prefilter_bytes()}
        del s
    out["records_equal"] = out["plain"]["records_crc32"] == out["prefilter"]["records_crc32"]
    out["table_build_s"] = round(out["prefilter"]["build_s"] - out["plain"]["build_s"], 4)
    out["plain_over_prefilter"] = round(out["plain"]["call_s"] / out["prefilter"]["call_s"], 2)
    print(json.dumps(out))


def wide_leg():
    """the same large references as a set of the single-index route and as a set of the wide route, one process"""
    big = wide_refs()
    out = {"workload": {"refs": WIDE_REFS, "ref_bp": WIDE_BP, "query_bp": int(offsets[-1]), "contigs": CONTIGS, "k": K, "strands": 2,
                        "pair_bases": WIDE_REFS * 2 * int(offsets[-1])}, "form": "summary_refset" if SUMMARY else "find_refset"}
    for label, rows in (("index_route", None), ("wide_route", refset.WIDE_MAX_ROWS)):
        a = time.perf_counter()
        s = refset.RefSet.build(big, opts, wide_rows=rows)
        b = time.perf_counter()
        s.to_device()
        torch.cuda.synchronize()
        c = time.perf_counter()

        def call():
            if SUMMARY:
                return refset.summary_refset(contigs, s, fopts.max_error_prob, strands=3)
            return refset.find_refset(contigs, s, fopts, strands=3)
        got = call()  # warm-up: code objects, the call's buffers, the plan structures of the single-index route
        ts = []
        for _ in range(REPEATS):
            t = time.perf_counter()
            got = call()
            ts.append(time.perf_counter() - t)
        routes, wide = refset.last_routes(), refset.last_wide()
        out[label] = {"build_s": round(b - a, 4), "to_device_s": round(c - b, 4), "call_s": round(statistics.median(ts), 4),
                      "call_s_all": [round(t, 4) for t in ts], "gbp_per_s": round(out["workload"]["pair_bases"] / statistics.median(ts) / 1e9, 2),
                      "records": int(len(got)), "records_crc32": zlib.crc32(got.tobytes()), "routes": routes, "wide": wide,
                      "wide_share_of_refs": round(wide[0] / max(1, routes[0] + routes[1] + wide[0]), 3)}
        del s
    out["records_equal"] = out["index_route"]["records_crc32"] == out["wide_route"]["records_crc32"]
    out["index_over_wide"] = round(out["index_route"]["call_s"] / out["wide_route"]["call_s"], 2)
    print(json.dumps(out))


def screened_dev_leg():
    """the screened device form next to the unscreened one and to the host form with the prefilter: one set, one session"""
    form = "best_refset" if BEST else "summary_refset" if SUMMARY else "find_refset"
    s = refset.RefSet.build(refs, opts, prefilter=True).to_device()
    d_q = torch.zeros(int(offsets[-1]) + 16, dtype=torch.uint8, device="cuda")
    d_q[:int(offsets[-1])].copy_(torch.from_numpy(concat))
    d_off = torch.from_numpy(offsets.astype(np.int64)).cuda()
    cand = [int(v) for v in s.candidates_dev(d_q, d_off, fopts.max_error_prob, strands=3)[1].cpu().numpy()]
    max_pairs, max_bases = max(1, cand[0]), cand[1]
    torch.cuda.synchronize()
    stats = {}

    def host_call():
        if BEST:
            return refset.best_refset(contigs, s, fopts.max_error_prob, strands=3)
        if SUMMARY:
            return refset.summary_refset(contigs, s, fopts.max_error_prob, strands=3)
        return refset.find_refset(contigs, s, fopts, strands=3)

    def dev_call(screened):
        kw = dict(screened=True, max_pairs=max_pairs, max_pair_bases=max_bases) if screened else dict(refs_per_slab=REFS_PER_SLAB)
        if BEST:
            got = refset.best_refset_dev(d_q, d_off, s, fopts.max_error_prob, strands=3, **kw)
            table = (got[0] if screened else got).cpu().numpy()  # (waits for the stream: the only synchronisation of the call)
            if screened:
                stats["stats"] = [int(v) for v in got[1].cpu().numpy()]
            return np.ascontiguousarray(table).view(np.uint32)
        if SUMMARY:
            got = refset.summary_refset_dev(d_q, d_off, s, fopts.max_error_prob, strands=3, capacity=DEV_CAPACITY, **kw)
        else:
            got = refset.find_refset_dev(d_q, d_off, s, fopts, strands=3, capacity=DEV_CAPACITY, **kw)
        n = int(got[1].item())  # (waits for the stream: the only synchronisation of the call)
        if screened:
            stats["stats"] = [int(v) for v in got[2].cpu().numpy()]
        return np.ascontiguousarray(got[0][:min(n, DEV_CAPACITY)].cpu().numpy()).view(np.uint32)

    def timed(fn):
        got = fn()  # warm-up: code objects, the allocator's blocks
        ts = []
        for _ in range(REPEATS):
            t = time.perf_counter()
            got = fn()
            ts.append(time.perf_counter() - t)
        return {"call_s": round(statistics.median(ts), 5), "call_s_all": [round(t, 5) for t in ts], "records": int(len(got)),
                "records_crc32": zlib.crc32(got.tobytes())}
    out = {"workload": {"refs": REFS, "ref_bp": REF_BP, "query_bp": int(offsets[-1]), "contigs": CONTIGS, "k": K, "strands": 2, "pair_bases": pair_bases},
           "form": form, "max_pairs": max_pairs, "max_pair_bases": max_bases}
    out["screened_dev"] = timed(lambda: dev_call(True))
    out["screened_dev"]["stats"] = dict(zip(("n_candidates", "candidate_bases", "n_walked", "walked_bases"), stats["stats"]))
    out["host_prefilter"] = timed(host_call)
    out["host_prefilter"]["prefilter_counters"] = refset.last_prefilter()
    out["unscreened_dev"] = timed(lambda: dev_call(False))
    out["unscreened_dev"]["refs_per_slab"] = REFS_PER_SLAB
    out["records_equal"] = out["screened_dev"]["records_crc32"] == out["host_prefilter"]["records_crc32"] == out["unscreened_dev"]["records_crc32"]
    out["unscreened_over_screened"] = round(out["unscreened_dev"]["call_s"] / out["screened_dev"]["call_s"], 2)
    out["host_over_screened"] = round(out["host_prefilter"]["call_s"] / out["screened_dev"]["call_s"], 2)
    print(json.dumps(out))


def locate_leg():
    """find, find + locate and locate alone on a set with the position table; its build next to the set without"""
    out = {"workload": {"refs": REFS, "ref_bp": REF_BP, "query_bp": int(offsets[-1]), "contigs": CONTIGS, "k": K, "strands": 2, "pair_bases": pair_bases},
           "prefilter": bool(PREFILTER)}
    sets = {}
    for label, pos in (("plain", False), ("positions", True)):
        a = time.perf_counter()
        s = refset.RefSet.build(refs, opts, prefilter=bool(PREFILTER), positions=pos)
        b = time.perf_counter()
        s.to_device()
        torch.cuda.synchronize()
        c = time.perf_counter()
        out[label] = {"build_s": round(b - a, 4), "to_device_s": round(c - b, 4), "positions_bytes": s.positions_bytes(),
                      "prefilter_bytes": s.prefilter_bytes()}
        sets[label] = s
    s = sets["positions"]

    def timed(fn):
        got = fn()  # warm-up: code objects, the call's buffers
        ts = []
        for _ in range(REPEATS):
            t = time.perf_counter()
            got = fn()
            ts.append(time.perf_counter() - t)
        return statistics.median(ts), [round(t, 5) for t in ts], got
    find_s, find_all, runs = timed(lambda: refset.find_refset(contigs, s, fopts, strands=3))
    both_s, both_all, (runs2, loci2) = timed(lambda: refset.find_refset(contigs, s, fopts, strands=3, locate=True))
    loc_s, loc_all, loci = timed(lambda: refset.locate_refset(contigs, s, runs))
    host = refset.locate_refset(contigs, s, runs, host=True)
    plain_runs = refset.find_refset(contigs, sets["plain"], fopts, strands=3)
    out.update({"find_refset_s": round(find_s, 5), "find_refset_s_all": find_all, "find_plus_locate_s": round(both_s, 5),
                "find_plus_locate_s_all": both_all, "locate_refset_s": round(loc_s, 5), "locate_refset_s_all": loc_all,
                "locate_over_find": round(loc_s / find_s, 4), "runs": int(len(runs)), "runs_crc32": zlib.crc32(runs.tobytes()),
                "runs_equal_plain_set": runs.tobytes() == plain_runs.tobytes() == runs2.tobytes(),
                "table_build_s": round(out["positions"]["build_s"] - out["plain"]["build_s"], 4),
                "n_tested_sum": int(loci["n_tested"].astype(np.int64).sum()), "with_anchor": int((loci["q_first"] != refset.LOCUS_NONE).sum()),
                "loci_crc32": zlib.crc32(loci.tobytes()), "host_loci_crc32": zlib.crc32(host.tobytes()),
                "loci_equal_host": loci.tobytes() == host.tobytes() == loci2.tobytes(), "prefilter_counters": refset.last_prefilter()})
    print(json.dumps(out))


def cover_leg():
    """find, locate and cover over the runs of the find on a set with the position table; breadth by an index of the query next to it"""
    out = {"workload": {"refs": REFS, "ref_bp": REF_BP, "query_bp": int(offsets[-1]), "contigs": CONTIGS, "k": K, "strands": 2, "pair_bases": pair_bases},
           "prefilter": bool(PREFILTER)}
    a = time.perf_counter()
    s = refset.RefSet.build(refs, opts, prefilter=bool(PREFILTER), positions=True)
    b = time.perf_counter()
    s.to_device()
    torch.cuda.synchronize()
    out["set"] = {"build_s": round(b - a, 4), "to_device_s": round(time.perf_counter() - b, 4), "positions_bytes": s.positions_bytes(),
                  "cover_bases": s.cover_bases(), "cover_work_bytes": s.cover_work_bytes()}

    def timed(fn):
        got = fn()  # warm-up: code objects, the call's buffers
        ts = []
        for _ in range(REPEATS):
            t = time.perf_counter()
            got = fn()
            ts.append(time.perf_counter() - t)
        return statistics.median(ts), [round(t, 5) for t in ts], got
    find_s, find_all, runs = timed(lambda: refset.find_refset(contigs, s, fopts, strands=3))
    loc_s, loc_all, loci = timed(lambda: refset.locate_refset(contigs, s, runs))
    cov_s, cov_all, covers = timed(lambda: refset.cover_refset(contigs, s, runs))
    dep_s, dep_all, (covers2, depth, _) = timed(lambda: refset.cover_refset(contigs, s, runs, depth=True))
    t = time.perf_counter()
    host, host_depth, _ = refset.cover_refset(contigs, s, runs, depth=True, host=True)
    host_s = time.perf_counter() - t

    def by_query_index():  # another definition of breadth: the references' bases that match an index of the query
        sbwt, _ = kbo_amd.build(contigs, kbo_amd.BuildOpts(k=K, add_revcomp=True, num_threads=THREADS), device=-1)
        return batch.summary_batch(sbwt, refs, fopts.max_error_prob)
    alt_s, alt_all, alt = timed(by_query_index)
    windows = np.maximum(0, runs["end"].astype(np.int64) - runs["start"].astype(np.int64) - K + 1)
    out.update({"find_refset_s": round(find_s, 5), "find_refset_s_all": find_all, "locate_refset_s": round(loc_s, 5), "locate_refset_s_all": loc_all,
                "cover_refset_s": round(cov_s, 5), "cover_refset_s_all": cov_all, "cover_refset_depth_s": round(dep_s, 5),
                "cover_refset_depth_s_all": dep_all, "cover_over_find": round(cov_s / find_s, 4), "cover_host_s": round(host_s, 4),
                "index_of_query_plus_summary_s": round(alt_s, 5), "index_of_query_plus_summary_s_all": alt_all,
                "index_of_query_refs_with_a_match": int((alt[:, 0] > 0).sum()),
                "runs": int(len(runs)), "runs_crc32": zlib.crc32(runs.tobytes()), "windows": int(windows.sum()),
                "refs_covered": int((covers["covered"] > 0).sum()), "covered_sum": int(covers["covered"].astype(np.int64).sum()),
                "segments_sum": int(covers["n_segments"].astype(np.int64).sum()), "n_anchors_sum": int(covers["n_anchors"].sum()),
                "n_multi_sum": int(covers["n_multi"].sum()), "max_depth": int(covers["max_depth"].max()),
                "covers_crc32": zlib.crc32(covers.tobytes()), "host_covers_crc32": zlib.crc32(host.tobytes()),
                "depth_crc32": zlib.crc32(depth.tobytes()), "host_depth_crc32": zlib.crc32(host_depth.tobytes()),
                "covers_equal_host": covers.tobytes() == host.tobytes() == covers2.tobytes(), "depth_equal_host": depth.tobytes() == host_depth.tobytes(),
                "loci_crc32": zlib.crc32(loci.tobytes()), "prefilter_counters": refset.last_prefilter()})
    print(json.dumps(out))


def call_leg():
    """kbo_call_refset next to kbo_summary_refset on the same set, and next to one index + kbo_call_batch per reference"""
    out = {"workload": {"refs": REFS, "ref_bp": REF_BP, "query_bp": int(offsets[-1]), "contigs": CONTIGS, "k": K, "strands": 2, "pair_bases": pair_bases},
           "prefilter": bool(PREFILTER)}
    copts = kbo_amd.CallOpts(max_error_prob=fopts.max_error_prob, sbwt_build_opts=kbo_amd.BuildOpts(k=K, build_select=True))
    a = time.perf_counter()
    s = refset.RefSet.build(refs, opts, prefilter=bool(PREFILTER))
    b = time.perf_counter()
    s.to_device()
    torch.cuda.synchronize()
    out["set"] = {"build_s": round(b - a, 4), "to_device_s": round(time.perf_counter() - b, 4)}

    def timed(fn):
        got = fn()  # warm-up: code objects, the call's buffers
        ts = []
        for _ in range(REPEATS):
            t = time.perf_counter()
            got = fn()
            ts.append(time.perf_counter() - t)
        return statistics.median(ts), [round(t, 5) for t in ts], got
    sum_s, sum_all, summ = timed(lambda: refset.summary_refset(contigs, s, fopts.max_error_prob, strands=3))
    call_s, call_all, (variants, chars) = timed(lambda: refset.call_refset(contigs, s, copts, strands=3))
    counters, pre = refset.last_call(), refset.last_prefilter()
    # the loop: the contigs and their reverse complements as one batch of 2 x CONTIGS sequences per reference
    comp = np.arange(256, dtype=np.uint8)
    for x, y in zip(b"ACGT", b"TGCA"):
        comp[x] = y
    both = np.concatenate([concat] + [comp[c[::-1]] for c in contigs])
    both_off = np.concatenate([offsets, offsets[1:] + offsets[-1]])
    picks = list(range(REFS)) if LOOP <= 0 else list(range(0, REFS, max(1, REFS // LOOP)))[:LOOP]
    kept = {(int(r), int(q), int(st)) for r, q, st in zip(summ["ref"], summ["seq"], summ["strand"])}

    def one(r):
        t0_ = time.perf_counter()
        sbwt, _ = kbo_amd.build([refs[r]], kbo_amd.BuildOpts(k=K))
        t1_ = time.perf_counter()
        sbwt.to_device()
        torch.cuda.synchronize()
        t2_ = time.perf_counter()
        res = batch.call_batch_arrays(sbwt, both, both_off, copts)
        t3_ = time.perf_counter()
        return (t1_ - t0_, t2_ - t1_, t3_ - t2_), res
    for r in (REFS - 1, REFS - 2):
        one(r)
    sums, loop_recs = np.zeros(3), []
    for r in picks:
        t, res = one(r)
        sums += t
        if int(res["var_offsets"][-1]) == 0:
            continue
        for x in range(2 * CONTIGS):
            key = (r, x % CONTIGS, x // CONTIGS + 1)
            if key in kept:
                loop_recs += [key + v for v in batch.variants_of(res, x)]
    loop_recs.sort(key=lambda v: v[:4])
    mine = [(int(v["ref"]), int(v["seq"]), int(v["strand"]), int(v["pos"])) + refset.variant_chars(v, chars)
            for v in variants[np.isin(variants["ref"], picks)]]
    crc = lambda recs: zlib.crc32(repr(recs).encode())
    per_ref = sums / max(1, len(picks))
    loop_all = float(per_ref.sum()) * REFS
    out.update({"summary_refset_s": round(sum_s, 5), "summary_refset_s_all": sum_all, "summary_records": int(len(summ)),
                "call_refset_s": round(call_s, 5), "call_refset_s_all": call_all, "call_over_summary": round(call_s / sum_s, 3),
                "pairs_scanned": counters[0], "candidates": counters[1], "sites": counters[2], "variants": counters[3],
                "n_chars": int(len(chars)), "prefilter_counters": pre, "variants_crc32": zlib.crc32(variants.tobytes() + chars.tobytes()),
                "loop_refs_timed": len(picks),
                "loop_per_ref_s": {"build": round(per_ref[0], 5), "to_device": round(per_ref[1], 5), "call_batch": round(per_ref[2], 5)},
                "loop_scaled_s": round(loop_all, 2), "ratio_loop_over_call": round(loop_all / call_s, 1),
                "loop_variants": len(loop_recs), "set_variants_of_loop_refs": len(mine),
                "loop_records_crc32": crc(loop_recs), "set_records_crc32": crc(mine), "records_equal_loop": loop_recs == mine})
    print(json.dumps(out))
    assert loop_recs == mine, "kbo_call_refset and the loop over single indexes differ"


def call_dev_leg():
    """kbo_call_refset next to its device-resident form and to the summary's device form, the floor: one set, one session"""
    max_sites = int(os.environ.get("MAX_SITES", 1 << 16))
    copts = kbo_amd.CallOpts(max_error_prob=fopts.max_error_prob, sbwt_build_opts=kbo_amd.BuildOpts(k=K, build_select=True))
    s = refset.RefSet.build(refs, opts, prefilter=bool(PREFILTER)).to_device()
    d_q = torch.zeros(int(offsets[-1]) + 16, dtype=torch.uint8, device="cuda")
    d_q[:int(offsets[-1])].copy_(torch.from_numpy(concat))
    d_off = torch.from_numpy(offsets.astype(np.int64)).cuda()
    kw = dict(refs_per_slab=REFS_PER_SLAB)
    if PREFILTER:
        cand = [int(v) for v in s.candidates_dev(d_q, d_off, fopts.max_error_prob, strands=3)[1].cpu().numpy()]
        kw = dict(screened=True, max_pairs=max(1, cand[0]), max_pair_bases=cand[1])
    torch.cuda.synchronize()
    stats = {}

    def host_call():
        variants, chars = refset.call_refset(contigs, s, copts, strands=3)
        return variants.tobytes() + chars.tobytes(), len(variants)

    def dev_call():
        got = refset.call_refset_dev(d_q, d_off, s, copts, strands=3, max_variants=DEV_CAPACITY, max_chars=4 * DEV_CAPACITY, max_sites=max_sites, **kw)
        st = [int(v) for v in got[2].cpu().numpy()]  # (waits for the stream: the only synchronisation of the call)
        stats["stats"] = dict(zip(("n_variants", "n_chars", "n_sites", "max_slab_candidates", "n_panics"), st))
        if PREFILTER:
            stats["screen"] = dict(zip(("n_candidates", "candidate_bases", "n_walked", "walked_bases"), (int(v) for v in got[3].cpu().numpy())))
        n, nc = min(st[0], DEV_CAPACITY), min(st[1], 4 * DEV_CAPACITY)
        return np.ascontiguousarray(got[0][:n].cpu().numpy()).tobytes() + got[1][:nc].cpu().numpy().tobytes(), n

    def floor_call():
        got = refset.summary_refset_dev(d_q, d_off, s, fopts.max_error_prob, strands=3, capacity=DEV_CAPACITY, **kw)
        n = int(got[1].item())
        return np.ascontiguousarray(got[0][:min(n, DEV_CAPACITY)].cpu().numpy()).tobytes(), n

    def timed(fn, what):
        got = fn()  # warm-up: code objects, the allocator's blocks
        ts = []
        for _ in range(REPEATS):
            t = time.perf_counter()
            got = fn()
            ts.append(time.perf_counter() - t)
        return {"call_s": round(statistics.median(ts), 5), "call_s_all": [round(t, 5) for t in ts], what: got[1], what + "_crc32": zlib.crc32(got[0])}
    out = {"workload": {"refs": REFS, "ref_bp": REF_BP, "query_bp": int(offsets[-1]), "contigs": CONTIGS, "k": K, "strands": 2, "pair_bases": pair_bases},
           "prefilter": bool(PREFILTER), "max_sites": max_sites}
    out["call_refset_dev"] = timed(dev_call, "variants")
    out["call_refset_dev"].update(stats)
    out["call_refset_dev"].update({k_: v for k_, v in kw.items() if k_ != "screened"})
    out["call_refset"] = timed(host_call, "variants")
    out["call_refset"]["counters"] = refset.last_call()
    out["summary_refset_dev"] = timed(floor_call, "records")
    st = stats["stats"]
    out["complete"] = st["max_slab_candidates"] <= max_sites and st["n_sites"] <= max_sites
    out["variants_equal"] = out["call_refset_dev"]["variants_crc32"] == out["call_refset"]["variants_crc32"]
    out["host_over_dev"] = round(out["call_refset"]["call_s"] / out["call_refset_dev"]["call_s"], 2)
    out["dev_over_floor"] = round(out["call_refset_dev"]["call_s"] / out["summary_refset_dev"]["call_s"], 2)
    print(json.dumps(out))
    assert out["variants_equal"], "kbo_call_refset and its device-resident form differ"


if CALL and DEV:
    call_dev_leg()
    sys.exit(0)

if CALL:
    call_leg()
    sys.exit(0)

if LOCATE:
    locate_leg()
    sys.exit(0)

if COVER:
    cover_leg()
    sys.exit(0)

if PREFILTER and DEV:
    screened_dev_leg()
    sys.exit(0)

if PREFILTER:
    prefilter_leg()
    sys.exit(0)

if WIDE:
    wide_leg()
    sys.exit(0)

t0 = time.perf_counter()
rs = refset.RefSet.build(refs, opts)
t1 = time.perf_counter()
rs.to_device()
torch.cuda.synchronize()
t2 = time.perf_counter()


def runs_per_pair(records):
    """{(ref, seq, strand): number of records} of find_refset's records"""
    keys, counts = np.unique(np.stack([records["ref"], records["seq"], records["strand"]], axis=1), axis=0, return_counts=True) \
        if len(records) else (np.zeros((0, 3), dtype=np.uint32), np.zeros(0, dtype=np.int64))
    return {tuple(int(v) for v in key): int(c) for key, c in zip(keys, counts)}


def fold_best(summ, n_seqs):
    """REF_BEST of every sequence from summary_refset's records, in numpy"""
    out = np.zeros(n_seqs, dtype=refset.REF_BEST)
    out["seq"] = np.arange(n_seqs, dtype=np.uint32)
    out["ref"] = out["second_ref"] = refset.REF_NONE
    if not len(summ):
        return out

    def firsts(rec):
        """the first record of every sequence that has one, by (most matches, ref, strand)"""
        order = np.lexsort((rec["strand"], rec["ref"], -rec["n_match"].astype(np.int64), rec["seq"]))
        rec = rec[order]
        return rec[np.concatenate([[True], rec["seq"][1:] != rec["seq"][:-1]])]
    top = firsts(summ)
    at = top["seq"]
    for f in ("ref", "strand", "n_match", "n_mismatch", "n_jump", "n_runs", "start", "end"):
        out[f][at] = top[f]
    out["n_hits"] = np.bincount(summ["seq"], minlength=n_seqs).astype(np.uint32)
    rest = summ[summ["ref"] != out["ref"][summ["seq"]]]
    if len(rest):
        second = firsts(rest)
        out["second_ref"][second["seq"]] = second["ref"]
        out["second_match"][second["seq"]] = second["n_match"]
    return out


def best_leg():
    def timed(fn):
        fn()  # warm-up: code objects, the call's buffers
        ts, got = [], None
        for _ in range(REPEATS):
            t = time.perf_counter()
            got = fn()
            ts.append(time.perf_counter() - t)
        return statistics.median(ts), [round(t, 4) for t in ts], got
    best_s, best_all, best = timed(lambda: refset.best_refset(contigs, rs, fopts.max_error_prob, strands=3))
    routes, launches = refset.last_routes(), refset.last_best()
    summ_s, summ_all, summ = timed(lambda: refset.summary_refset(contigs, rs, fopts.max_error_prob, strands=3))
    fold_s, fold_all, folded = timed(lambda: fold_best(summ, CONTIGS))
    print(json.dumps({
        "workload": {"refs": REFS, "ref_bp": REF_BP, "query_bp": int(offsets[-1]), "contigs": CONTIGS, "k": K, "strands": 2, "pair_bases": pair_bases},
        "best_refset_s": round(best_s, 4), "best_refset_s_all": best_all, "best_refset_gbp_per_s": round(pair_bases / best_s / 1e9, 2),
        "summary_refset_s": round(summ_s, 4), "summary_refset_s_all": summ_all, "numpy_fold_s": round(fold_s, 4), "numpy_fold_s_all": fold_all,
        "summary_plus_fold_s": round(summ_s + fold_s, 4), "summary_plus_fold_over_best": round((summ_s + fold_s) / best_s, 3),
        "summary_records": int(len(summ)), "best_records": int(len(best)), "best_with_a_hit": int((best["ref"] != refset.REF_NONE).sum()),
        "best_records_crc32": zlib.crc32(best.tobytes()), "folded_summary_crc32": zlib.crc32(folded.tobytes()),
        "best_equals_folded_summary": best.tobytes() == folded.tobytes(), "routes": routes, "best_launches": launches}))


if BEST:
    best_leg()
    sys.exit(0)

if SUMMARY:
    def call():
        return refset.summary_refset(contigs, rs, fopts.max_error_prob, strands=3)
    name = "summary_refset"
else:
    def call():
        return refset.find_refset(contigs, rs, fopts, strands=3)
    name = "find_refset"
got = call()  # warm-up: code objects, the call's buffers
times = []
for _ in range(REPEATS):
    t = time.perf_counter()
    got = call()
    times.append(time.perf_counter() - t)
find_s = statistics.median(times)
res = {"workload": {"refs": REFS, "ref_bp": REF_BP, "query_bp": int(offsets[-1]), "contigs": CONTIGS, "k": K, "strands": 2, "pair_bases": pair_bases},
       "refset_build_s": round(t1 - t0, 4), "refset_to_device_s": round(t2 - t1, 4), name + "_s": round(find_s, 4),
       name + "_s_all": [round(t, 4) for t in times], name + "_gbp_per_s": round(pair_bases / find_s / 1e9, 2),
       "records": int(len(got)), "records_crc32": zlib.crc32(got.tobytes()), "routes": refset.last_routes()}

if DEV:
    d_q = torch.zeros(int(offsets[-1]) + 16, dtype=torch.uint8, device="cuda")
    d_q[:int(offsets[-1])].copy_(torch.from_numpy(concat))
    d_off = torch.from_numpy(offsets.astype(np.int64)).cuda()
    torch.cuda.synchronize()

    def dev_call():
        if SUMMARY:
            rec, count = refset.summary_refset_dev(d_q, d_off, rs, fopts.max_error_prob, strands=3, capacity=DEV_CAPACITY, refs_per_slab=REFS_PER_SLAB)
        else:
            rec, count = refset.find_refset_dev(d_q, d_off, rs, fopts, strands=3, capacity=DEV_CAPACITY, refs_per_slab=REFS_PER_SLAB)
        n = int(count.item())  # (waits for the stream: the only synchronisation of the call)
        return n, rec[:min(n, DEV_CAPACITY)].cpu().numpy()
    dev_call()  # warm-up: code objects, the allocator's blocks
    dev_times = []
    for _ in range(REPEATS):
        t = time.perf_counter()
        n_dev, dev_rec = dev_call()
        dev_times.append(time.perf_counter() - t)
    dev_s = statistics.median(dev_times)
    queryable = sum(rs.status(r) == 0 for r in range(REFS))
    res.update({name + "_dev_s": round(dev_s, 4), name + "_dev_s_all": [round(t, 4) for t in dev_times],
                name + "_dev_gbp_per_s": round(pair_bases / dev_s / 1e9, 2), "dev_refs_per_slab": REFS_PER_SLAB,
                "dev_slabs": -(-queryable // REFS_PER_SLAB), "dev_records": n_dev,
                "dev_records_crc32": zlib.crc32(np.ascontiguousarray(dev_rec).view(np.uint32).tobytes()),
                "dev_over_host": round(dev_s / find_s, 3)})
    res["dev_records_equal_host"] = res["dev_records_crc32"] == res["records_crc32"] and n_dev == len(got)

if SUMMARY:
    mine = {(int(r), int(s), int(st)): int(n) for r, s, st, n in zip(got["ref"], got["seq"], got["strand"], got["n_runs"])}
    if LOOP > 0:  # against the single-index loop, for the references it takes
        picks = list(range(0, REFS, max(1, REFS // LOOP)))[:LOOP]
        want = {}
        for r in picks:
            sbwt, _ = kbo_amd.build([refs[r]], kbo_amd.BuildOpts(k=K))
            rles, ro = batch.find_batch_strands(sbwt, concat, offsets, kbo_amd.FindOpts(max_gap_len=0), strands=3)
            for x in range(2 * CONTIGS):
                if ro[x + 1] > ro[x]:
                    want[r, x // 2, x % 2 + 1] = int(ro[x + 1] - ro[x])
        mine = {key: n for key, n in mine.items() if key[0] in set(picks)}
        res["runs_checked_refs"] = len(picks)
    else:  # against kbo_find_refset without gap filling, every reference
        want = runs_per_pair(refset.find_refset(contigs, rs, kbo_amd.FindOpts(max_gap_len=0), strands=3))
        res["runs_checked_refs"] = REFS
    res["n_runs_equal_find"] = mine == want
elif LOOP > 0:
    def one(r):
        """(seconds of build, of to_device, of find) for reference r alone, and its records"""
        a = time.perf_counter()
        sbwt, _ = kbo_amd.build([refs[r]], kbo_amd.BuildOpts(k=K))
        b = time.perf_counter()
        sbwt.to_device()
        torch.cuda.synchronize()
        c = time.perf_counter()
        rles, ro = batch.find_batch_strands(sbwt, concat, offsets, fopts, strands=3)
        d = time.perf_counter()
        return (b - a, c - b, d - c), rles
    for r in (REFS - 1, REFS - 2):
        one(r)
    picks = list(range(0, REFS, max(1, REFS // LOOP)))[:LOOP]
    sums, equal = np.zeros(3), True
    for r in picks:
        t, rles = one(r)
        sums += t
        mine = got[got["ref"] == r]
        equal = equal and len(mine) == len(rles) and all(
            np.array_equal(mine[f].astype(np.uint64), rles[:, i]) for i, f in enumerate(("start", "end", "matches", "mismatches", "jumps", "gap_bases", "gap_opens")))
    per_ref = sums / len(picks)
    loop_all = float(per_ref.sum()) * REFS
    res.update({"loop_refs_timed": len(picks), "loop_per_ref_s": {"build": round(per_ref[0], 5), "to_device": round(per_ref[1], 5), "find": round(per_ref[2], 5)},
                "loop_scaled_s": round(loop_all, 2), "set_total_s": round(t2 - t0 + find_s, 4),
                "ratio_loop_over_set": round(loop_all / (t2 - t0 + find_s), 1), "ratio_find_only": round(float(per_ref[2]) * REFS / find_s, 1),
                "records_equal_loop": bool(equal)})
print(json.dumps(res))
