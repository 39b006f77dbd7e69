/*
 * kbo_hip_tuning.h — tuning knobs, experiment switches and test hooks of libkbo_hip.so.
 *
 * NOT part of the drop-in boundary (include/kbo_hip.h): nothing here has a counterpart in the reference crate, no
 * setting changes a result (every combination is parity-tested against the oracle), and a binding of the reference
 * never needs this file.  The in-repo tests, tools/ and bench.py use it to force code paths through their corners at
 * small sizes and to record the measurements behind DESIGN.md section 6.  All settings are process-wide and apply to
 * launches (or, where stated, to device copies of an index) made after the call.
 */
#ifndef KBO_HIP_TUNING_H
#define KBO_HIP_TUNING_H

#include "kbo_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ launch geometry of the walk kernels */
/* upper bound on resident waves of the plain walk, and threads per workgroup */
int kbo_walk_geometry(int *max_waves, int *threads);
int kbo_set_walk_waves_per_cu(int waves_per_cu); /* 0 = default (32) */
int kbo_set_walk_threads(int threads);           /* workgroup size 64 / 128 / 256 */
int kbo_set_walk_rare(int period);               /* hot-loop iterations between item-bookkeeping visits (default 8) */
/* The guided walk (the plan-guided form of A1).  waves_per_cu: resident waves per CU, 0 = default (8 or 12, scaled with
 * kbo_set_walk_waves_per_cu; few, so that the lines of the lanes in flight stay in L2: DESIGN.md 4.2), < 0 keeps.
 * recovery_lines: 1 / 0 = the walk reads the index through the recovery lines (one 128-byte line per 64 rows with rank
 * blocks and LCS values) / through the rank blocks and contraction entries, -1 = by index size (default), < -1 keeps. */
int kbo_set_guided_walk(int waves_per_cu, int recovery_lines);

/* ------------------------------------------------------------------ index layout on the device */
/* Two-base extension blocks (2.7 B per index row on the device): built for indexes with at least min_rows rows
 * (default 24 Mi; 0 = always, UINT64_MAX = never; applies to device copies made after the call), used by the walk from
 * matches at least min_depth deep (default 16; < 0 keeps it). */
int kbo_set_pair_steps(uint64_t min_rows, int min_depth);
/* tests: the rank blocks, contraction entries and two-base blocks of the index's copy on `device` (-1: the current one) - made on the
 * device from the row bit-vectors and the LCS bytes (layout_kernels.hip) - against the host's single-threaded construction of the same
 * layout: *n_diff = the bytes that differ.  KBO_DEVICE_LAYOUT=0 in the environment makes copies from the host's instead. */
int kbo_index_layout_check(kbo_index_t *idx, int device, uint64_t *n_diff);
/* tests: the handle's path cover - laid out on the device by the first copy that needed it (cover_kernels.hip) - against the host's
 * construction (path_cover.cpp): *n_diff = entries of text / pos / node_at that differ.  KBO_DEVICE_COVER=0: the host's from the start. */
int kbo_index_cover_check(kbo_index_t *idx, uint64_t *n_diff);
/* Host batches (kbo_matches_batch / kbo_map_batch / kbo_find_batch and the packed forms): caller's buffers that are pinned
 * already (hipHostMalloc / hipHostRegister) are used in place - no staging copies, no host threads busy - instead of being
 * staged through the slots' own pinned buffers like pageable ones.  Default 0: staged is the faster of the two on the MI355X
 * boxes this was measured on (600 Mbp: 34.9 against 27.7 Gbp/s, packed 123 against 104).  Environment: KBO_HOST_INPLACE. */
int kbo_set_host_in_place(int on);
/* tests: force the 64-bit-offset contraction-entry layout (device copies made after the call) */
int kbo_set_force_big_layout(int on);
/* tests: kbo_index_build makes at least this many shards whatever the size of its input (0 = by size: one index below
 * 3.76 * 10^9 rows); see kbo_hip.h "Sharded indexes" */
int kbo_set_index_shards(int shards);
/* tests: shard i of a sharded index - an ordinary index over its part of the input (n_kmers = its own), BORROWED: it lives as
 * long as `idx` and must not be freed.  An ordinary index is its own shard 0.  NULL when i is out of range. */
const kbo_index_t *kbo_index_shard(const kbo_index_t *idx, int i);
/* The depth table of device copies made after the call (kbo_amd/csrc/dtab_kernels.hip): for every string of `order` bases the
 * longest suffix of it that is a suffix of a row of the index, 4^order bytes of device memory.  With it, the stretches behind
 * a read's mismatches against the plan's diagonal - where the matching statistic is the length of a random match, about
 * log4(rows) - cost one independent byte look-up per base instead of a chain of dependent rank look-ups; values deeper than
 * `order` send their read to the plain walk.  0 = by index size (log4(rows) + 3.2 rounded up, at most 17 and k; none from
 * about 1.2 * 10^9 rows on - 17 bases are then too few - or when it would take more than half of the free device memory),
 * 1 .. 17 = that order (capped at k),
 * < 0 = none: new copies get no table and launches over copies that have one do not use it (until the knob is >= 0 again).
 * Results are identical with and without it. */
int kbo_set_depth_table(int order);
/* ... with ANCHORS (device copies made after the call): a hash of the strings of `order` bases that are the suffix of exactly
 * one row, with that row's place in the path cover; a base deeper than the table knows is then read off the path-cover text
 * (by a kernel of its own behind the plan kernel) instead of sending its read to the plain walk; a quarter of those reads
 * remain.  Measured: slower at C2 (the redo pass is bound by its longest chain, not by its size), 4 % faster at C3.
 * -1 = on indexes of 24 Mi rows and more whose table's margin over log4(rows) is below 3.75 bases (default: there the reads left to the plain walk are many
 * enough for it to pay - C4 +12 %, C3 +4 % - and from 3 * 10^8 rows on the table only wins with them), 0 = never, 1 = always. */
int kbo_set_depth_table_anchors(int mode);
/* bytes the seed + depth tables of a device copy may take while they are built (device copies made after the call): 0 = half of the
 * device memory that is free at that moment (default).  A table that does not fit is degraded - grouped layout -> plain layout
 * (a quarter of the bytes) -> fewer bases -> none (the copy then gets the host-built seed table and the guided walk) - never an
 * error, also when its order was forced with kbo_set_depth_table. */
int kbo_set_plan_table_budget(uint64_t bytes);
/* When a device copy makes its plan structures (path cover, recovery lines, seed and depth tables, 2-bit text): kbo_index_to_device
 * makes them at once; a copy made implicitly by a first query makes them once the batches that went through it add up to `bases`
 * bases - until then MS-only batches take the plain walk, with the same results.  -1 = by index size (default): at once when they
 * cost under a tenth of a second (up to ~ 1.5 * 10^6 rows), else after the bases whose saving pays for them (65 ns per row without
 * a stored path cover, 15 ns with one, against 7 ps saved per base: ~ 50 Gbp for a 5 Mbp index); 0 = always at once. */
int kbo_set_plan_lazy(int64_t bases);
/* inspection / tests: the depth table of the copy of `idx` on `device` (-1 = current; the copy is made if there is none):
 * *order bases per entry (0: the copy has no table), 4^*order bytes; entry of a string (2-bit digits A, C, G, T = 0 .. 3, the
 * last base least significant) = length of its longest suffix that is a suffix of a row of the index, or 0x80 | e when the
 * whole string is, bit c of e set when the string with base c in front of it is one too.  On the device the entries of
 * three consecutive bases of a read share a 64-byte line, so every entry is there three times; `view` (0 .. 2) says which
 * copy to hand back, in key order (ignored for tables too small to be grouped).  table == NULL only asks for *n_bytes and
 * *order; tables of more than 14 bases are not handed back (KBO_E_UNSUPPORTED). */
int kbo_index_depth_table(kbo_index_t *idx, int device, int view, uint8_t *table, size_t *n_bytes, int *order);
/* inspection / tests: one of the plan structures that the copy of `idx` on `device` (-1 = current; the copy and its plan
 * structures are made if there are none: as kbo_index_depth_table) built for itself on the device, handed back byte for byte as
 * it lies there - a plain download under the handle's lock; nothing on the device changes and no kernel runs.
 * out == NULL only asks for *n_bytes and info; a part the copy does not have gives 0 bytes, info all zero and KBO_OK (no depth
 * table: everything but a host-built seed table; KBO_SUBST_BITS=0, a default threshold below the table's order or an index without
 * a k-mer: no sub_clean).  KBO_E_BAD_ARG: a NULL idx / n_bytes / info, a part outside 0 .. KBO_PLAN_PARTS - 1, a buffer of fewer
 * than the part's bytes; a sharded index is refused as by the other hooks that need the rows of one index.
 * With U = info[0] units of 16 text positions (unit u = positions [16 u - 192, + 16) of the path-cover text):
 *   PC_TM     U x { digits, marks } (kbo_amd/csrc/map_text.hpp), 8 U bytes                      info = { U, cell shift }
 *   PC_T      U digit words and the 16 bytes of slack a window's last load may read              info = { U, cell shift }
 *   PC_MU     a bit per unit, whole workgroups of 256 units, and the 4 bytes of slack behind     info = { U, cell shift }
 *   PC_MC     2048 bits, a cell of 2^shift units each                                            info = { U, cell shift }
 *   SEED_TAB  { l, r } per string of seed_d bases, 8 * 4^seed_d bytes           info = { seed_d, 1 if built on the device else 0 }
 *   SEED_POS  a text position per string of seed_d bases, 4 * 4^seed_d bytes    info = { seed_d, as SEED_TAB }
 *   DFILT     a bit per string of F bases, 4^F / 8 bytes                        info = { F, order of the depth table }
 *   ANCHOR    2^bits slots of { text position, (uint32_t)key + 1 }, 8 bytes     info = { bits, order of the depth table }
 *   SUB_CLEAN a bit per text position (kbo_amd/csrc/map_subst.hpp), 4 * ((U + 1) / 2) bytes
 *                                                      info = { U, order of the depth table, threshold, 1 with anchors else 0 }
 *   SUB_GROUP a bit per group of 4 text positions, set where all four of SUB_CLEAN's are (bit G of the array: positions 4 G .. 4 G + 3,
 *             counted as SUB_CLEAN counts them), 4 * ((U + 7) / 8) bytes and the 64 zeroed bytes of slack a window's one 8-byte load may read;
 *             there when SUB_CLEAN is, unless the copy was made under KBO_SUBST_GROUPS=0
 *                                  info = as SUB_CLEAN */
#define KBO_PLAN_PART_PC_TM 0
#define KBO_PLAN_PART_PC_T 1
#define KBO_PLAN_PART_PC_MU 2
#define KBO_PLAN_PART_PC_MC 3
#define KBO_PLAN_PART_SEED_TAB 4
#define KBO_PLAN_PART_SEED_POS 5
#define KBO_PLAN_PART_DFILT 6
#define KBO_PLAN_PART_ANCHOR 7
#define KBO_PLAN_PART_SUB_CLEAN 8
#define KBO_PLAN_PART_SUB_GROUP 9
#define KBO_PLAN_PARTS 10
int kbo_index_plan_part(kbo_index_t *idx, int device, int part, void *out, size_t *n_bytes, uint32_t info[4]);
/* tests: depth of the seed table of device copies made after the call (0 = by index size: 8 / 10 / 12 / 13 bases;
 * 1 .. 13 = that many, capped at k).  Large tables are what large indexes get: 12 bases = 128 MiB, 13 = 512 MiB. */
int kbo_set_seed_table_depth(int bases);

/* ------------------------------------------------------------------ the plan-guided walk */
/* Device copies made while it is enabled (default) carry a path cover of the index's de Bruijn graph (9 B per row) and
 * kbo_ms_batch[_dev] / kbo_matches_batch / kbo_map_batch / kbo_find_batch skip the stretches of every read that match it;
 * results are identical either way.  enabled < 0 keeps the setting, > 0 also clears every copy's hold-off; seed_depth
 * (> 0: fixed; < 0: automatic = log4(rows) + 3, the default; 0 keeps) and seed_cap (default 64 = the most; <= 0 keeps)
 * tune the diagonal search. */
int kbo_set_plan(int enabled, int seed_depth, int seed_cap);
/* (0 keeps a value) mismatches closer than `gap` bases (>= 2; < 0: automatic = log4(rows) + 9, the default: 20 on a
 * 5 Mbp index, 22 on 100 Mbp) are walked by one unit; reads without a diagonal are walked in chunks of `chunk` bases
 * (default 32); a launch with more than bail_x16 / 16 units per read (default 50 / 16: the break-even is near 4 %
 * substitutions) gives the plan up and takes the plain walk, and the following 16 launches over that device copy of that
 * index do not plan at all.  bail_x16 = 0 forces that path (tests), < 0 keeps. */
int kbo_set_plan_tuning(int gap, int chunk, int bail_x16);
/* tests: the unit array of a launch gets 1 / divisor of its normal capacity (reads whose units do not fit take the plain
 * walk); 1 = normal */
int kbo_set_plan_unit_cap_divisor(int divisor);
/* inspection / tests: launches over the copy of `idx` on `device` (-1 = current) that gave the plan up so far, and the
 * launches the copy will still skip planning for; either pointer may be NULL.  KBO_E_BAD_ARG when no such copy exists. */
int kbo_index_plan_holdoff(kbo_index_t *idx, int device, uint32_t *bails, int *holdoff);

/* instrumentation (default off): launches of the plan-guided stage made while it is on count their own work - per-lane adds
 * in the walk's hot loop, one atomic per counter and wave at exit: about 1 % of the stage's time, which is why the default
 * instantiations of the kernels carry none of it */
int kbo_set_plan_stats(int on);
/* inspection: the work counters the plan-guided stage kept about its last launch over a device-resident batch (made with
 * kbo_set_plan_stats(1)) - what
 * the CPU model of the stage (oracle/plan_model.c), whose counts bench.py's roofline prices the stage by, is pinned to
 * (tests/test_gpu_model.py).  Arguments as for the kbo_ms_batch_dev call that ran on d_work; synchronises `stream`.
 * out[0..7]: units walked, accepted extensions, failed extensions, contraction levels, levels taken from the entries
 * (recovery-line form), seed-table look-ups, seed extensions, mismatches against the diagonals;  out[8]: units emitted,
 * [9]: entries of the redo list, [10]: 1 = the plan was given up, [11]: 1 = a walk left through its guard;  depth-table form
 * (kbo_set_depth_table) out[12]: table look-ups, [13]: values written from the table, [14] = [15]: items the table could not
 * resolve (counted by the lanes / by the launch's control word; out[8] is meaningless in that form), [16]: bases read off the
 * path-cover text (anchors), [17]: items resolved without a plan;  map_reads_kernel's direct form (kbo_map_batch_dev) [18]:
 * lone substitutions asked of the copy's bit per text position (a word each, but for those of [20]), [19]: mismatches those bits settled without a
 * filter word or a table byte (out[6] and out[12] count the filter words and table bytes actually looked up), [20]: those of [18]
 * and [19] alike that the read's own lane settled by its window of clean groups, before anything was dealt or looked up.  Meaningless
 * (stale or zero) when that launch did not plan (plain walk, hold-off, intervals requested) or did not count. */
#define KBO_PLAN_STATS 21
int kbo_plan_stats_dev(size_t n_seqs, uint64_t total_bases, size_t max_seq_len, uint32_t k, const void *d_work,
                       uint64_t out[KBO_PLAN_STATS], void *stream);

/* inspection: which reads the last planned launch over a device-resident batch of READS (kbo_ms_batch_dev, kbo_map_batch_dev: one
 * item per sequence) left to the plain walk - flags_out[s] != 0 - read out of the launch's work buffer.  Arguments as for that call;
 * synchronises `stream`. */
int kbo_plan_flags_dev(size_t n_seqs, uint64_t total_bases, size_t max_seq_len, uint32_t k, const void *d_work, uint8_t *flags_out, void *stream);
/* the kernel for sequences of more than 160 bases (long_kernels.hip: one wave per piece of a sequence): 0 = never (such batches
 * take the walk + the derandomize / translate kernels), 1 = wherever the index copy has what it needs (default), 2 = as 1 with
 * EVERY piece sent to its second pass (plain walk + literal recurrences) - a test hook, exact like the others. */
int kbo_set_map_long(int mode);
/* kbo_ms_batch_dev over a batch of reads (<= 160 bases, no intervals) and a copy with a depth table: 1 (default) = map_reads_kernel in its
 * MS-emitting form, stopped behind the values; 0 = the plan-guided walk as for every other batch (also taken while kbo_set_plan_stats is
 * on: the work counters are that walk's). */
int kbo_set_ms_one_kernel(int on);
/* kbo_call_batch[_flat]: 1 (default) = the variants are put in order, resolved and sliced on the device (call_emit_kernels.hip: two slots
 * on two streams, ten bytes per variant over PCIe); 0 = rounds 3 - 5's route for every slab (a record + a window per site to the host,
 * host threads sort, resolve and slice) - what the default falls back to for a slab it cannot finish; 2 = as 1, but the second pass's
 * depths for k <= 64 by the kernel that serves k > 64 (call_second_kernels.hip: every lane extends its own matches); same results (tests). */
int kbo_set_call_device_emit(int on);
/* inspection: what the last kbo_map_batch_dev / kbo_find_batch_dev call over sequences of more than 160 bases did when it took
 * the one kernel for sequences of any length (long_kernels.hip); arguments as for that call, synchronises `stream`.
 * out[0]: pieces, [1]: pieces whose proof failed (plain walk + literal recurrences), [2]: their sub-items; with kbo_set_plan_stats(1) [3]: seed look-ups,
 * [4]: filter look-ups, [5]: depth-table look-ups, [6]: of those, second look-ups behind a window that was present;
 * [8..12] (experiments, KBO_LONG_X & 128): shader cycles of the waves' first lanes by phase - staging, stretches, planes to
 * characters, proof, output; [13], [14] (kbo_set_plan_stats): pieces that tried all their words on a band of diagonals at once /
 * that kept the result; [16..24] (kbo_set_plan_stats): flagged pieces by what flagged them - other, list too long, a window one base
 * on present and extended, the window one base back, the one inside the next stretch; [21..24]: the last four after the band pass. */
#define KBO_LONG_STATS 25
int kbo_long_stats_dev(size_t n_seqs, uint64_t total_bases, size_t max_seq_len, uint32_t k, const void *d_work, uint64_t out[KBO_LONG_STATS],
                       void *stream);

/* instrumentation (default off): while on, every kbo_map_batch_dev call that takes the one-kernel route records HIP events on its
 * stream around map_reads_kernel and behind the redo pass (three event records per call).  kbo_stage_timing_read waits for the
 * recorded calls, returns their number and the sums of the two intervals in milliseconds - the kernel itself / the reads it left
 * to the plain walk (list, walk, their derandomize + translate) - and forgets them.  bench.py prices its roofline by the first.
 * on > 1: on, and the events of that many calls are made now instead of inside the first calls that record them. */
int kbo_set_stage_timing(int on);
int kbo_stage_timing_read(double *kernel_ms_sum, double *redo_ms_sum, int *n_calls);

/* test hook: what kbo_call_batch answers the reference-side walks of its sites with (variant_calling.rs:280: the matched
 * row's k-mer against the index the reference builds of the sequence itself, lib.rs:553) - the depths of the walk of each
 * of n_kmers k-mers (k bytes each, back to back) against the SBWT of `seq` built with (k, add_revcomp), computed from a
 * suffix automaton of the sequence's ACGT-runs of at least k characters instead of that index.  Host only (no GPU).
 * depths_out: n_kmers * k values.  tests/test_capi_host.py compares them with the oracle's walk of a real one-sequence index. */
int kbo_run_automaton_depths(const uint8_t *seq, size_t len, uint32_t k, int add_revcomp, const uint8_t *kmers,
                             size_t n_kmers, uint32_t *depths_out);

/* test hook: what the calling thread's last kbo_fill_gaps_batch / kbo_map_batch_opts did with the gaps: out[0] gaps found,
 * out[1] gaps finished on the device (gap_kernels.hip), out[2] sequences redone whole on the host (kbo::fill_gaps), out[3]
 * left-extension steps taken on the device. */
int kbo_fill_gaps_stats(uint64_t out[4]);
/* ... and where its time went, in seconds: out[0] walk, [1] translate, [2] gap kernels, [3] host fallback, [4] variant
 * calling, [5] add_variants + relative_to_ref (tools/bench_map_opts.py) */
int kbo_map_batch_opts_phases(double out[6]);
/* Test hook: where the calling thread's last kbo_index_build_device spent its time, in seconds (HIP events, [8] host clock):
 * out[0] upload, [1] extraction, [2] sort, [3] dedup, [4] orphans + dummy rows, [5] merge, [6] edge bits + LCS, [7] download of
 * the rows and LCS, [8] the device copy (layout and plan structures, as kbo_index_to_device) (tools/bench_build.py) */
int kbo_index_build_device_phases(double out[9]);
/* Test hook: bytes the calling thread's last host batch (kbo_ms_batch, kbo_matches_batch / kbo_map_batch / kbo_find_batch, their
 * packed and *_strands forms) copied from the host to the device: bases or words, exception lists, offsets, work items.  A batch
 * run in both strands stages what it stages for one (tests/test_gpu_strands.py) cut into the same slabs - both strands cut slabs of
 * half of kbo_set_slab_bytes, 32 KiB at least, and every slab stages one offset more than it has sequences. */
uint64_t kbo_last_batch_staged_bytes(void);
/* inspection / tests: slabs of kbo_summary_batch[_packed] since the process started, by route - records straight from map_reads_kernel's
 * summary form and its second pass (no character made), or characters on the device and the reducer over them.  Either may be NULL. */
int kbo_summary_slab_routes(uint64_t *kernel_slabs, uint64_t *reducer_slabs);
/* Test hook: the number of workgroups kbo_sparse_runs_dev launches its count and emit kernels with for these arguments (1 .. 2048;
 * max_seq_len = 0, unknown: the most; 0 for arguments it refuses) */
uint32_t kbo_sparse_runs_blocks(size_t n_seqs, size_t max_seq_len);

/* ------------------------------------------------------------------ kbo_find_refset */
/* bases a lane of refset_kernels.hip emits: a sequence is cut every max(KBO_REFSET_CHUNK, 4 k) bases, every chunk behind the first
 * restarts k - 1 bases upstream; rows of the largest index that takes that kernel (larger ones: the single-index pipeline) */
#define KBO_REFSET_CHUNK 256
#define KBO_REFSET_MAX_ROWS 16384
/* test hook: records the device buffer of a slab's runs has room for at first (default 65 536, at least 1; a slab with more runs
 * grows it - the run-length stage counts before it emits) */
int kbo_set_refset_record_capacity(size_t records);
/* test hook: what the calling thread's last kbo_find_refset did: out[0] references walked by the LDS kernel, out[1] references taken
 * through the single-index pipeline, out[2] (reference, sequence, strand) pairs walked over both routes, out[3] slabs */
int kbo_refset_last_routes(uint64_t out[4]);
/* test hook: the wide route (kbo_refset_build_wide) in the calling thread's last kbo_find_refset / kbo_summary_refset: out[0] references
 * walked by the wide kernel, out[1] the tasks (workgroups) it was launched with, over all slabs.  out[0] of kbo_refset_last_routes
 * counts the references of the LDS kernel only; its out[2], the pairs, includes the wide references' */
int kbo_refset_last_wide(uint64_t out[2]);
/* test hook: the launches of refset_best_kernel (kbo_amd/csrc/refset_best_kernels.hip) in the calling thread's last kbo_best_refset or
 * kbo_best_refset_dev, one a slab: out[0] with a wave per sequence, out[1] with a workgroup of four waves per sequence (batches of
 * fewer than 64 sequences) */
int kbo_refset_last_best(uint64_t out[2]);
/* test hook: the packed form of reference r (kernels.hpp: rank blocks, LCS bytes with the sentinel), *n_bytes of it, a multiple of
 * 16; out == NULL asks for the size only.  KBO_E_BAD_ARG for a reference with a status or of the single-index route */
int kbo_refset_form(const kbo_refset_t *set, size_t r, uint8_t *out, size_t *n_bytes);
/* test hook: the matching statistics of seq (len bytes, any values) against reference r, one depth a base, made on the CPU by the
 * step the wide kernel runs (kbo_amd/csrc/refset_step.hpp) over the set's host arena, unchunked.  No HIP call; not a fallback.
 * KBO_E_BAD_ARG as kbo_refset_form */
int kbo_refset_ms_host(const kbo_refset_t *set, size_t r, const uint8_t *seq, size_t len, uint8_t *ms_out);
/* start positions a lane of refset_screen_kernels.hip owns, lanes of its workgroups: lane boundaries lie at the multiples of
 * KBO_REFSET_SCREEN_RUN bases of the concatenated batch, workgroup boundaries at those of RUN x THREADS */
#define KBO_REFSET_SCREEN_RUN 64
#define KBO_REFSET_SCREEN_THREADS 256
/* test hook: kbo_refset_candidates restated on the CPU over the set's host table, by the seed, the shared prefix and the bucket scan
 * the kernel runs (kbo_amd/csrc/refset_screen.hpp), a sequence at a time, unchunked.  Same arguments, bitmap and errors.  No HIP
 * call; not a fallback */
int kbo_refset_candidates_host(const kbo_refset_t *set, const uint8_t *concat, const uint64_t *offsets, size_t n_seqs,
                               double max_error_prob, int strands, uint32_t *bits_out, uint64_t *n_candidates);
/* test hook: the bits of a call's bitmap (n_refs x n_seqs x 2) above which kbo_find_refset / kbo_summary_refset / kbo_best_refset on
 * a set with a prefilter run unscreened (default and most 2^31; 0 restores the default) */
int kbo_set_refset_prefilter_max_bits(uint64_t bits);
/* what the calling thread's last kbo_find_refset / kbo_summary_refset / kbo_best_refset did with the prefilter: out[0] the
 * (reference, sequence, strand) pairs of packed references, out[1] how many had their bit set (0 when the screen did not run),
 * out[2] how many were walked, out[3] 1 if the screen ran, else 0 (no prefilter, or the bitmap above the cap) */
int kbo_refset_last_prefilter(uint64_t out[4]);
/* what the calling thread's last kbo_call_refset / kbo_call_refset_host did: out[0] the (reference, sequence, strand) pairs handed to
 * the scan (the pairs walked; the host form walks every pair of a packed reference), out[1] candidate positions i, out[2] sites -
 * candidates with a match j -, out[3] variants.  The lists of a slab's candidates, sites and windows on the device have room for
 * kbo_set_refset_record_capacity records at first; a slab with more candidates is scanned again with room for its count */
int kbo_refset_last_call(uint64_t out[4]);
/* test hook: the k characters of row `row` of reference r's index ('$' in front of a row that is no full k-mer), read off the packed
 * form on the CPU by the inverse steps refset_call_kernels.hip spells a site's row with (kbo_amd/csrc/refset_call.hpp) -> out, k
 * bytes.  KBO_E_BAD_ARG as kbo_refset_form, and for a row that the reference does not have */
int kbo_refset_spell_row(const kbo_refset_t *set, size_t r, uint32_t row, uint8_t *out);
/* test hooks of the second pass the device-resident calls run (kbo_amd/csrc/refset_resolve.hpp), restated on the CPU over the same
 * arithmetic.  No HIP call; not a fallback.
 * kbo_call_refset_host_indexed: kbo_call_refset_host's pipeline with the second pass done as the device does it - the index of the
 * '+' batch, the probes, the three values, the resolve word, the order by keys - instead of an automaton per sequence.  Same
 * arguments, records, errors and counters; KBO_E_REF_PANIC for a site at which the reference would panic.
 * kbo_refset_kmer_depths_host: the depths of the k characters of `kmer` against the runs of at least k bases of seq[0, len):
 * mode 1 forwards, 2 against their reverse complements, 3 both; out[t] is the depth at t if it is at least q (1 <= q <= 12,
 * q <= k <= 255), else 0.
 * kbo_refset_resolve_word_host: resolve_variant's case analysis as the device states it, next to the host's copy
 * (resolve_variant_peaks): qpeak / rpeak 0xFF for none.  out[0] the device's word ({ q_from | q_len << 8 | r_from << 16 |
 * r_len << 24 }, 0xFFFFFFFF no variant, 0xFFFFFFFE a panic), out[1] the host's verdict (0 no variant, 1 a variant, 2 a panic),
 * out[2 .. 5] its q_from, q_to, r_from, r_to.  kbo_refset_resolve_words_check runs every (csl 0 .. k, qpeak, rpeak in none,
 * 0 .. k - 2) through both: out[0] cases, out[1] cases in which they differ, out[2] panics, out[3] variants.
 * kbo_refset_order_sites_host: the order of n sites by their keys (ref, seq, strand, i), by the radix passes the device runs over
 * the same key words: order_out[p] is the site at place p.  KBO_E_BAD_ARG for a site outside n_refs, n_seqs, strand 1 .. 2 or
 * i >= total_bases. */
int kbo_call_refset_host_indexed(const kbo_refset_t *set, const uint8_t *concat, const uint64_t *offsets, size_t n_seqs,
                                 const kbo_call_opts *opts, int strands, kbo_ref_calls *out);
int kbo_refset_kmer_depths_host(const uint8_t *seq, size_t len, uint32_t k, uint32_t q, int mode, const uint8_t *kmer, uint32_t *out);
int kbo_refset_resolve_word_host(uint32_t k, uint32_t csl, uint32_t qpeak, uint32_t rpeak, uint32_t out[6]);
int kbo_refset_resolve_words_check(uint32_t k, uint64_t out[4]);
int kbo_refset_order_sites_host(size_t n, const uint32_t *refs, const uint32_t *seqs, const uint32_t *strands, const uint32_t *is,
                                uint64_t n_refs, uint64_t n_seqs, uint64_t total_bases, uint32_t *order_out);

/* ------------------------------------------------------------------ kbo_derand_translate_seq_dev */
/* positions of a chunk and of a group (64 chunks) of derand_seq_kernels.hip; neither spans two sequences.  A sequence of more than
 * KBO_DERAND_SEQ_GROUP positions makes the lane that owns it loop over its groups */
#define KBO_DERAND_SEQ_CHUNK 128
#define KBO_DERAND_SEQ_GROUP 8192

/* ------------------------------------------------------------------ kbo_run_lengths_seq_dev */
/* positions of a chunk and of a group (64 chunks) of rle_seg_kernels.hip; neither spans two sequences.  A sequence of more than
 * KBO_RLE_SEG_GROUP positions makes the lane that owns it loop over its groups.  The library's own callers (kbo_find_batch and its
 * forms, kbo_run_lengths_gapped_batch, kbo_find_refset) do NOT take that stage yet: from which sequence length on it beats one lane
 * per sequence has to be measured first (tools/bench_rle_seg.py) */
#define KBO_RLE_SEG_CHUNK 128
#define KBO_RLE_SEG_GROUP 8192
/* test hook: count and emit calls of that stage since the process started (either pointer may be NULL) */
int kbo_run_lengths_seg_calls(uint64_t *count_calls, uint64_t *emit_calls);
/* test hook: the passes of kbo_run_lengths_seq_dev restated on the CPU over the same chunk-summary and combine functions
 * (kbo_amd/csrc/rle_seg.hpp), with chunks of `chunk` >= 1 positions and groups of `group` positions, a multiple of it; aln, offsets,
 * records (7 u32 each, `capacity` of them; more runs are counted, not written) and first (n_seqs + 1) are on the HOST.  A sequence
 * shorter than min_len has no run.  No HIP call: it runs without a GPU. */
int kbo_run_lengths_seq_host(const uint8_t *aln, const uint64_t *offsets, size_t n_seqs, size_t max_gap_len, size_t chunk, size_t group,
                             size_t min_len, uint32_t *records, size_t capacity, uint32_t *first);
/* ... with every sequence of the batch handed to it as a batch of ONE, in a buffer of exactly its own length; same outputs */
int kbo_run_lengths_seq_host_each(const uint8_t *aln, const uint64_t *offsets, size_t n_seqs, size_t max_gap_len, size_t chunk, size_t group,
                                  size_t min_len, uint32_t *records, size_t capacity, uint32_t *first);

/* ------------------------------------------------------------------ kbo_index_add_positions, kbo_segments_dev */
/* positions of a tile of locate_kernels.hip and of the halo it reads on either side (the largest bridge + 1), and the values a
 * workgroup of the three-pass scan takes; the getter returns what the kernels were compiled with (any pointer may be NULL) */
#define KBO_SEGMENTS_TILE 2048
#define KBO_SEGMENTS_HALO 256
#define KBO_SEGMENTS_MAX_BRIDGE 255
int kbo_segments_geometry(uint32_t *tile, uint32_t *halo, uint32_t *scan_chunk);
/* test hook: source bases a slab of kbo_index_add_positions adds to the table (each slab is walked with the k - 1 bases in front of
 * it); 0 = the default, 32 Mi.  Any value gives the same table. */
int kbo_set_positions_slab_bases(uint64_t bases);

/* ------------------------------------------------------------------ kbo_derand_translate_dev and the host batches' stage behind the walk */
/* test hook: the derandomize + translate stage of kbo_matches_batch / kbo_map_batch / kbo_find_batch / kbo_map_batch_opts over MS bytes
 * of the caller's making instead of a walk's.  ms (offsets[n_seqs] bytes, any values <= k), offsets (n_seqs + 1 values from 0, ascending)
 * and the optional ref (offsets[n_seqs] bytes, NULL = none: with it format::relative_to_ref is applied) are on the HOST; they are
 * uploaded into buffers of offsets[n_seqs] + 16 bytes and handed to the router the slab pipeline calls, scratch for the piece-wise kernel
 * included: sequences of up to 480 bases through the LDS kernel when none is longer, otherwise pieces up to 65 536 bases and the
 * chunk-table scan for every longer sequence.  chars_out (host, offsets[n_seqs] bytes) gets the characters; the bytes of sequences of
 * fewer than 3 bases are unspecified.  Synchronous, on the current device's default stream. */
int kbo_derand_translate_host(const uint8_t *ms, const uint64_t *offsets, size_t n_seqs, size_t k, size_t threshold, const uint8_t *ref,
                              uint8_t *chars_out);

/* ------------------------------------------------------------------ experiments recorded in DESIGN.md section 6 */
/* plain walk kernel: only the first lane_limit lanes of every wave take reads (64 = all; what a sub-wave tiling would
 * have to beat), and every workgroup reserves dummy_lds_bytes of LDS it never touches (what staging a wave's MS values
 * in LDS for a fused A5/A6 would cost in occupancy) */
int kbo_set_walk_experiment(int lane_limit, int dummy_lds_bytes);

#ifdef __cplusplus
}
#endif
#endif /* KBO_HIP_TUNING_H */
