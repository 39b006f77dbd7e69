// kernels.hpp — launch interface of the gfx950 kernels (walk_kernels.hip, derand_kernels.hip, rle_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "refset_plan.hpp"

namespace kbo {

// Device-resident index (32-bit positions).  Layout: sbwt_index.hpp.
struct DevIndexView {
    const uint4 *arena;   // one allocation: rank blocks of A,C,G,T, then the LCS windows
    uint32_t n_blocks;    // rank blocks per character (character c starts at c * n_blocks)
    uint32_t lcs_off;     // arena index (16-byte units) of contraction entry 0 (32-bit build)
    uint32_t pair_off;    // arena index (16-byte units) of the two-base extension blocks, 0 = none
    const uint8_t *ent;   // contraction entries as their own region (used when `big`)
    uint32_t big;         // 1: entries are addressed with 64-bit offsets (n_sets * 12 B >= 4 GiB)
    uint32_t n;           // n_sets
    uint32_t k;
    // path cover of the de Bruijn graph (sbwt_index.hpp PathCover), nullptr when the device copy has none:
    const uint8_t *pc_text;    // points at text position 0; kPlanPad zero bytes on either side
    const uint32_t *pc_pos;    // row -> text position
    const uint32_t *pc_node;   // text position -> row
    uint32_t C[5];             // C[c] of the index, C[4] = n_sets: extend(root, c) = [C[c], C[c+1])
    // plan_kernel's seed table: interval {l, r} of every string of seed_d bases (code = bases as 2-bit digits, first
    // base most significant), l >= r when it is no suffix of a row; nullptr / 0 when the index has none
    const uint2 *seed_tab;
    uint32_t seed_d;
    // recovery lines of the guided walk (sbwt_index.hpp make_recovery_lines), nullptr when the device copy has none
    const uint8_t *fat;
    uint32_t fat_null; // line index of an all-zero line (extensions by a non-ACGT byte)
    // depth table (dtab_kernels.hip), nullptr / 0 when the device copy has none: for every string of dtab_order bases (2-bit
    // digits, the newest base least significant) the longest suffix of it that is a suffix of a row; 0x80 | e when all of it
    // is, bit c of e = so is the string with base c in front of it
    const uint8_t *dtab;
    uint32_t dtab_order;
    uint32_t dtab_grouped; // 1: the entries of three consecutive bases share a 64-byte line (dtab_kernels.hip), 4^(order+1) bytes
    // anchors of the depth table, nullptr / 0 when there are none: open-addressing hash (2^anchor_bits slots) of the strings of
    // dtab_order bases that are the suffix of exactly ONE row: slot = (low 32 bits of key + 1) << 32 | text position of that
    // row in the path cover.  A base whose value the table cannot tell (deeper than dtab_order) is read off the path-cover
    // text in front of that position
    const uint64_t *anchor;
    uint32_t anchor_bits;
    // what map_reads_kernel (map_kernels.hip) reads instead of the byte text and the interval table, nullptr when the copy has
    // none: pc_tm[u] = { 2-bit digits of text positions [16 u - kMapPad, + 16), first one most significant; 01 at every
    // position that matches nothing (path start, padding) }; seed_pos[key of seed_d bases] = text position of the first row
    // whose k-mer ends with them, 0xFFFFFFFF when there is none
    const uint2 *pc_tm;
    const uint32_t *seed_pos;
    // the same text without its marks, which is what map_reads_kernel's common path reads (map_text.hpp): pc_t[u] = pc_tm[u].x, and
    // pc_mu = one bit per unit, set where pc_tm[u].y != 0 (and behind the last unit) - half the bytes of pc_tm and 1 / 256 of them
    // pc_mc: maptext::kCells bits, bit c set where a window that starts in cell c - 2^pc_mc_shift units - can see a marked unit
    const uint32_t *pc_t;
    const uint8_t *pc_mu;
    const uint32_t *pc_mc;
    uint32_t pc_mc_shift;
    // ... and its filter in front of the depth table (small indexes): bit [key of dfilt_bases bases] set where that string is a
    // suffix of a row - 4^dfilt_bases / 8 bytes (2 MB for 12 bases: stays in L2), nullptr when the copy has none
    const uint32_t *dfilt;
    uint32_t dfilt_bases;
    // ... and what settles a lone substitution without the table (map_subst.hpp): a bit per position of the 2-bit text (bit q of
    // word q / 32, q counted from the first unit's first position), set where no one-base neighbour of the text's windows around
    // it is in the index - for the proof's windows at threshold sub_thr with (sub_anch = 1) or without anchors.  nullptr when the
    // copy has none; launch_map_reads hands the kernel nullptr when the launch's threshold is another
    const uint32_t *sub_clean;
    uint32_t sub_thr, sub_anch;
    // ... and its coarser form: a bit per group of mapsubst::kGroup positions, set where all of the group's bits are - a read's whole
    // window of them is one 8-byte load beside the text's (any byte address; 64 zeroed bytes of slack behind the array).  There exactly
    // when sub_clean is (unless the copy was made under KBO_SUBST_GROUPS=0), nulled with it
    const uint8_t *sub_group;
};

// One unit of walk work: `len` bases starting at absolute offset `start` of the
// concatenated query buffer; the first `warm` of them only warm the state up (no
// output) — chunks of long sequences restart k-1 bases upstream.
struct alignas(16) WalkItem {
    uint64_t start;
    uint32_t len;
    uint32_t warm; // low 16 bits: warm-up bases; high 16 bits (call mode): bases at the end that are walked only to finish
                   // the search to the right of the breakpoints in front of them (they belong to the next chunk)
};

// ---- plan-guided walk (plan_kernels.hip) -------------------------------------------------------------------------
// plan_kernel finds, for every work item, a diagonal of the path-cover text (a short exact walk over the item's first
// bases to a single row u: diagonal p0 = pos[u] - j), compares the whole item with the text on that diagonal, writes the
// MS values this predicts - min(k, distance to the last mismatch) - and the list of mismatch positions.
// plan_emit_kernel turns the lists into UNITS: stretches that have to be walked, one per group of mismatches closer
// than `plan_gap`, starting on the diagonal in front of the group's first mismatch.  ms_walk_guided_kernel walks every
// unit until the walk itself proves it is back on the diagonal (a single-row interval whose depth equals the distance
// to the group's last mismatch); a unit that reaches the next group first flags its item, and flagged items are
// walked again in full by the plain kernel.  Every value that is not walked is exact: see path_cover.cpp.
constexpr uint32_t kPlanPad = 64;        // zero bytes in front of / behind the device text (== PathCover::kPad)
constexpr uint32_t kPlanList = 12;       // u16 list entries per item after the first (13 mismatch positions in all): reads
constexpr uint32_t kPlanListMax = 28;    // the same for long items (WalkArgs::plan_list); the list array is sized for it
constexpr uint32_t kPlanNone = 0xFF;     // GuidedItem::n_mm: no diagonal found, walk the item plainly
constexpr uint32_t kPlanInf = 0xFFFE;    // GuidedItem::mm0: no mismatch
struct alignas(16) GuidedItem {
    uint32_t start;   // absolute offset of the item's first base in the query buffer (< 4 GiB per launch)
    uint32_t p0;      // text position of item base 0 on the diagonal (mod 2^32)
    uint16_t len;     // bases, warm-up included
    uint16_t j_conv;  // > 0: the item's first j_conv bases match the diagonal and were walked exactly by plan_kernel
    uint16_t mm0;     // first mismatch position (kPlanInf: none)
    uint8_t warm;     // leading bases without output
    uint8_t n_mm;     // kPlanNone, or min(mismatches, 254); more than plan_list + 1: the list is incomplete
};
enum : uint32_t { kUnitHead = 1u, kUnitPlain = 2u, kUnitToEnd = 4u };
struct alignas(16) WalkUnit { // 32 bytes
    uint32_t start;    // as GuidedItem
    uint32_t p0;
    uint16_t pos;      // first base the unit walks (item-relative)
    uint16_t out_from; // first base it writes
    int16_t last_mm;   // last mismatch of its group (-1: none, head of an item without early mismatches)
    uint16_t bound;    // one past the last base it may walk: the next group's first mismatch, or the item's length
    uint8_t d_start;   // depth of the walk in front of `pos` (units that start on the diagonal)
    uint8_t flags;     // kUnitHead: starts at the root; kUnitPlain: no convergence test (chunk of an item without a
                       // plan: k-1 warm-up bases from the root); kUnitToEnd: bound is the item's end
    uint8_t warm;      // as GuidedItem (positions of the output words)
    uint8_t pad0;
    uint32_t item;     // work item it belongs to (for the redo flag)
    uint32_t lim_len;  // (call mode) bases of the item that are its own (the rest belong to the next chunk) | length << 16
    uint32_t pad1;
};

struct WalkArgs {
    DevIndexView ix;
    const uint8_t *q;      // concatenated queries (ASCII), 4-byte aligned
    uint64_t q_bytes;      // total bytes in q
    const WalkItem *items; // n_items
    uint32_t n_items;
    uint32_t rounds;       // items per lane (set by launch_ms_walk)
    uint32_t rare_period;  // hot-loop iterations between two visits of the rare block (set by launch_ms_walk)
    uint32_t pair_min_d;   // two-base steps only from matches at least this deep (set by launch_ms_walk)
    uint32_t lane_limit;   // plain kernel: lanes from this one on get no items (64 = all work; experiments)
    uint8_t *d_out;        // 1 byte per base, same indexing as q
    uint32_t *lo_out;      // optional (nullptr): interval start per base
    uint32_t *hi_out;      // optional: interval end per base
    // plan-guided walk (all or none): work buffers sized by plan_work_bytes(), see attach_plan()
    GuidedItem *gitems;    // nullptr: plain walk
    uint16_t *glist;       // plan_list entries per item
    uint32_t *ucount;      // units per item, heavy ones then light ones (2 n_items + 1 entries), scanned in place
    uint32_t *usums;       // block sums of that scan
    uint8_t *redo;         // per item: 1 = a unit could not vouch for its successor, walk the item again in full
    WalkUnit *units;       // unit_cap records (items whose units do not fit are flagged for the full walk instead)
    uint32_t unit_cap;
    uint32_t redo_cap;     // WalkItem records the unit array holds (the redo pass's list is built there)
    uint32_t unit_bail;    // more units than this in a launch: the plan is given up, every item takes the plain walk
    uint32_t *qctl;        // [0] queue head of the guided walk, [1] entries of the redo list, [2] plan given up, [3] a walk left through its guard,
                           // [4] (table mode) items the table could not resolve, [5] items without a plan, [6] entries of map_reads_kernel's list of the reads it left (finish_reads_kernel)
    uint32_t *pstats;      // work counters of the launch (kPlanStat*): kPlanStatSlots slots of kPlanStatWords u32, summed by the host
    uint32_t plan_dmin;    // plan_kernel: a seed must be this deep (capped at k) before its row is trusted
    uint32_t plan_cap;     // plan_kernel: seed iterations before an item is given up as unplanned
    uint32_t plan_gap;     // plan_emit_kernel: mismatches closer than this share a unit (>= 2)
    uint32_t plan_chunk;   // plan_emit_kernel: bases per unit of an item without a plan
    uint32_t plan_list;    // mismatch-list entries per item (kPlanList or kPlanListMax, set by launch_plan)
    // call mode of the plain kernel (all or none; call_kernels.hip has the stand-alone scan): the breakpoint scan of
    // call_variants (variant_calling.rs:268-273) done by the walking lane itself, sites {first base of the item + i, .. + j,
    // row, 0} appended to kCallSegs lists of call_cap records each (counters 64 bytes apart)
    uint4 *call_sites;
    uint32_t *call_counts;
    uint32_t call_cap;     // records per list
    uint32_t call_thr;     // derandomisation threshold t of the predicate
    uint32_t table_mode;   // 1: the stretches behind mismatches come from the depth table (set by launch_ms_walk)
    uint32_t table_fused;  // 1: plan_kernel did the table look-ups itself (reads; set by launch_plan_table)
    uint32_t redo_piece;   // table mode: output bases per piece of a flagged item in the redo pass
    uint32_t max_item_len; // 0 = not known, else no item is longer than this (plan_kernel sizes its LDS staging from it)
    const uint32_t *n_items_dev; // plain kernel: nullptr, or where the number of items is (the redo pass: qctl + 1)
    // map_reads_kernel (map_kernels.hip): where the characters go, the derandomisation threshold, 1 = format::relative_to_ref
    // on the way out, 1 = the MS values go to d_out as well
    uint8_t *chars_out;
    uint32_t map_thr, map_fmt, map_want_ms;
    // ... its packed-native instantiations (pack_kernels.hip has the layout): the reads as 2-bit words - qp_wps words per read, or
    // 0 and the scanned words-per-read (qp_data / qp_sums) -, one byte per read that is non-zero where the read holds a byte that
    // is no base (nullptr: none does), and, when the characters leave packed as well, where their words go
    uint32_t *host_bailed;   // (map_reads_kernel's route: pinned host word redo_collect_kernel sets when the plan is given up - the copy's
                             // hold-off, DevCopy::PlanState::bailed - instead of an 8-byte copy behind every launch)
    uint32_t *run_counts;    // (kbo::find with max_gap_len == 0: the number of runs - maximal stretches without '-' - of every read the
                             // kernel finishes itself, or nullptr: format::run_lengths_gapped then needs no counting pass of its own)
    const uint64_t *seq_off; // (reads: the batch's offsets instead of the item list - item s is sequence s, whole: the list is then
                             // only made for the second pass)
    uint32_t uniform_len;    // (... and when every sequence has max_item_len bases - n_items * max_item_len == q_bytes says so without
                             // looking at an offset - read s starts at seq_off[0] + s * uniform_len: one dependent load less per wave)
    const uint32_t *qp;
    uint32_t qp_wps;
    const uint32_t *qp_data, *qp_sums;
    const uint8_t *qp_exc;
    uint32_t *packed_out;
    uint4 *summary_out;      // (the summary forms of map_reads_kernel / finish_reads_kernel, launch_map_reads with summary = true: one record
                             // { 'M's, 'X's, 'R's, runs } per read instead of its characters - kbo_hip.h kbo_aln_summary; chars_out and d_out are null)
};
// Work counters the plan-guided stage keeps about itself (one wave-level atomic per counter and wave, spread over slots):
// what the CPU model of the stage (oracle/plan_model.c) is pinned to, tests/test_gpu_model.py
enum : uint32_t { kPlanStatUnits = 0, kPlanStatAccepted, kPlanStatFailed, kPlanStatLevels, kPlanStatEntryLevels,
                  kPlanStatSeedLookups, kPlanStatSeedExtensions, kPlanStatMismatches,
                  kPlanStatTabLookups, kPlanStatTabWritten, kPlanStatTabFlagged, kPlanStatTabAnchored,
                  kPlanStatSubstBits, kPlanStatSubstClean, // (map_reads_kernel: eligible lone substitutions asked, those settled - by a word of sub_clean or in the owner lane)
                  kPlanStatSubstGroups,                    // (... of which the owner lane settled by its window of sub_group, before stage 3 deals)
                  kPlanStatWords };
constexpr uint32_t kPlanStatSlots = 8;
// where the pieces of a launch's plan work live inside its work buffer (attach_plan)
struct PlanLayout {
    size_t gitems, units, glist, ucount, usums, qctl, pstats, redo, end;
    uint32_t unit_cap;
};
// capacity of the unit array and bytes of plan work for a launch of n_items items over total_bases bases
inline size_t plan_unit_cap(size_t n_items, uint64_t total_bases) { return 3 * n_items + total_bases / 64 + 64; }
inline PlanLayout plan_layout(size_t n_items, uint64_t total_bases)
{
    PlanLayout L;
    size_t w = 0;
    L.gitems = w;
    w += n_items * sizeof(GuidedItem);
    L.unit_cap = (uint32_t)(plan_unit_cap(n_items, total_bases) < 0x7FFFFF00ull ? plan_unit_cap(n_items, total_bases) : 0x7FFFFF00ull);
    L.units = w;
    w += (size_t)L.unit_cap * sizeof(WalkUnit);
    L.glist = w;
    w += (n_items * kPlanListMax * 2 + 15) / 16 * 16;
    L.ucount = w;
    w += (2 * n_items + 1) * 4;
    L.usums = w;
    w += (n_items / 512 + 4) * 4;
    w = (w + 15) / 16 * 16;
    L.qctl = w;
    w += 64;
    L.pstats = w;
    w += kPlanStatSlots * kPlanStatWords * 4;
    L.redo = w;
    w += (n_items + 15) / 16 * 16;
    L.end = w;
    return L;
}
inline size_t plan_work_bytes(size_t n_items, uint64_t total_bases) { return plan_layout(n_items, total_bases).end + 64; }
hipError_t launch_plan(WalkArgs &a, hipStream_t stream); // fills in the plan parameters of `a` (the later launches need them)
hipError_t launch_ms_walk_guided(WalkArgs a, uint32_t grid, uint32_t threads, hipStream_t stream);
// table mode: plan_kernel, then the stretches behind the mismatches from the depth table, then the list of the items the table
// could not resolve (for the plain kernel, like the guided walk's redo pass)
hipError_t launch_plan_table(WalkArgs &a, hipStream_t stream);
hipError_t launch_dtab_resolve(const WalkArgs &a, hipStream_t stream);
// ---- kbo::map / matches for a batch of reads in one launch (map_kernels.hip)
// the 2-bit text with its path-start marks from the padded byte text (n_bytes = kPlanPad + n_sets + kPlanPad), n_units of
// 16 positions; the text positions of the seed table's intervals
// (d_t: n_units words; d_mu: pack_text_mu_bytes(n_units) bytes, all of them written, and 4 bytes behind them readable; d_mc:
// maptext::kCells bits, cells of 2^maptext::cell_shift(n_units) units)
hipError_t launch_pack_text(const uint8_t *d_text_padded, uint64_t n_bytes, uint2 *d_out, uint32_t *d_t, uint32_t *d_mu, uint32_t *d_mc, uint64_t n_units,
                            hipStream_t stream);
// (a read's diagonal may start up to 160 bases in front of the text - it is seeded from its last bases too - and end 176 behind it)
constexpr uint32_t kMapPad = 192;
inline uint64_t pack_text_units(uint64_t n_sets) { return (n_sets + kMapPad + 256u) / 16u + 2u; }
inline uint64_t pack_text_mu_bytes(uint64_t n_units) { return (n_units + 255u) / 256u * 32u; } // (a bit per unit, whole workgroups of pack_text_kernel)
// the bit per text position of map_subst.hpp from the copy's own text and depth table (ix.pc_tm, ix.pc_t, ix.dtab), for the proof's
// windows at threshold thr: d_bits gets mapsubst::bitmap_words(n_units) words
// d_groups (may be nullptr: none): the clean groups of those bits, mapsubst::group_words(n_units) words, made from the bits just written
hipError_t launch_subst_bits(const DevIndexView &ix, uint64_t n_units, uint32_t thr, bool have_anch, uint32_t *d_bits, uint32_t *d_groups, hipStream_t stream);
hipError_t launch_seed_pos(const uint2 *d_seed_tab, const uint32_t *d_pc_pos, uint32_t *d_out, uint32_t seed_d, hipStream_t stream);
// true when the launch described by `a` (plan work attached, chars_out set) can take map_reads_kernel: reads of at most 160
// bases, MS values / characters only, an index copy with a depth table, the 2-bit text and the position table
bool map_reads_applies(const WalkArgs &a);
// the kernel; the reads it could not finish are flagged in a.redo (launch_redo_pass walks them, launch_derand_flagged
// translates them)
hipError_t launch_map_reads(WalkArgs &a, hipStream_t stream);
bool map_reads_finish_applies(const WalkArgs &a);
hipError_t launch_map_reads_finish(const WalkArgs &a, hipStream_t stream, bool one_wave_groups = false);
bool map_reads_direct(const WalkArgs &a);
bool map_reads_summary_applies(const DevIndexView &ix, uint32_t longest); // (a.summary_out: launch_map_reads + launch_map_reads_finish store records, no characters)
bool map_reads_packed_applies(const WalkArgs &a, bool packed_out); // (a.qp set: the reads as 2-bit words; a.packed_out: the characters too)
// packed-native batches (pack_kernels.hip): exc[s] = 1 for every read that holds a listed byte (d_exc zeroed first); the bytes of the
// flagged reads from their words (for the plain walk; the listed bytes then go over them: launch_exceptions); the characters of
// the flagged reads into their words
hipError_t launch_flag_exceptions(const uint64_t *d_pos, uint32_t n, uint64_t base, const uint64_t *d_off, uint32_t n_seqs, uint8_t *d_exc, hipStream_t stream);
hipError_t launch_unpack_flagged(const uint32_t *d_packed, const uint64_t *d_off, uint32_t n_seqs, uint32_t uniform_wps, const uint32_t *d_scratch,
                                 const uint8_t *d_flags, uint8_t *d_q, hipStream_t stream);
hipError_t launch_pack_flagged(const uint8_t *d_chars, const uint64_t *d_off, uint32_t n_seqs, uint32_t uniform_wps, const uint32_t *d_scratch,
                               const uint8_t *d_flags, uint32_t *d_packed, hipStream_t stream);
// the list of the flagged items (redo_collect_kernel) and their plain walk; `a` as the plan launch left it
hipError_t launch_redo_pass(WalkArgs a, hipStream_t stream);
// A5 + A6 (+ relative_to_ref) for the sequences with flags[s] != 0 only, one lane each; d_run_counts (unformatted characters only):
// the number of runs of each of those sequences for format::run_lengths_gapped with max_gap_len = 0, next to map_reads_kernel's own
hipError_t launch_derand_flagged(const uint8_t *d_ms, const uint64_t *d_offsets, uint32_t n_seqs, uint32_t k, uint32_t threshold,
                                 const uint8_t *d_ref, uint8_t *d_chars_out, const uint8_t *d_flags, uint32_t max_seq_len, hipStream_t stream,
                                 uint32_t *d_run_counts = nullptr);
// stretches the fused plan_kernel leaves to the anchors: one block per plan_kernel wave in the unit array (free in table mode
// until redo_collect_kernel builds its list there): {count, pad[3]} + kDtabStretchCap entries {item, start, m | next << 16,
// len | warm << 16}; a wave with more of them flags the items of the rest
constexpr uint32_t kDtabStretchCap = 96, kDtabStretchBlockBytes = 16u + kDtabStretchCap * 16u;
hipError_t launch_dtab_stretches(const WalkArgs &a, uint32_t n_waves, hipStream_t stream);
// the depth table of `order` bases (<= 17, <= k) of the index behind `ix`: 4^order bytes at d_tab; d_tmp: dtab_tmp_bytes(cap)
// with cap >= n rows + 1.  Synchronous.
size_t dtab_tmp_bytes(uint64_t frontier_cap);
inline size_t dtab_bytes(uint32_t order, bool grouped) { return grouped ? (size_t)64 << (2u * (order - 2u)) : (size_t)1 << (2u * order); }
hipError_t regroup_depth_table(const uint8_t *d_plain, uint32_t order, uint8_t *d_grouped, hipStream_t stream);
hipError_t build_depth_table(const DevIndexView &ix, uint32_t order, uint8_t *d_tab, void *d_tmp, uint64_t frontier_cap, hipStream_t stream,
                             uint64_t *d_anchor = nullptr, uint32_t anchor_bits = 0 /* ix.pc_pos must be set when d_anchor is */,
                             uint2 *d_seed = nullptr, uint32_t seed_d = 0 /* <= order: plan_kernel's seed table ({l, r} per string) */,
                             uint32_t *d_filter = nullptr, uint32_t filter_bases = 0 /* < order: one bit per string of that many bases,
                             set where it is a suffix of a row (4^filter_bases / 8 bytes) */);
// slots (log2) of the anchor hash of an index of n rows and a table of `order` bases: twice the strings it can hold
inline uint32_t dtab_anchor_bits(uint64_t n_rows, uint32_t order)
{
    const uint64_t most = order >= 16u ? n_rows : (n_rows < ((uint64_t)1 << (2u * order)) ? n_rows : (uint64_t)1 << (2u * order));
    uint32_t b = 4;
    while (((uint64_t)1 << b) < 2 * most + 16) b++;
    return b;
}
void set_guided_walk(int waves_per_cu, int recovery_lines); // tuning: see kbo_set_guided_walk
bool guided_uses_recovery_lines(const WalkArgs &a);
void set_plan_stage(int on); // experiments: plan_kernel with (default) / without its LDS staging
void set_plan_bail(int units_per_16_items); // tuning: launches with more units than this per 16 items give the plan up
void set_plan_params(int dmin, int cap, int gap = 0, int chunk = 0); // tuning (<= 0 keeps): seed depth / seed iterations, unit gap / chunk

// offsets (n_seqs+1) -> one item per sequence
hipError_t launch_make_items(const uint64_t *d_offsets, uint32_t n_seqs, WalkItem *d_items,
                             hipStream_t stream);
// offsets -> items of at most `chunk` emitted bases (+ k-1 warm-up bases; call mode: `chunk` a multiple of 4, else
// hipErrorInvalidValue: see the launcher), n_slots >= total/chunk + n_seqs item
// slots are written (unused ones as empty items); d_scratch: chunk_items_scratch_words(n_seqs) u32
size_t chunk_items_scratch_words(uint32_t n_seqs);
hipError_t launch_make_chunk_items(const uint64_t *d_offsets, uint32_t n_seqs, uint32_t chunk, uint32_t k,
                                   uint32_t n_slots, WalkItem *d_items, uint32_t *d_scratch, hipStream_t stream,
                                   bool call = false /* items for the call mode of the walk */);
// format::run_lengths_gapped over a batch of translated sequences (see rle_kernels.hip); records are 7 u32
// {start, end, matches, mismatches, jumps, gap_bases, gap_opens}; after launch_rle_count the first-run index of
// sequence s is d_scratch[n_seqs + 1 + s / 1024] + d_scratch[s] and *d_total the number of runs
hipError_t launch_rle_count(const uint8_t *d_chars, const uint64_t *d_offsets, uint32_t n_seqs, uint32_t max_gap_len,
                            uint32_t *d_scratch, uint32_t *d_total, hipStream_t stream, uint32_t max_seq_len = 0,
                            bool own_alphabet = false /* the characters are translate_ms_vec's own, unformatted: M - X R and nothing else */);
hipError_t launch_rle_scan_counts(uint32_t n_seqs, uint32_t *d_scratch, uint32_t *d_total, hipStream_t stream);
hipError_t launch_rle_emit(const uint8_t *d_chars, const uint64_t *d_offsets, uint32_t n_seqs, uint32_t max_gap_len,
                           uint32_t *d_scratch, uint32_t *d_rles, uint32_t capacity, hipStream_t stream,
                           uint32_t max_seq_len = 0 /* longest sequence if known: reads take the LDS-staged kernels */,
                           bool own_alphabet = false);
// The same stage segmented, for sequences of any length (rle_seg_kernels.hip): chunks and groups listed on the device, two carries
// along the chunks of a sequence, no lane over more than a chunk of characters.  The same records in the same order.  Count: 17
// launches, d_first[s] = index of sequence s's first run, d_first[n_seqs] = all runs (a plain prefix).  Emit: one launch over what
// the count left in d_work.  A sequence shorter than min_len has no run.  d_work >= rle_seg_work_bytes(), 16-byte aligned;
// n_seqs < 2^28, total_bases <= 2^32 - 16.
constexpr uint32_t kRleSegChunk = 128;      // positions per chunk (== KBO_RLE_SEG_CHUNK)
constexpr uint32_t kRleSegGroupChunks = 64; // chunks per group: KBO_RLE_SEG_GROUP = 8192 positions
size_t rle_seg_work_bytes(uint32_t n_seqs, uint64_t total_bases);
hipError_t launch_rle_seg_count(const uint8_t *d_chars, const uint64_t *d_offsets, uint32_t n_seqs, uint64_t total_bases, uint32_t max_gap_len,
                                uint32_t min_len, void *d_work, uint32_t *d_first, hipStream_t stream);
hipError_t launch_rle_seg_emit(const uint8_t *d_chars, uint32_t n_seqs, uint64_t total_bases, uint32_t max_gap_len, void *d_work, uint32_t *d_rles,
                               uint32_t capacity, hipStream_t stream);
void rle_seg_calls(uint64_t *count_calls, uint64_t *emit_calls); // launches of each since the process started
// A1: k-bounded matching statistics over all items
hipError_t launch_ms_walk(WalkArgs a, int max_waves, hipStream_t stream);
// A5+A6 (+ optional relative_to_ref when ref != nullptr, + optional i32 derandomised
// values when derand_out != nullptr): one lane per sequence.  max_seq_len = length of the
// longest sequence if known (0 = unknown); short reads take the LDS-staged kernel.
hipError_t launch_derand_translate(const uint8_t *d_ms, const uint64_t *d_offsets, uint32_t n_seqs,
                                   uint32_t k, uint32_t threshold, const uint8_t *d_ref,
                                   uint8_t *d_chars_out, int32_t *d_derand_out, uint32_t max_seq_len,
                                   uint32_t per_lane_max_len, hipStream_t stream, uint64_t total_bases = 0,
                                   void *d_work = nullptr, size_t work_bytes = 0);
// scratch that lets launch_derand_translate split long reads / contigs into pieces (one lane each)
size_t derand_piece_work_bytes(uint32_t n_seqs, uint64_t total_bases);
// A5+A6 for ONE very long sequence (pointers already offset to its first byte): chunked
// three-level scan over per-chunk transition tables; d_scratch >= derand_long_scratch_bytes().
size_t derand_long_scratch_bytes(uint64_t len, uint32_t k, uint32_t threshold);
hipError_t launch_derand_long(const uint8_t *d_ms, uint32_t len, uint32_t k, uint32_t threshold, const uint8_t *d_ref,
                              uint8_t *d_chars_out, int32_t *d_derand_out, void *d_scratch, hipStream_t stream);
constexpr uint32_t kLongSeq = 1u << 16; // sequences longer than this take the chunked path
// A5+A6 (+ relative_to_ref when d_ref != nullptr) for a batch in which sequence s has the threshold d_thresholds[s] and any length
// (derand_seq_kernels.hip): bit-identical to the sequential loops for every sequence of >= 3 bases whose threshold lies in
// [min_threshold, k]; shorter sequences are skipped, other thresholds give unspecified characters.  A constant number of launches,
// nothing read back; d_work >= derand_seq_work_bytes(), 16-byte aligned; n_seqs < 2^28, total_bases + 16 <= 2^32; not in place.
constexpr uint32_t kDerandSeqChunk = 128;      // positions per chunk (== KBO_DERAND_SEQ_CHUNK)
constexpr uint32_t kDerandSeqGroupChunks = 64; // chunks per group: KBO_DERAND_SEQ_GROUP = 8192 positions
size_t derand_seq_work_bytes(uint32_t n_seqs, uint64_t total_bases, uint32_t k, uint32_t min_threshold);
hipError_t launch_derand_translate_seq(const uint8_t *d_ms, const uint64_t *d_offsets, uint32_t n_seqs, uint64_t total_bases, uint32_t k,
                                       const uint32_t *d_thresholds, uint32_t min_threshold, const uint8_t *d_ref, uint8_t *d_chars_out,
                                       void *d_work, hipStream_t stream);
// The same passes with the characters counted in LDS instead of written (kbo_hip.h kbo_aln_extent): d_out = n_seqs records of six u32
// { 'M's, 'X's, 'R's, runs, start, end }, every one written (sequences of fewer than 3 bases: zeros); the same d_work.
hipError_t launch_derand_summary_seq(const uint8_t *d_ms, const uint64_t *d_offsets, uint32_t n_seqs, uint64_t total_bases, uint32_t k,
                                     const uint32_t *d_thresholds, uint32_t min_threshold, uint32_t *d_out, void *d_work, hipStream_t stream);
// A6 alone on clamped i32 derandomised values: one lane per position.
hipError_t launch_translate(const int32_t *d_derand, uint64_t len, uint32_t k, uint32_t threshold,
                            uint8_t *d_chars_out, hipStream_t stream);

// the breakpoint scan of call_variants over a batch (call_kernels.hip): 16-byte records {sequence, i, j, row of ms[j]} in
// kCallSegs lists (see launch_call_sites)
constexpr uint32_t kCallSegs = 256;
hipError_t launch_call_sites(const uint8_t *d_ms, const uint32_t *d_lo, const uint32_t *d_hi, const uint64_t *d_off,
                             uint32_t n_seqs, uint64_t total, uint32_t k, uint32_t threshold, void *d_sites, uint32_t cap,
                             uint32_t *d_count, hipStream_t stream);

// gap_filling::fill_gaps over a batch (gap_kernels.hip): the gap starts of a slab's translation as {sequence, start} records
// (d_count may end above cap: launch again with room), then one wave per gap writing the fills into d_out (a copy of d_tr);
// d_host_flag[s] = 1 for a sequence the host has to redo; d_stats = {gaps finished, left-extension steps}.
// d_log_tab[c] = log_rm_max_cdf(c + 1, 4, 1) for c < kGapFillLds; log_thr = log1p(-max_err_prob).
constexpr uint32_t kGapFillLds = 2048; // bytes of extended k-mer one wave keeps in LDS: longer extensions go to the host
hipError_t launch_gap_starts(const uint8_t *d_tr, const uint64_t *d_off, uint32_t n_seqs, uint64_t total, uint32_t threshold,
                             void *d_gaps, uint32_t cap, uint32_t *d_count, hipStream_t stream);
hipError_t launch_gap_fill(const uint8_t *d_q, const uint8_t *d_tr, uint8_t *d_out, const uint32_t *d_lo, const uint32_t *d_hi,
                           const uint64_t *d_off, const void *d_gaps, uint32_t n_gaps, uint32_t k, uint32_t threshold,
                           const double *d_log_tab, double log_thr, uint8_t *d_host_flag, unsigned long long *d_stats,
                           const DevIndexView &ix, hipStream_t stream);
// behind the first pass of a batch's call: every site of the kCallSegs lists becomes {sequence, i, j, row} (void records stay
// void) at index d_prefix[list] + slot of d_recs, and its window - the k MS bytes ending at j, the k characters of the row -
// goes to d_win (call_kernels.hip call_finalize_kernel); record stride = call_gather_stride(k) bytes: MS bytes at 0,
// characters at kpad, flag byte at 2 kpad
inline uint32_t call_gather_stride(uint32_t k) { return 2u * ((k + 15u) / 16u * 16u) + 16u; }
// the second pass of kbo::call on the device (call_second_kernels.hip): per-sequence tables of q-mer start positions, then per site
// { rpeak | qpeak << 8 | csl << 16 | flags << 24 } (0xFF = no peak; flags bit 0 = left to the host; ~0 for a void record)
hipError_t launch_call_qmer_index(const uint8_t *d_q, const uint64_t *d_off, uint32_t n_seqs, uint32_t qlen, const uint64_t *d_tab_off,
                                  uint32_t *d_tab, uint8_t *d_seq_flag, uint64_t total_slots, uint32_t max_slots, hipStream_t stream);
hipError_t launch_call_depths(const void *d_recs, const uint8_t *d_win, uint32_t stride, uint32_t n_sites, const uint8_t *d_q,
                              const uint64_t *d_off, uint32_t k, uint32_t thr, uint32_t qlen, bool revcomp, const uint64_t *d_tab_off,
                              const uint32_t *d_tab, const uint8_t *d_seq_flag, uint32_t *d_out, hipStream_t stream,
                              const uint32_t *d_n_sites = nullptr /* the number of sites on the device (n_sites then bounds it) */,
                              bool per_lane = false /* k <= 64 too through the kernel in which every lane extends its own matches (tests) */);
hipError_t launch_call_finalize(const void *d_lists, const uint32_t *d_counts, const uint32_t *d_prefix, uint32_t seg_cap, uint32_t max_count,
                                bool by_walk, const uint64_t *d_off, uint32_t n_seqs, uint32_t k, const uint8_t *d_ms,
                                const DevIndexView &ix, void *d_recs, uint8_t *d_win, uint32_t stride, hipStream_t stream);

// ---- a device copy's rank blocks / contraction entries / two-base blocks made on the device (layout_kernels.hip; formats: sbwt_index.hpp)
size_t device_layout_scratch_bytes(uint64_t n_sets);
hipError_t build_device_layout(const uint64_t *const d_rows[4], uint64_t n_words, const uint8_t *d_lcs, uint64_t n, const uint64_t C[4],
                               uint32_t n_blocks, uint4 *d_rank, uint32_t *d_ent, uint4 *d_pair, void *d_scratch, hipStream_t stream);

// ---- kbo::build on the device (build_kernels.hip, driven by build_device.cpp).  Keys are colex keys of W 64-bit words (sbwt_build.cpp
// Key<W>) stored as W word arrays: word j of key i at keys[j * stride + i].  Real counts ("real": non-$ characters of a row) are bytes.
constexpr uint32_t kBuildTile = 4096; // keys per tile of the radix sort and of the compaction
struct RadixPass {
    uint32_t a, nb; // the digit: key bits [a, a + nb) counted from the most significant bit of word 0 (nb <= 8)
    uint32_t real;  // 1: the digit is the real byte instead
};
size_t build_tiles(uint64_t n);
// every k-mer (and / or its reverse complement) ending an ACGT run of >= k bases of d_seq, appended at *d_count (any order)
hipError_t launch_build_extract(uint32_t W, const uint8_t *d_seq, uint64_t n_bytes, uint32_t k, bool fw, bool rc, uint64_t *d_keys,
                                uint64_t stride, unsigned long long *d_count, hipStream_t s);
// one stable LSD pass d_in -> d_out (n_words word arrays + the real bytes when d_rin); d_hist: 256 * build_tiles(n) words, d_sums:
// 256 * build_tiles(n) / kScanBlock + 2 words
hipError_t launch_build_radix_pass(const uint64_t *d_in, uint64_t *d_out, uint32_t n_words, uint64_t stride, const uint8_t *d_rin, uint8_t *d_rout,
                                   uint64_t n, const RadixPass &ps, uint32_t *d_hist, uint32_t *d_sums, hipStream_t s);
// flags[i] = key i (with its real byte when d_real) != key i - 1; flags[x] = sorted k-mer x has no predecessor
hipError_t launch_build_flag_distinct(uint32_t W, const uint64_t *d_keys, uint64_t stride, const uint8_t *d_real, uint64_t n, uint8_t *d_flags, hipStream_t s);
hipError_t launch_build_flag_orphan(uint32_t W, const uint64_t *d_keys, uint64_t stride, uint64_t n, uint32_t k, uint8_t *d_flags, hipStream_t s);
// the flagged keys, in order; *d_total += their number.  d_counts: build_tiles(n) words, d_sums: build_tiles(n) / kScanBlock + 2 words
hipError_t launch_build_compact(const uint64_t *d_in, uint64_t in_stride, uint64_t *d_out, uint64_t out_stride, uint32_t n_words, const uint8_t *d_rin,
                                uint8_t *d_rout, const uint8_t *d_flags, uint64_t n, uint32_t *d_counts, uint32_t *d_sums,
                                unsigned long long *d_total, hipStream_t s);
// the root and the k - 1 $-padded prefixes of every orphan: 1 + n_orph (k - 1) keys with their real bytes
hipError_t launch_build_dummies(uint32_t W, const uint64_t *d_orph, uint64_t o_stride, uint64_t n_orph, uint32_t k, uint64_t *d_keys, uint64_t stride,
                                uint8_t *d_real, hipStream_t s);
// sorted distinct k-mers + sorted distinct dummy rows -> rows in colex order (d_lb: n_d words)
hipError_t launch_build_merge(uint32_t W, const uint64_t *d_km, uint64_t km_stride, uint64_t n_km, uint32_t k, const uint64_t *d_dk, uint64_t d_stride,
                              const uint8_t *d_dreal, uint64_t n_d, uint32_t *d_lb, uint64_t *d_rk, uint64_t r_stride, uint8_t *d_rreal, hipStream_t s);
// edge bits into d_rows (4 zeroed bit-vectors of n_words words), LCS bytes; d_ctr (9 zeroed words): [0] rows without an incoming edge,
// [1 + c] rows >= 1 ending with c, [5 + c] edge bits of B_c
hipError_t launch_build_edges_lcs(uint32_t W, const uint64_t *d_rk, uint64_t stride, const uint8_t *d_rreal, uint64_t n, uint32_t k, uint64_t *d_rows,
                                  uint64_t n_words, uint8_t *d_lcs, unsigned long long *d_ctr, hipStream_t s);

// ---- the path cover laid out on the device (cover_kernels.hip; what it is: path_cover.cpp).  *ok = false: rows on cycles - the host's decides
hipError_t build_path_cover_device(const uint4 *d_rank, const uint32_t *d_ent, uint64_t n, uint32_t n_blocks, uint32_t k, const uint64_t C[4],
                                   uint8_t *d_text, uint32_t *d_pos, uint32_t *d_node, hipStream_t stream, bool *ok);

// ---- the tail of kbo::call on the device (call_emit_kernels.hip): the variants of a slab's sites in the order of (sequence, query
// position), as flat arrays.  d_meta: kCallMetaWords words
constexpr uint32_t kCallMetaSites = 0, kCallMetaValid = 1, kCallMetaVariants = 2, kCallMetaChars = 3, kCallMetaHost = 4, kCallMetaFlags = 5,
                   kCallMetaWorst = 6, kCallMetaWords = 16;
constexpr uint32_t kCallMaxRank = 4096;          // sites of one sequence the device puts in order itself (more: the host's)
constexpr uint32_t kCallNoVariant = 0xFFFFFFFFu; // per-site word: Err(ResolveVariantErr)
constexpr uint32_t kCallHostSite = 0xFFFFFFFEu;  // ... left to the host
struct CallEmitArgs {
    const uint4 *recs;       // call_finalize_kernel's records {sequence, i, j, row}; first word ~0 = void
    const uint32_t *codes;   // call_depths_kernel's word per site
    const uint8_t *win;      // ... and windows (row characters at kpad)
    uint32_t stride, kpad, k;
    const uint8_t *q;        // the slab's bases
    const uint64_t *off;     // ... and offsets
    uint32_t n_seqs;
    const uint32_t *n_sites; // on the device: d_prefix[kCallSegs]
    uint32_t cap;            // what bounds it
    uint32_t *seq_cnt, *seq_sums, *seq_fill; // n_seqs + 1 (+ scan sums), n_seqs
    uint32_t *bucket, *bkey, *sorted, *vrec; // cap each
    uint32_t *vcnt, *vsums, *ccnt, *csums;   // cap + 1 (+ scan sums) each
    uint32_t *out_pos, *out_lens;            // cap: query_pos; query_len | ref_len << 16
    uint8_t *out_chars;
    uint32_t chars_cap;
    uint32_t *seq_vfirst;    // n_seqs + 1: variants in front of every sequence
    uint32_t *host_list;     // sites left to the host (indices into recs), host_cap of them at most
    uint32_t host_cap;
    uint32_t *meta;
};
inline size_t call_scan_sums_words(size_t n) { return (n + 1023) / 1024 + 1; }
hipError_t launch_call_prefix(const uint32_t *d_counts, uint32_t seg_cap, uint32_t *d_prefix /* kCallSegs + 1 */, uint32_t *d_meta, hipStream_t stream);
hipError_t launch_call_emit(const CallEmitArgs &a, void *d_host_recs, uint8_t *d_host_win, hipStream_t stream);

// 2-bit packed reads in / packed alignments out (pack_kernels.hip): sequence s occupies ceil(len / 16) u32 words, base i in
// bits 2 (i mod 16) of word i / 16.  uniform_wps != 0: all sequences have that many words (no prefix needed); otherwise
// d_scratch holds the scanned words-per-sequence (launch_packed_prefix; chunk_items_scratch_words(n_seqs) u32)
hipError_t launch_uniform_offsets(uint64_t *d_off, uint32_t n_seqs, uint32_t len, hipStream_t stream);
hipError_t launch_packed_prefix(const uint64_t *d_off, uint32_t n_seqs, uint32_t *d_scratch, hipStream_t stream);
hipError_t launch_unpack2(const uint32_t *d_packed, uint32_t n_words, const uint64_t *d_off, uint32_t n_seqs, uint32_t uniform_wps,
                          const uint32_t *d_scratch, uint8_t *d_q, hipStream_t stream);
hipError_t launch_exceptions(const uint64_t *d_pos, const uint8_t *d_byte, uint32_t n, uint64_t base, uint8_t *d_q, hipStream_t stream);
hipError_t launch_pack2(const uint8_t *d_chars, uint32_t n_words, const uint64_t *d_off, uint32_t n_seqs, uint32_t uniform_wps,
                        const uint32_t *d_scratch, uint32_t *d_packed, hipStream_t stream);

// the reverse complement of a batch (revcomp_kernels.hip), per sequence: output base i = complement of input base len - 1 - i
// (A <-> T, C <-> G, a <-> t, c <-> g, other bytes as they are).  Bytes: d_in 16-byte aligned with the usual 16 bytes of slack,
// d_out anywhere; exactly [d_out, d_out + total) is written; sequences may be empty.  Packed: the layout above (d_data / d_sums:
// the scanned words-per-sequence and its block sums unless uniform_wps != 0), padding bits of the output zero.  The exception
// list mirrored within each sequence, ascending again: position p (pos - base in the batch of d_off) -> out_base + off[s] +
// off[s + 1] - 1 - p, the byte complemented.  None of them works in place.
hipError_t launch_revcomp_bytes(const uint8_t *d_in, const uint64_t *d_off, uint32_t n_seqs, uint64_t total, uint8_t *d_out, hipStream_t stream);
hipError_t launch_revcomp_packed(const uint32_t *d_in, uint32_t n_words, const uint64_t *d_off, uint32_t n_seqs, uint32_t uniform_wps,
                                 const uint32_t *d_data, const uint32_t *d_sums, uint32_t *d_out, hipStream_t stream);
hipError_t launch_revcomp_exceptions(const uint64_t *d_pos, const uint8_t *d_byte, uint32_t n, uint64_t base, const uint64_t *d_off,
                                     uint32_t n_seqs, uint64_t out_base, uint64_t *d_pos_out, uint8_t *d_byte_out, hipStream_t stream);
// a batch doubled on the device: off[n + 1 + j] = off[n] + off[j + 1] (d_off holds 2 n + 1 entries), items[n + i] = items[i]
// `shift` bases on
hipError_t launch_double_offsets(uint64_t *d_off, uint32_t n_seqs, hipStream_t stream);
hipError_t launch_double_items(WalkItem *d_items, uint32_t n_items, uint64_t shift, hipStream_t stream);

// the sparse form of kbo::matches (sparse_kernels.hip): the runs of characters other than 'M' of a packed batch's character words
// (the layout above), as kbo_aln_run records {seq_base + seq, start, (length << 2) | code} in (seq, start) order.  d_prefix: the
// scanned words-per-sequence (launch_packed_prefix) unless uniform_wps != 0; d_scratch: kSparseScratchWords u32.  n_blocks =
// sparse_blocks(an upper bound of the batch's words), the same for both launches; the batch itself holds < 2^32 - 256 words.
// launch_sparse_count: runs per workgroup, scanned; launch_sparse_emit: the first `capacity` records (the others are counted
// only) and *d_total = the number of runs; it may run again with a larger buffer behind the same count.
constexpr uint32_t kSparseMaxBlocks = 2048;
constexpr size_t kSparseScratchWords = kSparseMaxBlocks + 1 + 3; // counts per workgroup + 1, the scan's block sums
uint32_t sparse_blocks(uint64_t words_bound);
hipError_t launch_sparse_count(const uint32_t *d_words, const uint64_t *d_off, uint32_t n_seqs, uint32_t uniform_wps, const uint32_t *d_prefix,
                               uint32_t n_blocks, uint32_t *d_scratch, hipStream_t stream);
hipError_t launch_sparse_emit(const uint32_t *d_words, const uint64_t *d_off, uint32_t n_seqs, uint32_t uniform_wps, const uint32_t *d_prefix,
                              uint32_t n_blocks, const uint32_t *d_scratch, uint32_t seq_base, uint32_t *d_runs, uint32_t capacity,
                              uint32_t *d_total, hipStream_t stream);

// per-sequence alignment summaries of characters in memory (summary_kernels.hip): d_out[s] = { 'M's, 'X's, 'R's, runs } of sequence s (a run:
// a maximal stretch without '-'), zeros for a sequence of fewer than 3 bases.  Bytes: one character a byte at d_chars + d_off[s] (any
// alignment; nothing outside the 16-byte aligned blocks that hold a character is read); words: the packed layout's character words
// (M - X R = 0 .. 3) with d_prefix = the scanned words-per-sequence (launch_packed_prefix).  bases_bound: an upper bound of d_off[n_seqs] that
// sizes the grid, 0 = unknown (the most workgroups).  d_out is zeroed first and exactly n_seqs records are written.
hipError_t launch_summary_bytes(const uint8_t *d_chars, const uint64_t *d_off, uint32_t n_seqs, uint64_t bases_bound, uint4 *d_out, hipStream_t stream);
hipError_t launch_summary_words(const uint32_t *d_words, const uint64_t *d_off, uint32_t n_seqs, const uint32_t *d_prefix, uint64_t bases_bound,
                                uint4 *d_out, hipStream_t stream);

// a[i] = max(a[i], b[i]) over n bytes (n rounded up to 16: both buffers have that slack): the MS values of a further shard of a
// sharded index folded into the batch's (pack_kernels.hip)
hipError_t launch_max_bytes(uint8_t *d_a, const uint8_t *d_b, uint64_t n, hipStream_t stream);

// ---- kbo::map / matches for sequences of any length in one launch (long_kernels.hip): one wave per PIECE of a sequence - `own`
// bases inside a region of at most kLongRegion bases (k bases of the sequence in front of them, k + 1 behind)
constexpr uint32_t kLongRegion = 1008; // (+ up to 15 bases of alignment: 64 words of 16 positions)
constexpr uint32_t kLongOwnMin = 256;  // own bases a piece must have for the kernel to apply (k <= 375)
struct LongArgs {
    DevIndexView ix;
    const uint8_t *q;     // concatenated queries (ASCII), 16-byte aligned
    uint64_t q_bytes;
    const void *items;    // per piece { first byte of its region, that byte's place in its sequence, the sequence's length, own0 | own_n << 10 }
    uint32_t n_items;     // slots (those past the batch's last piece are empty)
    uint8_t *chars_out;
    uint8_t *redo;        // per piece: 1 = its proof failed (the plain walk + the literal recurrences decide: launch_map_long_redo)
    uint8_t *xin;         // per piece: the derandomised value of its first own base, 0 .. k (<= 0 as 0)
    uint32_t *qctl;       // [0] pieces, [1] sub-items of the flagged pieces, [2] flagged pieces listed, [4] flagged pieces
    uint32_t *pstats;     // work counters (kPlanStat*)
    uint32_t ppw;         // consecutive pieces a wave takes
    uint32_t xexp;        // experiment switches (KBO_LONG_X): timing only, results are wrong with any of them
    uint32_t thr, fmt, ca; // derandomisation threshold, 1 = format::relative_to_ref on the way out, bases of a region behind the own ones
    void *subs;           // WalkItem records of the flagged pieces' sub-items
    uint32_t *flist;      // the flagged pieces, listed (qctl[2] of them)
    uint32_t sub_cap;
};
size_t long_work_bytes(size_t n_seqs, uint64_t total_bases, uint32_t k); // bytes of work memory of a launch (0: k too large)
// true when the copy has what the kernel needs (depth table of fewer bases than the threshold, 2-bit text, seed positions)
bool map_long_applies(const DevIndexView &ix, uint32_t thr);
void set_map_long(int mode); // tuning / tests: see kbo_set_map_long
hipError_t launch_map_long(const DevIndexView &ix, const uint8_t *d_q, const uint64_t *d_off, uint32_t n_seqs, uint64_t total_bases, uint32_t thr,
                           bool fmt, uint8_t *d_chars, void *d_work, hipStream_t stream, LongArgs &a, bool count /* work counters: kbo_set_plan_stats */);
hipError_t launch_map_long_redo(const LongArgs &a, uint8_t *d_ms, hipStream_t stream);
// the control words (32) and work counters of the last launch over d_work; synchronises the stream
hipError_t long_read_stats(const void *d_work, size_t n_seqs, uint64_t total_bases, uint32_t k, uint32_t ctl[32], uint32_t *stats, hipStream_t stream);
// the plain walk over a list of items whose number is counted on the device (walk_kernels.hip): `lanes` lanes share them
hipError_t launch_walk_list(WalkArgs a, const WalkItem *d_list, uint32_t cap, const uint32_t *d_count, uint32_t lanes, hipStream_t stream);

// ---- the walk against a set of small indexes, each staged whole into LDS (refset_kernels.hip)
// LDS form of one index of n rows, in 16-byte units: 2 (n / 32 + 1) units of rank blocks - block b covers rows [32 b, 32 b + 32) and
// holds, for c = A, C, G, T, the 8 bytes { C[c] + rank_c(32 b), the 32 row bits } (one ds_read_b64 per rank) - then ceil((n + 1) / 16)
// units of LCS bytes with the sentinel LCS[n] = 0.  2 bytes a row; the packed device layout of a set is these forms back to back.
constexpr uint32_t kRefsetMaxRows = 16384; // rows of an index that takes this kernel: 32.8 KiB of LDS, four workgroups of it a compute unit
constexpr uint32_t kRefsetChunk = 256;     // bases a lane emits (== KBO_REFSET_CHUNK; max(this, 4 k) in all), + k - 1 warm-up bases
constexpr uint32_t kRefsetThreads = 256;   // lanes of a workgroup = the most chunks of one task
__host__ __device__ inline uint32_t refset_rank_units(uint32_t n_sets) { return 2u * (n_sets / 32u + 1u); }
__host__ __device__ inline uint32_t refset_units(uint32_t n_sets) { return refset_rank_units(n_sets) + (n_sets + 1u + 15u) / 16u; }
struct RefsetDesc { // one per reference of the set, on the device
    uint32_t off;     // first 16-byte unit of its LDS form in the set's arena
    uint32_t n_sets;
    uint32_t C[4];
    int32_t status;   // 0, or why the reference cannot be queried (then it has no units)
    uint32_t route;   // 0: this kernel, 1: an ordinary index of its own, 2: the same form, walked from memory (refset_wide_kernels.hip)
    uint64_t n_kmers;
};
struct RefsetWalkArgs {
    const RefsetDesc *descs;
    const uint4 *arena;
    const uint4 *tasks;  // { reference, first item, items (<= kRefsetThreads), 0 }: one workgroup each
    const uint4 *items;  // { first base in q, first byte in ms, bases | warm-up bases << 16, 0 }: one lane each
    uint32_t n_tasks;
    uint32_t k;
    const uint8_t *q;    // the query batch, both strands
    uint8_t *ms;         // the slab: one byte per (pair, base)
};
// (a task whose reference has another route than kRefsetRouteLds is skipped: the task list of a slab is shared by both walks)
hipError_t launch_refset_walk(const RefsetWalkArgs &a, uint32_t lds_units /* the largest refset_units() among the tasks' LDS references */, hipStream_t stream);
// ---- the same walk with the form read from the arena (refset_wide_kernels.hip): references of more than kRefsetMaxRows and at most
// kRefsetWideMaxRows rows (a form of 2 MiB, half of an XCD's L2).  It takes the tasks of the references of kRefsetRouteWide and skips the rest
constexpr uint32_t kRefsetWideMaxRows = 1u << 20;
constexpr uint32_t kRefsetRouteLds = 0, kRefsetRouteIndex = 1, kRefsetRouteWide = 2; // RefsetDesc::route
hipError_t launch_refset_wide_walk(const RefsetWalkArgs &a, hipStream_t stream);
// kbo_summary_refset: of the n_pairs extents of a slab (six u32 a pair, launch_derand_summary_seq's) those with n_runs > 0, in pair
// order, as records of seven u32 { pair, extent } at d_kept (room for n_pairs of them) and their number at d_total;
// d_scratch: chunk_items_scratch_words(n_pairs) u32.  Nothing read back.
hipError_t launch_refset_keep(const uint32_t *d_ext, uint32_t n_pairs, uint32_t *d_scratch, uint32_t *d_kept, uint32_t *d_total, hipStream_t stream);
// ---- the slab planner and the record stage of the device-resident reference-set calls (refset_plan_kernels.hip; the arithmetic:
// refset_plan.hpp).  Everything the planner reads is on the device: the batch's offsets, the references' thresholds (0: the
// reference cannot be queried), the scanned chunk counts and the list of the queryable references that launch_refset_plan_call makes
struct RefsetPlan {
    refplan::Geometry g;
    const uint64_t *off;                // n_seqs + 1
    const uint32_t *thr;                // per reference of the set
    const uint32_t *nch, *nch_sums;     // chunks of every sequence, scanned (n_seqs + 1 values, two levels)
    const uint32_t *qref;               // the queryable references, ascending
};
// once per call, 6 launches: d_nch and d_qflag take chunk_items_scratch_words(n_seqs) / (n_refs) u32, d_qref n_refs u32; *d_count = 0
hipError_t launch_refset_plan_call(const RefsetPlan &a, uint32_t n_refs, uint32_t *d_nch, uint32_t *d_qflag, uint32_t *d_qref, uint64_t *d_count,
                                   hipStream_t stream);
// a slab of `refs` queryable references from the first_q-th on, 2 launches: pair offsets (pairs + 1) and thresholds, the '-' of the
// pairs of fewer than 3 bases (d_chars, or nullptr), refs * g.item_slots item slots and refs * g.tasks_per_ref tasks of the walk
hipError_t launch_refset_plan_slab(const RefsetPlan &a, uint32_t first_q, uint32_t refs, uint64_t *d_poff, uint32_t *d_pthr, uint8_t *d_chars,
                                   uint4 *d_items, uint4 *d_tasks, hipStream_t stream);
// the slab's records into the call's list, 2 launches: record x becomes { ref, seq, strand, record } at element *d_count + x of d_out when
// that is in front of `capacity`; then *d_count grows by the slab's records, written or not.  Runs: d_first / d_local are the
// segmented run-length stage's prefix and its first local_cap records of seven u32; summaries: launch_refset_keep's list and count
hipError_t launch_refset_tag_runs(const RefsetPlan &a, uint32_t first_q, uint32_t n_pairs, const uint32_t *d_first, const uint32_t *d_local,
                                  uint32_t local_cap, uint64_t *d_count, uint64_t capacity, uint32_t *d_out, hipStream_t stream);
hipError_t launch_refset_tag_summaries(const RefsetPlan &a, uint32_t first_q, uint32_t n_pairs, const uint32_t *d_kept, const uint32_t *d_n_kept,
                                       uint64_t *d_count, uint64_t capacity, uint32_t *d_out, hipStream_t stream);
// ---- the best reference per sequence (refset_best_kernels.hip; the record and its merge: refset_best.hpp).  The table is n_seqs
// records of twelve u32 (kbo_ref_best), set to the empty records once per call; behind the summary stage of every slab its extents
// are merged in.  The slab's n_pairs pairs are numbers [lead, lead + n_pairs) of (reference of the slab, sequence, strand index) in
// that order, counted from the slab's first reference on: lead < n_seqs * n_strands is where the slab begins within that reference.
struct RefsetBestArgs {
    const uint32_t *ext;   // six u32 a pair of the slab (launch_derand_summary_seq's), 8-byte aligned
    const uint32_t *refs;  // the slab_refs references the slab's pairs belong to, in order
    uint32_t *table;       // n_seqs records, 4-byte aligned
    uint32_t n_pairs, lead, slab_refs;
    uint32_t n_seqs, n_strands, strands; // strands: KBO_STRAND_FWD, KBO_STRAND_REV or both (then n_strands = 2)
};
// below this many sequences a workgroup of four waves shares one sequence's pairs, from it on a wave has a sequence to itself
constexpr uint32_t kRefsetBestSplitBelow = 64;
bool refset_best_splits(uint32_t n_seqs);
hipError_t launch_refset_best_init(uint32_t *d_table, uint32_t n_seqs, hipStream_t stream); // n_seqs < 2^28
hipError_t launch_refset_best(const RefsetBestArgs &a, hipStream_t stream);                 // one launch; none for n_pairs == 0

// ---- the seed screen of a reference set (refset_screen_kernels.hip; the seed and the bucket scan: refset_screen.hpp).  The table is
// the set's: kBuckets + 1 offsets, then per entry a key (code << 16 | valid bases) and its reference, sorted by key.  A lane owns
// kRefsetScreenRun consecutive start positions of one strand of the batch, a workgroup kRefsetScreenThreads lanes; m: per reference,
// the shared bases that mark a pair (refscreen::kUnfilterable: never).  Bit (r * n_seqs + s) * 2 + strand - 1 of `bits` is set with
// atomicOr; the caller zeroes the bitmap.  n_refs * n_seqs * 2 <= 2^31 and total < 2^31.
constexpr uint32_t kRefsetScreenRun = 64;
constexpr uint32_t kRefsetScreenThreads = 256;
struct RefsetScreenArgs {
    const uint32_t *bucket;
    const uint64_t *keys;
    const uint32_t *refs;
    const uint8_t *m;       // n_refs bytes
    const uint8_t *q;       // the batch, 16-byte aligned: '+' at q, '-' at q + rev_base
    const uint64_t *off;    // n_seqs + 1, from 0
    uint32_t *bits;
    uint64_t total, rev_base; // rev_base: a multiple of 16, >= total
    uint32_t n_seqs, strands, first_strand; // strands: 1, 2 or 3; first_strand: 2 for strands == 2, else 1
};
hipError_t launch_refset_screen(const RefsetScreenArgs &a, hipStream_t stream); // one launch; none for total == 0

// ---- the locus of a run (refset_locate_kernels.hip; the look-up and the record: refset_locate.hpp).  One wave per record of d_runs,
// grid-strided over min(*n_runs, capacity); the kernel checks every record against the descs and the offsets itself and reads nothing
// outside the batch, the arena and the table.  positions: the set's entries, reference r's rows from pos_off[r] on
struct RefsetLocateArgs {
    const RefsetDesc *descs;
    const uint4 *arena;
    const uint32_t *positions;
    const uint64_t *pos_off;
    const uint8_t *q;        // the '+' batch
    const uint64_t *off;     // n_seqs + 1
    const uint32_t *runs;    // kbo_ref_run: ten u32 a record
    const uint64_t *n_runs;  // on the device
    uint32_t *loci;          // kbo_ref_locus: six u32 a record
    uint64_t capacity, total;
    uint32_t n_refs, n_seqs, k;
};
constexpr uint32_t kRefsetLocateThreads = 256;
hipError_t launch_refset_locate(const RefsetLocateArgs &a, hipStream_t stream); // one launch; none for capacity == 0

// ---- depth and breadth of every reference over a list of runs (refset_cover_kernels.hip; the arithmetic and the layout of `work`:
// refset_cover.hpp).  The records of d_runs are read and checked as the locate kernel does; an unusable one is skipped.  work: the
// references' counters, then one word per base of every reference with entries, reference r's from base_off[r] on - cleared by the
// launch; depth (or null): the profile, `bases` words laid out by base_off too
struct RefsetCoverArgs {
    const RefsetDesc *descs;
    const uint4 *arena;
    const uint32_t *positions;
    const uint64_t *pos_off;
    const uint64_t *base_off; // n_refs + 1
    const uint32_t *ref_len;  // n_refs: every reference's length as given
    const uint8_t *q;         // the '+' batch
    const uint64_t *off;      // n_seqs + 1
    const uint32_t *runs;     // kbo_ref_run: ten u32 a record
    const uint64_t *n_runs;   // on the device
    uint32_t *covers;         // kbo_ref_cover: twelve u32 a record, n_refs records
    uint32_t *depth;
    uint8_t *work;            // refcover::work_bytes(n_refs, bases) bytes, 16-byte aligned
    uint64_t capacity, total, bases;
    uint32_t n_refs, n_seqs, k;
};
constexpr uint32_t kRefsetCoverThreads = 256;
// the clear and refset_cover_count_kernel, refset_cover_scan_kernel, refset_cover_reduce_kernel; for capacity == 0 the clear and the last
hipError_t launch_refset_cover(const RefsetCoverArgs &a, hipStream_t stream);

// ---- the first pass of kbo::call over a slab of pairs (refset_call_kernels.hip; the arithmetic: refset_call.hpp), behind the walk and
// launch_derand_summary_seq of the slab: the candidates of the kept pairs, their sites {pair, i, j, row} and a window record per site
// (refcall::window_stride(k) bytes: the k depths that end at j, then at refcall::window_pad(k) the k characters of the row)
struct RefsetCallArgs {
    const RefsetDesc *descs;
    const uint4 *arena;
    const uint8_t *q;     // the walk's query buffer
    const uint8_t *ms;    // the slab's matching statistics, `bytes` of them
    const uint64_t *poff; // n_pairs + 1: the pairs' first bytes
    const uint32_t *pthr; // n_pairs: the pairs' thresholds
    const uint32_t *ext;  // n_pairs extents, six u32 each (launch_derand_summary_seq): a pair with n_runs == 0 is not scanned
    const uint32_t *pref; // n_pairs: the pairs' references
    const uint32_t *pq;   // n_pairs: the first base of the pair's sequence on its strand in q
    uint32_t *counts;     // kRefsetCallCountBytes: [0] candidates, [16] sites; zeroed by the launch
    uint2 *cands;         // cap records {pair, i}
    uint4 *sites;         // cap records {pair, i, j, row}, in no order
    uint8_t *win;         // cap window records, same index as sites
    uint64_t bytes;
    uint32_t n_pairs, k, min_thr, cap; // min_thr: no pair's threshold is below it
};
constexpr uint32_t kRefsetCallThreads = 256;
constexpr size_t kRefsetCallCountBytes = 128;
// a clear of the counts and three launches.  counts[0] > cap afterwards: candidates were dropped, repeat with cap >= counts[0]
hipError_t launch_refset_call(const RefsetCallArgs &a, hipStream_t stream);

// ---- the screened device forms (refset_cand_kernels.hip; the arithmetic: refset_cand.hpp): the bitmap of the screen to the list of
// its set bits, ONE slab of the list's longest prefix within the caps planned from it, and the record and merge stages that name a
// pair by the list.  Everything is read on the device; stream order is the only synchronisation.
struct RefsetCandArgs {
    const uint64_t *off;   // the batch's offsets, n_seqs + 1
    const uint32_t *thr;   // per reference of the set (0: it cannot be queried)
    const uint8_t *m;      // per reference: what the screen kernel takes, refcand::kMarkAll for a packed reference that cannot be screened
    uint32_t *bits;        // the bitmap, `words` words
    uint32_t *pc;          // chunk_items_scratch_words(words) u32: the words' popcounts, scanned (two levels)
    uint64_t *hdr;         // { candidates, pairs walked, bases walked, 0 }: the call's own copy of the figures
    uint64_t *stats;       // kbo_refset_screen_stats: { n_candidates, candidate_bases, n_walked, walked_bases }, zeroed by the caller
    uint32_t *list;        // max_pairs u32: the bit of the pair at every rank, refcand::kNoPair behind the candidates
    uint64_t *poff;        // max_pairs + 1: the pairs' lengths, then their prefix, then the pairs' first bytes (in place)
    uint64_t *bsum;        // (max_pairs + 1) / 1024 + 2 u64: the block sums of that prefix
    uint32_t *pthr;        // max_pairs
    uint32_t *nch;         // chunk_items_scratch_words(max_pairs) u32: the pairs' chunk counts, scanned
    uint32_t *rfirst;      // n_refs + 1: the first item of every reference
    uint32_t *ntask;       // chunk_items_scratch_words(n_refs) u32: the references' task counts, scanned
    uint64_t n_bits, max_bases, rev_off; // rev_off: where the '-' strand begins in the walk's query buffer
    uint32_t words, n_refs, n_seqs, strands, k, chunk, max_pairs, item_slots, task_slots, safe_ref; // safe_ref: names the empty tasks
};
// 3 launches: the pairs of the references that cannot be screened set in the bitmap, the words' popcounts and their scan;
// stats[1] += the candidates' bases
hipError_t launch_refset_cand_count(const RefsetCandArgs &a, hipStream_t stream);
// 1 launch: stats[0] = the candidates (kbo_refset_candidates_dev: nothing is walked)
hipError_t launch_refset_cand_stats(const RefsetCandArgs &a, hipStream_t stream);
// 4 launches behind launch_refset_cand_count: the list, the 64-bit scan of the lengths, the cut; hdr and stats written
hipError_t launch_refset_cand_list(const RefsetCandArgs &a, hipStream_t stream);
// 7 launches: pair offsets and thresholds (the '-' of pairs of fewer than 3 bases in d_chars, or nullptr), chunk counts and their scan,
// the references' items and tasks and their scan, a.item_slots item slots and a.task_slots tasks of the walk
hipError_t launch_refset_cand_plan(const RefsetCandArgs &a, uint8_t *d_chars, uint4 *d_items, uint4 *d_tasks, hipStream_t stream);
// 1 launch each: launch_refset_tag_runs / _summaries with (ref, seq, strand) from the list; *d_count = the records there are
hipError_t launch_refset_cand_tag_runs(const RefsetCandArgs &a, const uint32_t *d_first, const uint32_t *d_local, uint32_t local_cap, uint64_t *d_count,
                                       uint64_t capacity, uint32_t *d_out, hipStream_t stream);
hipError_t launch_refset_cand_tag_summaries(const RefsetCandArgs &a, const uint32_t *d_kept, const uint32_t *d_n_kept, uint64_t *d_count,
                                            uint64_t capacity, uint32_t *d_out, hipStream_t stream);
// 1 launch: the extents of the walked pairs (six u32 at the pair's rank) merged into the table, a sequence's pairs found by its bits
hipError_t launch_refset_cand_best(const RefsetCandArgs &a, const uint32_t *d_ext, uint32_t *d_table, hipStream_t stream);

// ---- the second pass of kbo::call on the device (refset_resolve_kernels.hip; the arithmetic: refset_resolve.hpp), for the
// device-resident calls kbo_call_refset_dev / kbo_call_refset_screened_dev.  Per slab: what launch_refset_call reads of a pair that
// only the slab's plan knows, made on the device, and the slab's sites appended to the call's list.  Per call: launch_refset_resolve.
struct RefsetSitePairs { // n_pairs words each
    uint32_t *pref; // the pair's reference
    uint32_t *pq;   // the first base of its sequence on its strand in the walk's query buffer
    uint32_t *pseq; // sequence << 1 | strand - 1
};
// 1 launch each: the pairs of a slab of the unscreened form (launch_refset_plan_slab's), of the ONE slab of the screened form
hipError_t launch_refset_site_pairs_plan(const RefsetPlan &a, uint32_t first_q, uint32_t n_pairs, const RefsetSitePairs &out, hipStream_t stream);
hipError_t launch_refset_site_pairs_cand(const RefsetCandArgs &a, const RefsetSitePairs &out, hipStream_t stream);
constexpr uint32_t kRefsetSiteTagWords = 8; // { ref, seq, strand, threshold, i, j, first base of the sequence on its strand, 0 }
struct RefsetResolveArgs {
    const uint8_t *concat; // the '+' batch: what the index is made of
    const uint8_t *q;      // the walk's query buffer: the query-side k-mers
    const uint64_t *off;   // n_seqs + 1
    uint64_t total;
    uint32_t n_seqs, k, qlen, add_revcomp;
    uint32_t max_sites;
    uint32_t *tags;        // max_sites records of kRefsetSiteTagWords words, 16-byte aligned
    uint8_t *wins;         // max_sites window records of refcall::window_stride(k) bytes
    uint64_t *ix[2];       // `total` words each: the index and the sort's other buffer
    uint64_t *keys[2];     // 2 * max_sites words each: the sites' key words (hi, then lo) and the sort's other buffer
    uint32_t *hist, *sums; // the radix passes': 256 * build_tiles(max(total, max_sites)) words, that / kScanBlock + 2 words
    uint32_t *words;       // max_sites: the sites' resolve words
    uint32_t *vcnt, *ccnt; // max_sites + 1 each: variants and characters in front of every place of the order ...
    uint32_t *vsums, *csums; // ... and their block sums, (max_sites + 1) / kScanBlock + 1 each
    uint32_t key_seq_bits, key_hi_bits, key_i_bits; // refresolve::key_shape
    uint32_t *variants;    // kbo_ref_variant: six u32 a record
    uint8_t *chars;
    uint64_t max_variants, max_chars;
    uint64_t *stats;       // kbo_ref_calls_stats: { n_variants, n_chars, n_sites, max_slab_candidates, n_panics, 0, 0, 0 }
};
// 1 launch behind launch_refset_call of a slab: site x of the slab becomes record stats[2] + x of the call's list when that is in
// front of max_sites, tagged by its pair; stats[2] grows by the slab's sites, stats[3] becomes the most candidates a slab had
hipError_t launch_refset_sites_append(const RefsetCallArgs &slab, const RefsetSitePairs &pairs, const RefsetResolveArgs &a, hipStream_t stream);
// behind the last slab, 25 + 4 refresolve::key_passes() launches whatever the batch holds: the index (1 + 4 x 4), the sites' words
// (1), their keys (1) and the sort (4 a pass), the counts (1), two scans (2 x 2), the records and characters (1)
hipError_t launch_refset_resolve(const RefsetResolveArgs &a, hipStream_t stream);

constexpr int kWalkThreads = 64; // default workgroup size (waves are independent: no LDS, no barriers)
void set_walk_threads(int threads); // tuning: 64, 128 or 256
void set_walk_experiment(int lane_limit, int dummy_lds_bytes); // experiments behind DESIGN.md section 6
void set_walk_rare(int period);            // tuning: hot-loop iterations between rare-block visits
// ---- locate_kernels.hip (the arithmetic, the tile and the d_work layout: index_locate.hpp)
// a walked slab of the sources into the rows' smallest / largest occurrence (d_min cleared to ones, d_max to zeros beforehand) and the
// bases with a full depth counted; then d_min turned into the entries and the rows that have one counted
hipError_t launch_locate_mark(const uint8_t *d_ms, const uint32_t *d_lo, uint32_t len, uint32_t k, uint32_t n_rows, uint32_t base, bool rev,
                              uint32_t *d_min, uint32_t *d_max, uint64_t *d_n_full, hipStream_t stream);
hipError_t launch_locate_entries(uint32_t *d_min, const uint32_t *d_max, uint32_t n_rows, uint64_t *d_n_entries, hipStream_t stream);
struct SegmentArgs {
    const uint8_t *ms;       // a batch as the interval walk left it
    const uint32_t *lo;
    const uint64_t *off;
    const uint32_t *entries; // n_rows words
    uint32_t n_seqs, n_rows, k, bridge, strand, n_delta;
    uint64_t total, capacity;
    uint32_t *segs;          // capacity records of 7 words
    uint64_t *n_segs;
    uint32_t *delta;         // n_delta words, or null
    void *work;              // idxlocate::seg_work(total).bytes
};
hipError_t launch_segments(const SegmentArgs &a, hipStream_t stream);
// d_depth = the inclusive prefix sums of n words of d_delta; d_work: idxlocate::depth_work(n) bytes
hipError_t launch_depth_finish(const uint32_t *d_delta, uint32_t *d_depth, uint64_t n, void *d_work, hipStream_t stream);
// ---- place_kernels.hip (the arithmetic, the ring and the d_work layout: index_place.hpp)
struct PlaceArgs {
    const uint32_t *segs;    // records of 7 words as launch_segments left them: min(*n_segs, capacity) are looked at
    const uint64_t *n_segs;
    uint64_t capacity;
    const uint64_t *src_off; // n_src + 1 values
    uint32_t n_seqs, n_src, k, max_gap, max_indel;
    bool merge;              // into what `place` holds
    void *place;             // n_seqs records of 48 bytes, 16-byte aligned
    void *work;              // idxplace::place_work(n_seqs, capacity).bytes
};
// at most four launches, sized by n_seqs and capacity alone: the ranges cleared, a lane per record, a lane per sequence, a wave per
// sequence with a long list (the second and the fourth only when capacity can hold such records)
hipError_t launch_place(const PlaceArgs &a, hipStream_t stream);
// ---- pileup_kernels.hip (the arithmetic and the d_work figure: index_pileup.hpp)
struct PileupArgs {
    const uint32_t *segs;    // records of 7 words as launch_segments left them: min(*n_segs, capacity) are looked at
    const uint64_t *n_segs;
    uint64_t capacity;
    const uint8_t *concat;   // the batch as it was walked, and the MS bytes of that walk: `total` bytes each
    const uint8_t *ms;
    const uint64_t *off;     // n_seqs + 1 values
    uint32_t n_seqs, k;
    uint64_t total, source_bases;
    bool skip_multi;
    uint32_t *pile;          // source_bases rows of four words, added to
};
// one launch, sized by capacity alone (none when capacity, total or source_bases is 0)
hipError_t launch_pileup(const PileupArgs &a, hipStream_t stream);
struct PileupSitesArgs {
    const void *pile;        // source_bases rows of four words, 16-byte aligned
    const uint32_t *depth;   // source_bases words
    const uint64_t *src_off; // n_src + 1 values
    uint32_t n_src, min_count, frac_num, frac_den;
    uint64_t source_bases, capacity;
    void *sites;             // capacity records of 32 bytes, 16-byte aligned
    uint64_t *n_sites;
    void *work;              // idxpile::sites_work(source_bases) bytes
};
// three launches: the sites of every chunk counted, the counts scanned by one workgroup, the records written
hipError_t launch_pileup_sites(const PileupSitesArgs &a, hipStream_t stream);
// ---- indel_kernels.hip (the arithmetic and the d_work figures: index_indel.hpp)
struct IndelEventArgs {
    const uint32_t *segs;    // records of 7 words as launch_segments left them: min(*n_segs, capacity) are looked at
    const uint64_t *n_segs;
    uint64_t capacity;
    const uint8_t *concat;   // the batch as it was walked: `total` bytes
    const uint64_t *off;     // n_seqs + 1 values
    const uint64_t *src_off; // n_src + 1 values
    uint32_t n_seqs, n_src, k, max_indel;
    uint64_t total, source_bases;
    bool skip_multi;
    void *events;            // event_capacity records of 16 bytes, 16-byte aligned: appended to behind *n_events
    uint64_t event_capacity;
    uint64_t *n_events;      // grows by the events of the call
    void *work;              // idxindel::event_work(capacity).bytes
};
// three launches, sized by capacity alone (none when capacity is 0): the events of every chunk counted, the counts scanned by one
// workgroup, the records written
hipError_t launch_indel_events(const IndelEventArgs &a, hipStream_t stream);
struct IndelSitesArgs {
    const void *events;      // min(*n_events, event_capacity) records are looked at
    const uint64_t *n_events;
    uint64_t event_capacity;
    const uint32_t *depth;   // source_bases words
    const uint64_t *src_off; // n_src + 1 values
    uint32_t n_src, min_count, frac_num, frac_den;
    uint64_t source_bases, capacity;
    void *sites;             // capacity records of 32 bytes, 16-byte aligned
    uint64_t *n_sites;
    void *work;              // idxindel::site_work(event_capacity).bytes
};
// 7 + 4 * idxindel::sort_passes(source_bases) launches, sized by event_capacity alone (4 when it is 0): the keys, four per radix pass,
// three for the heads, three for the sites
hipError_t launch_indel_sites(const IndelSitesArgs &a, hipStream_t stream);

void set_pair_min_depth(int d);            // tuning: depth from which two-base steps are tried
constexpr uint32_t kRankRows = 96; // rows per 16-byte rank block (== kRankRowsPerBlock)

} // namespace kbo
