// capi_internal.hpp — declarations shared by the translation units behind include/kbo_hip.h:
//   device_index.cpp  the index handle and its per-device copies,
//   host_batch.cpp    host batches: slabs, staging, the three-stage pipeline with one output stage per mode,
//   kbo_capi.cpp      the extern "C" entry points,
//   kbo_tuning.cpp    ... those of include/kbo_hip_tuning.h: knobs, experiment setters, test hooks,
//   device_batch.cpp  ... those over batches already on the device (d_work, kbo_*_dev, kbo_map_stream_*),
//   batch_route.cpp   the kernel route of a batch, for host slabs and device calls alike (batch_route.hpp),
//   build_device.cpp  kbo_index_build_device (the index built by the device),
//   index_locate.cpp  the position table of an index, the segments of a batch and the depth of the sources,
//   index_place.cpp   one placement per sequence from those segments,
//   index_pileup.cpp  allele counts per source base from those segments, and the candidate sites.
#pragma once
#include <atomic>
#include <cstdint>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "host_util.hpp"
#include "kernels.hpp"
#include "refine.hpp"
#include "sbwt_index.hpp"

namespace kbo_host {

struct DevCopy {
    // (an index that serves one small batch borrows its arena from a buffer the calling thread keeps: kbo::call builds
    // one such index per sequence, and a hipMalloc / hipFree pair per sequence serialises every thread of the process)
    bool arena_borrowed = false;
    static bool &transient_arena_in_use()
    {
        static thread_local bool in_use = false;
        return in_use;
    }
    DevBuf arena; // rank blocks of A,C,G,T | null block | contraction entries (32-bit build) | two-base blocks
    DevBuf ent;   // contraction entries as their own allocation (big build)
    uint64_t n_blocks = 0;
    bool big = false;
    uint32_t pair_off = 0; // arena index of the two-base extension blocks, 0 = none
    DevBuf seed_tab;                 // intervals of all strings of seed_d bases (plan_kernel's seeds)
    uint32_t seed_d = 0;
    DevBuf dtab;                     // depth table (dtab_kernels.hip): 4^dtab_order bytes
    uint32_t dtab_order = 0;
    bool dtab_grouped = false;
    DevBuf anchor;                   // anchors of the depth table (kernels.hpp DevIndexView::anchor): 2^anchor_bits slots of 8 bytes
    uint32_t anchor_bits = 0;
    DevBuf fat;                      // recovery lines of the guided walk (sbwt_index.hpp)
    uint32_t fat_null = 0;
    DevBuf pc_text, pc_pos, pc_node; // path cover (sbwt_index.hpp PathCover), empty when the plan-guided walk is off
    DevBuf dfilt;                    // ... and the filter in front of the depth table (dfilt_bases bases per string; small indexes)
    uint32_t dfilt_bases = 0;
    DevBuf pc_tm, seed_pos;          // map_reads_kernel's 2-bit text + marks and its table of seed positions (copies with a depth table)
    DevBuf pc_t, pc_mu, pc_mc;       // ... the text's digits alone, a bit per unit with a mark and the coarse summary of those (map_text.hpp)
    DevBuf sub_clean;                // ... and a bit per text position: a lone substitution there needs no table (map_subst.hpp), for the
    uint32_t sub_thr = 0;            // proof's windows at this threshold - what a call with default options gets on this index -
    bool sub_anch = false;           // with or without anchors
    DevBuf sub_group;                // ... and a bit per group of four positions whose bits are all set: a read's window of them in one load
    DevBuf positions;                // the position table (index_locate.cpp): a word per row, empty without one
    DevBuf src_off;                  // ... and where every source begins (kbo_index::src_off), made with it: what kbo_place_dev bisects
    // what making this copy cost (kbo_index_device_layout): seconds of host work / device builds / uploads, by part
    bool plan_built = false;         // path cover, recovery lines, tables: made by the first use that pays for them (device_index.cpp)
    bool plan_failed = false;        // ... or could not be made (no memory): not tried again on every call; the copy walks plainly
    uint64_t bases_seen = 0;         // bases of the batches that asked for this copy so far (guarded by the index's mutex)
    struct Setup {
        double layout_s = 0, cover_s = 0, lines_s = 0, seed_s = 0, dtab_s = 0, upload_s = 0;
        uint64_t rank_bytes = 0, entry_bytes = 0, pair_bytes = 0, cover_bytes = 0, lines_bytes = 0, seed_bytes = 0, dtab_bytes = 0,
                 anchor_bytes = 0;
    } setup;
    // Plan hold-off of THIS copy (one index on one device): a batch whose reads differ too much from the index gives the
    // plan up on the device; the host learns of it one launch late (asynchronous 8-byte copy into `bailed`, pinned, never
    // waited for) and then skips planning for the next kPlanHoldoff launches over this copy - and over no other.
    struct PlanState {
        std::atomic<int> holdoff{0};
        std::atomic<uint32_t> epoch{0};  // kbo_set_plan(1, ..) generation this state was last reset for
        uint32_t *bailed = nullptr;      // pinned: [0] plan given up, [1] a walk ended by its no-progress guard
        std::atomic<uint32_t> bails{0};  // launches that gave the plan up (inspection / tests)
    } plan;
    ~DevCopy()
    {
        if (plan.bailed) { // (a launch's 8-byte copy into it may still be in flight: plan_after_launch never waits for it)
            int prev = -1;
            (void)hipGetDevice(&prev);
            if (arena.dev >= 0 && arena.dev != prev) (void)hipSetDevice(arena.dev);
            (void)hipDeviceSynchronize();
            if (arena.dev >= 0 && arena.dev != prev && prev >= 0) (void)hipSetDevice(prev);
            (void)hipHostFree(plan.bailed);
        }
        if (arena_borrowed) {
            arena.p = nullptr;
            arena.cap = 0;
            transient_arena_in_use() = false;
        }
    }
};

} // namespace kbo_host

// per-handle options (kbo_index_set_opts, kbo_hip.h): what the process-wide knobs of kbo_hip_tuning.h set for every index, set
// for this one; kOptInherit = follow the process-wide value
constexpr int kOptInherit = INT32_MIN;
struct HandleOpts {
    std::atomic<int> plan{kOptInherit};                // 0 = plain walk only, 1 = plan structures + planned launches
    std::atomic<int> depth_table{kOptInherit};         // as kbo_set_depth_table: 0 by index size, < 0 none, else the order
    std::atomic<int> depth_table_anchors{kOptInherit}; // as kbo_set_depth_table_anchors
    std::atomic<size_t> slab_bytes{0};                 // 0 = inherit
    int n_devices = -1;                                // -1 = inherit (guarded by kbo_index::mu, with `devices`)
    std::vector<int> devices;
};

struct kbo_index {
    kbo::HostIndex host;
    std::mutex mu;
    HandleOpts opts;
    std::map<int, std::unique_ptr<kbo_host::DevCopy>> dev;
    uint64_t rank_bytes = 0, lcs_bytes = 0, plan_bytes = 0;
    bool transient = false; // an index that serves one small batch (kbo::call builds one per sequence): no path cover
    // the path cover of the plan-guided walk once it has been computed (or read from an index file), guarded by `mu`:
    // every device copy uploads it from here, kbo_index_save writes it (laying it out is a 26 s pointer chase per 10^8 rows)
    std::unique_ptr<kbo::PathCover> cover;
    // the position table (kbo_index_add_positions, index_locate.cpp), guarded by `mu`: a word per row, and where every source sequence
    // begins in source coordinates (+ their end); both empty without one.  Device copies keep theirs in DevCopy::positions
    std::vector<uint32_t> positions;
    std::vector<uint64_t> src_off;
    // A SHARDED index (kbo_capi.cpp build_sharded): an index whose rows would not fit 32-bit row numbers (a human genome
    // with its reverse complements: 6.2 * 10^9 rows) is built as several ordinary indexes over disjoint parts of the input -
    // groups of sequences, forward and reverse-complement strands apart - and this handle only holds them: host.k,
    // host.n_kmers (distinct k-mers of the union: what the threshold needs) and host.n_sets (rows over all shards) are set,
    // host.rows / host.lcs are empty.  The depth of the walk against the union index is the maximum of the depths against
    // the shards, so everything that only needs depths (matches / map without refinement / find / ms without intervals)
    // walks every shard and keeps the maximum; what needs rows of the union (intervals, call, fill_gaps, export) is refused.
    std::vector<std::unique_ptr<kbo_index>> shards;
    bool sharded() const { return !shards.empty(); }
};

namespace kbo_host {

// ---- tuning state (set through the kbo_set_* entry points)
extern std::atomic<int> g_waves_per_cu;           // walk: resident waves per CU, 0 = default (32)
extern std::vector<int> g_devices;   // guarded by g_devices_mu: read it through devices_snapshot()
extern std::mutex g_devices_mu;
std::vector<int> devices_snapshot();
// the same knobs as one index sees them (its own options first: HandleOpts)
bool plan_enabled(const kbo_index *idx);
int depth_table_setting(const kbo_index *idx);
int depth_table_anchor_setting(const kbo_index *idx);
size_t slab_bytes_for(const kbo_index *idx);
std::vector<int> devices_for(kbo_index *idx);
//   // devices the host batch entry points spread slabs over (empty = current)
extern std::atomic<bool> g_force_big;             // tests: use the 64-bit-offset entry layout regardless of size
extern std::atomic<uint64_t> g_pair_min_rows;     // indexes with at least this many rows get two-base blocks on the device
extern std::atomic<int> g_host_in_place;         // host batches use a caller's pinned buffers in place instead of staging them (kbo_set_host_in_place)
extern std::atomic<size_t> g_slab_bytes;          // host batches are cut into slabs of at most this many query bytes
extern std::atomic<int> g_plan_cap_div;           // tests: the unit array gets 1/this of its normal capacity
extern std::atomic<int> g_index_shards;           // tests: kbo_index_build makes at least this many shards (0 = by size)
extern std::atomic<bool> g_plan_stats;            // launches of the plan-guided stage count their own work (kbo_set_plan_stats)
extern std::atomic<int> g_depth_table_anchors;    // ... with anchors: -1 by margin, 0 no, 1 yes
extern std::atomic<int> g_depth_table;            // depth table of new device copies: 0 = by index size, < 0 none, else its order
extern std::atomic<int> g_seed_table_depth;       // tests: bases per seed-table entry of new device copies (0 = by index size)
extern std::atomic<bool> g_plan_enabled;          // device copies carry a path cover and MS-only batches take the plan-guided walk
extern std::atomic<uint64_t> g_plan_table_budget; // bytes a copy's tables may take (0 = half of the free device memory)
extern std::atomic<int64_t> g_plan_lazy_bases;    // bases through a copy before it builds its plan structures (-1 = by index size)

// ---- device_index.cpp
int current_device();
inline int resolve_device(int device) { return device < 0 ? current_device() : device; } // (< 0: the calling thread's)
// the copy of the index on `device` (resolved), which must exist; called with idx->mu held
DevCopy &copy_on(kbo_index *idx, int device);
// the indexes a walk goes over: the shards of a sharded handle, else the handle itself
inline std::vector<kbo_index *> shards_of(kbo_index *idx)
{
    std::vector<kbo_index *> v;
    if (idx->sharded()) for (auto &s : idx->shards) v.push_back(s.get());
    else v.push_back(idx);
    return v;
}
// throws KBO_E_UNSUPPORTED for a sharded handle: `what` needs the rows of ONE index
void require_unsharded(const kbo_index *idx, const char *what);
// the rows (4 bit-vectors of ceil(n_sets / 64) words, back to back) and LCS bytes of an index as they already lie on a device
struct DeviceRowsLcs {
    const uint64_t *rows;
    const uint8_t *lcs;
};
// uploads the index on first use; *plan (optional) receives the copy's plan hold-off state.  work_bases: the bases of the batch
// that asks (a copy makes its plan structures - cover, tables - once the bases it has seen pay for them); prepare: make them now.
// built: the index's rows and LCS on `device` already (kbo_index_build_device): the copy is made from them, nothing is uploaded
kbo::DevIndexView device_view(kbo_index *idx, int device, DevCopy::PlanState **plan = nullptr, uint64_t work_bases = 0,
                              bool prepare = false, const DeviceRowsLcs *built = nullptr);
int walk_max_waves();                                     // upper bound on resident walk waves: CUs x waves per CU
// points a.gitems / a.glist into `plan_work` (>= kbo::plan_work_bytes(n_items) bytes, 16-byte aligned) when the index
// view carries a path cover and the launch wants MS values only; otherwise leaves them null (plain walk)
void attach_plan(kbo::WalkArgs &a, void *plan_work, DevCopy::PlanState *ps);
void plan_reset_holdoff(); // every copy plans its next launch again
// after launch_ms_walk: lets the host learn whether the plan paid (and whether a walk was cut short by its guard)
void plan_after_launch(const kbo::WalkArgs &a, hipStream_t stream, DevCopy::PlanState *ps);

// ---- index_locate.cpp: the source offsets of the copy on `dev` as kbo_index_add_positions / kbo_index_positions_to_device left them
// (*n_src: the sources; n_src + 1 values), or null: no positions, or none on that device
const uint64_t *source_offsets_on(kbo_index *idx, int dev, uint32_t *n_src);

// ---- kbo_capi.cpp: shards kbo_index_build makes of `bases` bases (one per 3.76 * 10^9 rows, or kbo_set_index_shards); > 1 = sharded
size_t shards_wanted(uint64_t bases, bool add_revcomp);

// ---- A3 (kbo_capi.cpp): derandomize.rs:91-145
double log_rm_max_cdf(size_t t, size_t alphabet_size, size_t n_kmers);
size_t random_match_threshold(size_t k, size_t n_kmers, size_t alphabet_size, double p);

// ---- host_batch.cpp
struct BatchOnDevice {
    DevBuf q, off, items, ms, lo, hi, plan;
    DevBuf longw; // work of the kernel for sequences of more than 160 bases (long_kernels.hip)
    DevBuf ms_shard; // sharded indexes: the MS values of one further shard, folded into `ms` by maximum
    DevBuf packed, pscr, exc_pos, exc_byte, packed_out, exc_flag; // (exc_flag: one byte per read of a packed-native launch)
    DevBuf raw; // the '-' strand alone: the slab as uploaded (bytes or words); its reverse complement goes where the walk reads
    // packed entry points: 2-bit words in, scanned words per sequence, non-ACGT list, 2-bit words out
    uint64_t total = 0;
    void release()
    {
        for (DevBuf *b : {&q, &off, &items, &ms, &lo, &hi, &plan, &longw, &packed, &pscr, &exc_pos, &exc_byte, &packed_out, &exc_flag, &ms_shard, &raw}) b->release();
    }
};
// a slab of a packed batch (pack_kernels.hip: sequence s = ceil(len / 16) u32 words, 2 bits per base): what
// enqueue_walk_host uploads and unpacks into B.q instead of uploading bytes
struct PackedIn {
    const uint32_t *words;      // the slab's words (host; pinned or staged by the caller)
    size_t n_words;
    const uint64_t *exc_pos;    // non-ACGT bases of the slab: positions in the whole batch's base coordinates, ascending ...
    const uint8_t *exc_byte;    // ... and their bytes
    size_t n_exc;
    uint64_t base;              // the slab's first base in those coordinates
    uint32_t uniform_len;       // != 0: every sequence of the slab has this many bases (offsets are made on the device)
};
struct Slab {
    size_t s0, s1;   // sequences [s0, s1)
    uint64_t b0, b1; // bases [b0, b1)
};
struct OffsetScan { // one pass over the offsets of a batch: order, shortest and longest sequence
    bool monotone = true;
    uint64_t shortest = ~0ull, longest = 0;
};
constexpr size_t kRleWords = 7; // device run-length records are seven u32; kbo_rle has the reference's usize fields
void widen_rles(kbo_rle *dst, const uint32_t *src, size_t n, HostTeam &team);
// how a slab's records, as the device wrote them, become the sink's: as they are, or (kbo_rle) widened
template <typename T> void convert_records(T *dst, const void *src, size_t n, HostTeam &team) { team.copy(dst, src, n * sizeof(T)); }
inline void convert_records(kbo_rle *dst, const void *src, size_t n, HostTeam &team)
{
    widen_rles(dst, static_cast<const uint32_t *>(src), n, team);
}

// ... a few records, on the calling thread
template <typename T> void convert_records(T *dst, const uint32_t *src, size_t n) { std::memcpy(dst, src, n * sizeof(T)); }
inline void convert_records(kbo_rle *dst, const uint32_t *src, size_t n)
{
    for (size_t q = 0; q < n; q++, src += kRleWords) dst[q] = kbo_rle{src[0], src[1], src[2], src[3], src[4], src[5], src[6]};
}

// Where a host batch collects the records of its slabs (kbo_rle: kbo_find_batch, kbo_find_batch_into; kbo_rle32:
// kbo_find_batch_packed; kbo_aln_run: kbo_matches_batch_sparse), in one of two forms.
//   direct:   one worker, slabs complete in order: records are appended to one growing array - or to the caller's buffer
//             (use_buffer), which is never grown and never written past its capacity, while `used` keeps counting;
//   per slab: several workers, slabs complete out of order: kept per slab and put together by take().
template <typename T> struct RecordSink {
    bool direct = false;
    size_t used = 0;   // direct: records of the slabs so far
    GrowBuf<T> all;    // direct: the library's array
    T *fixed = nullptr; // ... or the caller's, of fixed_cap records
    size_t fixed_cap = 0;
    bool caller_owns = false;
    std::vector<std::vector<T>> per_slab;
    std::vector<uint64_t> base; // per slab, set by take(): where each slab's records start in the whole (+ the total)

    void use_buffer(T *buf, size_t capacity)
    {
        caller_owns = true;
        fixed = buf;
        fixed_cap = buf ? capacity : 0;
    }
    void begin(size_t n_slabs, size_t n_seqs, bool direct_)
    {
        direct = direct_;
        used = 0;
        if (!direct) per_slab.assign(n_slabs, {});
        else if (!caller_owns) all.reserve(2 * n_seqs + 1024); // room for 2 runs per sequence to start with (untouched pages cost nothing)
    }
    // the n records of a slab; returns where they start among the batch's (direct form; the other learns it in take())
    size_t append(size_t slab_id, const void *src, size_t n, HostTeam &team)
    {
        if (!direct) {
            per_slab[slab_id].resize(n);
            convert_records(per_slab[slab_id].data(), src, n, team);
            return 0;
        }
        const size_t at = used;
        if (caller_owns) {
            if (at + n <= fixed_cap) convert_records(fixed + at, src, n, team); // a caller's buffer that is too small only gets the count
        } else {
            if (at + n > all.cap) all.reserve((at + n) * 2);
            convert_records(all.p + at, src, n, team);
            all.n = at + n;
        }
        used += n;
        return at;
    }
    // room for the n records of a slab that the caller fills itself (nullptr: a caller's buffer that is too small); *at as append's
    T *place(size_t slab_id, size_t n, size_t *at)
    {
        if (!direct) {
            per_slab[slab_id].resize(n);
            *at = 0;
            return per_slab[slab_id].data();
        }
        *at = used;
        used += n;
        if (caller_owns) return *at + n <= fixed_cap ? fixed + *at : nullptr;
        if (*at + n > all.cap) all.reserve((*at + n) * 2);
        all.n = *at + n;
        return all.p + *at;
    }
    // The batch's records in slab order and their number.  The library's array (malloc'ed, at least one record long, the
    // caller's to free) goes to *out; a caller's buffer stays where it is and holds the records only if all of them fit.
    size_t take(T **out)
    {
        if (direct) {
            if (!caller_owns) {
                all.reserve(1);
                *out = all.release();
            }
            return used;
        }
        base.assign(per_slab.size() + 1, 0);
        for (size_t i = 0; i < per_slab.size(); i++) base[i + 1] = base[i] + per_slab[i].size();
        const size_t total = base.back();
        MallocPtr<T> mine;
        if (!caller_owns) mine = malloc_array<T>(total);
        T *dst = caller_owns ? fixed : mine.get();
        if (!caller_owns || total <= fixed_cap)
            HostTeam::get().run(per_slab.size(), [&](size_t i) {
                if (!per_slab[i].empty()) std::memcpy(dst + base[i], per_slab[i].data(), per_slab[i].size() * sizeof(T));
            });
        if (!caller_owns) *out = mine.release();
        return total;
    }
};

// Where kbo::find over a batch collects format::run_lengths_gapped of every slab (computed on the device from the slab's
// characters, which then never leave it): the records, wide or as the device writes them, and where each sequence's begin
template <typename T> struct RleSink {
    size_t max_gap_len = 0;
    uint64_t *rle_offsets = nullptr; // caller's n_seqs + 1 entries (strands != 0: 2 n_seqs + 1)
    // kbo_find_batch*_strands (KBO_STRAND_*; 0: the single-strand entry points): sequence s has the entries 2 s ('+') and
    // 2 s + 1 ('-'), a strand not asked for has no runs.  With both, a slab arrives as the device ran it - 2 ns sequences, the
    // '-' strands behind the '+' strands (HostStage) - and its records are put in (sequence, strand) order here.
    int strands = 0;
    RecordSink<T> records;
    std::vector<size_t> s0;                   // first sequence of every slab (+ n_seqs)
    std::vector<std::vector<uint32_t>> first; // per slab form: index of the first run of each sequence of the slab, +1 entry

    void begin(const std::vector<Slab> &slabs, size_t n_seqs, bool direct)
    {
        records.begin(slabs.size(), n_seqs, direct);
        s0.clear();
        for (const Slab &sl : slabs) s0.push_back(sl.s0);
        s0.push_back(n_seqs);
        if (!direct) first.assign(slabs.size(), {});
        rle_offsets[0] = 0;
    }
    // A slab's records and the device's scan of its sequences' run counts as it leaves the device: n + 1 indices within
    // blocks of 1024 sequences, then the blocks' sums.
    void append(size_t slab_id, const void *src, size_t n_records, const uint32_t *local, HostTeam &team)
    {
        const size_t ns = s0[slab_id + 1] - s0[slab_id];
        if (strands) return append_strands(slab_id, src, n_records, local, team);
        const uint32_t *sums = local + ns + 1;
        const size_t at = records.append(slab_id, src, n_records, team);
        if (records.direct) {
            set_offsets(slab_id, at, [&](size_t q) { return (uint64_t)sums[q / 1024] + local[q]; }, team);
        } else {
            first[slab_id].resize(ns + 1);
            for (size_t q = 0; q <= ns; q++) first[slab_id][q] = sums[q / 1024] + local[q];
        }
    }
    size_t take(T **out)
    {
        const size_t total = records.take(out);
        if (!records.direct)
            for (size_t i = 0; i < first.size(); i++)
                set_offsets(i, records.base[i], [&](size_t q) { return (uint64_t)first[i][q]; }, HostTeam::get());
        return total;
    }

private:
    void append_strands(size_t slab_id, const void *src, size_t n_records, const uint32_t *local, HostTeam &team)
    {
        const size_t ns = s0[slab_id + 1] - s0[slab_id], dn = strands == 3 ? 2 * ns : ns; // sequences: the caller's / the device's
        const uint32_t *sums = local + dn + 1;
        auto first_run = [&](size_t q) { return sums[q / 1024] + local[q]; };
        const uint32_t fwd_runs = strands == 3 ? first_run(ns) : 0;
        // where the runs of (sequence q, strand) begin within the slab's: entries 2 q and 2 q + 1, + the end
        std::vector<uint32_t> lo(2 * ns + 1);
        const size_t piece = 1u << 14, n_tasks = (ns + piece - 1) / piece;
        team.run(n_tasks, [&](size_t t) {
            for (size_t q = t * piece; q < std::min(ns, (t + 1) * piece); q++) {
                if (strands == 3) {
                    const uint32_t rev = first_run(ns + q) - fwd_runs;
                    lo[2 * q] = first_run(q) + rev;
                    lo[2 * q + 1] = first_run(q + 1) + rev;
                } else {
                    lo[2 * q] = first_run(q);
                    lo[2 * q + 1] = strands == 1 ? first_run(q + 1) : first_run(q);
                }
            }
        });
        lo[2 * ns] = (uint32_t)n_records;
        size_t at = 0;
        if (strands != 3) {
            at = records.append(slab_id, src, n_records, team);
        } else if (T *dst = records.place(slab_id, n_records, &at)) {
            const uint32_t *rec = static_cast<const uint32_t *>(src);
            team.run(n_tasks, [&](size_t t) {
                for (size_t q = t * piece; q < std::min(ns, (t + 1) * piece); q++) {
                    const uint32_t f0 = first_run(q), nf = first_run(q + 1) - f0, r0 = first_run(ns + q), nr = first_run(ns + q + 1) - r0;
                    if (nf) convert_records(dst + lo[2 * q], rec + (size_t)f0 * kRleWords, nf);
                    if (nr) convert_records(dst + lo[2 * q + 1], rec + (size_t)r0 * kRleWords, nr);
                }
            });
        }
        if (records.direct) set_offsets(slab_id, at, [&](size_t q) { return (uint64_t)lo[q]; }, team);
        else first[slab_id] = std::move(lo);
    }
    // rle_offsets of a slab's sequences: the slab's base + the index of the sequence's first run within the slab
    template <typename First> void set_offsets(size_t slab_id, uint64_t slab_base, First first_run, HostTeam &team)
    {
        const size_t per = strands ? 2 : 1, at = per * s0[slab_id], ns = per * (s0[slab_id + 1] - s0[slab_id]), piece = 1u << 15;
        team.run((ns + piece - 1) / piece, [&](size_t t) {
            const size_t a = t * piece + 1, b = std::min(ns, a + piece - 1);
            for (size_t q = a; q <= b; q++) rle_offsets[at + q] = slab_base + first_run(q);
        });
    }
};

uint32_t max_len(const uint64_t *offsets, size_t n_seqs);
uint64_t walk_chunk(uint64_t total, size_t n_seqs, uint32_t k);
void check_batch(const void *concat, const uint64_t *offsets, size_t n_seqs);
void check_len_threshold(const uint64_t *offsets, size_t n_seqs, size_t k, size_t threshold);
OffsetScan scan_offsets(const uint64_t *offsets, size_t n_seqs);
std::vector<Slab> make_slabs(const uint64_t *offsets, size_t n_seqs, size_t max_bytes);
size_t packed_slab_bytes(const kbo_index *idx); // bases per slab of a packed batch
// upload + A1 over a host batch (asynchronous on `stream`); leaves ms (and lo/hi) on the device.
// `items_keep` must stay alive until the stream has been synchronised.
// call mode of the walk (kernels.hpp WalkArgs::call_*): where the sites go
struct CallSink {
    void *d_sites;        // kCallSegs lists of cap_per_list 16-byte records
    uint32_t *d_counts;   // kCallSegs counters 64 bytes apart + the overflow counter behind them, zeroed by ms_batch_dev_impl once the call is accepted
    uint32_t cap_per_list;
    uint32_t threshold;
};
// what the caller wants behind the walk (kbo::matches / map): when the slab is a batch of reads over a copy with a depth table,
// enqueue_walk_host runs map_reads_kernel (map_kernels.hip) - characters straight into d_chars, no MS values in memory - and
// sets `done`; otherwise it leaves the MS values in B.ms as ever and the caller runs A5 / A6
struct FusedMap {
    uint8_t *d_chars;   // >= total + 16 bytes
    uint32_t threshold;
    bool format;        // + format::relative_to_ref
    bool want_ms = false; // the MS values go to memory as well (the device calls)
    bool done = false;
    // a packed batch whose characters leave packed as well: where their words go (nw words + 16 bytes); packed_done = the kernel
    // wrote them there itself (its packed-native form), else the characters are in d_chars as for any batch
    uint32_t *d_packed_out = nullptr;
    bool packed_done = false;
    // kbo::find with max_gap_len = 0: where the number of runs of every sequence goes (rle scratch, n_seqs + 1 words); counted = the
    // one kernel (and, for the reads of its second pass, derand_flagged_kernel) filled it: scan + emit are what is left
    uint32_t *run_counts = nullptr;
    bool counted = false;
    // kbo_summary_batch[_packed]: where the sequences' records go (n_seqs x 16 bytes); summarized = the one kernel's summary form and
    // its second pass wrote them and no character was made, else the characters are in d_chars for the reducer (summary_kernels.hip)
    uint4 *d_summary = nullptr;
    bool summarized = false;
    hipStream_t ts = nullptr; // done: where the route left the result complete (batch_route.hpp route_map)
};
// Strands of a host batch (kbo_*_batch_strands) and the count of what it uploads.  strands = KBO_STRAND_FWD: the slab as it is;
// KBO_STRAND_REV: its reverse complement, made on the device from the uploaded slab; both: the slab DOUBLED on the device -
// `offsets` / `n_seqs` (and a packed slab's uniform_len) then describe 2 n sequences, n .. 2n-1 the reverse complements of
// 0 .. n-1 behind them, of which only the first half - bases or words, exceptions, offsets, items - is uploaded (concat,
// PackedIn::words / n_words / n_exc are that half) and the rest is made by revcomp_kernels.hip.
struct HostStage {
    int strands = 1;
    std::atomic<uint64_t> *staged = nullptr; // += bytes of every host -> device copy
};
// what a caller of enqueue_walk_host asks for beyond the walk of the batch as it is; each sets the fields it means
struct WalkHostAsk {
    bool want_ival = false;            // the intervals as well (B.lo, B.hi)
    uint32_t longest = 0;              // longest sequence if the caller knows it
    hipStream_t copy_stream = nullptr; // uploads go here when given ...
    hipEvent_t copied = nullptr;       // ... and `stream` waits for this event
    const CallSink *call = nullptr;    // call mode: MS values + sites, no intervals
    const PackedIn *packed = nullptr;  // the queries arrive 2-bit packed (concat is not read)
    FusedMap *map = nullptr;           // kbo::matches / map: the one kernel where it applies
    const HostStage *stage = nullptr;  // strands, upload count
};
void enqueue_walk_host(kbo_index *idx, const uint8_t *concat, const uint64_t *offsets, size_t n_seqs, BatchOnDevice &B,
                       std::vector<kbo::WalkItem> &items_keep, hipStream_t stream, const WalkHostAsk &ask = {});
void run_walk_host(kbo_index *idx, const uint8_t *concat, const uint64_t *offsets, size_t n_seqs, bool want_ival,
                   BatchOnDevice &B, hipStream_t stream);
// A5+A6 over a batch whose offsets are known on the host
void derand_translate_host_offsets(const uint8_t *d_ms, const uint64_t *d_off, const uint64_t *offsets, size_t n_seqs,
                                   uint32_t k, uint32_t threshold, const uint8_t *d_ref, uint8_t *d_chars,
                                   int32_t *d_derand, hipStream_t stream, uint32_t longest = 0,
                                   DevBuf *piece_work = nullptr /* lets long reads / contigs be split into pieces */);
// what leaves the device for a slab of a host batch ...
enum class OutMode {
    Ms,     // kbo_ms_batch: the MS values (and the intervals, when lo / hi are given)
    Chars,  // kbo_matches_batch, kbo_map_batch: one character per base
    Words,  // kbo_matches_batch_packed: the characters as 2-bit words
    Rle,    // kbo_find_batch, kbo_find_batch_into: run-length records, widened to kbo_rle
    Rle32,  // kbo_find_batch_packed: run-length records as the device writes them
    Sparse, // kbo_matches_batch_sparse: the runs of characters other than 'M'
    Summary, // kbo_summary_batch, kbo_summary_batch_packed: one kbo_aln_summary per sequence, the characters stay on the device
};
// ... and where it goes: made by the maker of its mode, which sets that mode's destination and no other
struct HostOut {
    OutMode mode;
    uint8_t *ms_out = nullptr;                      // Ms ...
    uint32_t *lo_out = nullptr, *hi_out = nullptr;  // ... with the intervals when these are given
    uint8_t *chars_out = nullptr, *chars_rev = nullptr;    // Chars: the '+' strand (or the one strand as given) and the '-' strand ...
    bool format = false;                                   // ... with format::relative_to_ref applied
    uint32_t *packed_out = nullptr, *packed_rev = nullptr; // Words: the same
    RleSink<kbo_rle> *rle = nullptr;                // Rle
    RleSink<kbo_rle32> *rle32 = nullptr;            // Rle32
    RecordSink<kbo_aln_run> *sparse_runs = nullptr; // Sparse
    kbo_aln_summary *summary_out = nullptr;         // Summary: n_seqs records

    static HostOut ms(uint8_t *d, uint32_t *lo, uint32_t *hi) { HostOut o{OutMode::Ms}; o.ms_out = d; o.lo_out = lo; o.hi_out = hi; return o; }
    static HostOut chars(uint8_t *fwd, uint8_t *rev, bool format) { HostOut o{OutMode::Chars}; o.chars_out = fwd; o.chars_rev = rev; o.format = format; return o; }
    static HostOut words(uint32_t *fwd, uint32_t *rev) { HostOut o{OutMode::Words}; o.packed_out = fwd; o.packed_rev = rev; return o; }
    static HostOut runs(RleSink<kbo_rle> *sink) { HostOut o{OutMode::Rle}; o.rle = sink; return o; }
    static HostOut runs32(RleSink<kbo_rle32> *sink) { HostOut o{OutMode::Rle32}; o.rle32 = sink; return o; }
    static HostOut sparse(RecordSink<kbo_aln_run> *sink) { HostOut o{OutMode::Sparse}; o.sparse_runs = sink; return o; }
    static HostOut summary(kbo_aln_summary *out) { HostOut o{OutMode::Summary}; o.summary_out = out; return o; }
    bool takes_strands() const { return mode == OutMode::Chars || mode == OutMode::Words || mode == OutMode::Rle || mode == OutMode::Rle32; }
    // the destinations of a batch run in `strands` (KBO_STRAND_*) are there
    bool complete(int strands) const
    {
        const void *fwd = mode == OutMode::Chars ? (const void *)chars_out : packed_out, *rev = mode == OutMode::Chars ? (const void *)chars_rev : packed_rev;
        if (mode == OutMode::Chars || mode == OutMode::Words) return (fwd || !(strands & 1)) && (rev || !(strands & 2));
        return ms_out || rle || rle32 || sparse_runs || summary_out;
    }
};
// kbo::matches over a batch (lib.rs:618-627) into HostOut::chars (optional relative_to_ref, lib.rs:756-757), ::runs (the characters
// are turned into run lengths on the device instead of being downloaded, lib.rs:816-820) or ::summary.  strands = 0: one strand as
// given; else KBO_STRAND_*
void matches_batch_impl(kbo_index *idx, const uint8_t *concat, const uint64_t *offsets, size_t n_seqs, double max_error_prob,
                        const HostOut &out, int strands = 0);
// the same over 2-bit packed reads (pack_kernels.hip layout) with the non-ACGT bases in a side list, into HostOut::words (the characters
// 2-bit packed as well: M, -, X, R = 0 .. 3), ::runs32, ::sparse (their runs other than 'M') or ::summary
struct PackedBatch {
    const uint32_t *words;
    const uint64_t *exc_pos;
    const uint8_t *exc_byte;
    size_t n_exc;
};
void summary_slab_routes(uint64_t *kernel_slabs, uint64_t *reducer_slabs);
void matches_batch_packed_impl(kbo_index *idx, const PackedBatch &in, const uint64_t *offsets, size_t n_seqs, double max_error_prob,
                               const HostOut &out, int strands = 0);
// host -> device bytes the calling thread's last host batch staged (kbo_last_batch_staged_bytes)
extern thread_local uint64_t t_last_staged;
// A1 over a host batch: MS values, and intervals when lo/hi are given
void ms_batch_impl(kbo_index *idx, const uint8_t *concat, const uint64_t *offsets, size_t n_seqs, uint8_t *d_out,
                   uint32_t *lo_out, uint32_t *hi_out);
void release_host_scratch(); // frees the pooled per-device scratch of the host batch entry points + the calling thread's caches
void release_transient_arena();     // device_index.cpp: the calling thread's arena for transient indexes (when not in use)

} // namespace kbo_host
