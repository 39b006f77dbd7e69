// refset.cpp — kbo_refset_t (N one-sequence indexes in one packed device layout) and kbo_find_refset (kbo_hip.h "find against a
// set of references").  The walk is refset_kernels.hip's.  A slab of (reference, sequence, strand) pairs is laid out
// pair by pair and looks like an ordinary batch to what follows: derandomize_ms_vec / translate_ms_vec with a threshold per pair
// (derand_seq_kernels.hip: the pair's reference's), then the single-index pipeline's run_lengths_gapped kernels as they are.
// kbo_summary_refset shares the slabs, the upload, the '-' strand and the walk; behind the walk it runs the counting form of the
// derandomize / translate stage and keeps the pairs with a hit on the device: no characters, no run-length stage.
// kbo_best_refset shares all of that up to the extents and merges them, slab by slab, into a table of one record per sequence on the
// device (refset_best_kernels.hip): no record stage, nothing read back until the last slab is enqueued.
// A set built with a prefilter (kbo_refset_build_opts) carries a seed table (refset_screen.hpp); the host forms then mark the pairs
// that share a seed with one kernel over the uploaded batch (refset_screen_kernels.hip), read the bitmap back, and plan, upload and
// walk only the marked pairs.  kbo_refset_candidates is that screen alone, kbo_refset_candidates_host its restatement on the CPU.
// A set built with positions carries one entry per row of every packed reference (refset_locate.hpp); kbo_locate_refset turns the
// runs of a find into anchors on the references with one kernel (refset_locate_kernels.hip), kbo_locate_refset_host on the CPU.
// Such a set also carries one base offset per reference (refset_cover.hpp); kbo_cover_refset counts every anchor of the runs on the
// base its entry names and reduces along each reference to its depth and breadth (refset_cover_kernels.hip), kbo_cover_refset_host
// on the CPU.
// kbo_call_refset runs the first pass of kbo::call behind the summary's stages of every slab (refset_call.hpp;
// refset_call_kernels.hip): the sites and their windows come back, and the host resolves them as call_batch.cpp resolves a site left
// to it - one suffix automaton per (sequence, strand) with a site.  kbo_call_refset_host is the same pipeline on the CPU.
#include "../../include/kbo_hip_tuning.h"
#include "capi_internal.hpp"
#include "refset_best.hpp"
#include "refset_call.hpp"
#include "refset_cand.hpp"
#include "refset_cover.hpp"
#include "refset_locate.hpp"
#include "refset_screen.hpp"
#include "refset_step.hpp"
#include "run_automaton.hpp"

#include <algorithm>
#include <thread>

using namespace kbo_host;

static_assert(kbo::kRefsetChunk == KBO_REFSET_CHUNK && kbo::kRefsetMaxRows == KBO_REFSET_MAX_ROWS, "kbo_hip_tuning.h states the kernel's constants");
static_assert(kbo::kRefsetWideMaxRows == KBO_REFSET_WIDE_MAX_ROWS && kbo::kRefsetRouteLds == KBO_REFSET_ROUTE_LDS &&
                  kbo::kRefsetRouteIndex == KBO_REFSET_ROUTE_INDEX && kbo::kRefsetRouteWide == KBO_REFSET_ROUTE_WIDE,
              "kbo_hip.h states the wide walk's constants");

static_assert(kbo::refscreen::kSeedMax == KBO_REFSET_SEED_MAX && kbo::refscreen::kSeedMin == KBO_REFSET_SEED_MIN &&
                  kbo::kRefsetScreenRun == KBO_REFSET_SCREEN_RUN && kbo::kRefsetScreenThreads == KBO_REFSET_SCREEN_THREADS,
              "the headers state the screen's constants");
static_assert(kbo::reflocate::kPosNone == KBO_POS_NONE && kbo::reflocate::kPosNone == KBO_LOCUS_NONE && kbo::reflocate::kMulti == KBO_LOCUS_MULTI &&
                  sizeof(kbo_ref_locus) == 24 && sizeof(kbo_ref_locus) == sizeof(kbo::reflocate::Locus),
              "kbo_hip.h states the position table's constants and the six words of a locus");
static_assert(sizeof(kbo_ref_cover) == 48 && sizeof(kbo_ref_cover) == sizeof(kbo::refcover::Cover) && KBO_COVER_NO_ENTRIES == kbo::refcover::kFlagNoEntries &&
                  KBO_COVER_OVERFLOW == kbo::refcover::kFlagOverflow,
              "kbo_hip.h states the twelve words of a cover and its flags");
static_assert(sizeof(kbo_refset_opts) == sizeof(size_t) + 8, "kbo_refset_opts: positions lies in what was the struct's tail padding");

namespace {
constexpr uint64_t kPrefilterMaxBits = 1ull << 31; // the bitmap is read back: above this many bits a call runs unscreened
std::atomic<size_t> g_record_capacity{1u << 16};
std::atomic<uint64_t> g_prefilter_max_bits{kPrefilterMaxBits};
thread_local uint64_t t_pre[4] = {0, 0, 0, 0}; // pairs of packed references, with their bit set, walked; the screen ran
thread_local uint64_t t_routes[4] = {0, 0, 0, 0};
thread_local uint64_t t_wide[2] = {0, 0}; // references walked by the wide kernel, the tasks it was launched with
thread_local uint64_t t_best[2] = {0, 0}; // launches of refset_best_kernel: a wave per sequence, a workgroup per sequence
thread_local uint64_t t_call[4] = {0, 0, 0, 0}; // kbo_call_refset: pairs scanned, candidates, sites, variants

struct DevSet {
    DevBuf arena, descs;
    DevBuf pre_bucket, pre_keys, pre_refs; // the seed table of a set with a prefilter
    DevBuf pos, pos_off;                   // the position table of a set with positions, and where each reference's entries begin
    DevBuf cov;                            // ... and its base offsets (n_refs + 1 u64), then every reference's length (n_refs u32)
};

struct DeviceScope { // the calling thread on `device` until the scope ends
    int prev = -1;
    bool moved = false;
    explicit DeviceScope(int device)
    {
        HIP_OK(hipGetDevice(&prev));
        if (device >= 0 && device != prev) {
            HIP_OK(hipSetDevice(device));
            moved = true;
        }
    }
    ~DeviceScope()
    {
        if (moved) (void)hipSetDevice(prev);
    }
};

struct StreamScope {
    hipStream_t s = nullptr;
    StreamScope() { HIP_OK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking)); }
    ~StreamScope()
    {
        if (s) {
            (void)hipStreamSynchronize(s);
            (void)hipStreamDestroy(s);
        }
    }
};
} // namespace

struct kbo_refset {
    uint32_t k = 0;
    std::vector<kbo::RefsetDesc> descs;
    std::vector<uint32_t> arena;                  // the packed forms (LDS and wide references) back to back, four words a unit
    std::vector<std::unique_ptr<kbo_index>> own;  // per reference: its ordinary index when it takes the single-index route, else null
    // the seed table of a set built with a prefilter (refset_screen.hpp): bucket offsets, then the entries sorted by key
    bool prefilter = false;
    std::vector<uint32_t> pre_bucket, pre_refs;
    std::vector<uint64_t> pre_keys;
    // the position table of a set built with positions (refset_locate.hpp): one entry per row of every packed reference that can be
    // queried, reference r's from pos_off[r] on (n_refs + 1 offsets)
    bool positions = false;
    std::vector<uint32_t> pos;
    std::vector<uint64_t> pos_off;
    std::vector<uint64_t> ref_len; // every reference's length as given
    // the base offsets of a set built with positions (refset_cover.hpp): reference r's bases of the depth profile from cov_off[r] on,
    // none for a reference without entries (n_refs + 1 offsets)
    std::vector<uint64_t> cov_off;
    std::mutex mu;
    std::map<int, DevSet *> dev;
    ~kbo_refset()
    {
        for (auto &kv : dev) delete kv.second;
    }
};

namespace {

// the packed form of an index of any number of rows below 2^32 - 32 (kernels.hpp "LDS form"), appended to `arena`
void append_lds_form(const kbo::HostIndex &h, std::vector<uint32_t> &arena)
{
    const uint32_t n = (uint32_t)h.n_sets, nb = n / 32u + 1u;
    const size_t at = arena.size(), nw = h.rows[0].size();
    arena.resize(at + 4u * (size_t)kbo::refset_units(n), 0u);
    uint32_t *rank = arena.data() + at;
    uint32_t cum[4] = {(uint32_t)h.C[0], (uint32_t)h.C[1], (uint32_t)h.C[2], (uint32_t)h.C[3]};
    for (uint32_t b = 0; b < nb; b++)
        for (uint32_t c = 0; c < 4; c++) {
            const size_t w = b >> 1;
            const uint32_t bits = w < nw ? (uint32_t)(h.rows[c][w] >> (32u * (b & 1u))) : 0u;
            rank[(b * 4u + c) * 2u] = cum[c];
            rank[(b * 4u + c) * 2u + 1u] = bits;
            cum[c] += (uint32_t)__builtin_popcount(bits);
        }
    uint8_t *lcs = reinterpret_cast<uint8_t *>(rank + 4u * (size_t)kbo::refset_rank_units(n));
    std::memcpy(lcs, h.lcs.data(), n);
    lcs[0] = 0;
    lcs[n] = 0; // the sentinel that ends the contraction's scan upwards
}

DevSet *device_set(kbo_refset *set, int device)
{
    std::lock_guard<std::mutex> g(set->mu);
    auto it = set->dev.find(device);
    if (it != set->dev.end()) return it->second;
    DeviceScope on(device);
    std::unique_ptr<DevSet> d(new DevSet());
    d->arena.alloc(set->arena.size() * sizeof(uint32_t) + 16);
    d->descs.alloc(set->descs.size() * sizeof(kbo::RefsetDesc));
    if (!set->arena.empty()) HIP_OK(hipMemcpy(d->arena.p, set->arena.data(), set->arena.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d->descs.p, set->descs.data(), set->descs.size() * sizeof(kbo::RefsetDesc), hipMemcpyHostToDevice));
    if (set->prefilter) {
        const size_t n = set->pre_keys.size();
        d->pre_bucket.alloc(set->pre_bucket.size() * sizeof(uint32_t));
        d->pre_keys.alloc(n * sizeof(uint64_t));
        d->pre_refs.alloc(n * sizeof(uint32_t));
        HIP_OK(hipMemcpy(d->pre_bucket.p, set->pre_bucket.data(), set->pre_bucket.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
        if (n) {
            HIP_OK(hipMemcpy(d->pre_keys.p, set->pre_keys.data(), n * sizeof(uint64_t), hipMemcpyHostToDevice));
            HIP_OK(hipMemcpy(d->pre_refs.p, set->pre_refs.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice));
        }
    }
    if (set->positions) {
        d->pos.alloc(set->pos.size() * sizeof(uint32_t) + 16);
        d->pos_off.alloc(set->pos_off.size() * sizeof(uint64_t));
        if (!set->pos.empty()) HIP_OK(hipMemcpy(d->pos.p, set->pos.data(), set->pos.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
        HIP_OK(hipMemcpy(d->pos_off.p, set->pos_off.data(), set->pos_off.size() * sizeof(uint64_t), hipMemcpyHostToDevice));
        const size_t n_refs = set->descs.size();
        std::vector<uint32_t> lens(set->ref_len.begin(), set->ref_len.end()); // (below 2^30 each: kbo_refset_build_opts)
        d->cov.alloc((n_refs + 1) * sizeof(uint64_t) + n_refs * sizeof(uint32_t));
        HIP_OK(hipMemcpy(d->cov.p, set->cov_off.data(), (n_refs + 1) * sizeof(uint64_t), hipMemcpyHostToDevice));
        HIP_OK(hipMemcpy(d->cov.as<uint8_t>() + (n_refs + 1) * sizeof(uint64_t), lens.data(), n_refs * sizeof(uint32_t), hipMemcpyHostToDevice));
    }
    set->dev[device] = d.get();
    return d.release();
}

// the pairs of a slab, their chunks and the workgroups' tasks, as they go to the device
struct SlabPlan {
    std::vector<uint32_t> ref, seq, strand, thr; // per pair; thr: its reference's threshold
    std::vector<uint64_t> off;              // per pair + 1: its first byte in the slab
    std::vector<uint32_t> items, tasks;     // four words a record (kernels.hpp RefsetWalkArgs)
    uint32_t longest = 0, lds_units = 0; // lds_units: the largest form among the slab's LDS references
    bool has_lds = false, has_wide = false; // the kinds of reference the slab's tasks name
    void clear()
    {
        ref.clear(); seq.clear(); strand.clear(); thr.clear(); items.clear(); tasks.clear();
        off.assign(1, 0);
        longest = 0;
        lds_units = 0;
        has_lds = has_wide = false;
    }
    size_t pairs() const { return ref.size(); }
    uint64_t bytes() const { return off.back(); }
};

// A slab's uploads through pinned memory, two sets in turn: a walker that synchronises nothing per slab (Bester) plans the next
// slab while the device runs this one, and the slab's host arrays are free to change as soon as run_slab returns.  A set is taken
// again only when the copies out of it have run (its event).
struct SlabStage {
    PinBuf pin[2];
    hipEvent_t ev[2] = {nullptr, nullptr};
    bool used[2] = {false, false};
    size_t at = 0;
    int cur = 1;
    static size_t room(size_t bytes) { return (bytes + 15) / 16 * 16; }
    void begin(size_t bytes)
    {
        cur ^= 1;
        if (!ev[cur]) HIP_OK(hipEventCreateWithFlags(&ev[cur], hipEventDisableTiming));
        if (used[cur]) HIP_OK(hipEventSynchronize(ev[cur]));
        pin[cur].ensure(bytes);
        at = 0;
    }
    const void *put(const void *src, size_t bytes)
    {
        KBO_REQUIRE(at + bytes <= pin[cur].cap, KBO_E_HIP, "slab stage overrun");
        uint8_t *dst = pin[cur].as<uint8_t>() + at;
        if (bytes) std::memcpy(dst, src, bytes);
        at += room(bytes);
        return dst;
    }
    void end(hipStream_t st)
    {
        HIP_OK(hipEventRecord(ev[cur], st));
        used[cur] = true;
    }
    ~SlabStage()
    {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
};

// what kbo_find_refset, kbo_summary_refset and kbo_best_refset share: the batch on the device, slabs of pairs and their walk
struct SlabWalker {
    kbo_refset *set;
    SlabStage *stage = nullptr; // where the slab's arrays are copied from when they may change before the copies have run
    const uint64_t *offsets;
    uint32_t k, chunk, min_thr; // min_thr: the smallest threshold of the references that take a walk of the packed form
    uint64_t rev_base; // where the '-' strand of the batch begins in d_q
    hipStream_t st;
    DevSet *ds;
    DevBuf d_q, d_off, d_ms, d_poff, d_pthr, d_items, d_tasks, d_derand;
    std::vector<uint64_t> ref_begin, ref_end; // where every reference's records lie in the call's list
    std::vector<uint8_t> walked;              // per reference: a launch of its walk kernel has held it (the route counters)

    void add_pair(SlabPlan &P, uint32_t r, uint32_t s, uint32_t strand, uint32_t threshold)
    {
        const uint64_t len = offsets[s + 1] - offsets[s], q0 = (strand == KBO_STRAND_REV ? rev_base : 0) + offsets[s], o0 = P.bytes();
        bool fresh = P.tasks.empty() || P.tasks[P.tasks.size() - 4] != r;
        for (uint64_t c0 = 0; c0 < len; c0 += chunk) {
            const uint64_t c1 = std::min(len, c0 + chunk), warm = std::min<uint64_t>(c0, k - 1);
            if (fresh || P.tasks[P.tasks.size() - 2] == kbo::kRefsetThreads) {
                const uint32_t t[4] = {r, (uint32_t)(P.items.size() / 4), 0u, 0u};
                P.tasks.insert(P.tasks.end(), t, t + 4);
                fresh = false;
            }
            const uint32_t it[4] = {(uint32_t)(q0 + c0 - warm), (uint32_t)(o0 + c0), (uint32_t)(c1 - c0 + warm) | (uint32_t)warm << 16, 0u};
            P.items.insert(P.items.end(), it, it + 4);
            P.tasks[P.tasks.size() - 2]++;
        }
        P.ref.push_back(r);
        P.seq.push_back(s);
        P.strand.push_back(strand);
        P.thr.push_back(threshold);
        P.off.push_back(o0 + len);
        P.longest = std::max<uint32_t>(P.longest, (uint32_t)len);
        if (set->descs[r].route == kbo::kRefsetRouteWide) P.has_wide = true;
        else {
            P.has_lds = true;
            P.lds_units = std::max(P.lds_units, kbo::refset_units(set->descs[r].n_sets));
        }
    }

    // the slab's pairs, thresholds and tasks to the device, and the walk: the MS bytes of every pair in d_ms
    void walk_slab(const SlabPlan &P)
    {
        const size_t np = P.pairs();
        d_ms.ensure(slab_buffer_bytes(P));
        d_poff.ensure((np + 1) * sizeof(uint64_t));
        d_pthr.ensure(np * sizeof(uint32_t));
        d_derand.ensure(kbo::derand_seq_work_bytes((uint32_t)np, P.bytes(), k, min_thr));
        d_items.ensure(P.items.size() * sizeof(uint32_t));
        d_tasks.ensure(P.tasks.size() * sizeof(uint32_t));
        upload(d_poff.p, P.off.data(), (np + 1) * sizeof(uint64_t));
        upload(d_pthr.p, P.thr.data(), np * sizeof(uint32_t));
        upload(d_items.p, P.items.data(), P.items.size() * sizeof(uint32_t));
        upload(d_tasks.p, P.tasks.data(), P.tasks.size() * sizeof(uint32_t));
        kbo::RefsetWalkArgs a;
        a.descs = ds->descs.as<kbo::RefsetDesc>();
        a.arena = ds->arena.as<uint4>();
        a.tasks = d_tasks.as<uint4>();
        a.items = d_items.as<uint4>();
        a.n_tasks = (uint32_t)(P.tasks.size() / 4);
        a.k = k;
        a.q = d_q.as<uint8_t>();
        a.ms = d_ms.as<uint8_t>();
        if (P.has_lds) HIP_OK(kbo::launch_refset_walk(a, P.lds_units, st)); // (each kernel skips the other's tasks)
        if (P.has_wide) {
            HIP_OK(kbo::launch_refset_wide_walk(a, st));
            t_wide[1] += a.n_tasks;
        }
        for (size_t p = 0; p < np; p++)
            if (!walked[P.ref[p]]) {
                walked[P.ref[p]] = 1;
                if (set->descs[P.ref[p]].route == kbo::kRefsetRouteWide) t_wide[0]++;
                else t_routes[0]++;
            }
        t_routes[2] += np;
    }
    static size_t slab_buffer_bytes(const SlabPlan &P) { return ((size_t)P.bytes() + 15) / 16 * 16 + 64; }
    void upload(void *dst, const void *src, size_t bytes)
    {
        HIP_OK(hipMemcpyAsync(dst, stage ? stage->put(src, bytes) : src, bytes, hipMemcpyHostToDevice, st));
    }
    // what walk_slab puts into the stage
    static size_t stage_bytes(const SlabPlan &P)
    {
        return SlabStage::room((P.pairs() + 1) * sizeof(uint64_t)) + SlabStage::room(P.pairs() * sizeof(uint32_t)) +
               SlabStage::room(P.items.size() * sizeof(uint32_t)) + SlabStage::room(P.tasks.size() * sizeof(uint32_t));
    }
};

struct Finder : SlabWalker {
    uint32_t gap;
    DevBuf d_chars, d_scratch, d_total, d_rles;
    size_t rle_capacity = 0;
    std::vector<uint32_t> first, recs;
    std::vector<kbo_ref_run> out;

    // walk, derandomize + translate, run lengths of one slab; its records behind those of the slabs so far
    void run_slab(const SlabPlan &P)
    {
        const size_t np = P.pairs();
        if (!np) return;
        d_chars.ensure(slab_buffer_bytes(P));
        const size_t scratch_words = kbo::chunk_items_scratch_words((uint32_t)np);
        d_scratch.ensure(scratch_words * sizeof(uint32_t));
        d_total.ensure(16);
        walk_slab(P);
        HIP_OK(kbo::launch_derand_translate_seq(d_ms.as<uint8_t>(), d_poff.as<uint64_t>(), (uint32_t)np, P.bytes(), k, d_pthr.as<uint32_t>(), min_thr,
                                                nullptr, d_chars.as<uint8_t>(), d_derand.p, st));
        HIP_OK(kbo::launch_rle_count(d_chars.as<uint8_t>(), d_poff.as<uint64_t>(), (uint32_t)np, gap, d_scratch.as<uint32_t>(),
                                     d_total.as<uint32_t>(), st, P.longest, true));
        uint32_t total = 0;
        first.resize(scratch_words);
        HIP_OK(hipMemcpyAsync(&total, d_total.p, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        HIP_OK(hipMemcpyAsync(first.data(), d_scratch.p, scratch_words * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
        if (!rle_capacity) {
            rle_capacity = g_record_capacity.load();
            d_rles.ensure(rle_capacity * kRleWords * sizeof(uint32_t));
        }
        if (total > rle_capacity) { // (the count is known before anything is emitted: room for all of them, and some to spare)
            rle_capacity = (size_t)total + total / 4 + 16;
            d_rles.ensure(rle_capacity * kRleWords * sizeof(uint32_t));
        }
        if (total) {
            HIP_OK(kbo::launch_rle_emit(d_chars.as<uint8_t>(), d_poff.as<uint64_t>(), (uint32_t)np, gap, d_scratch.as<uint32_t>(),
                                        d_rles.as<uint32_t>(), (uint32_t)rle_capacity, st, P.longest, true));
            recs.resize((size_t)total * kRleWords);
            HIP_OK(hipMemcpyAsync(recs.data(), d_rles.p, recs.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
            HIP_OK(hipStreamSynchronize(st));
        }
        const uint32_t *sums = first.data() + np + 1;
        auto first_run = [&](size_t p) { return (size_t)sums[p / 1024] + first[p]; };
        for (size_t p = 0; p < np; p++) {
            const uint32_t r = P.ref[p];
            if (ref_begin[r] == ~0ull) ref_begin[r] = out.size();
            for (size_t x = first_run(p); x < first_run(p + 1); x++) {
                const uint32_t *w = recs.data() + x * kRleWords;
                out.push_back(kbo_ref_run{r, P.seq[p], P.strand[p], kbo_rle32{w[0], w[1], w[2], w[3], w[4], w[5], w[6]}});
            }
            ref_end[r] = out.size();
        }
        t_routes[3]++;
    }
};

struct Summarizer : SlabWalker {
    DevBuf d_ext, d_scratch, d_kept, d_total;
    std::vector<uint32_t> kept;
    std::vector<kbo_ref_summary> out;

    // walk, the counting form of derandomize + translate, the pairs with a hit kept: one count and those records come back
    void run_slab(const SlabPlan &P)
    {
        const size_t np = P.pairs();
        if (!np) return;
        d_ext.ensure(np * sizeof(kbo_aln_extent));
        d_scratch.ensure(kbo::chunk_items_scratch_words((uint32_t)np) * sizeof(uint32_t));
        d_kept.ensure(np * 7 * sizeof(uint32_t));
        d_total.ensure(16);
        walk_slab(P);
        HIP_OK(kbo::launch_derand_summary_seq(d_ms.as<uint8_t>(), d_poff.as<uint64_t>(), (uint32_t)np, P.bytes(), k, d_pthr.as<uint32_t>(), min_thr,
                                              d_ext.as<uint32_t>(), d_derand.p, st));
        HIP_OK(kbo::launch_refset_keep(d_ext.as<uint32_t>(), (uint32_t)np, d_scratch.as<uint32_t>(), d_kept.as<uint32_t>(), d_total.as<uint32_t>(), st));
        uint32_t total = 0;
        HIP_OK(hipMemcpyAsync(&total, d_total.p, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
        kept.resize((size_t)total * 7);
        if (total) { // (nothing runs in between: a copy, not a second pass)
            HIP_OK(hipMemcpyAsync(kept.data(), d_kept.p, kept.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
            HIP_OK(hipStreamSynchronize(st));
        }
        size_t x = 0;
        for (size_t p = 0; p < np; p++) { // (every pair of the slab, so that a reference without a hit still has its place)
            const uint32_t r = P.ref[p];
            if (ref_begin[r] == ~0ull) ref_begin[r] = out.size();
            if (x < total && kept[7 * x] == p) {
                const uint32_t *w = kept.data() + 7 * x + 1;
                out.push_back(kbo_ref_summary{r, P.seq[p], P.strand[p], kbo_aln_extent{w[0], w[1], w[2], w[3], w[4], w[5]}});
                x++;
            }
            ref_end[r] = out.size();
        }
        t_routes[3]++;
    }
};

// kbo_best_refset: the extents of a slab merged into the call's table where they are.  Nothing is read back and nothing waited for:
// the slab's arrays go through the stage, the device buffers are the stream's in order (one that grows is freed by hipFree, which
// waits for the device's work), and the table comes back once, behind the last slab.
struct Bester : SlabWalker {
    SlabStage pinned;
    DevBuf d_ext, d_refs, d_table;
    std::vector<uint32_t> refs; // the slab's references, in order
    uint32_t n_seqs = 0, n_strands = 0, strands = 0;

    void run_slab(const SlabPlan &P)
    {
        const size_t np = P.pairs();
        if (!np) return;
        refs.clear();
        for (size_t p = 0; p < np; p++)
            if (refs.empty() || refs.back() != P.ref[p]) refs.push_back(P.ref[p]);
        d_ext.ensure(np * sizeof(kbo_aln_extent));
        d_refs.ensure(refs.size() * sizeof(uint32_t));
        stage = &pinned;
        pinned.begin(stage_bytes(P) + SlabStage::room(refs.size() * sizeof(uint32_t)));
        walk_slab(P);
        upload(d_refs.p, refs.data(), refs.size() * sizeof(uint32_t));
        pinned.end(st);
        HIP_OK(kbo::launch_derand_summary_seq(d_ms.as<uint8_t>(), d_poff.as<uint64_t>(), (uint32_t)np, P.bytes(), k, d_pthr.as<uint32_t>(), min_thr,
                                              d_ext.as<uint32_t>(), d_derand.p, st));
        kbo::RefsetBestArgs a;
        a.ext = d_ext.as<uint32_t>();
        a.refs = d_refs.as<uint32_t>();
        a.table = d_table.as<uint32_t>();
        a.n_pairs = (uint32_t)np;
        // run_slabs adds the pairs in (reference, sequence, strand) order: the slab begins this far into its first reference
        a.lead = P.seq[0] * n_strands + (strands == 3 ? P.strand[0] - 1u : 0u);
        a.slab_refs = (uint32_t)refs.size();
        a.n_seqs = n_seqs;
        a.n_strands = n_strands;
        a.strands = strands;
        HIP_OK(kbo::launch_refset_best(a, st));
        t_best[kbo::refset_best_splits(n_seqs) ? 1 : 0]++;
        t_routes[3]++;
    }
};

// the threshold of every reference that can be queried (lib.rs:620); the errors of kbo_find on its handle
std::vector<uint32_t> refset_thresholds(const kbo_refset *set, double max_error_prob)
{
    KBO_REQUIRE(max_error_prob <= 1.0 && max_error_prob > 0.0, KBO_E_BAD_ARG, "0 < max_error_prob <= 1 (derandomize.rs:136-137)");
    std::vector<uint32_t> thr(set->descs.size(), 0);
    for (size_t r = 0; r < thr.size(); r++) {
        if (set->descs[r].status) continue;
        thr[r] = (uint32_t)random_match_threshold(set->k, set->descs[r].n_kmers, 4, max_error_prob);
        KBO_REQUIRE(thr[r] > 1, KBO_E_THRESHOLD_LE_1, "threshold > 1 (derandomize.rs:275, translate.rs:269)");
    }
    return thr;
}

// the checks on the batch, all before the first HIP call; its bases
uint64_t check_refset_batch(const kbo_refset *set, const uint8_t *concat, const uint64_t *offsets, size_t n_seqs)
{
    check_batch(concat, offsets, n_seqs);
    check_len_threshold(offsets, n_seqs, set->k, 2);
    const uint64_t total = offsets[n_seqs];
    KBO_REQUIRE(total < (1ull << 31), KBO_E_UNSUPPORTED, "a batch of 2^31 bases or more");
    return total;
}

// the batch to the device, once; its '-' strand behind it, made where it is
void upload_batch(SlabWalker &F, kbo_refset *set, const uint8_t *concat, const uint64_t *offsets, size_t n_seqs, uint64_t total, int strands,
                  hipStream_t stream)
{
    const size_t n_refs = set->descs.size();
    F.set = set;
    F.offsets = offsets;
    F.k = set->k;
    F.chunk = std::max<uint32_t>(kbo::kRefsetChunk, 4u * set->k);
    F.rev_base = (total + 15) / 16 * 16;
    F.ds = device_set(set, current_device());
    F.ref_begin.assign(n_refs, ~0ull);
    F.ref_end.assign(n_refs, 0);
    F.walked.assign(n_refs, 0);
    F.st = stream;
    F.d_q.alloc(2 * F.rev_base + 64);
    F.d_off.alloc((n_seqs + 1) * sizeof(uint64_t));
    HIP_OK(hipMemsetAsync(F.d_q.p, 0, 2 * F.rev_base + 64, F.st));
    HIP_OK(hipMemcpyAsync(F.d_q.p, concat, total, hipMemcpyHostToDevice, F.st));
    HIP_OK(hipMemcpyAsync(F.d_off.p, offsets, (n_seqs + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, F.st));
    if (strands & KBO_STRAND_REV)
        HIP_OK(kbo::launch_revcomp_bytes(F.d_q.as<uint8_t>(), F.d_off.as<uint64_t>(), (uint32_t)n_seqs, total, F.d_q.as<uint8_t>() + F.rev_base, F.st));
}


// ---- the seed screen (refset_screen.hpp; refset_screen_kernels.hip)
struct HostTable { // refset_screen.hpp's accessor over the set's host table
    const kbo_refset *set;
    uint32_t bucket(uint32_t b) const { return set->pre_bucket[b]; }
    uint64_t key(uint32_t x) const { return set->pre_keys[x]; }
    uint32_t ref(uint32_t x) const { return set->pre_refs[x]; }
};

// the reverse complement as revcomp_kernels.hip makes it: A <-> T, C <-> G in either case, any other byte as it is
void revcomp_host(const uint8_t *fwd, size_t len, std::vector<uint8_t> &out)
{
    out.resize(len);
    for (size_t i = 0; i < len; i++) {
        const uint8_t b = fwd[len - 1 - i], u = b & 0xDFu;
        out[i] = u == 'A' || u == 'T' ? b ^ ('A' ^ 'T') : (u == 'C' || u == 'G' ? b ^ ('C' ^ 'G') : b);
    }
}

bool packed_ok(const kbo::RefsetDesc &d) { return !d.status && d.route != kbo::kRefsetRouteIndex; }

struct HostForm { // refset_step.hpp's accessor over the host arena
    const uint32_t *rank_;
    const uint8_t *lcs_;
    kbo::refstep::Entry rank(uint32_t block, uint32_t c) const
    {
        const uint32_t *e = rank_ + ((size_t)block * 4u + c) * 2u;
        return kbo::refstep::Entry{e[0], e[1]};
    }
    uint32_t lcs(uint32_t i) const { return lcs_[i]; }
};
HostForm host_form(const kbo_refset *set, const kbo::RefsetDesc &d)
{
    const uint32_t *form = set->arena.data() + (size_t)d.off * 4u;
    return HostForm{form, reinterpret_cast<const uint8_t *>(form + 4u * (size_t)kbo::refset_rank_units(d.n_sets))};
}

// ---- the position table (refset_locate.hpp): every indexed stretch of every packed reference that can be queried - the stretches
// build_prefilter enumerates - walked through the reference's own packed form with the walk's step; at depth k the interval is the
// one row of the k-mer that ends there.  With add_revcomp the stretch's reverse complement too: its k-mers are REV occurrences
void build_positions(kbo_refset *set, const uint8_t *const *seqs, const size_t *lens, bool add_revcomp, uint32_t num_threads)
{
    namespace lc = kbo::reflocate;
    const size_t n_refs = set->descs.size();
    const uint32_t k = set->k;
    set->pos_off.assign(n_refs + 1, 0);
    for (size_t r = 0; r < n_refs; r++) set->pos_off[r + 1] = set->pos_off[r] + (packed_ok(set->descs[r]) ? set->descs[r].n_sets : 0u);
    set->pos.assign((size_t)set->pos_off[n_refs], lc::kPosNone);
    set->cov_off.assign(n_refs + 1, 0);
    for (size_t r = 0; r < n_refs; r++) set->cov_off[r + 1] = set->cov_off[r] + (packed_ok(set->descs[r]) ? lens[r] : 0u);
    std::atomic<size_t> next{0};
    std::atomic<bool> bad{false};
    auto work = [&] {
        std::vector<uint8_t> rc;
        for (size_t r; (r = next.fetch_add(1)) < n_refs;) {
            const kbo::RefsetDesc &d = set->descs[r];
            if (!packed_ok(d)) continue;
            const HostForm x = host_form(set, d);
            uint32_t *entries = set->pos.data() + set->pos_off[r];
            // b: a stretch (or its reverse complement) of n bases; the window [s, s + k) of it is the occurrence at p0 + s / p0 - s
            auto add_stretch = [&](const uint8_t *b, size_t n, size_t p0, bool rev) {
                uint32_t lo = 0, hi = d.n_sets, depth = 0;
                for (size_t i = 0; i < n; i++) {
                    kbo::refstep::step(x, d.n_sets, k, b[i], lo, hi, depth);
                    if (i + 1 < k) continue;
                    if (depth != k || hi - lo != 1u) { // (an indexed k-mer has exactly one row)
                        bad = true;
                        return;
                    }
                    const size_t s = i + 1 - k;
                    entries[lo] = lc::entry_merge(entries[lo], lc::entry_of((uint32_t)(rev ? p0 - s : p0 + s), rev));
                }
            };
            const uint8_t *q = seqs[r];
            for (size_t i = 0, n = lens[r]; i < n;) {
                if (kbo::refstep::base_code(q[i]) > 3u) {
                    i++;
                    continue;
                }
                size_t j = i;
                while (j < n && kbo::refstep::base_code(q[j]) <= 3u) j++;
                if (j - i >= k) {
                    add_stretch(q + i, j - i, i, false);
                    if (add_revcomp) { // window s of the reverse complement covers [j - s - k, j - s) of the reference
                        rc.resize(j - i);
                        for (size_t y = 0; y < j - i; y++) rc[y] = (uint8_t)"TGCA"[kbo::refstep::base_code(q[j - 1 - y])];
                        add_stretch(rc.data(), rc.size(), j - k, true);
                    }
                }
                i = j;
            }
        }
    };
    std::vector<std::thread> team;
    for (uint32_t t = 1; t < std::min<size_t>(num_threads, n_refs); t++) team.emplace_back(work);
    work();
    for (auto &t : team) t.join();
    // (the walk contradicts the index it walks: what building or querying such a reference alone cannot do either)
    KBO_REQUIRE(!bad.load(), KBO_E_UNSUPPORTED, "positions: an indexed k-mer without a row of its own in the reference's packed form");
    set->positions = true;
}

// One entry per start position of every indexed stretch (a maximal run of bases of at least k, as build_host_index sees them; its
// reverse complement too with add_revcomp) of every packed reference that can be queried, sorted by key, and the bucket offsets
void build_prefilter(kbo_refset *set, const uint8_t *const *seqs, const size_t *lens, bool add_revcomp)
{
    namespace sc = kbo::refscreen;
    std::vector<std::pair<uint64_t, uint32_t>> entries;
    std::vector<uint8_t> rc;
    auto add_stretch = [&](const uint8_t *b, size_t n, uint32_t r) { // right to left: the seed at i is base i in front of the one at i + 1
        sc::Seed seed{0u, 0u};
        for (size_t i = n; i-- > 0;) {
            seed = sc::step_left(seed, b[i]);
            entries.emplace_back(sc::key_of(seed), r);
        }
    };
    for (size_t r = 0; r < set->descs.size(); r++) {
        if (!packed_ok(set->descs[r])) continue;
        const uint8_t *q = seqs[r];
        for (size_t i = 0, n = lens[r]; i < n;) {
            if (kbo::refstep::base_code(q[i]) > 3u) {
                i++;
                continue;
            }
            size_t j = i;
            while (j < n && kbo::refstep::base_code(q[j]) <= 3u) j++;
            if (j - i >= set->k) {
                add_stretch(q + i, j - i, (uint32_t)r);
                if (add_revcomp) {
                    rc.resize(j - i);
                    for (size_t x = 0; x < j - i; x++) rc[x] = (uint8_t)"TGCA"[kbo::refstep::base_code(q[j - 1 - x])];
                    add_stretch(rc.data(), rc.size(), (uint32_t)r);
                }
            }
            i = j;
        }
    }
    KBO_REQUIRE(entries.size() < 0xFFFFFFFFull, KBO_E_UNSUPPORTED, "the set's seed table exceeds 2^32 - 1 entries");
    std::sort(entries.begin(), entries.end());
    set->pre_bucket.assign((size_t)sc::kBuckets + 1, 0u);
    set->pre_keys.resize(entries.size());
    set->pre_refs.resize(entries.size());
    for (size_t x = 0; x < entries.size(); x++) {
        set->pre_keys[x] = entries[x].first;
        set->pre_refs[x] = entries[x].second;
        set->pre_bucket[(size_t)sc::bucket_of(entries[x].first >> 16) + 1]++;
    }
    for (size_t b = 0; b < sc::kBuckets; b++) set->pre_bucket[b + 1] += set->pre_bucket[b];
    set->prefilter = true;
}

// the bitmap of a call: bit (r * n_seqs + s) * 2 + strand - 1
struct Screen {
    size_t n_seqs = 0;
    std::vector<uint32_t> bits;
    bool test(size_t r, size_t s, uint32_t strand) const
    {
        const uint64_t b = ((uint64_t)r * n_seqs + s) * 2u + (strand - 1u);
        return bits[b >> 5] >> (b & 31u) & 1u;
    }
    void set_bit(size_t r, size_t s, uint32_t strand)
    {
        const uint64_t b = ((uint64_t)r * n_seqs + s) * 2u + (strand - 1u);
        bits[b >> 5] |= 1u << (b & 31u);
    }
    uint64_t count() const
    {
        uint64_t n = 0;
        for (uint32_t w : bits) n += (uint64_t)__builtin_popcount(w);
        return n;
    }
};

uint64_t screen_bits(const kbo_refset *set, size_t n_seqs) { return (uint64_t)set->descs.size() * n_seqs * 2u; }

// m_r of every reference for this call's thresholds; 0: the reference is not packed or cannot be queried (it has no entries)
std::vector<uint8_t> seed_lens(const kbo_refset *set, const std::vector<uint32_t> &thr)
{
    std::vector<uint8_t> m(set->descs.size(), 0);
    for (size_t r = 0; r < m.size(); r++)
        if (packed_ok(set->descs[r])) m[r] = (uint8_t)kbo::refscreen::seed_len(thr[r], set->k);
    return m;
}

// a packed reference whose m_r does not reach a bucket's bases cannot be screened: all its pairs of the strands asked for are candidates
void mark_unfilterable(const std::vector<uint8_t> &m, int strands, Screen &scr)
{
    for (size_t r = 0; r < m.size(); r++) {
        if (m[r] == 0 || m[r] >= kbo::refscreen::kSeedMin) continue;
        for (size_t s = 0; s < scr.n_seqs; s++)
            for (uint32_t strand = 1; strand <= 2; strand++)
                if (strands & strand) scr.set_bit(r, s, strand);
    }
}

// the screen kernel over the batch upload_batch put on the device; the bitmap comes back (one copy, one wait)
void run_screen(SlabWalker &F, const std::vector<uint32_t> &thr, size_t n_seqs, uint64_t total, int strands, Screen &scr)
{
    const kbo_refset *set = F.set;
    const size_t n_refs = set->descs.size(), words = (size_t)((screen_bits(set, n_seqs) + 31) / 32);
    const std::vector<uint8_t> m = seed_lens(set, thr);
    std::vector<uint8_t> dev_m(n_refs);
    for (size_t r = 0; r < n_refs; r++) dev_m[r] = m[r] >= kbo::refscreen::kSeedMin ? m[r] : (uint8_t)kbo::refscreen::kUnfilterable;
    DevBuf d_bits(words * sizeof(uint32_t)), d_m(n_refs);
    HIP_OK(hipMemsetAsync(d_bits.p, 0, words * sizeof(uint32_t), F.st));
    HIP_OK(hipMemcpyAsync(d_m.p, dev_m.data(), n_refs, hipMemcpyHostToDevice, F.st));
    kbo::RefsetScreenArgs a;
    a.bucket = F.ds->pre_bucket.as<uint32_t>();
    a.keys = F.ds->pre_keys.as<uint64_t>();
    a.refs = F.ds->pre_refs.as<uint32_t>();
    a.m = d_m.as<uint8_t>();
    a.q = F.d_q.as<uint8_t>();
    a.off = F.d_off.as<uint64_t>();
    a.bits = d_bits.as<uint32_t>();
    a.total = total;
    a.rev_base = F.rev_base;
    a.n_seqs = (uint32_t)n_seqs;
    a.strands = (uint32_t)strands;
    a.first_strand = strands == 2 ? 2u : 1u;
    HIP_OK(kbo::launch_refset_screen(a, F.st));
    scr.n_seqs = n_seqs;
    scr.bits.assign(words, 0u);
    HIP_OK(hipMemcpyAsync(scr.bits.data(), d_bits.p, words * sizeof(uint32_t), hipMemcpyDeviceToHost, F.st));
    HIP_OK(hipStreamSynchronize(F.st));
    mark_unfilterable(m, strands, scr);
}

// what a host call does behind upload_batch: the counters of kbo_refset_last_prefilter, and the screen when the set has a prefilter
// and the bitmap is within the cap.  Returns the screen run_slabs goes by, or null: every pair.
const Screen *screen_call(SlabWalker &F, const std::vector<uint32_t> &thr, size_t n_seqs, uint64_t total, int strands, Screen &scr)
{
    const kbo_refset *set = F.set;
    uint64_t packed = 0;
    for (const kbo::RefsetDesc &d : set->descs) packed += packed_ok(d);
    std::fill(t_pre, t_pre + 4, 0);
    t_pre[0] = packed * n_seqs * (strands == 3 ? 2u : 1u);
    if (!set->prefilter || screen_bits(set, n_seqs) > g_prefilter_max_bits.load()) return nullptr;
    run_screen(F, thr, n_seqs, total, strands, scr);
    t_pre[1] = scr.count();
    t_pre[3] = 1;
    return &scr;
}

// the checks kbo_refset_candidates and its host form share, all before any work; the thresholds
std::vector<uint32_t> check_candidates(const kbo_refset_t *set, const uint8_t *concat, const uint64_t *offsets, size_t n_seqs,
                                       double max_error_prob, int strands, const uint32_t *bits_out, uint64_t *total)
{
    KBO_REQUIRE(strands >= 1 && strands <= 3, KBO_E_BAD_ARG, "strands: KBO_STRAND_FWD, KBO_STRAND_REV or both");
    KBO_REQUIRE(set && bits_out, KBO_E_BAD_ARG, "null argument");
    KBO_REQUIRE(set->prefilter, KBO_E_BAD_ARG, "the set has no prefilter (kbo_refset_build_opts)");
    std::vector<uint32_t> thr = refset_thresholds(set, max_error_prob);
    *total = check_refset_batch(set, concat, offsets, n_seqs);
    KBO_REQUIRE(screen_bits(set, n_seqs) <= kPrefilterMaxBits, KBO_E_UNSUPPORTED, "a bitmap of more than 2^31 bits");
    return thr;
}

// the references of the packed form, LDS and wide: every pair carries its reference's threshold, so a slab is cut by the budget alone
// With a screen (a set with a prefilter), only the pairs whose bit is set: the slabs are cut by the candidates alone, a reference
// none of whose pairs is one appears in no slab, and a call without a candidate runs no slab at all.
template <typename F> void run_slabs(F &f, const std::vector<uint32_t> &thr, size_t n_seqs, int strands, const Screen *screen)
{
    const kbo_refset *set = f.set;
    const size_t n_refs = set->descs.size();
    const uint64_t budget = slab_bytes_for(nullptr);
    f.min_thr = set->k;
    for (size_t r = 0; r < n_refs; r++)
        if (!set->descs[r].status && set->descs[r].route != kbo::kRefsetRouteIndex) f.min_thr = std::min(f.min_thr, thr[r]);
    SlabPlan P;
    P.clear();
    for (size_t r = 0; r < n_refs; r++) {
        if (set->descs[r].status || set->descs[r].route == kbo::kRefsetRouteIndex) continue;
        for (size_t s = 0; s < n_seqs; s++)
            for (uint32_t strand = 1; strand <= 2; strand++) {
                if (!(strands & strand)) continue;
                if (screen && !screen->test(r, s, strand)) continue;
                t_pre[2]++;
                const uint64_t len = f.offsets[s + 1] - f.offsets[s];
                if (P.pairs() && P.bytes() + len > budget) {
                    f.run_slab(P);
                    P.clear();
                }
                f.add_pair(P, (uint32_t)r, (uint32_t)s, strand, thr[r]);
            }
    }
    f.run_slab(P);
}

// the call's list: every reference's records, in the order of the references
template <typename T> T *gather_by_ref(const SlabWalker &F, const std::vector<T> &out, uint64_t *n)
{
    MallocPtr<T> res = malloc_array<T>(out.size());
    size_t at = 0;
    for (size_t r = 0; r < F.ref_begin.size(); r++) {
        if (F.ref_begin[r] == ~0ull) continue;
        std::copy(out.begin() + F.ref_begin[r], out.begin() + F.ref_end[r], res.get() + at);
        at += F.ref_end[r] - F.ref_begin[r];
    }
    *n = at;
    return res.release();
}

// kbo_aln_extent of one sequence's characters (the references that take the single-index pipeline)
kbo_aln_extent extent_of_chars(const uint8_t *c, uint64_t len)
{
    kbo_aln_extent e{0, 0, 0, 0, 0, 0};
    bool in_run = false;
    for (uint64_t i = 0; i < len; i++) {
        const bool hit = c[i] != '-';
        e.n_match += c[i] == 'M';
        e.n_mismatch += c[i] == 'X';
        e.n_jump += c[i] == 'R';
        if (hit) {
            if (!in_run) e.n_runs++;
            if (!e.end) e.start = (uint32_t)i;
            e.end = (uint32_t)i + 1;
        }
        in_run = hit;
    }
    return e;
}

// ---- the device-resident form (kbo_find_refset_dev / kbo_summary_refset_dev / kbo_best_refset_dev): the same stages enqueued on the
// caller's stream over the caller's work buffer.  A slab is a range of queryable references against the whole batch, planned on the
// device (refset_plan_kernels.hip); nothing comes back to the host.
enum DevKind { kDevSummary, kDevFind, kDevBest };
struct DevForm {
    kbo::refplan::Geometry g;
    uint32_t n_refs = 0, n_q = 0, max_refs = 0, refs = 0; // references of the set, queryable ones, the most a slab may hold, a slab's
    uint64_t local_cap = 0;                               // records of the slab-local buffer (find)
    // per call ...
    size_t q = 0, nch = 0, qflag = 0, qref = 0, thr = 0;
    // ... and per slab
    size_t poff = 0, pthr = 0, items = 0, tasks = 0, ms = 0, chars = 0, derand = 0, stage = 0, first = 0, local = 0, total = 0, end = 0;
    bool ok = false; // false: a limit of the kernels is exceeded even with one reference per slab
};

size_t up16(size_t b) { return (b + 15) / 16 * 16; }

// the layout of d_work for slabs of refs_per_slab references (0: as many as a slab may hold; more than that: that many)
DevForm dev_form(const kbo_refset *set, size_t n_seqs, uint64_t total, int strands, size_t capacity, size_t refs_per_slab, DevKind kind)
{
    const bool find = kind == kDevFind;
    DevForm F;
    if (!set || n_seqs == 0 || strands < 1 || strands > 3) return F;
    for (const kbo::RefsetDesc &d : set->descs)
        if (!d.status && d.route == kbo::kRefsetRouteIndex) return F; // (the call refuses the set)
    const uint64_t ns = strands == 3 ? 2 : 1;
    if (n_seqs * ns >= (1ull << 28) || n_seqs >= (1ull << 28) || ns * total >= (1ull << 32) - 16) return F;
    if (ns * kbo::refplan::chunks_bound(total, n_seqs, kbo::refplan::chunk_of(set->k)) > 0xFFFFFF00ull) return F;
    F.g = kbo::refplan::geometry(n_seqs, total, strands, set->k);
    F.n_refs = (uint32_t)set->descs.size();
    for (const kbo::RefsetDesc &d : set->descs) F.n_q += !d.status;
    // what a slab may hold: its bytes and item slots index with 32 bits, its pairs are the sequences of the stages behind the walk
    uint64_t most = std::max<uint32_t>(F.n_q, 1);
    if (total) most = std::min<uint64_t>(most, ((1ull << 32) - 17) / (ns * total));
    most = std::min<uint64_t>(most, ((1ull << 28) - 1) / (n_seqs * ns));
    most = std::min<uint64_t>(most, 0xFFFFFF00ull / F.g.item_slots);
    F.max_refs = (uint32_t)most;
    const uint64_t R = F.refs = (uint32_t)(refs_per_slab == 0 ? most : std::min<uint64_t>(refs_per_slab, most));
    const uint64_t B = R * ns * total, np = R * n_seqs * ns;
    const size_t rev = (size_t)(total + 15) / 16 * 16;
    size_t w = 0;
    F.q = w;      w += strands == 1 ? 0 : (strands == 3 ? 2 * rev : rev) + 64;
    F.nch = w;    w += up16(kbo::chunk_items_scratch_words((uint32_t)n_seqs) * sizeof(uint32_t));
    F.qflag = w;  w += up16(kbo::chunk_items_scratch_words(F.n_refs) * sizeof(uint32_t));
    F.qref = w;   w += up16((size_t)F.n_refs * sizeof(uint32_t));
    F.thr = w;    w += up16((size_t)F.n_refs * sizeof(uint32_t));
    F.total = w;  w += 16;
    F.poff = w;   w += up16((size_t)(np + 1) * sizeof(uint64_t));
    F.pthr = w;   w += up16((size_t)np * sizeof(uint32_t));
    F.items = w;  w += (size_t)R * F.g.item_slots * sizeof(uint4);
    F.tasks = w;  w += (size_t)R * F.g.tasks_per_ref * sizeof(uint4);
    F.ms = w;     w += up16((size_t)B) + 64;
    // (the thresholds depend on max_error_prob, which the figure does not know: room for the lowest one there is)
    F.derand = w; w += up16(kbo::derand_seq_work_bytes((uint32_t)np, B, set->k, 2));
    if (find) {
        F.local_cap = std::min<uint64_t>(capacity, B / 2 + np); // (a run holds a character other than '-' and ends at one)
        F.chars = w; w += up16((size_t)B) + 64;
        F.stage = w; w += up16(kbo::rle_seg_work_bytes((uint32_t)np, B));
        F.first = w; w += up16((size_t)(np + 1) * sizeof(uint32_t));
        F.local = w; w += up16((size_t)F.local_cap * kRleWords * sizeof(uint32_t));
    } else {
        F.chars = w; w += up16((size_t)np * sizeof(kbo_aln_extent));                                     // the extents
        if (kind == kDevSummary) { // (best: the extents are merged into the caller's table where they are)
            F.stage = w; w += up16(kbo::chunk_items_scratch_words((uint32_t)np) * sizeof(uint32_t));      // launch_refset_keep's scan
            F.local = w; w += up16((size_t)np * 7 * sizeof(uint32_t));                                   // the kept list
        }
    }
    F.end = w;
    F.ok = true;
    return F;
}

struct DevCall {
    kbo_refset *set;
    const uint8_t *d_concat;
    const uint64_t *d_offsets;
    size_t n_seqs;
    uint64_t total_bases;
    double max_error_prob;
    uint32_t gap;
    int strands;
    void *d_work;
    size_t work_bytes;
    void *d_out;
    size_t capacity;
    uint64_t *d_n;
    hipStream_t stream;
};

DevSet *device_set_if_any(kbo_refset *set, int device)
{
    std::lock_guard<std::mutex> g(set->mu);
    auto it = set->dev.find(device);
    return it == set->dev.end() ? nullptr : it->second;
}

// (best: c.d_out is the table of n_seqs records, there is no capacity and the count the planner zeroes lies in d_work)
void run_dev_form(const DevCall &c, DevKind kind)
{
    const bool find = kind == kDevFind, best = kind == kDevBest;
    KBO_REQUIRE(c.strands >= 1 && c.strands <= 3, KBO_E_BAD_ARG, "strands: KBO_STRAND_FWD, KBO_STRAND_REV or both");
    KBO_REQUIRE(c.set && c.d_concat && c.d_offsets && c.d_work && (c.d_n || best) && (c.d_out || (c.capacity == 0 && !best)), KBO_E_BAD_ARG,
                "null argument");
    KBO_REQUIRE(((uintptr_t)c.d_concat & 15) == 0 && ((uintptr_t)c.d_work & 15) == 0 && ((uintptr_t)c.d_offsets & 7) == 0 &&
                    ((uintptr_t)c.d_n & 7) == 0 && ((uintptr_t)c.d_out & 3) == 0,
                KBO_E_BAD_ARG, "d_concat and d_work 16-byte, d_offsets and the count 8-byte, the records 4-byte aligned");
    KBO_REQUIRE(c.n_seqs > 0, KBO_E_EMPTY_QUERY, "empty batch");
    kbo_refset *set = c.set;
    const std::vector<uint32_t> thr = refset_thresholds(set, c.max_error_prob);
    for (const kbo::RefsetDesc &d : set->descs)
        KBO_REQUIRE(d.status || d.route != kbo::kRefsetRouteIndex, KBO_E_UNSUPPORTED,
                    "a reference of the single-index route: the host calls take it (kbo_refset_packed_only)");
    DevForm F = dev_form(set, c.n_seqs, c.total_bases, c.strands, c.capacity, 1, kind);
    KBO_REQUIRE(F.ok, KBO_E_UNSUPPORTED, "a slab of one reference of 2^32 - 16 bytes or more, or 2^28 (sequence, strand) pairs or more");
    KBO_REQUIRE(c.work_bytes >= F.end, KBO_E_BAD_ARG, "work_bytes too small for one reference a slab");
    uint32_t lo = 1, hi = F.max_refs; // the largest refs_per_slab whose figure fits: the figure is monotonic
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo + 1) / 2;
        if (dev_form(set, c.n_seqs, c.total_bases, c.strands, c.capacity, mid, kind).end <= c.work_bytes) lo = mid;
        else hi = mid - 1;
    }
    F = dev_form(set, c.n_seqs, c.total_bases, c.strands, c.capacity, lo, kind);
    DevSet *ds = device_set_if_any(set, current_device());
    KBO_REQUIRE(ds, KBO_E_BAD_ARG, "the set has no copy on the current device (kbo_refset_to_device)");

    uint32_t min_thr = set->k;
    std::vector<uint32_t> qrefs;
    for (size_t r = 0; r < thr.size(); r++)
        if (!set->descs[r].status) {
            min_thr = std::min(min_thr, thr[r]);
            qrefs.push_back((uint32_t)r);
        }
    hipStream_t st = c.stream;
    uint8_t *w = static_cast<uint8_t *>(c.d_work);
    auto at = [&](size_t o) { return reinterpret_cast<uint32_t *>(w + o); };
    // the walk addresses ONE query buffer: the caller's for '+' alone, the '-' strand made here, or a copy of '+' with '-' behind it
    const uint8_t *q = c.strands == 1 ? c.d_concat : w + F.q;
    HIP_OK(hipMemcpyAsync(w + F.thr, thr.data(), thr.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    if (c.strands == 3 && c.total_bases) HIP_OK(hipMemcpyAsync(w + F.q, c.d_concat, c.total_bases, hipMemcpyDeviceToDevice, st));
    if (c.strands & KBO_STRAND_REV)
        HIP_OK(kbo::launch_revcomp_bytes(c.d_concat, c.d_offsets, (uint32_t)c.n_seqs, c.total_bases, w + F.q + F.g.rev_base, st));
    kbo::RefsetPlan P;
    P.g = F.g;
    P.off = c.d_offsets;
    P.thr = at(F.thr);
    P.nch = at(F.nch);
    P.nch_sums = at(F.nch) + c.n_seqs + 1;
    P.qref = at(F.qref);
    uint64_t *d_n = best ? reinterpret_cast<uint64_t *>(w + F.total) : c.d_n;
    HIP_OK(kbo::launch_refset_plan_call(P, F.n_refs, at(F.nch), at(F.qflag), at(F.qref), d_n, st));
    if (best) {
        HIP_OK(kbo::launch_refset_best_init(static_cast<uint32_t *>(c.d_out), (uint32_t)c.n_seqs, st));
        std::fill(t_best, t_best + 2, 0);
    }
    if (c.total_bases == 0) return; // (no base, no record)

    uint64_t *poff = reinterpret_cast<uint64_t *>(w + F.poff);
    uint8_t *ms = w + F.ms;
    for (size_t q0 = 0; q0 < qrefs.size(); q0 += F.refs) {
        const uint32_t refs = (uint32_t)std::min<size_t>(F.refs, qrefs.size() - q0);
        const uint32_t np = refs * (uint32_t)c.n_seqs * F.g.n_strands;
        const uint64_t bytes = kbo::refplan::slab_bytes(F.g, refs);
        uint32_t lds_units = 0; // the kinds of reference the slab holds: only their kernels are launched
        bool has_lds = false, has_wide = false;
        for (uint32_t j = 0; j < refs; j++) {
            const kbo::RefsetDesc &d = set->descs[qrefs[q0 + j]];
            if (d.route == kbo::kRefsetRouteWide) has_wide = true;
            else {
                has_lds = true;
                lds_units = std::max(lds_units, kbo::refset_units(d.n_sets));
            }
        }
        HIP_OK(kbo::launch_refset_plan_slab(P, (uint32_t)q0, refs, poff, at(F.pthr), find ? w + F.chars : nullptr,
                                            reinterpret_cast<uint4 *>(w + F.items), reinterpret_cast<uint4 *>(w + F.tasks), st));
        kbo::RefsetWalkArgs a;
        a.descs = ds->descs.as<kbo::RefsetDesc>();
        a.arena = ds->arena.as<uint4>();
        a.tasks = reinterpret_cast<const uint4 *>(w + F.tasks);
        a.items = reinterpret_cast<const uint4 *>(w + F.items);
        a.n_tasks = refs * F.g.tasks_per_ref;
        a.k = set->k;
        a.q = q;
        a.ms = ms;
        if (has_lds) HIP_OK(kbo::launch_refset_walk(a, lds_units, st));
        if (has_wide) HIP_OK(kbo::launch_refset_wide_walk(a, st));
        if (find) {
            HIP_OK(kbo::launch_derand_translate_seq(ms, poff, np, bytes, set->k, at(F.pthr), min_thr, nullptr, w + F.chars, w + F.derand, st));
            HIP_OK(kbo::launch_rle_seg_count(w + F.chars, poff, np, bytes, c.gap, 0u, w + F.stage, at(F.first), st));
            if (F.local_cap)
                HIP_OK(kbo::launch_rle_seg_emit(w + F.chars, np, bytes, c.gap, w + F.stage, at(F.local), (uint32_t)F.local_cap, st));
            HIP_OK(kbo::launch_refset_tag_runs(P, (uint32_t)q0, np, at(F.first), at(F.local), (uint32_t)F.local_cap, c.d_n, c.capacity,
                                               static_cast<uint32_t *>(c.d_out), st));
        } else if (best) {
            HIP_OK(kbo::launch_derand_summary_seq(ms, poff, np, bytes, set->k, at(F.pthr), min_thr, at(F.chars), w + F.derand, st));
            kbo::RefsetBestArgs b;
            b.ext = at(F.chars);
            b.refs = at(F.qref) + q0;
            b.table = static_cast<uint32_t *>(c.d_out);
            b.n_pairs = np;
            b.lead = 0;
            b.slab_refs = refs;
            b.n_seqs = (uint32_t)c.n_seqs;
            b.n_strands = F.g.n_strands;
            b.strands = (uint32_t)c.strands;
            HIP_OK(kbo::launch_refset_best(b, st));
            t_best[kbo::refset_best_splits(b.n_seqs) ? 1 : 0]++;
        } else {
            HIP_OK(kbo::launch_derand_summary_seq(ms, poff, np, bytes, set->k, at(F.pthr), min_thr, at(F.chars), w + F.derand, st));
            HIP_OK(kbo::launch_refset_keep(at(F.chars), np, at(F.stage), at(F.local), at(F.total), st));
            HIP_OK(kbo::launch_refset_tag_summaries(P, (uint32_t)q0, np, at(F.local), at(F.total), c.d_n, c.capacity,
                                                    static_cast<uint32_t *>(c.d_out), st));
        }
    }
}

// ---- the screened device-resident form (kbo_refset_candidates_dev, kbo_*_refset_screened_dev): the screen kernel over the batch
// where it is, the bitmap to the list of its set bits, and ONE slab of the list's longest prefix within the caller's caps planned
// from it (refset_cand_kernels.hip).  The stages behind the walk see the slab as max_pairs sequences over max_pair_bases bytes, of
// which those behind the walked pairs are empty: their total_bases only bounds their chunk lists (derand_seq_kernels.hip seq_layout,
// rle_seg_kernels.hip seg_layout), and walked_bases / 128 + n_walked chunks are within max_pair_bases / 128 + max_pairs.
enum CandKind { kCandSummary, kCandFind, kCandBest, kCandOnly };
constexpr uint64_t kCandMaxPairs = (1ull << 28) - 1, kCandMaxBases = (1ull << 32) - 17; // what ONE slab may hold
struct CandForm {
    uint32_t n_refs = 0, n_q = 0, words = 0, chunk = 0;
    uint64_t n_bits = 0, item_slots = 0, task_slots = 0, local_cap = 0;
    size_t rev = 0; // bytes of one strand of the batch in the query buffer
    size_t q = 0, thr = 0, pc = 0, hdr = 0, bits = 0, list = 0, poff = 0, bsum = 0, pthr = 0, nch = 0, rfirst = 0, ntask = 0, items = 0, tasks = 0, ms = 0,
           derand = 0, chars = 0, stage = 0, first = 0, local = 0, total = 0, end = 0;
    bool ok = false;
};

// why a call with these arguments is refused, in the order the calls report it; KBO_OK: it is not
int cand_refusal(const kbo_refset *set, size_t n_seqs, uint64_t total, int strands, size_t max_pairs, uint64_t max_bases, CandKind kind)
{
    if (!set || strands < 1 || strands > 3) return KBO_E_BAD_ARG;
    if (n_seqs == 0) return KBO_E_EMPTY_QUERY;
    if (!set->prefilter) return KBO_E_BAD_ARG;
    if (kind != kCandOnly && max_pairs == 0) return KBO_E_BAD_ARG;
    for (const kbo::RefsetDesc &d : set->descs)
        if (!d.status && d.route == kbo::kRefsetRouteIndex) return KBO_E_UNSUPPORTED;
    if (screen_bits(set, n_seqs) > kPrefilterMaxBits) return KBO_E_UNSUPPORTED;
    const uint64_t ns = strands == 3 ? 2 : 1;
    if (n_seqs * ns >= (1ull << 28) || total >= (1ull << 31) || ns * total >= (1ull << 32) - 16) return KBO_E_UNSUPPORTED;
    if (kind != kCandOnly && (max_pairs > kCandMaxPairs || max_bases > kCandMaxBases)) return KBO_E_UNSUPPORTED;
    return KBO_OK;
}

CandForm cand_form(const kbo_refset *set, size_t n_seqs, uint64_t total, int strands, size_t capacity, size_t max_pairs, uint64_t max_bases,
                   CandKind kind)
{
    CandForm F;
    if (cand_refusal(set, n_seqs, total, strands, max_pairs, max_bases, kind) != KBO_OK) return F;
    const uint64_t MP = max_pairs, MB = max_bases;
    F.n_refs = (uint32_t)set->descs.size();
    for (const kbo::RefsetDesc &d : set->descs) F.n_q += !d.status;
    F.n_bits = screen_bits(set, n_seqs);
    F.words = (uint32_t)((F.n_bits + 31) / 32);
    F.chunk = kbo::refplan::chunk_of(set->k);
    F.rev = (size_t)(total + 15) / 16 * 16;
    size_t w = 0;
    if (strands == 3) { // '+' copied to q, '-' made at q + rev: one buffer for the screen and the walk
        F.q = w;
        w += 2 * F.rev + 64;
    }
    F.thr = w;    w += up16((size_t)F.n_refs * 5);                                                 // the thresholds, then the m bytes
    F.pc = w;     w += up16(kbo::chunk_items_scratch_words(F.words) * sizeof(uint32_t));
    F.hdr = w;    w += 32;
    if (kind != kCandOnly) {
        F.item_slots = kbo::refcand::item_slots(MP, MB, F.chunk);
        F.task_slots = kbo::refcand::task_slots(F.item_slots, F.n_q, MP);
        F.bits = w;   w += up16((size_t)F.words * sizeof(uint32_t));
        F.list = w;   w += up16((size_t)MP * sizeof(uint32_t));
        F.poff = w;   w += up16((size_t)(MP + 1) * sizeof(uint64_t));
        F.bsum = w;   w += up16((size_t)((MP + 1) / kbo::refcand::kScan64Block + 2) * sizeof(uint64_t));
        F.pthr = w;   w += up16((size_t)MP * sizeof(uint32_t));
        F.nch = w;    w += up16(kbo::chunk_items_scratch_words((uint32_t)MP) * sizeof(uint32_t));
        F.rfirst = w; w += up16((size_t)(F.n_refs + 1) * sizeof(uint32_t));
        F.ntask = w;  w += up16(kbo::chunk_items_scratch_words(F.n_refs) * sizeof(uint32_t));
        F.items = w;  w += (size_t)F.item_slots * sizeof(uint4);
        F.tasks = w;  w += (size_t)F.task_slots * sizeof(uint4);
        F.ms = w;     w += up16((size_t)MB) + 64;
        F.derand = w; w += up16(kbo::derand_seq_work_bytes((uint32_t)MP, MB, set->k, 2));
        if (kind == kCandFind) {
            F.local_cap = std::min<uint64_t>(capacity, MB / 2 + MP); // (a run holds a character other than '-' and ends at one)
            F.chars = w; w += up16((size_t)MB) + 64;
            F.stage = w; w += up16(kbo::rle_seg_work_bytes((uint32_t)MP, MB));
            F.first = w; w += up16((size_t)(MP + 1) * sizeof(uint32_t));
            F.local = w; w += up16((size_t)F.local_cap * kRleWords * sizeof(uint32_t));
        } else {
            F.chars = w; w += up16((size_t)MP * sizeof(kbo_aln_extent)); // the extents
            if (kind == kCandSummary) {
                F.stage = w; w += up16(kbo::chunk_items_scratch_words((uint32_t)MP) * sizeof(uint32_t));
                F.local = w; w += up16((size_t)MP * 7 * sizeof(uint32_t));
                F.total = w; w += 16;
            }
        }
    }
    if (strands == 2) { // '-' alone: the screen kernel reads it at q + rev, so it lies at least rev bytes into d_work and q inside it
        F.q = std::max(w, F.rev);
        w = F.q + F.rev + 64;
    }
    F.end = w;
    F.ok = true;
    return F;
}

struct CandCall {
    DevCall c;
    size_t max_pairs;
    uint64_t max_bases;
    uint32_t *d_bits; // kCandOnly: the caller's bitmap
    kbo_refset_screen_stats *d_stats;
};

void run_cand_form(const CandCall &cc, CandKind kind)
{
    namespace sc = kbo::refscreen;
    const DevCall &c = cc.c;
    const bool find = kind == kCandFind, best = kind == kCandBest, only = kind == kCandOnly;
    KBO_REQUIRE(c.strands >= 1 && c.strands <= 3, KBO_E_BAD_ARG, "strands: KBO_STRAND_FWD, KBO_STRAND_REV or both");
    KBO_REQUIRE(c.set && c.d_concat && c.d_offsets && c.d_work && cc.d_stats && (only ? cc.d_bits != nullptr : (c.d_n || best)) &&
                    (only || c.d_out || (c.capacity == 0 && !best)),
                KBO_E_BAD_ARG, "null argument");
    KBO_REQUIRE(((uintptr_t)c.d_concat & 15) == 0 && ((uintptr_t)c.d_work & 15) == 0 && ((uintptr_t)c.d_offsets & 7) == 0 &&
                    ((uintptr_t)c.d_n & 7) == 0 && ((uintptr_t)c.d_out & 3) == 0 && ((uintptr_t)cc.d_stats & 7) == 0 && ((uintptr_t)cc.d_bits & 3) == 0,
                KBO_E_BAD_ARG, "d_concat and d_work 16-byte, d_offsets, the count and d_stats 8-byte, the records and d_bits 4-byte aligned");
    KBO_REQUIRE(c.n_seqs > 0, KBO_E_EMPTY_QUERY, "empty batch");
    kbo_refset *set = c.set;
    KBO_REQUIRE(set->prefilter, KBO_E_BAD_ARG, "the set has no prefilter (kbo_refset_build_opts)");
    KBO_REQUIRE(only || cc.max_pairs > 0, KBO_E_BAD_ARG, "max_pairs == 0");
    const std::vector<uint32_t> thr = refset_thresholds(set, c.max_error_prob);
    for (const kbo::RefsetDesc &d : set->descs)
        KBO_REQUIRE(d.status || d.route != kbo::kRefsetRouteIndex, KBO_E_UNSUPPORTED,
                    "a reference of the single-index route: the host calls take it (kbo_refset_packed_only)");
    KBO_REQUIRE(screen_bits(set, c.n_seqs) <= kPrefilterMaxBits, KBO_E_UNSUPPORTED, "a bitmap of more than 2^31 bits");
    KBO_REQUIRE(only || (cc.max_pairs <= kCandMaxPairs && cc.max_bases <= kCandMaxBases), KBO_E_UNSUPPORTED,
                "caps beyond one slab: 2^28 pairs or more, or more than 2^32 - 17 bases (the unscreened form cuts several slabs)");
    const CandForm F = cand_form(set, c.n_seqs, c.total_bases, c.strands, c.capacity, cc.max_pairs, cc.max_bases, kind);
    KBO_REQUIRE(F.ok, KBO_E_UNSUPPORTED, "a batch of 2^31 bases or more, or 2^28 (sequence, strand) pairs or more");
    KBO_REQUIRE(c.work_bytes >= F.end, KBO_E_BAD_ARG, "work_bytes below the figure of *_work_bytes");
    DevSet *ds = device_set_if_any(set, current_device());
    KBO_REQUIRE(ds, KBO_E_BAD_ARG, "the set has no copy on the current device (kbo_refset_to_device)");

    // the call's one upload: the thresholds and, behind them, the seed lengths as the kernels take them
    const std::vector<uint8_t> m = seed_lens(set, thr);
    std::vector<uint32_t> up(((size_t)F.n_refs * 5 + 3) / 4, 0u);
    std::copy(thr.begin(), thr.end(), up.begin());
    uint8_t *up_m = reinterpret_cast<uint8_t *>(up.data() + F.n_refs);
    uint32_t min_thr = set->k, safe_ref = 0, lds_units = 0;
    bool has_lds = false, has_wide = false, any = false;
    for (size_t r = 0; r < F.n_refs; r++) {
        up_m[r] = m[r] >= sc::kSeedMin ? m[r] : (uint8_t)(m[r] ? kbo::refcand::kMarkAll : sc::kUnfilterable);
        const kbo::RefsetDesc &d = set->descs[r];
        if (d.status) continue;
        if (!any) safe_ref = (uint32_t)r;
        any = true;
        min_thr = std::min(min_thr, thr[r]);
        if (d.route == kbo::kRefsetRouteWide) has_wide = true;
        else {
            has_lds = true;
            lds_units = std::max(lds_units, kbo::refset_units(d.n_sets));
        }
    }
    hipStream_t st = c.stream;
    uint8_t *w = static_cast<uint8_t *>(c.d_work);
    auto at = [&](size_t o) { return reinterpret_cast<uint32_t *>(w + o); };
    HIP_OK(hipMemcpyAsync(w + F.thr, up.data(), (size_t)F.n_refs * 5, hipMemcpyHostToDevice, st));
    // ONE query buffer for the screen and the walk: the caller's for '+' alone; '+' copied and '-' behind it; or '-' alone, which the
    // walk reads at its first byte and the screen at q + rev
    const uint8_t *walk_q = c.strands == 1 ? c.d_concat : w + F.q;
    if (c.strands == 3 && c.total_bases) HIP_OK(hipMemcpyAsync(w + F.q, c.d_concat, c.total_bases, hipMemcpyDeviceToDevice, st));
    if (c.strands & KBO_STRAND_REV)
        HIP_OK(kbo::launch_revcomp_bytes(c.d_concat, c.d_offsets, (uint32_t)c.n_seqs, c.total_bases, w + F.q + (c.strands == 3 ? F.rev : 0), st));
    uint32_t *bits = only ? cc.d_bits : at(F.bits);
    HIP_OK(hipMemsetAsync(bits, 0, (size_t)F.words * sizeof(uint32_t), st));
    HIP_OK(hipMemsetAsync(cc.d_stats, 0, sizeof(kbo_refset_screen_stats), st));
    kbo::RefsetScreenArgs s;
    s.bucket = ds->pre_bucket.as<uint32_t>();
    s.keys = ds->pre_keys.as<uint64_t>();
    s.refs = ds->pre_refs.as<uint32_t>();
    s.m = w + F.thr + (size_t)F.n_refs * 4;
    s.q = c.strands == 2 ? w + F.q - F.rev : walk_q;
    s.off = c.d_offsets;
    s.bits = bits;
    s.total = c.total_bases;
    s.rev_base = F.rev;
    s.n_seqs = (uint32_t)c.n_seqs;
    s.strands = (uint32_t)c.strands;
    s.first_strand = c.strands == 2 ? 2u : 1u;
    HIP_OK(kbo::launch_refset_screen(s, st));
    kbo::RefsetCandArgs a{};
    a.off = c.d_offsets;
    a.thr = at(F.thr);
    a.m = s.m;
    a.bits = bits;
    a.pc = at(F.pc);
    a.hdr = reinterpret_cast<uint64_t *>(w + F.hdr);
    a.stats = reinterpret_cast<uint64_t *>(cc.d_stats);
    a.n_bits = F.n_bits;
    a.words = F.words;
    a.n_refs = F.n_refs;
    a.n_seqs = (uint32_t)c.n_seqs;
    a.strands = (uint32_t)c.strands;
    a.k = set->k;
    a.chunk = F.chunk;
    HIP_OK(kbo::launch_refset_cand_count(a, st));
    if (only) {
        HIP_OK(kbo::launch_refset_cand_stats(a, st));
        return;
    }
    a.list = at(F.list);
    a.poff = reinterpret_cast<uint64_t *>(w + F.poff);
    a.bsum = reinterpret_cast<uint64_t *>(w + F.bsum);
    a.pthr = at(F.pthr);
    a.nch = at(F.nch);
    a.rfirst = at(F.rfirst);
    a.ntask = at(F.ntask);
    a.max_bases = cc.max_bases;
    a.rev_off = c.strands == 3 ? F.rev : 0;
    a.max_pairs = (uint32_t)cc.max_pairs;
    a.item_slots = (uint32_t)F.item_slots;
    a.task_slots = (uint32_t)F.task_slots;
    a.safe_ref = safe_ref;
    const uint32_t np = a.max_pairs;
    const uint64_t bytes = cc.max_bases;
    HIP_OK(kbo::launch_refset_cand_list(a, st));
    HIP_OK(kbo::launch_refset_cand_plan(a, find ? w + F.chars : nullptr, reinterpret_cast<uint4 *>(w + F.items), reinterpret_cast<uint4 *>(w + F.tasks), st));
    kbo::RefsetWalkArgs wa;
    wa.descs = ds->descs.as<kbo::RefsetDesc>();
    wa.arena = ds->arena.as<uint4>();
    wa.tasks = reinterpret_cast<const uint4 *>(w + F.tasks);
    wa.items = reinterpret_cast<const uint4 *>(w + F.items);
    wa.n_tasks = a.task_slots;
    wa.k = set->k;
    wa.q = walk_q;
    wa.ms = w + F.ms;
    if (has_lds) HIP_OK(kbo::launch_refset_walk(wa, lds_units, st));
    if (has_wide) HIP_OK(kbo::launch_refset_wide_walk(wa, st));
    uint8_t *ms = w + F.ms;
    if (find) {
        HIP_OK(kbo::launch_derand_translate_seq(ms, a.poff, np, bytes, set->k, a.pthr, min_thr, nullptr, w + F.chars, w + F.derand, st));
        HIP_OK(kbo::launch_rle_seg_count(w + F.chars, a.poff, np, bytes, c.gap, 0u, w + F.stage, at(F.first), st));
        if (F.local_cap) HIP_OK(kbo::launch_rle_seg_emit(w + F.chars, np, bytes, c.gap, w + F.stage, at(F.local), (uint32_t)F.local_cap, st));
        HIP_OK(kbo::launch_refset_cand_tag_runs(a, at(F.first), at(F.local), (uint32_t)F.local_cap, c.d_n, c.capacity, static_cast<uint32_t *>(c.d_out), st));
    } else if (best) {
        HIP_OK(kbo::launch_derand_summary_seq(ms, a.poff, np, bytes, set->k, a.pthr, min_thr, at(F.chars), w + F.derand, st));
        HIP_OK(kbo::launch_refset_best_init(static_cast<uint32_t *>(c.d_out), (uint32_t)c.n_seqs, st));
        HIP_OK(kbo::launch_refset_cand_best(a, at(F.chars), static_cast<uint32_t *>(c.d_out), st));
    } else {
        HIP_OK(kbo::launch_derand_summary_seq(ms, a.poff, np, bytes, set->k, a.pthr, min_thr, at(F.chars), w + F.derand, st));
        HIP_OK(kbo::launch_refset_keep(at(F.chars), np, at(F.stage), at(F.local), at(F.total), st));
        HIP_OK(kbo::launch_refset_cand_tag_summaries(a, at(F.local), at(F.total), c.d_n, c.capacity, static_cast<uint32_t *>(c.d_out), st));
    }
}

} // namespace

extern "C" {

int kbo_refset_build(const uint8_t *const *seqs, const size_t *lens, size_t n_refs, const kbo_build_opts *opts, kbo_refset_t **out)
{
    return kbo_refset_build_wide(seqs, lens, n_refs, opts, KBO_REFSET_MAX_ROWS, out);
}

int kbo_refset_build_wide(const uint8_t *const *seqs, const size_t *lens, size_t n_refs, const kbo_build_opts *opts, size_t max_wide_rows,
                          kbo_refset_t **out)
{
    kbo_refset_opts ro;
    kbo_refset_opts_default(&ro);
    ro.max_wide_rows = max_wide_rows;
    return kbo_refset_build_opts(seqs, lens, n_refs, opts, &ro, out);
}

void kbo_refset_opts_default(kbo_refset_opts *o)
{
    if (!o) return;
    o->max_wide_rows = KBO_REFSET_MAX_ROWS;
    o->prefilter = 0;
    o->positions = 0;
}

int kbo_refset_build_opts(const uint8_t *const *seqs, const size_t *lens, size_t n_refs, const kbo_build_opts *opts,
                          const kbo_refset_opts *refset_opts, kbo_refset_t **out)
{
    return guarded([&] {
        KBO_REQUIRE(out, KBO_E_BAD_ARG, "null out");
        *out = nullptr;
        kbo_refset_opts ro;
        if (refset_opts) ro = *refset_opts; else kbo_refset_opts_default(&ro);
        const size_t max_wide_rows = ro.max_wide_rows;
        KBO_REQUIRE(ro.prefilter == 0 || ro.prefilter == 1, KBO_E_BAD_ARG, "prefilter: 0 or 1");
        KBO_REQUIRE(ro.positions == 0 || ro.positions == 1, KBO_E_BAD_ARG, "positions: 0 or 1");
        KBO_REQUIRE(max_wide_rows >= KBO_REFSET_MAX_ROWS && max_wide_rows <= KBO_REFSET_WIDE_MAX_ROWS, KBO_E_BAD_ARG,
                    "max_wide_rows in KBO_REFSET_MAX_ROWS .. KBO_REFSET_WIDE_MAX_ROWS");
        KBO_REQUIRE(seqs && lens && n_refs > 0, KBO_E_BAD_ARG, "assert!(!slices.is_empty()) (index.rs:60)");
        KBO_REQUIRE(n_refs < 0xFFFFFFFFull, KBO_E_UNSUPPORTED, "more than 2^32-1 references");
        for (size_t r = 0; r < n_refs; r++) KBO_REQUIRE(seqs[r] || lens[r] == 0, KBO_E_BAD_ARG, "null reference sequence");
        if (ro.positions)
            for (size_t r = 0; r < n_refs; r++)
                KBO_REQUIRE(lens[r] < kbo::reflocate::kMaxRefLen, KBO_E_UNSUPPORTED, "positions: a reference of 2^30 bases or more");
        kbo_build_opts o;
        if (opts) o = *opts; else kbo_build_opts_default(&o);
        KBO_REQUIRE(o.k > 0 && o.k <= 255, KBO_E_BAD_ARG, "k must be in 1..255");
        std::unique_ptr<kbo_refset> set(new kbo_refset());
        set->k = o.k;
        set->descs.assign(n_refs, kbo::RefsetDesc{});
        set->own.resize(n_refs);
        set->ref_len.assign(lens, lens + n_refs);
        std::vector<std::vector<uint32_t>> forms(n_refs);
        std::atomic<size_t> next{0};
        auto work = [&] {
            for (size_t r; (r = next.fetch_add(1)) < n_refs;) {
                kbo::RefsetDesc &d = set->descs[r];
                std::unique_ptr<kbo_index> idx(new kbo_index());
                try {
                    kbo::BuildParams p;
                    p.k = o.k;
                    p.add_revcomp = o.add_revcomp != 0;
                    p.num_threads = 1;
                    kbo::build_host_index(&seqs[r], &lens[r], 1, p, idx->host);
                } catch (const std::exception &) {
                    d.status = KBO_E_UNSUPPORTED; // (what kbo_index_build of it alone cannot build either)
                    continue;
                }
                const kbo::HostIndex &h = idx->host;
                d.n_sets = (uint32_t)h.n_sets;
                d.n_kmers = h.n_kmers;
                for (int c = 0; c < 4; c++) d.C[c] = (uint32_t)h.C[c];
                if (h.n_kmers == 0) d.status = KBO_E_BAD_ARG; // n_kmers > 0 (derandomize.rs:134)
                else if (h.n_sets > max_wide_rows) {
                    d.route = kbo::kRefsetRouteIndex;
                    set->own[r] = std::move(idx);
                } else { // its packed form in the arena, and no index of its own: no plan structures
                    d.route = h.n_sets > kbo::kRefsetMaxRows ? kbo::kRefsetRouteWide : kbo::kRefsetRouteLds;
                    append_lds_form(h, forms[r]);
                }
            }
        };
        std::vector<std::thread> team;
        for (uint32_t t = 1; t < std::min<size_t>(std::max(1u, o.num_threads), n_refs); t++) team.emplace_back(work);
        work();
        for (auto &t : team) t.join();
        size_t words = 0;
        for (auto &f : forms) words += f.size();
        KBO_REQUIRE(words / 4 < 0xFFFFFFFFull, KBO_E_UNSUPPORTED, "the set's packed layout exceeds 2^32 units");
        set->arena.reserve(words);
        for (size_t r = 0; r < n_refs; r++) {
            set->descs[r].off = (uint32_t)(set->arena.size() / 4);
            set->arena.insert(set->arena.end(), forms[r].begin(), forms[r].end());
            std::vector<uint32_t>().swap(forms[r]);
        }
        if (ro.prefilter) build_prefilter(set.get(), seqs, lens, o.add_revcomp != 0); // (the sequences are at hand here only)
        if (ro.positions) build_positions(set.get(), seqs, lens, o.add_revcomp != 0, std::max(1u, o.num_threads));
        *out = set.release();
    });
}

void kbo_refset_free(kbo_refset_t *set) { delete set; }
size_t kbo_refset_size(const kbo_refset_t *set) { return set ? set->descs.size() : 0; }
size_t kbo_refset_k(const kbo_refset_t *set) { return set ? set->k : 0; }
uint64_t kbo_refset_n_kmers(const kbo_refset_t *set, size_t r) { return set && r < set->descs.size() ? set->descs[r].n_kmers : 0; }
int kbo_refset_status(const kbo_refset_t *set, size_t r) { return set && r < set->descs.size() ? set->descs[r].status : KBO_E_BAD_ARG; }

int kbo_refset_to_device(kbo_refset_t *set, int device)
{
    return guarded([&] {
        KBO_REQUIRE(set, KBO_E_BAD_ARG, "null set");
        const int dev = device < 0 ? current_device() : device;
        (void)device_set(set, dev);
        for (auto &idx : set->own)
            if (idx) (void)device_view(idx.get(), dev, nullptr, 0, true);
    });
}

int kbo_set_refset_record_capacity(size_t records)
{
    g_record_capacity = std::max<size_t>(1, records);
    return KBO_OK;
}

int kbo_refset_last_wide(uint64_t out[2])
{
    if (!out) return KBO_E_BAD_ARG;
    std::copy(t_wide, t_wide + 2, out);
    return KBO_OK;
}

int kbo_refset_route(const kbo_refset_t *set, size_t r)
{
    if (!set || r >= set->descs.size()) return KBO_E_BAD_ARG;
    return set->descs[r].status ? KBO_REFSET_ROUTE_NONE : (int)set->descs[r].route;
}

int kbo_refset_packed_only(const kbo_refset_t *set)
{
    if (!set) return 0;
    for (const kbo::RefsetDesc &d : set->descs)
        if (!d.status && d.route == kbo::kRefsetRouteIndex) return 0;
    return 1;
}

namespace {
const kbo::RefsetDesc *packed_desc(const kbo_refset_t *set, size_t r)
{
    if (!set || r >= set->descs.size()) return nullptr;
    const kbo::RefsetDesc &d = set->descs[r];
    return d.status || d.route == kbo::kRefsetRouteIndex ? nullptr : &d;
}
} // namespace

int kbo_refset_form(const kbo_refset_t *set, size_t r, uint8_t *out, size_t *n_bytes)
{
    const kbo::RefsetDesc *d = packed_desc(set, r);
    if (!d || !n_bytes) return KBO_E_BAD_ARG;
    *n_bytes = (size_t)kbo::refset_units(d->n_sets) * 16u;
    if (out) std::memcpy(out, set->arena.data() + (size_t)d->off * 4u, *n_bytes);
    return KBO_OK;
}

int kbo_refset_ms_host(const kbo_refset_t *set, size_t r, const uint8_t *seq, size_t len, uint8_t *ms_out)
{
    const kbo::RefsetDesc *d = packed_desc(set, r);
    if (!d || ((!seq || !ms_out) && len)) return KBO_E_BAD_ARG;
    const uint32_t n = d->n_sets;
    const uint32_t *form = set->arena.data() + (size_t)d->off * 4u;
    const HostForm x{form, reinterpret_cast<const uint8_t *>(form + 4u * (size_t)kbo::refset_rank_units(n))};
    uint32_t lo = 0, hi = n, depth = 0;
    for (size_t i = 0; i < len; i++) {
        kbo::refstep::step(x, n, set->k, seq[i], lo, hi, depth);
        ms_out[i] = (uint8_t)depth;
    }
    return KBO_OK;
}

int kbo_refset_has_prefilter(const kbo_refset_t *set) { return set && set->prefilter ? 1 : 0; }

uint64_t kbo_refset_prefilter_bytes(const kbo_refset_t *set)
{
    if (!set || !set->prefilter) return 0;
    return (uint64_t)set->pre_bucket.size() * sizeof(uint32_t) + (uint64_t)set->pre_keys.size() * (sizeof(uint64_t) + sizeof(uint32_t));
}

int kbo_set_refset_prefilter_max_bits(uint64_t bits)
{
    g_prefilter_max_bits = bits == 0 || bits > kPrefilterMaxBits ? kPrefilterMaxBits : bits;
    return KBO_OK;
}

int kbo_refset_last_prefilter(uint64_t out[4])
{
    if (!out) return KBO_E_BAD_ARG;
    std::copy(t_pre, t_pre + 4, out);
    return KBO_OK;
}

int kbo_refset_candidates(kbo_refset_t *set, const uint8_t *concat, const uint64_t *offsets, size_t n_seqs, double max_error_prob,
                          int strands, uint32_t *bits_out, uint64_t *n_candidates)
{
    return guarded([&] {
        uint64_t total = 0;
        const std::vector<uint32_t> thr = check_candidates(set, concat, offsets, n_seqs, max_error_prob, strands, bits_out, &total);
        SlabWalker F;
        StreamScope stream;
        upload_batch(F, set, concat, offsets, n_seqs, total, strands, stream.s);
        Screen scr;
        run_screen(F, thr, n_seqs, total, strands, scr);
        std::copy(scr.bits.begin(), scr.bits.end(), bits_out);
        if (n_candidates) *n_candidates = scr.count();
    });
}

int kbo_refset_candidates_host(const kbo_refset_t *set, const uint8_t *concat, const uint64_t *offsets, size_t n_seqs,
                               double max_error_prob, int strands, uint32_t *bits_out, uint64_t *n_candidates)
{
    return guarded([&] {
        namespace sc = kbo::refscreen;
        uint64_t total = 0;
        const std::vector<uint32_t> thr = check_candidates(set, concat, offsets, n_seqs, max_error_prob, strands, bits_out, &total);
        const std::vector<uint8_t> m = seed_lens(set, thr);
        Screen scr;
        scr.n_seqs = n_seqs;
        scr.bits.assign((size_t)((screen_bits(set, n_seqs) + 31) / 32), 0u);
        const HostTable table{set};
        std::vector<uint8_t> rc;
        for (size_t s = 0; s < n_seqs; s++) {
            const uint8_t *fwd = concat + offsets[s];
            const size_t len = (size_t)(offsets[s + 1] - offsets[s]);
            for (uint32_t strand = 1; strand <= 2; strand++) {
                if (!(strands & strand)) continue;
                const uint8_t *q = fwd;
                if (strand == KBO_STRAND_REV) {
                    revcomp_host(fwd, len, rc);
                    q = rc.data();
                }
                sc::Seed seed{0u, 0u};
                for (size_t i = len; i-- > 0;) {
                    seed = sc::step_left(seed, q[i]);
                    sc::scan(table, seed, [&](uint32_t r, uint32_t shared) {
                        if (m[r] >= sc::kSeedMin && shared >= m[r]) scr.set_bit(r, s, strand);
                    });
                }
            }
        }
        mark_unfilterable(m, strands, scr);
        std::copy(scr.bits.begin(), scr.bits.end(), bits_out);
        if (n_candidates) *n_candidates = scr.count();
    });
}

int kbo_refset_last_routes(uint64_t out[4])
{
    if (!out) return KBO_E_BAD_ARG;
    std::copy(t_routes, t_routes + 4, out);
    return KBO_OK;
}

int kbo_find_refset(kbo_refset_t *set, const uint8_t *concat, const uint64_t *offsets, size_t n_seqs, const kbo_find_opts *opts,
                    int strands, kbo_ref_run **runs, uint64_t *n_runs)
{
    return guarded([&] {
        static_assert(sizeof(kbo_ref_run) == 40, "kbo_ref_run is 40 bytes");
        KBO_REQUIRE(strands >= 1 && strands <= 3, KBO_E_BAD_ARG, "strands: KBO_STRAND_FWD, KBO_STRAND_REV or both");
        KBO_REQUIRE(set && runs && n_runs, KBO_E_BAD_ARG, "null argument");
        *runs = nullptr;
        *n_runs = 0;
        kbo_find_opts o;
        if (opts) o = *opts; else kbo_find_opts_default(&o);
        const std::vector<uint32_t> thr = refset_thresholds(set, o.max_error_prob);
        const uint64_t total = check_refset_batch(set, concat, offsets, n_seqs);
        std::fill(t_routes, t_routes + 4, 0);
        std::fill(t_wide, t_wide + 2, 0);

        const size_t n_refs = set->descs.size();
        const uint32_t n_strands = strands == 3 ? 2 : 1;
        Finder F;
        F.gap = (uint32_t)std::min<size_t>(o.max_gap_len, 0xFFFFFFFFu);
        StreamScope stream;
        upload_batch(F, set, concat, offsets, n_seqs, total, strands, stream.s);
        Screen scr;
        run_slabs(F, thr, n_seqs, strands, screen_call(F, thr, n_seqs, total, strands, scr));

        // the references of the single-index route: their own index through that pipeline, one at a time
        std::vector<uint64_t> rle_off(2 * n_seqs + 1);
        for (size_t r = 0; r < n_refs; r++) {
            if (set->descs[r].status || set->descs[r].route != kbo::kRefsetRouteIndex) continue;
            RleSink<kbo_rle> sink;
            sink.max_gap_len = o.max_gap_len;
            sink.rle_offsets = rle_off.data();
            matches_batch_impl(set->own[r].get(), concat, offsets, n_seqs, o.max_error_prob, false, nullptr, &sink, strands);
            kbo_rle *got = nullptr;
            sink.take(&got);
            MallocPtr<kbo_rle> hold(got);
            F.ref_begin[r] = F.out.size();
            for (size_t s = 0; s < n_seqs; s++)
                for (uint32_t strand = 1; strand <= 2; strand++)
                    for (uint64_t x = rle_off[2 * s + strand - 1]; x < rle_off[2 * s + strand]; x++) {
                        const kbo_rle &w = got[x];
                        F.out.push_back(kbo_ref_run{(uint32_t)r, (uint32_t)s, strand,
                                                    kbo_rle32{(uint32_t)w.start, (uint32_t)w.end, (uint32_t)w.matches, (uint32_t)w.mismatches,
                                                              (uint32_t)w.jumps, (uint32_t)w.gap_bases, (uint32_t)w.gap_opens}});
                    }
            F.ref_end[r] = F.out.size();
            t_routes[1]++;
            t_routes[2] += n_seqs * n_strands;
        }
        *runs = gather_by_ref(F, F.out, n_runs);
    });
}

int kbo_summary_refset(kbo_refset_t *set, const uint8_t *concat, const uint64_t *offsets, size_t n_seqs, double max_error_prob, int strands,
                       kbo_ref_summary **records, uint64_t *n_records)
{
    return guarded([&] {
        static_assert(sizeof(kbo_ref_summary) == 36, "kbo_ref_summary is 36 bytes");
        KBO_REQUIRE(strands >= 1 && strands <= 3, KBO_E_BAD_ARG, "strands: KBO_STRAND_FWD, KBO_STRAND_REV or both");
        KBO_REQUIRE(set && records && n_records, KBO_E_BAD_ARG, "null argument");
        *records = nullptr;
        *n_records = 0;
        const std::vector<uint32_t> thr = refset_thresholds(set, max_error_prob);
        const uint64_t total = check_refset_batch(set, concat, offsets, n_seqs);
        std::fill(t_routes, t_routes + 4, 0);
        std::fill(t_wide, t_wide + 2, 0);

        const size_t n_refs = set->descs.size();
        const uint32_t n_strands = strands == 3 ? 2 : 1;
        Summarizer F;
        StreamScope stream;
        upload_batch(F, set, concat, offsets, n_seqs, total, strands, stream.s);
        Screen scr;
        run_slabs(F, thr, n_seqs, strands, screen_call(F, thr, n_seqs, total, strands, scr));

        // the references of the single-index route: the characters of that pipeline, counted here
        std::vector<uint8_t> fwd, rev;
        for (size_t r = 0; r < n_refs; r++) {
            if (set->descs[r].status || set->descs[r].route != kbo::kRefsetRouteIndex) continue;
            if (strands & KBO_STRAND_FWD) fwd.resize(total);
            if (strands & KBO_STRAND_REV) rev.resize(total);
            matches_batch_impl(set->own[r].get(), concat, offsets, n_seqs, max_error_prob, false, fwd.data(), nullptr, strands, rev.data());
            F.ref_begin[r] = F.out.size();
            for (size_t s = 0; s < n_seqs; s++)
                for (uint32_t strand = 1; strand <= 2; strand++) {
                    if (!(strands & strand)) continue;
                    const uint8_t *c = (strand == KBO_STRAND_FWD ? fwd.data() : rev.data()) + offsets[s];
                    const kbo_aln_extent e = extent_of_chars(c, offsets[s + 1] - offsets[s]);
                    if (e.n_runs) F.out.push_back(kbo_ref_summary{(uint32_t)r, (uint32_t)s, strand, e});
                }
            F.ref_end[r] = F.out.size();
            t_routes[1]++;
            t_routes[2] += n_seqs * n_strands;
        }
        uint64_t n = 0;
        MallocPtr<kbo_ref_summary> res(gather_by_ref(F, F.out, &n));
        *n_records = n;
        if (n) *records = res.release(); // (none: *records stays NULL)
    });
}

int kbo_refset_lds_only(const kbo_refset_t *set)
{
    if (!set) return 0;
    for (const kbo::RefsetDesc &d : set->descs)
        if (!d.status && d.route != kbo::kRefsetRouteLds) return 0;
    return 1;
}

size_t kbo_find_refset_dev_work_bytes(const kbo_refset_t *set, size_t n_seqs, uint64_t total_bases, int strands, size_t capacity,
                                      size_t refs_per_slab)
{
    return dev_form(set, n_seqs, total_bases, strands, capacity, refs_per_slab, kDevFind).end;
}

size_t kbo_summary_refset_dev_work_bytes(const kbo_refset_t *set, size_t n_seqs, uint64_t total_bases, int strands, size_t capacity,
                                         size_t refs_per_slab)
{
    return dev_form(set, n_seqs, total_bases, strands, capacity, refs_per_slab, kDevSummary).end;
}

int kbo_find_refset_dev(kbo_refset_t *set, const uint8_t *d_concat, const uint64_t *d_offsets, size_t n_seqs, uint64_t total_bases,
                        const kbo_find_opts *opts, int strands, void *d_work, size_t work_bytes, kbo_ref_run *d_runs, size_t capacity,
                        uint64_t *d_n_runs, void *stream)
{
    return guarded([&] {
        kbo_find_opts o;
        if (opts) o = *opts; else kbo_find_opts_default(&o);
        run_dev_form(DevCall{set, d_concat, d_offsets, n_seqs, total_bases, o.max_error_prob, (uint32_t)std::min<size_t>(o.max_gap_len, 0xFFFFFFFFu),
                             strands, d_work, work_bytes, d_runs, capacity, d_n_runs, static_cast<hipStream_t>(stream)},
                     kDevFind);
    });
}

int kbo_summary_refset_dev(kbo_refset_t *set, const uint8_t *d_concat, const uint64_t *d_offsets, size_t n_seqs, uint64_t total_bases,
                           double max_error_prob, int strands, void *d_work, size_t work_bytes, kbo_ref_summary *d_records, size_t capacity,
                           uint64_t *d_n_records, void *stream)
{
    return guarded([&] {
        run_dev_form(DevCall{set, d_concat, d_offsets, n_seqs, total_bases, max_error_prob, 0u, strands, d_work, work_bytes, d_records, capacity,
                             d_n_records, static_cast<hipStream_t>(stream)},
                     kDevSummary);
    });
}

int kbo_refset_last_best(uint64_t out[2])
{
    if (!out) return KBO_E_BAD_ARG;
    std::copy(t_best, t_best + 2, out);
    return KBO_OK;
}

int kbo_best_refset(kbo_refset_t *set, const uint8_t *concat, const uint64_t *offsets, size_t n_seqs, double max_error_prob, int strands,
                    kbo_ref_best **out)
{
    return guarded([&] {
        namespace rb = kbo::refbest;
        static_assert(sizeof(kbo_ref_best) == 48 && sizeof(kbo_ref_best) == sizeof(rb::Best) && rb::kWords * 4 == sizeof(kbo_ref_best),
                      "kbo_ref_best is the twelve words of refset_best.hpp");
        KBO_REQUIRE(strands >= 1 && strands <= 3, KBO_E_BAD_ARG, "strands: KBO_STRAND_FWD, KBO_STRAND_REV or both");
        KBO_REQUIRE(set && out, KBO_E_BAD_ARG, "null argument");
        *out = nullptr;
        const std::vector<uint32_t> thr = refset_thresholds(set, max_error_prob);
        const uint64_t total = check_refset_batch(set, concat, offsets, n_seqs);
        KBO_REQUIRE(n_seqs < (1ull << 28), KBO_E_UNSUPPORTED, "2^28 sequences or more");
        std::fill(t_routes, t_routes + 4, 0);
        std::fill(t_wide, t_wide + 2, 0);
        std::fill(t_best, t_best + 2, 0);

        const size_t n_refs = set->descs.size();
        const uint32_t n_strands = strands == 3 ? 2 : 1;
        MallocPtr<kbo_ref_best> res = malloc_array<kbo_ref_best>(n_seqs);
        StreamScope stream;
        if (set->prefilter) {
            // refset_best_kernel finds a slab's pairs by arithmetic and cannot skip any: the summary's slabs over the candidate pairs,
            // and the kept records folded into the table here, by the merge the single-index references go through below
            Summarizer F;
            upload_batch(F, set, concat, offsets, n_seqs, total, strands, stream.s);
            Screen scr;
            run_slabs(F, thr, n_seqs, strands, screen_call(F, thr, n_seqs, total, strands, scr));
            std::vector<rb::Best> table(n_seqs);
            for (size_t s = 0; s < n_seqs; s++) table[s] = rb::empty((uint32_t)s);
            for (const kbo_ref_summary &w : F.out) {
                const uint32_t ext[6] = {w.aln.n_match, w.aln.n_mismatch, w.aln.n_jump, w.aln.n_runs, w.aln.start, w.aln.end};
                table[w.seq] = rb::merge(table[w.seq], rb::from_pair(w.seq, w.ref, w.strand, ext));
            }
            std::memcpy(res.get(), table.data(), n_seqs * sizeof(kbo_ref_best));
        } else {
            Bester F;
            F.n_seqs = (uint32_t)n_seqs;
            F.n_strands = n_strands;
            F.strands = (uint32_t)strands;
            upload_batch(F, set, concat, offsets, n_seqs, total, strands, stream.s);
            F.d_table.alloc(n_seqs * sizeof(kbo_ref_best));
            HIP_OK(kbo::launch_refset_best_init(F.d_table.as<uint32_t>(), (uint32_t)n_seqs, stream.s));
            Screen scr;
            run_slabs(F, thr, n_seqs, strands, screen_call(F, thr, n_seqs, total, strands, scr));
            HIP_OK(hipMemcpyAsync(res.get(), F.d_table.p, n_seqs * sizeof(kbo_ref_best), hipMemcpyDeviceToHost, stream.s));
            HIP_OK(hipStreamSynchronize(stream.s)); // the call's one wait
        }

        // the references of the single-index route: the characters of that pipeline, counted and merged here
        std::vector<uint8_t> fwd, rev;
        for (size_t r = 0; r < n_refs; r++) {
            if (set->descs[r].status || set->descs[r].route != kbo::kRefsetRouteIndex) continue;
            if (strands & KBO_STRAND_FWD) fwd.resize(total);
            if (strands & KBO_STRAND_REV) rev.resize(total);
            matches_batch_impl(set->own[r].get(), concat, offsets, n_seqs, max_error_prob, false, fwd.data(), nullptr, strands, rev.data());
            for (size_t s = 0; s < n_seqs; s++)
                for (uint32_t strand = 1; strand <= 2; strand++) {
                    if (!(strands & strand)) continue;
                    const uint8_t *c = (strand == KBO_STRAND_FWD ? fwd.data() : rev.data()) + offsets[s];
                    const kbo_aln_extent e = extent_of_chars(c, offsets[s + 1] - offsets[s]);
                    const uint32_t ext[6] = {e.n_match, e.n_mismatch, e.n_jump, e.n_runs, e.start, e.end};
                    rb::Best b;
                    std::memcpy(&b, &res[s], sizeof b);
                    b = rb::merge(b, rb::from_pair((uint32_t)s, (uint32_t)r, strand, ext));
                    std::memcpy(&res[s], &b, sizeof b);
                }
            t_routes[1]++;
            t_routes[2] += n_seqs * n_strands;
        }
        *out = res.release();
    });
}

size_t kbo_best_refset_dev_work_bytes(const kbo_refset_t *set, size_t n_seqs, uint64_t total_bases, int strands, size_t refs_per_slab)
{
    return dev_form(set, n_seqs, total_bases, strands, 0, refs_per_slab, kDevBest).end;
}

int kbo_best_refset_dev(kbo_refset_t *set, const uint8_t *d_concat, const uint64_t *d_offsets, size_t n_seqs, uint64_t total_bases,
                        double max_error_prob, int strands, void *d_work, size_t work_bytes, kbo_ref_best *d_out, void *stream)
{
    return guarded([&] {
        run_dev_form(DevCall{set, d_concat, d_offsets, n_seqs, total_bases, max_error_prob, 0u, strands, d_work, work_bytes, d_out, 0, nullptr,
                             static_cast<hipStream_t>(stream)},
                     kDevBest);
    });
}

size_t kbo_refset_candidates_dev_work_bytes(const kbo_refset_t *set, size_t n_seqs, uint64_t total_bases, int strands)
{
    return cand_form(set, n_seqs, total_bases, strands, 0, 0, 0, kCandOnly).end;
}

int kbo_refset_candidates_dev(kbo_refset_t *set, const uint8_t *d_concat, const uint64_t *d_offsets, size_t n_seqs, uint64_t total_bases,
                              double max_error_prob, int strands, void *d_work, size_t work_bytes, uint32_t *d_bits,
                              kbo_refset_screen_stats *d_stats, void *stream)
{
    return guarded([&] {
        static_assert(sizeof(kbo_refset_screen_stats) == 32, "kbo_refset_screen_stats is 32 bytes");
        run_cand_form(CandCall{DevCall{set, d_concat, d_offsets, n_seqs, total_bases, max_error_prob, 0u, strands, d_work, work_bytes, nullptr, 0, nullptr,
                                       static_cast<hipStream_t>(stream)},
                               0, 0, d_bits, d_stats},
                      kCandOnly);
    });
}

size_t kbo_find_refset_screened_dev_work_bytes(const kbo_refset_t *set, size_t n_seqs, uint64_t total_bases, int strands, size_t capacity,
                                               size_t max_pairs, uint64_t max_pair_bases)
{
    return cand_form(set, n_seqs, total_bases, strands, capacity, max_pairs, max_pair_bases, kCandFind).end;
}

int kbo_find_refset_screened_dev(kbo_refset_t *set, const uint8_t *d_concat, const uint64_t *d_offsets, size_t n_seqs, uint64_t total_bases,
                                 const kbo_find_opts *opts, int strands, void *d_work, size_t work_bytes, kbo_ref_run *d_runs, size_t capacity,
                                 uint64_t *d_n_runs, size_t max_pairs, uint64_t max_pair_bases, kbo_refset_screen_stats *d_stats, void *stream)
{
    return guarded([&] {
        kbo_find_opts o;
        if (opts) o = *opts; else kbo_find_opts_default(&o);
        run_cand_form(CandCall{DevCall{set, d_concat, d_offsets, n_seqs, total_bases, o.max_error_prob,
                                       (uint32_t)std::min<size_t>(o.max_gap_len, 0xFFFFFFFFu), strands, d_work, work_bytes, d_runs, capacity, d_n_runs,
                                       static_cast<hipStream_t>(stream)},
                               max_pairs, max_pair_bases, nullptr, d_stats},
                      kCandFind);
    });
}

size_t kbo_summary_refset_screened_dev_work_bytes(const kbo_refset_t *set, size_t n_seqs, uint64_t total_bases, int strands, size_t capacity,
                                                  size_t max_pairs, uint64_t max_pair_bases)
{
    return cand_form(set, n_seqs, total_bases, strands, capacity, max_pairs, max_pair_bases, kCandSummary).end;
}

int kbo_summary_refset_screened_dev(kbo_refset_t *set, const uint8_t *d_concat, const uint64_t *d_offsets, size_t n_seqs, uint64_t total_bases,
                                    double max_error_prob, int strands, void *d_work, size_t work_bytes, kbo_ref_summary *d_records,
                                    size_t capacity, uint64_t *d_n_records, size_t max_pairs, uint64_t max_pair_bases,
                                    kbo_refset_screen_stats *d_stats, void *stream)
{
    return guarded([&] {
        run_cand_form(CandCall{DevCall{set, d_concat, d_offsets, n_seqs, total_bases, max_error_prob, 0u, strands, d_work, work_bytes, d_records, capacity,
                                       d_n_records, static_cast<hipStream_t>(stream)},
                               max_pairs, max_pair_bases, nullptr, d_stats},
                      kCandSummary);
    });
}

size_t kbo_best_refset_screened_dev_work_bytes(const kbo_refset_t *set, size_t n_seqs, uint64_t total_bases, int strands, size_t max_pairs,
                                               uint64_t max_pair_bases)
{
    return cand_form(set, n_seqs, total_bases, strands, 0, max_pairs, max_pair_bases, kCandBest).end;
}

int kbo_best_refset_screened_dev(kbo_refset_t *set, const uint8_t *d_concat, const uint64_t *d_offsets, size_t n_seqs, uint64_t total_bases,
                                 double max_error_prob, int strands, void *d_work, size_t work_bytes, kbo_ref_best *d_out, size_t max_pairs,
                                 uint64_t max_pair_bases, kbo_refset_screen_stats *d_stats, void *stream)
{
    return guarded([&] {
        run_cand_form(CandCall{DevCall{set, d_concat, d_offsets, n_seqs, total_bases, max_error_prob, 0u, strands, d_work, work_bytes, d_out, 0, nullptr,
                                       static_cast<hipStream_t>(stream)},
                               max_pairs, max_pair_bases, nullptr, d_stats},
                      kCandBest);
    });
}

// ---- the locus of a run (refset_locate.hpp; refset_locate_kernels.hip)
} // extern "C"

namespace {
namespace lc = kbo::reflocate;

struct HostSeq { // refset_locate.hpp's accessors over the '+' batch and a reference's entries on the host
    const uint8_t *q_;
    uint32_t byte(uint64_t i) const { return q_[i]; }
};
struct HostPos {
    const uint32_t *pos_;
    uint32_t entry(uint32_t row) const { return pos_[row]; }
};

// what kbo_locate_refset, kbo_cover_refset and their host forms check behind their null arguments, all before any work: the set has
// positions, the batch, then every record; the batch's bases
uint64_t check_positions_batch_runs(const kbo_refset *set, const uint8_t *concat, const uint64_t *offsets, size_t n_seqs, const kbo_ref_run *runs,
                                    uint64_t n_runs)
{
    KBO_REQUIRE(set->positions, KBO_E_BAD_ARG, "the set has no positions (kbo_refset_build_opts)");
    const uint64_t total = check_refset_batch(set, concat, offsets, n_seqs);
    for (uint64_t x = 0; x < n_runs; x++) {
        const kbo_ref_run &w = runs[x];
        KBO_REQUIRE(w.ref < set->descs.size() && packed_ok(set->descs[w.ref]), KBO_E_BAD_ARG,
                    "a run of a reference that is not in the set, has a status or takes the single-index route");
        KBO_REQUIRE(w.seq < n_seqs && (w.strand == KBO_STRAND_FWD || w.strand == KBO_STRAND_REV), KBO_E_BAD_ARG,
                    "a run of a sequence that is not in the batch, or of no strand");
        KBO_REQUIRE(lc::span_ok(offsets[w.seq], offsets[w.seq + 1], total, w.run.start, w.run.end), KBO_E_BAD_ARG,
                    "a run with start > end, or end beyond its sequence");
    }
    return total;
}

uint64_t check_locate(const kbo_refset *set, const uint8_t *concat, const uint64_t *offsets, size_t n_seqs, const kbo_ref_run *runs,
                      uint64_t n_runs, const kbo_ref_locus *loci_out)
{
    KBO_REQUIRE(set && concat && offsets && (n_runs == 0 || (runs && loci_out)), KBO_E_BAD_ARG, "null argument");
    return check_positions_batch_runs(set, concat, offsets, n_seqs, runs, n_runs);
}

kbo::RefsetLocateArgs locate_args(const kbo_refset *set, const DevSet *ds)
{
    kbo::RefsetLocateArgs a{};
    a.descs = ds->descs.as<kbo::RefsetDesc>();
    a.arena = ds->arena.as<uint4>();
    a.positions = ds->pos.as<uint32_t>();
    a.pos_off = ds->pos_off.as<uint64_t>();
    a.n_refs = (uint32_t)set->descs.size();
    a.k = set->k;
    return a;
}
} // namespace

extern "C" {

int kbo_refset_has_positions(const kbo_refset_t *set) { return set && set->positions ? 1 : 0; }

uint64_t kbo_refset_positions_bytes(const kbo_refset_t *set)
{
    if (!set || !set->positions) return 0;
    return (uint64_t)set->pos.size() * sizeof(uint32_t) + (uint64_t)set->pos_off.size() * sizeof(uint64_t);
}

int kbo_refset_positions(const kbo_refset_t *set, size_t r, uint32_t *out, size_t *n_rows)
{
    if (!set || !set->positions || r >= set->descs.size() || !n_rows) return KBO_E_BAD_ARG;
    *n_rows = (size_t)(set->pos_off[r + 1] - set->pos_off[r]);
    if (out && *n_rows) std::memcpy(out, set->pos.data() + set->pos_off[r], *n_rows * sizeof(uint32_t));
    return KBO_OK;
}

uint64_t kbo_refset_ref_len(const kbo_refset_t *set, size_t r) { return set && r < set->ref_len.size() ? set->ref_len[r] : 0; }

int kbo_locate_refset_host(const kbo_refset_t *set, const uint8_t *concat, const uint64_t *offsets, size_t n_seqs, const kbo_ref_run *runs,
                           uint64_t n_runs, kbo_ref_locus *loci_out)
{
    return guarded([&] {
        (void)check_locate(set, concat, offsets, n_seqs, runs, n_runs, loci_out);
        const HostSeq q{concat};
        for (uint64_t x = 0; x < n_runs; x++) {
            const kbo_ref_run &w = runs[x];
            const kbo::RefsetDesc &d = set->descs[w.ref];
            const HostForm form = host_form(set, d);
            const HostPos pos{set->pos.data() + set->pos_off[w.ref]};
            const uint64_t begin = offsets[w.seq], len = offsets[w.seq + 1] - begin;
            const bool rev = w.strand == KBO_STRAND_REV;
            const lc::Locus L = lc::locate_serial(w.run.start, w.run.end, set->k, [&](uint32_t i) {
                return lc::kmer_entry(form, d.n_sets, set->k, q, begin, len, rev, pos, i);
            });
            std::memcpy(&loci_out[x], &L, sizeof L);
        }
    });
}

int kbo_locate_refset(kbo_refset_t *set, const uint8_t *concat, const uint64_t *offsets, size_t n_seqs, const kbo_ref_run *runs,
                      uint64_t n_runs, kbo_ref_locus *loci_out)
{
    return guarded([&] {
        const uint64_t total = check_locate(set, concat, offsets, n_seqs, runs, n_runs, loci_out);
        if (n_runs == 0) return;
        DevSet *ds = device_set(set, current_device());
        StreamScope stream;
        DevBuf d_q((size_t)(total + 15) / 16 * 16 + 16), d_off((n_seqs + 1) * sizeof(uint64_t)), d_runs((size_t)n_runs * sizeof(kbo_ref_run)), d_n(16),
            d_loci((size_t)n_runs * sizeof(kbo_ref_locus));
        HIP_OK(hipMemcpyAsync(d_q.p, concat, total, hipMemcpyHostToDevice, stream.s));
        HIP_OK(hipMemcpyAsync(d_off.p, offsets, (n_seqs + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, stream.s));
        HIP_OK(hipMemcpyAsync(d_runs.p, runs, (size_t)n_runs * sizeof(kbo_ref_run), hipMemcpyHostToDevice, stream.s));
        HIP_OK(hipMemcpyAsync(d_n.p, &n_runs, sizeof(uint64_t), hipMemcpyHostToDevice, stream.s));
        kbo::RefsetLocateArgs a = locate_args(set, ds);
        a.q = d_q.as<uint8_t>();
        a.off = d_off.as<uint64_t>();
        a.runs = d_runs.as<uint32_t>();
        a.n_runs = d_n.as<uint64_t>();
        a.loci = d_loci.as<uint32_t>();
        a.capacity = n_runs;
        a.total = total;
        a.n_seqs = (uint32_t)n_seqs;
        HIP_OK(kbo::launch_refset_locate(a, stream.s));
        HIP_OK(hipMemcpyAsync(loci_out, d_loci.p, (size_t)n_runs * sizeof(kbo_ref_locus), hipMemcpyDeviceToHost, stream.s));
        HIP_OK(hipStreamSynchronize(stream.s)); // the call's one wait
    });
}

int kbo_locate_refset_dev(kbo_refset_t *set, const uint8_t *d_concat, const uint64_t *d_offsets, size_t n_seqs, uint64_t total_bases,
                          const kbo_ref_run *d_runs, const uint64_t *d_n_runs, size_t capacity, kbo_ref_locus *d_loci, void *stream)
{
    return guarded([&] {
        KBO_REQUIRE(set && d_concat && d_offsets && d_n_runs && (capacity == 0 || (d_runs && d_loci)), KBO_E_BAD_ARG, "null argument");
        KBO_REQUIRE(((uintptr_t)d_concat & 15) == 0 && ((uintptr_t)d_offsets & 7) == 0 && ((uintptr_t)d_n_runs & 7) == 0 &&
                        ((uintptr_t)d_runs & 3) == 0 && ((uintptr_t)d_loci & 3) == 0,
                    KBO_E_BAD_ARG, "d_concat 16-byte, d_offsets and the count 8-byte, the records 4-byte aligned");
        KBO_REQUIRE(set->positions, KBO_E_BAD_ARG, "the set has no positions (kbo_refset_build_opts)");
        KBO_REQUIRE(n_seqs > 0, KBO_E_EMPTY_QUERY, "empty batch");
        KBO_REQUIRE(n_seqs < 0xFFFFFFFFull, KBO_E_UNSUPPORTED, "more than 2^32-1 sequences per call");
        bool any_copy;
        {
            std::lock_guard<std::mutex> g(set->mu);
            any_copy = !set->dev.empty();
        }
        KBO_REQUIRE(any_copy, KBO_E_BAD_ARG, "the set has no copy on any device (kbo_refset_to_device)"); // (no device is asked)
        DevSet *ds = device_set_if_any(set, current_device());
        KBO_REQUIRE(ds, KBO_E_BAD_ARG, "the set has no copy on the current device (kbo_refset_to_device)");
        kbo::RefsetLocateArgs a = locate_args(set, ds);
        a.q = d_concat;
        a.off = d_offsets;
        a.runs = reinterpret_cast<const uint32_t *>(d_runs);
        a.n_runs = d_n_runs;
        a.loci = reinterpret_cast<uint32_t *>(d_loci);
        a.capacity = capacity;
        a.total = total_bases;
        a.n_seqs = (uint32_t)n_seqs;
        HIP_OK(kbo::launch_refset_locate(a, static_cast<hipStream_t>(stream)));
    });
}

// ---- depth and breadth of every reference (refset_cover.hpp; refset_cover_kernels.hip)
} // extern "C"

namespace {
namespace cv = kbo::refcover;

struct HostWords { // refset_cover.hpp's accessors over H and the profile on the host
    uint32_t *h_;
    uint32_t get(uint64_t i) const { return h_[i]; }
    void set(uint64_t i, uint32_t v) { h_[i] = v; }
    void add(uint64_t i) { h_[i]++; }
};
struct HostDepth {
    uint32_t *d_;
    void put(uint64_t i, uint32_t v) { d_[i] = v; }
};

// the checks of kbo_cover_refset and its host form, all before any work; the batch's bases
uint64_t check_cover(const kbo_refset *set, const uint8_t *concat, const uint64_t *offsets, size_t n_seqs, const kbo_ref_run *runs, uint64_t n_runs,
                     const kbo_ref_cover *covers_out)
{
    KBO_REQUIRE(set && concat && offsets && covers_out && (n_runs == 0 || runs), KBO_E_BAD_ARG, "null argument");
    return check_positions_batch_runs(set, concat, offsets, n_seqs, runs, n_runs);
}

// the call on the CPU: count, scan and reduce as refset_cover.hpp's serial forms have them
void cover_host(const kbo_refset *set, const uint8_t *concat, const uint64_t *offsets, const kbo_ref_run *runs, uint64_t n_runs,
                kbo_ref_cover *covers_out, uint32_t *depth_out)
{
    const size_t n_refs = set->descs.size();
    std::vector<uint32_t> h((size_t)set->cov_off[n_refs], 0u), ref_runs(n_refs, 0u);
    std::vector<uint64_t> anchors(n_refs, 0), multi(n_refs, 0);
    HostWords H{h.data()};
    const HostSeq q{concat};
    for (uint64_t x = 0; x < n_runs; x++) {
        const kbo_ref_run &w = runs[x];
        const kbo::RefsetDesc &d = set->descs[w.ref];
        const HostForm form = host_form(set, d);
        const HostPos pos{set->pos.data() + set->pos_off[w.ref]};
        const uint64_t begin = offsets[w.seq], len = offsets[w.seq + 1] - begin;
        const bool rev = w.strand == KBO_STRAND_REV;
        cv::count_serial(
            H, set->cov_off[w.ref], (uint32_t)set->ref_len[w.ref], w.run.start, w.run.end, set->k,
            [&](uint32_t i) { return lc::kmer_entry(form, d.n_sets, set->k, q, begin, len, rev, pos, i); }, anchors[w.ref], multi[w.ref]);
        ref_runs[w.ref]++;
    }
    HostDepth depth{depth_out};
    for (size_t r = 0; r < n_refs; r++) {
        const uint32_t len = (uint32_t)set->ref_len[r];
        cv::Cover c = cv::no_entries(len);
        if (packed_ok(set->descs[r])) {
            cv::scan_serial(H, set->cov_off[r], len);
            c = cv::finish(len, cv::reduce_serial(H, set->cov_off[r], len, set->k, depth_out ? &depth : nullptr, set->cov_off[r]), ref_runs[r], anchors[r],
                           multi[r]);
        }
        std::memcpy(&covers_out[r], &c, sizeof c);
    }
}

kbo::RefsetCoverArgs cover_args(const kbo_refset *set, const DevSet *ds)
{
    kbo::RefsetCoverArgs a{};
    const size_t n_refs = set->descs.size();
    a.descs = ds->descs.as<kbo::RefsetDesc>();
    a.arena = ds->arena.as<uint4>();
    a.positions = ds->pos.as<uint32_t>();
    a.pos_off = ds->pos_off.as<uint64_t>();
    a.base_off = ds->cov.as<uint64_t>();
    a.ref_len = reinterpret_cast<const uint32_t *>(ds->cov.as<uint64_t>() + n_refs + 1);
    a.n_refs = (uint32_t)n_refs;
    a.bases = set->cov_off[n_refs];
    a.k = set->k;
    return a;
}
} // namespace

extern "C" {

uint64_t kbo_refset_cover_bases(const kbo_refset_t *set) { return set && set->positions ? set->cov_off.back() : 0; }

int kbo_refset_cover_offsets(const kbo_refset_t *set, uint64_t *out)
{
    if (!set || !set->positions || !out) return KBO_E_BAD_ARG;
    std::memcpy(out, set->cov_off.data(), set->cov_off.size() * sizeof(uint64_t));
    return KBO_OK;
}

size_t kbo_cover_refset_dev_work_bytes(const kbo_refset_t *set)
{
    if (!set || !set->positions) return 0;
    return (size_t)cv::work_bytes(set->descs.size(), set->cov_off.back());
}

int kbo_cover_refset_host(const kbo_refset_t *set, const uint8_t *concat, const uint64_t *offsets, size_t n_seqs, const kbo_ref_run *runs,
                          uint64_t n_runs, kbo_ref_cover *covers_out, uint32_t *depth_out)
{
    return guarded([&] {
        (void)check_cover(set, concat, offsets, n_seqs, runs, n_runs, covers_out);
        cover_host(set, concat, offsets, runs, n_runs, covers_out, depth_out);
    });
}

int kbo_cover_refset(kbo_refset_t *set, const uint8_t *concat, const uint64_t *offsets, size_t n_seqs, const kbo_ref_run *runs, uint64_t n_runs,
                     kbo_ref_cover *covers_out, uint32_t *depth_out)
{
    return guarded([&] {
        const uint64_t total = check_cover(set, concat, offsets, n_seqs, runs, n_runs, covers_out);
        if (n_runs == 0) { // (no device: the records of references nothing was found on, and a profile of zeros)
            cover_host(set, concat, offsets, runs, 0, covers_out, depth_out);
            return;
        }
        DevSet *ds = device_set(set, current_device());
        StreamScope stream;
        const size_t n_refs = set->descs.size(), bases = (size_t)set->cov_off[n_refs], work_bytes = (size_t)cv::work_bytes(n_refs, bases);
        DevBuf d_q((size_t)(total + 15) / 16 * 16 + 16), d_off((n_seqs + 1) * sizeof(uint64_t)), d_runs((size_t)n_runs * sizeof(kbo_ref_run)), d_n(16),
            d_covers(n_refs * sizeof(kbo_ref_cover)), d_work(work_bytes), d_depth(depth_out ? bases * sizeof(uint32_t) + 16 : 0);
        HIP_OK(hipMemcpyAsync(d_q.p, concat, total, hipMemcpyHostToDevice, stream.s));
        HIP_OK(hipMemcpyAsync(d_off.p, offsets, (n_seqs + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, stream.s));
        HIP_OK(hipMemcpyAsync(d_runs.p, runs, (size_t)n_runs * sizeof(kbo_ref_run), hipMemcpyHostToDevice, stream.s));
        HIP_OK(hipMemcpyAsync(d_n.p, &n_runs, sizeof(uint64_t), hipMemcpyHostToDevice, stream.s));
        kbo::RefsetCoverArgs a = cover_args(set, ds);
        a.q = d_q.as<uint8_t>();
        a.off = d_off.as<uint64_t>();
        a.runs = d_runs.as<uint32_t>();
        a.n_runs = d_n.as<uint64_t>();
        a.covers = d_covers.as<uint32_t>();
        a.depth = depth_out ? d_depth.as<uint32_t>() : nullptr;
        a.work = d_work.as<uint8_t>();
        a.capacity = n_runs;
        a.total = total;
        a.n_seqs = (uint32_t)n_seqs;
        HIP_OK(kbo::launch_refset_cover(a, stream.s));
        HIP_OK(hipMemcpyAsync(covers_out, d_covers.p, n_refs * sizeof(kbo_ref_cover), hipMemcpyDeviceToHost, stream.s));
        if (depth_out && bases) HIP_OK(hipMemcpyAsync(depth_out, d_depth.p, bases * sizeof(uint32_t), hipMemcpyDeviceToHost, stream.s));
        HIP_OK(hipStreamSynchronize(stream.s)); // the call's one wait
    });
}

int kbo_cover_refset_dev(kbo_refset_t *set, const uint8_t *d_concat, const uint64_t *d_offsets, size_t n_seqs, uint64_t total_bases,
                         const kbo_ref_run *d_runs, const uint64_t *d_n_runs, size_t capacity, kbo_ref_cover *d_covers, uint32_t *d_depth,
                         void *d_work, size_t work_bytes, void *stream)
{
    return guarded([&] {
        KBO_REQUIRE(set && d_concat && d_offsets && d_n_runs && d_covers && d_work && (capacity == 0 || d_runs), KBO_E_BAD_ARG, "null argument");
        KBO_REQUIRE(((uintptr_t)d_concat & 15) == 0 && ((uintptr_t)d_work & 15) == 0 && ((uintptr_t)d_offsets & 7) == 0 &&
                        ((uintptr_t)d_n_runs & 7) == 0 && ((uintptr_t)d_runs & 3) == 0 && ((uintptr_t)d_covers & 3) == 0 && ((uintptr_t)d_depth & 3) == 0,
                    KBO_E_BAD_ARG, "d_concat and d_work 16-byte, d_offsets and the count 8-byte, the records and d_depth 4-byte aligned");
        KBO_REQUIRE(set->positions, KBO_E_BAD_ARG, "the set has no positions (kbo_refset_build_opts)");
        KBO_REQUIRE(n_seqs > 0, KBO_E_EMPTY_QUERY, "empty batch");
        KBO_REQUIRE(n_seqs < 0xFFFFFFFFull, KBO_E_UNSUPPORTED, "more than 2^32-1 sequences per call");
        KBO_REQUIRE(work_bytes >= kbo_cover_refset_dev_work_bytes(set), KBO_E_BAD_ARG, "work_bytes below the figure of kbo_cover_refset_dev_work_bytes");
        bool any_copy;
        {
            std::lock_guard<std::mutex> g(set->mu);
            any_copy = !set->dev.empty();
        }
        KBO_REQUIRE(any_copy, KBO_E_BAD_ARG, "the set has no copy on any device (kbo_refset_to_device)"); // (no device is asked)
        DevSet *ds = device_set_if_any(set, current_device());
        KBO_REQUIRE(ds, KBO_E_BAD_ARG, "the set has no copy on the current device (kbo_refset_to_device)");
        kbo::RefsetCoverArgs a = cover_args(set, ds);
        a.q = d_concat;
        a.off = d_offsets;
        a.runs = reinterpret_cast<const uint32_t *>(d_runs);
        a.n_runs = d_n_runs;
        a.covers = reinterpret_cast<uint32_t *>(d_covers);
        a.depth = d_depth;
        a.work = static_cast<uint8_t *>(d_work);
        a.capacity = capacity;
        a.total = total_bases;
        a.n_seqs = (uint32_t)n_seqs;
        HIP_OK(kbo::launch_refset_cover(a, static_cast<hipStream_t>(stream)));
    });
}

} // extern "C"

// ---- the variants of a pair (refset_call.hpp; refset_call_kernels.hip)
namespace {
namespace rc = kbo::refcall;

struct CallSite { // a site as the second pass takes it; its window record has the same index
    uint32_t ref, seq, strand, thr, i, j;
};
struct CallSites {
    uint32_t k = 0, stride = 0, pad = 0;
    std::vector<CallSite> sites;
    std::vector<uint8_t> wins;
    void init(uint32_t k_)
    {
        k = k_;
        stride = rc::window_stride(k_);
        pad = rc::window_pad(k_);
    }
};

// the checks of kbo_call_refset and its host form, all before any work: the options, the thresholds, the batch's bases
struct CallCheck {
    kbo_call_opts o;
    std::vector<uint32_t> thr;
    uint64_t total = 0;
};
CallCheck check_call(const kbo_refset *set, const uint8_t *concat, const uint64_t *offsets, size_t n_seqs, const kbo_call_opts *opts, int strands,
                     kbo_ref_calls *out)
{
    static_assert(sizeof(kbo_ref_variant) == 24 && sizeof(rc::Site) == 16, "kbo_ref_variant is 24 bytes, a site record four words");
    KBO_REQUIRE(strands >= 1 && strands <= 3, KBO_E_BAD_ARG, "strands: KBO_STRAND_FWD, KBO_STRAND_REV or both");
    KBO_REQUIRE(set && out, KBO_E_BAD_ARG, "null argument");
    *out = kbo_ref_calls{0, 0, nullptr, nullptr};
    CallCheck c;
    if (opts) c.o = *opts; else kbo_call_opts_default(&c.o);
    KBO_REQUIRE(c.o.sbwt_build_opts.k == set->k, KBO_E_K_MISMATCH, "assert!(sbwt_ref.k() == sbwt_query.k()) (lib.rs:559)");
    for (const kbo::RefsetDesc &d : set->descs)
        KBO_REQUIRE(d.status || d.route != kbo::kRefsetRouteIndex, KBO_E_UNSUPPORTED,
                    "a reference of the single-index route: kbo_call_batch on an index of it (kbo_refset_packed_only)");
    c.thr = refset_thresholds(set, c.o.max_error_prob);
    c.total = check_refset_batch(set, concat, offsets, n_seqs);
    const uint64_t per_base = c.o.sbwt_build_opts.add_revcomp ? 2 : 1;
    for (size_t s = 0; s < n_seqs; s++) // (what RunAutomaton::build refuses)
        KBO_REQUIRE(per_base * (offsets[s + 1] - offsets[s]) < (1ull << 29), KBO_E_UNSUPPORTED,
                    "a sequence of 2^29 bases or more (2^28 with add_revcomp)");
    return c;
}

// The second pass (variant_calling.rs:275-284), as call_batch.cpp does it for a site left to the host: the query-side k-mer and its
// depths from the sequence and the window, the depths of the row's k-mer against the sequence's own index from a suffix automaton of
// the sequence on its strand - one per (sequence, strand) with a site - and resolve_variant with the pair's threshold.  The records
// in the order (reference, sequence, strand, position).
void resolve_sites(const CallSites &S, const uint8_t *concat, const uint64_t *offsets, bool add_revcomp, uint32_t num_threads, kbo_ref_calls *out)
{
    struct Rec {
        uint32_t site, group, chars;
        uint16_t q_len, r_len;
    };
    const uint32_t k = S.k;
    const size_t n = S.sites.size();
    std::vector<uint32_t> order(n);
    for (size_t x = 0; x < n; x++) order[x] = (uint32_t)x;
    auto key = [&](uint32_t x) { return (uint64_t)S.sites[x].seq * 2u + (S.sites[x].strand - 1u); };
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return key(a) != key(b) ? key(a) < key(b) : a < b; });
    std::vector<size_t> first; // the groups: the sites of one (sequence, strand)
    for (size_t x = 0; x < n; x++)
        if (x == 0 || key(order[x]) != key(order[x - 1])) first.push_back(x);
    first.push_back(n);
    const size_t n_groups = first.size() - 1;
    std::vector<std::vector<Rec>> recs(n_groups);
    std::vector<std::vector<uint8_t>> chars(n_groups);
    std::atomic<size_t> next{0};
    std::atomic<int> failed{KBO_OK};
    auto work = [&] {
        RunAutomaton sam;
        std::vector<uint32_t> dq(k), dr(k);
        std::vector<uint8_t> qk(k), rev;
        try {
            for (size_t g; (g = next.fetch_add(1)) < n_groups;) {
                const CallSite &head = S.sites[order[first[g]]];
                const size_t len = (size_t)(offsets[head.seq + 1] - offsets[head.seq]);
                const uint8_t *seq = concat + offsets[head.seq];
                if (head.strand == KBO_STRAND_REV) {
                    revcomp_host(seq, len, rev);
                    seq = rev.data();
                }
                sam.build(seq, len, k, add_revcomp);
                for (size_t y = first[g]; y < first[g + 1]; y++) {
                    const CallSite &w = S.sites[order[y]];
                    const uint8_t *win = S.wins.data() + (size_t)order[y] * S.stride, *rk = win + S.pad;
                    for (uint32_t t = 0; t < k; t++) { // (call_batch.cpp call_slow: variant_calling.rs:46-58, 275, 279)
                        const int64_t pos = (int64_t)w.j - (int64_t)(k - 1u) + t;
                        if (pos < 0) {
                            qk[t] = '$';
                            dr[t] = 0;
                            continue;
                        }
                        qk[t] = seq[pos];
                        dr[t] = std::min<uint32_t>(win[t], (uint32_t)std::min<int64_t>(t + 1u, pos + 1));
                    }
                    sam.depths(rk, k, dq.data()); // (:280)
                    size_t qf, qt, rf, rt;
                    if (!kbo::resolve_variant_ranges(qk.data(), rk, dq.data(), dr.data(), k, w.thr, qf, qt, rf, rt)) continue; // (:282-284)
                    recs[g].push_back(Rec{order[y], (uint32_t)g, (uint32_t)chars[g].size(), (uint16_t)(qt - qf), (uint16_t)(rt - rf)});
                    chars[g].insert(chars[g].end(), qk.begin() + qf, qk.begin() + qt);
                    chars[g].insert(chars[g].end(), rk + rf, rk + rt);
                }
            }
        } catch (const KboError &e) {
            failed = e.code;
        } catch (const std::exception &) {
            failed = KBO_E_NOMEM;
        }
    };
    std::vector<std::thread> team;
    try {
        for (uint32_t t = 1; t < std::min<size_t>(num_threads, n_groups); t++) team.emplace_back(work);
    } catch (const std::exception &) { // (no further thread: those that started and this one share the groups)
    }
    work();
    for (auto &t : team) t.join();
    KBO_REQUIRE(failed.load() == KBO_OK, failed.load(), "the second pass of kbo_call_refset failed");

    std::vector<Rec> all;
    uint64_t n_chars = 0;
    for (size_t g = 0; g < n_groups; g++) {
        all.insert(all.end(), recs[g].begin(), recs[g].end());
        n_chars += chars[g].size();
    }
    KBO_REQUIRE(n_chars < 0xFFFFFFFFull, KBO_E_UNSUPPORTED, "2^32 - 1 characters of variants or more");
    auto less = [&](const Rec &a, const Rec &b) {
        const CallSite &x = S.sites[a.site], &y = S.sites[b.site];
        if (x.ref != y.ref) return x.ref < y.ref;
        if (x.seq != y.seq) return x.seq < y.seq;
        if (x.strand != y.strand) return x.strand < y.strand;
        return x.i < y.i;
    };
    std::sort(all.begin(), all.end(), less);
    t_call[3] = all.size();
    if (all.empty()) return; // (none: the pointers stay NULL)
    MallocPtr<kbo_ref_variant> vars = malloc_array<kbo_ref_variant>(all.size());
    MallocPtr<uint8_t> bytes = malloc_array<uint8_t>((size_t)n_chars);
    uint32_t at = 0;
    for (size_t x = 0; x < all.size(); x++) {
        const Rec &r = all[x];
        const CallSite &w = S.sites[r.site];
        vars.get()[x] = kbo_ref_variant{w.ref, w.seq, w.strand, w.i, at, r.q_len, r.r_len};
        const uint32_t nc = (uint32_t)r.q_len + r.r_len;
        if (nc) std::memcpy(bytes.get() + at, chars[r.group].data() + r.chars, nc);
        at += nc;
    }
    out->n_variants = all.size();
    out->n_chars = n_chars;
    out->variants = vars.release();
    out->chars = n_chars ? bytes.release() : nullptr;
}

uint32_t call_threads()
{
    return std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
}

// kbo_call_refset: behind the summary's stages of a slab, the candidates of its kept pairs, their sites and the sites' windows
struct Caller : SlabWalker {
    DevBuf d_ext, d_pref, d_pq, d_counts, d_cands, d_sites, d_win;
    size_t cap = 0;
    CallSites S;
    std::vector<uint32_t> pq;
    std::vector<rc::Site> got;

    void run_slab(const SlabPlan &P)
    {
        const size_t np = P.pairs();
        if (!np) return;
        d_ext.ensure(np * sizeof(kbo_aln_extent));
        d_pref.ensure(np * sizeof(uint32_t));
        d_pq.ensure(np * sizeof(uint32_t));
        d_counts.ensure(kbo::kRefsetCallCountBytes);
        pq.resize(np);
        for (size_t p = 0; p < np; p++) pq[p] = (uint32_t)((P.strand[p] == KBO_STRAND_REV ? rev_base : 0) + offsets[P.seq[p]]);
        walk_slab(P);
        upload(d_pref.p, P.ref.data(), np * sizeof(uint32_t));
        upload(d_pq.p, pq.data(), np * sizeof(uint32_t));
        HIP_OK(kbo::launch_derand_summary_seq(d_ms.as<uint8_t>(), d_poff.as<uint64_t>(), (uint32_t)np, P.bytes(), k, d_pthr.as<uint32_t>(), min_thr,
                                              d_ext.as<uint32_t>(), d_derand.p, st));
        if (!cap) cap = g_record_capacity.load();
        uint32_t counts[32];
        for (;;) { // (once, unless the slab has more candidates than the lists hold: then once more, with room for the count)
            KBO_REQUIRE(cap < 0xFFFFFFFFull, KBO_E_UNSUPPORTED, "2^32 - 1 candidates or more in a slab");
            d_cands.ensure(cap * sizeof(rc::Cand));
            d_sites.ensure(cap * sizeof(rc::Site));
            d_win.ensure(cap * (size_t)S.stride);
            kbo::RefsetCallArgs a{};
            a.descs = ds->descs.as<kbo::RefsetDesc>();
            a.arena = ds->arena.as<uint4>();
            a.q = d_q.as<uint8_t>();
            a.ms = d_ms.as<uint8_t>();
            a.poff = d_poff.as<uint64_t>();
            a.pthr = d_pthr.as<uint32_t>();
            a.ext = d_ext.as<uint32_t>();
            a.pref = d_pref.as<uint32_t>();
            a.pq = d_pq.as<uint32_t>();
            a.counts = d_counts.as<uint32_t>();
            a.cands = d_cands.as<uint2>();
            a.sites = d_sites.as<uint4>();
            a.win = d_win.as<uint8_t>();
            a.bytes = P.bytes();
            a.n_pairs = (uint32_t)np;
            a.k = k;
            a.min_thr = min_thr;
            a.cap = (uint32_t)cap;
            HIP_OK(kbo::launch_refset_call(a, st));
            HIP_OK(hipMemcpyAsync(counts, d_counts.p, sizeof counts, hipMemcpyDeviceToHost, st));
            HIP_OK(hipStreamSynchronize(st));
            if (counts[0] <= cap) break;
            cap = (size_t)counts[0] + counts[0] / 4 + 16;
        }
        const size_t n_sites = counts[16];
        KBO_REQUIRE(n_sites <= counts[0], KBO_E_HIP, "more sites than candidates");
        t_call[0] += np;
        t_call[1] += counts[0];
        t_call[2] += n_sites;
        t_routes[3]++;
        if (!n_sites) return;
        got.resize(n_sites);
        const size_t w0 = S.wins.size();
        S.wins.resize(w0 + n_sites * S.stride);
        HIP_OK(hipMemcpyAsync(got.data(), d_sites.p, n_sites * sizeof(rc::Site), hipMemcpyDeviceToHost, st));
        HIP_OK(hipMemcpyAsync(S.wins.data() + w0, d_win.p, n_sites * (size_t)S.stride, hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
        for (const rc::Site &w : got) {
            KBO_REQUIRE(w.pair < np, KBO_E_HIP, "a site of no pair of the slab");
            S.sites.push_back(CallSite{P.ref[w.pair], P.seq[w.pair], P.strand[w.pair], P.thr[w.pair], w.i, w.j});
        }
    }
};

struct HostPairSlab { // refset_call.hpp's Slab over the depths of ONE pair on the host
    const uint8_t *ms_;
    uint64_t len_;
    uint32_t thr_;
    uint32_t ms(uint64_t p) const { return ms_[p]; }
    uint64_t off(uint32_t x) const { return x ? len_ : 0u; }
    uint32_t thr(uint32_t) const { return thr_; }
    bool kept(uint32_t) const { return true; }
};
struct HostStrandSeq {
    const uint8_t *q_;
    uint32_t byte(uint32_t s) const { return q_[s]; }
};
struct HostBytes {
    uint8_t *w_;
    void put(uint32_t t, uint32_t v) { w_[t] = (uint8_t)v; }
};
} // namespace

extern "C" {

int kbo_refset_last_call(uint64_t out[4])
{
    if (!out) return KBO_E_BAD_ARG;
    std::copy(t_call, t_call + 4, out);
    return KBO_OK;
}

int kbo_refset_spell_row(const kbo_refset_t *set, size_t r, uint32_t row, uint8_t *out)
{
    const kbo::RefsetDesc *d = packed_desc(set, r);
    if (!d || !out || row >= d->n_sets) return KBO_E_BAD_ARG;
    HostBytes o{out};
    rc::spell_row(host_form(set, *d), d->n_sets, set->k, row, o);
    return KBO_OK;
}

void kbo_ref_calls_free(kbo_ref_calls *calls)
{
    if (!calls) return;
    std::free(calls->variants);
    std::free(calls->chars);
    *calls = kbo_ref_calls{0, 0, nullptr, nullptr};
}

int kbo_call_refset(kbo_refset_t *set, const uint8_t *concat, const uint64_t *offsets, size_t n_seqs, const kbo_call_opts *opts, int strands,
                    kbo_ref_calls *out)
{
    return guarded([&] {
        const CallCheck c = check_call(set, concat, offsets, n_seqs, opts, strands, out);
        std::fill(t_routes, t_routes + 4, 0);
        std::fill(t_wide, t_wide + 2, 0);
        std::fill(t_call, t_call + 4, 0);
        Caller F;
        F.S.init(set->k);
        StreamScope stream;
        upload_batch(F, set, concat, offsets, n_seqs, c.total, strands, stream.s);
        Screen scr;
        run_slabs(F, c.thr, n_seqs, strands, screen_call(F, c.thr, n_seqs, c.total, strands, scr));
        resolve_sites(F.S, concat, offsets, c.o.sbwt_build_opts.add_revcomp != 0, call_threads(), out);
    });
}

int kbo_call_refset_host(const kbo_refset_t *set, const uint8_t *concat, const uint64_t *offsets, size_t n_seqs, const kbo_call_opts *opts,
                         int strands, kbo_ref_calls *out)
{
    return guarded([&] {
        const CallCheck c = check_call(set, concat, offsets, n_seqs, opts, strands, out);
        std::fill(t_call, t_call + 4, 0);
        const uint32_t k = set->k;
        CallSites S;
        S.init(k);
        std::vector<uint8_t> rev, ms;
        for (size_t s = 0; s < n_seqs; s++) {
            const size_t len = (size_t)(offsets[s + 1] - offsets[s]);
            ms.resize(len);
            for (uint32_t strand = 1; strand <= 2; strand++) {
                if (!(strands & strand)) continue;
                const uint8_t *q = concat + offsets[s];
                if (strand == KBO_STRAND_REV) {
                    revcomp_host(q, len, rev);
                    q = rev.data();
                }
                const HostStrandSeq seq{q};
                for (size_t r = 0; r < set->descs.size(); r++) {
                    const kbo::RefsetDesc &d = set->descs[r];
                    if (!packed_ok(d)) continue;
                    KBO_REQUIRE(kbo_refset_ms_host(set, r, q, len, ms.data()) == KBO_OK, KBO_E_BAD_ARG, "kbo_refset_ms_host");
                    t_call[0]++;
                    const uint32_t t = c.thr[r];
                    if (!rc::has_hit([&](uint64_t i) { return (uint32_t)ms[i]; }, len, k, t)) continue; // (no summary record: nothing)
                    const HostPairSlab slab{ms.data(), len, t};
                    const HostForm form = host_form(set, d);
                    for (uint64_t p = 1; p < len; p++) {
                        rc::Cand cand{0, 0};
                        if (!rc::scan_byte(slab, 1u, len, t, p, cand)) continue;
                        t_call[1]++;
                        uint32_t j = 0, row = 0;
                        if (!rc::match_serial(slab, form, d.n_sets, seq, 0u, len, k, t, cand.i, j, row)) continue;
                        t_call[2]++;
                        S.sites.push_back(CallSite{(uint32_t)r, (uint32_t)s, strand, t, cand.i, j});
                        S.wins.resize(S.wins.size() + S.stride, 0);
                        uint8_t *w = S.wins.data() + S.wins.size() - S.stride;
                        HostBytes depths{w}, kmer{w + S.pad};
                        rc::gather_depths(slab, 0u, j, k, depths);
                        rc::spell_row(form, d.n_sets, k, row, kmer);
                    }
                }
            }
        }
        resolve_sites(S, concat, offsets, c.o.sbwt_build_opts.add_revcomp != 0, call_threads(), out);
    });
}

} // extern "C"
