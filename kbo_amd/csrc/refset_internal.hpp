// refset_internal.hpp — what the units of the reference-set calls share: kbo_refset_t and its copies on the
// devices, the checks every call makes, the accessors of the refset_*.hpp arithmetic over the host arrays, the thread's counters,
// and the host slab pipeline that find, summary, best (refset.cpp) and call (refset_calls.cpp) run their stages behind.  The other
// units: refset_dev.cpp (the device-resident forms), refset_runs.cpp (locate and cover).
#pragma once
#include "../../include/kbo_hip_tuning.h"
#include "capi_internal.hpp"
#include "refset_slab.hpp"
#include "refset_step.hpp"

#include <algorithm>

static_assert(kbo::refplan::kTaskItems == kbo::kRefsetThreads, "refset_slab.hpp cuts a task where the walk kernel does");

namespace kbo_host {

constexpr uint64_t kPrefilterMaxBits = 1ull << 31; // the bitmap is read back: above this many bits a call runs unscreened
extern std::atomic<size_t> g_record_capacity;
extern thread_local uint64_t t_pre[4];    // pairs of packed references, with their bit set, walked; the screen ran
extern thread_local uint64_t t_routes[4];
extern thread_local uint64_t t_wide[2];   // references walked by the wide kernel, the tasks it was launched with
extern thread_local uint64_t t_best[2];   // launches of refset_best_kernel: a wave per sequence, a workgroup per sequence
extern thread_local uint64_t t_call[4];   // kbo_call_refset: pairs scanned, candidates, sites, variants
inline int read_counters(const uint64_t *t, size_t n, uint64_t *out) // (the kbo_refset_last_* calls)
{
    if (out) std::copy(t, t + n, out);
    return out ? KBO_OK : KBO_E_BAD_ARG;
}
// what every host call that walks begins with (best and call reset their own counters behind it)
inline void reset_call_counters()
{
    std::fill(t_routes, t_routes + 4, 0);
    std::fill(t_wide, t_wide + 2, 0);
}

struct DevSet {
    DevBuf arena, descs;
    DevBuf pre_bucket, pre_keys, pre_refs; // the seed table of a set with a prefilter
    DevBuf pos, pos_off;                   // the position table of a set with positions, and where each reference's entries begin
    DevBuf cov;                            // ... and its base offsets (n_refs + 1 u64), then every reference's length (n_refs u32)
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
} // namespace kbo_host

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
    std::map<int, std::unique_ptr<kbo_host::DevSet>> dev;
};

namespace kbo_host {

DevSet *device_set(kbo_refset *set, int device); // the set's copy on `device`, made when there is none
// the set's copy on the current device, which a device-resident call never makes: without one the call is refused.  any_first: the
// calls that otherwise ask no device refuse a set without a copy on any device before they ask for the current one
DevSet *require_device_set(kbo_refset *set, bool any_first = false);

inline size_t up16(size_t b) { return (b + 15) / 16 * 16; }
inline void require_strands(int strands) { KBO_REQUIRE(strands >= 1 && strands <= 3, KBO_E_BAD_ARG, "strands: KBO_STRAND_FWD, KBO_STRAND_REV or both"); }
inline bool packed_ok(const kbo::RefsetDesc &d) { return !d.status && d.route != kbo::kRefsetRouteIndex; }
inline const kbo::RefsetDesc *packed_desc(const kbo_refset *set, size_t r)
{
    return set && r < set->descs.size() && packed_ok(set->descs[r]) ? &set->descs[r] : nullptr;
}
// what the device-resident forms and the call refuse: a set with a reference of the single-index route
inline bool packed_only(const kbo_refset *set)
{
    return std::none_of(set->descs.begin(), set->descs.end(), [](const kbo::RefsetDesc &d) { return !d.status && d.route == kbo::kRefsetRouteIndex; });
}

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
inline HostForm host_form(const kbo_refset *set, const kbo::RefsetDesc &d)
{
    const uint32_t *form = set->arena.data() + (size_t)d.off * 4u;
    return HostForm{form, reinterpret_cast<const uint8_t *>(form + 4u * (size_t)kbo::refset_rank_units(d.n_sets))};
}
struct HostSeq { // refset_locate.hpp's accessors over the '+' batch and a reference's entries on the host
    const uint8_t *q_;
    uint32_t byte(uint64_t i) const { return q_[i]; }
};
struct HostPos {
    const uint32_t *pos_;
    uint32_t entry(uint32_t row) const { return pos_[row]; }
};

// the reverse complement as revcomp_kernels.hip makes it: A <-> T, C <-> G in either case, any other byte as it is
void revcomp_host(const uint8_t *fwd, size_t len, std::vector<uint8_t> &out);
// the threshold of every reference that can be queried (lib.rs:620); the errors of kbo_find on its handle
std::vector<uint32_t> refset_thresholds(const kbo_refset *set, double max_error_prob);
// the checks on the batch, all before the first HIP call; its bases
uint64_t check_refset_batch(const kbo_refset *set, const uint8_t *concat, const uint64_t *offsets, size_t n_seqs);
inline uint64_t screen_bits(const kbo_refset *set, size_t n_seqs) { return (uint64_t)set->descs.size() * n_seqs * 2u; }
// m_r of every reference for this call's thresholds; 0: the reference is not packed or cannot be queried (it has no entries)
std::vector<uint8_t> seed_lens(const kbo_refset *set, const std::vector<uint32_t> &thr);
// the screen kernel's arguments that the set and the batch's shape give; m, q, off and bits are the caller's
kbo::RefsetScreenArgs screen_args(const DevSet *ds, size_t n_seqs, uint64_t total, int strands);

// ---- the walk
inline void add_kind(WalkKinds &w, const kbo::RefsetDesc &d)
{
    const bool wide = d.route == kbo::kRefsetRouteWide;
    w.has_wide |= wide;
    w.has_lds |= !wide;
    if (!wide) w.lds_units = std::max(w.lds_units, kbo::refset_units(d.n_sets));
}
// of the references [first, last) that can be queried
inline WalkKinds walk_kinds(const kbo_refset *set, size_t first, size_t last)
{
    WalkKinds w;
    for (size_t r = first; r < last; r++)
        if (!set->descs[r].status) add_kind(w, set->descs[r]);
    return w;
}
// the walk of a slab's tasks: only the kernels of the kinds of reference it holds (each kernel skips the other's tasks)
void launch_walks(const DevSet *ds, const uint4 *tasks, const uint4 *items, uint32_t n_tasks, uint32_t k, const uint8_t *q, uint8_t *ms,
                  const WalkKinds &kinds, hipStream_t st);

// ---- the host slab pipeline
// A slab's uploads through pinned memory, two sets in turn: a walker that synchronises nothing per slab (Bester) plans the next
// slab while the device runs this one, and the slab's host arrays are free to change as soon as run_slab returns.  A set is taken
// again only when the copies out of it have run (its event).
struct SlabStage {
    PinBuf pin[2];
    hipEvent_t ev[2] = {nullptr, nullptr};
    bool used[2] = {false, false};
    size_t at = 0;
    int cur = 1;
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
        at += up16(bytes);
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

// what kbo_find_refset, kbo_summary_refset, kbo_best_refset and kbo_call_refset share: the batch on the device, slabs of pairs and
// their walk
struct SlabWalker : SlabBatch { // (rev_base: where the '-' strand of the batch begins in d_q)
    kbo_refset *set;
    SlabStage *stage = nullptr; // where the slab's arrays are copied from when they may change before the copies have run
    uint32_t min_thr;           // the smallest threshold of the references that take a walk of the packed form
    hipStream_t st;
    DevSet *ds;
    DevBuf d_q, d_off, d_ms, d_poff, d_pthr, d_items, d_tasks, d_derand;
    std::vector<uint64_t> ref_begin, ref_end; // where every reference's records lie in the call's list
    std::vector<uint8_t> walked;              // per reference: a launch of its walk kernel has held it (the route counters)

    void add_pair(SlabPlan &P, uint32_t r, uint32_t s, uint32_t strand, uint32_t threshold)
    {
        kbo_host::add_pair(P, *this, r, s, strand, threshold);
        add_kind(P.kinds, set->descs[r]);
    }
    // the slab's pairs, thresholds and tasks to the device, and the walk: the MS bytes of every pair in d_ms
    void walk_slab(const SlabPlan &P);
    // the counting form of derandomize + translate behind the walk: six u32 a pair at d_ext
    void summarize(const SlabPlan &P, DevBuf &d_ext);
    static size_t slab_buffer_bytes(const SlabPlan &P) { return up16((size_t)P.bytes()) + 64; }
    void upload(void *dst, const void *src, size_t bytes)
    {
        HIP_OK(hipMemcpyAsync(dst, stage ? stage->put(src, bytes) : src, bytes, hipMemcpyHostToDevice, st));
    }
    // what walk_slab puts into the stage
    static size_t stage_bytes(const SlabPlan &P)
    {
        return up16((P.pairs() + 1) * sizeof(uint64_t)) + up16(P.pairs() * sizeof(uint32_t)) + up16(P.items.size() * sizeof(uint32_t)) +
               up16(P.tasks.size() * sizeof(uint32_t));
    }
};

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

// the batch to the device, once; its '-' strand behind it, made where it is
void upload_batch(SlabWalker &F, kbo_refset *set, const uint8_t *concat, const uint64_t *offsets, size_t n_seqs, uint64_t total, int strands,
                  hipStream_t stream);
// what a host call does behind upload_batch: the counters of kbo_refset_last_prefilter, and the screen when the set has a prefilter
// and the bitmap is within the cap.  Returns the screen run_slabs goes by, or null: every pair.
const Screen *screen_call(SlabWalker &F, const std::vector<uint32_t> &thr, size_t n_seqs, uint64_t total, int strands, Screen &scr);

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
        if (packed_ok(set->descs[r])) f.min_thr = std::min(f.min_thr, thr[r]);
    SlabPlan P;
    for (size_t r = 0; r < n_refs; r++) {
        if (!packed_ok(set->descs[r])) continue;
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
    if (P.pairs()) f.run_slab(P);
}

} // namespace kbo_host
