// refset_dev.cpp — the device-resident reference-set calls (kbo_hip.h): the stages of refset.cpp's host calls
// enqueued on the caller's stream over the caller's work buffer, nothing read back.  Two forms share their checks, the strand
// buffer, the walk and the stages behind it:
//   unscreened  kbo_find_refset_dev, kbo_summary_refset_dev, kbo_best_refset_dev, kbo_call_refset_dev: slabs of queryable references
//               against the whole batch, planned on the device (refset_plan_kernels.hip)
//   screened    kbo_refset_candidates_dev, kbo_*_refset_screened_dev: the screen kernel, and ONE slab of the candidate pairs within the
//               caller's caps (refset_cand_kernels.hip)
// Every *_work_bytes figure is the end of a layout below; the calls run at exactly that figure.
#include "refset_internal.hpp"
#include "refset_call.hpp"
#include "refset_cand.hpp"
#include "refset_resolve.hpp"
#include "refset_screen.hpp"

using namespace kbo_host;

namespace {
enum Kind { kSummary, kFind, kBest, kCandidatesOnly, kCall }; // (kCandidatesOnly: the screen alone, which only the screened form has)

// ---- what the two forms share
// the regions of d_work a slab's walk and the stages behind it take: `pairs` sequences over `bytes` bytes to those stages
struct Tail {
    size_t poff = 0, pthr = 0, items = 0, tasks = 0, ms = 0, derand = 0, chars = 0, stage = 0, first = 0, local = 0, end = 0;
    uint64_t local_cap = 0; // records of the slab-local buffer (find)
};

Tail tail_layout(size_t w, uint32_t k, uint64_t pairs, uint64_t bytes, uint64_t item_slots, uint64_t task_slots, size_t capacity, Kind kind)
{
    Tail t;
    t.poff = w;   w += up16((size_t)(pairs + 1) * sizeof(uint64_t));
    t.pthr = w;   w += up16((size_t)pairs * sizeof(uint32_t));
    t.items = w;  w += (size_t)item_slots * sizeof(uint4);
    t.tasks = w;  w += (size_t)task_slots * sizeof(uint4);
    t.ms = w;     w += up16((size_t)bytes) + 64;
    // (the thresholds depend on max_error_prob, which the figure does not know: room for the lowest one there is)
    t.derand = w; w += up16(kbo::derand_seq_work_bytes((uint32_t)pairs, bytes, k, 2));
    if (kind == kFind) {
        t.local_cap = std::min<uint64_t>(capacity, bytes / 2 + pairs); // (a run holds a character other than '-' and ends at one)
        t.chars = w; w += up16((size_t)bytes) + 64;
        t.stage = w; w += up16(kbo::rle_seg_work_bytes((uint32_t)pairs, bytes));
        t.first = w; w += up16((size_t)(pairs + 1) * sizeof(uint32_t));
        t.local = w; w += up16((size_t)t.local_cap * kRleWords * sizeof(uint32_t));
    } else {
        t.chars = w; w += up16((size_t)pairs * sizeof(kbo_aln_extent));                                   // the extents
        if (kind == kSummary) { // (best: the extents are merged into the caller's table where they are)
            t.stage = w; w += up16(kbo::chunk_items_scratch_words((uint32_t)pairs) * sizeof(uint32_t));   // launch_refset_keep's scan
            t.local = w; w += up16((size_t)pairs * 7 * sizeof(uint32_t));                                // the kept list
        } else if (kind == kCall) {
            t.local = w; w += up16((size_t)pairs * 3 * sizeof(uint32_t));                                // RefsetSitePairs: three words a pair
        }
    }
    t.end = w;
    return t;
}

// ---- call: the regions behind everything else, so that no other figure moves.  A slab's candidates, sites and windows (max_sites of
// each); the call's list of tagged sites and their windows; the index of the '+' batch and its sort's other buffer (16 bytes a
// base), the radix passes' histograms; a resolve word, two key words twice, two counts a site
constexpr uint64_t kCallMaxSites = 1ull << 23; // (a site has at most 510 characters, and a record's `chars` is 32 bits)
constexpr size_t kScanValuesPerBlock = 1024;   // (values per block of launch_scan: device_util.hpp kScanBlock)
struct CallStage {
    size_t counts = 0, cands = 0, sites = 0, win = 0;
    size_t tags = 0, wins = 0, ix[2] = {0, 0}, hist = 0, sums = 0, words = 0, keys[2] = {0, 0}, vcnt = 0, ccnt = 0, vsums = 0, csums = 0, end = 0;
};
CallStage call_stage_layout(size_t w, uint32_t k, uint64_t total, uint64_t max_sites)
{
    CallStage s;
    const size_t stride = kbo::refcall::window_stride(k), tiles = kbo::build_tiles(std::max<uint64_t>(total, max_sites));
    const size_t scan_sums = up16(((size_t)(max_sites + 1) / kScanValuesPerBlock + 1) * sizeof(uint32_t));
    s.counts = w;  w += kbo::kRefsetCallCountBytes;
    s.cands = w;   w += up16((size_t)max_sites * sizeof(uint2));
    s.sites = w;   w += (size_t)max_sites * sizeof(uint4);
    s.win = w;     w += (size_t)max_sites * stride;
    s.tags = w;    w += (size_t)max_sites * kbo::kRefsetSiteTagWords * sizeof(uint32_t);
    s.wins = w;    w += (size_t)max_sites * stride;
    for (size_t &o : s.ix) { o = w; w += up16((size_t)total * sizeof(uint64_t)); }
    s.hist = w;    w += up16(256 * tiles * sizeof(uint32_t));
    s.sums = w;    w += up16((256 * tiles / kScanValuesPerBlock + 2) * sizeof(uint32_t));
    s.words = w;   w += up16((size_t)max_sites * sizeof(uint32_t));
    for (size_t &o : s.keys) { o = w; w += (size_t)max_sites * 2 * sizeof(uint64_t); }
    s.vcnt = w;    w += up16((size_t)(max_sites + 1) * sizeof(uint32_t));
    s.ccnt = w;    w += up16((size_t)(max_sites + 1) * sizeof(uint32_t));
    s.vsums = w;   w += scan_sums;
    s.csums = w;   w += scan_sums;
    s.end = w;
    return s;
}

// a walked slab as the stages behind the walk take it; total: the count launch_refset_keep leaves (summary)
struct TailRun {
    uint8_t *w;
    const Tail &t;
    uint32_t pairs;
    uint64_t bytes;
    uint32_t k, min_thr, gap;
    uint32_t *total;
    hipStream_t st;
};

// The stages behind the walk: find - derandomize + translate, the runs counted and emitted; summary - the extents, those with a hit
// kept; best - the extents.  What ends the tail differs between the forms (which kernel tags the records with their pairs, or merges
// the extents): `tag` enqueues it.
template <typename Tag> void enqueue_tail(Kind kind, const TailRun &r, Tag tag)
{
    const Tail &t = r.t;
    auto at = [&](size_t o) { return reinterpret_cast<uint32_t *>(r.w + o); };
    const uint8_t *ms = r.w + t.ms;
    const uint64_t *poff = reinterpret_cast<const uint64_t *>(r.w + t.poff);
    if (kind == kFind) {
        HIP_OK(kbo::launch_derand_translate_seq(ms, poff, r.pairs, r.bytes, r.k, at(t.pthr), r.min_thr, nullptr, r.w + t.chars, r.w + t.derand, r.st));
        HIP_OK(kbo::launch_rle_seg_count(r.w + t.chars, poff, r.pairs, r.bytes, r.gap, 0u, r.w + t.stage, at(t.first), r.st));
        if (t.local_cap)
            HIP_OK(kbo::launch_rle_seg_emit(r.w + t.chars, r.pairs, r.bytes, r.gap, r.w + t.stage, at(t.local), (uint32_t)t.local_cap, r.st));
    } else {
        HIP_OK(kbo::launch_derand_summary_seq(ms, poff, r.pairs, r.bytes, r.k, at(t.pthr), r.min_thr, at(t.chars), r.w + t.derand, r.st));
        if (kind == kSummary) HIP_OK(kbo::launch_refset_keep(at(t.chars), r.pairs, at(t.stage), at(t.local), r.total, r.st));
    }
    tag();
}

// (best: d_out is the table of n_seqs records, there is no capacity and no d_n; the caps, d_bits and d_stats: the screened form's)
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
    size_t max_pairs = 0;
    uint64_t max_bases = 0;
    uint32_t *d_bits = nullptr; // kCandidatesOnly: the caller's bitmap
    kbo_refset_screen_stats *d_stats = nullptr;
    // kCall: d_out / capacity are the variants and max_variants, there is no d_n
    uint32_t opts_k = 0, add_revcomp = 0;
    size_t max_sites = 0, max_chars = 0;
    uint8_t *d_chars = nullptr;
    kbo_ref_calls_stats *d_calls = nullptr;
};
// what sizes a layout besides the batch: the records' capacity, or the sites of a call
size_t layout_capacity(const DevCall &c, Kind kind) { return kind == kCall ? c.max_sites : c.capacity; }

constexpr uint64_t kCandMaxPairs = (1ull << 28) - 1, kCandMaxBases = (1ull << 32) - 17; // what the ONE slab of the screened form may hold

// the checks of a call's arguments, in the order the calls report them; the thresholds.  Each form then checks d_work against its
// own layout and asks for the set's copy on the current device
std::vector<uint32_t> check_dev_call(const DevCall &c, Kind kind, bool screened)
{
    const bool best = kind == kBest, only = kind == kCandidatesOnly, call = kind == kCall;
    require_strands(c.strands);
    KBO_REQUIRE(c.set && c.d_concat && c.d_offsets && c.d_work && (c.d_stats || !screened) && (only ? c.d_bits != nullptr : (c.d_n || best || call)) &&
                    (only || c.d_out || (c.capacity == 0 && !best)) && (!call || (c.d_calls && (c.d_chars || c.max_chars == 0))),
                KBO_E_BAD_ARG, "null argument");
    KBO_REQUIRE(((uintptr_t)c.d_concat & 15) == 0 && ((uintptr_t)c.d_work & 15) == 0 && ((uintptr_t)c.d_offsets & 7) == 0 &&
                    ((uintptr_t)c.d_n & 7) == 0 && ((uintptr_t)c.d_out & 3) == 0 && ((uintptr_t)c.d_stats & 7) == 0 && ((uintptr_t)c.d_bits & 3) == 0 &&
                    ((uintptr_t)c.d_calls & 7) == 0,
                KBO_E_BAD_ARG,
                screened ? "d_concat and d_work 16-byte, d_offsets, the count and d_stats 8-byte, the records and d_bits 4-byte aligned"
                         : "d_concat and d_work 16-byte, d_offsets and the count 8-byte, the records 4-byte aligned");
    KBO_REQUIRE(c.n_seqs > 0, KBO_E_EMPTY_QUERY, "empty batch");
    if (screened) {
        KBO_REQUIRE(c.set->prefilter, KBO_E_BAD_ARG, "the set has no prefilter (kbo_refset_build_opts)");
        KBO_REQUIRE(only || c.max_pairs > 0, KBO_E_BAD_ARG, "max_pairs == 0");
    }
    std::vector<uint32_t> thr = refset_thresholds(c.set, c.max_error_prob);
    KBO_REQUIRE(packed_only(c.set), KBO_E_UNSUPPORTED, "a reference of the single-index route: the host calls take it (kbo_refset_packed_only)");
    if (screened) {
        KBO_REQUIRE(screen_bits(c.set, c.n_seqs) <= kPrefilterMaxBits, KBO_E_UNSUPPORTED, "a bitmap of more than 2^31 bits");
        KBO_REQUIRE(only || (c.max_pairs <= kCandMaxPairs && c.max_bases <= kCandMaxBases), KBO_E_UNSUPPORTED,
                    "caps beyond one slab: 2^28 pairs or more, or more than 2^32 - 17 bases (the unscreened form cuts several slabs)");
    }
    if (call) { // (behind the device forms' checks: the call's own)
        KBO_REQUIRE(c.opts_k == c.set->k, KBO_E_K_MISMATCH, "assert!(sbwt_ref.k() == sbwt_query.k()) (lib.rs:559)");
        KBO_REQUIRE(c.max_sites > 0, KBO_E_BAD_ARG, "max_sites == 0");
        KBO_REQUIRE(c.max_sites <= kCallMaxSites, KBO_E_UNSUPPORTED, "max_sites above 2^23");
    }
    return thr;
}

// ONE query buffer for the walk (and the screen): the caller's for '+' alone; a copy of '+' at q with '-' made behind it, 16-byte
// aligned; or '-' alone at q.  Returns the buffer
const uint8_t *prepare_strands(const DevCall &c, uint8_t *q)
{
    if (c.strands == 1) return c.d_concat;
    if (c.strands == 3 && c.total_bases) HIP_OK(hipMemcpyAsync(q, c.d_concat, c.total_bases, hipMemcpyDeviceToDevice, c.stream));
    HIP_OK(kbo::launch_revcomp_bytes(c.d_concat, c.d_offsets, (uint32_t)c.n_seqs, c.total_bases, q + (c.strands == 3 ? up16(c.total_bases) : 0), c.stream));
    return q;
}

// ---- call: what the two forms share behind the extents of a slab, and behind the last slab
struct CallRun {
    kbo::RefsetSitePairs pairs;
    kbo::RefsetResolveArgs r;
};
CallRun call_run(const DevCall &c, uint8_t *w, const Tail &t, const CallStage &s, uint64_t pairs, const uint8_t *walk_q, uint32_t min_thr)
{
    namespace rr = kbo::refresolve;
    auto at = [&](size_t o) { return reinterpret_cast<uint32_t *>(w + o); };
    auto at64 = [&](size_t o) { return reinterpret_cast<uint64_t *>(w + o); };
    CallRun R{};
    R.pairs = kbo::RefsetSitePairs{at(t.local), at(t.local) + pairs, at(t.local) + 2 * pairs};
    kbo::RefsetResolveArgs &r = R.r;
    r.concat = c.d_concat;
    r.q = walk_q;
    r.off = c.d_offsets;
    r.total = c.total_bases;
    r.n_seqs = (uint32_t)c.n_seqs;
    r.k = c.set->k;
    r.qlen = rr::qmer_len(min_thr, c.set->k);
    r.add_revcomp = c.add_revcomp;
    r.max_sites = (uint32_t)c.max_sites;
    r.tags = at(s.tags);
    r.wins = w + s.wins;
    r.ix[0] = at64(s.ix[0]);
    r.ix[1] = at64(s.ix[1]);
    r.keys[0] = at64(s.keys[0]);
    r.keys[1] = at64(s.keys[1]);
    r.hist = at(s.hist);
    r.sums = at(s.sums);
    r.words = at(s.words);
    r.vcnt = at(s.vcnt);
    r.ccnt = at(s.ccnt);
    r.vsums = at(s.vsums);
    r.csums = at(s.csums);
    const rr::KeyShape shape = rr::key_shape(c.set->descs.size(), c.n_seqs, c.total_bases);
    r.key_seq_bits = shape.seq_bits;
    r.key_hi_bits = shape.hi_bits;
    r.key_i_bits = shape.i_bits;
    r.variants = static_cast<uint32_t *>(c.d_out);
    r.chars = c.d_chars;
    r.max_variants = c.capacity;
    r.max_chars = c.max_chars;
    r.stats = reinterpret_cast<uint64_t *>(c.d_calls);
    return R;
}
// behind the extents of a slab whose RefsetSitePairs the form has made: Caller::run_slab's launch_refset_call, and the sites appended
void enqueue_call_slab(const DevSet *ds, const CallRun &R, uint8_t *w, const Tail &t, const CallStage &s, uint32_t pairs, uint64_t bytes, uint32_t min_thr,
                       hipStream_t st)
{
    if (!pairs || !bytes) return;
    kbo::RefsetCallArgs a{};
    a.descs = ds->descs.as<kbo::RefsetDesc>();
    a.arena = ds->arena.as<uint4>();
    a.q = R.r.q;
    a.ms = w + t.ms;
    a.poff = reinterpret_cast<const uint64_t *>(w + t.poff);
    a.pthr = reinterpret_cast<const uint32_t *>(w + t.pthr);
    a.ext = reinterpret_cast<const uint32_t *>(w + t.chars);
    a.pref = R.pairs.pref;
    a.pq = R.pairs.pq;
    a.counts = reinterpret_cast<uint32_t *>(w + s.counts);
    a.cands = reinterpret_cast<uint2 *>(w + s.cands);
    a.sites = reinterpret_cast<uint4 *>(w + s.sites);
    a.win = w + s.win;
    a.bytes = bytes;
    a.n_pairs = pairs;
    a.k = R.r.k;
    a.min_thr = min_thr;
    a.cap = R.r.max_sites;
    HIP_OK(kbo::launch_refset_call(a, st));
    HIP_OK(kbo::launch_refset_sites_append(a, R.pairs, R.r, st));
}

// ---- the unscreened form: a slab is a range of queryable references against the whole batch
struct DevForm {
    kbo::refplan::Geometry g;
    uint32_t n_refs = 0, n_q = 0, max_refs = 0, refs = 0; // references of the set, queryable ones, the most a slab may hold, a slab's
    size_t q = 0, nch = 0, qflag = 0, qref = 0, thr = 0, total = 0; // per call ...
    Tail t;                                                         // ... and per slab
    CallStage cs;                                                   // (call)
    size_t end = 0;  // the figure
    bool ok = false; // false: a limit of the kernels is exceeded even with one reference per slab
};

// the layout of d_work for slabs of refs_per_slab references (0: as many as a slab may hold; more than that: that many)
DevForm dev_form(const kbo_refset *set, size_t n_seqs, uint64_t total, int strands, size_t capacity, size_t refs_per_slab, Kind kind)
{
    DevForm F;
    if (!set || n_seqs == 0 || strands < 1 || strands > 3 || !packed_only(set)) return F; // (the call refuses them)
    if (kind == kCall && (capacity == 0 || capacity > kCallMaxSites)) return F;              // (call: capacity is max_sites)
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
    const size_t rev = up16((size_t)total);
    size_t w = 0;
    F.q = w;      w += strands == 1 ? 0 : (strands == 3 ? 2 * rev : rev) + 64;
    F.nch = w;    w += up16(kbo::chunk_items_scratch_words((uint32_t)n_seqs) * sizeof(uint32_t));
    F.qflag = w;  w += up16(kbo::chunk_items_scratch_words(F.n_refs) * sizeof(uint32_t));
    F.qref = w;   w += up16((size_t)F.n_refs * sizeof(uint32_t));
    F.thr = w;    w += up16((size_t)F.n_refs * sizeof(uint32_t));
    F.total = w;  w += 16;
    F.t = tail_layout(w, set->k, R * n_seqs * ns, R * ns * total, R * F.g.item_slots, R * F.g.tasks_per_ref, capacity, kind);
    F.end = F.t.end;
    if (kind == kCall) { // (the figure is never below the summary's: many pairs and few sites would put it there)
        F.cs = call_stage_layout(F.t.end, set->k, total, capacity);
        F.end = std::max(F.cs.end, tail_layout(w, set->k, R * n_seqs * ns, R * ns * total, R * F.g.item_slots, R * F.g.tasks_per_ref, 0, kSummary).end);
    }
    F.ok = true;
    return F;
}

void run_dev_form(const DevCall &c, Kind kind)
{
    const bool find = kind == kFind, best = kind == kBest, call = kind == kCall;
    const std::vector<uint32_t> thr = check_dev_call(c, kind, false);
    kbo_refset *set = c.set;
    const size_t cap = layout_capacity(c, kind);
    DevForm F = dev_form(set, c.n_seqs, c.total_bases, c.strands, cap, 1, kind);
    KBO_REQUIRE(F.ok, KBO_E_UNSUPPORTED, "a slab of one reference of 2^32 - 16 bytes or more, or 2^28 (sequence, strand) pairs or more");
    KBO_REQUIRE(c.work_bytes >= F.end, KBO_E_BAD_ARG, "work_bytes too small for one reference a slab");
    uint32_t lo = 1, hi = F.max_refs; // the largest refs_per_slab whose figure fits: the figure is monotonic
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo + 1) / 2;
        if (dev_form(set, c.n_seqs, c.total_bases, c.strands, cap, mid, kind).end <= c.work_bytes) lo = mid;
        else hi = mid - 1;
    }
    F = dev_form(set, c.n_seqs, c.total_bases, c.strands, cap, lo, kind);
    DevSet *ds = require_device_set(set);

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
    HIP_OK(hipMemcpyAsync(w + F.thr, thr.data(), thr.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    const uint8_t *q = prepare_strands(c, w + F.q);
    kbo::RefsetPlan P;
    P.g = F.g;
    P.off = c.d_offsets;
    P.thr = at(F.thr);
    P.nch = at(F.nch);
    P.nch_sums = at(F.nch) + c.n_seqs + 1;
    P.qref = at(F.qref);
    uint64_t *d_n = best || call ? reinterpret_cast<uint64_t *>(w + F.total) : c.d_n; // (best, call: the count the planner zeroes lies in d_work)
    HIP_OK(kbo::launch_refset_plan_call(P, F.n_refs, at(F.nch), at(F.qflag), at(F.qref), d_n, st));
    if (call) HIP_OK(hipMemsetAsync(c.d_calls, 0, sizeof(kbo_ref_calls_stats), st));
    if (best) {
        HIP_OK(kbo::launch_refset_best_init(static_cast<uint32_t *>(c.d_out), (uint32_t)c.n_seqs, st));
        std::fill(t_best, t_best + 2, 0);
    }
    if (c.total_bases == 0) return; // (no base, no record)

    const Tail &t = F.t;
    uint32_t *out = static_cast<uint32_t *>(c.d_out);
    CallRun R{};
    if (call) R = call_run(c, w, t, F.cs, (uint64_t)F.refs * c.n_seqs * F.g.n_strands, q, min_thr);
    for (size_t q0 = 0; q0 < qrefs.size(); q0 += F.refs) {
        const uint32_t refs = (uint32_t)std::min<size_t>(F.refs, qrefs.size() - q0);
        const uint32_t np = refs * (uint32_t)c.n_seqs * F.g.n_strands;
        uint4 *items = reinterpret_cast<uint4 *>(w + t.items), *tasks = reinterpret_cast<uint4 *>(w + t.tasks);
        HIP_OK(kbo::launch_refset_plan_slab(P, (uint32_t)q0, refs, reinterpret_cast<uint64_t *>(w + t.poff), at(t.pthr), find ? w + t.chars : nullptr,
                                            items, tasks, st));
        // (qrefs holds every queryable reference in order: the slab's are those of this range of the set)
        launch_walks(ds, tasks, items, refs * F.g.tasks_per_ref, set->k, q, w + t.ms, walk_kinds(set, qrefs[q0], (size_t)qrefs[q0 + refs - 1] + 1), st);
        const TailRun run{w, t, np, kbo::refplan::slab_bytes(F.g, refs), set->k, min_thr, c.gap, at(F.total), st};
        enqueue_tail(kind, run, [&] {
            if (find) {
                HIP_OK(kbo::launch_refset_tag_runs(P, (uint32_t)q0, np, at(t.first), at(t.local), (uint32_t)t.local_cap, c.d_n, c.capacity, out, st));
            } else if (call) {
                HIP_OK(kbo::launch_refset_site_pairs_plan(P, (uint32_t)q0, np, R.pairs, st));
                enqueue_call_slab(ds, R, w, t, F.cs, np, run.bytes, min_thr, st);
            } else if (best) {
                kbo::RefsetBestArgs b;
                b.ext = at(t.chars);
                b.refs = at(F.qref) + q0;
                b.table = out;
                b.n_pairs = np;
                b.lead = 0;
                b.slab_refs = refs;
                b.n_seqs = (uint32_t)c.n_seqs;
                b.n_strands = F.g.n_strands;
                b.strands = (uint32_t)c.strands;
                HIP_OK(kbo::launch_refset_best(b, st));
                t_best[kbo::refset_best_splits(b.n_seqs) ? 1 : 0]++;
            } else {
                HIP_OK(kbo::launch_refset_tag_summaries(P, (uint32_t)q0, np, at(t.local), at(F.total), c.d_n, c.capacity, out, st));
            }
        });
    }
    if (call) HIP_OK(kbo::launch_refset_resolve(R.r, st));
}

// ---- the screened form: the screen kernel over the batch where it is, the bitmap to the list of its set bits, and ONE slab of the
// list's longest prefix within the caller's caps planned from it (refset_cand_kernels.hip).  The stages behind the walk see the slab
// as max_pairs sequences over max_pair_bases bytes, of which those behind the walked pairs are empty: their total_bases only bounds
// their chunk lists (derand_seq_kernels.hip seq_layout, rle_seg_kernels.hip seg_layout), and walked_bases / 128 + n_walked chunks
// are within max_pair_bases / 128 + max_pairs.
struct CandForm {
    uint32_t n_refs = 0, n_q = 0, words = 0, chunk = 0;
    uint64_t n_bits = 0, item_slots = 0, task_slots = 0;
    size_t rev = 0; // bytes of one strand of the batch in the query buffer
    size_t q = 0, thr = 0, pc = 0, hdr = 0, bits = 0, list = 0, bsum = 0, nch = 0, rfirst = 0, ntask = 0, total = 0, end = 0;
    Tail t;
    CallStage cs; // (call)
    bool ok = false;
};

CandForm cand_form(const kbo_refset *set, size_t n_seqs, uint64_t total, int strands, size_t capacity, size_t max_pairs, uint64_t max_bases, Kind kind)
{
    CandForm F;
    const uint64_t MP = max_pairs, ns = strands == 3 ? 2 : 1;
    // (what the calls refuse has no figure)
    if (!set || strands < 1 || strands > 3 || n_seqs == 0 || !set->prefilter || !packed_only(set) || screen_bits(set, n_seqs) > kPrefilterMaxBits) return F;
    if (n_seqs * ns >= (1ull << 28) || total >= (1ull << 31) || ns * total >= (1ull << 32) - 16) return F;
    if (kind != kCandidatesOnly && (MP == 0 || MP > kCandMaxPairs || max_bases > kCandMaxBases)) return F;
    if (kind == kCall && (capacity == 0 || capacity > kCallMaxSites)) return F; // (call: capacity is max_sites)
    F.n_refs = (uint32_t)set->descs.size();
    for (const kbo::RefsetDesc &d : set->descs) F.n_q += !d.status;
    F.n_bits = screen_bits(set, n_seqs);
    F.words = (uint32_t)((F.n_bits + 31) / 32);
    F.chunk = kbo::refplan::chunk_of(set->k);
    F.rev = up16((size_t)total);
    size_t w = 0;
    if (strands == 3) { // '+' copied to q, '-' made at q + rev: one buffer for the screen and the walk
        F.q = w;
        w += 2 * F.rev + 64;
    }
    F.thr = w;    w += up16((size_t)F.n_refs * 5);                                                 // the thresholds, then the m bytes
    F.pc = w;     w += up16(kbo::chunk_items_scratch_words(F.words) * sizeof(uint32_t));
    F.hdr = w;    w += 32;
    if (kind != kCandidatesOnly) {
        F.item_slots = kbo::refcand::item_slots(MP, max_bases, F.chunk);
        F.task_slots = kbo::refcand::task_slots(F.item_slots, F.n_q, MP);
        F.bits = w;   w += up16((size_t)F.words * sizeof(uint32_t));
        F.list = w;   w += up16((size_t)MP * sizeof(uint32_t));
        F.bsum = w;   w += up16((size_t)((MP + 1) / kbo::refcand::kScan64Block + 2) * sizeof(uint64_t));
        F.nch = w;    w += up16(kbo::chunk_items_scratch_words((uint32_t)MP) * sizeof(uint32_t));
        F.rfirst = w; w += up16((size_t)(F.n_refs + 1) * sizeof(uint32_t));
        F.ntask = w;  w += up16(kbo::chunk_items_scratch_words(F.n_refs) * sizeof(uint32_t));
        F.t = tail_layout(w, set->k, MP, max_bases, F.item_slots, F.task_slots, capacity, kind);
        const size_t summary_end = kind == kCall ? tail_layout(w, set->k, MP, max_bases, F.item_slots, F.task_slots, 0, kSummary).end + 16 : 0;
        w = F.t.end;
        if (kind == kSummary) {
            F.total = w;
            w += 16;
        }
        if (kind == kCall) w = std::max((F.cs = call_stage_layout(w, set->k, total, capacity)).end, summary_end); // (never below the summary's)
    }
    if (strands == 2) { // '-' alone: the screen kernel reads it at q + rev, so it lies at least rev bytes into d_work and q inside it
        F.q = std::max(w, F.rev);
        w = F.q + F.rev + 64;
    }
    F.end = w;
    F.ok = true;
    return F;
}

void run_cand_form(const DevCall &c, Kind kind)
{
    namespace sc = kbo::refscreen;
    const bool find = kind == kFind, best = kind == kBest, only = kind == kCandidatesOnly, call = kind == kCall;
    const std::vector<uint32_t> thr = check_dev_call(c, kind, true);
    kbo_refset *set = c.set;
    const CandForm F = cand_form(set, c.n_seqs, c.total_bases, c.strands, layout_capacity(c, kind), c.max_pairs, c.max_bases, kind);
    KBO_REQUIRE(F.ok, KBO_E_UNSUPPORTED, "a batch of 2^31 bases or more, or 2^28 (sequence, strand) pairs or more");
    KBO_REQUIRE(c.work_bytes >= F.end, KBO_E_BAD_ARG, "work_bytes below the figure of *_work_bytes");
    DevSet *ds = require_device_set(set);

    // the call's one upload: the thresholds and, behind them, the seed lengths as the kernels take them
    const std::vector<uint8_t> m = seed_lens(set, thr);
    std::vector<uint32_t> up(((size_t)F.n_refs * 5 + 3) / 4, 0u);
    std::copy(thr.begin(), thr.end(), up.begin());
    uint8_t *up_m = reinterpret_cast<uint8_t *>(up.data() + F.n_refs);
    uint32_t min_thr = set->k, safe_ref = 0;
    bool any = false;
    for (size_t r = 0; r < F.n_refs; r++) {
        up_m[r] = m[r] >= sc::kSeedMin ? m[r] : (uint8_t)(m[r] ? kbo::refcand::kMarkAll : sc::kUnfilterable);
        if (set->descs[r].status) continue;
        if (!any) safe_ref = (uint32_t)r;
        any = true;
        min_thr = std::min(min_thr, thr[r]);
    }
    hipStream_t st = c.stream;
    uint8_t *w = static_cast<uint8_t *>(c.d_work);
    auto at = [&](size_t o) { return reinterpret_cast<uint32_t *>(w + o); };
    HIP_OK(hipMemcpyAsync(w + F.thr, up.data(), (size_t)F.n_refs * 5, hipMemcpyHostToDevice, st));
    // (the walk reads '-' alone at its first byte, the screen at q + rev)
    const uint8_t *walk_q = prepare_strands(c, w + F.q);
    uint32_t *bits = only ? c.d_bits : at(F.bits);
    HIP_OK(hipMemsetAsync(bits, 0, (size_t)F.words * sizeof(uint32_t), st));
    HIP_OK(hipMemsetAsync(c.d_stats, 0, sizeof(kbo_refset_screen_stats), st));
    if (call) HIP_OK(hipMemsetAsync(c.d_calls, 0, sizeof(kbo_ref_calls_stats), st));
    kbo::RefsetScreenArgs s = screen_args(ds, c.n_seqs, c.total_bases, c.strands);
    s.m = w + F.thr + (size_t)F.n_refs * 4;
    s.q = c.strands == 2 ? w + F.q - F.rev : walk_q;
    s.off = c.d_offsets;
    s.bits = bits;
    HIP_OK(kbo::launch_refset_screen(s, st));
    kbo::RefsetCandArgs a{};
    a.off = c.d_offsets;
    a.thr = at(F.thr);
    a.m = s.m;
    a.bits = bits;
    a.pc = at(F.pc);
    a.hdr = reinterpret_cast<uint64_t *>(w + F.hdr);
    a.stats = reinterpret_cast<uint64_t *>(c.d_stats);
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
    const Tail &t = F.t;
    a.list = at(F.list);
    a.poff = reinterpret_cast<uint64_t *>(w + t.poff);
    a.bsum = reinterpret_cast<uint64_t *>(w + F.bsum);
    a.pthr = at(t.pthr);
    a.nch = at(F.nch);
    a.rfirst = at(F.rfirst);
    a.ntask = at(F.ntask);
    a.max_bases = c.max_bases;
    a.rev_off = c.strands == 3 ? F.rev : 0;
    a.max_pairs = (uint32_t)c.max_pairs;
    a.item_slots = (uint32_t)F.item_slots;
    a.task_slots = (uint32_t)F.task_slots;
    a.safe_ref = safe_ref;
    uint4 *items = reinterpret_cast<uint4 *>(w + t.items), *tasks = reinterpret_cast<uint4 *>(w + t.tasks);
    HIP_OK(kbo::launch_refset_cand_list(a, st));
    HIP_OK(kbo::launch_refset_cand_plan(a, find ? w + t.chars : nullptr, items, tasks, st));
    // (which references the slab will hold is known on the device alone: the kinds of all that can be queried)
    launch_walks(ds, tasks, items, a.task_slots, set->k, walk_q, w + t.ms, walk_kinds(set, 0, F.n_refs), st);
    uint32_t *out = static_cast<uint32_t *>(c.d_out);
    const TailRun run{w, t, a.max_pairs, c.max_bases, set->k, min_thr, c.gap, at(F.total), st};
    CallRun R{};
    if (call) R = call_run(c, w, t, F.cs, a.max_pairs, walk_q, min_thr);
    enqueue_tail(kind, run, [&] {
        if (find) {
            HIP_OK(kbo::launch_refset_cand_tag_runs(a, at(t.first), at(t.local), (uint32_t)t.local_cap, c.d_n, c.capacity, out, st));
        } else if (call) {
            HIP_OK(kbo::launch_refset_site_pairs_cand(a, R.pairs, st));
            enqueue_call_slab(ds, R, w, t, F.cs, a.max_pairs, c.max_bases, min_thr, st);
            if (c.total_bases) HIP_OK(kbo::launch_refset_resolve(R.r, st));
        } else if (best) { // (the table is initialised here, behind the extents; the unscreened form does it once per call, up front)
            HIP_OK(kbo::launch_refset_best_init(out, (uint32_t)c.n_seqs, st));
            HIP_OK(kbo::launch_refset_cand_best(a, at(t.chars), out, st));
        } else {
            HIP_OK(kbo::launch_refset_cand_tag_summaries(a, at(t.local), at(F.total), c.d_n, c.capacity, out, st));
        }
    });
}

// an entry point's call in either form; find takes its error probability and gap from the options
int run_call(DevCall c, Kind kind, bool screened, const kbo_find_opts *opts = nullptr, const kbo_call_opts *copts = nullptr)
{
    return guarded([&] {
        if (kind == kFind) {
            kbo_find_opts o;
            if (opts) o = *opts; else kbo_find_opts_default(&o);
            c.max_error_prob = o.max_error_prob;
            c.gap = (uint32_t)std::min<size_t>(o.max_gap_len, 0xFFFFFFFFu);
        }
        if (kind == kCall) {
            kbo_call_opts o;
            if (copts) o = *copts; else kbo_call_opts_default(&o);
            c.max_error_prob = o.max_error_prob;
            c.opts_k = o.sbwt_build_opts.k;
            c.add_revcomp = o.sbwt_build_opts.add_revcomp ? 1u : 0u;
        }
        if (screened) run_cand_form(c, kind);
        else run_dev_form(c, kind);
    });
}
static_assert(sizeof(kbo_refset_screen_stats) == 32, "kbo_refset_screen_stats is 32 bytes");
static_assert(sizeof(kbo_ref_calls_stats) == 64 && sizeof(kbo_ref_variant) == 24, "kbo_ref_calls_stats is 64 bytes, kbo_ref_variant six words");

DevCall call_args(kbo_refset *set, const uint8_t *d_concat, const uint64_t *d_offsets, size_t n_seqs, uint64_t total_bases, int strands, void *d_work,
                  size_t work_bytes, kbo_ref_variant *d_variants, size_t max_variants, uint8_t *d_chars, size_t max_chars, size_t max_sites,
                  kbo_ref_calls_stats *d_stats, void *stream)
{
    DevCall c{set, d_concat, d_offsets, n_seqs, total_bases, /* from opts: */ 0, 0u, strands, d_work, work_bytes, d_variants, max_variants, nullptr,
              static_cast<hipStream_t>(stream)};
    c.max_sites = max_sites;
    c.max_chars = max_chars;
    c.d_chars = d_chars;
    c.d_calls = d_stats;
    return c;
}

} // namespace

extern "C" {

size_t kbo_find_refset_dev_work_bytes(const kbo_refset_t *set, size_t n_seqs, uint64_t total_bases, int strands, size_t capacity,
                                      size_t refs_per_slab)
{
    return dev_form(set, n_seqs, total_bases, strands, capacity, refs_per_slab, kFind).end;
}

size_t kbo_summary_refset_dev_work_bytes(const kbo_refset_t *set, size_t n_seqs, uint64_t total_bases, int strands, size_t capacity,
                                         size_t refs_per_slab)
{
    return dev_form(set, n_seqs, total_bases, strands, capacity, refs_per_slab, kSummary).end;
}

size_t kbo_best_refset_dev_work_bytes(const kbo_refset_t *set, size_t n_seqs, uint64_t total_bases, int strands, size_t refs_per_slab)
{
    return dev_form(set, n_seqs, total_bases, strands, 0, refs_per_slab, kBest).end;
}

int kbo_find_refset_dev(kbo_refset_t *set, const uint8_t *d_concat, const uint64_t *d_offsets, size_t n_seqs, uint64_t total_bases,
                        const kbo_find_opts *opts, int strands, void *d_work, size_t work_bytes, kbo_ref_run *d_runs, size_t capacity,
                        uint64_t *d_n_runs, void *stream)
{
    return run_call(DevCall{set, d_concat, d_offsets, n_seqs, total_bases, /* from opts: */ 0, 0u, strands, d_work, work_bytes, d_runs, capacity, d_n_runs,
                            static_cast<hipStream_t>(stream)}, kFind, false, opts);
}

int kbo_summary_refset_dev(kbo_refset_t *set, const uint8_t *d_concat, const uint64_t *d_offsets, size_t n_seqs, uint64_t total_bases,
                           double max_error_prob, int strands, void *d_work, size_t work_bytes, kbo_ref_summary *d_records, size_t capacity,
                           uint64_t *d_n_records, void *stream)
{
    return run_call(DevCall{set, d_concat, d_offsets, n_seqs, total_bases, max_error_prob, 0u, strands, d_work, work_bytes, d_records, capacity,
                            d_n_records, static_cast<hipStream_t>(stream)}, kSummary, false);
}

int kbo_best_refset_dev(kbo_refset_t *set, const uint8_t *d_concat, const uint64_t *d_offsets, size_t n_seqs, uint64_t total_bases,
                        double max_error_prob, int strands, void *d_work, size_t work_bytes, kbo_ref_best *d_out, void *stream)
{
    return run_call(DevCall{set, d_concat, d_offsets, n_seqs, total_bases, max_error_prob, 0u, strands, d_work, work_bytes, d_out, 0, nullptr,
                            static_cast<hipStream_t>(stream)}, kBest, false);
}

size_t kbo_refset_candidates_dev_work_bytes(const kbo_refset_t *set, size_t n_seqs, uint64_t total_bases, int strands)
{
    return cand_form(set, n_seqs, total_bases, strands, 0, 0, 0, kCandidatesOnly).end;
}

size_t kbo_find_refset_screened_dev_work_bytes(const kbo_refset_t *set, size_t n_seqs, uint64_t total_bases, int strands, size_t capacity,
                                               size_t max_pairs, uint64_t max_pair_bases)
{
    return cand_form(set, n_seqs, total_bases, strands, capacity, max_pairs, max_pair_bases, kFind).end;
}

size_t kbo_summary_refset_screened_dev_work_bytes(const kbo_refset_t *set, size_t n_seqs, uint64_t total_bases, int strands, size_t capacity,
                                                  size_t max_pairs, uint64_t max_pair_bases)
{
    return cand_form(set, n_seqs, total_bases, strands, capacity, max_pairs, max_pair_bases, kSummary).end;
}

size_t kbo_best_refset_screened_dev_work_bytes(const kbo_refset_t *set, size_t n_seqs, uint64_t total_bases, int strands, size_t max_pairs,
                                               uint64_t max_pair_bases)
{
    return cand_form(set, n_seqs, total_bases, strands, 0, max_pairs, max_pair_bases, kBest).end;
}

int kbo_refset_candidates_dev(kbo_refset_t *set, const uint8_t *d_concat, const uint64_t *d_offsets, size_t n_seqs, uint64_t total_bases,
                              double max_error_prob, int strands, void *d_work, size_t work_bytes, uint32_t *d_bits,
                              kbo_refset_screen_stats *d_stats, void *stream)
{
    return run_call(DevCall{set, d_concat, d_offsets, n_seqs, total_bases, max_error_prob, 0u, strands, d_work, work_bytes, nullptr, 0, nullptr,
                            static_cast<hipStream_t>(stream), 0, 0, d_bits, d_stats}, kCandidatesOnly, true);
}

int kbo_find_refset_screened_dev(kbo_refset_t *set, const uint8_t *d_concat, const uint64_t *d_offsets, size_t n_seqs, uint64_t total_bases,
                                 const kbo_find_opts *opts, int strands, void *d_work, size_t work_bytes, kbo_ref_run *d_runs, size_t capacity,
                                 uint64_t *d_n_runs, size_t max_pairs, uint64_t max_pair_bases, kbo_refset_screen_stats *d_stats, void *stream)
{
    return run_call(DevCall{set, d_concat, d_offsets, n_seqs, total_bases, /* from opts: */ 0, 0u, strands, d_work, work_bytes, d_runs, capacity, d_n_runs,
                            static_cast<hipStream_t>(stream), max_pairs, max_pair_bases, nullptr, d_stats}, kFind, true, opts);
}

int kbo_summary_refset_screened_dev(kbo_refset_t *set, const uint8_t *d_concat, const uint64_t *d_offsets, size_t n_seqs, uint64_t total_bases,
                                    double max_error_prob, int strands, void *d_work, size_t work_bytes, kbo_ref_summary *d_records,
                                    size_t capacity, uint64_t *d_n_records, size_t max_pairs, uint64_t max_pair_bases,
                                    kbo_refset_screen_stats *d_stats, void *stream)
{
    return run_call(DevCall{set, d_concat, d_offsets, n_seqs, total_bases, max_error_prob, 0u, strands, d_work, work_bytes, d_records, capacity,
                            d_n_records, static_cast<hipStream_t>(stream), max_pairs, max_pair_bases, nullptr, d_stats}, kSummary, true);
}

int kbo_best_refset_screened_dev(kbo_refset_t *set, const uint8_t *d_concat, const uint64_t *d_offsets, size_t n_seqs, uint64_t total_bases,
                                 double max_error_prob, int strands, void *d_work, size_t work_bytes, kbo_ref_best *d_out, size_t max_pairs,
                                 uint64_t max_pair_bases, kbo_refset_screen_stats *d_stats, void *stream)
{
    return run_call(DevCall{set, d_concat, d_offsets, n_seqs, total_bases, max_error_prob, 0u, strands, d_work, work_bytes, d_out, 0, nullptr,
                            static_cast<hipStream_t>(stream), max_pairs, max_pair_bases, nullptr, d_stats}, kBest, true);
}

size_t kbo_call_refset_dev_work_bytes(const kbo_refset_t *set, size_t n_seqs, uint64_t total_bases, int strands, size_t max_sites,
                                      size_t refs_per_slab)
{
    return dev_form(set, n_seqs, total_bases, strands, max_sites, refs_per_slab, kCall).end;
}

int kbo_call_refset_dev(kbo_refset_t *set, const uint8_t *d_concat, const uint64_t *d_offsets, size_t n_seqs, uint64_t total_bases,
                        const kbo_call_opts *opts, int strands, void *d_work, size_t work_bytes, kbo_ref_variant *d_variants, size_t max_variants,
                        uint8_t *d_chars, size_t max_chars, size_t max_sites, kbo_ref_calls_stats *d_stats, void *stream)
{
    return run_call(call_args(set, d_concat, d_offsets, n_seqs, total_bases, strands, d_work, work_bytes, d_variants, max_variants, d_chars, max_chars,
                              max_sites, d_stats, stream), kCall, false, nullptr, opts);
}

size_t kbo_call_refset_screened_dev_work_bytes(const kbo_refset_t *set, size_t n_seqs, uint64_t total_bases, int strands, size_t max_sites,
                                               size_t max_pairs, uint64_t max_pair_bases)
{
    return cand_form(set, n_seqs, total_bases, strands, max_sites, max_pairs, max_pair_bases, kCall).end;
}

int kbo_call_refset_screened_dev(kbo_refset_t *set, const uint8_t *d_concat, const uint64_t *d_offsets, size_t n_seqs, uint64_t total_bases,
                                 const kbo_call_opts *opts, int strands, void *d_work, size_t work_bytes, kbo_ref_variant *d_variants,
                                 size_t max_variants, uint8_t *d_chars, size_t max_chars, size_t max_sites, kbo_ref_calls_stats *d_stats,
                                 size_t max_pairs, uint64_t max_pair_bases, kbo_refset_screen_stats *d_screen_stats, void *stream)
{
    DevCall c = call_args(set, d_concat, d_offsets, n_seqs, total_bases, strands, d_work, work_bytes, d_variants, max_variants, d_chars, max_chars,
                          max_sites, d_stats, stream);
    c.max_pairs = max_pairs;
    c.max_bases = max_pair_bases;
    c.d_stats = d_screen_stats;
    return run_call(c, kCall, true, nullptr, opts);
}

} // extern "C"
