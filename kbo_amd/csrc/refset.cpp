// refset.cpp — kbo_refset_t (N one-sequence indexes in one packed device layout), its builder and accessors, and the host calls
// kbo_find_refset, kbo_summary_refset and kbo_best_refset (kbo_hip.h "find against a set of references").  What the
// other units of the reference-set calls share with them is declared in refset_internal.hpp and defined here.
// The walk is refset_kernels.hip's.  A slab of (reference, sequence, strand) pairs is laid out pair by pair (refset_slab.hpp) and
// looks like an ordinary batch to what follows: derandomize_ms_vec / translate_ms_vec with a threshold per pair
// (derand_seq_kernels.hip: the pair's reference's), then the single-index pipeline's run_lengths_gapped kernels as they are.
// kbo_summary_refset shares the slabs, the upload, the '-' strand and the walk; behind the walk it runs the counting form of the
// derandomize / translate stage and keeps the pairs with a hit on the device: no characters, no run-length stage.
// kbo_best_refset shares all of that up to the extents and merges them, slab by slab, into a table of one record per sequence on the
// device (refset_best_kernels.hip): no record stage, nothing read back until the last slab is enqueued.
// A set built with a prefilter (kbo_refset_build_opts) carries a seed table (refset_screen.hpp); the host forms then mark the pairs
// that share a seed with one kernel over the uploaded batch (refset_screen_kernels.hip), read the bitmap back, and plan, upload and
// walk only the marked pairs.  kbo_refset_candidates is that screen alone, kbo_refset_candidates_host its restatement on the CPU.
// A set built with positions carries one entry per row of every packed reference (refset_locate.hpp) and one base offset per
// reference (refset_cover.hpp): build_positions here, the calls that read them in refset_runs.cpp.
#include "refset_internal.hpp"
#include "refset_best.hpp"
#include "refset_locate.hpp"
#include "refset_screen.hpp"

#include <thread>

using namespace kbo_host;

static_assert(kbo::kRefsetChunk == KBO_REFSET_CHUNK && kbo::kRefsetMaxRows == KBO_REFSET_MAX_ROWS, "kbo_hip_tuning.h states the kernel's constants");
static_assert(kbo::kRefsetWideMaxRows == KBO_REFSET_WIDE_MAX_ROWS && kbo::kRefsetRouteLds == KBO_REFSET_ROUTE_LDS &&
                  kbo::kRefsetRouteIndex == KBO_REFSET_ROUTE_INDEX && kbo::kRefsetRouteWide == KBO_REFSET_ROUTE_WIDE,
              "kbo_hip.h states the wide walk's constants");
static_assert(kbo::refscreen::kSeedMax == KBO_REFSET_SEED_MAX && kbo::refscreen::kSeedMin == KBO_REFSET_SEED_MIN &&
                  kbo::kRefsetScreenRun == KBO_REFSET_SCREEN_RUN && kbo::kRefsetScreenThreads == KBO_REFSET_SCREEN_THREADS,
              "the headers state the screen's constants");
static_assert(sizeof(kbo_refset_opts) == sizeof(size_t) + 8, "kbo_refset_opts: positions lies in what was the struct's tail padding");

namespace kbo_host {
std::atomic<size_t> g_record_capacity{1u << 16};
static std::atomic<uint64_t> g_prefilter_max_bits{kPrefilterMaxBits};
thread_local uint64_t t_pre[4] = {0, 0, 0, 0};
thread_local uint64_t t_routes[4] = {0, 0, 0, 0};
thread_local uint64_t t_wide[2] = {0, 0};
thread_local uint64_t t_best[2] = {0, 0};
thread_local uint64_t t_call[4] = {0, 0, 0, 0};

DevSet *device_set(kbo_refset *set, int device)
{
    std::lock_guard<std::mutex> g(set->mu);
    auto it = set->dev.find(device);
    if (it != set->dev.end()) return it->second.get();
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
    return (set->dev[device] = std::move(d)).get();
}

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

uint64_t check_refset_batch(const kbo_refset *set, const uint8_t *concat, const uint64_t *offsets, size_t n_seqs)
{
    check_batch(concat, offsets, n_seqs);
    check_len_threshold(offsets, n_seqs, set->k, 2);
    const uint64_t total = offsets[n_seqs];
    KBO_REQUIRE(total < (1ull << 31), KBO_E_UNSUPPORTED, "a batch of 2^31 bases or more");
    return total;
}

void upload_batch(SlabWalker &F, kbo_refset *set, const uint8_t *concat, const uint64_t *offsets, size_t n_seqs, uint64_t total, int strands,
                  hipStream_t stream)
{
    const size_t n_refs = set->descs.size();
    F.set = set;
    F.offsets = offsets;
    F.k = set->k;
    F.chunk = std::max<uint32_t>(kbo::kRefsetChunk, 4u * set->k);
    F.rev_base = up16(total);
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

void revcomp_host(const uint8_t *fwd, size_t len, std::vector<uint8_t> &out)
{
    out.resize(len);
    for (size_t i = 0; i < len; i++) {
        const uint8_t b = fwd[len - 1 - i], u = b & 0xDFu;
        out[i] = u == 'A' || u == 'T' ? b ^ ('A' ^ 'T') : (u == 'C' || u == 'G' ? b ^ ('C' ^ 'G') : b);
    }
}

std::vector<uint8_t> seed_lens(const kbo_refset *set, const std::vector<uint32_t> &thr)
{
    std::vector<uint8_t> m(set->descs.size(), 0);
    for (size_t r = 0; r < m.size(); r++)
        if (packed_ok(set->descs[r])) m[r] = (uint8_t)kbo::refscreen::seed_len(thr[r], set->k);
    return m;
}

DevSet *require_device_set(kbo_refset *set, bool any_first)
{
    if (any_first) {
        std::lock_guard<std::mutex> g(set->mu);
        KBO_REQUIRE(!set->dev.empty(), KBO_E_BAD_ARG, "the set has no copy on any device (kbo_refset_to_device)"); // (no device is asked)
    }
    const int device = current_device();
    std::lock_guard<std::mutex> g(set->mu);
    auto it = set->dev.find(device);
    KBO_REQUIRE(it != set->dev.end(), KBO_E_BAD_ARG, "the set has no copy on the current device (kbo_refset_to_device)");
    return it->second.get();
}

kbo::RefsetScreenArgs screen_args(const DevSet *ds, size_t n_seqs, uint64_t total, int strands)
{
    kbo::RefsetScreenArgs a;
    a.bucket = ds->pre_bucket.as<uint32_t>();
    a.keys = ds->pre_keys.as<uint64_t>();
    a.refs = ds->pre_refs.as<uint32_t>();
    a.total = total;
    a.rev_base = up16(total);
    a.n_seqs = (uint32_t)n_seqs;
    a.strands = (uint32_t)strands;
    a.first_strand = strands == 2 ? 2u : 1u;
    return a;
}

void launch_walks(const DevSet *ds, const uint4 *tasks, const uint4 *items, uint32_t n_tasks, uint32_t k, const uint8_t *q, uint8_t *ms,
                  const WalkKinds &kinds, hipStream_t st)
{
    kbo::RefsetWalkArgs a;
    a.descs = ds->descs.as<kbo::RefsetDesc>();
    a.arena = ds->arena.as<uint4>();
    a.tasks = tasks;
    a.items = items;
    a.n_tasks = n_tasks;
    a.k = k;
    a.q = q;
    a.ms = ms;
    if (kinds.has_lds) HIP_OK(kbo::launch_refset_walk(a, kinds.lds_units, st));
    if (kinds.has_wide) HIP_OK(kbo::launch_refset_wide_walk(a, st));
}

void SlabWalker::walk_slab(const SlabPlan &P)
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
    const uint32_t n_tasks = (uint32_t)(P.tasks.size() / 4);
    launch_walks(ds, d_tasks.as<uint4>(), d_items.as<uint4>(), n_tasks, k, d_q.as<uint8_t>(), d_ms.as<uint8_t>(), P.kinds, st);
    if (P.kinds.has_wide) t_wide[1] += n_tasks;
    for (size_t p = 0; p < np; p++)
        if (!walked[P.ref[p]]) {
            walked[P.ref[p]] = 1;
            if (set->descs[P.ref[p]].route == kbo::kRefsetRouteWide) t_wide[0]++;
            else t_routes[0]++;
        }
    t_routes[2] += np;
}

void SlabWalker::summarize(const SlabPlan &P, DevBuf &d_ext)
{
    HIP_OK(kbo::launch_derand_summary_seq(d_ms.as<uint8_t>(), d_poff.as<uint64_t>(), (uint32_t)P.pairs(), P.bytes(), k, d_pthr.as<uint32_t>(), min_thr,
                                          d_ext.as<uint32_t>(), d_derand.p, st));
}
} // namespace kbo_host

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
        d_ext.ensure(np * sizeof(kbo_aln_extent));
        d_scratch.ensure(kbo::chunk_items_scratch_words((uint32_t)np) * sizeof(uint32_t));
        d_kept.ensure(np * 7 * sizeof(uint32_t));
        d_total.ensure(16);
        walk_slab(P);
        summarize(P, d_ext);
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
        refs.clear();
        for (size_t p = 0; p < np; p++)
            if (refs.empty() || refs.back() != P.ref[p]) refs.push_back(P.ref[p]);
        d_ext.ensure(np * sizeof(kbo_aln_extent));
        d_refs.ensure(refs.size() * sizeof(uint32_t));
        stage = &pinned;
        pinned.begin(stage_bytes(P) + up16(refs.size() * sizeof(uint32_t)));
        walk_slab(P);
        upload(d_refs.p, refs.data(), refs.size() * sizeof(uint32_t));
        pinned.end(st);
        summarize(P, d_ext);
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

// ---- the seed screen (refset_screen.hpp; refset_screen_kernels.hip)
struct HostTable { // refset_screen.hpp's accessor over the set's host table
    const kbo_refset *set;
    uint32_t bucket(uint32_t b) const { return set->pre_bucket[b]; }
    uint64_t key(uint32_t x) const { return set->pre_keys[x]; }
    uint32_t ref(uint32_t x) const { return set->pre_refs[x]; }
};

// The indexed stretches of a reference: its maximal runs of bases of at least k, as build_host_index sees them.  fn(b, n, p0, rev) for
// every stretch (n bases from position p0 on) and, with add_revcomp, for its reverse complement (made in rc), whose window s covers
// [p0 - s, p0 - s + k) of the reference
template <typename Fn> void for_each_stretch(const uint8_t *q, size_t n, uint32_t k, bool add_revcomp, std::vector<uint8_t> &rc, Fn fn)
{
    for (size_t i = 0; i < n;) {
        size_t j = i;
        while (j < n && kbo::refstep::base_code(q[j]) <= 3u) j++;
        if (j - i >= k) {
            fn(q + i, j - i, i, false);
            if (add_revcomp) {
                rc.resize(j - i);
                for (size_t y = 0; y < j - i; y++) rc[y] = (uint8_t)"TGCA"[kbo::refstep::base_code(q[j - 1 - y])];
                fn(rc.data(), rc.size(), j - k, true);
            }
        }
        i = j + 1;
    }
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
            for_each_stretch(seqs[r], lens[r], k, add_revcomp, rc, add_stretch);
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
        for_each_stretch(seqs[r], lens[r], set->k, add_revcomp, rc, [&](const uint8_t *b, size_t n, size_t, bool) { add_stretch(b, n, (uint32_t)r); });
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
    kbo::RefsetScreenArgs a = screen_args(F.ds, n_seqs, total, strands);
    a.m = d_m.as<uint8_t>();
    a.q = F.d_q.as<uint8_t>();
    a.off = F.d_off.as<uint64_t>();
    a.bits = d_bits.as<uint32_t>();
    HIP_OK(kbo::launch_refset_screen(a, F.st));
    scr.n_seqs = n_seqs;
    scr.bits.assign(words, 0u);
    HIP_OK(hipMemcpyAsync(scr.bits.data(), d_bits.p, words * sizeof(uint32_t), hipMemcpyDeviceToHost, F.st));
    HIP_OK(hipStreamSynchronize(F.st));
    mark_unfilterable(m, strands, scr);
}
} // namespace

namespace kbo_host {
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
} // namespace kbo_host

namespace {
// the checks kbo_refset_candidates and its host form share, all before any work; the thresholds
std::vector<uint32_t> check_candidates(const kbo_refset_t *set, const uint8_t *concat, const uint64_t *offsets, size_t n_seqs,
                                       double max_error_prob, int strands, const uint32_t *bits_out, uint64_t *total)
{
    require_strands(strands);
    KBO_REQUIRE(set && bits_out, KBO_E_BAD_ARG, "null argument");
    KBO_REQUIRE(set->prefilter, KBO_E_BAD_ARG, "the set has no prefilter (kbo_refset_build_opts)");
    std::vector<uint32_t> thr = refset_thresholds(set, max_error_prob);
    *total = check_refset_batch(set, concat, offsets, n_seqs);
    KBO_REQUIRE(screen_bits(set, n_seqs) <= kPrefilterMaxBits, KBO_E_UNSUPPORTED, "a bitmap of more than 2^31 bits");
    return thr;
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

// The references of the single-index route, one at a time: the characters of that pipeline, counted here.  fn(r, s, strand, extent)
// for every (sequence, strand) asked for.  (kbo_find_refset takes that pipeline's records, not its characters: a loop of its own.)
template <typename Fn>
void index_route_extents(kbo_refset *set, const uint8_t *concat, const uint64_t *offsets, size_t n_seqs, double max_error_prob, int strands, Fn fn)
{
    const uint64_t total = offsets[n_seqs];
    std::vector<uint8_t> fwd, rev;
    for (size_t r = 0; r < set->descs.size(); r++) {
        if (set->descs[r].status || set->descs[r].route != kbo::kRefsetRouteIndex) continue;
        if (strands & KBO_STRAND_FWD) fwd.resize(total);
        if (strands & KBO_STRAND_REV) rev.resize(total);
        matches_batch_impl(set->own[r].get(), concat, offsets, n_seqs, max_error_prob, HostOut::chars(fwd.data(), rev.data(), false), strands);
        for (size_t s = 0; s < n_seqs; s++)
            for (uint32_t strand = 1; strand <= 2; strand++) {
                if (!(strands & strand)) continue;
                const uint8_t *c = (strand == KBO_STRAND_FWD ? fwd.data() : rev.data()) + offsets[s];
                fn((uint32_t)r, (uint32_t)s, strand, extent_of_chars(c, offsets[s + 1] - offsets[s]));
            }
        t_routes[1]++;
        t_routes[2] += n_seqs * (strands == 3 ? 2u : 1u);
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
        const int dev = resolve_device(device);
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

int kbo_refset_last_wide(uint64_t out[2]) { return read_counters(t_wide, 2, out); }

int kbo_refset_route(const kbo_refset_t *set, size_t r)
{
    if (!set || r >= set->descs.size()) return KBO_E_BAD_ARG;
    return set->descs[r].status ? KBO_REFSET_ROUTE_NONE : (int)set->descs[r].route;
}

int kbo_refset_packed_only(const kbo_refset_t *set) { return set && packed_only(set) ? 1 : 0; }

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
    const HostForm x = host_form(set, *d);
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

int kbo_refset_last_prefilter(uint64_t out[4]) { return read_counters(t_pre, 4, out); }

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

int kbo_refset_last_routes(uint64_t out[4]) { return read_counters(t_routes, 4, out); }

int kbo_find_refset(kbo_refset_t *set, const uint8_t *concat, const uint64_t *offsets, size_t n_seqs, const kbo_find_opts *opts,
                    int strands, kbo_ref_run **runs, uint64_t *n_runs)
{
    return guarded([&] {
        static_assert(sizeof(kbo_ref_run) == 40, "kbo_ref_run is 40 bytes");
        require_strands(strands);
        KBO_REQUIRE(set && runs && n_runs, KBO_E_BAD_ARG, "null argument");
        *runs = nullptr;
        *n_runs = 0;
        kbo_find_opts o;
        if (opts) o = *opts; else kbo_find_opts_default(&o);
        const std::vector<uint32_t> thr = refset_thresholds(set, o.max_error_prob);
        const uint64_t total = check_refset_batch(set, concat, offsets, n_seqs);
        reset_call_counters();

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
            matches_batch_impl(set->own[r].get(), concat, offsets, n_seqs, o.max_error_prob, HostOut::runs(&sink), strands);
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
        require_strands(strands);
        KBO_REQUIRE(set && records && n_records, KBO_E_BAD_ARG, "null argument");
        *records = nullptr;
        *n_records = 0;
        const std::vector<uint32_t> thr = refset_thresholds(set, max_error_prob);
        const uint64_t total = check_refset_batch(set, concat, offsets, n_seqs);
        reset_call_counters();

        Summarizer F;
        StreamScope stream;
        upload_batch(F, set, concat, offsets, n_seqs, total, strands, stream.s);
        Screen scr;
        run_slabs(F, thr, n_seqs, strands, screen_call(F, thr, n_seqs, total, strands, scr));

        index_route_extents(set, concat, offsets, n_seqs, max_error_prob, strands, [&](uint32_t r, uint32_t s, uint32_t strand, const kbo_aln_extent &e) {
            if (F.ref_begin[r] == ~0ull) F.ref_begin[r] = F.out.size();
            if (e.n_runs) F.out.push_back(kbo_ref_summary{r, s, strand, e});
            F.ref_end[r] = F.out.size();
        });
        uint64_t n = 0;
        MallocPtr<kbo_ref_summary> res(gather_by_ref(F, F.out, &n));
        *n_records = n;
        if (n) *records = res.release(); // (none: *records stays NULL)
    });
}

int kbo_refset_lds_only(const kbo_refset_t *set)
{
    return set && std::none_of(set->descs.begin(), set->descs.end(),
                               [](const kbo::RefsetDesc &d) { return !d.status && d.route != kbo::kRefsetRouteLds; });
}

int kbo_refset_last_best(uint64_t out[2]) { return read_counters(t_best, 2, out); }

int kbo_best_refset(kbo_refset_t *set, const uint8_t *concat, const uint64_t *offsets, size_t n_seqs, double max_error_prob, int strands,
                    kbo_ref_best **out)
{
    return guarded([&] {
        namespace rb = kbo::refbest;
        static_assert(sizeof(kbo_ref_best) == 48 && sizeof(kbo_ref_best) == sizeof(rb::Best) && rb::kWords * 4 == sizeof(kbo_ref_best),
                      "kbo_ref_best is the twelve words of refset_best.hpp");
        require_strands(strands);
        KBO_REQUIRE(set && out, KBO_E_BAD_ARG, "null argument");
        *out = nullptr;
        const std::vector<uint32_t> thr = refset_thresholds(set, max_error_prob);
        const uint64_t total = check_refset_batch(set, concat, offsets, n_seqs);
        KBO_REQUIRE(n_seqs < (1ull << 28), KBO_E_UNSUPPORTED, "2^28 sequences or more");
        reset_call_counters();
        std::fill(t_best, t_best + 2, 0);

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

        // the references of the single-index route, merged here
        index_route_extents(set, concat, offsets, n_seqs, max_error_prob, strands, [&](uint32_t r, uint32_t s, uint32_t strand, const kbo_aln_extent &e) {
            const uint32_t ext[6] = {e.n_match, e.n_mismatch, e.n_jump, e.n_runs, e.start, e.end};
            rb::Best b;
            std::memcpy(&b, &res[s], sizeof b);
            b = rb::merge(b, rb::from_pair(s, r, strand, ext));
            std::memcpy(&res[s], &b, sizeof b);
        });
        *out = res.release();
    });
}

} // extern "C"
