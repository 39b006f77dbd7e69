// batch_route.cpp — the kernel route of a batch over one index (batch_route.hpp): the only place that launches map_long_kernel,
// map_reads_kernel's second passes and the walk over shards, for batches in HBM and for host slabs alike.
#include "batch_route.hpp"

#include <map>

namespace kbo_host {

kbo::WalkArgs walk_args(const BatchView &v, const CopyView &c, uint8_t *ms_out, const WalkAsk &w, const FusedMap *map)
{
    kbo::WalkArgs a{};
    a.ix = c.ix;
    a.q = v.q;
    a.q_bytes = v.total;
    a.items = v.items;
    a.n_items = v.n_items;
    a.d_out = ms_out;
    a.lo_out = w.lo;
    a.hi_out = w.hi;
    a.call_sites = w.call ? static_cast<uint4 *>(w.call->d_sites) : nullptr;
    a.call_counts = w.call ? w.call->d_counts : nullptr;
    a.call_cap = w.call ? w.call->cap_per_list : 0;
    a.call_thr = w.call ? w.call->threshold : 0;
    // (no item is longer than this: chunk + k - 1 warm-up bases; call mode: k warm-up + up to k borrowed bases)
    a.max_item_len = v.chunk ? v.chunk + (w.call ? 2u : 1u) * c.ix.k : v.longest;
    attach_plan(a, c.ix.pc_text && !(w.lo && w.hi) ? v.plan.get(kbo::plan_work_bytes(v.n_items, v.total)) : nullptr, c.plan);
    if (map) {
        a.chars_out = map->d_chars;
        a.map_thr = map->threshold;
        a.map_fmt = map->format ? 1u : 0u;
        a.map_want_ms = map->want_ms ? 1u : 0u;
        a.seq_off = v.reads_seq_off;
    }
    return a;
}

// the bytes of a packed batch: only when something needs them (the one kernel takes the words as they are)
static void need_bytes(BatchView &v, hipStream_t s)
{
    if (v.have_bytes) return;
    KBO_REQUIRE(v.n_words, KBO_E_UNSUPPORTED, "a packed batch whose words are not counted is not unpacked whole");
    v.have_bytes = true;
    HIP_OK(kbo::launch_unpack2(v.qp, (uint32_t)v.n_words, v.offsets, v.n_seqs, v.wps, v.pscr, v.bytes_out, s));
    HIP_OK(kbo::launch_exceptions(v.exc_pos, v.exc_byte, v.n_exc, v.exc_base, v.bytes_out, s));
}

void packed_native_args(const BatchView &v, kbo::WalkArgs &a, uint32_t *packed_out, hipStream_t s)
{
    a.qp = v.qp;
    a.qp_wps = v.wps;
    a.qp_data = v.pscr;
    a.qp_sums = v.pscr ? v.pscr + v.n_seqs + 1u : nullptr;
    a.packed_out = packed_out;
    if (!v.n_exc) return;
    uint8_t *flag = static_cast<uint8_t *>(v.exc_flag.get((size_t)v.n_seqs + 16));
    HIP_OK(hipMemsetAsync(flag, 0, v.n_seqs, s));
    HIP_OK(kbo::launch_flag_exceptions(v.exc_pos, v.n_exc, v.exc_base, v.offsets, v.n_seqs, flag, s));
    a.qp_exc = flag;
}

// the second pass on the caller's other stream, behind what `s` holds so far; returns the stream it goes to.  `a`: a batch of reads'
// second pass, whose pieces grow to 32 bases there (beside another batch's kernel the pass costs by the look-ups it takes away from
// that kernel rather than by its longest chain: longer pieces, fewer warm-up bases.  Pieces of 16 / 24 / 32 / 48 / 64 bases at C2,
// two batches in flight: 0.341 / 0.324 / 0.316 / 0.343 / 0.337 ms per batch)
hipStream_t fork_tail(hipStream_t s, hipStream_t tail, kbo::WalkArgs *a)
{
    if (tail == s) return s;
    // one fence event per host thread and device: hipStreamWaitEvent takes the event's state at the time of the call, so recording it
    // again for the next batch does not disturb a wait that is already queued
    thread_local std::map<int, hipEvent_t> fences;
    hipEvent_t &fence = fences[current_device()];
    if (!fence) HIP_OK(hipEventCreateWithFlags(&fence, hipEventDisableTiming));
    HIP_OK(hipEventRecord(fence, s));
    HIP_OK(hipStreamWaitEvent(tail, fence, 0));
    if (a) a->redo_piece = 32u;
    return tail;
}

// The reads map_reads_kernel left, on `t`.  Packed-native: their bytes first (the plain walk and finish_reads_kernel read bytes),
// their characters into words last.  Between: the reads the kernel listed finished by one kernel where that applies - walk,
// derandomize + translate, characters or records (and their runs) - else the plain walk of the flagged reads (redo_collect_kernel
// reads the offsets or the item list, as the kernel did) and, where characters are asked for, derandomize + translate of those reads
// (the flagged reads' runs counted on the way)
void second_pass(const BatchView &v, const kbo::WalkArgs &a, hipStream_t t, bool one_wave_groups)
{
    if (a.qp) {
        HIP_OK(kbo::launch_unpack_flagged(a.qp, v.offsets, v.n_seqs, a.qp_wps, a.qp_data, a.redo, v.bytes_out, t));
        HIP_OK(kbo::launch_exceptions(v.exc_pos, v.exc_byte, v.n_exc, v.exc_base, v.bytes_out, t));
    }
    kbo::WalkArgs fa = a; // (item s is sequence s, whole: finish_reads_kernel reads the offsets)
    fa.seq_off = v.offsets;
    if (a.summary_out) fa.qp = nullptr; // (the summary form is asked for only where its second pass applies: over the bytes just unpacked)
    if (kbo::map_reads_finish_applies(fa)) {
        HIP_OK(kbo::launch_map_reads_finish(fa, t, one_wave_groups));
    } else {
        HIP_OK(kbo::launch_redo_pass(a, t));
        if (a.chars_out)
            HIP_OK(kbo::launch_derand_flagged(a.d_out, v.offsets, v.n_seqs, a.ix.k, a.map_thr, a.map_fmt ? a.q : nullptr, a.chars_out, a.redo,
                                              a.max_item_len, t, a.run_counts));
    }
    if (a.packed_out) HIP_OK(kbo::launch_pack_flagged(a.chars_out, v.offsets, v.n_seqs, a.qp_wps, a.qp_data, a.redo, a.packed_out, t));
}

hipStream_t run_reads(const BatchView &v, kbo::WalkArgs &a, DevCopy::PlanState *plan, const ReadsLaunch &L)
{
    hipStream_t ts = L.s;
    if (L.then) ts = L.then(v, a, L);
    else {
        HIP_OK(kbo::launch_map_reads(a, L.s));
        second_pass(v, a, L.s, false);
    }
    if (!a.host_bailed) plan_after_launch(a, ts, plan);
    return ts;
}

void walk_shards(BatchView &v, kbo_index *idx, const CopyView *given, const WalkAsk &w, hipStream_t s, const kbo::WalkArgs *filled)
{
    const std::vector<kbo_index *> shards = shards_of(idx);
    for (size_t sh = 0; sh < shards.size(); sh++) {
        const CopyView c = given ? *given : copy_view(shards[sh], v.total);
        const kbo::WalkArgs a = filled ? *filled : walk_args(v, c, sh == 0 ? v.ms : v.ms_shard, w, nullptr);
        need_bytes(v, s);
        HIP_OK(kbo::launch_ms_walk(a, walk_max_waves(), s));
        plan_after_launch(a, s, c.plan);
        // the depth against the union of the shards is the maximum of the depths against each (capi_internal.hpp)
        if (sh > 0) HIP_OK(kbo::launch_max_bytes(v.ms, v.ms_shard, v.total, s));
    }
}

// kbo::matches / map / find over sequences of more than 160 bases - contigs, whole reference sequences, long reads: one wave per
// piece of a sequence (long_kernels.hip), the pieces whose proof fails by the plain walk + the literal recurrences behind it (on the
// tail stream when the caller gave one)
static void map_long(BatchView &v, const kbo::DevIndexView &ix, FusedMap &m, size_t work_bytes, const ReadsLaunch &L)
{
    need_bytes(v, L.s);
    kbo::LongArgs la{};
    HIP_OK(kbo::launch_map_long(ix, v.q, v.offsets, v.n_seqs, v.total, m.threshold, m.format, m.d_chars, v.long_work.get(work_bytes), L.s, la,
                                g_plan_stats.load()));
    m.ts = fork_tail(L.s, L.tail, nullptr);
    HIP_OK(kbo::launch_map_long_redo(la, v.ms, m.ts));
    m.done = true;
}

void route_map(BatchView &v, const CopyView &c, kbo::WalkArgs &a, FusedMap &m, const ReadsLaunch &L)
{
    const size_t long_bytes = long_seqs(v) && !m.want_ms && kbo::map_long_applies(c.ix, m.threshold) ? kbo::long_work_bytes(v.n_seqs, v.total, c.ix.k) : 0;
    if (long_bytes) return map_long(v, c.ix, m, long_bytes, L);
    if (!a.gitems || v.chunk) return; // (no plan structures, the copy is held off, or chunks of longer sequences: two kernels)
    // the summaries: the kernel's summary form - reads as bytes, or (packed-native, direct form) as words - and finish_reads_kernel's
    // behind it, over the bytes of the reads the kernel listed: records, no characters, no MS values
    if (m.d_summary && !m.format && !a.pstats) {
        kbo::WalkArgs sa = a;
        sa.chars_out = sa.d_out = nullptr;
        sa.summary_out = m.d_summary;
        if (v.qp && kbo::map_reads_packed_applies(sa, false)) packed_native_args(v, sa, nullptr, L.s);
        else need_bytes(v, L.s);
        kbo::WalkArgs fa = sa; // (the second pass reads bytes: those of the listed reads are unpacked for it)
        fa.qp = nullptr;
        fa.seq_off = v.offsets;
        if (kbo::map_reads_applies(sa) && kbo::map_reads_finish_applies(fa)) {
            m.ts = run_reads(v, sa, c.plan, L);
            m.done = m.summarized = true;
            return;
        }
    }
    // packed-native: the words go into the kernel as they are and (m.d_packed_out) the characters leave it as words; only the reads
    // it leaves to the plain walk get their bytes, and their characters are packed behind it.  Else the reads as bytes
    const bool native = v.qp && kbo::map_reads_packed_applies(a, m.d_packed_out != nullptr);
    if (native) packed_native_args(v, a, m.d_packed_out, L.s);
    else need_bytes(v, L.s);
    if (!native && !kbo::map_reads_applies(a)) return;
    // kbo::find with max_gap_len = 0: the kernel counts the runs of the reads it finishes (their characters are in LDS anyway), so
    // that format::run_lengths_gapped is one pass over the characters instead of two
    m.counted = m.run_counts && !m.format && !m.want_ms && !a.packed_out && kbo::map_reads_direct(a);
    if (m.counted) a.run_counts = m.run_counts;
    m.ts = run_reads(v, a, c.plan, L);
    m.packed_done = a.packed_out != nullptr;
    m.done = true;
}

} // namespace kbo_host
