// device_batch.cpp — the device-resident batch entry points of include/kbo_hip.h: the d_work layout and its size queries,
// kbo_ms_batch_dev / kbo_call_walk_dev, kbo_map_batch_dev / kbo_find_batch_dev and their pipelines (kbo_map_stream_*),
// kbo_matches_packed_dev, the derandomize and run-length passes over device buffers, and the tuning state only they read.
#include "../../include/kbo_hip.h"
#include "../../include/kbo_hip_tuning.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <deque>
#include <memory>
#include <mutex>
#include <vector>

#include "batch_route.hpp"

using namespace kbo_host;

// (the entry points have C linkage by their declarations in kbo_hip.h / kbo_hip_tuning.h)

namespace {
// The d_work layout of every entry point in this file - and the only place that knows it:
//   [0, scan_off)            work items: one per sequence, or per chunk of a batch that holds (or may hold) long sequences ...
//   [scan_off, plan_off)     ... and the scan scratch of the chunked list
//   [plan_off, ms_bytes)     work of the plan-guided walk (kbo_plan_stats_dev / kbo_plan_flags_dev read it)
//   [long_off, derand_off)   batches with sequences of more than 160 bases: work of map_long_kernel (long_kernels.hip) ...
//   [derand_off, bytes)      ... and of the piece-wise derandomize + translate pass behind the walk when it does not apply
//   [shard_off, +shard_bytes) a sharded index: the MS values of one further shard, at ms_bytes.  This region overlaps the two above,
//                            and only stream order keeps them apart: the walks never touch those, and a sharded batch reaches the
//                            derandomize pass only behind launch_max_bytes on the same stream (map_batch_dev_impl's two-kernel route)
// walk_min is what the walks alone check (kbo_ms_work_bytes, + the shard region), map_min what map / find check (kbo_work_bytes, + the
// shard region: kbo_index_work_bytes)
struct DevWork {
    bool chunked;
    uint32_t chunk, n_slots;
    size_t scan_off, plan_off, ms_bytes, bytes;
    size_t long_off, long_bytes, derand_off, derand_bytes;
    size_t shard_off, shard_bytes;
    size_t walk_min, map_min;
};
DevWork dev_work(size_t n_seqs, uint64_t total_bases, size_t max_seq_len, uint32_t k, bool sharded)
{
    DevWork w;
    w.chunk = (uint32_t)walk_chunk(total_bases, n_seqs, k);
    w.chunked = max_seq_len == 0 || max_seq_len > w.chunk;
    const uint64_t slots = w.chunked ? total_bases / w.chunk + n_seqs : n_seqs;
    w.n_slots = (uint32_t)std::min<uint64_t>(slots, 0xFFFFFFFFu);
    w.scan_off = ((size_t)w.n_slots * sizeof(kbo::WalkItem) + 15) / 16 * 16;
    w.bytes = std::max<uint64_t>(1, slots) * sizeof(kbo::WalkItem);
    if (w.chunked) w.bytes += kbo::chunk_items_scratch_words((uint32_t)n_seqs) * sizeof(uint32_t) + 16;
    w.bytes = (w.bytes + 15) / 16 * 16;
    w.plan_off = w.bytes;
    w.bytes += kbo::plan_work_bytes(std::max<uint64_t>(1, slots), total_bases);
    w.bytes = (w.bytes + 63) / 64 * 64;
    w.long_off = w.derand_off = w.ms_bytes = w.bytes;
    w.long_bytes = w.derand_bytes = 0;
    if (max_seq_len == 0 || max_seq_len > 160) {
        w.long_bytes = (kbo::long_work_bytes(n_seqs, total_bases, k) + 63) / 64 * 64;
        w.derand_bytes = (kbo::derand_piece_work_bytes((uint32_t)std::min<size_t>(n_seqs, 0xFFFFFFFEu), total_bases) + 63) / 64 * 64;
        w.derand_off = w.long_off + w.long_bytes;
        w.bytes += w.long_bytes + w.derand_bytes;
    }
    w.shard_off = w.ms_bytes;
    w.shard_bytes = sharded ? ((size_t)total_bases + 15) / 16 * 16 + 16 : 0;
    w.walk_min = w.ms_bytes + w.shard_bytes;
    w.map_min = w.bytes + w.shard_bytes;
    return w;
}
} // namespace

size_t kbo_work_bytes(size_t n_seqs, uint64_t total_bases, size_t max_seq_len, uint32_t k)
{
    return dev_work(n_seqs, total_bases, max_seq_len, k, false).bytes;
}

size_t kbo_ms_work_bytes(size_t n_seqs, uint64_t total_bases, size_t max_seq_len, uint32_t k)
{
    return dev_work(n_seqs, total_bases, max_seq_len, k, false).ms_bytes;
}

size_t kbo_index_work_bytes(const kbo_index_t *idx, size_t n_seqs, uint64_t total_bases, size_t max_seq_len)
{
    if (!idx) return 0;
    return dev_work(n_seqs, total_bases, max_seq_len, idx->host.k, idx->sharded()).map_min;
}

namespace {
std::atomic<bool> g_ms_one_kernel{true}; // kbo_ms_batch_dev: batches of reads through map_reads_kernel's MS-emitting form (kbo_set_ms_one_kernel)

// the checks every batch entry point makes first, in this order: the arguments, an empty batch, what one launch covers, alignment
void require_batch(bool args, size_t n_seqs, uint64_t total_bases, std::initializer_list<const void *> at16,
                   std::initializer_list<const void *> at4, const char *alignment, bool fits = true)
{
    KBO_REQUIRE(args, KBO_E_BAD_ARG, "null argument");
    KBO_REQUIRE(n_seqs > 0 && total_bases > 0, KBO_E_EMPTY_QUERY, "empty batch");
    KBO_REQUIRE(fits && n_seqs < (1ull << 28) && total_bases < 0xFFFFFF00ull, KBO_E_UNSUPPORTED,
                "one launch covers < 2^28 sequences and < 4 GiB of query: split the batch");
    uintptr_t low = 0;
    for (const void *p : at16) low |= (uintptr_t)p & 15;
    for (const void *p : at4) low |= (uintptr_t)p & 3;
    KBO_REQUIRE(low == 0, KBO_E_BAD_ARG, alignment);
}

// a batch of bytes in HBM with its d_work as the routes see it (batch_route.hpp): one item per sequence or chunks, made by walk_ms
// for the walk alone - map_reads_kernel and its second pass read the offsets themselves
BatchView batch_view(const DevWork &w, void *d_work, const uint8_t *q, const uint64_t *d_offsets, size_t n_seqs, uint64_t total_bases,
                     uint32_t longest, uint8_t *d_ms)
{
    uint8_t *work = static_cast<uint8_t *>(d_work);
    BatchView v;
    v.q = q;
    v.offsets = v.reads_seq_off = d_offsets;
    v.n_seqs = (uint32_t)n_seqs;
    v.total = total_bases;
    v.longest = longest;
    v.items = static_cast<kbo::WalkItem *>(d_work);
    v.n_items = w.n_slots;
    v.chunk = w.chunked ? w.chunk : 0;
    v.plan.p = work + w.plan_off;
    v.ms = d_ms;
    v.ms_shard = work + w.shard_off;
    v.long_work.p = work + w.long_off;
    return v;
}

// the MS values of a batch (kbo_ms_batch_dev, kbo_call_walk_dev, and the first of map / find's two kernels) into v.ms.  `given`:
// the caller's view of an unsharded index, or null (asked for here); a sharded index has every shard walked, the maximum kept
void walk_ms(kbo_index *idx, const CopyView *given, const DevWork &w, BatchView &v, void *d_work, const WalkAsk &ask, hipStream_t s)
{
    KBO_REQUIRE(v.total / w.chunk + v.n_seqs < (1ull << 28), KBO_E_UNSUPPORTED, "more than 2^28 work items per launch");
    if (ask.call) HIP_OK(hipMemsetAsync(ask.call->d_counts, 0, kbo::kCallSegs * 64 + 64, s)); // (kbo_call_walk_dev's counters: once the call is accepted)
    CopyView own;
    if (!given && !idx->sharded()) {
        own = copy_view(idx, v.total);
        given = &own;
    }
    // a batch of reads over a copy with a depth table, nothing but the MS values asked for: map_reads_kernel in the form that puts
    // the values together in LDS (k where nothing happened, the ramps behind the mismatches, the table's values right behind them),
    // stopping there - no characters are made - and the plain walk for the reads it leaves (C2: 0.33 against 0.61 ms per
    // 1 M reads for the plan-guided walk below, which stays what larger batches' chunks, the intervals, the call mode and the
    // work counters take)
    if (!idx->sharded() && !ask.lo && !ask.call && !w.chunked && g_ms_one_kernel.load() != 0 && !g_plan_stats.load()) {
        const FusedMap values{nullptr, (uint32_t)idx->host.k /* (no value is derandomised here) */, false, true};
        kbo::WalkArgs a = walk_args(v, *given, v.ms, WalkAsk{}, &values);
        if (a.gitems && kbo::map_reads_applies(a)) {
            a.host_bailed = given->plan ? given->plan->bailed : nullptr;
            run_reads(v, a, given->plan, ReadsLaunch{s, s}); // (the reads it left: their values by one kernel, or by the plain walk)
            return;
        }
    }
    if (w.chunked)
        HIP_OK(kbo::launch_make_chunk_items(v.offsets, v.n_seqs, w.chunk, idx->host.k, w.n_slots, v.items,
                                            reinterpret_cast<uint32_t *>(static_cast<uint8_t *>(d_work) + w.scan_off), s, ask.call != nullptr));
    else
        HIP_OK(kbo::launch_make_items(v.offsets, v.n_seqs, v.items, s));
    walk_shards(v, idx, given, ask, s);
}

int ms_batch_dev_impl(kbo_index_t *idx, const uint8_t *d_concat, const uint64_t *d_offsets, size_t n_seqs,
                      uint64_t total_bases, size_t max_seq_len, uint8_t *d_ms_out, uint32_t *d_lo_out,
                      uint32_t *d_hi_out, void *d_work, size_t work_bytes, void *stream, const CallSink *call)
{
    return guarded([&] {
        require_batch(idx && d_concat && d_offsets && d_ms_out && d_work, n_seqs, total_bases, {d_concat, d_work}, {d_ms_out},
                      "d_concat/d_work must be 16-byte and d_ms_out 4-byte aligned");
#ifndef KBO_WALK_DEBUG
        KBO_REQUIRE((d_lo_out == nullptr) == (d_hi_out == nullptr), KBO_E_BAD_ARG, "lo/hi must come together");
#endif
        KBO_REQUIRE(!idx->sharded() || (!d_lo_out && !call), KBO_E_UNSUPPORTED,
                    "intervals and the call mode need the rows of one index; this handle is a sharded index");
        const DevWork w = dev_work(n_seqs, total_bases, max_seq_len, idx->host.k, idx->sharded());
        KBO_REQUIRE(work_bytes >= w.walk_min, KBO_E_BAD_ARG,
                    "d_work is smaller than kbo_ms_work_bytes() (+ one shard's MS values for a sharded index: kbo_index_work_bytes()) for this batch");
        BatchView v = batch_view(w, d_work, d_concat, d_offsets, n_seqs, total_bases, (uint32_t)std::min<size_t>(max_seq_len, 0xFFFFFFFFu), d_ms_out);
        walk_ms(idx, nullptr, w, v, d_work, WalkAsk{d_lo_out, d_hi_out, call}, static_cast<hipStream_t>(stream));
    });
}
} // namespace

int kbo_ms_batch_dev(kbo_index_t *idx, const uint8_t *d_concat, const uint64_t *d_offsets, size_t n_seqs,
                     uint64_t total_bases, size_t max_seq_len, uint8_t *d_ms_out, uint32_t *d_lo_out,
                     uint32_t *d_hi_out, void *d_work, size_t work_bytes, void *stream)
{
    return ms_batch_dev_impl(idx, d_concat, d_offsets, n_seqs, total_bases, max_seq_len, d_ms_out, d_lo_out, d_hi_out, d_work,
                             work_bytes, stream, nullptr);
}

int kbo_call_walk_dev(kbo_index_t *idx, const uint8_t *d_concat, const uint64_t *d_offsets, size_t n_seqs,
                      uint64_t total_bases, size_t max_seq_len, size_t threshold, uint8_t *d_ms_out, void *d_sites,
                      size_t capacity, uint32_t *d_count, void *d_work, size_t work_bytes, void *stream)
{
    if (!d_sites || !d_count || capacity < kbo::kCallSegs || capacity > 0x7FFFFF00ull) {
        last_error() = "kbo_call_walk_dev: bad site buffer";
        return KBO_E_BAD_ARG;
    }
    const CallSink sink{d_sites, d_count, (uint32_t)(capacity / kbo::kCallSegs), (uint32_t)threshold};
    return ms_batch_dev_impl(idx, d_concat, d_offsets, n_seqs, total_bases, max_seq_len, d_ms_out, nullptr, nullptr, d_work,
                             work_bytes, stream, &sink);
}

int kbo_plan_stats_dev(size_t n_seqs, uint64_t total_bases, size_t max_seq_len, uint32_t k, const void *d_work,
                       uint64_t out[KBO_PLAN_STATS], void *stream)
{
    return guarded([&] {
        KBO_REQUIRE(d_work && out && n_seqs > 0 && total_bases > 0, KBO_E_BAD_ARG, "null / empty argument");
        const DevWork w = dev_work(n_seqs, total_bases, max_seq_len, k, false);
        const kbo::PlanLayout L = kbo::plan_layout(w.n_slots, total_bases);
        const uint8_t *plan = static_cast<const uint8_t *>(d_work) + w.plan_off;
        hipStream_t s = static_cast<hipStream_t>(stream);
        uint32_t ctl[16], st[kbo::kPlanStatSlots * kbo::kPlanStatWords], tot[2];
        const uint32_t last = 2u * w.n_slots; // the scan's extra entry: its prefix is the number of units
        HIP_OK(hipMemcpyAsync(ctl, plan + L.qctl, sizeof ctl, hipMemcpyDeviceToHost, s));
        HIP_OK(hipMemcpyAsync(st, plan + L.pstats, sizeof st, hipMemcpyDeviceToHost, s));
        HIP_OK(hipMemcpyAsync(&tot[0], plan + L.ucount + (size_t)last * 4, 4, hipMemcpyDeviceToHost, s));
        HIP_OK(hipMemcpyAsync(&tot[1], plan + L.usums + (size_t)(last / 1024u) * 4, 4, hipMemcpyDeviceToHost, s));
        HIP_OK(hipStreamSynchronize(s));
        for (uint32_t i = 0; i < KBO_PLAN_STATS; i++) out[i] = 0;
        for (uint32_t sl = 0; sl < kbo::kPlanStatSlots; sl++) {
            for (uint32_t i = 0; i < 8; i++) out[i] += st[sl * kbo::kPlanStatWords + i];
            for (uint32_t i = 0; i < 3; i++) out[12 + i] += st[sl * kbo::kPlanStatWords + kbo::kPlanStatTabLookups + i];
            out[16] += st[sl * kbo::kPlanStatWords + kbo::kPlanStatTabAnchored];
            out[18] += st[sl * kbo::kPlanStatWords + kbo::kPlanStatSubstBits];
            out[19] += st[sl * kbo::kPlanStatWords + kbo::kPlanStatSubstClean];
            out[20] += st[sl * kbo::kPlanStatWords + kbo::kPlanStatSubstGroups];
        }
        out[15] = ctl[4];
        out[17] = ctl[5];
        out[8] = (uint64_t)tot[0] + tot[1];
        out[9] = ctl[1];
        out[10] = ctl[2];
        out[11] = ctl[3];
    });
}

int kbo_plan_flags_dev(size_t n_seqs, uint64_t total_bases, size_t max_seq_len, uint32_t k, const void *d_work, uint8_t *flags_out, void *stream)
{
    return guarded([&] {
        KBO_REQUIRE(d_work && flags_out && n_seqs > 0 && total_bases > 0, KBO_E_BAD_ARG, "null / empty argument");
        const DevWork w = dev_work(n_seqs, total_bases, max_seq_len, k, false);
        KBO_REQUIRE(!w.chunked, KBO_E_UNSUPPORTED, "one item per sequence only (reads)");
        const kbo::PlanLayout L = kbo::plan_layout(w.n_slots, total_bases);
        hipStream_t s = static_cast<hipStream_t>(stream);
        HIP_OK(hipMemcpyAsync(flags_out, static_cast<const uint8_t *>(d_work) + w.plan_off + L.redo, n_seqs, hipMemcpyDeviceToHost, s));
        HIP_OK(hipStreamSynchronize(s));
    });
}

int kbo_set_ms_one_kernel(int on)
{
    g_ms_one_kernel = on != 0;
    return KBO_OK;
}

int kbo_long_stats_dev(size_t n_seqs, uint64_t total_bases, size_t max_seq_len, uint32_t k, const void *d_work, uint64_t out[KBO_LONG_STATS],
                       void *stream)
{
    return guarded([&] {
        KBO_REQUIRE(d_work && out && n_seqs > 0 && total_bases > 0, KBO_E_BAD_ARG, "null / empty argument");
        const DevWork w = dev_work(n_seqs, total_bases, max_seq_len, k, false);
        KBO_REQUIRE(w.long_bytes != 0, KBO_E_UNSUPPORTED, "not a batch of long sequences");
        uint32_t ctl[32], st[kbo::kPlanStatSlots * kbo::kPlanStatWords];
        HIP_OK(kbo::long_read_stats(static_cast<const uint8_t *>(d_work) + w.long_off, n_seqs, total_bases, k, ctl, st, static_cast<hipStream_t>(stream)));
        for (uint32_t i = 0; i < KBO_LONG_STATS; i++) out[i] = 0;
        out[0] = ctl[0];
        out[1] = ctl[4];
        out[2] = ctl[1];
        for (uint32_t i = 0; i < 5 && 8 + i < KBO_LONG_STATS; i++) out[8 + i] = (uint64_t)ctl[16 + i] << 4; // (KBO_LONG_X & 128: shader cycles by phase)
        for (uint32_t i = 0; i < 9 && 16 + i < KBO_LONG_STATS; i++) out[16 + i] = ctl[8 + i]; // (why flagged: list cap / ext / back / on; +4: after the band pass)
        for (uint32_t sl = 0; sl < kbo::kPlanStatSlots; sl++) {
            out[3] += st[sl * kbo::kPlanStatWords + kbo::kPlanStatSeedLookups];
            out[4] += st[sl * kbo::kPlanStatWords + kbo::kPlanStatSeedExtensions];
            out[5] += st[sl * kbo::kPlanStatWords + kbo::kPlanStatTabLookups];
            out[6] += st[sl * kbo::kPlanStatWords + kbo::kPlanStatTabAnchored];
            out[13] += st[sl * kbo::kPlanStatWords + kbo::kPlanStatUnits];
            out[14] += st[sl * kbo::kPlanStatWords + kbo::kPlanStatAccepted];
        }
    });
}

size_t kbo_derand_work_bytes(size_t n_seqs, uint64_t total_bases)
{
    return kbo::derand_piece_work_bytes((uint32_t)std::min<size_t>(n_seqs, 0xFFFFFFFEu), total_bases);
}

int kbo_derand_translate_dev(const uint8_t *d_ms, const uint64_t *d_offsets, size_t n_seqs, uint64_t total_bases,
                             size_t k, size_t threshold, const uint8_t *d_ref, uint8_t *d_chars_out,
                             size_t max_seq_len, void *d_work, size_t work_bytes, void *stream)
{
    return guarded([&] {
        KBO_REQUIRE(d_ms && d_offsets && d_chars_out, KBO_E_BAD_ARG, "null argument");
        KBO_REQUIRE(n_seqs > 0 && n_seqs < 0xFFFFFFFFull, KBO_E_EMPTY_QUERY, "empty batch");
        KBO_REQUIRE(k > 0 && k <= 255, KBO_E_BAD_ARG, "k in 1..255");
        KBO_REQUIRE(threshold > 1, KBO_E_THRESHOLD_LE_1, "threshold > 1 (derandomize.rs:275)");
        KBO_REQUIRE(((uintptr_t)d_ms & 3) == 0 && ((uintptr_t)d_chars_out & 3) == 0 && ((uintptr_t)d_ref & 3) == 0 &&
                        ((uintptr_t)d_work & 15) == 0,
                    KBO_E_BAD_ARG, "device buffers must be 4-byte (d_work 16-byte) aligned");
        // (the piece-wise route reads d_ms again - look-aheads into other waves' spans, the redo launch - after characters were written)
        KBO_REQUIRE(d_chars_out != d_ms, KBO_E_BAD_ARG, "not in place");
        HIP_OK(kbo::launch_derand_translate(d_ms, d_offsets, (uint32_t)n_seqs, (uint32_t)k, (uint32_t)threshold,
                                            d_ref, d_chars_out, nullptr,
                                            (uint32_t)std::min<size_t>(max_seq_len, 0xFFFFFFFFu), 0xFFFFFFFFu,
                                            static_cast<hipStream_t>(stream), total_bases, d_work, work_bytes));
    });
}

static_assert(kbo::kDerandSeqChunk == KBO_DERAND_SEQ_CHUNK && kbo::kDerandSeqChunk * kbo::kDerandSeqGroupChunks == KBO_DERAND_SEQ_GROUP,
              "kbo_hip_tuning.h states the kernels' constants");

size_t kbo_derand_seq_work_bytes(size_t n_seqs, uint64_t total_bases, size_t k, size_t min_threshold)
{
    return kbo::derand_seq_work_bytes((uint32_t)std::min<size_t>(n_seqs, 0xFFFFFFFEu), total_bases, (uint32_t)std::min<size_t>(k, 255),
                                      (uint32_t)std::min<size_t>(min_threshold, 255));
}

int kbo_derand_translate_seq_dev(const uint8_t *d_ms, const uint64_t *d_offsets, size_t n_seqs, uint64_t total_bases, size_t k,
                                 const uint32_t *d_thresholds, size_t min_threshold, const uint8_t *d_ref, uint8_t *d_chars_out,
                                 void *d_work, size_t work_bytes, void *stream)
{
    return guarded([&] {
        KBO_REQUIRE(d_ms && d_offsets && d_thresholds && d_chars_out && d_work, KBO_E_BAD_ARG, "null argument");
        KBO_REQUIRE(n_seqs > 0, KBO_E_EMPTY_QUERY, "empty batch");
        KBO_REQUIRE(k > 0 && k <= 255, KBO_E_BAD_ARG, "k in 1..255");
        KBO_REQUIRE(min_threshold <= k, KBO_E_BAD_ARG, "min_threshold <= k");
        KBO_REQUIRE(min_threshold > 1, KBO_E_THRESHOLD_LE_1, "threshold > 1 (derandomize.rs:275)");
        KBO_REQUIRE(total_bases + 16 <= (1ull << 32) && n_seqs < (1ull << 28), KBO_E_UNSUPPORTED, "a batch of 2^32 - 16 bases or 2^28 sequences, or more");
        KBO_REQUIRE(((uintptr_t)d_ms & 3) == 0 && ((uintptr_t)d_chars_out & 3) == 0 && ((uintptr_t)d_ref & 3) == 0 &&
                        ((uintptr_t)d_work & 15) == 0,
                    KBO_E_BAD_ARG, "device buffers must be 4-byte (d_work 16-byte) aligned");
        KBO_REQUIRE(d_chars_out != d_ms, KBO_E_BAD_ARG, "not in place");
        KBO_REQUIRE(work_bytes >= kbo_derand_seq_work_bytes(n_seqs, total_bases, k, min_threshold), KBO_E_BAD_ARG, "work_bytes too small");
        HIP_OK(kbo::launch_derand_translate_seq(d_ms, d_offsets, (uint32_t)n_seqs, total_bases, (uint32_t)k, d_thresholds, (uint32_t)min_threshold,
                                                d_ref, d_chars_out, d_work, static_cast<hipStream_t>(stream)));
    });
}

size_t kbo_derand_summary_seq_work_bytes(size_t n_seqs, uint64_t total_bases, size_t k, size_t min_threshold)
{
    return kbo_derand_seq_work_bytes(n_seqs, total_bases, k, min_threshold); // (the owner of a chunk is found in the scanned counts)
}

int kbo_derand_summary_seq_dev(const uint8_t *d_ms, const uint64_t *d_offsets, size_t n_seqs, uint64_t total_bases, size_t k,
                               const uint32_t *d_thresholds, size_t min_threshold, kbo_aln_extent *d_out, void *d_work, size_t work_bytes,
                               void *stream)
{
    return guarded([&] {
        static_assert(sizeof(kbo_aln_extent) == 24, "kbo_aln_extent is 24 bytes");
        KBO_REQUIRE(d_ms && d_offsets && d_thresholds && d_out && d_work, KBO_E_BAD_ARG, "null argument");
        KBO_REQUIRE(n_seqs > 0, KBO_E_EMPTY_QUERY, "empty batch");
        KBO_REQUIRE(k > 0 && k <= 255, KBO_E_BAD_ARG, "k in 1..255");
        KBO_REQUIRE(min_threshold <= k, KBO_E_BAD_ARG, "min_threshold <= k");
        KBO_REQUIRE(min_threshold > 1, KBO_E_THRESHOLD_LE_1, "threshold > 1 (derandomize.rs:275)");
        KBO_REQUIRE(total_bases + 16 <= (1ull << 32) && n_seqs < (1ull << 28), KBO_E_UNSUPPORTED, "a batch of 2^32 - 16 bases or 2^28 sequences, or more");
        KBO_REQUIRE(((uintptr_t)d_ms & 3) == 0 && ((uintptr_t)d_out & 3) == 0 && ((uintptr_t)d_work & 15) == 0, KBO_E_BAD_ARG,
                    "device buffers must be 4-byte (d_work 16-byte) aligned");
        KBO_REQUIRE(work_bytes >= kbo_derand_summary_seq_work_bytes(n_seqs, total_bases, k, min_threshold), KBO_E_BAD_ARG, "work_bytes too small");
        HIP_OK(kbo::launch_derand_summary_seq(d_ms, d_offsets, (uint32_t)n_seqs, total_bases, (uint32_t)k, d_thresholds, (uint32_t)min_threshold,
                                              reinterpret_cast<uint32_t *>(d_out), d_work, static_cast<hipStream_t>(stream)));
    });
}

size_t kbo_run_lengths_work_bytes(size_t n_seqs)
{
    return kbo::chunk_items_scratch_words((uint32_t)std::min<size_t>(n_seqs, 0xFFFFFFFEu)) * sizeof(uint32_t) + 16;
}

namespace {
// kbo_set_stage_timing: event triples of the one-kernel route's calls (guarded by g_timing_mu)
std::atomic<int> g_stage_timing{0};
std::mutex g_timing_mu;
struct StageEvents { hipEvent_t e0, e1, e1t, e2; };
std::vector<StageEvents> g_timing_pool, g_timing_used;
StageEvents timing_take()
{
    std::lock_guard<std::mutex> g(g_timing_mu);
    StageEvents ev{};
    if (!g_timing_pool.empty()) {
        ev = g_timing_pool.back();
        g_timing_pool.pop_back();
    } else {
        HIP_OK(hipEventCreate(&ev.e0));
        HIP_OK(hipEventCreate(&ev.e1));
        HIP_OK(hipEventCreate(&ev.e1t));
        HIP_OK(hipEventCreate(&ev.e2));
    }
    return ev;
}
} // namespace

int kbo_set_stage_timing(int on)
{
    if (on <= 1) {
        g_stage_timing = on != 0;
        return KBO_OK;
    }
    // on > 1: the events of that many calls are made here, not inside the calls that are to be timed
    return guarded([&] {
        std::vector<StageEvents> held;
        for (int i = 0; i < on; ++i)
            held.push_back(timing_take());
        std::lock_guard<std::mutex> g(g_timing_mu);
        g_timing_pool.insert(g_timing_pool.end(), held.begin(), held.end());
        g_stage_timing = 1;
    });
}

int kbo_stage_timing_read(double *kernel_ms_sum, double *redo_ms_sum, int *n_calls)
{
    return guarded([&] {
        std::lock_guard<std::mutex> g(g_timing_mu);
        double a = 0, b = 0;
        for (const StageEvents &ev : g_timing_used) {
            HIP_OK(hipEventSynchronize(ev.e2));
            float x = 0, y = 0;
            HIP_OK(hipEventElapsedTime(&x, ev.e0, ev.e1));
            HIP_OK(hipEventElapsedTime(&y, ev.e1t, ev.e2));
            a += x;
            b += y;
            g_timing_pool.push_back(ev);
        }
        if (kernel_ms_sum) *kernel_ms_sum = a;
        if (redo_ms_sum) *redo_ms_sum = b;
        if (n_calls) *n_calls = (int)g_timing_used.size();
        g_timing_used.clear();
    });
}

namespace {
// map_reads_kernel on L.s, then the second pass over the reads it leaves on the stream fork_tail gives; returns that stream
// (ReadsLaunch::then of every call of this file but the MS values alone).  kbo_set_stage_timing: the kernel and the second pass each
// between two events
hipStream_t map_reads_then(const BatchView &v, kbo::WalkArgs &a, const ReadsLaunch &L)
{
    const hipStream_t s = L.s;
    const bool timing = g_stage_timing.load() != 0;
    StageEvents ev{};
    if (timing) {
        ev = timing_take();
        HIP_OK(hipEventRecord(ev.e0, s));
    }
    HIP_OK(kbo::launch_map_reads(a, s));
    if (timing) HIP_OK(hipEventRecord(ev.e1, s));
    const hipStream_t ts = fork_tail(s, L.tail, &a);
    if (timing) HIP_OK(hipEventRecord(ev.e1t, ts)); // (when the second pass starts: behind the kernel and behind what `ts` held)
    second_pass(v, a, ts, L.one_wave_tail && ts != s);
    if (timing) {
        HIP_OK(hipEventRecord(ev.e2, ts));
        std::lock_guard<std::mutex> g(g_timing_mu);
        g_timing_used.push_back(ev);
    }
    return ts;
}

// format::run_lengths_gapped on the device into d_records (kbo::find behind the characters: kbo_find_batch_dev; kbo_run_lengths_dev)
struct FindTail {
    size_t max_gap_len;
    void *d_rle_work;
    uint32_t *d_records;
    size_t capacity;
};
// own: the characters are the kernels' own (M - X R); counted: the runs of every sequence are counted already (scan + emit are left)
void run_lengths(const FindTail &f, const uint8_t *d_chars, const uint64_t *d_offsets, uint32_t n_seqs, uint32_t longest, hipStream_t s,
                 bool own, bool counted = false)
{
    uint32_t *scratch = static_cast<uint32_t *>(f.d_rle_work);
    uint32_t *total = scratch + kbo::chunk_items_scratch_words(n_seqs); // last word of the work buffer
    const uint32_t gap = (uint32_t)std::min<size_t>(f.max_gap_len, 0xFFFFFFFFu), cap = (uint32_t)std::min<size_t>(f.capacity, 0xFFFFFFFFu);
    if (counted) HIP_OK(kbo::launch_rle_scan_counts(n_seqs, scratch, total, s));
    else HIP_OK(kbo::launch_rle_count(d_chars, d_offsets, n_seqs, gap, scratch, total, s, longest, own));
    if (cap) HIP_OK(kbo::launch_rle_emit(d_chars, d_offsets, n_seqs, gap, scratch, f.d_records, cap, s, longest, own));
}

// kbo::map / kbo::matches over a batch on the device, by one of three routes: sequences of any length by map_long_kernel, reads by
// map_reads_kernel (both *fused = 1), else two kernels - the walk, then derandomize + translate; kbo::find's run lengths behind it
int map_batch_dev_impl(kbo_index_t *idx, const uint8_t *d_concat, const uint64_t *d_offsets, size_t n_seqs, uint64_t total_bases,
                       size_t max_seq_len, double max_error_prob, int format, int want_ms, uint8_t *d_ms, uint8_t *d_chars_out,
                       void *d_work, size_t work_bytes, void *stream, void *tail_stream, int *fused, const FindTail *find = nullptr,
                       bool urgent_tail = false, uint4 *summary_of_chars = nullptr)
{
    if (fused) *fused = 0;
    return guarded([&] {
        require_batch(idx && d_concat && d_offsets && d_ms && d_chars_out && d_work, n_seqs, total_bases, {d_concat, d_work}, {d_ms, d_chars_out},
                      "d_concat/d_work must be 16-byte, d_ms/d_chars_out 4-byte aligned");
        const size_t threshold = random_match_threshold(idx->host.k, idx->host.n_kmers, 4, max_error_prob);
        KBO_REQUIRE(threshold > 1, KBO_E_THRESHOLD_LE_1, "threshold > 1 (derandomize.rs:275)");
        const DevWork w = dev_work(n_seqs, total_bases, max_seq_len, idx->host.k, idx->sharded());
        KBO_REQUIRE(work_bytes >= w.map_min, KBO_E_BAD_ARG,
                    idx->sharded() ? "d_work is smaller than kbo_index_work_bytes() for this batch over a sharded index"
                                   : "d_work is smaller than kbo_work_bytes() for this batch");
        const hipStream_t s = static_cast<hipStream_t>(stream);
        const uint32_t n = (uint32_t)n_seqs, thr = (uint32_t)threshold, longest = (uint32_t)std::min<size_t>(max_seq_len, 0xFFFFFFFFu);
        BatchView v = batch_view(w, d_work, d_concat, d_offsets, n_seqs, total_bases, longest, d_ms);
        FusedMap m{d_chars_out, thr, format != 0, want_ms != 0};
        if (find && find->max_gap_len == 0) m.run_counts = static_cast<uint32_t *>(find->d_rle_work);
        m.ts = s;
        CopyView c; // (a sharded index takes the two-kernel route: the walk asks for its shards' views)
        if (!idx->sharded()) {
            c = copy_view(idx, total_bases);
            kbo::WalkArgs a = !long_seqs(v) && !v.chunk ? walk_args(v, c, d_ms, WalkAsk{}, &m) : kbo::WalkArgs{};
            a.host_bailed = c.plan ? c.plan->bailed : nullptr; // (set by redo_collect_kernel itself: no 8-byte copy behind the launch)
            route_map(v, c, a, m, ReadsLaunch{s, static_cast<hipStream_t>(tail_stream), urgent_tail, map_reads_then});
        }
        if (!m.done) {
            walk_ms(idx, idx->sharded() ? nullptr : &c, w, v, d_work, WalkAsk{}, s);
            HIP_OK(kbo::launch_derand_translate(d_ms, d_offsets, n, idx->host.k, thr, format ? d_concat : nullptr, d_chars_out, nullptr, longest,
                                                0xFFFFFFFFu, s, total_bases, w.derand_bytes ? static_cast<uint8_t *>(d_work) + w.derand_off : nullptr, w.derand_bytes));
        }
        // the run lengths of the kernels' own characters: on the two-kernel route no run for a sequence of fewer than 3 bases, whose bytes
        // of d_chars_out it leaves unwritten (kbo_run_lengths_dev would count runs in whatever the caller's buffer held there)
        if (find) run_lengths(*find, d_chars_out, d_offsets, n, longest, m.ts, true, m.counted);
        // kbo_summary_batch_dev's batches that do not take map_reads_kernel's summary form: the records off the characters, behind them
        if (summary_of_chars) HIP_OK(kbo::launch_summary_bytes(d_chars_out, d_offsets, n, total_bases, summary_of_chars, m.ts));
        if (fused) *fused = m.done ? 1 : 0;
    });
}
} // namespace

int kbo_find_batch_dev(kbo_index_t *idx, const uint8_t *d_concat, const uint64_t *d_offsets, size_t n_seqs, uint64_t total_bases,
                       size_t max_seq_len, double max_error_prob, size_t max_gap_len, uint8_t *d_ms, uint8_t *d_chars_out, void *d_work,
                       size_t work_bytes, void *d_rle_work, uint32_t *d_records, size_t capacity, void *stream, void *tail_stream, int *fused)
{
    if (!d_rle_work || (!d_records && capacity) || ((uintptr_t)d_rle_work & 3) || ((uintptr_t)d_records & 3) || n_seqs >= (1ull << 31)) {
        last_error() = "kbo_find_batch_dev: bad run-length buffers";
        return KBO_E_BAD_ARG;
    }
    const FindTail ft{max_gap_len, d_rle_work, d_records, capacity};
    return map_batch_dev_impl(idx, d_concat, d_offsets, n_seqs, total_bases, max_seq_len, max_error_prob, 0, 0, d_ms, d_chars_out, d_work,
                              work_bytes, stream, tail_stream, fused, &ft);
}

int kbo_map_batch_dev(kbo_index_t *idx, const uint8_t *d_concat, const uint64_t *d_offsets, size_t n_seqs, uint64_t total_bases,
                      size_t max_seq_len, double max_error_prob, int format, int want_ms, uint8_t *d_ms, uint8_t *d_chars_out,
                      void *d_work, size_t work_bytes, void *stream, int *fused)
{
    return map_batch_dev_impl(idx, d_concat, d_offsets, n_seqs, total_bases, max_seq_len, max_error_prob, format, want_ms, d_ms, d_chars_out,
                              d_work, work_bytes, stream, stream, fused);
}

int kbo_map_batch_dev_tail(kbo_index_t *idx, const uint8_t *d_concat, const uint64_t *d_offsets, size_t n_seqs, uint64_t total_bases,
                           size_t max_seq_len, double max_error_prob, int format, int want_ms, uint8_t *d_ms, uint8_t *d_chars_out,
                           void *d_work, size_t work_bytes, void *stream, void *tail_stream, int *fused)
{
    return map_batch_dev_impl(idx, d_concat, d_offsets, n_seqs, total_bases, max_seq_len, max_error_prob, format, want_ms, d_ms, d_chars_out,
                              d_work, work_bytes, stream, tail_stream, fused);
}

// ---- per-sequence alignment summaries (kbo_aln_summary): kbo::matches' characters counted on the device, 16 bytes a sequence
namespace {
// Two routes.  Reads over an unsharded copy that map_reads_kernel takes: the kernel's summary form and finish_reads_kernel's - no
// character and no MS value is stored, d_work is the walk's alone.  Every other batch: kbo_map_batch_dev_tail's routes with the
// characters in d_work behind the map's own regions, and the reducer (summary_kernels.hip) over them.
struct SummaryWork {
    bool one_kernel;
    size_t chars_off, bytes; // (one_kernel: no characters, chars_off == bytes)
};
size_t summary_chars_bytes(uint64_t total_bases) { return ((size_t)total_bases + 16 + 63) / 64 * 64; }
SummaryWork summary_work(const kbo_index *idx, const kbo::DevIndexView *ix, const DevWork &w, size_t max_seq_len, uint64_t total_bases)
{
    SummaryWork sw{};
    const bool long_seqs = max_seq_len == 0 || max_seq_len > 160;
    sw.one_kernel = !idx->sharded() && !long_seqs && !w.chunked && ix && !g_plan_stats.load() &&
                    kbo::map_reads_summary_applies(*ix, (uint32_t)max_seq_len);
    sw.chars_off = sw.one_kernel ? w.bytes : (w.map_min + 63) / 64 * 64;
    sw.bytes = sw.one_kernel ? w.bytes : sw.chars_off + summary_chars_bytes(total_bases);
    return sw;
}

// slot_chars: a pipeline slot's buffer for the characters of the second route (made here, slot_chars_bytes, when the first batch that takes
// that route comes) - null: they go into d_work at SummaryWork::chars_off (work_bytes covers them)
int summary_batch_dev_impl(kbo_index_t *idx, const uint8_t *d_concat, const uint64_t *d_offsets, size_t n_seqs, uint64_t total_bases,
                           size_t max_seq_len, double max_error_prob, uint8_t *d_ms, kbo_aln_summary *d_summary_out, void *d_work,
                           size_t work_bytes, DevBuf *slot_chars, size_t slot_chars_bytes, void *stream, void *tail_stream, int *fused,
                           bool urgent_tail)
{
    uint8_t *d_chars = nullptr;
    if (fused) *fused = 0;
    bool generic = false;
    size_t map_bytes = 0;
    int rc = guarded([&] {
        require_batch(idx && d_concat && d_offsets && d_ms && d_summary_out && d_work, n_seqs, total_bases, {d_concat, d_work, d_summary_out}, {d_ms},
                      "d_concat/d_work/d_summary_out must be 16-byte, d_ms 4-byte aligned");
        const size_t threshold = random_match_threshold(idx->host.k, idx->host.n_kmers, 4, max_error_prob);
        KBO_REQUIRE(threshold > 1, KBO_E_THRESHOLD_LE_1, "threshold > 1 (derandomize.rs:275)");
        const DevWork w = dev_work(n_seqs, total_bases, max_seq_len, idx->host.k, idx->sharded());
        CopyView c;
        if (!idx->sharded()) c = copy_view(idx, total_bases);
        const SummaryWork sw = summary_work(idx, idx->sharded() ? nullptr : &c.ix, w, max_seq_len, total_bases);
        KBO_REQUIRE(work_bytes >= (slot_chars ? (sw.one_kernel ? w.bytes : w.map_min) : sw.bytes), KBO_E_BAD_ARG,
                    "d_work is smaller than kbo_summary_work_bytes() for this batch");
        if (!sw.one_kernel) {
            generic = true;
            map_bytes = w.map_min;
            if (slot_chars) { // (a pipeline's slot: its character buffer is made when the first batch that needs one comes, and kept)
                if (!slot_chars->p) slot_chars->alloc(slot_chars_bytes);
                d_chars = slot_chars->as<uint8_t>();
            } else {
                d_chars = static_cast<uint8_t *>(d_work) + sw.chars_off;
            }
            return;
        }
        // (planned whatever the copy's hold-off says - summary_work: the route is the copy's and the batch's alone -, and a batch that
        // leaves most of its reads to the second pass still reports it: the character batches behind it honour the hold-off)
        const BatchView v = batch_view(w, d_work, d_concat, d_offsets, n_seqs, total_bases, (uint32_t)max_seq_len, nullptr);
        const FusedMap ask{nullptr, (uint32_t)threshold, false};
        kbo::WalkArgs a = walk_args(v, CopyView{c.ix, nullptr}, nullptr, WalkAsk{}, &ask);
        a.summary_out = reinterpret_cast<uint4 *>(d_summary_out);
        KBO_REQUIRE(a.gitems && kbo::map_reads_applies(a) && kbo::map_reads_finish_applies(a), KBO_E_UNSUPPORTED, "the summary form of map_reads_kernel does not apply");
        a.host_bailed = c.plan ? c.plan->bailed : nullptr;
        run_reads(v, a, c.plan, ReadsLaunch{static_cast<hipStream_t>(stream), static_cast<hipStream_t>(tail_stream), urgent_tail, map_reads_then});
        if (fused) *fused = 1;
    });
    if (rc != KBO_OK || !generic) return rc;
    return map_batch_dev_impl(idx, d_concat, d_offsets, n_seqs, total_bases, max_seq_len, max_error_prob, 0, 0, d_ms, d_chars, d_work, map_bytes,
                              stream, tail_stream, fused, nullptr, urgent_tail, reinterpret_cast<uint4 *>(d_summary_out));
}
} // namespace

size_t kbo_summary_work_bytes(kbo_index_t *idx, size_t n_seqs, uint64_t total_bases, size_t max_seq_len)
{
    size_t bytes = 0;
    (void)guarded([&] {
        KBO_REQUIRE(idx && n_seqs > 0 && total_bases > 0, KBO_E_BAD_ARG, "null / empty argument");
        const DevWork w = dev_work(n_seqs, total_bases, max_seq_len, idx->host.k, idx->sharded());
        CopyView c;
        if (!idx->sharded()) c = copy_view(idx, 0);
        bytes = summary_work(idx, idx->sharded() ? nullptr : &c.ix, w, max_seq_len, total_bases).bytes;
    });
    return bytes;
}

int kbo_summary_batch_dev(kbo_index_t *idx, const uint8_t *d_concat, const uint64_t *d_offsets, size_t n_seqs, uint64_t total_bases,
                          size_t max_seq_len, double max_error_prob, uint8_t *d_ms, kbo_aln_summary *d_summary_out, void *d_work,
                          size_t work_bytes, void *stream, void *tail_stream, int *fused)
{
    return summary_batch_dev_impl(idx, d_concat, d_offsets, n_seqs, total_bases, max_seq_len, max_error_prob, d_ms, d_summary_out, d_work,
                                  work_bytes, nullptr, 0, stream, tail_stream, fused, false);
}

int kbo_summary_dev(const uint8_t *d_chars, const uint64_t *d_offsets, size_t n_seqs, size_t max_seq_len, kbo_aln_summary *d_summary_out,
                    void *stream)
{
    return guarded([&] {
        KBO_REQUIRE(d_chars && d_offsets && d_summary_out, KBO_E_BAD_ARG, "null argument");
        KBO_REQUIRE(n_seqs > 0 && n_seqs < (1ull << 31), KBO_E_BAD_ARG, "1 .. 2^31-1 sequences");
        KBO_REQUIRE(((uintptr_t)d_offsets & 7) == 0 && ((uintptr_t)d_summary_out & 15) == 0, KBO_E_BAD_ARG,
                    "d_offsets must be 8-byte, d_summary_out 16-byte aligned");
        const uint64_t bound = max_seq_len && max_seq_len < (1ull << 32) ? (uint64_t)n_seqs * max_seq_len : 0;
        HIP_OK(kbo::launch_summary_bytes(d_chars, d_offsets, (uint32_t)n_seqs, bound, reinterpret_cast<uint4 *>(d_summary_out),
                                         static_cast<hipStream_t>(stream)));
    });
}

size_t kbo_summary_words_work_bytes(size_t n_seqs)
{
    if (n_seqs == 0 || n_seqs >= (1ull << 31)) return 0;
    return (kbo::chunk_items_scratch_words((uint32_t)n_seqs) * sizeof(uint32_t) + 15) / 16 * 16;
}

int kbo_summary_words_dev(const uint32_t *d_words, const uint64_t *d_offsets, size_t n_seqs, size_t max_seq_len, kbo_aln_summary *d_summary_out,
                          void *d_work, void *stream)
{
    return guarded([&] {
        KBO_REQUIRE(d_words && d_offsets && d_summary_out && d_work, KBO_E_BAD_ARG, "null argument");
        KBO_REQUIRE(n_seqs > 0 && n_seqs < (1ull << 31), KBO_E_BAD_ARG, "1 .. 2^31-1 sequences");
        KBO_REQUIRE(((uintptr_t)d_words & 3) == 0 && ((uintptr_t)d_offsets & 7) == 0 && ((uintptr_t)d_summary_out & 15) == 0 &&
                        ((uintptr_t)d_work & 15) == 0,
                    KBO_E_BAD_ARG, "d_words must be 4-byte, d_offsets 8-byte, d_summary_out and d_work 16-byte aligned");
        hipStream_t s = static_cast<hipStream_t>(stream);
        uint32_t *prefix = static_cast<uint32_t *>(d_work);
        const uint64_t bound = max_seq_len && max_seq_len < (1ull << 32) ? (uint64_t)n_seqs * max_seq_len : 0;
        HIP_OK(kbo::launch_packed_prefix(d_offsets, (uint32_t)n_seqs, prefix, s));
        HIP_OK(kbo::launch_summary_words(d_words, d_offsets, (uint32_t)n_seqs, prefix, bound, reinterpret_cast<uint4 *>(d_summary_out), s));
    });
}

// ---- kbo_map_stream_*: pipelines of (kernel stream, second-pass stream), two slots each
// A (kernel stream, second-pass stream) pair in which the KERNELS' stream is kept off some compute units (32 of the device's 256 by
// default; KBO_TAIL_CUS / tail_cus = how many, 0 = two plain streams) and the second passes' stream is a plain one: a second pass is a
// chain of dependent look-ups by a few hundred waves, and beside kernels that hold every wave slot of the device each link of the chain
// waits for a slot - 0.12 ms alone, 0.37 beside two kernels, which then wait for it in turn.  With units the kernels cannot take, the
// pass's workgroups find free slots at once - and one that is WORK (5 % substitutions, long sequences, repeats) still spreads over the
// whole device.  C2, two pipelines, same box: plain / plain 757 Gbp/s; second passes CONFINED to 16 units of their own 973, but 5 %
// substitutions 245 -> 76 (adaptive forms of that: LABNOTES round 6); kernels off 32 units, second passes plain: 967 and every variant at
// or above the plain arrangement (reserved 16 / 24 / 32 / 40 / 48 units: 878 / 958 / 967 / 904 / 896 - 32 is four per XCD).
static int tail_cus_default() // compute units the kernels' streams stay off (KBO_TAIL_CUS; 0 = plain streams, the arrangement of rounds 4 - 5)
{
    static const int v = std::getenv("KBO_TAIL_CUS") ? std::atoi(std::getenv("KBO_TAIL_CUS")) : 32;
    return v;
}
// The pair of kbo_map_stream's pipelines whose batches are reads (map_reads_kernel, its list finished by finish_reads_kernel): the kernels'
// stream a plain one on all 256 units, the second passes' stream one of the device's highest priority, and the second pass launched as
// workgroups of one wave (launch_map_reads_finish).  A wave slot that a kernel's wave leaves then goes to the second pass first, and any
// free slot takes one of its waves: its few hundred waves are resident within microseconds, not behind the kernels' waves - each of which
// needed four slots on one unit at once before.  Priority alone: 918 Gbp/s, one-wave workgroups alone: 795, both: 1075 against 1035 for
// the 32 reserved units on the same box - what a build that never runs the second pass reaches
static void make_urgent_pair(hipStream_t *ks, hipStream_t *ts)
{
    int least = 0, greatest = 0;
    HIP_OK(hipDeviceGetStreamPriorityRange(&least, &greatest));
    HIP_OK(hipStreamCreateWithPriority(ts, hipStreamNonBlocking, greatest));
    HIP_OK(hipStreamCreateWithFlags(ks, hipStreamNonBlocking));
}
static void make_stream_pair(int device, int tail_cus, hipStream_t *ks, hipStream_t *ts)
{
    const int want = tail_cus >= 0 ? tail_cus : tail_cus_default();
    hipDeviceProp_t prop;
    HIP_OK(hipGetDeviceProperties(&prop, device));
    const int n_cu = prop.multiProcessorCount;
    HIP_OK(hipStreamCreateWithFlags(ts, hipStreamNonBlocking));
    if (want <= 0 || want >= n_cu) {
        HIP_OK(hipStreamCreateWithFlags(ks, hipStreamNonBlocking));
        return;
    }
    std::vector<uint32_t> mask_k((size_t)(n_cu + 31) / 32, 0u);
    for (int cu = want; cu < n_cu; cu++) mask_k[(size_t)cu / 32] |= 1u << (cu % 32);
    // (a runtime that refuses the mask - none seen - gets a plain stream: slower, never wrong)
    if (hipExtStreamCreateWithCUMask(ks, (uint32_t)mask_k.size(), mask_k.data()) != hipSuccess) {
        (void)hipGetLastError();
        *ks = nullptr;
        HIP_OK(hipStreamCreateWithFlags(ks, hipStreamNonBlocking));
    }
}

int kbo_stream_pair_create(int tail_cus, void **stream, void **tail_stream)
{
    return guarded([&] {
        KBO_REQUIRE(stream && tail_stream, KBO_E_BAD_ARG, "null argument");
        hipStream_t ks = nullptr, ts = nullptr;
        make_stream_pair(current_device(), tail_cus, &ks, &ts);
        *stream = ks;
        *tail_stream = ts;
    });
}

void kbo_stream_pair_destroy(void *stream, void *tail_stream)
{
    if (stream) (void)hipStreamDestroy(static_cast<hipStream_t>(stream));
    if (tail_stream) (void)hipStreamDestroy(static_cast<hipStream_t>(tail_stream));
}

struct kbo_map_stream {
    kbo_index_t *idx = nullptr;
    int device = 0;
    // a pipeline: the kernels' stream `ks` and the second passes' stream `ts`: make_urgent_pair (plain, highest priority) or make_stream_pair
    // (kept off 32 compute units, plain)
    struct Pipe { hipStream_t ks = nullptr, ts = nullptr; };
    bool urgent = false; // the pipelines are make_urgent_pair's (batches of reads), not make_stream_pair's
    struct Slot {
        DevBuf work, ms;
        DevBuf chars; // (summary batches that do not take the one kernel: their characters - made when the first such batch comes)
        hipEvent_t done = nullptr;
        uint64_t ticket = 0; // the batch that used it last (0: none yet)
    };
    std::vector<Pipe> pipes;
    std::deque<Slot> slots; // 2 per pipeline (a deque: the buffers do not move)
    size_t max_seqs = 0, max_seq_len = 0, work_bytes = 0;
    uint64_t max_bases = 0, next = 0;
    hipEvent_t ready = nullptr, kdone = nullptr;
    std::mutex mu;
    kbo_map_stream() = default;
    kbo_map_stream(const kbo_map_stream &) = delete;
    kbo_map_stream &operator=(const kbo_map_stream &) = delete;
    ~kbo_map_stream() // (also what a create that fails half-way leaves: whatever it had made so far)
    {
        for (auto &p : pipes) {
            if (p.ks) (void)hipStreamSynchronize(p.ks);
            if (p.ts) (void)hipStreamSynchronize(p.ts);
        }
        for (auto &sl : slots)
            if (sl.done) (void)hipEventDestroy(sl.done);
        if (ready) (void)hipEventDestroy(ready);
        if (kdone) (void)hipEventDestroy(kdone);
        for (auto &p : pipes) {
            if (p.ks) (void)hipStreamDestroy(p.ks);
            if (p.ts) (void)hipStreamDestroy(p.ts);
        }
    }
};

int kbo_map_stream_create(kbo_index_t *idx, int pipelines, size_t max_seqs, uint64_t max_bases, size_t max_seq_len, kbo_map_stream_t **out)
{
    return guarded([&] {
        KBO_REQUIRE(idx && out && max_seqs > 0 && max_bases > 0, KBO_E_BAD_ARG, "null / empty argument");
        KBO_REQUIRE(pipelines >= 1 && pipelines <= 8, KBO_E_BAD_ARG, "1 .. 8 pipelines");
        *out = nullptr;
        std::unique_ptr<kbo_map_stream> m(new kbo_map_stream());
        m->idx = idx;
        m->device = current_device();
        m->max_seqs = max_seqs;
        m->max_bases = max_bases;
        m->max_seq_len = max_seq_len;
        m->work_bytes = dev_work(max_seqs, max_bases, max_seq_len, idx->host.k, idx->sharded()).map_min;
        m->pipes.resize((size_t)pipelines);
        m->slots.resize(2 * (size_t)pipelines);
        // batches of reads (map_reads_kernel, then finish_reads_kernel) take the unmasked pair; sequences of any length, a sharded index, the
        // three-launch second pass (KBO_MAP_FINISH=0) and an explicit KBO_TAIL_CUS keep the kernels' stream off KBO_TAIL_CUS units
        const char *fin = std::getenv("KBO_MAP_FINISH");
        m->urgent = !idx->sharded() && max_seq_len > 0 && max_seq_len <= 160 && !std::getenv("KBO_TAIL_CUS") && !(fin && std::atoi(fin) == 0);
        for (auto &p : m->pipes) {
            if (m->urgent) make_urgent_pair(&p.ks, &p.ts);
            else make_stream_pair(m->device, -1, &p.ks, &p.ts);
        }
        for (auto &sl : m->slots) {
            sl.work.alloc(m->work_bytes + 64);
            sl.ms.alloc(((size_t)max_bases + 15) / 16 * 16 + 64);
            HIP_OK(hipEventCreateWithFlags(&sl.done, hipEventDisableTiming));
        }
        HIP_OK(hipEventCreateWithFlags(&m->ready, hipEventDisableTiming));
        HIP_OK(hipEventCreateWithFlags(&m->kdone, hipEventDisableTiming));
        *out = m.release();
    });
}

namespace {
// one batch into the next pipeline and slot; run(slot, kernels' stream, second passes' stream) enqueues it and returns its code
template <class Run>
int map_stream_submit_impl(kbo_map_stream_t *m, size_t n_seqs, uint64_t total_bases, size_t max_seq_len, void *ready_stream, uint64_t *ticket, Run run)
{
    if (!m) {
        last_error() = "kbo_map_stream_submit: null stream";
        return KBO_E_BAD_ARG;
    }
    std::lock_guard<std::mutex> g(m->mu);
    int rc = guarded([&] {
        KBO_REQUIRE(n_seqs <= m->max_seqs && total_bases <= m->max_bases, KBO_E_BAD_ARG, "the batch exceeds what the stream's slots were made for");
        // (the stream's queues, events and slots live on the device it was created on: a submit from a thread whose current device is another
        // one would pair that device's copy of the index with them)
        KBO_REQUIRE(current_device() == m->device, KBO_E_BAD_ARG, "kbo_map_stream_submit: the calling thread's current device is not the one the stream was created on");
        KBO_REQUIRE(dev_work(n_seqs, total_bases, max_seq_len, m->idx->host.k, m->idx->sharded()).map_min <= m->work_bytes, KBO_E_BAD_ARG,
                    "the batch needs more work memory than the stream's slots have (max_seq_len of kbo_map_stream_create)");
    });
    if (rc != KBO_OK) return rc;
    const uint64_t n = m->next;
    kbo_map_stream::Pipe &p = m->pipes[n % m->pipes.size()];
    kbo_map_stream::Slot &sl = m->slots[n % m->slots.size()];
    hipStream_t kern = p.ks, tail = p.ts;
    rc = guarded([&] {
        // the slot's buffers are free again behind its last batch; the inputs are there behind what ready_stream holds so far
        if (sl.ticket) HIP_OK(hipStreamWaitEvent(kern, sl.done, 0));
        if (ready_stream) {
            HIP_OK(hipEventRecord(m->ready, static_cast<hipStream_t>(ready_stream)));
            HIP_OK(hipStreamWaitEvent(kern, m->ready, 0));
        }
    });
    if (rc != KBO_OK) return rc;
    rc = run(sl, kern, tail);
    if (rc != KBO_OK) return rc;
    rc = guarded([&] { // complete when both streams have come this far
        HIP_OK(hipEventRecord(m->kdone, kern));
        HIP_OK(hipStreamWaitEvent(tail, m->kdone, 0));
        HIP_OK(hipEventRecord(sl.done, tail));
    });
    if (rc != KBO_OK) return rc;
    m->next = n + 1;
    sl.ticket = n + 1;
    if (ticket) *ticket = n + 1;
    return KBO_OK;
}
} // namespace

int kbo_map_stream_submit(kbo_map_stream_t *m, const uint8_t *d_concat, const uint64_t *d_offsets, size_t n_seqs, uint64_t total_bases,
                          size_t max_seq_len, double max_error_prob, int format, uint8_t *d_ms_out, uint8_t *d_chars_out, void *ready_stream,
                          uint64_t *ticket, int *fused)
{
    return map_stream_submit_impl(m, n_seqs, total_bases, max_seq_len, ready_stream, ticket, [&](kbo_map_stream::Slot &sl, hipStream_t kern, hipStream_t tail) {
        return map_batch_dev_impl(m->idx, d_concat, d_offsets, n_seqs, total_bases, max_seq_len, max_error_prob, format, d_ms_out ? 1 : 0,
                                  d_ms_out ? d_ms_out : sl.ms.as<uint8_t>(), d_chars_out, sl.work.p, m->work_bytes, kern, tail, fused, nullptr,
                                  m->urgent);
    });
}

int kbo_map_stream_submit_summary(kbo_map_stream_t *m, const uint8_t *d_concat, const uint64_t *d_offsets, size_t n_seqs, uint64_t total_bases,
                                  size_t max_seq_len, double max_error_prob, kbo_aln_summary *d_summary_out, void *ready_stream, uint64_t *ticket,
                                  int *fused)
{
    return map_stream_submit_impl(m, n_seqs, total_bases, max_seq_len, ready_stream, ticket, [&](kbo_map_stream::Slot &sl, hipStream_t kern, hipStream_t tail) {
        return summary_batch_dev_impl(m->idx, d_concat, d_offsets, n_seqs, total_bases, max_seq_len, max_error_prob, sl.ms.as<uint8_t>(), d_summary_out,
                                      sl.work.p, m->work_bytes, &sl.chars, summary_chars_bytes(m->max_bases) + 64, kern, tail, fused, m->urgent);
    });
}

namespace {
// the event that says the batch with this ticket is complete: its own while its slot still holds it, else that of the next batch of
// the same pipeline whose slot still holds it - a pipeline's batches complete in the order they were submitted (submit never blocks, so
// a slot taken again says nothing about the batch that had it before; the pipeline's latest batch is always held)
hipEvent_t map_stream_event(kbo_map_stream_t *m, uint64_t ticket)
{
    KBO_REQUIRE(m && ticket >= 1 && ticket <= m->next, KBO_E_BAD_ARG, "no such batch");
    for (uint64_t t = ticket; t <= m->next; t += m->pipes.size()) {
        kbo_map_stream::Slot &sl = m->slots[(t - 1) % m->slots.size()];
        if (sl.ticket == t) return sl.done;
    }
    return nullptr; // (not reached: the pipeline's latest batch holds its slot)
}
} // namespace

int kbo_map_stream_wait(kbo_map_stream_t *m, uint64_t ticket)
{
    return guarded([&] {
        hipEvent_t ev;
        {
            KBO_REQUIRE(m, KBO_E_BAD_ARG, "null stream");
            std::lock_guard<std::mutex> g(m->mu);
            ev = map_stream_event(m, ticket);
        }
        if (ev) HIP_OK(hipEventSynchronize(ev));
    });
}

int kbo_map_stream_wait_on(kbo_map_stream_t *m, uint64_t ticket, void *stream)
{
    return guarded([&] {
        KBO_REQUIRE(m, KBO_E_BAD_ARG, "null stream");
        std::lock_guard<std::mutex> g(m->mu);
        hipEvent_t ev = map_stream_event(m, ticket);
        if (ev) HIP_OK(hipStreamWaitEvent(static_cast<hipStream_t>(stream), ev, 0));
    });
}

int kbo_map_stream_sync(kbo_map_stream_t *m)
{
    return guarded([&] {
        KBO_REQUIRE(m, KBO_E_BAD_ARG, "null stream");
        std::lock_guard<std::mutex> g(m->mu);
        for (auto &p : m->pipes)
            for (hipStream_t s : {p.ks, p.ts})
                if (s) HIP_OK(hipStreamSynchronize(s));
    });
}

void kbo_map_stream_free(kbo_map_stream_t *m)
{
    delete m; // (waits for what its streams still hold)
}

namespace {
struct PackedScratch { size_t q, ms, chars, pscr, exc, bytes; };
PackedScratch packed_scratch(size_t n_seqs, uint64_t total_bases)
{
    auto up = [](size_t v) { return (v + 63) / 64 * 64; };
    PackedScratch L{};
    const size_t padded = up(total_bases + 32);
    L.q = 0;
    L.ms = L.q + padded;
    L.chars = L.ms + padded;
    L.pscr = L.chars + padded;
    L.exc = L.pscr + up(kbo::chunk_items_scratch_words((uint32_t)n_seqs) * sizeof(uint32_t));
    L.bytes = L.exc + up(n_seqs + 16);
    return L;
}
} // namespace

size_t kbo_matches_packed_dev_scratch_bytes(size_t n_seqs, uint64_t total_bases) { return packed_scratch(n_seqs, total_bases).bytes; }

int kbo_matches_packed_dev(kbo_index_t *idx, const uint32_t *d_words, const uint64_t *d_offsets, size_t n_seqs, uint64_t total_bases,
                           size_t max_seq_len, size_t uniform_len, const uint64_t *d_exc_pos, const uint8_t *d_exc_byte, size_t n_exc,
                           double max_error_prob, uint32_t *d_words_out, void *d_scratch, void *d_work, size_t work_bytes, void *stream,
                           void *tail_stream)
{
    return guarded([&] {
        KBO_REQUIRE(n_exc == 0 || (d_exc_pos && d_exc_byte), KBO_E_BAD_ARG, "exception list missing");
        require_batch(idx && d_words && d_offsets && d_words_out && d_scratch && d_work, n_seqs, total_bases, {d_scratch, d_work},
                      {d_words, d_words_out}, "d_scratch/d_work must be 16-byte, the words 4-byte aligned", n_exc < 0xFFFFFFFFull);
        KBO_REQUIRE(max_seq_len > 0 && max_seq_len <= 160 && !idx->sharded(), KBO_E_UNSUPPORTED,
                    "kbo_matches_packed_dev: reads of at most 160 bases over an unsharded index (else: kbo_matches_batch_packed)");
        const size_t threshold = random_match_threshold(idx->host.k, idx->host.n_kmers, 4, max_error_prob);
        KBO_REQUIRE(threshold > 1, KBO_E_THRESHOLD_LE_1, "threshold > 1 (derandomize.rs:275)");
        hipStream_t s = static_cast<hipStream_t>(stream);
        const DevWork w = dev_work(n_seqs, total_bases, max_seq_len, idx->host.k, false);
        KBO_REQUIRE(!w.chunked, KBO_E_UNSUPPORTED, "reads only");
        KBO_REQUIRE(work_bytes >= w.bytes, KBO_E_BAD_ARG, "d_work is smaller than kbo_work_bytes() for this batch");
        const PackedScratch L = packed_scratch(n_seqs, total_bases);
        uint8_t *sc = static_cast<uint8_t *>(d_scratch);
        uint32_t *pscr = uniform_len ? nullptr : reinterpret_cast<uint32_t *>(sc + L.pscr);
        // (the second pass's bytes, MS values and characters go to the scratch; none of the batch's bytes is there before it)
        BatchView v = batch_view(w, d_work, sc + L.q, d_offsets, n_seqs, total_bases, (uint32_t)max_seq_len, sc + L.ms);
        v.bytes_out = sc + L.q;
        v.have_bytes = false; // (and the number of words is not known here: this view takes run_reads alone)
        v.qp = d_words;
        v.wps = uniform_len ? (uint32_t)((uniform_len + 15) / 16) : 0u;
        v.pscr = pscr;
        v.exc_pos = d_exc_pos;
        v.exc_byte = d_exc_byte;
        v.n_exc = (uint32_t)n_exc;
        v.exc_flag.p = sc + L.exc;
        const CopyView c = copy_view(idx, total_bases);
        const FusedMap ask{sc + L.chars, (uint32_t)threshold, false};
        kbo::WalkArgs a = walk_args(v, c, v.ms, WalkAsk{}, &ask);
        KBO_REQUIRE(a.gitems && kbo::map_reads_packed_applies(a, true), KBO_E_UNSUPPORTED,
                    "this copy of the index cannot take the packed-native kernel (no depth table, a held-off copy, a threshold below the "
                    "table's order): kbo_matches_batch_packed takes any batch");
        if (pscr) HIP_OK(kbo::launch_packed_prefix(d_offsets, (uint32_t)n_seqs, pscr, s));
        packed_native_args(v, a, d_words_out, s);
        run_reads(v, a, c.plan, ReadsLaunch{s, static_cast<hipStream_t>(tail_stream), false, map_reads_then});
    });
}

int kbo_run_lengths_dev(const uint8_t *d_chars, const uint64_t *d_offsets, size_t n_seqs, size_t max_seq_len,
                        size_t max_gap_len, void *d_work, uint32_t *d_records, size_t capacity, void *stream)
{
    return guarded([&] {
        KBO_REQUIRE(d_chars && d_offsets && d_work && (d_records || capacity == 0), KBO_E_BAD_ARG, "null argument");
        KBO_REQUIRE(n_seqs > 0 && n_seqs < (1ull << 31), KBO_E_BAD_ARG, "1 .. 2^31-1 sequences");
        KBO_REQUIRE(((uintptr_t)d_work & 3) == 0 && ((uintptr_t)d_records & 3) == 0, KBO_E_BAD_ARG, "4-byte alignment");
        run_lengths(FindTail{max_gap_len, d_work, d_records, capacity}, d_chars, d_offsets, (uint32_t)n_seqs,
                    (uint32_t)std::min<size_t>(max_seq_len, 0xFFFFFFFFu), static_cast<hipStream_t>(stream), false);
    });
}

static_assert(kbo::kRleSegChunk == KBO_RLE_SEG_CHUNK && kbo::kRleSegChunk * kbo::kRleSegGroupChunks == KBO_RLE_SEG_GROUP,
              "kbo_hip_tuning.h states the kernels' constants");

size_t kbo_run_lengths_seq_work_bytes(size_t n_seqs, uint64_t total_bases)
{
    return kbo::rle_seg_work_bytes((uint32_t)std::min<size_t>(n_seqs, 0xFFFFFFFEu), total_bases);
}

int kbo_run_lengths_seq_dev(const uint8_t *d_chars, const uint64_t *d_offsets, size_t n_seqs, uint64_t total_bases, size_t max_gap_len,
                            void *d_work, size_t work_bytes, uint32_t *d_records, size_t capacity, uint32_t *d_first, void *stream)
{
    return guarded([&] {
        KBO_REQUIRE(d_chars && d_offsets && d_work && d_first && (d_records || capacity == 0), KBO_E_BAD_ARG, "null argument");
        KBO_REQUIRE(n_seqs > 0, KBO_E_EMPTY_QUERY, "empty batch");
        KBO_REQUIRE(total_bases <= (1ull << 32) - 16 && n_seqs < (1ull << 28), KBO_E_UNSUPPORTED, "a batch of 2^32 - 16 bases or 2^28 sequences, or more");
        KBO_REQUIRE(((uintptr_t)d_offsets & 7) == 0 && ((uintptr_t)d_records & 3) == 0 && ((uintptr_t)d_first & 3) == 0 &&
                        ((uintptr_t)d_work & 15) == 0,
                    KBO_E_BAD_ARG, "d_offsets 8-byte, d_records and d_first 4-byte, d_work 16-byte aligned");
        KBO_REQUIRE(work_bytes >= kbo_run_lengths_seq_work_bytes(n_seqs, total_bases), KBO_E_BAD_ARG, "work_bytes too small");
        const uint32_t gap = (uint32_t)std::min<size_t>(max_gap_len, 0xFFFFFFFFu);
        hipStream_t s = static_cast<hipStream_t>(stream);
        HIP_OK(kbo::launch_rle_seg_count(d_chars, d_offsets, (uint32_t)n_seqs, total_bases, gap, 0u, d_work, d_first, s));
        HIP_OK(kbo::launch_rle_seg_emit(d_chars, (uint32_t)n_seqs, total_bases, gap, d_work, d_records,
                                        (uint32_t)std::min<size_t>(capacity, 0xFFFFFFFFu), s));
    });
}

int kbo_run_lengths_seg_calls(uint64_t *count_calls, uint64_t *emit_calls)
{
    kbo::rle_seg_calls(count_calls, emit_calls);
    return KBO_OK;
}

// ---- the sparse form of kbo::matches over device-resident character words (sparse_kernels.hip)
namespace {
size_t sparse_prefix_bytes(size_t n_seqs) { return (kbo::chunk_items_scratch_words((uint32_t)n_seqs) * sizeof(uint32_t) + 15) / 16 * 16; }
// the words are known on the device only: the longest sequence bounds them, an unknown length takes the most workgroups
uint32_t sparse_dev_blocks(size_t n_seqs, size_t max_seq_len)
{
    return max_seq_len ? kbo::sparse_blocks((uint64_t)n_seqs * ((max_seq_len + 15) / 16)) : kbo::kSparseMaxBlocks;
}
} // namespace

uint32_t kbo_sparse_runs_blocks(size_t n_seqs, size_t max_seq_len)
{
    if (n_seqs == 0 || n_seqs >= (1ull << 31) || max_seq_len >= (1ull << 30)) return 0;
    return sparse_dev_blocks(n_seqs, max_seq_len);
}

size_t kbo_sparse_runs_work_bytes(size_t n_seqs, uint64_t total_words)
{
    if (n_seqs == 0 || n_seqs >= (1ull << 31) || total_words > 0xFFFFFF00ull) return 0;
    return sparse_prefix_bytes(n_seqs) + (kbo::kSparseScratchWords * sizeof(uint32_t) + 15) / 16 * 16;
}

int kbo_sparse_runs_dev(const uint32_t *d_words, const uint64_t *d_offsets, size_t n_seqs, size_t max_seq_len, void *d_work,
                        kbo_aln_run *d_runs, size_t capacity, uint32_t *d_n_runs, void *stream)
{
    return guarded([&] {
        KBO_REQUIRE(d_words && d_offsets && d_work && d_n_runs && (d_runs || capacity == 0), KBO_E_BAD_ARG, "null argument");
        KBO_REQUIRE(n_seqs > 0 && n_seqs < (1ull << 31), KBO_E_BAD_ARG, "1 .. 2^31-1 sequences");
        KBO_REQUIRE(max_seq_len < (1ull << 30), KBO_E_UNSUPPORTED, "sequences of 2^30 bases or more (the records' length field has 30 bits)");
        KBO_REQUIRE(((uintptr_t)d_work & 15) == 0 && ((uintptr_t)d_words & 3) == 0 && ((uintptr_t)d_offsets & 7) == 0 &&
                        ((uintptr_t)d_runs & 3) == 0 && ((uintptr_t)d_n_runs & 3) == 0,
                    KBO_E_BAD_ARG, "device buffers must be 4-byte (d_offsets 8-byte, d_work 16-byte) aligned");
        hipStream_t s = static_cast<hipStream_t>(stream);
        uint32_t *prefix = static_cast<uint32_t *>(d_work);
        uint32_t *scratch = reinterpret_cast<uint32_t *>(static_cast<uint8_t *>(d_work) + sparse_prefix_bytes(n_seqs));
        const uint32_t n_blocks = sparse_dev_blocks(n_seqs, max_seq_len);
        const uint32_t cap = (uint32_t)std::min<size_t>(capacity, 0xFFFFFFFFu);
        HIP_OK(kbo::launch_packed_prefix(d_offsets, (uint32_t)n_seqs, prefix, s));
        HIP_OK(kbo::launch_sparse_count(d_words, d_offsets, (uint32_t)n_seqs, 0u, prefix, n_blocks, scratch, s));
        HIP_OK(kbo::launch_sparse_emit(d_words, d_offsets, (uint32_t)n_seqs, 0u, prefix, n_blocks, scratch, 0u,
                                       reinterpret_cast<uint32_t *>(d_runs), cap, d_n_runs, s));
    });
}

// ---- the reverse complement of a device-resident batch (revcomp_kernels.hip)

namespace {
bool dev_ranges_overlap(const void *a, const void *b, uint64_t n)
{
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return x < y + n && y < x + n;
}
} // namespace

int kbo_revcomp_batch_dev(const uint8_t *d_concat, const uint64_t *d_offsets, size_t n_seqs, uint64_t total_bases, size_t max_seq_len,
                          uint8_t *d_out, void *stream)
{
    return guarded([&] {
        (void)max_seq_len; // (the work is cut by output bytes, not by sequence: every shape of batch fills the device alike)
        KBO_REQUIRE(d_concat && d_offsets && d_out, KBO_E_BAD_ARG, "null argument");
        KBO_REQUIRE(n_seqs > 0 && n_seqs < 0xFFFFFFFFull, KBO_E_BAD_ARG, "1 .. 2^32-2 sequences");
        KBO_REQUIRE(((uintptr_t)d_concat & 15) == 0 && ((uintptr_t)d_offsets & 7) == 0 && ((uintptr_t)d_out & 3) == 0, KBO_E_BAD_ARG,
                    "d_concat must be 16-byte, d_offsets 8-byte, d_out 4-byte aligned");
        KBO_REQUIRE(total_bases + 16 <= (1ull << 32), KBO_E_UNSUPPORTED, "4 GiB or more of bases in one launch");
        KBO_REQUIRE(!dev_ranges_overlap(d_concat, d_out, total_bases), KBO_E_BAD_ARG, "d_out overlaps d_concat");
        HIP_OK(kbo::launch_revcomp_bytes(d_concat, d_offsets, (uint32_t)n_seqs, total_bases, d_out, static_cast<hipStream_t>(stream)));
    });
}

size_t kbo_revcomp_packed_scratch_bytes(size_t n_seqs)
{
    if (n_seqs == 0 || n_seqs >= (1ull << 28)) return 0;
    return (kbo::chunk_items_scratch_words((uint32_t)n_seqs) * sizeof(uint32_t) + 15) / 16 * 16;
}

int kbo_revcomp_packed_dev(const uint32_t *d_words, const uint64_t *d_offsets, size_t n_seqs, uint64_t total_words, const uint64_t *d_exc_pos,
                           const uint8_t *d_exc_byte, size_t n_exc, uint32_t *d_words_out, uint64_t *d_exc_pos_out, uint8_t *d_exc_byte_out,
                           void *d_scratch, void *stream)
{
    return guarded([&] {
        KBO_REQUIRE(d_words && d_offsets && d_words_out && d_scratch, KBO_E_BAD_ARG, "null argument");
        KBO_REQUIRE(n_exc == 0 || (d_exc_pos && d_exc_byte && d_exc_pos_out && d_exc_byte_out), KBO_E_BAD_ARG, "null exception list");
        KBO_REQUIRE(n_seqs > 0 && n_seqs < (1ull << 28), KBO_E_BAD_ARG, "1 .. 2^28-1 sequences");
        KBO_REQUIRE(total_words < 0xFFFFFF00ull && n_exc < 0xFFFFFFFFull, KBO_E_UNSUPPORTED, "2^32 - 256 words or more in one launch");
        KBO_REQUIRE(((uintptr_t)d_words & 3) == 0 && ((uintptr_t)d_words_out & 3) == 0 && ((uintptr_t)d_offsets & 7) == 0 &&
                        ((uintptr_t)d_exc_pos & 7) == 0 && ((uintptr_t)d_exc_pos_out & 7) == 0 && ((uintptr_t)d_scratch & 15) == 0,
                    KBO_E_BAD_ARG, "device buffers must be 4-byte (offsets and positions 8-byte, d_scratch 16-byte) aligned");
        KBO_REQUIRE(!dev_ranges_overlap(d_words, d_words_out, total_words * 4), KBO_E_BAD_ARG, "d_words_out overlaps d_words");
        KBO_REQUIRE(n_exc == 0 || (!dev_ranges_overlap(d_exc_pos, d_exc_pos_out, n_exc * 8) && !dev_ranges_overlap(d_exc_byte, d_exc_byte_out, n_exc)),
                    KBO_E_BAD_ARG, "the exception list's output overlaps its input");
        hipStream_t s = static_cast<hipStream_t>(stream);
        uint32_t *prefix = static_cast<uint32_t *>(d_scratch);
        HIP_OK(kbo::launch_packed_prefix(d_offsets, (uint32_t)n_seqs, prefix, s));
        HIP_OK(kbo::launch_revcomp_packed(d_words, (uint32_t)total_words, d_offsets, (uint32_t)n_seqs, 0u, prefix, prefix + n_seqs + 1u, d_words_out, s));
        HIP_OK(kbo::launch_revcomp_exceptions(d_exc_pos, d_exc_byte, (uint32_t)n_exc, 0, d_offsets, (uint32_t)n_seqs, 0, d_exc_pos_out, d_exc_byte_out, s));
    });
}
