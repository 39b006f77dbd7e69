// refset_cand_kernels.hip — gfx950 (MI355X, CDNA4): the planner, the record stage and the merge of the SCREENED device-resident
// reference-set calls (kbo_refset_candidates_dev, kbo_find / summary / best_refset_screened_dev).  The unscreened
// forms plan from closed forms over all pairs (refset_plan_kernels.hip); here the pairs are the set bits of the screen's bitmap, so
// every place comes from a prefix sum and every owner from a bisection.  refset_cand.hpp has the arithmetic
// (tools/refset_cand_check.cpp runs it on the CPU against the host's plan over the candidate pairs).
//   rc_count_kernel      lane = bitmap word: the pairs of the references that cannot be screened set, its popcount (then a scan), the
//                        bases of its pairs summed across the wave into the statistics (one 64-bit atomic add a wave that has any)
//   rc_stats_kernel      one lane: the number of candidates (kbo_refset_candidates_dev ends here)
//   rc_list_kernel       lane = bitmap word: its set bits of rank < max_pairs to the list, their lengths next to them; the slots behind
//                        the candidates cleared
//   rc_scan64_kernel     the lengths' exclusive scan in 64 bits, two levels (launch_scan is 32-bit: 2^28 pairs of up to 2^31 bases)
//   rc_cut_kernel        one lane: the longest prefix within both caps by bisection; the four figures written
//   rc_pairs_kernel      lane = pair slot: first byte, threshold, chunk count (then a scan); '-' for a pair of fewer than 3 bases
//   rc_refs_kernel       lane = reference: its pairs in the list by bisection, its first item and its tasks (then a scan)
//   rc_items_kernel      lane = item slot, then lane = task slot: the walk's item of the pair that owns it, the task of its reference
//   rc_tag_runs_kernel / rc_tag_summaries_kernel   lane = record: { ref, seq, strand } of the pair's bit in front of it
//   rc_best_kernel       a wave (a workgroup of four below kRefsetBestSplitBelow sequences) per sequence over the references: the
//                        sequence's one or two bits, the extent at a set bit's rank when that is walked, refbest::merge
// Grids are sized by the caps; lanes behind the device-side counts return.  Stream order is the only synchronisation.  Integer work.
#include "device_util.hpp"
#include "refset_best.hpp"
#include "refset_cand.hpp"

#include <algorithm>

namespace kbo {
namespace {

using namespace refcand;

static_assert(kScan64Block == kScanBlock, "both scans cut their blocks alike");

__device__ __forceinline__ uint32_t scanned(const uint32_t *data, const uint32_t *sums, uint32_t i) { return sums[i / kScanBlock] + data[i]; }
__device__ __forceinline__ uint32_t n_candidates(const RefsetCandArgs &a) { return scanned(a.pc, a.pc + a.words + 1u, a.words); }

__global__ void rc_count_kernel(RefsetCandArgs a)
{
    const uint32_t w = blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long bases = 0ull;
    if (w < a.words) {
        const uint32_t had = a.bits[w];
        uint32_t v = had | mark_mask(w, a.n_bits, a.n_seqs, a.strands, [&](uint32_t r) { return a.m[r] == kMarkAll; });
        if (v != had) a.bits[w] = v;
        a.pc[w] = (uint32_t)__popc(v);
        while (v) {
            const uint32_t bit = w * 32u + (uint32_t)__builtin_ctz(v);
            v &= v - 1u;
            const uint32_t s = (bit >> 1) % a.n_seqs;
            bases += a.off[s + 1u] - a.off[s];
        }
    } else if (w == a.words) a.pc[w] = 0u;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) bases += __shfl_xor(bases, m); // (every lane of the wave is here: none has returned)
    if ((threadIdx.x & 63u) == 0u && bases) atomicAdd(reinterpret_cast<unsigned long long *>(a.stats) + 1, bases);
}

__global__ void rc_stats_kernel(RefsetCandArgs a)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) a.stats[0] = n_candidates(a);
}

__global__ void rc_list_kernel(RefsetCandArgs a)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < a.words) {
        uint32_t v = a.bits[i], rank = scanned(a.pc, a.pc + a.words + 1u, i);
        for (; v && rank < a.max_pairs; rank++) {
            const uint32_t bit = i * 32u + (uint32_t)__builtin_ctz(v);
            v &= v - 1u;
            const uint32_t s = (bit >> 1) % a.n_seqs;
            a.list[rank] = bit;
            a.poff[rank] = a.off[s + 1u] - a.off[s];
        }
    }
    if (i <= a.max_pairs && i >= min(n_candidates(a), a.max_pairs)) { // (the slots no set bit writes)
        a.poff[i] = 0ull;
        if (i < a.max_pairs) a.list[i] = kNoPair;
    }
}

// exclusive scan of `per` consecutive values a thread, in place; sums[block] = the block's total (device_util.hpp scan_kernel in 64 bits)
__global__ void rc_scan64_kernel(uint64_t *__restrict__ data, uint32_t n, uint32_t per, uint64_t *__restrict__ sums)
{
    __shared__ uint64_t sh[1024];
    const uint32_t t = threadIdx.x, nt = blockDim.x;
    const uint64_t base = ((uint64_t)blockIdx.x * nt + t) * per;
    uint64_t local = 0;
    for (uint32_t j = 0; j < per; j++)
        if (base + j < n) local += data[base + j];
    sh[t] = local;
    __syncthreads();
    for (uint32_t step = 1; step < nt; step <<= 1) {
        const uint64_t v = t >= step ? sh[t - step] : 0ull;
        __syncthreads();
        sh[t] += v;
        __syncthreads();
    }
    uint64_t run = sh[t] - local;
    for (uint32_t j = 0; j < per; j++)
        if (base + j < n) {
            const uint64_t v = data[base + j];
            data[base + j] = run;
            run += v;
        }
    if (sums && t == nt - 1) sums[blockIdx.x] = sh[t];
}

__device__ __forceinline__ uint64_t pre64(const RefsetCandArgs &a, uint32_t n) { return a.bsum[n / kScan64Block] + a.poff[n]; }

__global__ void rc_cut_kernel(RefsetCandArgs a)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const uint32_t cand = n_candidates(a);
    const uint32_t walked = cut(min(cand, a.max_pairs), a.max_bases, [&](uint32_t n) { return pre64(a, n); });
    const uint64_t bases = pre64(a, walked);
    a.hdr[0] = cand;
    a.hdr[1] = walked;
    a.hdr[2] = bases;
    a.hdr[3] = 0ull;
    a.stats[0] = cand;
    a.stats[2] = walked;
    a.stats[3] = bases;
}

__global__ void rc_pairs_kernel(RefsetCandArgs a, uint8_t *__restrict__ chars)
{
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p > a.max_pairs) return;
    const uint32_t walked = (uint32_t)a.hdr[1];
    const uint64_t bases = a.hdr[2], o = pre64(a, p); // (a lane reads its own slot and its block's sum, and writes its own slot)
    uint32_t nch = 0;
    if (p < walked) {
        const PairId id = pair_of_bit(a.list[p], a.n_seqs);
        const uint64_t len = a.off[id.seq + 1u] - a.off[id.seq];
        a.poff[p] = o;
        a.pthr[p] = a.thr[id.ref];
        nch = refplan::chunks_of(len, a.chunk);
        if (chars && len < 3u) // (the derandomize stage skips the pair and leaves these bytes as they are; the run-length stage reads them)
            for (uint64_t i = 0; i < len; i++) chars[o + i] = (uint8_t)'-';
    } else {
        a.poff[p] = bases; // an empty pair behind the slab: the stages behind the walk skip it
        if (p < a.max_pairs) a.pthr[p] = a.k;
    }
    a.nch[p] = nch;
}

__global__ void rc_refs_kernel(RefsetCandArgs a)
{
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r > a.n_refs) return;
    const uint32_t walked = (uint32_t)a.hdr[1];
    auto ref_of = [&](uint32_t p) { return pair_of_bit(a.list[p], a.n_seqs).ref; };
    auto ifirst = [&](uint32_t p) { return scanned(a.nch, a.nch + a.max_pairs + 1u, p); };
    const uint32_t i0 = ifirst(first_pair_of_ref(walked, r, ref_of));
    a.rfirst[r] = i0;
    a.ntask[r] = r < a.n_refs ? tasks_of(ifirst(first_pair_of_ref(walked, r + 1u, ref_of)) - i0) : 0u;
}

__global__ void rc_items_kernel(RefsetCandArgs a, uint4 *__restrict__ items, uint4 *__restrict__ tasks)
{
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g < a.item_slots) {
        const uint32_t i = (uint32_t)g, walked = (uint32_t)a.hdr[1];
        auto ifirst = [&](uint32_t p) { return scanned(a.nch, a.nch + a.max_pairs + 1u, p); };
        if (i >= ifirst(walked)) return; // (a slot behind the slab's items: no task names it)
        const uint32_t p = refplan::record_owner(walked, i, ifirst);
        const PairId id = pair_of_bit(a.list[p], a.n_seqs);
        const uint64_t b = a.off[id.seq];
        const Words4 w = make_item(a.k, a.chunk, (id.strand == 2u ? a.rev_off : 0u) + b, a.poff[p], i - ifirst(p), a.off[id.seq + 1u] - b);
        items[i] = make_uint4(w.x, w.y, w.z, w.w);
        return;
    }
    if (g - a.item_slots >= a.task_slots) return;
    const uint32_t t = (uint32_t)(g - a.item_slots);
    auto tfirst = [&](uint32_t r) { return scanned(a.ntask, a.ntask + a.n_refs + 1u, r); };
    Words4 w{a.safe_ref, 0u, 0u, 0u};
    if (t < tfirst(a.n_refs)) {
        const uint32_t r = refplan::record_owner(a.n_refs, t, tfirst);
        w = make_task(r, a.rfirst[r], a.rfirst[r + 1u] - a.rfirst[r], t - tfirst(r));
    }
    tasks[t] = make_uint4(w.x, w.y, w.z, w.w);
}

// record x, WORDS words of it at src, to { ref, seq, strand, those words } at element x of the call's list when that lies in front of
// `capacity`; the pair is the list's p-th
template <uint32_t WORDS>
__device__ __forceinline__ void rc_tag(const RefsetCandArgs &a, uint32_t p, const uint32_t *__restrict__ src, uint64_t at, uint64_t capacity,
                                       uint32_t *__restrict__ out)
{
    if (at >= capacity) return;
    const PairId id = pair_of_bit(a.list[p], a.n_seqs);
    uint32_t *o = out + at * (3u + WORDS);
    o[0] = id.ref;
    o[1] = id.seq;
    o[2] = id.strand;
#pragma unroll
    for (uint32_t i = 0; i < WORDS; i++) o[3u + i] = src[i];
}

__global__ void rc_tag_runs_kernel(RefsetCandArgs a, const uint32_t *__restrict__ first, const uint32_t *__restrict__ local, uint32_t local_cap,
                                   unsigned long long *__restrict__ count, uint64_t capacity, uint32_t *__restrict__ out)
{
    const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x, n = first[a.max_pairs];
    if (x == 0u) *count = n;
    if (x >= local_cap || x >= n) return;
    const uint32_t p = refplan::record_owner(a.max_pairs, x, [&](uint32_t q) { return first[q]; });
    rc_tag<7u>(a, p, local + (size_t)x * 7u, x, capacity, out);
}

__global__ void rc_tag_summaries_kernel(RefsetCandArgs a, const uint32_t *__restrict__ kept, const uint32_t *__restrict__ n_kept,
                                        unsigned long long *__restrict__ count, uint64_t capacity, uint32_t *__restrict__ out)
{
    const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x, n = *n_kept;
    if (x == 0u) *count = n;
    if (x >= a.max_pairs || x >= n) return;
    const uint32_t *rec = kept + (size_t)x * 7u;
    rc_tag<6u>(a, rec[0], rec + 1, x, capacity, out);
}

using namespace refbest;
constexpr uint32_t kBestThreads = 256, kBestWaves = kBestThreads / 64u;

__device__ __forceinline__ Best shfl_xor_best(const Best &b, int mask)
{
    Best o;
    o.seq = b.seq;
    o.ref = __shfl_xor(b.ref, mask);
    o.strand = __shfl_xor(b.strand, mask);
    o.n_match = __shfl_xor(b.n_match, mask);
    o.n_mismatch = __shfl_xor(b.n_mismatch, mask);
    o.n_jump = __shfl_xor(b.n_jump, mask);
    o.n_runs = __shfl_xor(b.n_runs, mask);
    o.start = __shfl_xor(b.start, mask);
    o.end = __shfl_xor(b.end, mask);
    o.n_hits = __shfl_xor(b.n_hits, mask);
    o.second_ref = __shfl_xor(b.second_ref, mask);
    o.second_match = __shfl_xor(b.second_match, mask);
    return o;
}

template <bool SPLIT> __global__ __launch_bounds__(kBestThreads) void rc_best_kernel(RefsetCandArgs a, const uint32_t *__restrict__ ext, uint32_t *__restrict__ table)
{
    __shared__ uint32_t part[SPLIT ? kBestWaves * kWords : 1u];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t s = SPLIT ? blockIdx.x : blockIdx.x * kBestWaves + wave;
    const bool live = s < a.n_seqs; // (a wave behind the last sequence visits no place and writes nothing; it still meets no barrier)
    const uint64_t places = live ? 2ull * a.n_refs : 0ull;
    const uint32_t walked = (uint32_t)a.hdr[1];
    Best mine = empty(s);
    for (uint64_t i = SPLIT ? threadIdx.x : lane; i < places; i += SPLIT ? kBestThreads : 64u) {
        const uint32_t r = (uint32_t)(i >> 1), strand = (uint32_t)(i & 1u) + 1u;
        if (!(a.strands & strand)) continue;
        const uint64_t bit = bit_of_pair(r, s, strand, a.n_seqs);
        const uint32_t wi = (uint32_t)(bit >> 5), pos = (uint32_t)(bit & 31u), word = a.bits[wi];
        if (!(word >> pos & 1u)) continue;
        const uint32_t rank = rank_of(scanned(a.pc, a.pc + a.words + 1u, wi), word, pos);
        if (rank >= walked) continue; // (a candidate behind the slab)
        const uint2 *e = reinterpret_cast<const uint2 *>(ext + (size_t)rank * 6u);
        const uint2 e0 = e[0], e1 = e[1], e2 = e[2];
        const uint32_t x[6] = {e0.x, e0.y, e1.x, e1.y, e2.x, e2.y};
        mine = merge(mine, from_pair(s, r, strand, x));
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) mine = merge(mine, shfl_xor_best(mine, m));
    if (SPLIT) {
        if (lane == 0u) {
            uint32_t *o = part + wave * kWords;
            o[0] = mine.seq; o[1] = mine.ref; o[2] = mine.strand; o[3] = mine.n_match; o[4] = mine.n_mismatch; o[5] = mine.n_jump;
            o[6] = mine.n_runs; o[7] = mine.start; o[8] = mine.end; o[9] = mine.n_hits; o[10] = mine.second_ref; o[11] = mine.second_match;
        }
        __syncthreads();
        if (threadIdx.x != 0u) return;
        for (uint32_t w = 1; w < kBestWaves; w++) {
            const uint32_t *o = part + w * kWords;
            mine = merge(mine, Best{o[0], o[1], o[2], o[3], o[4], o[5], o[6], o[7], o[8], o[9], o[10], o[11]});
        }
    } else if (lane != 0u || !live) return;
    uint32_t *t = table + (size_t)s * kWords;
    mine = merge(Best{t[0], t[1], t[2], t[3], t[4], t[5], t[6], t[7], t[8], t[9], t[10], t[11]}, mine);
    t[0] = mine.seq; t[1] = mine.ref; t[2] = mine.strand; t[3] = mine.n_match; t[4] = mine.n_mismatch; t[5] = mine.n_jump;
    t[6] = mine.n_runs; t[7] = mine.start; t[8] = mine.end; t[9] = mine.n_hits; t[10] = mine.second_ref; t[11] = mine.second_match;
}

dim3 blocks_of(uint64_t lanes) { return dim3((unsigned)((lanes + 255u) / 256u)); }

bool args_ok(const RefsetCandArgs &a)
{
    return a.n_seqs != 0 && a.n_refs != 0 && a.strands >= 1u && a.strands <= 3u && a.n_bits == (uint64_t)a.n_refs * a.n_seqs * 2u &&
           a.n_bits <= (1ull << 31) && a.words == (uint32_t)((a.n_bits + 31u) / 32u);
}
bool plan_ok(const RefsetCandArgs &a)
{
    return args_ok(a) && a.max_pairs != 0 && a.max_pairs < (1u << 28) && a.max_bases <= 0xFFFFFFFFull - 16u &&
           a.item_slots == item_slots(a.max_pairs, a.max_bases, a.chunk) && a.task_slots != 0 && a.safe_ref < a.n_refs;
}

} // namespace

hipError_t launch_refset_cand_count(const RefsetCandArgs &a, hipStream_t stream)
{
    if (!args_ok(a)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(rc_count_kernel, blocks_of((uint64_t)a.words + 1u), dim3(256), 0, stream, a);
    return launch_scan(a.pc, a.words + 1u, a.pc + a.words + 1u, stream);
}

hipError_t launch_refset_cand_stats(const RefsetCandArgs &a, hipStream_t stream)
{
    hipLaunchKernelGGL(rc_stats_kernel, dim3(1), dim3(64), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_refset_cand_list(const RefsetCandArgs &a, hipStream_t stream)
{
    if (!plan_ok(a)) return hipErrorInvalidValue;
    const uint32_t n = a.max_pairs + 1u, nb = (n + kScan64Block - 1u) / kScan64Block;
    hipLaunchKernelGGL(rc_list_kernel, blocks_of(std::max(a.words, n)), dim3(256), 0, stream, a);
    hipLaunchKernelGGL(rc_scan64_kernel, dim3(nb), dim3(256), 0, stream, a.poff, n, kScan64Block / 256u, a.bsum);
    hipLaunchKernelGGL(rc_scan64_kernel, dim3(1), dim3(1024), 0, stream, a.bsum, nb, (nb + 1023u) / 1024u, (uint64_t *)nullptr);
    hipLaunchKernelGGL(rc_cut_kernel, dim3(1), dim3(64), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_refset_cand_plan(const RefsetCandArgs &a, uint8_t *d_chars, uint4 *d_items, uint4 *d_tasks, hipStream_t stream)
{
    if (!plan_ok(a)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(rc_pairs_kernel, blocks_of((uint64_t)a.max_pairs + 1u), dim3(256), 0, stream, a, d_chars);
    hipError_t e = launch_scan(a.nch, a.max_pairs + 1u, a.nch + a.max_pairs + 1u, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(rc_refs_kernel, blocks_of((uint64_t)a.n_refs + 1u), dim3(256), 0, stream, a);
    e = launch_scan(a.ntask, a.n_refs + 1u, a.ntask + a.n_refs + 1u, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(rc_items_kernel, blocks_of((uint64_t)a.item_slots + a.task_slots), dim3(256), 0, stream, a, d_items, d_tasks);
    return hipGetLastError();
}

hipError_t launch_refset_cand_tag_runs(const RefsetCandArgs &a, const uint32_t *d_first, const uint32_t *d_local, uint32_t local_cap, uint64_t *d_count,
                                       uint64_t capacity, uint32_t *d_out, hipStream_t stream)
{
    hipLaunchKernelGGL(rc_tag_runs_kernel, blocks_of(std::max(local_cap, 1u)), dim3(256), 0, stream, a, d_first, d_local, local_cap,
                       reinterpret_cast<unsigned long long *>(d_count), capacity, d_out);
    return hipGetLastError();
}

hipError_t launch_refset_cand_tag_summaries(const RefsetCandArgs &a, const uint32_t *d_kept, const uint32_t *d_n_kept, uint64_t *d_count,
                                            uint64_t capacity, uint32_t *d_out, hipStream_t stream)
{
    hipLaunchKernelGGL(rc_tag_summaries_kernel, blocks_of(std::max<uint64_t>(std::min<uint64_t>(a.max_pairs, capacity), 1u)), dim3(256), 0, stream, a,
                       d_kept, d_n_kept, reinterpret_cast<unsigned long long *>(d_count), capacity, d_out);
    return hipGetLastError();
}

hipError_t launch_refset_cand_best(const RefsetCandArgs &a, const uint32_t *d_ext, uint32_t *d_table, hipStream_t stream)
{
    if (!plan_ok(a) || a.n_seqs >= (1u << 28)) return hipErrorInvalidValue;
    if (refset_best_splits(a.n_seqs)) hipLaunchKernelGGL(rc_best_kernel<true>, dim3(a.n_seqs), dim3(kBestThreads), 0, stream, a, d_ext, d_table);
    else hipLaunchKernelGGL(rc_best_kernel<false>, dim3((a.n_seqs + kBestWaves - 1u) / kBestWaves), dim3(kBestThreads), 0, stream, a, d_ext, d_table);
    return hipGetLastError();
}

} // namespace kbo
