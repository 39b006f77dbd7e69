// refset_plan_kernels.hip — gfx950 (MI355X, CDNA4): the slab planner and the record stage of the device-resident reference-set
// calls (kbo_find_refset_dev / kbo_summary_refset_dev).  What refset.cpp plans on the host slab by slab - pair
// offsets and thresholds, the walk's items and tasks - comes from the batch's offsets on the device here, and the records of a slab
// get their (ref, seq, strand) in front and their place in the call's list without a count leaving the device.  refset_plan.hpp has
// the arithmetic (tools/refset_plan_check.cpp runs it on the CPU against the host's plan).
//   rp_count_kernel     once per call: chunks of every sequence, a flag per queryable reference (then two scans), the count zeroed
//   rp_refs_kernel      once per call: the queryable references, listed
//   rp_pairs_kernel     lane = pair of the slab: its first byte and threshold; a pair of fewer than 3 bases gets its characters '-'
//   rp_items_kernel     lane = item slot of the slab: the walk's item, and every 256th lane the task of the 256 slots it heads
//   rp_tag_runs_kernel / rp_tag_summaries_kernel   lane = record of the slab: its pair found, { ref, seq, strand, record } written
//                       behind the records of the slabs before
//   rp_add_kernel       one lane: the slab's records added to the call's count
// Per call 6 launches, per slab 4 (pairs, items, tag, add); stream order is the only synchronisation, no atomics.  Integer work only.
#include "device_util.hpp"
#include "refset_plan.hpp"

#include <algorithm>

namespace kbo {
namespace {

using namespace refplan;

static_assert(kChunkMin == kRefsetChunk && kTaskItems == kRefsetThreads, "refset_plan.hpp states the walk's constants");

__device__ __forceinline__ uint32_t scanned(const uint32_t *data, const uint32_t *sums, uint32_t i) { return sums[i / kScanBlock] + data[i]; }

__global__ void rp_count_kernel(const uint64_t *__restrict__ off, uint32_t n_seqs, uint32_t chunk, const uint32_t *__restrict__ thr, uint32_t n_refs,
                                uint32_t *__restrict__ nch, uint32_t *__restrict__ qflag, unsigned long long *__restrict__ count)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i <= n_seqs) nch[i] = i < n_seqs ? chunks_of(off[i + 1] - off[i], chunk) : 0u;
    if (i <= n_refs) qflag[i] = i < n_refs && thr[i] ? 1u : 0u; // (a reference that cannot be queried has no threshold)
    if (i == 0) *count = 0ull;
}

__global__ void rp_refs_kernel(const uint32_t *__restrict__ thr, uint32_t n_refs, const uint32_t *__restrict__ qflag,
                               const uint32_t *__restrict__ qsums, uint32_t *__restrict__ qref)
{
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < n_refs && thr[r]) qref[scanned(qflag, qsums, r)] = r;
}

__global__ void rp_pairs_kernel(RefsetPlan a, uint32_t first_q, uint32_t refs, uint64_t *__restrict__ poff, uint32_t *__restrict__ pthr,
                                uint8_t *__restrict__ chars)
{
    const uint32_t n_pairs = refs * a.g.n_seqs * a.g.n_strands;
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p > n_pairs) return;
    if (p == n_pairs) {
        poff[p] = slab_bytes(a.g, refs);
        return;
    }
    const Pair pr = pair_of(a.g, p);
    const uint64_t b = a.off[pr.s], len = a.off[pr.s + 1] - b, o = pair_offset(a.g, pr.j, pr.x, b, len);
    poff[p] = o;
    pthr[p] = a.thr[a.qref[first_q + pr.j]];
    if (chars && len < 3u) // (the derandomize stage skips the pair and leaves these bytes as they are; the run-length stage reads them)
        for (uint64_t i = 0; i < len; i++) chars[o + i] = (uint8_t)'-';
}

__global__ void rp_items_kernel(RefsetPlan a, uint32_t first_q, uint32_t refs, uint4 *__restrict__ items, uint4 *__restrict__ tasks)
{
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (uint64_t)refs * a.g.item_slots) return;
    const uint32_t j = (uint32_t)(t / a.g.item_slots), i = (uint32_t)(t % a.g.item_slots);
    auto first = [&](uint32_t s) { return scanned(a.nch, a.nch_sums, s); };
    const uint32_t real = a.g.n_strands * first(a.g.n_seqs);
    if (i % kTaskItems == 0u) {
        const Words4 w = make_task(a.g, a.qref[first_q + j], j, i / kTaskItems, real);
        tasks[j * a.g.tasks_per_ref + i / kTaskItems] = make_uint4(w.x, w.y, w.z, w.w);
    }
    if (i >= real) return; // (a slot behind the reference's items: no task counts it)
    const ItemAt at = item_at(a.g, i, first);
    const uint64_t b = a.off[at.s];
    const Words4 w = make_item(a.g, j, at, b, a.off[at.s + 1] - b);
    items[t] = make_uint4(w.x, w.y, w.z, w.w);
}

// record x of the slab, WORDS words of it at src + WORDS x, to { ref, seq, strand, those words } at element base + x of the call's
// list when that lies in front of `capacity`
template <uint32_t WORDS>
__device__ __forceinline__ void rp_tag(const RefsetPlan &a, uint32_t first_q, uint32_t p, const uint32_t *__restrict__ src, uint64_t at, uint64_t capacity,
                                       uint32_t *__restrict__ out)
{
    if (at >= capacity) return;
    const Pair pr = pair_of(a.g, p);
    uint32_t *o = out + at * (3u + WORDS);
    o[0] = a.qref[first_q + pr.j];
    o[1] = pr.s;
    o[2] = strand_of(a.g, pr.x);
#pragma unroll
    for (uint32_t i = 0; i < WORDS; i++) o[3u + i] = src[i];
}

// first: launch_rle_seg_count's plain prefix over the slab's pairs; local: launch_rle_seg_emit's records, the first local_cap of them
__global__ void rp_tag_runs_kernel(RefsetPlan a, uint32_t first_q, uint32_t n_pairs, const uint32_t *__restrict__ first, const uint32_t *__restrict__ local,
                                   uint32_t local_cap, const unsigned long long *__restrict__ count, uint64_t capacity, uint32_t *__restrict__ out)
{
    const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= local_cap || x >= first[n_pairs]) return;
    const uint32_t p = record_owner(n_pairs, x, [&](uint32_t q) { return first[q]; });
    rp_tag<7u>(a, first_q, p, local + (size_t)x * 7u, *count + x, capacity, out);
}

// kept: launch_refset_keep's records { pair, extent }, *n_kept of them
__global__ void rp_tag_summaries_kernel(RefsetPlan a, uint32_t first_q, uint32_t n_pairs, const uint32_t *__restrict__ kept, const uint32_t *__restrict__ n_kept,
                                        const unsigned long long *__restrict__ count, uint64_t capacity, uint32_t *__restrict__ out)
{
    const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= n_pairs || x >= *n_kept) return;
    const uint32_t *rec = kept + (size_t)x * 7u;
    rp_tag<6u>(a, first_q, rec[0], rec + 1, *count + x, capacity, out);
}

__global__ void rp_add_kernel(unsigned long long *__restrict__ count, const uint32_t *__restrict__ n)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) *count += *n;
}

dim3 blocks_of(uint64_t lanes) { return dim3((unsigned)((lanes + 255u) / 256u)); }

} // namespace

hipError_t launch_refset_plan_call(const RefsetPlan &a, uint32_t n_refs, uint32_t *d_nch, uint32_t *d_qflag, uint32_t *d_qref, uint64_t *d_count,
                                   hipStream_t stream)
{
    const uint32_t ns = a.g.n_seqs + 1u, nr = n_refs + 1u;
    hipLaunchKernelGGL(rp_count_kernel, blocks_of(std::max(ns, nr)), dim3(256), 0, stream, a.off, a.g.n_seqs, a.g.chunk, a.thr, n_refs, d_nch, d_qflag,
                       reinterpret_cast<unsigned long long *>(d_count));
    hipError_t e = launch_scan(d_nch, ns, d_nch + ns, stream);
    if (e != hipSuccess) return e;
    e = launch_scan(d_qflag, nr, d_qflag + nr, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(rp_refs_kernel, blocks_of(n_refs), dim3(256), 0, stream, a.thr, n_refs, d_qflag, d_qflag + nr, d_qref);
    return hipGetLastError();
}

hipError_t launch_refset_plan_slab(const RefsetPlan &a, uint32_t first_q, uint32_t refs, uint64_t *d_poff, uint32_t *d_pthr, uint8_t *d_chars,
                                   uint4 *d_items, uint4 *d_tasks, hipStream_t stream)
{
    if (refs == 0) return hipErrorInvalidValue;
    const uint64_t n_pairs = (uint64_t)refs * a.g.n_seqs * a.g.n_strands, slots = (uint64_t)refs * a.g.item_slots;
    if (n_pairs >= (1ull << 28) || slots > 0xFFFFFF00ull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(rp_pairs_kernel, blocks_of(n_pairs + 1u), dim3(256), 0, stream, a, first_q, refs, d_poff, d_pthr, d_chars);
    hipLaunchKernelGGL(rp_items_kernel, blocks_of(slots), dim3(256), 0, stream, a, first_q, refs, d_items, d_tasks);
    return hipGetLastError();
}

hipError_t launch_refset_tag_runs(const RefsetPlan &a, uint32_t first_q, uint32_t n_pairs, const uint32_t *d_first, const uint32_t *d_local,
                                  uint32_t local_cap, uint64_t *d_count, uint64_t capacity, uint32_t *d_out, hipStream_t stream)
{
    unsigned long long *count = reinterpret_cast<unsigned long long *>(d_count);
    if (local_cap)
        hipLaunchKernelGGL(rp_tag_runs_kernel, blocks_of(local_cap), dim3(256), 0, stream, a, first_q, n_pairs, d_first, d_local, local_cap, count, capacity,
                           d_out);
    hipLaunchKernelGGL(rp_add_kernel, dim3(1), dim3(64), 0, stream, count, d_first + n_pairs);
    return hipGetLastError();
}

hipError_t launch_refset_tag_summaries(const RefsetPlan &a, uint32_t first_q, uint32_t n_pairs, const uint32_t *d_kept, const uint32_t *d_n_kept,
                                       uint64_t *d_count, uint64_t capacity, uint32_t *d_out, hipStream_t stream)
{
    unsigned long long *count = reinterpret_cast<unsigned long long *>(d_count);
    if (capacity)
        hipLaunchKernelGGL(rp_tag_summaries_kernel, blocks_of(std::min<uint64_t>(n_pairs, capacity)), dim3(256), 0, stream, a, first_q, n_pairs, d_kept,
                           d_n_kept, count, capacity, d_out);
    hipLaunchKernelGGL(rp_add_kernel, dim3(1), dim3(64), 0, stream, count, d_n_kept);
    return hipGetLastError();
}

} // namespace kbo
