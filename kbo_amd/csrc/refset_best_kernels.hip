// refset_best_kernels.hip — gfx950 (MI355X, CDNA4): the best reference of every query sequence, reduced on the device
// (kbo_best_refset / kbo_best_refset_dev).  Behind the summary stage of a slab every pair's kbo_aln_extent lies in
// d_ext; this stage folds them into the call's table of one kbo_ref_best per sequence, so that n_seqs records leave the device per
// call where kbo_summary_refset's record stage sends one per pair with a hit per slab.  refset_best.hpp has the record and its merge.
//
// A slab's pairs lie in (reference, sequence, strand) order and may begin and end in the middle of a reference (the host form cuts
// by bytes): pair p of the slab is number g = lead + p of the slab's FIRST reference on, g = (j * n_seqs + s) * n_strands + x for
// the slab's j-th reference, sequence s and strand index x - so the pairs of one sequence are strided and their places are
// arithmetic; the only list the kernel reads is the slab's references.
//   refset_best_init_kernel    once per call: the table set to the empty records
//   refset_best_kernel<false>  a wave per sequence: its lanes stride over the sequence's (reference, strand) places in the slab
//   refset_best_kernel<true>   a workgroup of four waves per sequence: the places split over 256 lanes, the waves' records through LDS
// In both a lane merges the pairs it visits, the wave reduces with merge over __shfl_xor, and ONE lane merges the result into the
// sequence's table entry: a sequence has one owner per launch and the slabs of a call are ordered on its stream, so there are no
// atomics.  merge is exact and its order of pairs total: the table does not depend on the mapping, the slab cut or the lane order.
#include "device_util.hpp"
#include "refset_best.hpp"

namespace kbo {
namespace {

using namespace refbest;

constexpr uint32_t kBestThreads = 256, kBestWaves = kBestThreads / 64u;

__global__ void refset_best_init_kernel(uint32_t *__restrict__ table, uint32_t n_seqs)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; // a lane per word
    if (i >= n_seqs * kWords) return;
    const uint32_t s = i / kWords, w = i % kWords;
    table[i] = w == 0u ? s : (w == 1u || w == 10u ? kNone : 0u);
}

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

template <bool SPLIT> __global__ __launch_bounds__(kBestThreads) void refset_best_kernel(RefsetBestArgs a)
{
    __shared__ uint32_t part[SPLIT ? kBestWaves * kWords : 1u];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t s = SPLIT ? blockIdx.x : blockIdx.x * kBestWaves + wave;
    const bool live = s < a.n_seqs; // (a wave behind the last sequence visits no place and writes nothing; it still meets no barrier)
    const uint64_t per_ref = (uint64_t)a.n_seqs * a.n_strands;
    const uint32_t places = live ? a.slab_refs * a.n_strands : 0u;
    Best mine = empty(s);
    for (uint32_t i = SPLIT ? threadIdx.x : lane; i < places; i += SPLIT ? kBestThreads : 64u) {
        const uint32_t j = i / a.n_strands, x = i % a.n_strands;
        const uint64_t g = j * per_ref + (uint64_t)s * a.n_strands + x;
        if (g < a.lead || g - a.lead >= a.n_pairs) continue; // (the slab begins or ends inside this reference)
        const uint2 *e = reinterpret_cast<const uint2 *>(a.ext + (g - a.lead) * 6u);
        const uint2 e0 = e[0], e1 = e[1], e2 = e[2];
        const uint32_t ext[6] = {e0.x, e0.y, e1.x, e1.y, e2.x, e2.y};
        mine = merge(mine, from_pair(s, a.refs[j], a.strands == 3u ? x + 1u : a.strands, ext));
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
    uint32_t *t = a.table + (size_t)s * kWords;
    mine = merge(Best{t[0], t[1], t[2], t[3], t[4], t[5], t[6], t[7], t[8], t[9], t[10], t[11]}, mine);
    t[0] = mine.seq; t[1] = mine.ref; t[2] = mine.strand; t[3] = mine.n_match; t[4] = mine.n_mismatch; t[5] = mine.n_jump;
    t[6] = mine.n_runs; t[7] = mine.start; t[8] = mine.end; t[9] = mine.n_hits; t[10] = mine.second_ref; t[11] = mine.second_match;
}

} // namespace

hipError_t launch_refset_best_init(uint32_t *d_table, uint32_t n_seqs, hipStream_t stream)
{
    if (n_seqs == 0 || n_seqs >= (1u << 28)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(refset_best_init_kernel, dim3((n_seqs * kWords + 255u) / 256u), dim3(256), 0, stream, d_table, n_seqs);
    return hipGetLastError();
}

bool refset_best_splits(uint32_t n_seqs) { return n_seqs < kRefsetBestSplitBelow; }

hipError_t launch_refset_best(const RefsetBestArgs &a, hipStream_t stream)
{
    if (a.n_pairs == 0) return hipSuccess;
    if (a.n_seqs == 0 || a.n_seqs >= (1u << 28) || a.n_strands < 1u || a.n_strands > 2u || a.slab_refs == 0 ||
        (uint64_t)a.slab_refs * a.n_strands > 0xFFFFFFFFull)
        return hipErrorInvalidValue;
    // the slab's pairs lie within its slab_refs references, and begin in the first
    const uint64_t per_ref = (uint64_t)a.n_seqs * a.n_strands;
    if (a.lead >= per_ref || a.lead + a.n_pairs > a.slab_refs * per_ref) return hipErrorInvalidValue;
    if (refset_best_splits(a.n_seqs)) hipLaunchKernelGGL(refset_best_kernel<true>, dim3(a.n_seqs), dim3(kBestThreads), 0, stream, a);
    else hipLaunchKernelGGL(refset_best_kernel<false>, dim3((a.n_seqs + kBestWaves - 1u) / kBestWaves), dim3(kBestThreads), 0, stream, a);
    return hipGetLastError();
}

} // namespace kbo
