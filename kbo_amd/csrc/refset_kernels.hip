// refset_kernels.hip — k-bounded matching statistics against a SET of small indexes (kbo_find_refset).
//
// The walks of walk_kernels.hip read ONE index's rank blocks and contraction entries from HBM.  A gene database is hundreds to
// thousands of indexes of a few thousand rows each, and every one of them fits in a compute unit's LDS: a workgroup takes one
// reference, stages its LDS form (kernels.hpp: 8-byte rank blocks of 32 rows per character, the LCS bytes; 2 bytes a row) with
// 16-byte loads, and then every lane walks one chunk of the query against it.  Everything a base needs comes from LDS:
//   extend   [l, r) by c  ->  [rank_c(l), rank_c(r))           two ds_read_b64 (the block's count has C[c] folded in)
//   contract              ->  m = max(LCS[l], LCS[r]); l goes down and r goes up while their LCS bytes are >= m; depth = m
//                             (the levels between the depth and m leave the interval as it is, so the reference's loop of
//                             single levels, index.rs:243-256, fails its extension at each of them: they are skipped)
// The scans are linear in the LCS bytes: contracting to level m passes about n / 4^m rows and happens when a string of m + 2
// bases is absent from the reference, which for the levels that are wide is rare.  Rows are random from one base to the next, so
// the lanes' LDS addresses are: bank conflicts are those of 64 random addresses and no layout avoids them.
#include "refset_walk.hpp"

namespace kbo {
namespace {

__global__ __launch_bounds__(kRefsetThreads) void refset_walk_kernel(RefsetWalkArgs a)
{
    extern __shared__ uint4 smem[];
    const uint4 task = a.tasks[blockIdx.x];
    const RefsetDesc desc = a.descs[task.x];
    if (desc.route != kRefsetRouteLds) return; // (the whole workgroup, before anything is staged: refset_wide_kernels.hip has this task)
    const uint32_t n = desc.n_sets, units = refset_units(n);
    const uint4 *src = a.arena + desc.off;
    for (uint32_t i = threadIdx.x; i < units; i += kRefsetThreads) smem[i] = src[i];
    __syncthreads();
    if (threadIdx.x >= task.z) return;
    refset_walk_chunk(PackedForm(smem, n), n, a.k, a.items[task.y + threadIdx.x], a.q, a.ms);
}

// kbo_summary_refset: the pairs of a slab with a hit (n_runs > 0), kept in pair order.  ext: six words a pair (kbo_aln_extent)
__global__ void refset_keep_flag_kernel(const uint32_t *__restrict__ ext, uint32_t n_pairs, uint32_t *__restrict__ flag)
{
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p > n_pairs) return;
    flag[p] = p < n_pairs && ext[(size_t)p * 6u + 3u] ? 1u : 0u;
}

// kept record: { pair, the six words of its extent }; *total: their number
__global__ void refset_keep_kernel(const uint32_t *__restrict__ ext, uint32_t n_pairs, const uint32_t *__restrict__ at,
                                   const uint32_t *__restrict__ sums, uint32_t *__restrict__ kept, uint32_t *__restrict__ total)
{
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p > n_pairs) return;
    const uint32_t pos = sums[p / kScanBlock] + at[p];
    if (p == n_pairs) {
        *total = pos;
        return;
    }
    const uint32_t *e = ext + (size_t)p * 6u;
    if (!e[3]) return;
    uint32_t *o = kept + (size_t)pos * 7u;
    o[0] = p;
    for (uint32_t i = 0; i < 6u; i++) o[1u + i] = e[i];
}

} // namespace

hipError_t launch_refset_keep(const uint32_t *d_ext, uint32_t n_pairs, uint32_t *d_scratch, uint32_t *d_kept, uint32_t *d_total, hipStream_t stream)
{
    if (n_pairs == 0) return hipErrorInvalidValue;
    const dim3 blocks((n_pairs + 1u + 255u) / 256u);
    hipLaunchKernelGGL(refset_keep_flag_kernel, blocks, dim3(256), 0, stream, d_ext, n_pairs, d_scratch);
    const hipError_t e = launch_scan(d_scratch, n_pairs + 1u, d_scratch + n_pairs + 1u, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(refset_keep_kernel, blocks, dim3(256), 0, stream, d_ext, n_pairs, d_scratch, d_scratch + n_pairs + 1u, d_kept, d_total);
    return hipGetLastError();
}

hipError_t launch_refset_walk(const RefsetWalkArgs &a, uint32_t lds_units, hipStream_t stream)
{
    if (a.n_tasks == 0) return hipSuccess;
    if (lds_units > refset_units(kRefsetMaxRows)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(refset_walk_kernel, dim3(a.n_tasks), dim3(kRefsetThreads), (size_t)lds_units * 16u, stream, a);
    return hipGetLastError();
}

} // namespace kbo
