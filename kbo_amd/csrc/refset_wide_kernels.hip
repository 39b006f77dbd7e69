// refset_wide_kernels.hip — gfx950 (MI355X, CDNA4): k-bounded matching statistics against the references of a set whose packed
// form does not fit a compute unit's LDS (kbo_refset_build_wide).  The form is the one refset_kernels.hip stages -
// 2 bytes a row: 8-byte rank blocks, then the LCS bytes with the sentinel - and nothing in it needs LDS: the walk reads it where it
// lies in the set's arena.  At most 2^20 rows, so at most 2 MiB: the workgroups of a reference's tasks re-read it from their XCD's L2
// while the query and the MS bytes stream past.
//   task   one workgroup of kRefsetThreads lanes; a task whose reference is not of the wide route returns at once
//   lane   one chunk (refset_walk.hpp): k - 1 warm-up bases for the state, then a depth per base; the query 16 bytes at a time, the depths too
//   base   refset_step.hpp's step: a rank is one 8-byte load and a population count, a contraction scans LCS bytes linearly
// The task list is the slab's, shared with refset_walk_kernel, which skips the tasks this kernel takes.  No LDS, no atomics.
#include "refset_walk.hpp"

namespace kbo {
namespace {

__global__ __launch_bounds__(kRefsetThreads) void refset_wide_walk_kernel(RefsetWalkArgs a)
{
    const uint4 task = a.tasks[blockIdx.x];
    const RefsetDesc desc = a.descs[task.x];
    if (desc.route != kRefsetRouteWide) return; // (the whole workgroup: the LDS kernel has this task)
    if (threadIdx.x >= task.z) return;
    const uint32_t n = desc.n_sets;
    refset_walk_chunk(PackedForm(a.arena + desc.off, n), n, a.k, a.items[task.y + threadIdx.x], a.q, a.ms);
}

} // namespace

hipError_t launch_refset_wide_walk(const RefsetWalkArgs &a, hipStream_t stream)
{
    if (a.n_tasks == 0) return hipSuccess;
    hipLaunchKernelGGL(refset_wide_walk_kernel, dim3(a.n_tasks), dim3(kRefsetThreads), 0, stream, a);
    return hipGetLastError();
}

} // namespace kbo
