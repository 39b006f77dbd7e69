// refset_locate_kernels.hip — gfx950 (MI355X, CDNA4): where the runs of kbo_find_refset lie on their references (kbo_locate_refset,
// kbo_locate_refset_dev).  refset_locate.hpp has the k-mer look-up, the strand's bases and the entry's decode; this is
// the mapping of a list of runs onto waves.
//
//   wave   one record of d_runs, grid-strided over min(*n_runs, capacity): the host does not know the count, the kernel reads it.
//          The record is checked against the descs and the batch's offsets before anything is looked up (refset_locate.hpp span_ok),
//          so garbage in d_runs gives a record with bit 4 and never an address outside the batch, the arena or the table
//   lane   lane j of group g looks up the window that starts at run.start + 64 g + j: k rank steps from the root over the packed form
//          where it lies in the arena (two 8-byte loads and a byte of the batch a step; the forms are L2-resident at these sizes),
//          leaving at the first empty interval.  '-' reads the '+' batch backwards and complements
//   ballot the lowest lane with a hit is the first anchor; the wave goes on to group g + 1 only when there is none.  The last anchor
//          is searched the same way from the back, and not at all when the first search found nothing
// Lane 0 writes the record's six words with plain stores.  No LDS, no scratch, no atomics; every loop ends at the run's last window.
#include "kernels.hpp"
#include "refset_locate.hpp"
#include "refset_walk.hpp"

namespace kbo {
namespace {

using namespace reflocate;

struct DevSeq { // refset_locate.hpp's accessors over the '+' batch and a reference's entries
    const uint8_t *q_;
    __device__ __forceinline__ uint32_t byte(uint64_t i) const { return q_[i]; }
};
struct DevPos {
    const uint32_t *pos_;
    __device__ __forceinline__ uint32_t entry(uint32_t row) const { return pos_[row]; }
};

constexpr uint32_t kWavesPerBlock = kRefsetLocateThreads / kWindow;
static_assert(kWindow == 64u, "a group of windows is a wave's lanes");

// front == true: the first group with an anchor from the front, its lowest lane; else from the back, the lane nearest the end
template <bool front>
__device__ __forceinline__ bool search(const PackedForm &form, uint32_t n, uint32_t k, const DevSeq &q, uint64_t begin, uint64_t len, bool rev,
                                       const DevPos &pos, uint32_t start, uint32_t starts, uint32_t lane, Locus &L)
{
    for (uint64_t done = 0; done < starts; done += kWindow) {
        const uint32_t lanes = group_lanes(starts - done);
        L.n_tested += lanes;
        const uint32_t at = (uint32_t)done + lane; // (used only below `lanes`: within the run's window starts)
        const uint32_t i = front ? start + at : start + (starts - 1u - at);
        const uint32_t e = lane < lanes ? kmer_entry(form, n, k, q, begin, len, rev, pos, i) : kPosNone;
        const uint64_t hits = __ballot(e != kPosNone);
        if (hits) {
            const int src = __ffsll((unsigned long long)hits) - 1;
            const uint32_t hit_e = (uint32_t)__shfl((int)e, src), hit_i = (uint32_t)__shfl((int)i, src);
            if (front) set_first(L, hit_i, hit_e);
            else set_last(L, hit_i, hit_e);
            return true;
        }
    }
    return false;
}

__global__ __launch_bounds__(kRefsetLocateThreads) void refset_locate_kernel(RefsetLocateArgs a)
{
    const uint32_t lane = threadIdx.x % kWindow;
    const uint64_t waves = (uint64_t)gridDim.x * kWavesPerBlock;
    const uint64_t have = *a.n_runs, n_records = have < a.capacity ? have : a.capacity;
    for (uint64_t x = (uint64_t)blockIdx.x * kWavesPerBlock + threadIdx.x / kWindow; x < n_records; x += waves) {
        const uint32_t *w = a.runs + x * 10u;
        const uint32_t ref = w[0], seq = w[1], strand = w[2], start = w[3], end = w[4];
        Locus L = no_locus(kFlagUnusable);
        if (ref < a.n_refs && seq < a.n_seqs && (strand == 1u || strand == 2u)) {
            const RefsetDesc d = a.descs[ref];
            const uint64_t begin = a.off[seq], seq_end = a.off[seq + 1u];
            if (!d.status && d.route != kRefsetRouteIndex && span_ok(begin, seq_end, a.total, start, end)) {
                L = no_locus(0u);
                if (end - start >= a.k) {
                    const uint32_t starts = end - start - a.k + 1u;
                    const PackedForm form(a.arena + d.off, d.n_sets);
                    const DevSeq q{a.q};
                    const DevPos pos{a.positions + a.pos_off[ref]};
                    const bool rev = strand == 2u;
                    if (search<true>(form, d.n_sets, a.k, q, begin, seq_end - begin, rev, pos, start, starts, lane, L))
                        (void)search<false>(form, d.n_sets, a.k, q, begin, seq_end - begin, rev, pos, start, starts, lane, L);
                }
            }
        }
        if (lane == 0u) {
            uint32_t *o = a.loci + x * 6u;
            o[0] = L.q_first;
            o[1] = L.ref_first;
            o[2] = L.q_last;
            o[3] = L.ref_last;
            o[4] = L.flags;
            o[5] = L.n_tested;
        }
    }
}

} // namespace

hipError_t launch_refset_locate(const RefsetLocateArgs &a, hipStream_t stream)
{
    if (a.capacity == 0) return hipSuccess;
    if (a.n_seqs == 0 || a.k == 0) return hipErrorInvalidValue;
    const uint64_t want = (a.capacity + kWavesPerBlock - 1u) / kWavesPerBlock;
    const uint32_t blocks = (uint32_t)(want < 2048u ? want : 2048u); // (eight workgroups a compute unit; the rest by the stride)
    hipLaunchKernelGGL(refset_locate_kernel, dim3(blocks), dim3(kRefsetLocateThreads), 0, stream, a);
    return hipGetLastError();
}

} // namespace kbo
