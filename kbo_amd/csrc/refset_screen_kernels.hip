// refset_screen_kernels.hip — gfx950 (MI355X, CDNA4): the seed screen of a reference set (kbo_refset_candidates, and the host forms
// of find / summary / best over a set built with a prefilter).  refset_screen.hpp has the seed, the shared prefix and
// the bucket scan; this is the mapping of a batch onto lanes.
//
// The batch lies on the device as upload_batch put it: '+' at q, '-' at q + rev_base, a sequence at the same offsets in both.  A
// lane owns the kRefsetScreenRun start positions [p0, p1) of one strand, counted over the whole batch, so a run may span several
// sequences; it finds the sequence of p1 - 1 by bisection and goes from RIGHT to LEFT:
//   - up to kSeedMax - 1 bases behind p1, as far as that sequence goes, only warm the seed up (they are another lane's positions)
//   - every position of [p0, p1): the seed one base to the left, its bucket, the bucket's entries; an entry of reference r that
//     shares at least m[r] bases sets bit (r * n_seqs + s) * 2 + strand - 1 of the bitmap
//   - in front of a sequence's first base the seed starts again, in the sequence before it
// The bytes come 16 at a time (the run begins at a multiple of 16 and both strands' bases do); the groups read lie below
// round_up(total, 16) <= rev_base of the strand, inside d_q.  The bit is tested before it is set: bits only ever go from 0 to 1
// within a launch, so a stale 0 costs an atomic and a 1 is true.  atomicOr is idempotent: no order, no waits, and every loop ends at
// a bucket's end or at p0.  No LDS; the table is read through L2 (bucket offsets, keys, references, the m bytes).
#include "kernels.hpp"
#include "refset_screen.hpp"

namespace kbo {
namespace {

using namespace refscreen;

struct DevTable { // refset_screen.hpp's accessor over the device copy of the table
    const uint32_t *bucket_;
    const uint64_t *key_;
    const uint32_t *ref_;
    __device__ __forceinline__ uint32_t bucket(uint32_t b) const { return bucket_[b]; }
    __device__ __forceinline__ uint64_t key(uint32_t x) const { return key_[x]; }
    __device__ __forceinline__ uint32_t ref(uint32_t x) const { return ref_[x]; }
};

__global__ __launch_bounds__(kRefsetScreenThreads) void refset_screen_kernel(RefsetScreenArgs a)
{
    const uint64_t p0 = ((uint64_t)blockIdx.x * kRefsetScreenThreads + threadIdx.x) * kRefsetScreenRun;
    if (p0 >= a.total) return;
    const uint64_t p1 = p0 + kRefsetScreenRun < a.total ? p0 + kRefsetScreenRun : a.total;
    const uint32_t strand = a.first_strand + blockIdx.y; // 1: '+', 2: '-'
    const uint8_t *q = a.q + (strand == 2u ? a.rev_base : 0u);
    // the sequence of p1 - 1: the largest s with off[s] <= p1 - 1 (off[0] = 0 qualifies, off[n_seqs] = total does not)
    uint32_t s = 0, s1 = a.n_seqs;
    while (s1 - s > 1u) {
        const uint32_t m = s + (s1 - s) / 2u;
        if (a.off[m] <= p1 - 1u) s = m;
        else s1 = m;
    }
    uint64_t begin = a.off[s];
    const uint64_t seq_end = a.off[s + 1u];
    const uint64_t e = p1 + (kSeedMax - 1u) < seq_end ? p1 + (kSeedMax - 1u) : seq_end; // warm-up: [p1, e)
    const DevTable table{a.bucket, a.keys, a.refs};
    Seed seed{0u, 0u};
    for (uint64_t g = (e + 15u) / 16u; g-- > p0 / 16u;) {
        const uint4 v = *reinterpret_cast<const uint4 *>(q + g * 16u);
        for (int j = 15; j >= 0; j--) {
            const uint64_t pos = g * 16u + (uint32_t)j;
            if (pos >= e) continue;
            while (pos < begin && s > 0u) { // (off[0] = 0 <= pos ends it; an empty sequence is stepped over)
                s--;
                begin = a.off[s];
                seed = Seed{0u, 0u};
            }
            const uint32_t w = (j & 8) ? ((j & 4) ? v.w : v.z) : ((j & 4) ? v.y : v.x);
            seed = step_left(seed, (w >> (8u * ((uint32_t)j & 3u))) & 0xFFu);
            if (pos >= p1) continue;
            const uint64_t pair = (uint64_t)s * 2u + (strand - 1u);
            scan(table, seed, [&](uint32_t r, uint32_t shared) {
                if (shared < a.m[r]) return;
                const uint64_t bit = (uint64_t)r * a.n_seqs * 2u + pair;
                uint32_t *word = a.bits + (bit >> 5);
                const uint32_t mask = 1u << (bit & 31u);
                if (!(__atomic_load_n(word, __ATOMIC_RELAXED) & mask)) atomicOr(word, mask);
            });
        }
    }
}

} // namespace

hipError_t launch_refset_screen(const RefsetScreenArgs &a, hipStream_t stream)
{
    if (a.total == 0) return hipSuccess;
    if (a.n_seqs == 0 || a.strands < 1u || a.strands > 3u || a.first_strand != (a.strands == 2u ? 2u : 1u) || (a.rev_base & 15u) ||
        a.rev_base < a.total || a.total >= (1ull << 31) || ((uintptr_t)a.q & 15u))
        return hipErrorInvalidValue;
    const uint64_t lanes = (a.total + kRefsetScreenRun - 1u) / kRefsetScreenRun;
    const uint32_t blocks = (uint32_t)((lanes + kRefsetScreenThreads - 1u) / kRefsetScreenThreads);
    hipLaunchKernelGGL(refset_screen_kernel, dim3(blocks, a.strands == 3u ? 2u : 1u), dim3(kRefsetScreenThreads), 0, stream, a);
    return hipGetLastError();
}

} // namespace kbo
