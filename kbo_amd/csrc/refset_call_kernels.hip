// refset_call_kernels.hip — gfx950 (MI355X, CDNA4): the first pass of kbo::call over a slab of (reference, sequence, strand) pairs
// (kbo_call_refset).  refset_call.hpp has the candidate test, the interval of a position, the spelling of a row and
// the window of depths; this is their mapping onto lanes and waves, behind the walk and the counting derandomize of the slab.
//
//   scan   a lane per byte of the slab's matching statistics.  The test with the slab's smallest threshold costs two bytes; only a
//          lane that passes it bisects the pairs' offsets, reads its pair's threshold and whether the pair was kept (the extent's run
//          count).  A wave appends its candidates with one atomic add on the list's counter; a candidate beyond the list's capacity is
//          counted and not written, and the host repeats the slab with room for the count
//   match  a wave per candidate, grid-strided over min(count, capacity).  Lane x takes j = i + 1 + x (further rounds for k > 64): a
//          depth of at least t, then d[j] rank steps from the root over the packed form where it lies in the arena (two 8-byte loads a
//          step; LDS and wide references alike).  A ballot picks the first lane whose interval is one row; lane 0 appends the site
//   spell  a lane per site: k inverse steps over the packed form for the row's k-mer and the k depths that end at j, into the site's
//          window record
// Only the two counts, the site records and the windows leave the device.  Plain vector stores; the only atomics are the adds on the
// two list counters; no LDS, no scratch.  Every index is below a bound read from the slab's own arrays: a pair's bytes lie inside the
// slab, j inside the pair, a rank block inside the form of the pair's reference.
#include "kernels.hpp"
#include "refset_call.hpp"
#include "refset_walk.hpp"

namespace kbo {
namespace {

using namespace refcall;

struct DevSlab { // refset_call.hpp's accessor over the slab's arrays
    const uint8_t *ms_;
    const uint64_t *off_;
    const uint32_t *thr_, *ext_;
    __device__ __forceinline__ uint32_t ms(uint64_t p) const { return ms_[p]; }
    __device__ __forceinline__ uint64_t off(uint32_t x) const { return off_[x]; }
    __device__ __forceinline__ uint32_t thr(uint32_t x) const { return thr_[x]; }
    __device__ __forceinline__ bool kept(uint32_t x) const { return ext_[6u * x + 3u] != 0u; } // kbo_aln_extent::n_runs
};
struct DevSeq {
    const uint8_t *q_;
    __device__ __forceinline__ uint32_t byte(uint32_t s) const { return q_[s]; }
};
struct DevBytes {
    uint8_t *w_;
    __device__ __forceinline__ void put(uint32_t t, uint32_t v) { w_[t] = (uint8_t)v; }
};

constexpr uint32_t kWavesPerBlock = kRefsetCallThreads / kWindow;
static_assert(kWindow == 64u, "a round of positions is a wave's lanes");

__device__ __forceinline__ DevSlab slab_of(const RefsetCallArgs &a) { return DevSlab{a.ms, a.poff, a.pthr, a.ext}; }

__global__ __launch_bounds__(kRefsetCallThreads) void refset_call_scan_kernel(RefsetCallArgs a)
{
    const uint64_t p = (uint64_t)blockIdx.x * kRefsetCallThreads + threadIdx.x;
    const DevSlab s = slab_of(a);
    Cand c{0u, 0u};
    const bool hit = scan_byte(s, a.n_pairs, a.bytes, a.min_thr, p, c);
    const uint64_t mk = __ballot(hit);
    if (mk) {
        const uint32_t lane = threadIdx.x % kWindow, leader = (uint32_t)__builtin_ctzll(mk);
        uint32_t base = 0;
        if (lane == leader) base = atomicAdd(a.counts, (uint32_t)__popcll(mk));
        base = (uint32_t)__shfl((int)base, (int)leader);
        const uint32_t slot = base + __builtin_amdgcn_mbcnt_hi((uint32_t)(mk >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mk, 0u));
        if (hit && slot < a.cap) a.cands[slot] = make_uint2(c.pair, c.i);
    }
}

__global__ __launch_bounds__(kRefsetCallThreads) void refset_call_match_kernel(RefsetCallArgs a)
{
    const uint32_t lane = threadIdx.x % kWindow;
    const uint64_t waves = (uint64_t)gridDim.x * kWavesPerBlock;
    const uint32_t have = a.counts[0], n_cands = have < a.cap ? have : a.cap;
    const DevSlab s = slab_of(a);
    for (uint64_t x = (uint64_t)blockIdx.x * kWavesPerBlock + threadIdx.x / kWindow; x < n_cands; x += waves) {
        const uint2 c = a.cands[x];
        const uint32_t pair = c.x, i = c.y, t = a.pthr[pair];
        const uint64_t begin = a.poff[pair], len = a.poff[pair + 1u] - begin;
        const RefsetDesc d = a.descs[a.pref[pair]];
        const PackedForm form(a.arena + d.off, d.n_sets);
        const DevSeq q{a.q + a.pq[pair]};
        const uint32_t j_end = match_end(i, a.k, len);
        for (uint32_t j0 = i + 1u; j0 < j_end; j0 += kWindow) {
            const uint32_t j = j0 + lane;
            uint32_t row = 0;
            bool ok = false;
            if (j < j_end) {
                const uint32_t depth = s.ms(begin + j);
                ok = depth >= t && one_row(form, d.n_sets, q, j, depth, row);
            }
            const uint64_t okm = __ballot(ok);
            if (okm) {
                const int first = __builtin_ctzll(okm);
                const uint32_t hit_row = (uint32_t)__shfl((int)row, first);
                if (lane == 0u) {
                    const uint32_t slot = atomicAdd(a.counts + 16, 1u);
                    if (slot < a.cap) a.sites[slot] = make_uint4(pair, i, j0 + (uint32_t)first, hit_row); // (sites <= candidates <= cap)
                }
                break;
            }
        }
    }
}

__global__ __launch_bounds__(kRefsetCallThreads) void refset_call_spell_kernel(RefsetCallArgs a)
{
    const uint32_t have = a.counts[16], n_sites = have < a.cap ? have : a.cap;
    const uint32_t pad = window_pad(a.k), stride = window_stride(a.k);
    const DevSlab s = slab_of(a);
    for (uint64_t x = (uint64_t)blockIdx.x * kRefsetCallThreads + threadIdx.x; x < n_sites; x += (uint64_t)gridDim.x * kRefsetCallThreads) {
        const uint4 site = a.sites[x];
        const RefsetDesc d = a.descs[a.pref[site.x]];
        const PackedForm form(a.arena + d.off, d.n_sets);
        uint8_t *w = a.win + x * stride;
        DevBytes depths{w}, kmer{w + pad};
        gather_depths(s, a.poff[site.x], site.z, a.k, depths);
        spell_row(form, d.n_sets, a.k, site.w, kmer);
    }
}

} // namespace

hipError_t launch_refset_call(const RefsetCallArgs &a, hipStream_t stream)
{
    if (a.n_pairs == 0 || a.bytes == 0 || a.cap == 0 || a.k == 0) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(a.counts, 0, kRefsetCallCountBytes, stream);
    if (e != hipSuccess) return e;
    const uint64_t scan_blocks = (a.bytes + kRefsetCallThreads - 1u) / kRefsetCallThreads;
    hipLaunchKernelGGL(refset_call_scan_kernel, dim3((uint32_t)scan_blocks), dim3(kRefsetCallThreads), 0, stream, a);
    // (the counts stay on the device: grids sized by the capacity, eight workgroups a compute unit at the most, the rest by the stride)
    const uint32_t match_blocks = std::min<uint32_t>((a.cap + kWavesPerBlock - 1u) / kWavesPerBlock, 2048u);
    hipLaunchKernelGGL(refset_call_match_kernel, dim3(match_blocks), dim3(kRefsetCallThreads), 0, stream, a);
    const uint32_t spell_blocks = std::min<uint32_t>((a.cap + kRefsetCallThreads - 1u) / kRefsetCallThreads, 2048u);
    hipLaunchKernelGGL(refset_call_spell_kernel, dim3(spell_blocks), dim3(kRefsetCallThreads), 0, stream, a);
    return hipGetLastError();
}

} // namespace kbo
