// pileup_kernels.hip — allele counts per source base from the segments of a walked batch, and the candidate sites (kbo_hip.h "Pileup";
// the arithmetic: index_pileup.hpp).
//   pileup_kernel        waves stride over the records.  A wave takes a record's windows 64 at a time: a lane loads one MS byte, one
//                        ballot gives the anchors, and the lane of an anchor takes the gap in front of it - behind the nearest anchor
//                        below it in the ballot, or behind where the rounds before ended (a uniform value: a gap may be longer than a
//                        round at bridge 255).  A bridged base is a byte load, a projection and one integer atomic.  What lies behind
//                        the last anchor (nothing, in a record kbo_segments_dev wrote) the lanes share.
//   site_count_kernel    a workgroup per chunk of kScanChunk source bases: the sites flagged and counted
//   site_sums_kernel     ONE workgroup: the counts' exclusive scan in place, the total to *n_sites
//   site_emit_kernel     the same chunks behind that scan: the n-th site writes record n when n < capacity
// No pass waits for another workgroup of its own launch.  The number of records is read on the device: min(*d_n_segs, capacity).
#include "device_util.hpp"
#include "index_pileup.hpp"

namespace kbo {
namespace {

using namespace idxpile;

struct PArgs {
    const uint32_t *segs; // records of 7 words
    const uint64_t *n_segs;
    const uint8_t *concat, *ms;
    const uint64_t *off;
    uint32_t *pile;
    uint64_t capacity, total, source_bases;
    uint32_t n_seqs, k, skip_multi;
};

__device__ __forceinline__ void pile_base(const PArgs &a, const Segment &s, uint64_t o, uint32_t x)
{
    uint64_t word;
    if (pile_word(s, x, a.concat[o + x], a.k, a.source_bases, &word)) atomicAdd(a.pile + word, 1u);
}

__global__ void __launch_bounds__(kThreads) pileup_kernel(PArgs a)
{
    const uint32_t lane = threadIdx.x & (kRound - 1u);
    const uint64_t n_all = *a.n_segs, n = n_all < a.capacity ? n_all : a.capacity;
    const uint64_t wave = (uint64_t)blockIdx.x * kWaves + threadIdx.x / kRound, n_waves = (uint64_t)gridDim.x * kWaves;
    for (uint64_t r = wave; r < n; r += n_waves) { // (uniform over the wave from here on, but for what a lane does with its anchor)
        const uint32_t *p = a.segs + r * 7u;
        const Segment s{p[0], p[1], p[2], p[3], p[4], p[5], p[6]};
        if (!record_taken(s, a.n_seqs, a.skip_multi != 0u)) continue;
        const uint64_t o = a.off[s.seq];
        if (!record_span(s, o, a.off[(uint64_t)s.seq + 1u], a.total, a.k)) continue;
        uint64_t end = s.q_first;
        for (uint64_t w0 = s.q_first; w0 <= s.q_last; w0 += kRound) {
            const uint64_t w = w0 + lane;
            const bool anchor = w <= s.q_last && is_anchor(a.ms[anchor_byte(o, (uint32_t)w, a.k)], a.k);
            const uint64_t mask = __ballot(anchor);
            if (anchor) {
                uint64_t from;
                const uint32_t to = gap_before(mask, lane, (uint32_t)w0, end, a.k, &from);
                for (uint64_t x = from; x < to; x++) pile_base(a, s, o, (uint32_t)x);
            }
            end = round_end(mask, (uint32_t)w0, end, a.k);
        }
        for (uint64_t x = end + lane; x < (uint64_t)s.q_last + a.k; x += kRound) pile_base(a, s, o, (uint32_t)x);
    }
}

// ---- sites
struct SArgs {
    const uint4 *pile;
    const uint32_t *depth;
    const uint64_t *src_off;
    uint32_t *sums;
    uint4 *sites;
    uint64_t *n_sites;
    uint64_t source_bases, capacity;
    uint32_t n_src;
    Thresholds t;
};
struct DevSrcOff {
    const uint64_t *p;
    __device__ uint64_t off(size_t s) const { return p[s]; }
};
constexpr uint32_t kPer = kScanChunk / kThreads;

// the sites among the kPer consecutive bases of this lane, a bit each
__device__ __forceinline__ uint32_t lane_flags(const SArgs &a, uint64_t at)
{
    uint32_t f = 0;
    for (uint32_t u = 0; u < kPer; u++) {
        if (at + u >= a.source_bases) break;
        const uint4 c = a.pile[at + u];
        if ((c.x | c.y | c.z | c.w) == 0u) continue; // (most bases: nothing bridged there, and min_count is at least 1)
        if (is_site(c.x, c.y, c.z, c.w, a.depth[at + u], a.t)) f |= 1u << u;
    }
    return f;
}

__global__ void __launch_bounds__(kThreads) site_count_kernel(SArgs a)
{
    __shared__ uint32_t sh[kWaves];
    const uint32_t t = threadIdx.x;
    const uint32_t mine = wave_sum((uint32_t)__popc(lane_flags(a, (uint64_t)blockIdx.x * kScanChunk + (uint64_t)t * kPer)));
    if ((t & (kRound - 1u)) == 0) sh[t / kRound] = mine;
    __syncthreads();
    if (t == 0) {
        uint32_t v = 0;
        for (uint32_t w = 0; w < kWaves; w++) v += sh[w];
        a.sums[blockIdx.x] = v;
    }
}

__global__ void __launch_bounds__(kThreads) site_sums_kernel(uint32_t *__restrict__ sums, uint64_t n_chunks, uint64_t *__restrict__ total_out)
{
    __shared__ uint32_t sh[kThreads];
    const uint32_t t = threadIdx.x;
    uint32_t run = 0;
    for (uint64_t c0 = 0; c0 < n_chunks; c0 += kThreads) {
        const uint64_t c = c0 + t;
        const uint32_t v = c < n_chunks ? sums[c] : 0u;
        sh[t] = v;
        __syncthreads();
        for (uint32_t step = 1; step < kThreads; step <<= 1) {
            const uint32_t x = t >= step ? sh[t - step] : 0u;
            __syncthreads();
            sh[t] += x;
            __syncthreads();
        }
        if (c < n_chunks) sums[c] = run + sh[t] - v;
        run += sh[kThreads - 1u];
        __syncthreads();
    }
    if (t == 0) *total_out = run;
}

__global__ void __launch_bounds__(kThreads) site_emit_kernel(SArgs a)
{
    __shared__ uint32_t sh[kThreads];
    const uint32_t t = threadIdx.x;
    const uint64_t at = (uint64_t)blockIdx.x * kScanChunk + (uint64_t)t * kPer;
    const uint32_t f = lane_flags(a, at), mine = (uint32_t)__popc(f);
    sh[t] = mine;
    __syncthreads();
    for (uint32_t step = 1; step < kThreads; step <<= 1) {
        const uint32_t x = t >= step ? sh[t - step] : 0u;
        __syncthreads();
        sh[t] += x;
        __syncthreads();
    }
    uint64_t x = (uint64_t)a.sums[blockIdx.x] + sh[t] - mine;
    for (uint32_t u = 0; u < kPer; u++) {
        if (!(f >> u & 1u)) continue;
        if (x < a.capacity) {
            const uint64_t j = at + u;
            const uint4 c = a.pile[j];
            a.sites[2u * x] = make_uint4((uint32_t)j, seq_of(DevSrcOff{a.src_off}, a.n_src, j), a.depth[j], c.x);
            a.sites[2u * x + 1u] = make_uint4(c.y, c.z, c.w, 0u);
        }
        x++;
    }
}

} // namespace

hipError_t launch_pileup(const PileupArgs &x, hipStream_t stream)
{
    if (x.n_seqs == 0 || x.n_seqs >= kMaxSeqs || x.capacity > kMaxSegs || x.k == 0 || x.total + 16u > (1ull << 32)) return hipErrorInvalidValue;
    if (x.capacity == 0 || x.total == 0 || x.source_bases == 0) return hipSuccess;
    PArgs a;
    a.segs = x.segs;
    a.n_segs = x.n_segs;
    a.concat = x.concat;
    a.ms = x.ms;
    a.off = x.off;
    a.pile = x.pile;
    a.capacity = x.capacity;
    a.total = x.total;
    a.source_bases = x.source_bases;
    a.n_seqs = x.n_seqs;
    a.k = x.k;
    a.skip_multi = x.skip_multi ? 1u : 0u;
    const uint64_t want = (x.capacity + kWaves - 1u) / kWaves;
    hipLaunchKernelGGL(pileup_kernel, dim3((uint32_t)(want < 8192u ? want : 8192u)), dim3(kThreads), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_pileup_sites(const PileupSitesArgs &x, hipStream_t stream)
{
    if (x.n_src == 0 || x.min_count == 0 || x.frac_den == 0 || x.source_bases >= idxlocate::kMaxSourceBases) return hipErrorInvalidValue;
    SArgs a;
    a.pile = static_cast<const uint4 *>(x.pile);
    a.depth = x.depth;
    a.src_off = x.src_off;
    a.sums = static_cast<uint32_t *>(x.work);
    a.sites = static_cast<uint4 *>(x.sites);
    a.n_sites = x.n_sites;
    a.source_bases = x.source_bases;
    a.capacity = x.capacity;
    a.n_src = x.n_src;
    a.t = Thresholds{x.min_count, x.frac_num, x.frac_den};
    const uint32_t chunks = (uint32_t)scan_chunks(x.source_bases);
    if (chunks) hipLaunchKernelGGL(site_count_kernel, dim3(chunks), dim3(kThreads), 0, stream, a);
    hipLaunchKernelGGL(site_sums_kernel, dim3(1), dim3(kThreads), 0, stream, a.sums, (uint64_t)chunks, x.n_sites);
    if (chunks) hipLaunchKernelGGL(site_emit_kernel, dim3(chunks), dim3(kThreads), 0, stream, a);
    return hipGetLastError();
}

} // namespace kbo
