// refset_cover_kernels.hip — gfx950 (MI355X, CDNA4): depth and breadth of every reference of a set over the runs of kbo_find_refset
// (kbo_cover_refset, kbo_cover_refset_dev).  refset_cover.hpp has the arithmetic and the layout of d_work - the
// references' counters, then H, one word per base of every reference with entries; this is its mapping onto waves.  Three launches
// behind a clear of d_work, stream order the only synchronisation between them:
//
//   count   a wave per record of d_runs, grid-strided over min(*n_runs, capacity) and checked as refset_locate_kernel checks it - an
//           unusable record is skipped.  Lane j of group g looks up the window at run.start + 64 g + j (refset_locate.hpp kmer_entry)
//           and on an anchor adds 1 to H[base_off[ref] + p]; EVERY group is visited.  The ballots' counts of anchors and of MULTI
//           anchors stay in the wave and go to the reference's counters once, with the run.  Integer atomics only: any order of the
//           runs gives the same words
//   scan    a wave per reference, grid-strided: 64 words a step, an inclusive sum over the lanes by six shuffles, the sum of the
//           steps before in a register; in place
//   reduce  a wave per reference, grid-strided, a lane per base over tiles of 64: D[j] = S[j] - S[j - k] from two loads (S is not
//           written any more), to d_depth when given.  The tile's covered bases and segment starts are ballots (the base in front of
//           lane 0 comes from the tile before), its largest D six shuffles; refset_cover.hpp tile_add folds them.  Lane 0 writes the
//           record's twelve words with plain stores - also for a reference without entries, which owns no word of H.  No atomics
// No LDS, no scratch; every loop ends at the run's last window or the reference's last base.
#include "kernels.hpp"
#include "refset_cover.hpp"
#include "refset_walk.hpp"

namespace kbo {
namespace {

using namespace reflocate;
using namespace refcover;

struct DevSeq { // refset_locate.hpp's accessors over the '+' batch and a reference's entries
    const uint8_t *q_;
    __device__ __forceinline__ uint32_t byte(uint64_t i) const { return q_[i]; }
};
struct DevPos {
    const uint32_t *pos_;
    __device__ __forceinline__ uint32_t entry(uint32_t row) const { return pos_[row]; }
};

constexpr uint32_t kWavesPerBlock = kRefsetCoverThreads / kWindow;
static_assert(kWindow == 64u && kTile == 64u, "a group of windows and a tile of bases are a wave's lanes");

__device__ __forceinline__ bool has_entries(const RefsetDesc &d) { return !d.status && d.route != kRefsetRouteIndex; }
__device__ __forceinline__ uint64_t *counters(const RefsetCoverArgs &a, uint32_t ref)
{
    return reinterpret_cast<uint64_t *>(a.work + (uint64_t)ref * kCounterBytes);
}
__device__ __forceinline__ uint32_t *words(const RefsetCoverArgs &a) { return reinterpret_cast<uint32_t *>(a.work + counter_bytes(a.n_refs)); }

__global__ __launch_bounds__(kRefsetCoverThreads) void refset_cover_count_kernel(RefsetCoverArgs a)
{
    const uint32_t lane = threadIdx.x % kWindow;
    const uint64_t waves = (uint64_t)gridDim.x * kWavesPerBlock;
    const uint64_t have = *a.n_runs, n_records = have < a.capacity ? have : a.capacity;
    uint32_t *H = words(a);
    for (uint64_t x = (uint64_t)blockIdx.x * kWavesPerBlock + threadIdx.x / kWindow; x < n_records; x += waves) {
        const uint32_t *w = a.runs + x * 10u;
        const uint32_t ref = w[0], seq = w[1], strand = w[2], start = w[3], end = w[4];
        if (!(ref < a.n_refs && seq < a.n_seqs && (strand == 1u || strand == 2u))) continue;
        const RefsetDesc d = a.descs[ref];
        const uint64_t begin = a.off[seq], seq_end = a.off[seq + 1u];
        if (!has_entries(d) || !span_ok(begin, seq_end, a.total, start, end)) continue;
        uint32_t n_anchors = 0, n_multi = 0; // (a run has fewer than 2^32 windows)
        if (end - start >= a.k) {
            const uint32_t starts = end - start - a.k + 1u;
            const uint64_t base = a.base_off[ref];
            const uint32_t len = a.ref_len[ref];
            const PackedForm form(a.arena + d.off, d.n_sets);
            const DevSeq q{a.q};
            const DevPos pos{a.positions + a.pos_off[ref]};
            const bool rev = strand == 2u;
            for (uint64_t done = 0; done < starts; done += kWindow) {
                const uint32_t lanes = group_lanes(starts - done);
                const uint32_t i = start + (uint32_t)done + lane; // (used only below `lanes`: within the run's window starts)
                const uint32_t e = lane < lanes ? kmer_entry(form, d.n_sets, a.k, q, begin, seq_end - begin, rev, pos, i) : kPosNone;
                uint32_t p;
                const bool hit = hit_start(e, len, p);
                if (hit) atomicAdd(&H[base + p], 1u);
                n_anchors += (uint32_t)__popcll(__ballot(hit));
                n_multi += (uint32_t)__popcll(__ballot(hit && (e & kMulti)));
            }
        }
        if (lane == 0u) {
            uint64_t *c = counters(a, ref);
            if (n_anchors) atomicAdd(reinterpret_cast<unsigned long long *>(c), (unsigned long long)n_anchors);
            if (n_multi) atomicAdd(reinterpret_cast<unsigned long long *>(c + 1), (unsigned long long)n_multi);
            atomicAdd(reinterpret_cast<uint32_t *>(c + 2), 1u);
        }
    }
}

__global__ __launch_bounds__(kRefsetCoverThreads) void refset_cover_scan_kernel(RefsetCoverArgs a)
{
    const uint32_t lane = threadIdx.x % kTile;
    const uint32_t waves = gridDim.x * kWavesPerBlock;
    uint32_t *H = words(a);
    for (uint32_t r = blockIdx.x * kWavesPerBlock + threadIdx.x / kTile; r < a.n_refs; r += waves) {
        const uint64_t base = a.base_off[r];
        const uint32_t len = (uint32_t)(a.base_off[r + 1u] - base); // (0 for a reference without entries)
        uint32_t carry = 0;
        for (uint32_t t = 0; t < len; t += kTile) {
            const bool in = lane < len - t;
            uint32_t v = in ? H[base + t + lane] : 0u;
#pragma unroll
            for (uint32_t d = 1; d < kTile; d <<= 1) {
                const uint32_t up = (uint32_t)__shfl_up((int)v, d);
                if (lane >= d) v += up;
            }
            if (in) H[base + t + lane] = v + carry;
            carry += (uint32_t)__shfl((int)v, (int)kTile - 1); // (lanes beyond the reference add 0: the last lane has the tile's sum)
        }
    }
}

__global__ __launch_bounds__(kRefsetCoverThreads) void refset_cover_reduce_kernel(RefsetCoverArgs a)
{
    const uint32_t lane = threadIdx.x % kTile;
    const uint32_t waves = gridDim.x * kWavesPerBlock;
    const uint32_t *S = words(a);
    for (uint32_t r = blockIdx.x * kWavesPerBlock + threadIdx.x / kTile; r < a.n_refs; r += waves) {
        const uint32_t ref_len = a.ref_len[r];
        Cover c = no_entries(ref_len);
        if (has_entries(a.descs[r])) {
            const uint64_t base = a.base_off[r];
            Tally tally = no_tally();
            uint32_t prev_tile = 0; // D of the base in front of the tile
            for (uint32_t t = 0; t < ref_len; t += kTile) {
                const uint32_t j = t + lane;
                const bool in = j < ref_len;
                const uint32_t d = in ? depth_of(S[base + j], j >= a.k ? S[base + j - a.k] : 0u) : 0u;
                if (in && a.depth) a.depth[base + j] = d;
                const uint32_t up = (uint32_t)__shfl_up((int)d, 1u);
                const uint32_t prev = lane ? up : prev_tile;
                const uint64_t covered = __ballot(d != 0u), starts = __ballot(d != 0u && prev == 0u);
                uint32_t m = d;
#pragma unroll
                for (uint32_t s = kTile / 2u; s; s >>= 1) {
                    const uint32_t o = (uint32_t)__shfl_xor((int)m, (int)s);
                    m = o > m ? o : m;
                }
                tile_add(tally, t, covered, starts, m);
                prev_tile = (uint32_t)__shfl((int)d, (int)kTile - 1);
            }
            const uint64_t *cnt = counters(a, r);
            c = finish(ref_len, tally, *reinterpret_cast<const uint32_t *>(cnt + 2), cnt[0], cnt[1]);
        }
        if (lane == 0u) {
            uint32_t *o = a.covers + (uint64_t)r * 12u;
            o[0] = c.ref_len;
            o[1] = c.covered;
            o[2] = c.n_segments;
            o[3] = c.first;
            o[4] = c.last;
            o[5] = c.max_depth;
            o[6] = c.n_runs;
            o[7] = c.flags;
            o[8] = (uint32_t)c.n_anchors;
            o[9] = (uint32_t)(c.n_anchors >> 32);
            o[10] = (uint32_t)c.n_multi;
            o[11] = (uint32_t)(c.n_multi >> 32);
        }
    }
}

uint32_t blocks_for(uint64_t waves_wanted)
{
    const uint64_t want = (waves_wanted + kWavesPerBlock - 1u) / kWavesPerBlock;
    return (uint32_t)(want < 2048u ? (want ? want : 1u) : 2048u); // (eight workgroups a compute unit; the rest by the stride)
}

} // namespace

hipError_t launch_refset_cover(const RefsetCoverArgs &a, hipStream_t stream)
{
    if (a.n_refs == 0 || a.n_seqs == 0 || a.k == 0) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(a.work, 0, (size_t)work_bytes(a.n_refs, a.bases), stream);
    if (e != hipSuccess) return e;
    if (a.capacity) {
        hipLaunchKernelGGL(refset_cover_count_kernel, dim3(blocks_for(a.capacity)), dim3(kRefsetCoverThreads), 0, stream, a);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        hipLaunchKernelGGL(refset_cover_scan_kernel, dim3(blocks_for(a.n_refs)), dim3(kRefsetCoverThreads), 0, stream, a);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    hipLaunchKernelGGL(refset_cover_reduce_kernel, dim3(blocks_for(a.n_refs)), dim3(kRefsetCoverThreads), 0, stream, a);
    return hipGetLastError();
}

} // namespace kbo
