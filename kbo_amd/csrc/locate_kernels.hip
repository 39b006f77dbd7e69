// locate_kernels.hip — the position table of an index, the segments of a walked batch and the depth of the sources (kbo_hip.h
// "Positions, segments, depth"; the arithmetic: index_locate.hpp).
//   locate_mark_kernel      a lane per base of a walked slab of the sources: at full depth the row keeps the smallest and the largest
//                           occurrence it is given (two integer atomics: whatever the arrival order, the same words)
//   locate_entries_kernel   a lane per row: the entry from the two, and the rows that have one counted
//   segment_flag_kernel     a workgroup per tile of kTile positions with kHalo on each side: every anchor's kStarts / kEnds into a byte
//                           per base, the tile's starts and ends counted
//   segment_emit_kernel     the same tiles behind the scan of those counts: the n-th start and the n-th end write their halves of
//                           record n, and one integer atomic each into delta
//   scan_*_kernel           the three-pass scan: of the tiles' counts (64-bit: starts low, ends high) and of delta (32-bit, inclusive)
// A lane never walks a sequence: a tile bisects the offsets once and marks the sequence starts inside it.
#include "device_util.hpp"
#include "index_locate.hpp"

namespace kbo {
namespace {

using namespace idxlocate;

__global__ void __launch_bounds__(kThreads) locate_mark_kernel(const uint8_t *__restrict__ ms, const uint32_t *__restrict__ lo, uint32_t len,
                                                               uint32_t k, uint32_t n_rows, uint32_t base, uint32_t rev,
                                                               uint32_t *__restrict__ mn, uint32_t *__restrict__ mx,
                                                               unsigned long long *__restrict__ n_full)
{
    uint32_t mine = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x; i < len; i += (uint64_t)gridDim.x * kThreads) {
        if (!full_depth(ms[i], k, (uint32_t)i)) continue;
        const uint32_t row = lo[i];
        if (row >= n_rows) continue;
        const uint32_t occ = occ_of(base, len, (uint32_t)i, k, rev != 0u);
        atomicMin(mn + row, occ);
        atomicMax(mx + row, occ);
        mine++;
    }
    mine = wave_sum(mine);
    if ((threadIdx.x & 63u) == 0 && mine) atomicAdd(n_full, (unsigned long long)mine);
}

__global__ void __launch_bounds__(kThreads) locate_entries_kernel(uint32_t *__restrict__ mn, const uint32_t *__restrict__ mx, uint32_t n_rows,
                                                                  unsigned long long *__restrict__ n_entries)
{
    uint32_t mine = 0;
    for (uint64_t r = (uint64_t)blockIdx.x * kThreads + threadIdx.x; r < n_rows; r += (uint64_t)gridDim.x * kThreads) {
        const uint32_t e = entry_from_minmax(mn[r], mx[r]);
        mn[r] = e;
        mine += e != kPosNone;
    }
    mine = wave_sum(mine);
    if ((threadIdx.x & 63u) == 0 && mine) atomicAdd(n_entries, (unsigned long long)mine);
}

struct SegArgs {
    const uint8_t *ms;
    const uint32_t *lo;
    const uint64_t *off;
    const uint32_t *entries;
    uint8_t *flags;
    uint64_t *counts;
    uint32_t n_seqs, n_rows, k, bridge, strand, n_delta;
    uint64_t total, capacity;
    uint32_t *segs;
    uint32_t *delta;
    uint64_t *n_segs;
};

struct DevOff {
    const uint64_t *p;
    __device__ uint64_t off(size_t s) const { return p[s]; }
};

// sseq[j], j < n_ext: seq_mark of the sequence that holds position ext_lo + j.  All threads; ends behind a barrier
__device__ void tile_sequences(const SegArgs &a, const TileSpan &sp, uint32_t *sseq, uint32_t *carry)
{
    const uint32_t t = threadIdx.x;
    for (uint32_t j = t; j < kExt; j += kThreads) sseq[j] = 0;
    __syncthreads();
    const uint32_t s0 = seq_of(DevOff{a.off}, a.n_seqs, sp.ext_lo);
    const uint64_t ext_hi = (uint64_t)sp.ext_lo + sp.n_ext;
    for (uint64_t s = (uint64_t)s0 + 1u + t; s < a.n_seqs; s += kThreads) { // (the starts inside the tile: ascending, so a lane stops at the first beyond it)
        const uint64_t o = a.off[s];
        if (o >= ext_hi) break;
        if (o > sp.ext_lo && a.off[s + 1u] > o) sseq[o - sp.ext_lo] = seq_mark((uint32_t)s);
    }
    __syncthreads();
    // inclusive max-scan: kPer consecutive positions a lane, the lanes' last values scanned in LDS
    uint32_t run = t == 0 ? seq_mark(s0) : 0u;
    for (uint32_t u = 0; u < kPer; u++) {
        const uint32_t v = sseq[t * kPer + u];
        run = v > run ? v : run;
    }
    carry[t] = run;
    __syncthreads();
    for (uint32_t step = 1; step < kThreads; step <<= 1) {
        const uint32_t v = t >= step ? carry[t - step] : 0u;
        __syncthreads();
        carry[t] = v > carry[t] ? v : carry[t];
        __syncthreads();
    }
    run = t ? carry[t - 1u] : seq_mark(s0);
    for (uint32_t u = 0; u < kPer; u++) {
        const uint32_t v = sseq[t * kPer + u];
        run = v > run ? v : run;
        sseq[t * kPer + u] = run;
    }
    __syncthreads();
}

struct DevTile {
    const uint64_t *bits;
    const uint32_t *sseq, *sent;
    const SegArgs *a;
    TileSpan sp;
    __device__ uint64_t word(uint32_t w) const { return bits[w]; }
    __device__ uint32_t seq(uint32_t j) const { return sseq[j]; }
    __device__ uint32_t entry(uint32_t j) const // (an anchor of the halo: the few lanes at a tile's edge gather it themselves)
    {
        if (j - sp.head < sp.n_tile) return sent[j - sp.head];
        return a->entries[a->lo[(uint64_t)sp.ext_lo + j]];
    }
};

// exclusive scan of a 64-bit value over the workgroup's lanes (in lane order); *total: the sum
__device__ uint64_t block_scan64(uint64_t v, uint64_t *sh, uint64_t *total)
{
    const uint32_t t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (uint32_t step = 1; step < blockDim.x; step <<= 1) {
        const uint64_t x = t >= step ? sh[t - step] : 0ull;
        __syncthreads();
        sh[t] += x;
        __syncthreads();
    }
    const uint64_t incl = sh[t];
    *total = sh[blockDim.x - 1u];
    __syncthreads();
    return incl - v;
}

__global__ void __launch_bounds__(kThreads) segment_flag_kernel(SegArgs a)
{
    __shared__ uint32_t sseq[kExt], sent[kTile], carry[kThreads];
    __shared__ uint64_t bits[kWords], sh64[kThreads];
    const uint32_t t = threadIdx.x;
    const TileSpan sp = tile_span(blockIdx.x, a.total);
    tile_sequences(a, sp, sseq, carry);
    for (uint32_t r = 0; r < kPer; r++) { // (a wave's round: 64 consecutive positions, one word of anchor bits)
        const uint32_t j = r * kThreads + t;
        bool anchor = false;
        uint32_t row = 0;
        if (j < sp.n_ext) {
            const uint64_t g = (uint64_t)sp.ext_lo + j;
            if (a.ms[g] == a.k && is_anchor(a.k, a.k, g, a.off[sseq[j] - 1u])) {
                row = a.lo[g];
                anchor = row < a.n_rows;
            }
        }
        const uint64_t b = __ballot(anchor);
        if ((t & 63u) == 0) bits[j >> 6] = b;
        if (anchor && j - sp.head < sp.n_tile) sent[j - sp.head] = a.entries[row];
    }
    __syncthreads();
    const DevTile tile{bits, sseq, sent, &a, sp};
    uint64_t f8 = 0;
    for (uint32_t u = 0; u < kTilePer; u++) {
        const uint32_t x = t * kTilePer + u, j = sp.head + x;
        if (x < sp.n_tile && (bits[j >> 6] >> (j & 63u) & 1ull)) f8 |= (uint64_t)decide(tile, j, sp.n_ext, a.bridge, sent[x]) << (8u * u);
    }
    if (t * kTilePer < sp.n_tile) *reinterpret_cast<uint64_t *>(a.flags + (uint64_t)blockIdx.x * kTile + t * kTilePer) = f8;
    uint64_t total;
    (void)block_scan64((uint64_t)__popcll(f8 & 0x0101010101010101ull) | (uint64_t)__popcll(f8 & 0x0202020202020202ull) << 32, sh64, &total);
    if (t == 0) a.counts[blockIdx.x] = total;
}

__global__ void __launch_bounds__(kThreads) segment_emit_kernel(SegArgs a)
{
    __shared__ uint32_t sseq[kExt], carry[kThreads];
    __shared__ uint64_t sh64[kThreads];
    const uint32_t t = threadIdx.x;
    const TileSpan sp = tile_span(blockIdx.x, a.total);
    const uint64_t f8 = t * kTilePer < sp.n_tile ? *reinterpret_cast<const uint64_t *>(a.flags + (uint64_t)blockIdx.x * kTile + t * kTilePer) : 0ull;
    uint64_t total;
    const uint64_t mine = (uint64_t)__popcll(f8 & 0x0101010101010101ull) | (uint64_t)__popcll(f8 & 0x0202020202020202ull) << 32;
    const uint64_t before = a.counts[blockIdx.x] + block_scan64(mine, sh64, &total);
    if (blockIdx.x == 0 && t == 0) *a.n_segs = (uint32_t)*a.n_segs; // (the scan left starts and ends there: as many of either)
    if (total == 0) return; // (uniform: a tile without a boundary, most tiles of a batch of long matches)
    tile_sequences(a, sp, sseq, carry);
    uint64_t n_start = (uint32_t)before, n_end = before >> 32;
    for (uint32_t u = 0; u < kTilePer; u++) {
        const uint32_t f = (uint32_t)(f8 >> (8u * u)) & 3u;
        if (!f) continue;
        const uint32_t j = sp.head + t * kTilePer + u, s = sseq[j] - 1u;
        const uint64_t g = (uint64_t)sp.ext_lo + j;
        const uint32_t e = a.entries[a.lo[g]], q = (uint32_t)(g - a.off[s]) + 1u - a.k;
        if (f & kStarts) {
            if (n_start < a.capacity) {
                uint32_t *o = a.segs + n_start * 7u;
                o[0] = s;
                o[1] = a.strand;
                o[2] = q;
                o[4] = e & kPosMask;
                atomicOr(o + 6, start_flags(e)); // (the word is shared with the lane that ends the record: cleared before this launch)
            }
            if (a.delta && delta_index(e, a.k, true) < a.n_delta) atomicAdd(a.delta + delta_index(e, a.k, true), delta_value(e, true));
            n_start++;
        }
        if (f & kEnds) {
            if (n_end < a.capacity) {
                uint32_t *o = a.segs + n_end * 7u;
                o[3] = q;
                o[5] = e & kPosMask;
                atomicOr(o + 6, end_flags(e));
            }
            if (a.delta && delta_index(e, a.k, false) < a.n_delta) atomicAdd(a.delta + delta_index(e, a.k, false), delta_value(e, false));
            n_end++;
        }
    }
}

// the flag words of the records that will be written, cleared
__global__ void __launch_bounds__(kThreads) segment_clear_kernel(const uint64_t *__restrict__ total, uint64_t capacity, uint32_t *__restrict__ segs)
{
    const uint64_t n = (uint32_t)*total, have = n < capacity ? n : capacity;
    for (uint64_t x = (uint64_t)blockIdx.x * kThreads + threadIdx.x; x < have; x += (uint64_t)gridDim.x * kThreads) segs[x * 7u + 6u] = 0;
}

// ---- the three-pass scan
template <typename T> __device__ T block_sum(T v, T *sh)
{
    const uint32_t t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (uint32_t step = blockDim.x / 2u; step > 0; step >>= 1) {
        if (t < step) sh[t] += sh[t + step];
        __syncthreads();
    }
    const T r = sh[0];
    __syncthreads();
    return r;
}
template <typename T> __global__ void __launch_bounds__(kThreads) scan_sum_kernel(const T *__restrict__ in, uint64_t n, T *__restrict__ sums)
{
    __shared__ T sh[kThreads];
    T v = 0;
    const uint64_t c0 = (uint64_t)blockIdx.x * kScanChunk;
    for (uint32_t u = threadIdx.x; u < kScanChunk; u += kThreads)
        if (c0 + u < n) v += in[c0 + u];
    v = block_sum(v, sh);
    if (threadIdx.x == 0) sums[blockIdx.x] = v;
}
// ONE workgroup: the sums' exclusive scan in place, kThreads at a time; the total behind them when asked for
template <typename T> __global__ void __launch_bounds__(kThreads) scan_sums_kernel(T *__restrict__ sums, uint64_t n_chunks, T *__restrict__ total_out)
{
    __shared__ T sh[kThreads];
    T run = 0;
    for (uint64_t c0 = 0; c0 < n_chunks; c0 += kThreads) {
        const uint64_t c = c0 + threadIdx.x;
        const T v = c < n_chunks ? sums[c] : (T)0;
        sh[threadIdx.x] = v;
        __syncthreads();
        for (uint32_t step = 1; step < kThreads; step <<= 1) {
            const T x = threadIdx.x >= step ? sh[threadIdx.x - step] : (T)0;
            __syncthreads();
            sh[threadIdx.x] += x;
            __syncthreads();
        }
        if (c < n_chunks) sums[c] = run + sh[threadIdx.x] - v;
        run += sh[kThreads - 1u];
        __syncthreads();
    }
    if (total_out && threadIdx.x == 0) *total_out = run;
}
template <typename T> __global__ void __launch_bounds__(kThreads) scan_apply_kernel(const T *in, uint64_t n, const T *__restrict__ sums, T *out, // (out may be in)
                                                                                     uint32_t inclusive)
{
    __shared__ T sh[kThreads];
    constexpr uint32_t per = kScanChunk / kThreads;
    const uint32_t t = threadIdx.x;
    const uint64_t at = (uint64_t)blockIdx.x * kScanChunk + (uint64_t)t * per;
    T v[per], mine = 0;
    for (uint32_t u = 0; u < per; u++) {
        v[u] = at + u < n ? in[at + u] : (T)0;
        mine += v[u];
    }
    sh[t] = mine;
    __syncthreads();
    for (uint32_t step = 1; step < kThreads; step <<= 1) {
        const T x = t >= step ? sh[t - step] : (T)0;
        __syncthreads();
        sh[t] += x;
        __syncthreads();
    }
    T run = sums[blockIdx.x] + sh[t] - mine;
    for (uint32_t u = 0; u < per; u++) {
        if (at + u < n) out[at + u] = inclusive ? run + v[u] : run;
        run += v[u];
    }
}

template <typename T> void launch_scan3(const T *in, uint64_t n, T *sums, T *out, bool inclusive, T *total_out, hipStream_t stream)
{
    const uint32_t chunks = (uint32_t)scan_chunks(n);
    hipLaunchKernelGGL(scan_sum_kernel<T>, dim3(chunks), dim3(kThreads), 0, stream, in, n, sums);
    hipLaunchKernelGGL(scan_sums_kernel<T>, dim3(1), dim3(kThreads), 0, stream, sums, (uint64_t)chunks, total_out);
    hipLaunchKernelGGL(scan_apply_kernel<T>, dim3(chunks), dim3(kThreads), 0, stream, in, n, (const T *)sums, out, inclusive ? 1u : 0u);
}

uint32_t stride_blocks(uint64_t n)
{
    const uint64_t want = (n + kThreads - 1u) / kThreads;
    return (uint32_t)(want < 1u ? 1u : want < 4096u ? want : 4096u);
}

} // namespace

hipError_t launch_locate_mark(const uint8_t *d_ms, const uint32_t *d_lo, uint32_t len, uint32_t k, uint32_t n_rows, uint32_t base, bool rev,
                              uint32_t *d_min, uint32_t *d_max, uint64_t *d_n_full, hipStream_t stream)
{
    if (len == 0) return hipSuccess;
    hipLaunchKernelGGL(locate_mark_kernel, dim3(stride_blocks(len)), dim3(kThreads), 0, stream, d_ms, d_lo, len, k, n_rows, base, rev ? 1u : 0u, d_min,
                       d_max, reinterpret_cast<unsigned long long *>(d_n_full));
    return hipGetLastError();
}

hipError_t launch_locate_entries(uint32_t *d_min, const uint32_t *d_max, uint32_t n_rows, uint64_t *d_n_entries, hipStream_t stream)
{
    if (n_rows == 0) return hipSuccess;
    hipLaunchKernelGGL(locate_entries_kernel, dim3(stride_blocks(n_rows)), dim3(kThreads), 0, stream, d_min, d_max, n_rows,
                       reinterpret_cast<unsigned long long *>(d_n_entries));
    return hipGetLastError();
}

hipError_t launch_segments(const SegmentArgs &x, hipStream_t stream)
{
    if (x.total == 0 || x.total + 16u > (1ull << 32) || x.n_seqs == 0 || x.k == 0 || x.bridge > kMaxBridge) return hipErrorInvalidValue;
    const SegWork w = seg_work(x.total);
    uint8_t *work = static_cast<uint8_t *>(x.work);
    SegArgs a;
    a.ms = x.ms;
    a.lo = x.lo;
    a.off = x.off;
    a.entries = x.entries;
    a.flags = work;
    a.counts = reinterpret_cast<uint64_t *>(work + w.counts_off);
    a.n_seqs = x.n_seqs;
    a.n_rows = x.n_rows;
    a.k = x.k;
    a.bridge = x.bridge;
    a.strand = x.strand;
    a.n_delta = x.n_delta;
    a.total = x.total;
    a.capacity = x.capacity;
    a.segs = x.segs;
    a.delta = x.delta;
    a.n_segs = x.n_segs;
    uint64_t *sums = reinterpret_cast<uint64_t *>(work + w.sums_off);
    const uint32_t tiles = n_tiles(x.total);
    hipLaunchKernelGGL(segment_flag_kernel, dim3(tiles), dim3(kThreads), 0, stream, a);
    // (the total - starts low, ends high - goes to *n_segs, which the last launch cuts down to the starts)
    launch_scan3<uint64_t>(a.counts, tiles, sums, a.counts, false, x.n_segs, stream);
    const uint64_t most = x.capacity < x.total ? x.capacity : x.total;
    hipLaunchKernelGGL(segment_clear_kernel, dim3(stride_blocks(most)), dim3(kThreads), 0, stream, (const uint64_t *)x.n_segs, x.capacity, x.segs);
    hipLaunchKernelGGL(segment_emit_kernel, dim3(tiles), dim3(kThreads), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_depth_finish(const uint32_t *d_delta, uint32_t *d_depth, uint64_t n, void *d_work, hipStream_t stream)
{
    if (n == 0) return hipSuccess;
    launch_scan3<uint32_t>(d_delta, n, static_cast<uint32_t *>(d_work), d_depth, true, nullptr, stream);
    return hipGetLastError();
}

} // namespace kbo
