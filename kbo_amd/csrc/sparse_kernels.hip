// sparse_kernels.hip — gfx950 (MI355X, CDNA4): the sparse form of kbo::matches over a packed batch (kbo_hip.h kbo_aln_run): only
// the runs of characters other than 'M', one 12-byte record { seq, start, (length << 2) | code } each, in (seq, start) order.
// Input: the 2-bit character words of the packed layout (pack_kernels.hip: every sequence starts a word, 16 characters a u32,
// M - X R = 0 .. 3), as kbo_matches_packed_dev and pack2_kernel write them.
//
// Count, scan, emit (as rle_kernels.hip), one lane per word.  A word's characters are turned into two bit masks at once (bit
// 2 i = character i): `starts` (not 'M' and unlike the character in front of it) and `ends` (not 'M' and unlike the one behind
// it, or the sequence's last).  The characters either side of a word come from the neighbouring lanes' words (ds_bpermute), or
// from memory at a wave's two ends, and only when they belong to the same sequence.  Runs are numbered by their starts: the
// start of run r is start number r of the batch, and so is its end, since a run open at the front of word w is the only
// difference between the starts and the ends counted in front of w.  The lane that holds a run's start writes its first
// eight bytes, the lane that holds its end writes (end << 2) | code behind them, and a last pass over the records subtracts
// start << 2 - no lane has to walk a run to its end, however long it is.
//
// The grid is at most kSparseMaxBlocks workgroups that each take a contiguous range of 256-word chunks, so that the count to
// scan is one per workgroup and the number of words may be known on the device only (kbo_sparse_runs_dev).  Stores are
// vector stores only.
#include "device_util.hpp"

namespace kbo {
namespace {

// words of the batch: uniform_wps per sequence, or the scanned words-per-sequence total (launch_packed_prefix)
__device__ __forceinline__ uint32_t sparse_n_words(uint32_t n_seqs, uint32_t uniform_wps, const uint32_t *data, const uint32_t *sums)
{
    return uniform_wps ? n_seqs * uniform_wps : sums[n_seqs / kScanBlock] + data[n_seqs];
}

// the run masks of word w (every lane of the wave calls it with consecutive w: the neighbours are shuffled in).
// open = 1 when a run of the sequence is open in front of the word's first character (it goes on into the word).
struct WordRuns {
    uint32_t starts, ends, codes, seq, first, open; // codes: the word's characters, those past the sequence 'M'
};
// v = word w as the caller loaded it (0 for a word that is not this workgroup's)
__device__ __forceinline__ WordRuns word_runs(const uint32_t *__restrict__ words, uint32_t w, uint32_t v, const uint64_t *__restrict__ off,
                                              uint32_t n_seqs, uint32_t uniform_wps, const uint32_t *data, const uint32_t *sums)
{
    WordRuns r{0u, 0u, 0u, 0u, 0u, 0u};
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t up = __shfl_up(v, 1), down = __shfl_down(v, 1);
    if (__ballot(v != 0u) == 0) return r; // all 'M' (or past the batch): nothing here, nothing to look up
    if (v == 0u) return r;
    uint32_t seq, blk;
    locate_word(w, n_seqs, uniform_wps, data, sums, seq, blk);
    const uint64_t b0 = off[seq];
    const uint32_t len = (uint32_t)(off[seq + 1] - b0), first = 16u * blk;
    if (len < 3u) return r; // no alignment (derandomize.rs:274-276): no records, as kbo_find_batch_dev reports no run
    const uint32_t nb = min(16u, len - first);
    const uint32_t vm = nb == 16u ? v : v & ((1u << (2u * nb)) - 1u); // (the padding of a sequence's last word counts for nothing)
    uint32_t prev = 0u, next = 0u;                                       // the codes in front of / behind the word, 'M' when none
    if (blk > 0u) prev = (lane == 0u ? words[w - 1u] : up) >> 30;        // (a word in front of the last: all 16 codes are the sequence's)
    if (first + 16u < len) next = (lane == 63u ? words[w + 1u] : down) & 3u;
    const uint32_t nm = (vm | (vm >> 1)) & 0x55555555u;
    const uint32_t dp = vm ^ ((vm << 2) | prev), dn = vm ^ ((vm >> 2) | (next << 30));
    r.starts = nm & (dp | (dp >> 1));
    r.ends = nm & (dn | (dn >> 1));
    r.codes = vm;
    r.seq = seq;
    r.first = first;
    r.open = prev != 0u && (vm & 3u) == prev;
    return r;
}

// the words of kSparseUnroll chunks from c on, loaded before any is looked at (a wave has that many loads in flight, not one)
constexpr uint32_t kSparseUnroll = 4;
__device__ __forceinline__ void load_chunks(const uint32_t *__restrict__ words, uint32_t c, uint32_t c1, uint32_t n_words, uint32_t (&v)[kSparseUnroll])
{
#pragma unroll
    for (uint32_t u = 0; u < kSparseUnroll; u++) {
        const uint32_t w = (c + u) * 256u + threadIdx.x;
        v[u] = c + u < c1 && w < n_words ? words[w] : 0u;
    }
}

// the chunks [c0, c1) of this workgroup
__device__ __forceinline__ void sparse_range(uint32_t n_words, uint32_t &c0, uint32_t &c1)
{
    const uint32_t n_chunks = (uint32_t)(((uint64_t)n_words + 255u) / 256u);
    const uint32_t per = (n_chunks + gridDim.x - 1u) / gridDim.x;
    c0 = min((uint64_t)blockIdx.x * per, (uint64_t)n_chunks);
    c1 = min(c0 + per, n_chunks);
}

// starts per workgroup -> counts[blockIdx.x]; counts[gridDim.x] = 0 (the scan turns it into the total)
__global__ __launch_bounds__(256) void sparse_count_kernel(const uint32_t *__restrict__ words, const uint64_t *__restrict__ off, uint32_t n_seqs,
                                                           uint32_t uniform_wps, const uint32_t *__restrict__ data,
                                                           const uint32_t *__restrict__ sums, uint32_t *__restrict__ counts)
{
    __shared__ uint32_t part[4];
    const uint32_t n_words = sparse_n_words(n_seqs, uniform_wps, data, sums);
    uint32_t c0, c1;
    sparse_range(n_words, c0, c1);
    uint32_t n = 0;
    for (uint32_t c = c0; c < c1; c += kSparseUnroll) {
        uint32_t v[kSparseUnroll];
        load_chunks(words, c, c1, n_words, v);
#pragma unroll
        for (uint32_t u = 0; u < kSparseUnroll; u++)
            n += __popc(word_runs(words, (c + u) * 256u + threadIdx.x, v[u], off, n_seqs, uniform_wps, data, sums).starts);
    }
    n = wave_sum(n);
    if ((threadIdx.x & 63u) == 0) part[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
        counts[blockIdx.x] = part[0] + part[1] + part[2] + part[3];
        if (blockIdx.x == 0) counts[gridDim.x] = 0u;
    }
}

// the records: starts write { seq_base + seq, start }, ends (end << 2) | code into the third word (sparse_finish_kernel makes
// it the length); *d_total = the number of runs
__global__ __launch_bounds__(256) void sparse_emit_kernel(const uint32_t *__restrict__ words, const uint64_t *__restrict__ off, uint32_t n_seqs,
                                                          uint32_t uniform_wps, const uint32_t *__restrict__ data,
                                                          const uint32_t *__restrict__ sums, const uint32_t *__restrict__ counts,
                                                          const uint32_t *__restrict__ csums, uint32_t seq_base, uint32_t *__restrict__ runs,
                                                          uint32_t capacity, uint32_t *__restrict__ d_total)
{
    __shared__ uint32_t part[4];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t n_words = sparse_n_words(n_seqs, uniform_wps, data, sums);
    if (blockIdx.x == 0 && threadIdx.x == 0) *d_total = csums[gridDim.x / kScanBlock] + counts[gridDim.x];
    uint32_t c0, c1;
    sparse_range(n_words, c0, c1);
    uint32_t running = csums[blockIdx.x / kScanBlock] + counts[blockIdx.x]; // runs that start in front of this workgroup's words
    uint32_t v[kSparseUnroll];
    for (uint32_t c = c0; c < c1; c++) {
        const uint32_t u = (c - c0) % kSparseUnroll;
        if (u == 0) load_chunks(words, c, c1, n_words, v);
        const WordRuns r = word_runs(words, c * 256u + threadIdx.x, v[u], off, n_seqs, uniform_wps, data, sums);
        if (!__syncthreads_or((int)(r.starts | r.ends))) continue; // (the same answer in every lane of the workgroup)
        const uint32_t n = __popc(r.starts);
        uint32_t incl = n; // inclusive scan over the wave
#pragma unroll
        for (uint32_t o = 1; o < 64u; o <<= 1) {
            const uint32_t t = __shfl_up(incl, o);
            if (lane >= o) incl += t;
        }
        if (lane == 63u) part[wave] = incl;
        __syncthreads();
        uint32_t before = 0, chunk = 0;
#pragma unroll
        for (uint32_t q = 0; q < 4u; q++) {
            before += q < wave ? part[q] : 0u;
            chunk += part[q];
        }
        __syncthreads(); // (part is written again in the next chunk)
        const uint32_t slot0 = running + before + incl - n; // run number of the word's first start
        const uint32_t seq = seq_base + r.seq;
        uint32_t m = r.starts, slot = slot0;
        while (m) {
            const uint32_t i = (uint32_t)__ffs((int)m) >> 1; // (bit 2 i + 1 of the mask: __ffs is one past it)
            m &= m - 1u;
            if (slot < capacity) {
                const uint32_t rec[2] = {seq, r.first + i};
                __builtin_memcpy(runs + (uint64_t)slot * 3u, rec, 8);
            }
            slot++;
        }
        m = r.ends;
        slot = slot0 - r.open;
        while (m) {
            const uint32_t b = (uint32_t)__ffs((int)m) - 1u, i = b >> 1;
            m &= m - 1u;
            if (slot < capacity) runs[(uint64_t)slot * 3u + 2u] = ((r.first + i + 1u) << 2) | ((r.codes >> b) & 3u);
            slot++;
        }
        running += chunk;
    }
}

// (end << 2) | code -> (length << 2) | code for the records written
__global__ __launch_bounds__(256) void sparse_finish_kernel(const uint32_t *__restrict__ counts, const uint32_t *__restrict__ csums,
                                                            uint32_t n_blocks, uint32_t *__restrict__ runs, uint32_t capacity)
{
    const uint32_t total = min(csums[n_blocks / kScanBlock] + counts[n_blocks], capacity);
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < total; r += gridDim.x * blockDim.x) {
        uint32_t *p = runs + (uint64_t)r * 3u;
        p[2] -= p[1] << 2;
    }
}

} // namespace

uint32_t sparse_blocks(uint64_t words_bound)
{
    if (words_bound >= (uint64_t)kSparseMaxBlocks * 256u) return kSparseMaxBlocks; // (no rounding up that could wrap round)
    return (uint32_t)std::max<uint64_t>(1u, (words_bound + 255u) / 256u);
}

hipError_t launch_sparse_count(const uint32_t *d_words, const uint64_t *d_off, uint32_t n_seqs, uint32_t uniform_wps, const uint32_t *d_prefix,
                               uint32_t n_blocks, uint32_t *d_scratch, hipStream_t stream)
{
    if (n_seqs == 0 || n_blocks == 0 || n_blocks > kSparseMaxBlocks) return hipErrorInvalidValue;
    const uint32_t *data = uniform_wps ? nullptr : d_prefix, *sums = uniform_wps ? nullptr : d_prefix + n_seqs + 1u;
    hipLaunchKernelGGL(sparse_count_kernel, dim3(n_blocks), dim3(256), 0, stream, d_words, d_off, n_seqs, uniform_wps, data, sums, d_scratch);
    return launch_scan(d_scratch, n_blocks + 1u, d_scratch + kSparseMaxBlocks + 1u, stream);
}

hipError_t launch_sparse_emit(const uint32_t *d_words, const uint64_t *d_off, uint32_t n_seqs, uint32_t uniform_wps, const uint32_t *d_prefix,
                              uint32_t n_blocks, const uint32_t *d_scratch, uint32_t seq_base, uint32_t *d_runs, uint32_t capacity,
                              uint32_t *d_total, hipStream_t stream)
{
    if (n_seqs == 0 || n_blocks == 0 || n_blocks > kSparseMaxBlocks) return hipErrorInvalidValue;
    const uint32_t *data = uniform_wps ? nullptr : d_prefix, *sums = uniform_wps ? nullptr : d_prefix + n_seqs + 1u;
    const uint32_t *counts = d_scratch, *csums = d_scratch + kSparseMaxBlocks + 1u;
    hipLaunchKernelGGL(sparse_emit_kernel, dim3(n_blocks), dim3(256), 0, stream, d_words, d_off, n_seqs, uniform_wps, data, sums, counts, csums,
                       seq_base, d_runs, capacity, d_total);
    hipLaunchKernelGGL(sparse_finish_kernel, dim3(n_blocks), dim3(256), 0, stream, counts, csums, n_blocks, d_runs, capacity);
    return hipGetLastError();
}

} // namespace kbo
