// summary_kernels.hip — gfx950 (MI355X, CDNA4): per-sequence alignment summaries (kbo_hip.h kbo_aln_summary) of characters that are
// already in memory: one 16-byte record { 'M's, 'X's, 'R's, runs } per sequence, a run being a maximal stretch without '-'
// (format::run_lengths_gapped with max_gap_len = 0 closes a run at every '-': what kbo_find_batch counts).  The form for every batch
// that map_reads_kernel does not count itself (map_kernels.hip), and kbo_summary_dev / kbo_summary_words_dev on their own.
//
// Input: one byte a character (kbo_matches_batch's M - X R), or the 2-bit character words of the packed layout (pack_kernels.hip:
// every sequence starts a word, 16 characters a u32, M - X R = 0 .. 3).  Either way the characters are laid out along one axis of
// UNITS - for bytes the 16-byte aligned blocks of memory the characters stand in, for words the words themselves, 16 units each - and
// sequence s owns the units [begin(s), begin(s) + len(s)).  A lane classifies one whole block / word into bit masks (is 'M', is 'X',
// is 'R', is not '-'), a wave takes a TILE of 64 of them (1 024 units) and walks the sequences that meet it: per sequence the lanes
// mask their bits to its units, count, and the wave sums - two sums of two 16-bit fields, a tile holds at most 1 024 of anything.
// A run is counted where it STARTS (a character that is not '-' behind one that is, or at the sequence's head; the character in
// front of a block comes from the neighbouring lane, in front of a tile from memory), so one that crosses a block, a tile or a
// wave's range is counted once.  The boundaries of 64 sequences at a time sit in the lanes (one coalesced load), and lane j keeps
// the record of sequence j of that window: a window leaves as one store of 16 bytes per lane.  A wave takes a contiguous range of
// tiles; a sequence that lies inside it is stored, one that crosses into another wave's range - a contig is reduced by as many
// waves as it has KiB - is added to its record with atomics (the records are zeroed in front of the kernel).
// Sequences of fewer than 3 bases have no alignment (the reference asserts, derandomize.rs:274-276): zeros, whatever their
// characters in memory are.  Stores are vector stores only.
#include "device_util.hpp"

namespace kbo {
namespace {

constexpr uint32_t kSummaryTile = 1024;     // units a wave takes at a time: 64 lanes x 16
constexpr uint32_t kSummaryMaxBlocks = 2048; // workgroups of four waves

// bit i = byte i of w equals the byte c4 repeats four times
__device__ __forceinline__ uint32_t eq_bytes(uint32_t w, uint32_t c4)
{
    const uint32_t x = w ^ c4;
    const uint32_t t = ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu); // 0x80 in every byte that is zero
    return ((t >> 7) * 0x01020408u) >> 24;                                    // bits 0, 8, 16, 24 -> bits 0 .. 3
}
__device__ __forceinline__ uint32_t eq_block(const uint4 &v, uint32_t c)
{
    const uint32_t c4 = c * 0x01010101u;
    return eq_bytes(v.x, c4) | (eq_bytes(v.y, c4) << 4) | (eq_bytes(v.z, c4) << 8) | (eq_bytes(v.w, c4) << 12);
}

// the units [lo, hi) of a lane's 16 as a mask: SH bits a unit (1: bytes, 2: words), the unit's lowest bit set
template <uint32_t SH> __device__ __forceinline__ uint32_t unit_range(uint32_t lo, uint32_t hi)
{
    constexpr uint32_t full = SH == 1u ? 0xFFFFu : 0x55555555u;
    if (lo >= hi || lo >= 16u) return 0u;
    const uint32_t below_hi = hi >= 16u ? 0xFFFFFFFFu : (1u << (SH * hi)) - 1u;
    return below_hi & ~((1u << (SH * lo)) - 1u) & full;
}

struct SummaryArgs {
    const uint8_t *blocks;   // bytes: the 16-byte aligned address at or below the first character
    uint32_t shift;          // bytes: characters start that many bytes behind `blocks` (0 .. 15)
    const uint32_t *words;   // words: the character words
    const uint32_t *data, *sums; // words: the scanned words-per-sequence (launch_packed_prefix)
    const uint64_t *off;     // n_seqs + 1 offsets, in bases
    uint32_t n_seqs;
    uint4 *out;              // n_seqs records, zeroed
};

// where sequence s begins on the unit axis, and its length
template <bool WORDS> __device__ __forceinline__ uint64_t seq_begin(const SummaryArgs &a, uint32_t s)
{
    if (WORDS) return 16ull * (a.sums[s / kScanBlock] + a.data[s]);
    return a.off[s] + a.shift;
}

template <bool WORDS> __global__ __launch_bounds__(256) void summary_kernel(SummaryArgs a)
{
    constexpr uint32_t SH = WORDS ? 2u : 1u;
    const uint32_t lane = threadIdx.x & 63u, n = a.n_seqs;
    const uint64_t n_units = seq_begin<WORDS>(a, n); // (words: every word of the batch; bytes: up to the last character)
    const uint64_t first_unit = seq_begin<WORDS>(a, 0u); // (bytes with d_off[0] != 0: nothing in front of the first character is read)
    const uint64_t n_tiles = (n_units + kSummaryTile - 1u) / kSummaryTile;
    const uint64_t n_waves = (uint64_t)gridDim.x * (blockDim.x >> 6), wave = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const uint64_t per = (n_tiles + n_waves - 1u) / n_waves;
    const uint64_t t0 = min(wave * per, n_tiles), t1 = min(t0 + per, n_tiles);
    if (t0 >= t1) return;
    const uint64_t R0 = t0 * kSummaryTile, R1 = t1 * kSummaryTile; // this wave's units

    // the last sequence that begins at or in front of R0 (the first one when none does): 64 probes a round
    uint32_t s_lo = 0, s_hi = n;
    while (s_hi - s_lo > 1u) {
        const uint32_t step = (s_hi - s_lo + 63u) / 64u, p = s_lo + lane * step;
        const uint32_t c = (uint32_t)__popcll(__ballot(p < s_hi && seq_begin<WORDS>(a, p) <= R0)); // (the begins ascend)
        if (c == 0u) break;
        s_lo += (c - 1u) * step;
        s_hi = min(s_hi, s_lo + step);
    }

    // the window: lane j holds the begin, the length and the record of sequence s_base + j
    uint32_t s_base = s_lo, j = 0;
    uint64_t bb = 0;
    uint32_t ll = 0;
    uint4 rec = make_uint4(0, 0, 0, 0);
    auto load_window = [&]() {
        const uint32_t s = s_base + lane;
        bb = ~0ull;
        ll = 0u;
        if (s < n) {
            bb = seq_begin<WORDS>(a, s);
            ll = (uint32_t)min(a.off[s + 1u] - a.off[s], (uint64_t)0xFFFFFFFFu);
        }
        rec = make_uint4(0, 0, 0, 0);
    };
    auto flush_window = [&]() { // a sequence inside this wave's units is stored; one shared with another wave is added to
        const uint32_t s = s_base + lane;
        if (s >= n || (rec.x | rec.y | rec.z | rec.w) == 0u) return; // (the records start as zeros)
        if (bb >= R0 && bb + ll <= R1) {
            a.out[s] = rec;
        } else {
            uint32_t *o = reinterpret_cast<uint32_t *>(a.out + s);
            if (rec.x) atomicAdd(o + 0, rec.x);
            if (rec.y) atomicAdd(o + 1, rec.y);
            if (rec.z) atomicAdd(o + 2, rec.z);
            if (rec.w) atomicAdd(o + 3, rec.w);
        }
    };
    load_window();

    for (uint64_t t = t0; t < t1; t++) {
        const uint64_t T0 = t * kSummaryTile, T1 = T0 + kSummaryTile;
        // ---- classify: one block / word a lane
        uint32_t mM, mX, mR, nd, prev; // prev: the character in front of the lane's units is not a '-' (bit 0)
        if (WORDS) {
            const uint64_t w = T0 / 16u + lane;
            const uint32_t v = 16u * w < n_units ? a.words[w] : 0u;
            const uint32_t lo = v & 0x55555555u, hi = (v >> 1) & 0x55555555u;
            mM = ~(lo | hi) & 0x55555555u;
            mX = hi & ~lo;
            mR = hi & lo;
            nd = ~(lo & ~hi) & 0x55555555u;
            prev = __shfl_up(nd, 1) >> 30;
            if (lane == 0u) prev = t > 0u ? (((a.words[w - 1u] >> 30) != 1u) ? 1u : 0u) : 0u;
        } else {
            const uint64_t b = T0 + 16u * lane;
            uint4 v = make_uint4(0, 0, 0, 0);
            // (an aligned block that holds a character lies in memory that is there: it shares its 16 bytes with that character)
            if (b < n_units && b + 16u > first_unit) v = *reinterpret_cast<const uint4 *>(a.blocks + b);
            mM = eq_block(v, 'M');
            mX = eq_block(v, 'X');
            mR = eq_block(v, 'R');
            nd = ~eq_block(v, '-') & 0xFFFFu;
            prev = __shfl_up(nd, 1) >> 15;
            if (lane == 0u) prev = (t > 0u && T0 > first_unit) ? (a.blocks[T0 - 1u] != (uint8_t)'-' ? 1u : 0u) : 0u; // (a character of the batch - or no sequence reaches back to it)
        }
        const uint32_t inner_starts = nd & ~((nd << SH) | prev);
        // ---- the sequences that meet the tile
        while (s_base + j < n) {
            const uint32_t b_lo = __shfl((uint32_t)bb, (int)j), b_hi = __shfl((uint32_t)(bb >> 32), (int)j), len = __shfl(ll, (int)j);
            const uint64_t b = ((uint64_t)b_hi << 32) | b_lo, e = b + len;
            if (b >= T1) break;
            if (e > T0 && len >= 3u) {
                const uint32_t r0 = b > T0 ? (uint32_t)(b - T0) : 0u, r1 = e < T1 ? (uint32_t)(e - T0) : kSummaryTile; // inside the tile
                const uint32_t mine = 16u * lane;
                const uint32_t m = unit_range<SH>(r0 > mine ? r0 - mine : 0u, r1 > mine ? min(r1 - mine, 16u) : 0u);
                // the sequence's head starts a run when it is not a '-', whatever stands in front of it
                const uint32_t head = (b >= T0 && r0 >= mine && r0 < mine + 16u) ? (1u << (SH * (r0 - mine))) : 0u;
                const uint32_t starts = (inner_starts | (nd & head)) & m;
                uint32_t pa = (uint32_t)__popc(mM & m) | ((uint32_t)__popc(mX & m) << 16);
                uint32_t pb = (uint32_t)__popc(mR & m) | ((uint32_t)__popc(starts) << 16);
                pa = wave_sum(pa);
                pb = wave_sum(pb);
                if (lane == j) {
                    rec.x += pa & 0xFFFFu;
                    rec.y += pa >> 16;
                    rec.z += pb & 0xFFFFu;
                    rec.w += pb >> 16;
                }
            }
            if (e > T1) break; // (it goes on in the next tile)
            if (++j == 64u) {
                flush_window();
                s_base += 64u;
                j = 0;
                load_window();
            }
        }
    }
    flush_window();
}

uint32_t summary_blocks(uint64_t units_bound)
{
    const uint64_t per_block = 4ull * kSummaryTile;
    if (units_bound == 0 || units_bound >= (uint64_t)kSummaryMaxBlocks * per_block) return kSummaryMaxBlocks;
    return (uint32_t)((units_bound + per_block - 1u) / per_block);
}

} // namespace

hipError_t launch_summary_bytes(const uint8_t *d_chars, const uint64_t *d_off, uint32_t n_seqs, uint64_t bases_bound, uint4 *d_out,
                                hipStream_t stream)
{
    if (n_seqs == 0) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(d_out, 0, (size_t)n_seqs * sizeof(uint4), stream);
    if (e != hipSuccess) return e;
    SummaryArgs a{};
    a.shift = (uint32_t)(reinterpret_cast<uintptr_t>(d_chars) & 15u);
    a.blocks = d_chars - a.shift;
    a.off = d_off;
    a.n_seqs = n_seqs;
    a.out = d_out;
    hipLaunchKernelGGL(summary_kernel<false>, dim3(summary_blocks(bases_bound ? bases_bound + 16u : 0u)), dim3(256), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_summary_words(const uint32_t *d_words, const uint64_t *d_off, uint32_t n_seqs, const uint32_t *d_prefix, uint64_t bases_bound,
                                uint4 *d_out, hipStream_t stream)
{
    if (n_seqs == 0) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(d_out, 0, (size_t)n_seqs * sizeof(uint4), stream);
    if (e != hipSuccess) return e;
    SummaryArgs a{};
    a.words = d_words;
    a.data = d_prefix;
    a.sums = d_prefix + n_seqs + 1u;
    a.off = d_off;
    a.n_seqs = n_seqs;
    a.out = d_out;
    // (every sequence's last word is padded to 16 units)
    hipLaunchKernelGGL(summary_kernel<true>, dim3(summary_blocks(bases_bound ? bases_bound + 16ull * n_seqs : 0u)), dim3(256), 0, stream, a);
    return hipGetLastError();
}

} // namespace kbo
