// derand_seq_kernels.hip — gfx950 (MI355X, CDNA4): derandomize_ms_vec (derandomize.rs:269-288) fused with translate_ms_vec
// (translate.rs:263-293) and, optionally, format::relative_to_ref (format.rs:266-287) over a whole batch in which every sequence
// has a threshold of its own and any length.  The segmented form of derand_kernels.hip's table scan (its dl_* kernels have the
// algebra): the recurrence x[i] = f(noisy[i], x[i+1]) looks at x only through the state  S(x) = x > t ? x - t : 0, and a stretch
// of positions is a table  state -> fired ? exact x_out : "x_in - length"  that composes exactly.
//   ds_count_kernel         chunks and groups of every sequence (then two scans)
//   ds_desc_kernel          one descriptor per chunk and per group slot; neither ever spans two sequences
//   ds_chunk_tables_kernel  lane = (chunk, state): the chunk's table; 64 chunks of a workgroup staged in LDS once
//   ds_group_tables_kernel  lane = (group, state): the tables of the group's chunks composed
//   ds_top_kernel           lane = sequence: the exact value entering each of its groups
//   ds_chunk_inputs_kernel  lane = group: the exact value entering each of its chunks
//   ds_emit_kernel          lane = chunk, staged in LDS: characters, moved out in 16-byte blocks
// Eleven launches whatever the batch holds, nothing read back.  Integer / byte work only.  Wavefront = 64 lanes.
// The summary form (kbo_hip.h kbo_aln_extent: counts, runs and extent per sequence instead of characters) shares every pass up to
// ds_chunk_inputs_kernel and ends differently - thirteen launches:
//   ds_extent_init_kernel   lane = sequence: its record as the atomics expect it
//   ds_count_chars_kernel   lane = chunk, staged in LDS: the characters are counted where ds_emit_kernel packs them and never leave
//                           the lane; the lanes of a wave that sit on one sequence are summed, then added to its record
//   ds_extent_finish_kernel lane = sequence: start of a sequence without a hit
#include "device_util.hpp"

#include <algorithm>

namespace kbo {
namespace {

constexpr uint32_t kC = kDerandSeqChunk, kGC = kDerandSeqGroupChunks;
constexpr int32_t kPass = (int32_t)0x80000000; // table value: "not fired, x_out = x_in - length"
constexpr uint32_t kRows = 64;                 // chunks a workgroup stages
// LDS words per staged chunk: 33, so that the rows of consecutive chunks start one bank apart.  Lanes that sit on different chunks
// read the same position of their rows in the same step: with 32 words a row they would all hit one bank (derand_kernels.hip
// measured 0.67 ms against 0.44 ms for that with its pieces)
constexpr uint32_t kRowWords = kC / 4u + 1u;

// chunk descriptor { first byte in the batch, first position in its sequence, the sequence's length (0: empty slot), threshold }
// group descriptor { first chunk, chunks (0: empty slot), positions of its last chunk, threshold }
__device__ __forceinline__ uint32_t chunk_len(const uint4 &d) { return min(d.z - d.y, kC); }
__device__ __forceinline__ uint32_t group_span(const uint4 &g) { return (g.y - 1u) * kC + g.z; }
__device__ __forceinline__ uint32_t ds_state(int x, int T, uint32_t stride)
{ // (the clamp: thresholds and MS bytes outside their ranges give unspecified characters, never an index outside the tables)
    return x > T ? min((uint32_t)(x - T), stride - 1u) : 0u;
}
__device__ __forceinline__ int ds_apply(int32_t e, int x_in, uint32_t span) { return e == kPass ? x_in - (int)span : e; }
__device__ __forceinline__ int ds_step(int a, int x, int K, int T) { return (a == K) ? K : ((a > T && x < a) ? a : x - 1); }

__global__ void ds_count_kernel(const uint64_t *__restrict__ off, uint32_t n_seqs, uint32_t *__restrict__ cc, uint32_t *__restrict__ gc)
{
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s > n_seqs) return;
    uint32_t nc = 0;
    if (s < n_seqs) {
        const uint64_t len = off[s + 1] - off[s];
        if (len >= 3) nc = (uint32_t)((len + kC - 1u) / kC); // shorter ones are skipped (derandomize.rs:276)
    }
    cc[s] = nc;
    gc[s] = (nc + kGC - 1u) / kGC;
}

// largest s with first(s) <= t, first = the scanned counts (sequences without chunks own no slot)
__device__ __forceinline__ uint32_t ds_owner(const uint32_t *local, const uint32_t *sums, uint32_t n_seqs, uint32_t t)
{
    uint32_t lo = 0, hi = n_seqs;
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (sums[mid / kScanBlock] + local[mid] <= t) lo = mid;
        else hi = mid;
    }
    return lo;
}

__global__ void ds_desc_kernel(const uint64_t *__restrict__ off, const uint32_t *__restrict__ thr, uint32_t n_seqs, uint32_t k, uint32_t min_thr,
                               const uint32_t *__restrict__ cc, const uint32_t *__restrict__ csums, const uint32_t *__restrict__ gc,
                               const uint32_t *__restrict__ gsums, uint32_t n_cslots, uint32_t n_gslots, uint4 *__restrict__ cdesc,
                               uint4 *__restrict__ gdesc)
{
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_cslots + n_gslots) return;
    auto cfirst = [&](uint32_t s) { return csums[s / kScanBlock] + cc[s]; };
    auto gfirst = [&](uint32_t s) { return gsums[s / kScanBlock] + gc[s]; };
    uint4 d = make_uint4(0, 0, 0, 0);
    if (t < n_cslots) {
        if (t < cfirst(n_seqs)) {
            const uint32_t s = ds_owner(cc, csums, n_seqs, t);
            const uint64_t b = off[s];
            const uint32_t p0 = (t - cfirst(s)) * kC;
            d = make_uint4((uint32_t)(b + p0), p0, (uint32_t)(off[s + 1] - b), min(max(thr[s], min_thr), k));
        }
        cdesc[t] = d;
    } else {
        const uint32_t g = t - n_cslots;
        if (g < gfirst(n_seqs)) {
            const uint32_t s = ds_owner(gc, gsums, n_seqs, g);
            const uint32_t len = (uint32_t)(off[s + 1] - off[s]);
            const uint32_t c0 = (g - gfirst(s)) * kGC, nc = min(kGC, cfirst(s + 1) - cfirst(s) - c0);
            d = make_uint4(cfirst(s) + c0, nc, min(len - (c0 + nc - 1u) * kC, kC), min(max(thr[s], min_thr), k));
        }
        gdesc[g] = d;
    }
}

// the MS bytes of kRows consecutive chunks into LDS, 16 bytes a lane and step: eight lanes take one chunk (a block is loaded when
// it holds a byte of the chunk, so nothing further than 15 bytes behind a sequence is read: the batch's slack)
__device__ __forceinline__ void ds_stage(const uint8_t *__restrict__ ms, const uint32_t *sh_start, const uint32_t *sh_len, uint32_t *rows)
{
    for (uint32_t id = threadIdx.x; id < kRows * (kC / 16u); id += blockDim.x) {
        const uint32_t i = id / (kC / 16u), j = id % (kC / 16u);
        if (16u * j < sh_len[i]) {
            const uint4 v = ld16u(ms + sh_start[i], 16u * j);
            uint32_t *d = rows + i * kRowWords + 4u * j;
            d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
        }
    }
}

// lane = (chunk, state).  The recurrence runs once per state over bytes that are the same for all states of a chunk: they are
// staged once, and the lanes of a wave that share a chunk read the same LDS word (a broadcast)
__global__ __launch_bounds__(256) void ds_chunk_tables_kernel(const uint8_t *__restrict__ ms, const uint4 *__restrict__ cdesc, uint32_t n_cslots,
                                                              uint32_t k, uint32_t stride, int32_t *__restrict__ t1)
{
    __shared__ uint32_t rows[kRows * kRowWords];
    __shared__ uint32_t sh_start[kRows], sh_len[kRows], sh_thr[kRows], sh_last[kRows]; // sh_last: the sequence ends in the chunk
    const uint32_t c0 = blockIdx.x * kRows;
    if (threadIdx.x < kRows) {
        uint4 d = make_uint4(0, 0, 0, 0);
        if (c0 + threadIdx.x < n_cslots) d = cdesc[c0 + threadIdx.x];
        const uint32_t cl = d.z ? chunk_len(d) : 0u;
        sh_start[threadIdx.x] = d.x;
        sh_len[threadIdx.x] = cl;
        sh_thr[threadIdx.x] = d.w;
        sh_last[threadIdx.x] = d.y + cl == d.z;
    }
    __syncthreads();
    ds_stage(ms, sh_start, sh_len, rows);
    __syncthreads();
    const int K = (int)k;
    for (uint32_t id = threadIdx.x; id < kRows * stride; id += blockDim.x) {
        const uint32_t i = id / stride, st = id - i * stride;
        const uint32_t cl = sh_len[i];
        const int T = (int)sh_thr[i];
        if (!cl || st > k - (uint32_t)T) continue; // an empty slot; a state this sequence's threshold does not have
        const uint32_t *row = rows + i * kRowWords;
        int x = T + (int)st; // representative of the state (st == 0: any value <= t)
        bool fired = false;
        uint32_t n = cl; // positions [0, n) take the general rule
        if (sh_last[i]) { // the sequence's last position (derandomize.rs:282)
            n = cl - 1u;
            const int a = (int)((row[n >> 2] >> (8u * (n & 3u))) & 0xFFu);
            x = a > T ? a : 0;
            fired = true;
        }
        for (uint32_t w = (n + 3u) >> 2; w-- > 0;) {
            const uint32_t v = row[w];
#pragma unroll
            for (int j = 3; j >= 0; j--) {
                if (4u * w + (uint32_t)j < n) {
                    const int a = (int)((v >> (8 * j)) & 0xFFu);
                    const bool hit = a == K || (a > T && x < a);
                    x = hit ? a : x - 1;
                    fired = fired || hit;
                }
            }
        }
        t1[(size_t)(c0 + i) * stride + st] = fired ? x : kPass;
    }
}

// lane = (group, state): the chunk tables of the group composed, right to left
__global__ void ds_group_tables_kernel(const int32_t *__restrict__ t1, const uint4 *__restrict__ gdesc, uint32_t n_gslots, uint32_t k,
                                       uint32_t stride, int32_t *__restrict__ t2)
{
    const uint64_t id = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= (uint64_t)n_gslots * stride) return;
    const uint32_t g = (uint32_t)(id / stride), st = (uint32_t)(id - (uint64_t)g * stride);
    const uint4 gd = gdesc[g];
    const int T = (int)gd.w;
    if (!gd.y || st > k - gd.w) return;
    int x = T + (int)st;
    bool fired = false;
    for (uint32_t c = gd.x + gd.y; c-- > gd.x;) {
        const int32_t e = t1[(size_t)c * stride + ds_state(x, T, stride)];
        fired = fired || e != kPass;
        x = ds_apply(e, x, c == gd.x + gd.y - 1u ? gd.z : kC);
    }
    t2[id] = fired ? x : kPass;
}

// lane = sequence: the exact x entering every one of its groups (from the right)
__global__ void ds_top_kernel(const int32_t *__restrict__ t2, const uint4 *__restrict__ gdesc, const uint32_t *__restrict__ gc,
                              const uint32_t *__restrict__ gsums, uint32_t n_seqs, uint32_t stride, int32_t *__restrict__ g_in)
{
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_seqs) return;
    const uint32_t g0 = gsums[s / kScanBlock] + gc[s], g1 = gsums[(s + 1u) / kScanBlock] + gc[s + 1u];
    int x = 0; // irrelevant: the last position's rule ignores it
    for (uint32_t g = g1; g-- > g0;) {
        const uint4 gd = gdesc[g];
        g_in[g] = x;
        x = ds_apply(t2[(size_t)g * stride + ds_state(x, (int)gd.w, stride)], x, group_span(gd));
    }
}

// lane = group: the exact x entering every chunk of the group
__global__ void ds_chunk_inputs_kernel(const int32_t *__restrict__ t1, const int32_t *__restrict__ g_in, const uint4 *__restrict__ gdesc,
                                       uint32_t n_gslots, uint32_t stride, int32_t *__restrict__ c_in)
{
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n_gslots) return;
    const uint4 gd = gdesc[g];
    if (!gd.y) return;
    const int T = (int)gd.w;
    int x = g_in[g];
    for (uint32_t c = gd.x + gd.y; c-- > gd.x;) {
        c_in[c] = x;
        x = ds_apply(t1[(size_t)c * stride + ds_state(x, T, stride)], x, c == gd.x + gd.y - 1u ? gd.z : kC);
    }
}

// lane = chunk: the final pass with the exact incoming value.  A wave stages its 64 chunks in LDS, every lane overwrites its row in
// place (four MS bytes in, four characters out a step) and the wave moves the rows out, 16 bytes a lane and step, applying
// format::relative_to_ref on the way when a reference is given
__global__ __launch_bounds__(64) void ds_emit_kernel(const uint8_t *__restrict__ ms, const uint4 *__restrict__ cdesc, const int32_t *__restrict__ c_in,
                                                     uint32_t n_cslots, uint32_t k, const uint8_t *__restrict__ ref, uint8_t *__restrict__ out)
{
    __shared__ uint32_t rows[kRows * kRowWords];
    __shared__ uint32_t sh_start[kRows], sh_len[kRows];
    const uint32_t c = blockIdx.x * kRows + threadIdx.x;
    uint4 d = make_uint4(0, 0, 0, 0);
    if (c < n_cslots) d = cdesc[c];
    const uint32_t cl = d.z ? chunk_len(d) : 0u;
    sh_start[threadIdx.x] = d.x;
    sh_len[threadIdx.x] = cl;
    __syncthreads();
    ds_stage(ms, sh_start, sh_len, rows);
    __syncthreads();
    if (cl) {
        const int K = (int)k, T = (int)d.w;
        const uint32_t len = d.z, p0 = d.y, p1 = p0 + cl;
        uint32_t *row = rows + threadIdx.x * kRowWords;
        const uint32_t a_under = p0 > 0 ? (uint32_t)ms[d.x - 1u] : 0u; // the MS byte below the chunk: the same sequence's
        const int a_top = (int)((row[(cl - 1u) >> 2] >> (8u * ((cl - 1u) & 3u))) & 0xFFu);
        int x_next = c_in[c], x_cur; // x[p1] (unused when the sequence ends here), x[p1 - 1]
        if (p1 == len) {             // derandomize.rs:282
            x_cur = a_top > T ? a_top : 0;
            x_next = x_cur;
        } else x_cur = ds_step(a_top, x_next, K, T);
        uint32_t v = row[(cl - 1u) >> 2];
        for (uint32_t w = (cl + 3u) >> 2; w-- > 0;) {
            const uint32_t below = w > 0 ? row[w - 1u] : a_under << 24;
            uint32_t o = 0;
#pragma unroll
            for (int j = 3; j >= 0; j--) {
                const uint32_t q = 4u * w + (uint32_t)j;
                if (q < cl) {
                    const int a = (int)((j > 0 ? v >> (8 * (j - 1)) : below >> 24) & 0xFFu); // noisy[p - 1]
                    const int x_prev = p0 + q > 0 ? ds_step(a, x_cur, K, T) : K;
                    o |= translate_char(x_prev, x_cur, x_next, p0 + q, len, K, T) << (8 * j);
                    x_next = x_cur;
                    x_cur = x_prev;
                }
            }
            row[w] = o;
            v = below;
        }
    }
    __syncthreads();
    for (uint32_t id = threadIdx.x; id < kRows * (kC / 16u); id += blockDim.x) {
        const uint32_t i = id / (kC / 16u), j = id % (kC / 16u), n = sh_len[i];
        if (16u * j >= n) continue;
        const uint32_t *r = rows + i * kRowWords + 4u * j;
        uint4 ch = make_uint4(r[0], r[1], r[2], r[3]);
        if (ref) {
            const uint4 rf = ld16u(ref + sh_start[i], 16u * j);
            ch.x = fmt_word(ch.x, rf.x);
            ch.y = fmt_word(ch.y, rf.y);
            ch.z = fmt_word(ch.z, rf.z);
            ch.w = fmt_word(ch.w, rf.w);
        }
        if (16u * j + 16u <= n) st16u(out + sh_start[i], 16u * j, ch);
        else st_partial(out + sh_start[i] + 16u * j, ch, n - 16u * j);
    }
}

// the summary form's record: kbo_aln_extent as six words; while the chunks arrive `start` is a minimum over 0xFFFFFFFF
constexpr uint32_t kExtentWords = 6;
constexpr uint32_t kNoStart = 0xFFFFFFFFu;

__global__ void ds_extent_init_kernel(uint32_t n_seqs, uint32_t *__restrict__ out)
{
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_seqs) return;
    uint32_t *o = out + (size_t)s * kExtentWords;
    o[0] = 0; o[1] = 0; o[2] = 0; o[3] = 0; o[4] = kNoStart; o[5] = 0;
}

__global__ void ds_extent_finish_kernel(uint32_t n_seqs, uint32_t *__restrict__ out)
{
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_seqs) return;
    uint32_t *o = out + (size_t)s * kExtentWords;
    if (o[4] == kNoStart) o[4] = 0; // no character other than '-': start = end = 0
}

// lane = chunk: ds_emit_kernel's pass with the characters counted instead of packed.  A run is counted where it STARTS - a
// character other than '-' at the head of the sequence or behind a '-' - so one that crosses a chunk, a wave's 64 chunks or a group
// is counted once: the character in front of the chunk is another lane's, and the lane makes that one character itself from
// x[p0 - 2 .. p0] (one more step of the recurrence with the MS byte at p0 - 2).  The chunks of a sequence are consecutive slots, so
// the lanes of a wave that share an owner are neighbours: a segmented sum over the wave, then the segment's first lane adds to the
// record (integers: any order gives the same record).  Nothing is written to LDS behind the staging and no character exists in memory.
__global__ __launch_bounds__(64) void ds_count_chars_kernel(const uint8_t *__restrict__ ms, const uint4 *__restrict__ cdesc,
                                                            const int32_t *__restrict__ c_in, uint32_t n_cslots, uint32_t k,
                                                            const uint32_t *__restrict__ cc, const uint32_t *__restrict__ csums,
                                                            uint32_t n_seqs, uint32_t *__restrict__ out)
{
    __shared__ uint32_t rows[kRows * kRowWords];
    __shared__ uint32_t sh_start[kRows], sh_len[kRows];
    const uint32_t lane = threadIdx.x, c = blockIdx.x * kRows + lane;
    uint4 d = make_uint4(0, 0, 0, 0);
    if (c < n_cslots) d = cdesc[c];
    const uint32_t cl = d.z ? chunk_len(d) : 0u;
    sh_start[lane] = d.x;
    sh_len[lane] = cl;
    __syncthreads();
    ds_stage(ms, sh_start, sh_len, rows);
    __syncthreads();
    // per chunk at most 128 of anything: 'M's, 'X's, 'R's and run starts in the four bytes of one word
    uint32_t cnt = 0, first = kNoStart, last = 0; // first / last: positions in the sequence; last is one past
    if (cl) {
        const int K = (int)k, T = (int)d.w;
        const uint32_t len = d.z, p0 = d.y, p1 = p0 + cl;
        const uint32_t *row = rows + lane * kRowWords;
        const uint32_t a_under = p0 > 0 ? (uint32_t)ms[d.x - 1u] : 0u; // the MS bytes below the chunk: the same sequence's
        const uint32_t a_under2 = p0 > 0 ? (uint32_t)ms[d.x - 2u] : 0u; // (p0 > 0: p0 >= kC)
        const int a_top = (int)((row[(cl - 1u) >> 2] >> (8u * ((cl - 1u) & 3u))) & 0xFFu);
        int x_next = c_in[c], x_cur;
        if (p1 == len) { // derandomize.rs:282
            x_cur = a_top > T ? a_top : 0;
            x_next = x_cur;
        } else x_cur = ds_step(a_top, x_next, K, T);
        uint32_t v = row[(cl - 1u) >> 2];
        bool above = false; // the character one position up is not a '-'
        for (uint32_t w = (cl + 3u) >> 2; w-- > 0;) {
            const uint32_t below = w > 0 ? row[w - 1u] : a_under << 24;
#pragma unroll
            for (int j = 3; j >= 0; j--) {
                const uint32_t q = 4u * w + (uint32_t)j;
                if (q < cl) {
                    const int a = (int)((j > 0 ? v >> (8 * (j - 1)) : below >> 24) & 0xFFu); // noisy[p - 1]
                    const int x_prev = p0 + q > 0 ? ds_step(a, x_cur, K, T) : K;
                    const uint32_t ch = translate_char(x_prev, x_cur, x_next, p0 + q, len, K, T);
                    const bool hit = ch != (uint32_t)'-';
                    cnt += (ch == (uint32_t)'M' ? 1u : 0u) + (ch == (uint32_t)'X' ? 1u << 8 : 0u) + (ch == (uint32_t)'R' ? 1u << 16 : 0u) +
                           (above && !hit ? 1u << 24 : 0u); // a run starts one position up
                    if (hit) {
                        first = p0 + q;
                        if (!last) last = p0 + q + 1u;
                    }
                    above = hit;
                    x_next = x_cur;
                    x_cur = x_prev;
                }
            }
            v = below;
        }
        // the chunk's first position: x_cur = x[p0 - 1], x_next = x[p0]
        bool front = false; // the character in front of the chunk is not a '-'
        if (p0 > 0) {
            const int x_pp = ds_step((int)a_under2, x_cur, K, T); // x[p0 - 2]
            front = translate_char(x_pp, x_cur, x_next, p0 - 1u, len, K, T) != (uint32_t)'-';
        }
        if (above && !front) cnt += 1u << 24;
    }
    // the owner: a search per first chunk of a sequence (and per wave), handed on to the lanes behind it
    const bool head = cl && (lane == 0u || d.y == 0u);
    uint32_t own = head ? ds_owner(cc, csums, n_seqs, c) : 0u;
    const uint64_t heads = __ballot(head);
    own = __shfl(own, cl ? 63 - __clzll(heads & (~0ull >> (63u - lane))) : (int)lane);
    if (!cl) own = kNoStart; // (empty slots: behind every chunk of the batch)
    uint32_t pa = (cnt & 0xFFu) | ((cnt >> 8 & 0xFFu) << 16), pb = (cnt >> 16 & 0xFFu) | ((cnt >> 24) << 16); // a wave: at most 8 192 of each
#pragma unroll
    for (uint32_t step = 1; step < 64u; step <<= 1) {
        const uint32_t o2 = __shfl_down(own, step), a2 = __shfl_down(pa, step), b2 = __shfl_down(pb, step);
        const uint32_t f2 = __shfl_down(first, step), l2 = __shfl_down(last, step);
        if (lane + step < 64u && o2 == own) {
            pa += a2;
            pb += b2;
            first = min(first, f2);
            last = max(last, l2);
        }
    }
    if (head && last) { // (a hit: at least one character other than '-', so first and last are set)
        uint32_t *o = out + (size_t)own * kExtentWords;
        if (pa & 0xFFFFu) atomicAdd(o + 0, pa & 0xFFFFu);
        if (pa >> 16) atomicAdd(o + 1, pa >> 16);
        if (pb & 0xFFFFu) atomicAdd(o + 2, pb & 0xFFFFu);
        if (pb >> 16) atomicAdd(o + 3, pb >> 16);
        atomicMin(o + 4, first);
        atomicMax(o + 5, last);
    }
}

struct SeqLayout {
    uint32_t n_cslots, n_gslots, stride;
    size_t cc, gc, cdesc, gdesc, t1, t2, g_in, c_in, end;
};
SeqLayout seq_layout(uint32_t n_seqs, uint64_t total_bases, uint32_t k, uint32_t min_thr)
{
    SeqLayout L;
    const uint64_t nc = total_bases / kC + n_seqs, ng = nc / kGC + n_seqs + 1u;
    L.n_cslots = (uint32_t)std::min<uint64_t>(nc, 0xFFFFFFFFu);
    L.n_gslots = (uint32_t)std::min<uint64_t>(ng, 0xFFFFFFFFu);
    L.stride = (k > min_thr ? k - min_thr : 0u) + 1u;
    auto up = [](size_t b) { return (b + 15) / 16 * 16; };
    const size_t scan = up(chunk_items_scratch_words(n_seqs) * sizeof(uint32_t));
    size_t w = 0;
    L.cc = w;    w += scan;
    L.gc = w;    w += scan;
    L.cdesc = w; w += (size_t)nc * sizeof(uint4);
    L.gdesc = w; w += (size_t)ng * sizeof(uint4);
    L.t1 = w;    w += up((size_t)nc * L.stride * sizeof(int32_t));
    L.t2 = w;    w += up((size_t)ng * L.stride * sizeof(int32_t));
    L.g_in = w;  w += up((size_t)ng * sizeof(int32_t));
    L.c_in = w;  w += up((size_t)nc * sizeof(int32_t));
    L.end = w;
    return L;
}

} // namespace

size_t derand_seq_work_bytes(uint32_t n_seqs, uint64_t total_bases, uint32_t k, uint32_t min_threshold)
{
    return seq_layout(n_seqs, total_bases, k, min_threshold).end;
}

namespace {

struct SeqWork {
    SeqLayout L;
    uint32_t *cc, *csums;
    uint4 *cdesc;
    int32_t *c_in;
    dim3 chunk_groups;
};

// the ten launches both forms share: everything up to the exact value entering every chunk
hipError_t enqueue_chunk_inputs(const uint8_t *d_ms, const uint64_t *d_offsets, uint32_t n_seqs, uint64_t total_bases, uint32_t k,
                                const uint32_t *d_thresholds, uint32_t min_threshold, void *d_work, hipStream_t stream, SeqWork &W)
{
    const SeqLayout L = seq_layout(n_seqs, total_bases, k, min_threshold);
    if ((uint64_t)L.n_cslots + L.n_gslots > 0xFFFFFFFFull) return hipErrorInvalidValue; // (n_seqs < 2^31: the callers check)
    uint8_t *w = static_cast<uint8_t *>(d_work);
    const uint32_t n = n_seqs + 1u;
    uint32_t *cc = reinterpret_cast<uint32_t *>(w + L.cc), *csums = cc + n;
    uint32_t *gc = reinterpret_cast<uint32_t *>(w + L.gc), *gsums = gc + n;
    uint4 *cdesc = reinterpret_cast<uint4 *>(w + L.cdesc), *gdesc = reinterpret_cast<uint4 *>(w + L.gdesc);
    int32_t *t1 = reinterpret_cast<int32_t *>(w + L.t1), *t2 = reinterpret_cast<int32_t *>(w + L.t2);
    int32_t *g_in = reinterpret_cast<int32_t *>(w + L.g_in), *c_in = reinterpret_cast<int32_t *>(w + L.c_in);
    const uint32_t T = 256;
    auto blocks = [&](uint64_t lanes) { return dim3((unsigned)((lanes + T - 1) / T)); };
    hipLaunchKernelGGL(ds_count_kernel, blocks(n), dim3(T), 0, stream, d_offsets, n_seqs, cc, gc);
    hipError_t e = launch_scan(cc, n, csums, stream);
    if (e != hipSuccess) return e;
    e = launch_scan(gc, n, gsums, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(ds_desc_kernel, blocks((uint64_t)L.n_cslots + L.n_gslots), dim3(T), 0, stream, d_offsets, d_thresholds, n_seqs, k,
                       min_threshold, cc, csums, gc, gsums, L.n_cslots, L.n_gslots, cdesc, gdesc);
    const dim3 chunk_groups((L.n_cslots + kRows - 1u) / kRows);
    hipLaunchKernelGGL(ds_chunk_tables_kernel, chunk_groups, dim3(T), 0, stream, d_ms, cdesc, L.n_cslots, k, L.stride, t1);
    hipLaunchKernelGGL(ds_group_tables_kernel, blocks((uint64_t)L.n_gslots * L.stride), dim3(T), 0, stream, t1, gdesc, L.n_gslots, k, L.stride, t2);
    hipLaunchKernelGGL(ds_top_kernel, blocks(n_seqs), dim3(T), 0, stream, t2, gdesc, gc, gsums, n_seqs, L.stride, g_in);
    hipLaunchKernelGGL(ds_chunk_inputs_kernel, blocks(L.n_gslots), dim3(T), 0, stream, t1, g_in, gdesc, L.n_gslots, L.stride, c_in);
    W = SeqWork{L, cc, csums, cdesc, c_in, chunk_groups};
    return hipGetLastError();
}

} // namespace

hipError_t launch_derand_translate_seq(const uint8_t *d_ms, const uint64_t *d_offsets, uint32_t n_seqs, uint64_t total_bases, uint32_t k,
                                       const uint32_t *d_thresholds, uint32_t min_threshold, const uint8_t *d_ref, uint8_t *d_chars_out,
                                       void *d_work, hipStream_t stream)
{
    if (n_seqs == 0) return hipSuccess;
    SeqWork W;
    const hipError_t e = enqueue_chunk_inputs(d_ms, d_offsets, n_seqs, total_bases, k, d_thresholds, min_threshold, d_work, stream, W);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(ds_emit_kernel, W.chunk_groups, dim3(kRows), 0, stream, d_ms, W.cdesc, W.c_in, W.L.n_cslots, k, d_ref, d_chars_out);
    return hipGetLastError();
}

hipError_t launch_derand_summary_seq(const uint8_t *d_ms, const uint64_t *d_offsets, uint32_t n_seqs, uint64_t total_bases, uint32_t k,
                                     const uint32_t *d_thresholds, uint32_t min_threshold, uint32_t *d_out, void *d_work, hipStream_t stream)
{
    if (n_seqs == 0) return hipSuccess;
    SeqWork W;
    const hipError_t e = enqueue_chunk_inputs(d_ms, d_offsets, n_seqs, total_bases, k, d_thresholds, min_threshold, d_work, stream, W);
    if (e != hipSuccess) return e;
    const dim3 per_seq((n_seqs + 255u) / 256u);
    hipLaunchKernelGGL(ds_extent_init_kernel, per_seq, dim3(256), 0, stream, n_seqs, d_out);
    hipLaunchKernelGGL(ds_count_chars_kernel, W.chunk_groups, dim3(kRows), 0, stream, d_ms, W.cdesc, W.c_in, W.L.n_cslots, k, W.cc, W.csums, n_seqs,
                       d_out);
    hipLaunchKernelGGL(ds_extent_finish_kernel, per_seq, dim3(256), 0, stream, n_seqs, d_out);
    return hipGetLastError();
}

} // namespace kbo
