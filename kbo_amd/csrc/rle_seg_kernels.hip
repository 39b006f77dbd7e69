// rle_seg_kernels.hip — gfx950 (MI355X, CDNA4): format::run_lengths_gapped (format.rs:143-193) over a batch of sequences of any
// length, segmented: no lane steps over more than a chunk of characters or a group's worth of summaries, except the lane that owns
// a sequence, which steps over that sequence's groups.  rle_seg.hpp has the algebra (and rle_seg_host.cpp the same passes on the
// CPU): a '-' decides by its place in its stretch and by the byte in front of the stretch, so two carries run along the chunks of
// a sequence - the dash carry, then, with it known, the record of the run open where a chunk begins - and the number of runs that
// end in a chunk is a plain count once its dash carry is known.
//   rs_list_count_kernel   chunks and groups of every sequence (then two scans)
//   rs_desc_kernel         one descriptor per chunk and per group slot; neither ever spans two sequences
//   rs_dash_kernel         lane = chunk: its dash summary (the '-' at its end)
//   rs_dash_group_kernel   lane = group: the summaries of its chunks combined
//   rs_dash_top_kernel     lane = sequence: the dash carry entering each of its groups
//   rs_dash_in_kernel      lane = group: the dash carry entering each of its chunks
//   rs_walk_kernel<false>  lane = chunk, staged in LDS: runs that end in it, and the run it leaves open
//   rs_part_group_kernel / rs_part_top_kernel / rs_part_in_kernel   the same two levels for the open run
//   (one two-level scan of the chunks' counts: two launches)
//   rs_first_kernel        lane = sequence: the index of its first run = that of its first chunk
//   rs_walk_kernel<true>   lane = chunk, staged in LDS: the records that end in it, 16 + 12 bytes each
// Count: 17 launches (11 kernels + 3 two-level scans of 2); emit: 1; 18 whatever the batch holds, nothing read back.
// Integer / byte work only.  Wavefront = 64 lanes.
#include "device_util.hpp"
#include "rle_seg.hpp"

#include <algorithm>
#include <atomic>

namespace kbo {
namespace {

using namespace rleseg;

constexpr uint32_t kC = kRleSegChunk, kGC = kRleSegGroupChunks;
constexpr uint32_t kRows = 64; // chunks a wave stages
// LDS words per staged chunk: 33, so that the rows of consecutive chunks start one bank apart (the lanes of a wave sit on 64
// chunks and read the same position of their rows in the same step: derand_seq_kernels.hip has the measurement)
constexpr uint32_t kRowWords = kC / 4u + 1u;

// chunk descriptor { first byte in the batch, first position in its sequence, the sequence's length (0: empty slot), 0 }
// group descriptor { first chunk, chunks (0: empty slot), 0, 0 }
__device__ __forceinline__ uint32_t chunk_len(const uint4 &d) { return min(d.z - d.y, kC); }

__global__ void rs_list_count_kernel(const uint64_t *__restrict__ off, uint32_t n_seqs, uint32_t min_len, uint32_t *__restrict__ cc,
                                     uint32_t *__restrict__ gc)
{
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s > n_seqs) return;
    uint32_t nc = 0;
    if (s < n_seqs) {
        const uint64_t len = off[s + 1] - off[s];
        if (len >= min_len) nc = (uint32_t)((len + kC - 1u) / kC); // (shorter ones have no run, whatever stands there)
    }
    cc[s] = nc;
    gc[s] = (nc + kGC - 1u) / kGC;
}

// largest s with first(s) <= t, first = the scanned counts (sequences without chunks own no slot)
__device__ __forceinline__ uint32_t rs_owner(const uint32_t *local, const uint32_t *sums, uint32_t n_seqs, uint32_t t)
{
    uint32_t lo = 0, hi = n_seqs;
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (sums[mid / kScanBlock] + local[mid] <= t) lo = mid;
        else hi = mid;
    }
    return lo;
}

__global__ void rs_desc_kernel(const uint64_t *__restrict__ off, uint32_t n_seqs, const uint32_t *__restrict__ cc,
                               const uint32_t *__restrict__ csums, const uint32_t *__restrict__ gc, const uint32_t *__restrict__ gsums,
                               uint32_t n_cslots, uint32_t n_gslots, uint4 *__restrict__ cdesc, uint4 *__restrict__ gdesc)
{
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_cslots + n_gslots) return;
    auto cfirst = [&](uint32_t s) { return csums[s / kScanBlock] + cc[s]; };
    auto gfirst = [&](uint32_t s) { return gsums[s / kScanBlock] + gc[s]; };
    uint4 d = make_uint4(0, 0, 0, 0);
    if (t < n_cslots) {
        if (t < cfirst(n_seqs)) {
            const uint32_t s = rs_owner(cc, csums, n_seqs, t);
            const uint64_t b = off[s];
            const uint32_t p0 = (t - cfirst(s)) * kC;
            d = make_uint4((uint32_t)(b + p0), p0, (uint32_t)(off[s + 1] - b), 0u);
        }
        cdesc[t] = d;
    } else {
        const uint32_t g = t - n_cslots;
        if (g < gfirst(n_seqs)) {
            const uint32_t s = rs_owner(gc, gsums, n_seqs, g);
            const uint32_t c0 = (g - gfirst(s)) * kGC;
            d = make_uint4(cfirst(s) + c0, min(kGC, cfirst(s + 1) - cfirst(s) - c0), 0u, 0u);
        }
        gdesc[g] = d;
    }
}

// ---- the dash carry
// lane = chunk slot.  The '-' at a chunk's end are few as a rule: read from the end, a byte at a time, no staging.  (The lane
// behind the last slot clears the word the scan of the counts ends on.)
__global__ void rs_dash_kernel(const uint8_t *__restrict__ chars, const uint4 *__restrict__ cdesc, uint32_t n_cslots, Dash *__restrict__ cdash,
                               uint32_t *__restrict__ cnt)
{
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c > n_cslots) return;
    if (c == n_cslots) {
        cnt[c] = 0u;
        return;
    }
    const uint4 d = cdesc[c];
    Dash out = dash_identity();
    if (d.z) {
        const uint8_t *row = chars + d.x;
        out = dash_summary([&](uint32_t q) { return (uint32_t)row[q]; }, chunk_len(d));
    }
    cdash[c] = out;
}

// lane = group: its chunks' summaries combined.  Two levels, the same for both carries (T = Dash / Part)
template <typename T, typename Combine>
__device__ __forceinline__ void rs_group(const T *__restrict__ csum, const uint4 *__restrict__ gdesc, uint32_t n_gslots, T *__restrict__ gsum,
                                         T identity, Combine combine)
{
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n_gslots) return;
    const uint4 gd = gdesc[g];
    T acc = identity;
    for (uint32_t c = gd.x; c < gd.x + gd.y; c++) acc = combine(acc, csum[c]);
    gsum[g] = acc;
}
// lane = sequence: what enters each of its groups, left where the group's summary was
template <typename T, typename Combine>
__device__ __forceinline__ void rs_top(T *__restrict__ gsum, const uint32_t *__restrict__ gc, const uint32_t *__restrict__ gsums, uint32_t n_seqs,
                                       T identity, Combine combine)
{
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_seqs) return;
    const uint32_t g0 = gsums[s / kScanBlock] + gc[s], g1 = gsums[(s + 1u) / kScanBlock] + gc[s + 1u];
    T state = identity;
    for (uint32_t g = g0; g < g1; g++) {
        const T own = gsum[g];
        gsum[g] = state;
        state = combine(state, own);
    }
}
// lane = group: what enters each of its chunks, left where the chunk's summary was
template <typename T, typename Combine>
__device__ __forceinline__ void rs_inputs(T *__restrict__ csum, const T *__restrict__ g_in, const uint4 *__restrict__ gdesc, uint32_t n_gslots,
                                          Combine combine)
{
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n_gslots) return;
    const uint4 gd = gdesc[g];
    if (!gd.y) return;
    T state = g_in[g];
    for (uint32_t c = gd.x; c < gd.x + gd.y; c++) {
        const T own = csum[c];
        csum[c] = state;
        state = combine(state, own);
    }
}
struct DashCombine {
    __device__ __forceinline__ Dash operator()(const Dash &a, const Dash &b) const { return dash_combine(a, b); }
};
struct PartCombine {
    __device__ __forceinline__ Part operator()(const Part &a, const Part &b) const { return part_combine(a, b); }
};

__global__ void rs_dash_group_kernel(const Dash *__restrict__ cdash, const uint4 *__restrict__ gdesc, uint32_t n_gslots, Dash *__restrict__ gdash)
{
    rs_group(cdash, gdesc, n_gslots, gdash, dash_identity(), DashCombine());
}
__global__ void rs_dash_top_kernel(Dash *__restrict__ gdash, const uint32_t *__restrict__ gc, const uint32_t *__restrict__ gsums, uint32_t n_seqs)
{
    rs_top(gdash, gc, gsums, n_seqs, dash_identity(), DashCombine());
}
__global__ void rs_dash_in_kernel(Dash *__restrict__ cdash, const Dash *__restrict__ gdash, const uint4 *__restrict__ gdesc, uint32_t n_gslots)
{
    rs_inputs(cdash, gdash, gdesc, n_gslots, DashCombine());
}
__global__ void rs_part_group_kernel(const Part *__restrict__ cpart, const uint4 *__restrict__ gdesc, uint32_t n_gslots, Part *__restrict__ gpart)
{
    rs_group(cpart, gdesc, n_gslots, gpart, part_identity(), PartCombine());
}
__global__ void rs_part_top_kernel(Part *__restrict__ gpart, const uint32_t *__restrict__ gc, const uint32_t *__restrict__ gsums, uint32_t n_seqs)
{
    rs_top(gpart, gc, gsums, n_seqs, part_identity(), PartCombine());
}
__global__ void rs_part_in_kernel(Part *__restrict__ cpart, const Part *__restrict__ gpart, const uint4 *__restrict__ gdesc, uint32_t n_gslots)
{
    rs_inputs(cpart, gpart, gdesc, n_gslots, PartCombine());
}

// ---- the walk of a chunk
// the characters of kRows consecutive chunks into LDS, 16 bytes a lane and step: eight lanes take one chunk (a block is loaded
// when it holds a byte of the chunk, so nothing further than 15 bytes behind a sequence is read: the batch's slack)
__device__ __forceinline__ void rs_stage(const uint8_t *__restrict__ chars, const uint32_t *sh_start, const uint32_t *sh_len, uint32_t *rows)
{
    for (uint32_t id = threadIdx.x; id < kRows * (kC / 16u); id += blockDim.x) {
        const uint32_t i = id / (kC / 16u), j = id % (kC / 16u);
        if (16u * j < sh_len[i]) {
            const uint4 v = ld16u(chars + sh_start[i], 16u * j);
            uint32_t *d = rows + i * kRowWords + 4u * j;
            d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
        }
    }
}

// lane = chunk: a wave stages its 64 chunks, every lane walks its row, four characters a word, from the dash carry that enters it.
// EMIT = false: from no open run - the runs that end in the chunk are counted and the run it leaves open is its summary;
// EMIT = true: from the run that is open where it begins - the records that end in it leave, behind those of the chunks before
template <bool EMIT>
__global__ __launch_bounds__(64) void rs_walk_kernel(const uint8_t *__restrict__ chars, const uint4 *__restrict__ cdesc, const Dash *__restrict__ cdash,
                                                     Part *__restrict__ cpart, uint32_t *__restrict__ cnt, const uint32_t *__restrict__ cnt_sums,
                                                     uint32_t n_cslots, uint32_t max_gap_len, uint32_t *__restrict__ out, uint32_t capacity)
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
    rs_stage(chars, sh_start, sh_len, rows);
    __syncthreads();
    if (c >= n_cslots) return;
    uint32_t n_out = 0;
    if (!cl) {
        if (!EMIT) {
            cnt[c] = 0u;
            cpart[c] = part_identity();
        }
        return;
    }
    const uint32_t len = d.z, p0 = d.y;
    const uint32_t *row = rows + threadIdx.x * kRowWords;
    // the bytes in front of and behind the chunk: the same sequence's
    uint32_t prev = p0 > 0u ? (uint32_t)chars[d.x - 1u] : 0u;
    const uint32_t after = p0 + cl < len ? (uint32_t)chars[d.x + cl] : 0u;
    const uint32_t slot0 = EMIT ? cnt_sums[c / kScanBlock] + cnt[c] : 0u;
    Walk w = walk_begin(cdash[c], EMIT ? cpart[c] : part_identity());
    bool broke = false;
    auto close = [&](const Rec &r) {
        if (EMIT) {
            const uint32_t slot = slot0 + n_out;
            if (slot < capacity) {
                const uint32_t rec[7] = {r.start, r.end, r.matches, r.mismatches, r.jumps, r.gap_bases, r.gap_opens};
                __builtin_memcpy(out + (uint64_t)slot * 7u, rec, 28); // (16 + 12 bytes: two stores instead of seven)
            }
        }
        n_out++;
    };
    const uint32_t nw = (cl + 3u) >> 2;
    uint32_t v = row[0];
    for (uint32_t wi = 0; wi < nw; wi++) {
        const uint32_t nx = wi + 1u < nw ? row[wi + 1u] : 0u;
#pragma unroll
        for (uint32_t j = 0; j < 4u; j++) {
            const uint32_t q = 4u * wi + j;
            if (q < cl) {
                const uint32_t ch = (v >> (8u * j)) & 0xFFu;
                uint32_t next = (j < 3u ? v >> (8u * (j + 1u)) : nx) & 0xFFu;
                if (q + 1u == cl) next = after; // (behind the chunk's last position the row holds whatever follows the sequence)
                walk_step(w, ch, prev, next, p0 + q, len, max_gap_len, broke, close);
                prev = ch;
            }
        }
        v = nx;
    }
    if (!EMIT) {
        cnt[c] = n_out;
        cpart[c] = walk_end(w, broke);
    }
}

// lane = sequence (and one behind the last: the batch's total): the index of its first run is that of its first chunk's
__global__ void rs_first_kernel(const uint32_t *__restrict__ cc, const uint32_t *__restrict__ csums, const uint32_t *__restrict__ cnt,
                                const uint32_t *__restrict__ cnt_sums, uint32_t n_seqs, uint32_t *__restrict__ first)
{
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s > n_seqs) return;
    const uint32_t c = csums[s / kScanBlock] + cc[s];
    first[s] = cnt_sums[c / kScanBlock] + cnt[c];
}

struct SegLayout {
    uint32_t n_cslots, n_gslots;
    size_t cc, gc, cdesc, gdesc, cdash, gdash, cpart, gpart, cnt, end;
};
SegLayout seg_layout(uint32_t n_seqs, uint64_t total_bases)
{
    SegLayout L;
    const uint64_t nc = total_bases / kC + n_seqs, ng = nc / kGC + n_seqs + 1u;
    L.n_cslots = (uint32_t)std::min<uint64_t>(nc, 0xFFFFFFFEu);
    L.n_gslots = (uint32_t)std::min<uint64_t>(ng, 0xFFFFFFFEu);
    auto up = [](size_t b) { return (b + 15) / 16 * 16; };
    const size_t scan = up(chunk_items_scratch_words(n_seqs) * sizeof(uint32_t));
    size_t w = 0;
    L.cc = w;    w += scan;
    L.gc = w;    w += scan;
    L.cdesc = w; w += (size_t)nc * sizeof(uint4);
    L.gdesc = w; w += (size_t)ng * sizeof(uint4);
    L.cpart = w; w += (size_t)nc * sizeof(Part);
    L.gpart = w; w += (size_t)ng * sizeof(Part);
    L.cdash = w; w += up((size_t)nc * sizeof(Dash));
    L.gdash = w; w += up((size_t)ng * sizeof(Dash));
    L.cnt = w;   w += up(chunk_items_scratch_words(L.n_cslots) * sizeof(uint32_t));
    L.end = w;
    return L;
}
static_assert(sizeof(Part) == 48 && sizeof(Dash) == 8, "the scratch formula in kbo_hip.h counts on these");

std::atomic<uint64_t> g_count_calls{0}, g_emit_calls{0};

} // namespace

size_t rle_seg_work_bytes(uint32_t n_seqs, uint64_t total_bases) { return seg_layout(n_seqs, total_bases).end; }

void rle_seg_calls(uint64_t *count_calls, uint64_t *emit_calls)
{
    if (count_calls) *count_calls = g_count_calls.load();
    if (emit_calls) *emit_calls = g_emit_calls.load();
}

hipError_t launch_rle_seg_count(const uint8_t *d_chars, const uint64_t *d_offsets, uint32_t n_seqs, uint64_t total_bases, uint32_t max_gap_len,
                                uint32_t min_len, void *d_work, uint32_t *d_first, hipStream_t stream)
{
    if (n_seqs == 0) return hipSuccess;
    const SegLayout L = seg_layout(n_seqs, total_bases);
    if ((uint64_t)L.n_cslots + L.n_gslots > 0xFFFFFFFEull) return hipErrorInvalidValue; // (n_seqs < 2^28: the callers check)
    g_count_calls.fetch_add(1);
    uint8_t *w = static_cast<uint8_t *>(d_work);
    const uint32_t n = n_seqs + 1u;
    uint32_t *cc = reinterpret_cast<uint32_t *>(w + L.cc), *csums = cc + n;
    uint32_t *gc = reinterpret_cast<uint32_t *>(w + L.gc), *gsums = gc + n;
    uint4 *cdesc = reinterpret_cast<uint4 *>(w + L.cdesc), *gdesc = reinterpret_cast<uint4 *>(w + L.gdesc);
    Dash *cdash = reinterpret_cast<Dash *>(w + L.cdash), *gdash = reinterpret_cast<Dash *>(w + L.gdash);
    Part *cpart = reinterpret_cast<Part *>(w + L.cpart), *gpart = reinterpret_cast<Part *>(w + L.gpart);
    uint32_t *cnt = reinterpret_cast<uint32_t *>(w + L.cnt), *cnt_sums = cnt + L.n_cslots + 1u;
    const uint32_t T = 256;
    auto blocks = [&](uint64_t lanes) { return dim3((unsigned)((lanes + T - 1) / T)); };
    hipLaunchKernelGGL(rs_list_count_kernel, blocks(n), dim3(T), 0, stream, d_offsets, n_seqs, min_len, cc, gc);
    hipError_t e = launch_scan(cc, n, csums, stream);
    if (e != hipSuccess) return e;
    e = launch_scan(gc, n, gsums, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(rs_desc_kernel, blocks((uint64_t)L.n_cslots + L.n_gslots), dim3(T), 0, stream, d_offsets, n_seqs, cc, csums, gc, gsums,
                       L.n_cslots, L.n_gslots, cdesc, gdesc);
    hipLaunchKernelGGL(rs_dash_kernel, blocks((uint64_t)L.n_cslots + 1u), dim3(T), 0, stream, d_chars, cdesc, L.n_cslots, cdash, cnt);
    hipLaunchKernelGGL(rs_dash_group_kernel, blocks(L.n_gslots), dim3(T), 0, stream, cdash, gdesc, L.n_gslots, gdash);
    hipLaunchKernelGGL(rs_dash_top_kernel, blocks(n_seqs), dim3(T), 0, stream, gdash, gc, gsums, n_seqs);
    hipLaunchKernelGGL(rs_dash_in_kernel, blocks(L.n_gslots), dim3(T), 0, stream, cdash, gdash, gdesc, L.n_gslots);
    const dim3 waves((L.n_cslots + kRows - 1u) / kRows);
    hipLaunchKernelGGL((rs_walk_kernel<false>), waves, dim3(kRows), 0, stream, d_chars, cdesc, cdash, cpart, cnt, (const uint32_t *)nullptr,
                       L.n_cslots, max_gap_len, (uint32_t *)nullptr, 0u);
    hipLaunchKernelGGL(rs_part_group_kernel, blocks(L.n_gslots), dim3(T), 0, stream, cpart, gdesc, L.n_gslots, gpart);
    hipLaunchKernelGGL(rs_part_top_kernel, blocks(n_seqs), dim3(T), 0, stream, gpart, gc, gsums, n_seqs);
    hipLaunchKernelGGL(rs_part_in_kernel, blocks(L.n_gslots), dim3(T), 0, stream, cpart, gpart, gdesc, L.n_gslots);
    e = launch_scan(cnt, L.n_cslots + 1u, cnt_sums, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(rs_first_kernel, blocks(n), dim3(T), 0, stream, cc, csums, cnt, cnt_sums, n_seqs, d_first);
    return hipGetLastError();
}

hipError_t launch_rle_seg_emit(const uint8_t *d_chars, uint32_t n_seqs, uint64_t total_bases, uint32_t max_gap_len, void *d_work, uint32_t *d_rles,
                               uint32_t capacity, hipStream_t stream)
{
    if (n_seqs == 0) return hipSuccess;
    const SegLayout L = seg_layout(n_seqs, total_bases);
    g_emit_calls.fetch_add(1);
    uint8_t *w = static_cast<uint8_t *>(d_work);
    const uint4 *cdesc = reinterpret_cast<const uint4 *>(w + L.cdesc);
    const Dash *cdash = reinterpret_cast<const Dash *>(w + L.cdash);
    Part *cpart = reinterpret_cast<Part *>(w + L.cpart);
    uint32_t *cnt = reinterpret_cast<uint32_t *>(w + L.cnt);
    hipLaunchKernelGGL((rs_walk_kernel<true>), dim3((L.n_cslots + kRows - 1u) / kRows), dim3(kRows), 0, stream, d_chars, cdesc, cdash, cpart, cnt,
                       cnt + L.n_cslots + 1u, L.n_cslots, max_gap_len, d_rles, capacity);
    return hipGetLastError();
}

} // namespace kbo
