// gap_kernels.hip — gfx950 (MI355X, CDNA4): gap_filling::fill_gaps (reference gap_filling.rs:444-526) over a batch, on
// the device, behind the walk with intervals and the translation.
//
// gap_starts_kernel, one lane per base.  The reference finds its gaps with a sequential scan, but its gaps are
// independent: a fill writes only [start, end) and later starts read only characters at or after `end`, and a fill never
// writes '-'.  So with t = threshold and tr = the translation, position s starts a gap iff
//     t <= s < n - t - 1,  tr[s] is '-' or 'X',  and not (tr[s] == '-' && s - 1 >= t && tr[s - 1] is '-' or 'X')
// (tests/test_map_batch_opts_host.py checks this rule against the scan).  Starts are compacted with a ballot and one
// atomic per wave, as call_sites_kernel does; the count may exceed the capacity (the host launches again with room).
//
// gap_fill_kernel, one wave per gap: kbo::left_extend_over_gap and the checks of kbo::fill_gaps (refine.cpp), with
//  * the candidate scan of nearest_unique_context 64 positions at a time (the highest single-row position wins: the
//    reference scans downwards),
//  * the candidate row spelled off the path cover as call_finalize_kernel does (a window that crosses a path start goes
//    to the host),
//  * count_right_overlaps / count_left_overlaps by lanes and a ballot (the right count never compares kmer[0], the left
//    one starts at ref_start_pos, as the reference's),
//  * left_extend_kmer: every step searches c + kmer[0 .. k-1] for the four bases, one lane each, k rank steps over the
//    arena's rank blocks; the step succeeds iff exactly one search finds a row and that one finds a single row.  The
//    growing k-mer lives in LDS,
//  * the fill_overlaps test from a host-made table of log_rm_max_cdf(run + 1, 4, 1), summed in the reference's order
//    and compared with log1p(-max_err_prob) from the host: no log runs on the device.
// Every index condition where refine.cpp would throw RefPanic, a missing cover, a broken window and an extension longer
// than the LDS budget flag the gap's sequence: the host redoes that sequence whole with kbo::fill_gaps (from a pristine
// copy of the translation), so results and errors are the reference's by construction.
#include "device_util.hpp"

#include <algorithm>

namespace kbo {
namespace {

constexpr uint32_t kGapLds = kGapFillLds;

__device__ __forceinline__ bool is_gap_char(uint32_t c) { return c == '-' || c == 'X'; }

__global__ __launch_bounds__(256) void gap_starts_kernel(const uint8_t *__restrict__ tr, const uint64_t *__restrict__ off,
                                                         uint32_t n_seqs, uint64_t total, uint32_t t, uint2 *__restrict__ gaps,
                                                         uint32_t cap, uint32_t *__restrict__ count)
{
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    bool hit = false;
    uint2 rec = make_uint2(0, 0);
    if (p < total) {
        const uint32_t c = tr[p];
        if (is_gap_char(c)) {
            uint32_t s0 = 0, s1 = n_seqs; // the sequence that holds p: largest s with off[s] <= p
            while (s1 - s0 > 1) {
                const uint32_t m = s0 + (s1 - s0) / 2;
                if (off[m] <= p) s0 = m;
                else s1 = m;
            }
            const uint64_t s = p - off[s0], n = off[s0 + 1] - off[s0];
            hit = s >= t && s + t + 1 < n && !(c == '-' && s >= (uint64_t)t + 1 && is_gap_char(tr[p - 1]));
            rec = make_uint2(s0, (uint32_t)s);
        }
    }
    const uint64_t mk = __ballot(hit);
    if (mk) {
        const uint32_t leader = (uint32_t)__builtin_ctzll(mk);
        uint32_t base = 0;
        if (lane == leader) base = atomicAdd(count, (uint32_t)__popcll(mk));
        base = __shfl(base, leader);
        const uint32_t slot = base + __builtin_amdgcn_mbcnt_hi((uint32_t)(mk >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mk, 0u));
        if (hit && slot < cap) gaps[slot] = rec;
    }
}

// sbwt search() of c followed by the `rest` bytes at pre[0 ..], from the root; false when a byte is no base or the
// interval empties (HostNav::search)
__device__ bool search_rows(const DevIndexView &ix, uint32_t c, const uint8_t *pre, uint32_t rest, uint32_t &l, uint32_t &r)
{
    l = 0;
    r = ix.n;
    const uint8_t *arena = reinterpret_cast<const uint8_t *>(ix.arena);
    for (uint32_t i = 0;; i++) {
        const uint32_t bl = div96(l), br = div96(r);
        const uint4 xA = ld16(arena, (c * ix.n_blocks + bl) << 4), xB = ld16(arena, (c * ix.n_blocks + br) << 4);
        l = rank_eval(xA, l - bl * 96u);
        r = rank_eval(xB, r - br * 96u);
        if (l >= r) return false;
        if (i == rest) return true;
        c = decode_base(pre[i]);
        if (c > 3u) return false;
    }
}

// first x in [0, cnt) where pred(x) holds, cnt if none (whole wave, 64 at a time)
template <typename P> __device__ __forceinline__ uint32_t wave_first(uint32_t cnt, uint32_t lane, P pred)
{
    for (uint32_t x0 = 0; x0 < cnt; x0 += 64u) {
        const uint32_t x = x0 + lane;
        const uint64_t m = __ballot(x < cnt && pred(x));
        if (m) return x0 + (uint32_t)__builtin_ctzll(m);
    }
    return cnt;
}

struct GapArgs {
    const uint8_t *q;     // the slab's bases
    const uint8_t *tr;    // its translation (read only)
    uint8_t *out;         // where the fills go (a copy of tr)
    const uint32_t *lo, *hi;
    const uint64_t *off;
    const uint2 *gaps;    // {sequence, start}
    uint32_t n_gaps;
    uint32_t t, k;
    const double *log_tab; // log_tab[c] = log_rm_max_cdf(c + 1, 4, 1), c < kGapFillLds
    double log_thr;        // log1p(-max_err_prob)
    uint8_t *host_flag;    // per sequence: 1 = redo on the host
    unsigned long long *stats; // [0] gaps finished here, [1] left-extension steps
};

__global__ __launch_bounds__(64) void gap_fill_kernel(GapArgs a, DevIndexView ix)
{
    __shared__ uint8_t kb[kGapLds];  // the k-mer, right-aligned: kb[kGapLds - S .. kGapLds)
    __shared__ uint8_t mat[kGapLds]; // matching[] of the fill test
    const uint32_t lane = threadIdx.x;
    const uint32_t k = a.k, t = a.t;
    for (uint32_t g = blockIdx.x; g < a.n_gaps; g += gridDim.x) {
        const uint2 gp = a.gaps[g];
        const uint32_t seq = gp.x, start = gp.y;
        const uint64_t b0 = a.off[seq];
        const uint32_t n = (uint32_t)(a.off[seq + 1] - b0);
        const uint8_t *ref = a.q + b0;
        const uint8_t *tr = a.tr + b0;
        bool host = false;
        // gap end: first index > start whose character is not '-', at most n - t (gap_filling.rs:471-474)
        const uint32_t lim = n - t;
        const uint32_t end = start + 1u + wave_first(lim - start - 1u, lane, [&](uint32_t x) { return tr[start + 1u + x] != '-'; });
        const uint32_t gap = end - start;
        const bool owe = gap + 2u * t <= k; // overlap_without_extend
        uint32_t S = 0, rs = 0, re = 0;     // the result: kb[kGapLds - S + rs .. kGapLds - S + re)
        bool have = false;
        if (!host) {
            // ---- left_extend_over_gap (gap_filling.rs:295-361), left/right_overlap_req = t
            const uint32_t radius = owe ? k - t : k;
            const uint32_t search_start = min(end + radius, n - 1u);
            const uint32_t search_end = end + t;
            uint32_t idx = search_start;
            while (idx >= search_end && !host) {
                // nearest_unique_context: highest j in [search_end, idx] with a single row
                const uint32_t span = idx - search_end + 1u;
                const uint32_t x = wave_first(span, lane, [&](uint32_t y) { return a.hi[b0 + idx - y] - a.lo[b0 + idx - y] == 1u; });
                if (x == span) break; // no context: the kmer stays empty
                const uint32_t j = idx - x;
                // spell the row off the path cover (call_finalize_kernel)
                const uint32_t row = a.lo[b0 + j];
                bool broken = ix.pc_text == nullptr;
                if (!broken) {
                    const int64_t p = (int64_t)ix.pc_pos[row];
                    for (uint32_t tt = lane; tt < k; tt += 64u) {
                        const int64_t qq = p - (int64_t)(k - 1u) + tt;
                        uint32_t ch = 0;
                        if (qq >= -(int64_t)kPlanPad) ch = ix.pc_text[qq];
                        if (tt == 0 && qq >= 0) {
                            const uint32_t r0 = ix.pc_node[qq];
                            ch = r0 >= ix.C[3] ? 'T' : r0 >= ix.C[2] ? 'G' : r0 >= ix.C[1] ? 'C' : r0 >= ix.C[0] ? 'A' : '$';
                        }
                        broken = broken || ch == 0 || ch == '$';
                        kb[kGapLds - k + tt] = (uint8_t)ch;
                    }
                }
                if (__ballot(broken)) { host = true; break; }
                __syncthreads();
                S = k;
                const uint32_t rmw = j - end + 1u; // right_matches_want
                // count_right_overlaps(kmer, ref, j + 1): kmer[k-1-m] vs ref[j-m], m = 0 .. k-2
                const uint32_t mr = min(k - 1u, j + 1u);
                const uint32_t m0 = wave_first(mr, lane, [&](uint32_t m) { return kb[kGapLds - 1u - m] != ref[j - m]; });
                if (m0 == mr && j <= k - 2u) { host = true; break; } // ref_pos -= 1 below 0
                const uint32_t right = m0;
                const uint32_t rsp = start > t ? start - t : 0u; // ref_start_pos
                // count_left_overlaps(kmer, ref, rsp)
                auto left_count = [&](uint32_t size, bool &panic) {
                    const uint32_t x0 = wave_first(size, lane, [&](uint32_t y) { return rsp + y >= n || kb[kGapLds - size + y] != ref[rsp + y]; });
                    panic = x0 < size && rsp + x0 >= n;
                    return x0;
                };
                bool panic = false;
                const uint32_t left = left_count(S, panic);
                if (panic) { host = true; break; }
                const bool should_extend = S < t + gap + right;
                const bool right_ok = right >= min(rmw, k);
                if (right_ok && left >= t) {
                    if (right < t) { host = true; break; }
                    rs = left - t;
                    re = S - (right - t);
                    if (rs > re) { host = true; break; }
                    have = true;
                    break;
                } else if (should_extend && right_ok && left < t) {
                    const uint32_t L = t + gap + right - k; // left_extend_length
                    if (k + L > kGapLds) { host = true; break; }
                    // ---- left_extend_kmer (gap_filling.rs:205-232): c + kmer[0 .. k-1], four searches
                    uint32_t steps = 0;
                    while (steps < L) {
                        const uint8_t *pre = kb + kGapLds - S; // kmer[0 ..]
                        uint32_t l = 0, r = 0;
                        bool found = false;
                        if (lane < 4u) found = search_rows(ix, lane, pre, k - 1u, l, r);
                        const uint64_t fm = __ballot(found) & 0xFull;
                        const uint32_t lead = fm ? (uint32_t)__builtin_ctzll(fm) : 0u;
                        const uint32_t width = __shfl(r - l, lead);
                        if (__popcll(fm) != 1 || width != 1u) break;
                        __syncthreads();
                        if (lane == 0) kb[kGapLds - S - 1u] = (uint8_t)"ACGT"[lead];
                        __syncthreads();
                        S++;
                        steps++;
                    }
                    if (lane == 0 && steps) atomicAdd(a.stats + 1, (unsigned long long)steps);
                    const uint32_t lm = left_count(S, panic);
                    if (panic) { host = true; break; }
                    if (lm >= t) {
                        if (right < t) { host = true; break; }
                        rs = lm - t;
                        re = S - (right - t);
                        if (rs > re) { host = true; break; }
                        have = true;
                        break;
                    }
                }
                S = 0;
                idx = j - 1u;
                __syncthreads();
            }
        }
        if (host) {
            if (lane == 0) a.host_flag[seq] = 1;
            __syncthreads();
            continue;
        }
        // ---- the checks of fill_gaps (gap_filling.rs:480-519): the kmer found, no indels, and one of three tests
        const uint32_t R = have ? re - rs : 0u;
        const uint8_t *res = kb + kGapLds - S + rs;
        if (have && R == 2u * t + gap) {
            bool fill = owe;
            if (!fill) {
                // matching[w] = res[t + w] == ref[start + w], w < gap
                for (uint32_t w = lane; w < gap; w += 64u) mat[w] = res[t + w] == ref[start + w] ? 1 : 0;
                __syncthreads();
                uint32_t total = 0;
                for (uint32_t w = lane; w < gap; w += 64u) total += mat[w];
                for (int sh = 32; sh > 0; sh >>= 1) total += __shfl_xor(total, sh);
                bool fill_overlaps = false;
                if (lane == 0) {
                    double log_probs = 0.0;
                    uint32_t consecutive = 0;
                    for (uint32_t w = 0; w + 1u < gap; w++) {
                        if (mat[w] && mat[w + 1u]) consecutive++;
                        else {
                            if (consecutive > 0) log_probs += a.log_tab[consecutive]; // consecutive < gap < kGapLds
                            consecutive = 0;
                        }
                    }
                    fill_overlaps = log_probs > a.log_thr;
                }
                fill_overlaps = __shfl((int)fill_overlaps, 0) != 0;
                const bool fill_flanked = gap > 0 && !mat[0] && !mat[gap - 1u] && total + 2u == gap;
                fill = fill_overlaps || fill_flanked;
            }
            if (fill)
                for (uint32_t w = lane; w < gap; w += 64u) {
                    const uint8_t c = res[t + w];
                    a.out[b0 + start + w] = c == ref[start + w] ? (uint8_t)'M' : c;
                }
        }
        if (lane == 0) atomicAdd(a.stats, 1ull);
        __syncthreads();
    }
}

} // namespace

hipError_t launch_gap_starts(const uint8_t *d_tr, const uint64_t *d_off, uint32_t n_seqs, uint64_t total, uint32_t threshold,
                             void *d_gaps, uint32_t cap, uint32_t *d_count, hipStream_t stream)
{
    if (total == 0 || n_seqs == 0) return hipSuccess;
    hipLaunchKernelGGL(gap_starts_kernel, dim3((uint32_t)((total + 255) / 256)), dim3(256), 0, stream, d_tr, d_off, n_seqs, total,
                       threshold, static_cast<uint2 *>(d_gaps), cap, d_count);
    return hipGetLastError();
}

hipError_t launch_gap_fill(const uint8_t *d_q, const uint8_t *d_tr, uint8_t *d_out, const uint32_t *d_lo, const uint32_t *d_hi,
                           const uint64_t *d_off, const void *d_gaps, uint32_t n_gaps, uint32_t k, uint32_t threshold,
                           const double *d_log_tab, double log_thr, uint8_t *d_host_flag,
                           unsigned long long *d_stats, const DevIndexView &ix, hipStream_t stream)
{
    if (n_gaps == 0) return hipSuccess;
    if (k > 255u) return hipErrorInvalidValue;
    GapArgs a;
    a.q = d_q;
    a.tr = d_tr;
    a.out = d_out;
    a.lo = d_lo;
    a.hi = d_hi;
    a.off = d_off;
    a.gaps = static_cast<const uint2 *>(d_gaps);
    a.n_gaps = n_gaps;
    a.t = threshold;
    a.k = k;
    a.log_tab = d_log_tab;
    a.log_thr = log_thr;
    a.host_flag = d_host_flag;
    a.stats = d_stats;
    hipLaunchKernelGGL(gap_fill_kernel, dim3(std::min<uint32_t>(n_gaps, 16384u)), dim3(64), 0, stream, a, ix);
    return hipGetLastError();
}

} // namespace kbo
