// build_kernels.hip — gfx950 (MI355X, CDNA4): kbo::build on the device (build_device.cpp drives the passes).  The same five steps as
// build_impl in sbwt_build.cpp, over the same colex keys (digit t = code of the t-th character from the END of the row, 2 bits, most
// significant first, left-aligned in W 64-bit words; '$' = 0, told apart by the row's count of real characters).  Keys are kept as W
// word arrays ("SoA": word j of key i at keys[j * stride + i]) so that the sort moves one 8-byte word array at a time.
//
//   extract_kernel       tile of 8 192 bases + a (k - 1)-base halo in LDS as 2-bit codes (4 = not ACGT); a lane rolls the forward and
//                        reverse-complement keys over its 32 positions, emitting those that end an ACGT run of >= k bases; one atomic
//                        per wave reserves the output (order is free: the sort restores it)
//   radix_hist_kernel    LSD radix sort, 8-bit digits over the 2k significant bits (and, for dummy rows, a first pass over `real`):
//   radix_scatter_kernel per tile of 4 096 keys a histogram, a scan over (digit, tile), then a stable rank inside the tile (wave ballots
//                        over the digit bits) and a scatter staged through LDS so that each word array is written digit run by run
//   flag_* / compact_*   duplicate and orphan flags, then a stable compaction (per-tile counts, a scan, ballots inside the tile)
//   dummy_kernel         the k - 1 $-padded prefixes of every orphan (and the root)
//   merge_*_kernel       rows in colex order: dummy i goes to i + (k-mers with a smaller key), k-mer a to a + (dummies before it)
//   edge_kernel          each row finds the first row of its predecessor's (k-1)-suffix group by a search over the rows and sets that
//                        group's bit in B_c (64-bit atomicOr: no two rows of one c hit the same bit); rows per last character counted
//   popc_kernel          edge bits per character (for C[] and the edge-count check)
//   lcs_kernel           one lane per row: common leading digits of the neighbouring keys, capped by the two real counts
//
// Integer / bit work only: no MFMA.  Stores are vector stores.
#include "device_util.hpp"

namespace kbo {
namespace {

constexpr uint32_t kBT = 256;                   // threads per workgroup
constexpr uint32_t kPerLane = 32;               // extraction: positions per lane
constexpr uint32_t kExtTile = kBT * kPerLane;   // extraction: positions per workgroup
constexpr uint32_t kItems = kBuildTile / kBT;   // sort / compaction: keys per thread of a tile

__device__ __forceinline__ uint32_t code_of(uint8_t ch)
{
    return ch == 'A' ? 0u : ch == 'C' ? 1u : ch == 'G' ? 2u : ch == 'T' ? 3u : 4u; // (lower case splits a run, as on the host)
}

// the bits of the 2k significant bits that word j holds
__device__ __forceinline__ uint64_t mask_word(uint32_t k, int j)
{
    const int bits = (int)(2u * k) - 64 * j;
    return bits <= 0 ? 0ull : bits >= 64 ? ~0ull : ~0ull << (64 - bits);
}

template <int W> __device__ __forceinline__ void ld_key(const uint64_t *__restrict__ keys, uint64_t stride, uint64_t i, uint64_t (&w)[W])
{
#pragma unroll
    for (int j = 0; j < W; j++) w[j] = keys[(uint64_t)j * stride + i];
}
template <int W> __device__ __forceinline__ void st_key(uint64_t *__restrict__ keys, uint64_t stride, uint64_t i, const uint64_t (&w)[W])
{
#pragma unroll
    for (int j = 0; j < W; j++) keys[(uint64_t)j * stride + i] = w[j];
}
template <int W> __device__ __forceinline__ void shl2(uint64_t (&w)[W])
{
#pragma unroll
    for (int j = 0; j < W; j++) w[j] = (w[j] << 2) | (j + 1 < W ? w[j + 1 < W ? j + 1 : j] >> 62 : 0ull);
}
template <int W> __device__ __forceinline__ void shr2(uint64_t (&w)[W])
{
#pragma unroll
    for (int j = W - 1; j > 0; j--) w[j] = (w[j] >> 2) | (w[j - 1] << 62);
    w[0] >>= 2;
}
// digit p := v (p < 32 W; the word is picked without indexing the register array by a run-time value)
template <int W> __device__ __forceinline__ void set_digit(uint64_t (&w)[W], uint32_t p, uint64_t v)
{
    const uint32_t wi = (2u * p) >> 6, sh = 62u - ((2u * p) & 63u);
#pragma unroll
    for (int j = 0; j < W; j++)
        if ((uint32_t)j == wi) w[j] = (w[j] & ~(3ull << sh)) | (v << sh);
}
// -1 / 0 / 1
template <int W> __device__ __forceinline__ int cmp_key(const uint64_t (&a)[W], const uint64_t (&b)[W])
{
#pragma unroll
    for (int j = 0; j < W; j++)
        if (a[j] != b[j]) return a[j] < b[j] ? -1 : 1;
    return 0;
}

// ---- 1. extraction
template <int W>
__global__ __launch_bounds__(kBT) void extract_kernel(const uint8_t *__restrict__ seq, uint64_t n_bytes, uint32_t k, uint32_t want_fw,
                                                      uint32_t want_rc, uint64_t *__restrict__ keys, uint64_t stride,
                                                      unsigned long long *__restrict__ count)
{
    __shared__ uint8_t code[kExtTile + 256];
    const uint64_t t0 = (uint64_t)blockIdx.x * kExtTile;
    const uint32_t halo = k - 1u; // slot s holds position t0 - halo + s
    for (uint32_t s = threadIdx.x; s < kExtTile + halo; s += kBT) {
        const uint64_t p = t0 + s - halo; // (wraps below 0: then >= n_bytes)
        code[s] = (uint8_t)(t0 + s >= halo && p < n_bytes ? code_of(seq[p]) : 4u);
    }
    __syncthreads();
    const uint32_t s0 = threadIdx.x * kPerLane, lane = threadIdx.x & 63u;
    uint32_t run = 0, cnt = 0;
    for (uint32_t j = 0; j < halo + kPerLane; j++) {
        run = code[s0 + j] < 4u ? run + 1u : 0u;
        cnt += (j >= halo && run >= k) ? 1u : 0u;
    }
    const uint32_t mine = cnt * (want_fw + want_rc);
    uint32_t incl = mine; // inclusive scan over the wave
#pragma unroll
    for (uint32_t o = 1; o < 64u; o <<= 1) {
        const uint32_t v = (uint32_t)__shfl_up((int)incl, o);
        if (lane >= o) incl += v;
    }
    unsigned long long base = 0;
    if (lane == 63u && incl) base = atomicAdd(count, (unsigned long long)incl);
    base = __shfl(base, 63);
    if (!mine) return;
    uint64_t o = base + incl - mine;
    uint64_t fw[W], rc[W], m[W];
#pragma unroll
    for (int j = 0; j < W; j++) { fw[j] = rc[j] = 0ull; m[j] = mask_word(k, j); }
    run = 0;
    for (uint32_t j = 0; j < halo + kPerLane; j++) {
        const uint32_t c = code[s0 + j];
        if (c >= 4u) {
            run = 0;
#pragma unroll
            for (int q = 0; q < W; q++) fw[q] = rc[q] = 0ull;
            continue;
        }
        run++;
        shr2(fw); // older characters move away from the end
        fw[0] |= (uint64_t)c << 62;
#pragma unroll
        for (int q = 0; q < W; q++) fw[q] &= m[q];
        if (want_rc) { // the reverse complement ends with comp(first character)
            shl2(rc);
            set_digit(rc, k - 1u, (uint64_t)(3u - c));
        }
        if (j >= halo && run >= k) {
            if (want_fw) st_key(keys, stride, o++, fw);
            if (want_rc) st_key(keys, stride, o++, rc);
        }
    }
}

// ---- 2. LSD radix sort
// digit of key i: `real` byte (sel.real) or the bits [a, a + nb) of the key counted from its most significant bit (nb <= 8)
__device__ __forceinline__ uint32_t digit_at(const uint64_t *__restrict__ keys, uint64_t stride, const uint8_t *__restrict__ real, uint64_t i,
                                             const RadixPass &ps)
{
    if (ps.real) return real[i];
    const uint32_t b = ps.a + ps.nb, w1 = (b - 1u) >> 6, msk = (1u << ps.nb) - 1u;
    const uint64_t x1 = keys[(uint64_t)w1 * stride + i];
    if ((ps.a >> 6) == w1) return (uint32_t)(x1 >> (64u * (w1 + 1u) - b)) & msk;
    const uint32_t nlo = b - 64u * w1; // bits from the top of word w1, the rest from the bottom of word w1 - 1
    const uint64_t x0 = keys[(uint64_t)(w1 - 1u) * stride + i];
    return (uint32_t)((x0 << nlo) | (x1 >> (64u - nlo))) & msk;
}

__global__ __launch_bounds__(kBT) void radix_hist_kernel(const uint64_t *__restrict__ keys, uint64_t stride, const uint8_t *__restrict__ real,
                                                         uint64_t n, RadixPass ps, uint32_t n_tiles, uint32_t *__restrict__ hist)
{
    __shared__ uint32_t h[256];
    h[threadIdx.x] = 0u;
    __syncthreads();
    const uint64_t base = (uint64_t)blockIdx.x * kBuildTile;
#pragma unroll 4
    for (uint32_t j = 0; j < kItems; j++) {
        const uint64_t i = base + j * kBT + threadIdx.x;
        if (i < n) atomicAdd(&h[digit_at(keys, stride, real, i, ps)], 1u);
    }
    __syncthreads();
    hist[(uint64_t)threadIdx.x * n_tiles + blockIdx.x] = h[threadIdx.x];
}

// exclusive prefix of v over the 256 threads of the workgroup (tmp: 4 words of LDS)
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t v, uint32_t *tmp)
{
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    uint32_t incl = v;
#pragma unroll
    for (uint32_t o = 1; o < 64u; o <<= 1) {
        const uint32_t t = (uint32_t)__shfl_up((int)incl, o);
        if (lane >= o) incl += t;
    }
    if (lane == 63u) tmp[wv] = incl;
    __syncthreads();
    uint32_t before = 0;
    for (uint32_t w = 0; w < wv; w++) before += tmp[w];
    __syncthreads();
    return before + incl - v;
}

__device__ __forceinline__ uint64_t lanes_below()
{
    const uint32_t lane = threadIdx.x & 63u;
    return lane ? (~0ull >> (64u - lane)) : 0ull;
}

// one pass: keys [0, n) of `kin` (n_words word arrays, + `rin` bytes when given) to `kout` (+ `rout`), stable in the digit
__global__ __launch_bounds__(kBT) void radix_scatter_kernel(const uint64_t *__restrict__ kin, uint64_t *__restrict__ kout, uint32_t n_words,
                                                            uint64_t stride, const uint8_t *__restrict__ rin, uint8_t *__restrict__ rout,
                                                            uint64_t n, RadixPass ps, uint32_t n_tiles, const uint32_t *__restrict__ hist,
                                                            const uint32_t *__restrict__ sums)
{
    __shared__ uint64_t stage[kBuildTile];
    __shared__ uint8_t sdig[kBuildTile];
    __shared__ uint32_t lstart[256], gbase[256], run[256], wcnt[4][256], tmp[4];
    const uint32_t tid = threadIdx.x, wv = tid >> 6;
    const uint64_t base = (uint64_t)blockIdx.x * kBuildTile;
    const uint32_t in_tile = (uint32_t)min((uint64_t)kBuildTile, n - base);
    run[tid] = 0u;
#pragma unroll
    for (int w = 0; w < 4; w++) wcnt[w][tid] = 0u;
    __syncthreads();
    uint32_t dig[kItems];
#pragma unroll
    for (uint32_t j = 0; j < kItems; j++) {
        const uint64_t i = base + j * kBT + tid;
        dig[j] = i < n ? digit_at(kin, stride, rin, i, ps) : 256u;
        if (dig[j] < 256u) atomicAdd(&run[dig[j]], 1u);
    }
    __syncthreads();
    const uint32_t mine = run[tid], ex = block_excl_scan(mine, tmp);
    const uint64_t hi = (uint64_t)tid * n_tiles + blockIdx.x;
    lstart[tid] = ex;
    gbase[tid] = sums[hi / kScanBlock] + hist[hi];
    run[tid] = 0u;
    __syncthreads();
    // stable rank inside the tile: key order is (j, wave, lane)
    uint32_t slot[kItems];
    const uint64_t below = lanes_below();
#pragma unroll
    for (uint32_t j = 0; j < kItems; j++) {
        const uint32_t d = dig[j];
        const bool valid = d < 256u;
        uint64_t eq = __ballot(valid);
#pragma unroll
        for (uint32_t b = 0; b < 8u; b++) {
            const uint64_t bal = __ballot((d >> b) & 1u);
            eq &= ((d >> b) & 1u) ? bal : ~bal;
        }
        if (valid && !(eq & below)) wcnt[wv][d] = (uint32_t)__popcll(eq);
        __syncthreads();
        if (valid) {
            uint32_t off = run[d] + (uint32_t)__popcll(eq & below);
            for (uint32_t w = 0; w < wv; w++) off += wcnt[w][d];
            slot[j] = lstart[d] + off;
            sdig[slot[j]] = (uint8_t)d;
        }
        __syncthreads();
        run[tid] += wcnt[0][tid] + wcnt[1][tid] + wcnt[2][tid] + wcnt[3][tid];
#pragma unroll
        for (int w = 0; w < 4; w++) wcnt[w][tid] = 0u;
        __syncthreads();
    }
    // move every word array (and the real bytes) through LDS: consecutive slots of one digit go to consecutive addresses
    const uint32_t n_arr = n_words + (rin ? 1u : 0u);
    for (uint32_t a = 0; a < n_arr; a++) {
        const bool is_real = a == n_words;
#pragma unroll
        for (uint32_t j = 0; j < kItems; j++) {
            const uint64_t i = base + j * kBT + tid;
            if (dig[j] < 256u) stage[slot[j]] = is_real ? (uint64_t)rin[i] : kin[(uint64_t)a * stride + i];
        }
        __syncthreads();
        for (uint32_t s = tid; s < in_tile; s += kBT) {
            const uint32_t d = sdig[s];
            const uint64_t o = (uint64_t)gbase[d] + (s - lstart[d]);
            if (is_real) rout[o] = (uint8_t)stage[s];
            else kout[(uint64_t)a * stride + o] = stage[s];
        }
        __syncthreads();
    }
}

// ---- flags + stable compaction
// flags[i] = key i (with its real byte) differs from key i - 1
template <int W>
__global__ __launch_bounds__(kBT) void flag_distinct_kernel(const uint64_t *__restrict__ keys, uint64_t stride, const uint8_t *__restrict__ real,
                                                            uint64_t n, uint8_t *__restrict__ flags)
{
    const uint64_t i = (uint64_t)blockIdx.x * kBT + threadIdx.x;
    if (i >= n) return;
    bool f = i == 0;
    if (!f) {
        uint64_t a[W], b[W];
        ld_key(keys, stride, i, a);
        ld_key(keys, stride, i - 1u, b);
        f = cmp_key(a, b) != 0 || (real && real[i] != real[i - 1u]);
    }
    flags[i] = f ? 1u : 0u;
}

// flags[x] = k-mer x has no predecessor: no k-mer y with S(y) = P(x), P(x) = key(x) << 2 (drop the last character), S(y) = key(y) with
// digit k - 1 cleared (drop the first); S is ascending over the sorted k-mers, so a lower bound decides
template <int W>
__global__ __launch_bounds__(kBT) void flag_orphan_kernel(const uint64_t *__restrict__ keys, uint64_t stride, uint64_t n, uint32_t k,
                                                          uint8_t *__restrict__ flags)
{
    const uint64_t x = (uint64_t)blockIdx.x * kBT + threadIdx.x;
    if (x >= n) return;
    if (k == 1u) { flags[x] = 0u; return; }
    uint64_t P[W], S[W];
    ld_key(keys, stride, x, P);
    shl2(P);
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2u;
        ld_key(keys, stride, mid, S);
        set_digit(S, k - 1u, 0ull);
        if (cmp_key(S, P) < 0) lo = mid + 1u; else hi = mid;
    }
    bool found = false;
    if (lo < n) {
        ld_key(keys, stride, lo, S);
        set_digit(S, k - 1u, 0ull);
        found = cmp_key(S, P) == 0;
    }
    flags[x] = found ? 0u : 1u;
}

__global__ __launch_bounds__(kBT) void compact_count_kernel(const uint8_t *__restrict__ flags, uint64_t n, uint32_t *__restrict__ counts,
                                                            unsigned long long *__restrict__ total)
{
    __shared__ uint32_t tmp[4];
    const uint64_t base = (uint64_t)blockIdx.x * kBuildTile;
    uint32_t c = 0;
    for (uint32_t j = 0; j < kItems; j++) {
        const uint64_t i = base + j * kBT + threadIdx.x;
        c += (i < n && flags[i]) ? 1u : 0u;
    }
    const uint32_t ex = block_excl_scan(c, tmp);
    if (threadIdx.x == kBT - 1u) {
        counts[blockIdx.x] = ex + c;
        atomicAdd(total, (unsigned long long)(ex + c));
    }
}

// the flagged keys (n_words word arrays, + real bytes when given) in order to kout / rout
__global__ __launch_bounds__(kBT) void compact_kernel(const uint64_t *__restrict__ kin, uint64_t in_stride, uint64_t *__restrict__ kout,
                                                      uint64_t out_stride, uint32_t n_words, const uint8_t *__restrict__ rin,
                                                      uint8_t *__restrict__ rout, const uint8_t *__restrict__ flags, uint64_t n,
                                                      const uint32_t *__restrict__ counts, const uint32_t *__restrict__ sums)
{
    __shared__ uint32_t wsum[4];
    __shared__ uint32_t run;
    const uint32_t tid = threadIdx.x, wv = tid >> 6;
    const uint64_t base = (uint64_t)blockIdx.x * kBuildTile, below = lanes_below();
    const uint64_t tbase = (uint64_t)sums[blockIdx.x / kScanBlock] + counts[blockIdx.x];
    if (tid == 0) run = 0u;
    __syncthreads();
    for (uint32_t j = 0; j < kItems; j++) {
        const uint64_t i = base + j * kBT + tid;
        const bool f = i < n && flags[i];
        const uint64_t bal = __ballot(f);
        if ((tid & 63u) == 0) wsum[wv] = (uint32_t)__popcll(bal);
        __syncthreads();
        if (f) {
            uint32_t off = run + (uint32_t)__popcll(bal & below);
            for (uint32_t w = 0; w < wv; w++) off += wsum[w];
            const uint64_t o = tbase + off;
            for (uint32_t a = 0; a < n_words; a++) kout[(uint64_t)a * out_stride + o] = kin[(uint64_t)a * in_stride + i];
            if (rin) rout[o] = rin[i];
        }
        __syncthreads();
        if (tid == 0) run += wsum[0] + wsum[1] + wsum[2] + wsum[3];
        __syncthreads();
    }
}

// ---- 3. dummy rows: row 0 = the root $^k; row 1 + o (k - 1) + (j - 1) = $^(k-j) x[0 .. j) of orphan o, real j
// (key(x) shifted left by 2 (k - j) bits: the word arrays are read at run-time word offsets, no register array is indexed)
template <int W>
__global__ __launch_bounds__(kBT) void dummy_kernel(const uint64_t *__restrict__ orph, uint64_t o_stride, uint64_t n_orph, uint32_t k,
                                                    uint64_t *__restrict__ keys, uint64_t stride, uint8_t *__restrict__ real)
{
    const uint64_t t = (uint64_t)blockIdx.x * kBT + threadIdx.x, n = 1u + n_orph * (k - 1u);
    if (t >= n) return;
    uint64_t w[W];
    if (t == 0) {
#pragma unroll
        for (int q = 0; q < W; q++) w[q] = 0ull;
        st_key(keys, stride, 0, w);
        real[0] = 0u;
        return;
    }
    const uint64_t o = (t - 1u) / (k - 1u);
    const uint32_t j = (uint32_t)((t - 1u) % (k - 1u)) + 1u, bits = 2u * (k - j), ws = bits >> 6, bs = bits & 63u;
#pragma unroll
    for (int q = 0; q < W; q++) {
        const uint32_t src = (uint32_t)q + ws;
        uint64_t v = src < (uint32_t)W ? orph[(uint64_t)src * o_stride + o] << bs : 0ull;
        if (bs && src + 1u < (uint32_t)W) v |= orph[(uint64_t)(src + 1u) * o_stride + o] >> (64u - bs);
        w[q] = v;
    }
    st_key(keys, stride, t, w);
    real[t] = (uint8_t)j;
}

// ---- 4. merge: dummy i (all reals < k) precedes the k-mers with a key >= its own
template <int W>
__global__ __launch_bounds__(kBT) void merge_dummy_kernel(const uint64_t *__restrict__ km, uint64_t km_stride, uint64_t n_km,
                                                          const uint64_t *__restrict__ dk, uint64_t d_stride, const uint8_t *__restrict__ dreal,
                                                          uint64_t n_d, uint32_t *__restrict__ lb, uint64_t *__restrict__ rk, uint64_t r_stride,
                                                          uint8_t *__restrict__ rreal)
{
    const uint64_t i = (uint64_t)blockIdx.x * kBT + threadIdx.x;
    if (i >= n_d) return;
    uint64_t key[W], m[W];
    ld_key(dk, d_stride, i, key);
    uint64_t lo = 0, hi = n_km;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2u;
        ld_key(km, km_stride, mid, m);
        if (cmp_key(m, key) < 0) lo = mid + 1u; else hi = mid;
    }
    lb[i] = (uint32_t)lo;
    st_key(rk, r_stride, i + lo, key);
    rreal[i + lo] = dreal[i];
}

// k-mer a lands behind the dummies with lb <= a (lb is ascending: an upper bound)
template <int W>
__global__ __launch_bounds__(kBT) void merge_kmer_kernel(const uint64_t *__restrict__ km, uint64_t km_stride, uint64_t n_km, uint32_t k,
                                                         const uint32_t *__restrict__ lb, uint64_t n_d, uint64_t *__restrict__ rk, uint64_t r_stride,
                                                         uint8_t *__restrict__ rreal)
{
    const uint64_t a = (uint64_t)blockIdx.x * kBT + threadIdx.x;
    if (a >= n_km) return;
    uint64_t lo = 0, hi = n_d;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2u;
        if ((uint64_t)lb[mid] <= a) lo = mid + 1u; else hi = mid;
    }
    uint64_t key[W];
    ld_key(km, km_stride, a, key);
    st_key(rk, r_stride, a + lo, key);
    rreal[a + lo] = (uint8_t)k;
}

// ---- 4. edge bits.  Row y (real >= 1) receives its single incoming edge from the first row of the group whose (k-1)-suffix frame
// (key with digit k - 1 cleared, min(real, k - 1)) equals (key(y) << 2, real(y) - 1); frames are ascending over the rows.
// ctr[0] = rows without such a group, ctr[1 + c] = rows >= 1 whose last character is c
template <int W>
__global__ __launch_bounds__(kBT) void edge_kernel(const uint64_t *__restrict__ rk, uint64_t stride, const uint8_t *__restrict__ rreal, uint64_t n,
                                                   uint32_t k, uint64_t *__restrict__ rows, uint64_t n_words, unsigned long long *__restrict__ ctr)
{
    const uint64_t y = (uint64_t)blockIdx.x * kBT + threadIdx.x;
    const bool valid = y >= 1u && y < n;
    uint32_t c = 4u;
    bool missing = false;
    if (valid) {
        uint64_t P[W], F[W];
        ld_key(rk, stride, y, P);
        c = (uint32_t)(P[0] >> 62);
        shl2(P);
        const uint32_t pr = (uint32_t)rreal[y] - 1u;
        uint64_t lo = 0, hi = n;
        while (lo < hi) {
            const uint64_t mid = lo + (hi - lo) / 2u;
            ld_key(rk, stride, mid, F);
            set_digit(F, k - 1u, 0ull);
            const int cm = cmp_key(F, P);
            const uint32_t fr = min((uint32_t)rreal[mid], k - 1u);
            if (cm < 0 || (cm == 0 && fr < pr)) lo = mid + 1u; else hi = mid;
        }
        bool found = false;
        if (lo < n) {
            ld_key(rk, stride, lo, F);
            set_digit(F, k - 1u, 0ull);
            found = cmp_key(F, P) == 0 && min((uint32_t)rreal[lo], k - 1u) == pr;
        }
        if (found) atomicOr(reinterpret_cast<unsigned long long *>(rows + (uint64_t)c * n_words + (lo >> 6)), 1ull << (lo & 63u));
        else missing = true;
    }
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t miss = __ballot(missing);
    if (lane == 0 && miss) atomicAdd(ctr, (unsigned long long)__popcll(miss));
#pragma unroll
    for (uint32_t q = 0; q < 4u; q++) {
        const uint64_t b = __ballot(c == q);
        if (lane == 0 && b) atomicAdd(ctr + 1u + q, (unsigned long long)__popcll(b));
    }
}

// ctr[5 + c] += edge bits of B_c
__global__ __launch_bounds__(kBT) void popc_kernel(const uint64_t *__restrict__ rows, uint64_t n_words, unsigned long long *__restrict__ ctr)
{
    const uint64_t i = (uint64_t)blockIdx.x * kBT + threadIdx.x;
    const uint32_t c = blockIdx.y;
    uint32_t v = i < n_words ? (uint32_t)__popcll(rows[(uint64_t)c * n_words + i]) : 0u;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o);
    if ((threadIdx.x & 63u) == 0 && v) atomicAdd(ctr + 5u + c, (unsigned long long)v);
}

// ---- 5. LCS
template <int W>
__global__ __launch_bounds__(kBT) void lcs_kernel(const uint64_t *__restrict__ rk, uint64_t stride, const uint8_t *__restrict__ rreal, uint64_t n,
                                                  uint8_t *__restrict__ lcs)
{
    const uint64_t i = (uint64_t)blockIdx.x * kBT + threadIdx.x;
    if (i >= n) return;
    if (i == 0) { lcs[0] = 0u; return; }
    uint64_t a[W], b[W];
    ld_key(rk, stride, i, a);
    ld_key(rk, stride, i - 1u, b);
    uint32_t cd = 32u * W;
#pragma unroll
    for (int j = W - 1; j >= 0; j--) { // (the first differing word decides)
        const uint64_t x = a[j] ^ b[j];
        if (x) cd = 32u * (uint32_t)j + ((uint32_t)__clzll(x) >> 1);
    }
    lcs[i] = (uint8_t)min(cd, min((uint32_t)rreal[i], (uint32_t)rreal[i - 1u]));
}

inline dim3 grid_of(uint64_t n) { return dim3((uint32_t)((n + kBT - 1u) / kBT)); }

template <int W> struct Launch {
    static void extract(const uint8_t *seq, uint64_t n_bytes, uint32_t k, bool fw, bool rc, uint64_t *keys, uint64_t stride,
                        unsigned long long *count, hipStream_t s)
    {
        const uint64_t tiles = (n_bytes + kExtTile - 1u) / kExtTile;
        if (tiles) hipLaunchKernelGGL(extract_kernel<W>, dim3((uint32_t)tiles), dim3(kBT), 0, s, seq, n_bytes, k, fw ? 1u : 0u, rc ? 1u : 0u, keys, stride, count);
    }
    static void flag_distinct(const uint64_t *keys, uint64_t stride, const uint8_t *real, uint64_t n, uint8_t *flags, hipStream_t s)
    {
        hipLaunchKernelGGL(flag_distinct_kernel<W>, grid_of(n), dim3(kBT), 0, s, keys, stride, real, n, flags);
    }
    static void flag_orphan(const uint64_t *keys, uint64_t stride, uint64_t n, uint32_t k, uint8_t *flags, hipStream_t s)
    {
        hipLaunchKernelGGL(flag_orphan_kernel<W>, grid_of(n), dim3(kBT), 0, s, keys, stride, n, k, flags);
    }
    static void dummies(const uint64_t *orph, uint64_t o_stride, uint64_t n_orph, uint32_t k, uint64_t *keys, uint64_t stride, uint8_t *real, hipStream_t s)
    {
        hipLaunchKernelGGL(dummy_kernel<W>, grid_of(1u + n_orph * (k - 1u)), dim3(kBT), 0, s, orph, o_stride, n_orph, k, keys, stride, real);
    }
    static void merge(const uint64_t *km, uint64_t km_stride, uint64_t n_km, uint32_t k, const uint64_t *dk, uint64_t d_stride, const uint8_t *dreal,
                      uint64_t n_d, uint32_t *lb, uint64_t *rk, uint64_t r_stride, uint8_t *rreal, hipStream_t s)
    {
        hipLaunchKernelGGL(merge_dummy_kernel<W>, grid_of(n_d), dim3(kBT), 0, s, km, km_stride, n_km, dk, d_stride, dreal, n_d, lb, rk, r_stride, rreal);
        if (n_km) hipLaunchKernelGGL(merge_kmer_kernel<W>, grid_of(n_km), dim3(kBT), 0, s, km, km_stride, n_km, k, lb, n_d, rk, r_stride, rreal);
    }
    static void edges(const uint64_t *rk, uint64_t stride, const uint8_t *rreal, uint64_t n, uint32_t k, uint64_t *rows, uint64_t n_words,
                      unsigned long long *ctr, hipStream_t s)
    {
        hipLaunchKernelGGL(edge_kernel<W>, grid_of(n), dim3(kBT), 0, s, rk, stride, rreal, n, k, rows, n_words, ctr);
    }
    static void lcs(const uint64_t *rk, uint64_t stride, const uint8_t *rreal, uint64_t n, uint8_t *out, hipStream_t s)
    {
        hipLaunchKernelGGL(lcs_kernel<W>, grid_of(n), dim3(kBT), 0, s, rk, stride, rreal, n, out);
    }
};

template <typename F> void by_words(uint32_t W, F f)
{
    if (W == 1) f(Launch<1>());
    else if (W == 2) f(Launch<2>());
    else if (W == 4) f(Launch<4>());
    else f(Launch<8>());
}

} // namespace

size_t build_tiles(uint64_t n) { return (size_t)((n + kBuildTile - 1u) / kBuildTile); }

hipError_t launch_build_extract(uint32_t W, const uint8_t *d_seq, uint64_t n_bytes, uint32_t k, bool fw, bool rc, uint64_t *d_keys,
                                uint64_t stride, unsigned long long *d_count, hipStream_t s)
{
    by_words(W, [&](auto L) { L.extract(d_seq, n_bytes, k, fw, rc, d_keys, stride, d_count, s); });
    return hipGetLastError();
}

hipError_t launch_build_radix_pass(const uint64_t *d_in, uint64_t *d_out, uint32_t n_words, uint64_t stride, const uint8_t *d_rin, uint8_t *d_rout,
                                   uint64_t n, const RadixPass &ps, uint32_t *d_hist, uint32_t *d_sums, hipStream_t s)
{
    const uint32_t tiles = (uint32_t)build_tiles(n);
    if (!tiles) return hipSuccess;
    hipLaunchKernelGGL(radix_hist_kernel, dim3(tiles), dim3(kBT), 0, s, d_in, stride, d_rin, n, ps, tiles, d_hist);
    hipError_t e = launch_scan(d_hist, 256u * tiles, d_sums, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(radix_scatter_kernel, dim3(tiles), dim3(kBT), 0, s, d_in, d_out, n_words, stride, d_rin, d_rout, n, ps, tiles, d_hist, d_sums);
    return hipGetLastError();
}

hipError_t launch_build_flag_distinct(uint32_t W, const uint64_t *d_keys, uint64_t stride, const uint8_t *d_real, uint64_t n, uint8_t *d_flags, hipStream_t s)
{
    if (n) by_words(W, [&](auto L) { L.flag_distinct(d_keys, stride, d_real, n, d_flags, s); });
    return hipGetLastError();
}

hipError_t launch_build_flag_orphan(uint32_t W, const uint64_t *d_keys, uint64_t stride, uint64_t n, uint32_t k, uint8_t *d_flags, hipStream_t s)
{
    if (n) by_words(W, [&](auto L) { L.flag_orphan(d_keys, stride, n, k, d_flags, s); });
    return hipGetLastError();
}

hipError_t launch_build_compact(const uint64_t *d_in, uint64_t in_stride, uint64_t *d_out, uint64_t out_stride, uint32_t n_words, const uint8_t *d_rin,
                                uint8_t *d_rout, const uint8_t *d_flags, uint64_t n, uint32_t *d_counts, uint32_t *d_sums,
                                unsigned long long *d_total, hipStream_t s)
{
    const uint32_t tiles = (uint32_t)build_tiles(n);
    if (!tiles) return hipSuccess;
    hipLaunchKernelGGL(compact_count_kernel, dim3(tiles), dim3(kBT), 0, s, d_flags, n, d_counts, d_total);
    hipError_t e = launch_scan(d_counts, tiles, d_sums, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(compact_kernel, dim3(tiles), dim3(kBT), 0, s, d_in, in_stride, d_out, out_stride, n_words, d_rin, d_rout, d_flags, n, d_counts, d_sums);
    return hipGetLastError();
}

hipError_t launch_build_dummies(uint32_t W, const uint64_t *d_orph, uint64_t o_stride, uint64_t n_orph, uint32_t k, uint64_t *d_keys, uint64_t stride,
                                uint8_t *d_real, hipStream_t s)
{
    by_words(W, [&](auto L) { L.dummies(d_orph, o_stride, n_orph, k, d_keys, stride, d_real, s); });
    return hipGetLastError();
}

hipError_t launch_build_merge(uint32_t W, const uint64_t *d_km, uint64_t km_stride, uint64_t n_km, uint32_t k, const uint64_t *d_dk, uint64_t d_stride,
                              const uint8_t *d_dreal, uint64_t n_d, uint32_t *d_lb, uint64_t *d_rk, uint64_t r_stride, uint8_t *d_rreal, hipStream_t s)
{
    by_words(W, [&](auto L) { L.merge(d_km, km_stride, n_km, k, d_dk, d_stride, d_dreal, n_d, d_lb, d_rk, r_stride, d_rreal, s); });
    return hipGetLastError();
}

hipError_t launch_build_edges_lcs(uint32_t W, const uint64_t *d_rk, uint64_t stride, const uint8_t *d_rreal, uint64_t n, uint32_t k, uint64_t *d_rows,
                                  uint64_t n_words, uint8_t *d_lcs, unsigned long long *d_ctr, hipStream_t s)
{
    by_words(W, [&](auto L) {
        L.edges(d_rk, stride, d_rreal, n, k, d_rows, n_words, d_ctr, s);
        L.lcs(d_rk, stride, d_rreal, n, d_lcs, s);
    });
    hipLaunchKernelGGL(popc_kernel, dim3((uint32_t)((n_words + kBT - 1u) / kBT), 4), dim3(kBT), 0, s, d_rows, n_words, d_ctr);
    return hipGetLastError();
}

} // namespace kbo
