// refset_step.hpp — one base of the k-bounded matching statistics against the packed form of a reference (kernels.hpp "LDS form":
// 8-byte rank blocks { C[c] + rank_c(32 b), 32 row bits }, then the LCS bytes with the sentinel LCS[n] = 0), for host and device
// alike: refset_kernels.hip and refset_wide_kernels.hip run it a chunk per lane (refset_walk.hpp) with the form in LDS and in global
// memory, refset.cpp's kbo_refset_ms_host runs it over the host arena, tools/refset_step_check.cpp through an accessor that checks
// every index.
//
// The state is the interval [l, r) of the rows whose k-mer ends with the longest suffix of the bases so far that some row ends with,
// and d, that suffix's length (at most k):
//   extend    [l, r) by c  ->  [rank_c(l), rank_c(r)): one entry and a population count per rank (the entry's count has C[c] in it)
//   contract               ->  m = min(max(LCS[l], LCS[r]), d - 1); m == 0 is the root [0, n); otherwise l goes down and r goes up
//                              while their LCS bytes are >= m, and d = m (the levels between d and m leave the interval as it is, so
//                              the reference's loop of single levels, index.rs:243-256, fails its extension at each: they are skipped)
// The scans are linear in the LCS bytes.  An accessor has
//   Entry rank(uint32_t block, uint32_t c)   entry c of rank block `block` (block <= n / 32)
//   uint32_t lcs(uint32_t i)                 LCS byte i (i <= n; LCS[0] = LCS[n] = 0 end the scans)
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define KBO_ST_FN __host__ __device__ __forceinline__
#else
#define KBO_ST_FN inline
#endif

namespace kbo {
namespace refstep {

struct Entry {
    uint32_t count, bits;
};

// A, C, G, T -> 0 .. 3; any other byte, lower case included -> 4 (device_util.hpp decode_base)
KBO_ST_FN uint32_t base_code(uint32_t ch)
{
    const uint32_t c = ((ch >> 1) & 3u) ^ ((ch >> 2) & 1u);
    const uint32_t back = (0x54474341u >> (8u * c)) & 0xFFu;
    return back == ch ? c : 4u;
}

template <typename Acc> KBO_ST_FN uint32_t rank_of(const Acc &x, uint32_t c, uint32_t i)
{
    const Entry e = x.rank(i >> 5, c);
    return e.count + (uint32_t)__builtin_popcount(e.bits & ((1u << (i & 31u)) - 1u));
}

// one base ch of the query against a form of n rows
template <typename Acc> KBO_ST_FN void step(const Acc &x, uint32_t n, uint32_t k, uint32_t ch, uint32_t &l, uint32_t &r, uint32_t &d)
{
    const uint32_t c = base_code(ch);
    if (c > 3u) { // no row continues with a byte that is no base: every level fails
        l = 0;
        r = n;
        d = 0;
        return;
    }
    for (;;) {
        const uint32_t nl = rank_of(x, c, l), nr = rank_of(x, c, r);
        if (nl < nr) {
            l = nl;
            r = nr;
            d = d + 1u < k ? d + 1u : k;
            return;
        }
        if (d == 0) return;
        const uint32_t a = x.lcs(l), b = x.lcs(r), top = a > b ? a : b;
        const uint32_t m = top < d - 1u ? top : d - 1u;
        if (m == 0) {
            l = 0;
            r = n;
        } else {
            while (x.lcs(l) >= m) l--;
            while (x.lcs(r) >= m) r++;
        }
        d = m;
    }
}

} // namespace refstep
} // namespace kbo
