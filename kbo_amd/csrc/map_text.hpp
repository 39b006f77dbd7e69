// map_text.hpp — the window of the 2-bit text that map_reads_kernel (map_kernels.hip) compares a read with, for host and device alike.
//
// The path-cover text lies in units of 16 positions, unit u = positions [16 u - kMapPad, + 16), in two layouts:
//   interleaved   pc_tm[u] = { digits, marks }: 32 bits of 2-bit digits (the first position most significant) and 01 at every position
//                 that matches nothing (a path start, the padding).  8 bytes a unit; map_long_kernel reads it
//   split         pc_t[u] = the digits word alone (4 bytes a unit), and pc_mu: one bit per unit, set where pc_tm[u].y != 0 (and for
//                 every unit behind the last).  Marks are rare - a path start per contig, the padding - so a window asks pc_mu whether
//                 any of its units has one, and takes the marks of exactly those units from pc_tm.  And even that look costs the kernel
//                 a gathered load per read, so a coarse summary stands in front of it: pc_mc, kCells bits - a word per lane of a wave,
//                 held in a register -, bit c set where a window that starts in cell c (2^shift units) can see a marked unit
// Both forms give the same mismatch words for every window the kernel can form: tools/map_text_check.cpp compares them over every
// diagonal, length and alignment, through accessors that check every index.
//
// Accessors (the kernel's are loads, the check program's check the index first):
//   Units   void pair(uint64_t u, uint32_t (&d)[2], uint32_t (&m)[2])   digits and marks of units u, u + 1 of pc_tm (one 16-byte load)
//           void unit(uint64_t u, uint32_t &d, uint32_t &m)             ... of unit u
//           uint32_t marks(uint64_t u)                                  pc_tm[u].y
//   Digits  void quad(uint64_t u, uint32_t (&d)[4])                     pc_t[u .. u + 3] (one 16-byte load at a 4-byte boundary)
//           uint32_t word(uint64_t u)                                   pc_t[u]
//   Bits    uint32_t from(uint64_t u)                                   bit i = pc_mu's bit of unit u + i, for i < 25 (the four bytes from
//                                                                       byte u / 8 on)
//           (near: the coarse summary's bit of the window's first unit - cell_of -, looked up by the caller: false = no mark in sight)
//   Any     bool operator()(bool b)                                     whether b holds anywhere the marked path would be taken together:
//                                                                       a ballot over the wave in the kernel, b itself on the host
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define KBO_MT_FN __host__ __device__ __forceinline__
#else
#define KBO_MT_FN inline
#endif

namespace kbo {
namespace maptext {

constexpr uint32_t kWords = 10;     // 16-base words of a read (== kMapWords: reads of up to 160 bases)
constexpr uint32_t kUnits = 12;     // units a window's loads cover; its bases touch at most eleven of them
constexpr uint32_t kBeside = 3;     // units of stage 2b's look beside the diagonal
constexpr uint32_t kCells = 2048;   // bits of the coarse summary pc_mc

// the 16 positions from position r of unit `hi` on (lo = the unit behind it)
KBO_MT_FN uint32_t shifted(uint32_t hi, uint32_t lo, uint32_t r) { return (uint32_t)((((uint64_t)hi << 32) | lo) >> (32u - 2u * r)); }
// bit 2 (15 - j) for each of the first nb of 16 positions
KBO_MT_FN uint32_t first_bases(uint32_t nb) { return nb < 16u ? (~0u << (32u - 2u * nb)) & 0x55555555u : 0x55555555u; }
// units that the len >= 1 positions from position r of a unit on touch
KBO_MT_FN uint32_t units_touched(uint32_t r, uint32_t len) { return ((r + len - 1u) >> 4) + 1u; }

// ---- the coarse summary: cells of 2^shift units, the fewest (but whole words of pc_mu) with which kCells cells cover the text
KBO_MT_FN uint32_t cell_shift(uint64_t n_units)
{
    uint32_t s = 5;
    while (((uint64_t)kCells << s) < n_units) s++;
    return s;
}
KBO_MT_FN uint32_t cell_of(uint64_t u, uint32_t shift) { return (uint32_t)(u >> shift); }
// whether a window (kUnits units at most) that starts in cell c can see a marked unit, or a unit behind the last
template <class Bits> KBO_MT_FN bool cell_marked(const Bits &mu, uint64_t c, uint32_t shift, uint64_t n_units)
{
    const uint64_t lo = c << shift, hi = ((c + 1u) << shift) + kUnits - 1u; // units [lo, hi)
    if (hi > n_units) return true;
    for (uint64_t u = lo; u < hi; u += 24u) {
        const uint64_t n = hi - u < 24u ? hi - u : 24u;
        if (mu.from(u) & ((1u << n) - 1u)) return true;
    }
    return false;
}

// ---- the compare step: mm[g] has bit 2 (15 - j) set where base 16 g + j of the read (qw: its 16-base words) differs from the text at
// position q0 + 16 g + j (q0 counted from the first unit's first position), or the text has a mark there; -> the bits set
template <class Units> KBO_MT_FN uint32_t compare_interleaved(const Units &tm, const uint32_t (&qw)[kWords], uint64_t q0, uint32_t len, uint32_t (&mm)[kWords])
{
    const uint32_t r = (uint32_t)(q0 & 15u);
    uint32_t T[kUnits], M[kUnits];
#pragma unroll
    for (uint32_t i = 0; i < kUnits / 2u; i++) {
        uint32_t d[2], m[2];
        tm.pair((q0 >> 4) + 2u * i, d, m);
        T[2u * i] = d[0];
        T[2u * i + 1u] = d[1];
        M[2u * i] = m[0];
        M[2u * i + 1u] = m[1];
    }
    uint32_t c = 0;
#pragma unroll
    for (uint32_t g = 0; g < kWords; g++) {
        mm[g] = 0;
        if (16u * g < len) {
            const uint32_t x = qw[g] ^ shifted(T[g], T[g + 1u], r);
            mm[g] = (x | (x >> 1) | shifted(M[g], M[g + 1u], r)) & first_bases(len - 16u * g);
            c += (uint32_t)__builtin_popcount(mm[g]);
        }
    }
    return c;
}

template <class Digits, class Bits, class Units, class Any>
KBO_MT_FN uint32_t compare_split(const Digits &tx, const Bits &mu, const Units &tm, const Any &any, bool near, const uint32_t (&qw)[kWords], uint64_t q0,
                                 uint32_t len, uint32_t (&mm)[kWords])
{
    const uint32_t r = (uint32_t)(q0 & 15u);
    const uint64_t u0 = q0 >> 4;
    uint32_t T[kUnits];
#pragma unroll
    for (uint32_t i = 0; i < kUnits / 4u; i++) {
        uint32_t d[4];
        tx.quad(u0 + 4u * i, d);
#pragma unroll
        for (uint32_t j = 0; j < 4u; j++) T[4u * i + j] = d[j];
    }
#pragma unroll
    for (uint32_t g = 0; g < kWords; g++) {
        mm[g] = 0;
        if (16u * g < len) {
            const uint32_t x = qw[g] ^ shifted(T[g], T[g + 1u], r);
            mm[g] = (x | (x >> 1)) & first_bases(len - 16u * g);
        }
    }
    if (any(near)) { // (rare: a window near a path start or the padding)
        // (only the units the read's bases touch: a mark beyond them is masked out of the interleaved form's words as well)
        const uint32_t marked = near ? mu.from(u0) & ((1u << units_touched(r, len)) - 1u) : 0u;
        if (marked != 0u) {
            uint32_t M[kUnits];
#pragma unroll
            for (uint32_t i = 0; i < kUnits; i++) M[i] = (i + 1u < kUnits && ((marked >> i) & 1u)) ? tm.marks(u0 + i) : 0u;
#pragma unroll
            for (uint32_t g = 0; g < kWords; g++)
                if (16u * g < len) mm[g] |= shifted(M[g], M[g + 1u], r) & first_bases(len - 16u * g);
        }
    }
    uint32_t c = 0;
#pragma unroll
    for (uint32_t g = 0; g < kWords; g++) c += (uint32_t)__builtin_popcount(mm[g]);
    return c;
}

// ---- stage 2b's look beside the diagonal: three units from unit u on
template <class Units> KBO_MT_FN void beside_interleaved(const Units &tm, uint64_t u, uint32_t (&d)[kBeside], uint32_t (&m)[kBeside])
{
#pragma unroll
    for (uint32_t i = 0; i < kBeside; i++) tm.unit(u + i, d[i], m[i]);
}

template <class Digits, class Bits, class Units, class Any>
KBO_MT_FN void beside_split(const Digits &tx, const Bits &mu, const Units &tm, const Any &any, bool near, uint64_t u, uint32_t (&d)[kBeside],
                            uint32_t (&m)[kBeside])
{
#pragma unroll
    for (uint32_t i = 0; i < kBeside; i++) {
        d[i] = tx.word(u + i);
        m[i] = 0u;
    }
    if (any(near)) {
        const uint32_t marked = near ? mu.from(u) & ((1u << kBeside) - 1u) : 0u;
#pragma unroll
        for (uint32_t i = 0; i < kBeside; i++)
            if ((marked >> i) & 1u) m[i] = tm.marks(u + i);
    }
}

// 16 bases (`word`) against the text one to three positions to either side of position qb + 3 of the units d / m (qb counted like q0;
// only its place in its unit matters): -> the fewest mismatches over the six shifts, best_j = that shift + 3.  A shift on which the
// eight bases `end8` all match wins when none has fewer than three mismatches (a break within 16 bases of that end)
KBO_MT_FN uint32_t beside_best(const uint32_t (&d)[kBeside], const uint32_t (&m)[kBeside], uint32_t qb, uint32_t word, uint32_t end8, uint32_t &best_j)
{
    uint32_t best = 99u, j8 = 3u;
    best_j = 3u;
#pragma unroll
    for (uint32_t j = 0; j < 7u; j++) {
        if (j == 3u) continue;
        const uint32_t rel = (qb & 15u) + j, r = rel & 15u;
        const uint32_t x = word ^ shifted(rel < 16u ? d[0] : d[1], rel < 16u ? d[1] : d[2], r);
        const uint32_t mb = (x | (x >> 1) | shifted(rel < 16u ? m[0] : m[1], rel < 16u ? m[1] : m[2], r)) & 0x55555555u;
        const uint32_t c = (uint32_t)__builtin_popcount(mb);
        if (c < best) {
            best = c;
            best_j = j;
        }
        if ((mb & end8) == 0u) j8 = j;
    }
    if (best > 2u && j8 != 3u) {
        best = 0u;
        best_j = j8;
    }
    return best;
}

} // namespace maptext
} // namespace kbo
