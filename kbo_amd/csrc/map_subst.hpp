// map_subst.hpp — a lone substitution in a read, settled by one bit per text position; for host and device alike.
//
// Stage 3 of map_reads_kernel (map_kernels.hip) proves for every mismatch of a read that no string of thr + 1 bases through it is in
// the index: the windows of `order` bases that end at the mismatch's base m and at up to three bases behind it (window_offset) must
// each not be the suffix of any row (bit 7 of their depth-table entries clear).  Where the mismatch is a LONE substitution on the
// read's one diagonal p0 - no other entry of the read's list within order - 1 bases of it on either side - each of those windows is
// the text's own window around position p = p0 + m with the one base at p replaced.  Whether any such one-base neighbour is in the
// index depends on the index alone, so the device copy answers it once per text position: sub_clean, a bit per position, set where
//   (a) no position in [p - (order - 1), p + (order - 1)] carries a mark or lies outside the text, and
//   (b) for each of the three bases b != text[p] and every window offset o, the string text[p + o - order + 1 .. p + o] with b at p
//       is no suffix of a row.
// A set bit answers every window of the proof "absent" (a window the read's ends cut off is not asked at all: a subset).  A clear
// bit promises nothing - the kernel asks the table as before -, so only a wrongly SET bit could change a result:
// tools/map_subst_check.cpp compares clean() with a brute-force set of strings over every placement of a read.
//
// The bit of a mismatch is bit_of(p0, m): position p0 + m counted from the first unit's first position (the padding of kPad
// positions in front of the text handled here and nowhere else), as compare_split's q0 is (map_text.hpp).
//
// Accessors of clean() (the device's are loads, the check program's check the index first):
//   Text    uint64_t positions()          positions of the padded text (16 per unit)
//           bool marked(uint64_t q)       whether position q matches nothing (a path start, the padding)
//           uint32_t base(uint64_t q)     its 2-bit digit
//   Table   bool present(uint64_t key)    whether the string of `order` bases (first base most significant) is a suffix of a row
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define KBO_MS_FN __host__ __device__ __forceinline__
#else
#define KBO_MS_FN inline
#endif

namespace kbo {
namespace mapsubst {

constexpr uint32_t kWindows = 4; // windows of a break's proof at most (map_reads_direct admits no threshold that needs more)
constexpr uint32_t kPad = 192;   // positions in front of text position 0 (== kMapPad)

// ---- the windows of a break's proof.  cov: bases between two of them - every string of thr + 1 bases through the break holds one;
// with anchors (have_anch) two bases closer, so that one of them may be present as long as its exact depth is at most order + 1.
// jn: the bases of the break beyond its first (a mismatch: 0; the junction of two diagonals: 1 + the bases that lie on both)
KBO_MS_FN uint32_t window_step(uint32_t order, uint32_t thr, bool have_anch) { return have_anch ? thr - order : thr - order + 2u; }
// bases behind the break's last base at which window i ends (the last one is clamped: it starts at the break)
KBO_MS_FN uint32_t window_offset(uint32_t i, uint32_t cov, uint32_t order, uint32_t jn) { return i * cov < order - 1u - jn ? i * cov : order - 1u - jn; }
// whether window i is one of the proof's (not the clamped window again)
KBO_MS_FN bool window_used(uint32_t i, uint32_t cov, uint32_t order, uint32_t jn) { return i == 0u || (i - 1u) * cov < order - 1u - jn; }
// whether window i starts at the break: nothing of the read stands in it in front of the break
KBO_MS_FN bool window_last(uint32_t i, uint32_t cov, uint32_t order, uint32_t jn) { return i * cov >= order - 1u - jn; }

// ---- which mismatches the bit speaks for.  m: the read's base; prev / next: the list entries around it (has_prev / has_next: whether
// there are any); block_mode: the read has no diagonal (no seed, a chance seed); cut: its bases lie on two diagonals (stage 2b cut it
// - also where the cut merged with a mismatch and left no junction entry); junction: the entry is the cut itself
KBO_MS_FN bool eligible(bool block_mode, bool cut, bool junction, bool has_prev, uint32_t prev, uint32_t m, bool has_next, uint32_t next, uint32_t order)
{
    return !block_mode && !cut && !junction && (!has_prev || m - prev > order - 1u) && (!has_next || next - m > order - 1u);
}

// ---- the bitmap
KBO_MS_FN uint64_t bit_of(uint32_t p0, uint32_t m) { return (uint64_t)(uint32_t)(p0 + m + kPad); }
KBO_MS_FN uint64_t bitmap_words(uint64_t n_units) { return (n_units + 1u) / 2u; } // a bit per position, 16 positions a unit
// Bits: uint32_t word(uint64_t w)
template <class Bits> KBO_MS_FN bool clean_bit(const Bits &bits, uint64_t q) { return (bits.word(q >> 5) >> (uint32_t)(q & 31u)) & 1u; }

// ---- the definition of clean (header), for position q counted like bit_of's result
// (leave_out: bit i = window i is not asked - only tools/map_subst_check.cpp sets it, to see its own check fail)
template <class Text, class Table>
KBO_MS_FN bool clean(const Text &tx, const Table &tab, uint64_t q, uint32_t order, uint32_t thr, bool have_anch, uint32_t leave_out = 0u)
{
    if (order < 2u || order > 32u || thr < order || (have_anch && thr == order)) return false;
    if (q + 1u < order || q + order > tx.positions()) return false;
    for (uint64_t x = q + 1u - order; x < q + order; x++)
        if (tx.marked(x)) return false;
    const uint32_t cov = window_step(order, thr, have_anch), own = tx.base(q);
    for (uint32_t i = 0; i < kWindows; i++) {
        if (!window_used(i, cov, order, 0u) || ((leave_out >> i) & 1u)) continue;
        const uint32_t o = window_offset(i, cov, order, 0u); // position q is base o from the window's end
        uint64_t key = 0;
        for (uint32_t j = 0; j < order; j++) key = (key << 2) | tx.base(q + o + 1u - order + j);
        for (uint32_t b = 0; b < 4u; b++) {
            if (b == own) continue;
            if (tab.present((key & ~(3ull << (2u * o))) | ((uint64_t)b << (2u * o)))) return false;
        }
    }
    // (a proof of more than kWindows windows: not this kernel's - map_reads_direct)
    return !window_used(kWindows, cov, order, 0u);
}

// ---- clean GROUPS: a coarser bitmap next to the bits, sub_group - bit G set when the kGroup bits of positions kGroup G ..
// kGroup G + kGroup - 1 (counted like bit_of's result, padding included) are all set.  A set group bit implies the position's own
// bit, so it settles a lone substitution by the same proof; a clear one promises nothing.  A read's whole window of groups is ONE
// byte-aligned load of 8 bytes that depends on nothing but its diagonal: stage 2 of map_reads_kernel issues it beside the text's, and
// the read's own lane settles its list before stage 3 deals what is left.
//   q0 = p0 + kPad, the window's first position; its first group q0 / 4 lies in byte q0 / 32 of the array, at bit (q0 / 4) mod 8
//   base m <= 159 of the read: bit (q0 + m) / 4 - 8 (q0 / 32) of the 64 loaded ones, at most (31 + 159) / 4 = 47
//   the load's byte offset: at most group_load_max(units) for any q0 inside the padded text; behind the array's 4 group_words(units)
//   bytes lie kGroupSlack zeroed ones (a window near the text's end reads into them: no group there is clean)
constexpr uint32_t kGroup = 4, kGroupSlack = 64;
KBO_MS_FN uint64_t group_of(uint64_t q) { return q / kGroup; }
KBO_MS_FN uint64_t group_words(uint64_t n_units) { return (n_units * (16u / kGroup) + 31u) / 32u; }
KBO_MS_FN uint64_t group_load_byte(uint32_t q0) { return group_of(q0) >> 3; }
KBO_MS_FN uint64_t group_load_max(uint64_t n_units) { return group_of(16u * n_units - 1u) >> 3; }
KBO_MS_FN bool group_in_window(uint64_t loaded, uint32_t q0, uint32_t m)
{
    return (loaded >> (uint32_t)(group_of((uint64_t)q0 + m) - 8u * group_load_byte(q0))) & 1u;
}
// the 32 / kGroup group bits of one word of position bits (any_bit: an OR where the rule says AND - only tools/map_group_check.cpp
// sets it, to see its own check fail)
KBO_MS_FN uint32_t group_bits_of_word(uint32_t w, bool any_bit = false)
{
    uint32_t out = 0;
    for (uint32_t j = 0; j < 32u / kGroup; j++) {
        const uint32_t f = (w >> (kGroup * j)) & ((1u << kGroup) - 1u);
        if (any_bit ? f != 0u : f == (1u << kGroup) - 1u) out |= 1u << j;
    }
    return out;
}
// word W of the group bitmap from the position bits (Bits: uint32_t word(uint64_t w), zero behind its last word)
template <class Bits> KBO_MS_FN uint32_t group_word(const Bits &bits, uint64_t W, uint64_t n_bit_words, bool any_bit = false)
{
    uint32_t out = 0;
    for (uint32_t i = 0; i < kGroup; i++) {
        const uint64_t w = kGroup * W + i;
        if (w < n_bit_words) out |= group_bits_of_word(bits.word(w), any_bit) << (32u / kGroup * i);
    }
    return out;
}
// ---- dealing what is left of a read's list: `settled` has bit i set for entry i; -> the list index of the t-th entry that is not
KBO_MS_FN uint32_t nth_unsettled(uint32_t settled, uint32_t t)
{
    uint32_t open = ~settled;
    for (uint32_t i = 0; i < t; i++) open &= open - 1u;
    return (uint32_t)__builtin_ctz(open);
}

} // namespace mapsubst
} // namespace kbo
