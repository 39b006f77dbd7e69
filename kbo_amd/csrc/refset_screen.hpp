// refset_screen.hpp — the seed screen of a reference set (kbo_hip.h "screen pairs by shared seeds"), for host and
// device alike: refset_screen_kernels.hip runs it a run of start positions per lane, refset.cpp builds the table with it and restates
// the screen on the CPU (kbo_refset_candidates_host), tools/refset_screen_check.cpp runs it through an accessor that checks every
// index.
//
// A SEED at a position is the 2-bit code of the next up to kSeedMax bases, the first base in the most significant of 48 bits, and
// how many of them are valid (`len`): the stretch or the sequence ends there, or a byte that refstep::base_code maps to 4 follows.
// The positions behind `len` hold zeros.  The table has one entry per start position of every indexed stretch of every packed
// reference - key = code << 16 | len, and the reference - sorted by key, and a direct-address array of kBuckets + 1 offsets by the
// first kSeedMin bases.  Two seeds share a prefix of
//   min(len_a, len_b, leading zero bit pairs of code_a ^ code_b)
// bases.  A pair (reference r, sequence, strand) is a candidate when some position of the sequence shares at least m_r bases with
// some entry of r; m_r >= kSeedMin, so both lie in one bucket.
// The state goes from RIGHT to LEFT over a sequence: the seed at i is base i in front of the seed at i + 1, cut to kSeedMax.
// An accessor has
//   uint32_t bucket(uint32_t b)     offset b of the bucket array (b <= kBuckets)
//   uint64_t key(uint32_t x)        key of entry x
//   uint32_t ref(uint32_t x)        reference of entry x
#pragma once
#include <stdint.h>

#include "refset_step.hpp"

namespace kbo {
namespace refscreen {

constexpr uint32_t kSeedMax = 24; // == KBO_REFSET_SEED_MAX: bases of a code (48 bits)
constexpr uint32_t kSeedMin = 11; // == KBO_REFSET_SEED_MIN: bases that address a bucket
constexpr uint32_t kBuckets = 1u << (2u * kSeedMin);
constexpr uint32_t kUnfilterable = 255; // m of a reference the kernel never marks (no entries, or m_r < kSeedMin: the host decides)

struct Seed {
    uint64_t code; // 48 bits, first base highest
    uint32_t len;  // valid bases, <= kSeedMax
};

// the seed one position to the left: byte ch in front of s
KBO_ST_FN Seed step_left(Seed s, uint32_t ch)
{
    const uint32_t c = refstep::base_code(ch);
    if (c > 3u) return Seed{0u, 0u};
    // (a full seed loses its last base; a shorter one has zeros behind its bases and keeps them)
    return Seed{(uint64_t)c << 46 | s.code >> 2, s.len < kSeedMax ? s.len + 1u : kSeedMax};
}

KBO_ST_FN uint64_t key_of(Seed s) { return s.code << 16 | s.len; }
KBO_ST_FN uint32_t bucket_of(uint64_t code) { return (uint32_t)(code >> (48u - 2u * kSeedMin)); }

// bases a seed shares with the entry of `key`
KBO_ST_FN uint32_t common_prefix(Seed s, uint64_t key)
{
    const uint64_t x = s.code ^ key >> 16;
    const uint32_t klen = (uint32_t)(key & 0xFFFFu);
    uint32_t n = x ? ((uint32_t)__builtin_clzll(x) - 16u) / 2u : kSeedMax;
    n = n < s.len ? n : s.len;
    return n < klen ? n : klen;
}

// m_r of a call: the seed length a record of reference r needs (threshold t, derandomize.rs:282-285: a value > t or == k is kept)
KBO_ST_FN uint32_t seed_len(uint32_t threshold, uint32_t k)
{
    uint32_t m = threshold + 1u < k ? threshold + 1u : k;
    return m < kSeedMax ? m : kSeedMax;
}

// every entry of the seed's bucket: hit(reference, shared bases).  Nothing is looked up for a seed of fewer than kSeedMin bases
template <typename Acc, typename Hit> KBO_ST_FN void scan(const Acc &x, Seed s, Hit &&hit)
{
    if (s.len < kSeedMin) return;
    const uint32_t b = bucket_of(s.code);
    const uint32_t end = x.bucket(b + 1u);
    for (uint32_t e = x.bucket(b); e < end; e++) hit(x.ref(e), common_prefix(s, x.key(e)));
}

} // namespace refscreen
} // namespace kbo
