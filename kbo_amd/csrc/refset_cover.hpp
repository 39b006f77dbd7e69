// refset_cover.hpp — depth and breadth of every reference of a set over a list of runs (kbo_hip.h "The COVER of a reference";
// DESIGN.md 4.12), for host and device alike: refset_cover_kernels.hip runs it a wave per run and a wave per reference, refset.cpp
// makes the base offsets, refset_runs.cpp restates the call on the CPU (kbo_cover_refset_host) and writes a call without runs,
// tools/refset_cover_check.cpp runs it through accessors that check every index.
//
// Three steps over one array of 32-bit words, H, that holds L_r words for every reference r with entries, reference r's from
// base_off[r] on (refset_locate.hpp says what an entry and an anchor are):
//   count   H[p] += 1 for every anchor of every usable run whose entry has position p; the reference's counters take the run, its
//           anchors and those among them with MULTI.  Additions only, so the order of the runs does not matter
//   scan    in place, per reference: S[j] = H[0] + ... + H[j] modulo 2^32, kTile words at a time with the sum so far carried along
//   reduce  D[j] = S[j] - S[j - k] (S[j] for j < k): the anchors whose k-mer covers base j.  Exact whenever the reference's anchors
//           are fewer than 2^32, the differences of sums modulo 2^32 being the sums of at most k of the H.  A tile of kTile bases
//           becomes two masks - the covered bases, and those among them that begin a segment - and its largest D; tile_add folds
//           them into the reference's Tally, the same way in the kernel (the masks are ballots) and in the serial forms here
// Accessors: Words    uint32_t get(uint64_t i), void set(uint64_t i, uint32_t v), void add(uint64_t i)   i < the words of H
//            DepthOut void put(uint64_t i, uint32_t v)                                                    the optional profile
#pragma once
#include <stdint.h>

#include "refset_locate.hpp"

namespace kbo {
namespace refcover {

constexpr uint32_t kTile = 64;                      // bases a step of the scan and of the reduce: a wave's lanes
constexpr uint32_t kFlagNoEntries = 1u, kFlagOverflow = 2u;
constexpr uint32_t kNone = reflocate::kPosNone;     // == KBO_LOCUS_NONE
constexpr uint32_t kCounterBytes = 24;              // a reference's counters in d_work: n_anchors, n_multi (u64), n_runs (u32), padding

struct Cover { // == kbo_ref_cover
    uint32_t ref_len, covered, n_segments, first, last, max_depth, n_runs, flags;
    uint64_t n_anchors, n_multi;
};

struct Tally { // what the reduce carries from tile to tile
    uint32_t covered, segments, first, last, max_depth;
};
KBO_ST_FN Tally no_tally() { return Tally{0u, 0u, kNone, kNone, 0u}; }

// the words of d_work in front of H: the counters of n_refs references, a multiple of 16 bytes
KBO_ST_FN uint64_t counter_bytes(uint64_t n_refs) { return (n_refs * kCounterBytes + 15u) / 16u * 16u; }
KBO_ST_FN uint64_t work_bytes(uint64_t n_refs, uint64_t bases) { return counter_bytes(n_refs) + (bases * 4u + 15u) / 16u * 16u; }

// where an anchor with entry e counts on a reference of len bases: false for an entry that names no base of it (a table that
// contradicts the lengths - the build makes none)
KBO_ST_FN bool hit_start(uint32_t e, uint32_t len, uint32_t &p)
{
    p = e & reflocate::kPosMask;
    return e != reflocate::kPosNone && p < len;
}

// D[j] from S[j] and S[j - k] (back: 0 for j < k)
KBO_ST_FN uint32_t depth_of(uint32_t s, uint32_t back) { return s - back; }

// a tile that begins at base t: bit i of `covered` for D[t + i] > 0, of `starts` for a covered base whose predecessor is not
KBO_ST_FN void tile_add(Tally &a, uint32_t t, uint64_t covered, uint64_t starts, uint32_t tile_max)
{
    if (!covered) return;
    a.covered += (uint32_t)__builtin_popcountll(covered);
    a.segments += (uint32_t)__builtin_popcountll(starts);
    if (a.first == kNone) a.first = t + (uint32_t)__builtin_ctzll(covered);
    a.last = t + 63u - (uint32_t)__builtin_clzll(covered);
    if (tile_max > a.max_depth) a.max_depth = tile_max;
}

KBO_ST_FN Cover no_entries(uint32_t ref_len) { return Cover{ref_len, 0u, 0u, kNone, kNone, 0u, 0u, kFlagNoEntries, 0ull, 0ull}; }
KBO_ST_FN Cover finish(uint32_t ref_len, const Tally &a, uint32_t n_runs, uint64_t n_anchors, uint64_t n_multi)
{
    return Cover{ref_len, a.covered, a.segments, a.first, a.last, a.max_depth, n_runs, (n_anchors >> 32) ? kFlagOverflow : 0u, n_anchors, n_multi};
}

// ---- the serial forms: what the kernels do, a tile after the other and a lane after the other

// count: the anchors of the run [start, end), start <= end, on a reference of len bases whose words begin at base
template <typename Words, typename EntryAt>
KBO_ST_FN void count_serial(Words &h, uint64_t base, uint32_t len, uint32_t start, uint32_t end, uint32_t k, EntryAt &&entry_at, uint64_t &n_anchors,
                            uint64_t &n_multi)
{
    if (end - start < k) return;
    const uint32_t starts = end - start - k + 1u;
    for (uint64_t done = 0; done < starts; done += reflocate::kWindow) {
        const uint32_t lanes = reflocate::group_lanes(starts - done);
        for (uint32_t j = 0; j < lanes; j++) {
            const uint32_t e = entry_at(start + (uint32_t)done + j);
            uint32_t p;
            if (!hit_start(e, len, p)) continue;
            h.add(base + p);
            n_anchors++;
            n_multi += (e & reflocate::kMulti) ? 1u : 0u;
        }
    }
}

// scan, in place
template <typename Words> KBO_ST_FN void scan_serial(Words &h, uint64_t base, uint32_t len)
{
    uint32_t carry = 0;
    for (uint32_t t = 0; t < len; t += kTile) {
        const uint32_t lanes = len - t < kTile ? len - t : kTile;
        uint32_t v[kTile];
        for (uint32_t j = 0; j < lanes; j++) v[j] = h.get(base + t + j);
        for (uint32_t d = 1; d < kTile; d <<= 1) // (the wave's steps: lane j takes lane j - d)
            for (uint32_t j = lanes; j-- > d;) v[j] += v[j - d];
        for (uint32_t j = 0; j < lanes; j++) h.set(base + t + j, v[j] + carry);
        carry += v[lanes - 1u];
    }
}

// reduce over the scanned words; depth: the profile's words of this reference from out_base on, or none
template <typename Words, typename DepthOut>
KBO_ST_FN Tally reduce_serial(const Words &s, uint64_t base, uint32_t len, uint32_t k, DepthOut *depth, uint64_t out_base)
{
    Tally a = no_tally();
    uint32_t prev = 0; // D of the base in front of the tile
    for (uint32_t t = 0; t < len; t += kTile) {
        const uint32_t lanes = len - t < kTile ? len - t : kTile;
        uint64_t covered = 0, starts = 0;
        uint32_t tile_max = 0;
        for (uint32_t i = 0; i < lanes; i++) {
            const uint32_t j = t + i, d = depth_of(s.get(base + j), j >= k ? s.get(base + j - k) : 0u);
            if (depth) depth->put(out_base + j, d);
            if (d) covered |= 1ull << i;
            if (d && !prev) starts |= 1ull << i;
            if (d > tile_max) tile_max = d;
            prev = d;
        }
        tile_add(a, t, covered, starts, tile_max);
    }
    return a;
}

} // namespace refcover
} // namespace kbo
