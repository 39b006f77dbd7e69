// refset_plan.hpp — the index arithmetic of a reference-set slab, for host and device alike (kbo_find_refset_dev /
// kbo_summary_refset_dev): what refset_slab.hpp's add_pair does pair by pair on the host, as closed forms
// that need only the batch's offsets.  refset_plan_kernels.hip runs them a lane per pair and per item; tools/refset_plan_check.cpp
// runs them on the CPU next to add_pair's loop.
//
// A slab is `refs` consecutive queryable references against the WHOLE batch on the strands asked for:
//   pair   p = (j * n_seqs + s) * n_strands + x      j: reference of the slab, s: sequence, x: strand index ('+' first)
//   byte   first byte of pair p in the slab = j * n_strands * total + n_strands * off[s] + x * len_s   (back to back, no padding)
//   item   i of reference j = n_strands * first[s] + x * nch[s] + c       c: chunk of the sequence; first = exclusive scan of nch
//   task   t of reference j = items [256 t, 256 t + 256) of it, of which the real ones count
// Every reference owns item_slots = n_strands * (total / chunk + n_seqs) item slots - a bound of n_strands * first[n_seqs] the host
// knows without the lengths - and ceil(item_slots / 256) tasks; a task behind the real items has items = 0.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define KBO_RP_FN __host__ __device__ __forceinline__
#else
#define KBO_RP_FN inline
#endif

namespace kbo {
namespace refplan {

constexpr uint32_t kChunkMin = 256;  // == kRefsetChunk
constexpr uint32_t kTaskItems = 256; // == kRefsetThreads

struct Geometry {
    uint32_t n_seqs, n_strands, strands; // strands: KBO_STRAND_FWD, KBO_STRAND_REV or both (then n_strands = 2)
    uint32_t k, chunk;
    uint32_t item_slots, tasks_per_ref;
    uint64_t total;    // bases of the batch
    uint64_t rev_base; // where the '-' strand begins in the walk's query buffer (0 when it is the only one there)
};

KBO_RP_FN uint32_t chunk_of(uint32_t k) { return 4u * k > kChunkMin ? 4u * k : kChunkMin; }
KBO_RP_FN uint32_t chunks_of(uint64_t len, uint32_t chunk) { return (uint32_t)((len + chunk - 1u) / chunk); }
KBO_RP_FN uint64_t chunks_bound(uint64_t total, uint64_t n_seqs, uint32_t chunk) { return total / chunk + n_seqs; }

KBO_RP_FN Geometry geometry(uint64_t n_seqs, uint64_t total, int strands, uint32_t k)
{
    Geometry g;
    g.n_seqs = (uint32_t)n_seqs;
    g.n_strands = strands == 3 ? 2u : 1u;
    g.strands = (uint32_t)strands;
    g.k = k;
    g.chunk = chunk_of(k);
    g.item_slots = (uint32_t)(g.n_strands * chunks_bound(total, n_seqs, g.chunk));
    g.tasks_per_ref = (g.item_slots + kTaskItems - 1u) / kTaskItems;
    g.total = total;
    g.rev_base = strands == 3 ? (total + 15u) / 16u * 16u : 0u;
    return g;
}

KBO_RP_FN uint32_t strand_of(const Geometry &g, uint32_t x) { return g.strands == 3u ? x + 1u : g.strands; }

struct Pair {
    uint32_t j, s, x;
};
KBO_RP_FN Pair pair_of(const Geometry &g, uint32_t p)
{
    const uint32_t per_ref = g.n_seqs * g.n_strands, rem = p % per_ref;
    return Pair{p / per_ref, rem / g.n_strands, rem % g.n_strands};
}
KBO_RP_FN uint64_t pair_offset(const Geometry &g, uint32_t j, uint32_t x, uint64_t off_s, uint64_t len_s)
{
    return (uint64_t)j * g.n_strands * g.total + g.n_strands * off_s + x * len_s;
}
KBO_RP_FN uint64_t slab_bytes(const Geometry &g, uint32_t refs) { return (uint64_t)refs * g.n_strands * g.total; }

// item i of a reference: its sequence, strand index and chunk.  first(s): the exclusive scan of the chunk counts, s = 0 .. n_seqs;
// i < n_strands * first(n_seqs)
struct ItemAt {
    uint32_t s, x, c;
};
template <typename First> KBO_RP_FN ItemAt item_at(const Geometry &g, uint32_t i, First first)
{
    const uint32_t t = i / g.n_strands;
    uint32_t lo = 0, hi = g.n_seqs; // the largest s with first(s) <= t: sequences without a chunk own no item
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (first(mid) <= t) lo = mid;
        else hi = mid;
    }
    const uint32_t f = first(lo), n = first(lo + 1u) - f, rem = i - g.n_strands * f;
    return ItemAt{lo, rem / n, rem % n};
}

struct Words4 {
    uint32_t x, y, z, w;
};
// { first base in q minus the warm-up, first byte in ms, (bases + warm-up) | warm-up << 16, 0 } (kernels.hpp RefsetWalkArgs)
KBO_RP_FN Words4 make_item(const Geometry &g, uint32_t j, const ItemAt &a, uint64_t off_s, uint64_t len_s)
{
    const uint64_t c0 = (uint64_t)a.c * g.chunk, c1 = c0 + g.chunk < len_s ? c0 + g.chunk : len_s;
    const uint64_t warm = c0 < g.k - 1u ? c0 : g.k - 1u;
    const uint64_t q0 = (strand_of(g, a.x) == 2u ? g.rev_base : 0u) + off_s, o0 = pair_offset(g, j, a.x, off_s, len_s);
    return Words4{(uint32_t)(q0 + c0 - warm), (uint32_t)(o0 + c0), (uint32_t)(c1 - c0 + warm) | (uint32_t)warm << 16, 0u};
}
// { reference, first item, items, 0 }: task t of the slab's reference j, which has `real` items in all
KBO_RP_FN Words4 make_task(const Geometry &g, uint32_t ref, uint32_t j, uint32_t t, uint32_t real)
{
    const uint32_t at = t * kTaskItems, n = real > at ? (real - at < kTaskItems ? real - at : kTaskItems) : 0u;
    return Words4{ref, j * g.item_slots + at, n, 0u};
}

// the pair that owns record x of a slab: the largest p < n_pairs with first[p] <= x (first: a plain prefix of n_pairs + 1 counts,
// x < first[n_pairs]; pairs without a record own none)
template <typename First> KBO_RP_FN uint32_t record_owner(uint32_t n_pairs, uint32_t x, First first)
{
    uint32_t lo = 0, hi = n_pairs;
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (first(mid) <= x) lo = mid;
        else hi = mid;
    }
    return lo;
}

} // namespace refplan
} // namespace kbo
