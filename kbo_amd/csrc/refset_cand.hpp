// refset_cand.hpp — the index arithmetic of a SCREENED reference-set slab, for host and device alike (kbo_refset_candidates_dev,
// kbo_*_refset_screened_dev): what the host's run_slabs / add_pair (refset_slab.hpp) do pair by pair on the host over the
// pairs whose bit is set, as steps that need only the bitmap, the batch's offsets and prefix sums.  refset_cand_kernels.hip runs them
// a lane per word, pair, reference, item slot and task slot; tools/refset_cand_check.cpp runs them on the CPU next to add_pair's loop.
//
//   bit    b = (r * n_seqs + s) * 2 + strand - 1 of the bitmap (kbo_refset_candidates): ascending bits are (ref, seq, strand) order
//   rank   of a set bit = set bits in front of it = prefix[word] + popcount(lower bits of the word): its place in the candidate list
//   list   the first max_pairs set bits, by rank; the pairs' lengths in that order, scanned: pre(n) = bases of the first n pairs
//   cut    n_walked = the largest n <= min(candidates, max_pairs) with pre(n) <= max_pair_bases: the ONE slab that is walked
//   pair   p < n_walked: first byte pre(p) (back to back, as add_pair), the threshold of its reference; behind: empty at walked_bases
//   item   i = ifirst(p) + c: chunk c of pair p; ifirst = exclusive scan of the pairs' chunk counts; the pair by bisection
//   task   the list is sorted by reference, so a reference's pairs [pb(r), pb(r + 1)) and items [ifirst(pb(r)), ifirst(pb(r + 1))) are
//          contiguous: ceil(items / 256) tasks each, their first by a scan; a task slot finds its reference by bisection
// The host knows the bounds without the bitmap: item_slots() and task_slots().  A task behind the real ones has items = 0.
#pragma once
#include "refset_plan.hpp"

#if defined(__HIPCC__) || defined(__HIP__)
#define KBO_RC_FN __host__ __device__ __forceinline__
#else
#define KBO_RC_FN inline
#endif

namespace kbo {
namespace refcand {

using refplan::Words4;
using refplan::kTaskItems;

constexpr uint32_t kMarkAll = 254;     // m of a packed reference whose m_r < kSeedMin: the screen never marks it, ALL its pairs are set
constexpr uint32_t kNoPair = 0xFFFFFFFFu; // a list slot behind the candidates
constexpr uint32_t kScan64Block = 1024;   // values per block of the 64-bit scan of the pairs' lengths

struct PairId {
    uint32_t ref, seq, strand; // strand: 1 '+', 2 '-'
};
KBO_RC_FN PairId pair_of_bit(uint32_t bit, uint32_t n_seqs)
{
    const uint32_t t = bit >> 1;
    return PairId{t / n_seqs, t % n_seqs, (bit & 1u) + 1u};
}
KBO_RC_FN uint64_t bit_of_pair(uint32_t ref, uint32_t seq, uint32_t strand, uint32_t n_seqs) { return ((uint64_t)ref * n_seqs + seq) * 2u + (strand - 1u); }

// the bits of word w that belong to a reference with mark_all(r) on the strands asked for, below n_bits (refset.cpp mark_unfilterable)
template <typename MarkAll> KBO_RC_FN uint32_t mark_mask(uint32_t w, uint64_t n_bits, uint32_t n_seqs, uint32_t strands, MarkAll mark_all)
{
    const uint64_t b0 = (uint64_t)w * 32u, per_ref = 2ull * n_seqs;
    const uint64_t end = b0 + 32u < n_bits ? b0 + 32u : n_bits;
    uint32_t out = 0;
    for (uint64_t b = b0; b < end;) {
        const uint64_t r = b / per_ref, ref_end = (r + 1u) * per_ref, e = ref_end < end ? ref_end : end;
        if (mark_all((uint32_t)r)) {
            const uint32_t lo = (uint32_t)(b - b0), n = (uint32_t)(e - b); // n in 1 .. 32
            out |= (n >= 32u ? 0xFFFFFFFFu : (1u << n) - 1u) << lo;
        }
        b = e;
    }
    return out & ((strands & 1u ? 0x55555555u : 0u) | (strands & 2u ? 0xAAAAAAAAu : 0u));
}

// the rank of bit `pos` of a word whose first bit has rank `prefix`
KBO_RC_FN uint32_t rank_of(uint32_t prefix, uint32_t word, uint32_t pos) { return prefix + (uint32_t)__builtin_popcount(word & ((1u << pos) - 1u)); }

// the pairs walked: the largest n <= listed with pre(n) <= max_bases; pre(n): bases of the first n listed pairs, pre(0) = 0, ascending
template <typename Pre> KBO_RC_FN uint32_t cut(uint32_t listed, uint64_t max_bases, Pre pre)
{
    uint32_t lo = 0, hi = listed;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo + 1u) / 2u;
        if (pre(mid) <= max_bases) lo = mid;
        else hi = mid - 1u;
    }
    return lo;
}

// the first of the n_walked pairs whose reference is >= r (n_walked: none); ref_of(p): the reference of pair p, ascending
template <typename RefOf> KBO_RC_FN uint32_t first_pair_of_ref(uint32_t n_walked, uint32_t r, RefOf ref_of)
{
    uint32_t lo = 0, hi = n_walked;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (ref_of(mid) >= r) hi = mid;
        else lo = mid + 1u;
    }
    return lo;
}

KBO_RC_FN uint32_t tasks_of(uint32_t items) { return (items + kTaskItems - 1u) / kTaskItems; }

// what the host knows of a slab of at most max_pairs pairs over at most max_bases bases: its item slots and its task slots
KBO_RC_FN uint64_t item_slots(uint64_t max_pairs, uint64_t max_bases, uint32_t chunk) { return max_bases / chunk + max_pairs; }
KBO_RC_FN uint64_t task_slots(uint64_t slots, uint64_t n_queryable, uint64_t max_pairs)
{
    return slots / kTaskItems + (n_queryable < max_pairs ? n_queryable : max_pairs) + 1u;
}

// chunk c of a pair of `len` bases whose sequence begins at q0 of the walk's query buffer (its strand's copy) and whose bytes begin
// at o0 of the slab: refplan::make_item's fields { first base minus the warm-up, first byte, (bases + warm-up) | warm-up << 16, 0 }
KBO_RC_FN Words4 make_item(uint32_t k, uint32_t chunk, uint64_t q0, uint64_t o0, uint32_t c, uint64_t len)
{
    const uint64_t c0 = (uint64_t)c * chunk, c1 = c0 + chunk < len ? c0 + chunk : len;
    const uint64_t warm = c0 < k - 1u ? c0 : k - 1u;
    return Words4{(uint32_t)(q0 + c0 - warm), (uint32_t)(o0 + c0), (uint32_t)(c1 - c0 + warm) | (uint32_t)warm << 16, 0u};
}
// task t of a reference whose `items` items begin at first_item: { reference, first item, items (<= 256), 0 }
KBO_RC_FN Words4 make_task(uint32_t ref, uint32_t first_item, uint32_t items, uint32_t t)
{
    const uint32_t at = t * kTaskItems, n = items > at ? (items - at < kTaskItems ? items - at : kTaskItems) : 0u;
    return Words4{ref, first_item + at, n, 0u};
}

} // namespace refcand
} // namespace kbo
