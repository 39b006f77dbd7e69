// refset_best.hpp — the best reference of one query sequence against a reference set, as a record that is its own reduction state
// (kbo_hip.h kbo_ref_best), for host and device alike: refset_best_kernels.hip merges the (reference, strand) pairs of
// a slab across a wave and into the call's table, refset.cpp merges the references of the single-index route into the downloaded
// table, tools/refset_best_check.cpp runs every small list of pairs through every cut and merge order on the CPU.
//
// A pair (reference, strand) of the sequence has a HIT when its extent's n_runs > 0 (the rule by which kbo_summary_refset keeps a
// record).  Pairs with a hit are ordered by
//   larger n_match first, then smaller ref, then '+' (1) before '-' (2)
// which is total: no two pairs share (ref, strand).  The record holds
//   ref, strand, the six extent words   of the FIRST pair in that order                     (none: ref = kNone, strand = 0, zeros)
//   n_hits                               the pairs with a hit
//   second_ref, second_match             ref and n_match of the first pair in that order among those of ANOTHER reference than `ref`
//                                        (none: kNone, 0)
// merge(a, b) of the records of two disjoint sets of pairs of one sequence is the record of their union: the first pair of the union
// is the better of the two firsts, and the first pair of another reference than the winner's is, within either set, that set's first
// pair when its reference differs from the winner's and that set's runner-up otherwise - so the runner-up of the union is the best
// of { a's first, b's first, a's runner-up, b's runner-up } whose reference differs from the winner's.  Only (n_match, ref) of a
// runner-up is kept and only that is compared: candidates that agree in both are the same answer.  Exact integer logic, commutative
// and associative, so the result does not depend on how the pairs are cut into slabs, lanes or waves.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define KBO_RB_FN __host__ __device__ __forceinline__
#else
#define KBO_RB_FN inline
#endif

namespace kbo {
namespace refbest {

constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr uint32_t kWords = 12; // == sizeof(kbo_ref_best) / 4

struct Best { // the words of kbo_ref_best, in its order
    uint32_t seq, ref, strand, n_match, n_mismatch, n_jump, n_runs, start, end, n_hits, second_ref, second_match;
};

// the record of no pair
KBO_RB_FN Best empty(uint32_t seq) { return Best{seq, kNone, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, kNone, 0u}; }

// the record of one pair; ext: the six words of its kbo_aln_extent { n_match, n_mismatch, n_jump, n_runs, start, end }
KBO_RB_FN Best from_pair(uint32_t seq, uint32_t ref, uint32_t strand, const uint32_t ext[6])
{
    if (ext[3] == 0u) return empty(seq);
    return Best{seq, ref, strand, ext[0], ext[1], ext[2], ext[3], ext[4], ext[5], 1u, kNone, 0u};
}

// (n_match, ref, strand) of a pair with a hit comes before that of another (ref == kNone: no pair, behind every pair)
KBO_RB_FN bool before(uint32_t match_a, uint32_t ref_a, uint32_t strand_a, uint32_t match_b, uint32_t ref_b, uint32_t strand_b)
{
    if (ref_a == kNone || ref_b == kNone) return ref_b == kNone && ref_a != kNone;
    if (match_a != match_b) return match_a > match_b;
    if (ref_a != ref_b) return ref_a < ref_b;
    return strand_a < strand_b;
}

KBO_RB_FN Best merge(const Best &a, const Best &b)
{
    const bool a_wins = !before(b.n_match, b.ref, b.strand, a.n_match, a.ref, a.strand);
    Best out = a_wins ? a : b;
    out.n_hits = a.n_hits + b.n_hits;
    const uint32_t cand_ref[4] = {a.ref, b.ref, a.second_ref, b.second_ref};
    const uint32_t cand_match[4] = {a.n_match, b.n_match, a.second_match, b.second_match};
    uint32_t ref = kNone, match = 0u;
    for (int i = 0; i < 4; i++)
        if (cand_ref[i] != out.ref && before(cand_match[i], cand_ref[i], 0u, match, ref, 0u)) {
            ref = cand_ref[i];
            match = cand_match[i];
        }
    out.second_ref = ref;
    out.second_match = match;
    return out;
}

} // namespace refbest
} // namespace kbo
