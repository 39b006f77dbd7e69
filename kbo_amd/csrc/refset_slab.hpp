// refset_slab.hpp — a slab of (reference, sequence, strand) pairs as the host plans it, pair by pair: the pairs, their chunks and
// the workgroups' tasks of the reference-set walk (kernels.hpp RefsetWalkArgs).  Plain host C++ without a HIP
// include: refset.cpp's host pipelines plan with it, and tools/refset_plan_check.cpp and tools/refset_cand_check.cpp hold the
// device planners' closed forms (refset_plan.hpp, refset_cand.hpp) against this very loop.
#pragma once
#include "refset_plan.hpp"

#include <algorithm>
#include <stdint.h>
#include <vector>

namespace kbo_host {

// the kinds of reference a range of references holds: which walk kernels run, and the LDS kernel's largest form
struct WalkKinds {
    bool has_lds = false, has_wide = false;
    uint32_t lds_units = 0;
};

struct SlabPlan {
    std::vector<uint32_t> ref, seq, strand, thr; // per pair; thr: its reference's threshold
    std::vector<uint64_t> off{0};                // per pair + 1: its first byte in the slab
    std::vector<uint32_t> items, tasks;          // four words a record (kernels.hpp RefsetWalkArgs)
    uint32_t longest = 0;
    WalkKinds kinds; // of the references the slab's tasks name
    void clear()
    {
        ref.clear(); seq.clear(); strand.clear(); thr.clear(); items.clear(); tasks.clear();
        off.assign(1, 0);
        longest = 0;
        kinds = WalkKinds{};
    }
    size_t pairs() const { return ref.size(); }
    uint64_t bytes() const { return off.back(); }
};

struct SlabBatch { // the batch as the planner sees it.  rev_base: where the '-' strand (2) begins in the walk's query buffer
    const uint64_t *offsets;
    uint32_t k, chunk;
    uint64_t rev_base;
};

// Sequence s of the batch on `strand` against reference r, behind the slab's pairs so far: an item per chunk with its warm-up of up to
// k - 1 bases, a new task per reference and per kTaskItems items.  (b by reference: as arguments held across the inserts, 3 % slower.)
inline void add_pair(SlabPlan &P, const SlabBatch &b, uint32_t r, uint32_t s, uint32_t strand, uint32_t threshold)
{
    const uint64_t len = b.offsets[s + 1] - b.offsets[s], q0 = (strand == 2u ? b.rev_base : 0) + b.offsets[s], o0 = P.bytes();
    bool fresh = P.tasks.empty() || P.tasks[P.tasks.size() - 4] != r;
    for (uint64_t c0 = 0; c0 < len; c0 += b.chunk) {
        const uint64_t c1 = std::min(len, c0 + b.chunk), warm = std::min<uint64_t>(c0, b.k - 1);
        if (fresh || P.tasks[P.tasks.size() - 2] == kbo::refplan::kTaskItems) {
            const uint32_t t[4] = {r, (uint32_t)(P.items.size() / 4), 0u, 0u};
            P.tasks.insert(P.tasks.end(), t, t + 4);
            fresh = false;
        }
        const uint32_t it[4] = {(uint32_t)(q0 + c0 - warm), (uint32_t)(o0 + c0), (uint32_t)(c1 - c0 + warm) | (uint32_t)warm << 16, 0u};
        P.items.insert(P.items.end(), it, it + 4);
        P.tasks[P.tasks.size() - 2]++;
    }
    P.ref.push_back(r);
    P.seq.push_back(s);
    P.strand.push_back(strand);
    P.thr.push_back(threshold);
    P.off.push_back(o0 + len);
    P.longest = std::max<uint32_t>(P.longest, (uint32_t)len);
}

} // namespace kbo_host
