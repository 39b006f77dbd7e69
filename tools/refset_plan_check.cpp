// refset_plan_check.cpp — the slab planner's arithmetic (kbo_amd/csrc/refset_plan.hpp) on the CPU, next to the loop it replaces:
// pairs, items and tasks of slabs of the device-resident reference-set calls, built the way refset_plan_kernels.hip builds them
// (a closed form per pair and per item slot, from the offsets alone) and compared with what the host's own planner (add_pair,
// refset_slab.hpp) appends pair by pair.  No GPU, no library: a stand-alone program, meant to run under sanitizers.
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -I kbo_amd/csrc tools/refset_plan_check.cpp -o refset_plan_check && ./refset_plan_check
#include "refset_plan.hpp"
#include "refset_slab.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace kbo::refplan;

namespace {

int g_bad = 0;
#define CHECK(cond, ...)                                                                                                                     \
    do {                                                                                                                                     \
        if (!(cond)) {                                                                                                                       \
            if (g_bad++ < 20) {                                                                                                              \
                std::fprintf(stderr, "%s:%d: %s: ", __FILE__, __LINE__, #cond);                                                             \
                std::fprintf(stderr, __VA_ARGS__);                                                                                           \
                std::fprintf(stderr, "\n");                                                                                                  \
            }                                                                                                                                \
        }                                                                                                                                    \
    } while (0)

// one slab of `refs` references whose set indexes are ref_ids, planned both ways
void check_slab(const std::vector<uint64_t> &offsets, uint32_t k, int strands, const std::vector<uint32_t> &ref_ids)
{
    const uint32_t n_seqs = (uint32_t)offsets.size() - 1, refs = (uint32_t)ref_ids.size();
    const Geometry g = geometry(n_seqs, offsets.back(), strands, k);
    kbo_host::SlabPlan H;
    for (uint32_t r : ref_ids)
        for (uint32_t s = 0; s < n_seqs; s++)
            for (uint32_t strand = 1; strand <= 2; strand++)
                if (strands & strand) kbo_host::add_pair(H, kbo_host::SlabBatch{offsets.data(), k, g.chunk, g.rev_base}, r, s, strand, 0u);

    // the device's inputs: chunks per sequence, scanned
    std::vector<uint32_t> first(n_seqs + 1, 0);
    for (uint32_t s = 0; s < n_seqs; s++) first[s + 1] = first[s] + chunks_of(offsets[s + 1] - offsets[s], g.chunk);
    const uint32_t real = g.n_strands * first[n_seqs];
    CHECK(real <= g.item_slots, "%u items, %u slots", real, g.item_slots);
    auto first_of = [&](uint32_t s) { return first[s]; };

    // rp_pairs_kernel
    const uint32_t n_pairs = refs * n_seqs * g.n_strands;
    CHECK(n_pairs == H.ref.size(), "%u pairs, the host has %zu", n_pairs, H.ref.size());
    for (uint32_t p = 0; p < n_pairs && p < H.ref.size(); p++) {
        const Pair pr = pair_of(g, p);
        const uint64_t b = offsets[pr.s], len = offsets[pr.s + 1] - b;
        CHECK(ref_ids[pr.j] == H.ref[p] && pr.s == H.seq[p] && strand_of(g, pr.x) == H.strand[p], "pair %u", p);
        CHECK(pair_offset(g, pr.j, pr.x, b, len) == H.off[p], "pair %u: first byte", p);
    }
    CHECK(slab_bytes(g, refs) == H.off.back(), "slab bytes");

    // rp_items_kernel: a lane per slot; the host's items follow each other without the unused slots
    std::vector<Words4> items((size_t)refs * g.item_slots, Words4{~0u, ~0u, ~0u, ~0u}), tasks((size_t)refs * g.tasks_per_ref, Words4{~0u, ~0u, ~0u, ~0u});
    for (uint64_t t = 0; t < (uint64_t)refs * g.item_slots; t++) {
        const uint32_t j = (uint32_t)(t / g.item_slots), i = (uint32_t)(t % g.item_slots);
        if (i % kTaskItems == 0) tasks.at((size_t)j * g.tasks_per_ref + i / kTaskItems) = make_task(g, ref_ids[j], j, i / kTaskItems, real);
        if (i >= real) continue;
        const ItemAt at = item_at(g, i, first_of);
        CHECK(at.s < n_seqs && at.x < g.n_strands && at.c < first[at.s + 1] - first[at.s], "slot %llu: (%u, %u, %u)", (unsigned long long)t, at.s, at.x, at.c);
        if (at.s >= n_seqs) continue;
        items[t] = make_item(g, j, at, offsets[at.s], offsets[at.s + 1] - offsets[at.s]);
    }
    CHECK((size_t)refs * real * 4 == H.items.size(), "%u items a reference, the host has %zu words", real, H.items.size());
    size_t h = 0;
    for (uint32_t j = 0; j < refs; j++)
        for (uint32_t i = 0; i < real && h + 4 <= H.items.size(); i++, h += 4) {
            const Words4 &w = items[(size_t)j * g.item_slots + i];
            CHECK(w.x == H.items[h] && w.y == H.items[h + 1] && w.z == H.items[h + 2] && w.w == H.items[h + 3], "reference %u item %u", j, i);
        }
    // the tasks with items are the host's, in its order, over the same items; the others are empty and name a reference of the slab
    size_t ht = 0;
    for (uint32_t j = 0; j < refs; j++)
        for (uint32_t t = 0; t < g.tasks_per_ref; t++) {
            const Words4 &w = tasks[(size_t)j * g.tasks_per_ref + t];
            CHECK(w.x == ref_ids[j] && w.z <= kTaskItems && w.w == 0u, "reference %u task %u", j, t);
            CHECK((uint64_t)w.y + w.z <= (uint64_t)(j + 1) * g.item_slots && w.y >= j * g.item_slots, "reference %u task %u: its items", j, t);
            if (!w.z) continue;
            CHECK(ht + 4 <= H.tasks.size(), "more tasks than the host has");
            if (ht + 4 > H.tasks.size()) continue;
            // (the host's items are dense: item y of the host is slot y - j * real + j * item_slots here)
            CHECK(w.x == H.tasks[ht] && w.y - j * g.item_slots + j * real == H.tasks[ht + 1] && w.z == H.tasks[ht + 2], "reference %u task %u against the host's", j, t);
            ht += 4;
        }
    CHECK(ht == H.tasks.size(), "%zu task words matched, the host has %zu", ht, H.tasks.size());

    // record_owner over a prefix with pairs that own nothing
    std::vector<uint32_t> rf(n_pairs + 1, 0);
    for (uint32_t p = 0; p < n_pairs; p++) rf[p + 1] = rf[p] + (p % 7 == 3 ? 3 : p % 5 == 0 ? 1 : 0);
    for (uint32_t p = 0; p < n_pairs; p++)
        for (uint32_t x = rf[p]; x < rf[p + 1]; x++) CHECK(record_owner(n_pairs, x, [&](uint32_t q) { return rf[q]; }) == p, "record %u", x);
}

} // namespace

int main()
{
    // one contig of 70 000 bases (more than 256 chunks a reference at k = 31), odd lengths, 0 .. 3 bases in the middle, 300 contigs of 5
    std::vector<uint64_t> lens = {70000, 40, 257, 0, 1, 2, 3, 511};
    for (int i = 0; i < 300; i++) lens.push_back(5);
    std::vector<uint64_t> offsets(1, 0);
    for (uint64_t n : lens) offsets.push_back(offsets.back() + n);
    int slabs = 0;
    for (uint32_t k : {31u, 96u, 3u, 255u})
        for (int strands = 1; strands <= 3; strands++) {
            for (uint32_t r = 0; r < 4; r++, slabs++) check_slab(offsets, k, strands, {r * 3 + 1}); // one reference a slab, as the issue's comparison
            check_slab(offsets, k, strands, {1, 2, 5});
            check_slab(offsets, k, strands, {0, 7, 8, 9, 11});
            slabs += 2;
        }
    // batches without a base, of one base, of exact multiples of the chunk
    for (const std::vector<uint64_t> &o : {std::vector<uint64_t>{0, 0}, std::vector<uint64_t>{0, 0, 1, 1}, std::vector<uint64_t>{0, 256, 512, 1536},
                                           std::vector<uint64_t>{0, 255, 512, 769, 769}})
        for (int strands = 1; strands <= 3; strands++, slabs++) check_slab(o, 31, strands, {4, 6});
    if (g_bad) {
        std::fprintf(stderr, "%d checks failed\n", g_bad);
        return 1;
    }
    std::printf("refset_plan_check: %d slabs agree with the host's plan\n", slabs);
    return 0;
}
