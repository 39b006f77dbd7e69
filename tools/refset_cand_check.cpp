// refset_cand_check.cpp — the screened slab planner's arithmetic (kbo_amd/csrc/refset_cand.hpp) on the CPU, next to the loops it
// replaces: the candidate list, the cut by the caps, pairs, items and tasks of the ONE slab of the screened device-resident
// reference-set calls, built the way refset_cand_kernels.hip builds them (a step per bitmap word, pair slot, reference, item slot and
// task slot, from the bitmap, the offsets and prefix sums) and compared with brute force and with what the host's own planner (add_pair,
// refset_slab.hpp, in refset.cpp's run_slabs order) appends pair by pair over the pairs whose bit is set.  Every array is read through at(): an index
// outside it ends the program.  No GPU, no library: a stand-alone program, meant to run under sanitizers.
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -I kbo_amd/csrc tools/refset_cand_check.cpp -o refset_cand_check && ./refset_cand_check
#include "refset_cand.hpp"
#include "refset_slab.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace kbo::refcand;
using kbo::refplan::chunk_of;
using kbo::refplan::chunks_of;
using kbo::refplan::record_owner;

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

uint64_t g_rng = 0x9E3779B97F4A7C15ull;
uint32_t rnd()
{
    g_rng ^= g_rng << 13;
    g_rng ^= g_rng >> 7;
    g_rng ^= g_rng << 17;
    return (uint32_t)(g_rng >> 32);
}

// one call: `screened` is the kernel's bitmap (per mille of the pairs set), mark_all the references that cannot be screened
void check_call(const std::vector<uint64_t> &offsets, uint32_t n_refs, uint32_t k, int strands, uint32_t per_mille, const std::vector<uint8_t> &mark_all,
                uint32_t max_pairs, uint64_t max_bases)
{
    const uint32_t n_seqs = (uint32_t)offsets.size() - 1, chunk = chunk_of(k);
    const uint64_t n_bits = (uint64_t)n_refs * n_seqs * 2u, total = offsets.back(), rev_off = strands == 3 ? (total + 15) / 16 * 16 : 0;
    const uint32_t words = (uint32_t)((n_bits + 31) / 32);
    auto len_of = [&](uint32_t s) { return offsets.at(s + 1) - offsets.at(s); };

    // the screen kernel's bits: only pairs of the strands asked for, of references it can screen
    std::vector<uint32_t> bits(words, 0u), brute(words, 0u);
    for (uint64_t b = 0; b < n_bits; b++) {
        const PairId id = pair_of_bit((uint32_t)b, n_seqs);
        CHECK(bit_of_pair(id.ref, id.seq, id.strand, n_seqs) == b && id.ref < n_refs && id.seq < n_seqs, "bit %llu", (unsigned long long)b);
        if ((strands & id.strand) && !mark_all.at(id.ref) && rnd() % 1000u < per_mille) bits.at(b >> 5) |= 1u << (b & 31u);
    }
    // rc_count_kernel against refset.cpp mark_unfilterable
    brute = bits;
    for (uint32_t r = 0; r < n_refs; r++)
        if (mark_all.at(r))
            for (uint32_t s = 0; s < n_seqs; s++)
                for (uint32_t strand = 1; strand <= 2; strand++)
                    if (strands & strand) {
                        const uint64_t b = bit_of_pair(r, s, strand, n_seqs);
                        brute.at(b >> 5) |= 1u << (b & 31u);
                    }
    std::vector<uint32_t> prefix(words + 1, 0u);
    uint64_t cand_bases = 0;
    for (uint32_t w = 0; w < words; w++) {
        bits.at(w) |= mark_mask(w, n_bits, n_seqs, (uint32_t)strands, [&](uint32_t r) { return mark_all.at(r) != 0; });
        CHECK(bits.at(w) == brute.at(w), "word %u: %08x, by brute force %08x", w, bits.at(w), brute.at(w));
        prefix.at(w + 1) = prefix.at(w) + (uint32_t)__builtin_popcount(bits.at(w));
    }
    const uint32_t cand = prefix.at(words);

    // the host's order of the candidates (run_slabs: reference, sequence, strand) is the ascending bits; rank by brute force
    std::vector<uint32_t> order;
    for (uint32_t r = 0; r < n_refs; r++)
        for (uint32_t s = 0; s < n_seqs; s++)
            for (uint32_t strand = 1; strand <= 2; strand++) {
                const uint64_t b = bit_of_pair(r, s, strand, n_seqs);
                if (!(bits.at(b >> 5) >> (b & 31u) & 1u)) continue;
                CHECK(rank_of(prefix.at(b >> 5), bits.at(b >> 5), (uint32_t)(b & 31u)) == order.size(), "rank of bit %llu", (unsigned long long)b);
                order.push_back((uint32_t)b);
                cand_bases += len_of(s);
            }
    CHECK(order.size() == cand, "%zu candidates, the prefix says %u", order.size(), cand);

    // rc_list_kernel: a step per word, then the slots behind the candidates; the lengths' scan
    std::vector<uint32_t> list(max_pairs, 0xDEADBEEFu);
    std::vector<uint64_t> pre(max_pairs + 1, ~0ull);
    for (uint32_t w = 0; w < words; w++) {
        uint32_t v = bits.at(w), rank = prefix.at(w);
        for (; v && rank < max_pairs; rank++) {
            const uint32_t bit = w * 32u + (uint32_t)__builtin_ctz(v);
            v &= v - 1u;
            list.at(rank) = bit;
            pre.at(rank) = len_of((bit >> 1) % n_seqs);
        }
    }
    for (uint32_t i = std::min(cand, max_pairs); i <= max_pairs; i++) {
        pre.at(i) = 0;
        if (i < max_pairs) list.at(i) = kNoPair;
    }
    for (uint32_t i = 0; i < max_pairs; i++) CHECK(list.at(i) == (i < cand ? order.at(i) : kNoPair), "list slot %u", i);
    uint64_t run = 0;
    for (uint32_t i = 0; i <= max_pairs; i++) { // exclusive, in place
        const uint64_t v = pre.at(i);
        pre.at(i) = run;
        run += v;
    }

    // rc_cut_kernel against the loop
    const uint32_t listed = std::min(cand, max_pairs);
    const uint32_t walked = cut(listed, max_bases, [&](uint32_t n) { return pre.at(n); });
    uint32_t bw = 0;
    uint64_t bb = 0;
    while (bw < cand && bw < max_pairs && bb + len_of((order.at(bw) >> 1) % n_seqs) <= max_bases) bb += len_of((order.at(bw++) >> 1) % n_seqs);
    CHECK(walked == bw && pre.at(walked) == bb, "cut: %u pairs / %llu bases, by the loop %u / %llu", walked, (unsigned long long)pre.at(walked), bw,
          (unsigned long long)bb);
    const uint64_t walked_bases = pre.at(walked);
    CHECK(walked_bases <= max_bases && walked <= max_pairs && cand_bases >= walked_bases, "the caps");

    // the host's plan over the walked pairs
    kbo_host::SlabPlan H;
    for (uint32_t p = 0; p < walked; p++) {
        const PairId id = pair_of_bit(order.at(p), n_seqs);
        kbo_host::add_pair(H, kbo_host::SlabBatch{offsets.data(), k, chunk, rev_off}, id.ref, id.seq, id.strand, 0u);
    }

    // rc_pairs_kernel
    std::vector<uint64_t> poff(max_pairs + 1);
    std::vector<uint32_t> ifirst(max_pairs + 2, 0u);
    for (uint32_t p = 0; p <= max_pairs; p++) {
        uint32_t nch = 0;
        if (p < walked) {
            const PairId id = pair_of_bit(list.at(p), n_seqs);
            poff.at(p) = pre.at(p);
            nch = chunks_of(len_of(id.seq), chunk);
            CHECK(id.ref == H.ref.at(p) && id.seq == H.seq.at(p) && id.strand == H.strand.at(p) && poff.at(p) == H.off.at(p), "pair %u", p);
        } else poff.at(p) = walked_bases;
        ifirst.at(p + 1) = ifirst.at(p) + nch;
    }
    CHECK(poff.at(walked) == H.off.back(), "slab bytes");
    for (uint32_t p = 0; p < max_pairs; p++) CHECK(poff.at(p) <= poff.at(p + 1) && poff.at(p + 1) <= walked_bases, "pair %u: offsets ascend", p);
    const uint32_t real = ifirst.at(max_pairs);
    const uint64_t islots = item_slots(max_pairs, max_bases, chunk);
    CHECK(real <= islots && (size_t)real * 4 == H.items.size(), "%u items, %llu slots, the host has %zu words", real, (unsigned long long)islots, H.items.size());

    // rc_refs_kernel
    uint32_t n_q = 0;
    std::vector<uint32_t> seen(n_refs, 0u);
    for (uint32_t p = 0; p < walked; p++) seen.at(pair_of_bit(list.at(p), n_seqs).ref) = 1;
    for (uint32_t r = 0; r < n_refs; r++) n_q += seen.at(r);
    std::vector<uint32_t> rfirst(n_refs + 1), tfirst(n_refs + 2, 0u);
    auto ref_of = [&](uint32_t p) { return pair_of_bit(list.at(p), n_seqs).ref; };
    for (uint32_t r = 0; r <= n_refs; r++) {
        const uint32_t pb = first_pair_of_ref(walked, r, ref_of);
        uint32_t brute_pb = 0;
        while (brute_pb < walked && ref_of(brute_pb) < r) brute_pb++;
        CHECK(pb == brute_pb, "reference %u: first pair %u, by the loop %u", r, pb, brute_pb);
        rfirst.at(r) = ifirst.at(pb);
        tfirst.at(r + 1) = tfirst.at(r) + (r < n_refs ? tasks_of(ifirst.at(first_pair_of_ref(walked, r + 1, ref_of)) - ifirst.at(pb)) : 0u);
    }
    const uint32_t real_tasks = tfirst.at(n_refs);
    const uint64_t tslots = task_slots(islots, n_q, max_pairs); // (the references the call can query are at least those it walks)
    CHECK(real_tasks < tslots && (size_t)real_tasks * 4 == H.tasks.size(), "%u tasks, %llu slots, the host has %zu words", real_tasks,
          (unsigned long long)tslots, H.tasks.size());

    // rc_items_kernel: a step per item slot, then per task slot
    for (uint64_t g = 0; g < islots; g++) {
        const uint32_t i = (uint32_t)g;
        if (i >= ifirst.at(walked)) continue;
        const uint32_t p = record_owner(walked, i, [&](uint32_t q) { return ifirst.at(q); });
        CHECK(p < walked && ifirst.at(p) <= i && i < ifirst.at(p + 1), "item %u: pair %u", i, p);
        const PairId id = pair_of_bit(list.at(p), n_seqs);
        const uint64_t b = offsets.at(id.seq);
        const kbo::refplan::Words4 w = make_item(k, chunk, (id.strand == 2u ? rev_off : 0u) + b, poff.at(p), i - ifirst.at(p), len_of(id.seq));
        const size_t h = (size_t)i * 4;
        CHECK(w.x == H.items.at(h) && w.y == H.items.at(h + 1) && w.z == H.items.at(h + 2) && w.w == H.items.at(h + 3), "item %u", i);
    }
    for (uint64_t g = 0; g < tslots; g++) {
        const uint32_t t = (uint32_t)g;
        if (t >= real_tasks) continue; // (an empty task: { a reference that can be queried, 0, 0, 0 })
        const uint32_t r = record_owner(n_refs, t, [&](uint32_t q) { return tfirst.at(q); });
        CHECK(r < n_refs && tfirst.at(r) <= t && t < tfirst.at(r + 1), "task %u: reference %u", t, r);
        const kbo::refplan::Words4 w = make_task(r, rfirst.at(r), rfirst.at(r + 1) - rfirst.at(r), t - tfirst.at(r));
        const size_t h = (size_t)t * 4;
        CHECK(w.x == H.tasks.at(h) && w.y == H.tasks.at(h + 1) && w.z == H.tasks.at(h + 2) && w.w == 0u && w.z >= 1u && w.z <= kTaskItems, "task %u", t);
    }
}

} // namespace

int main()
{
    // one contig of 70 000 bases (more than 256 chunks a pair at k = 31), odd lengths, 0 .. 3 bases in the middle, 300 contigs of 5
    std::vector<uint64_t> lens = {70000, 40, 257, 0, 1, 2, 3, 511};
    for (int i = 0; i < 300; i++) lens.push_back(5);
    std::vector<uint64_t> offsets(1, 0);
    for (uint64_t n : lens) offsets.push_back(offsets.back() + n);
    const uint32_t n_refs = 11;
    std::vector<uint8_t> none(n_refs, 0), some(n_refs, 0);
    some[0] = some[4] = some[10] = 1;
    int calls = 0;
    for (uint32_t k : {31u, 96u, 3u, 255u})
        for (int strands = 1; strands <= 3; strands++)
            for (uint32_t per_mille : {0u, 7u, 300u, 1000u})
                for (const std::vector<uint8_t> &mark : {none, some}) {
                    const uint32_t all = n_refs * (uint32_t)lens.size() * 2u;
                    // ample caps, a cap on the pairs, on the bases, below the first pair, on both
                    check_call(offsets, n_refs, k, strands, per_mille, mark, all, 1ull << 31);
                    check_call(offsets, n_refs, k, strands, per_mille, mark, 37, 1ull << 31);
                    check_call(offsets, n_refs, k, strands, per_mille, mark, all, 71000);
                    check_call(offsets, n_refs, k, strands, per_mille, mark, all, 4);
                    check_call(offsets, n_refs, k, strands, per_mille, mark, 1, 0);
                    check_call(offsets, n_refs, k, strands, per_mille, mark, 700, 150000);
                    calls += 6;
                }
    // one sequence (a word spans sixteen references), batches without a base, exact multiples of the chunk
    for (const std::vector<uint64_t> &o : {std::vector<uint64_t>{0, 100}, std::vector<uint64_t>{0, 0}, std::vector<uint64_t>{0, 0, 1, 1},
                                           std::vector<uint64_t>{0, 256, 512, 1536}, std::vector<uint64_t>{0, 255, 512, 769, 769}})
        for (int strands = 1; strands <= 3; strands++)
            for (uint32_t per_mille : {200u, 1000u}) {
                std::vector<uint8_t> mark(37, 0);
                mark[1] = mark[2] = mark[17] = mark[36] = 1;
                check_call(o, 37, 31, strands, per_mille, mark, 1000, 1ull << 20);
                check_call(o, 37, 31, strands, per_mille, mark, 5, 600);
                calls += 2;
            }
    if (g_bad) {
        std::fprintf(stderr, "%d checks failed\n", g_bad);
        return 1;
    }
    std::printf("refset_cand_check: %d calls agree with the host's plan and with brute force\n", calls);
    return 0;
}
