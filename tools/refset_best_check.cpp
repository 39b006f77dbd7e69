// refset_best_check.cpp — the record of kbo_best_refset and its merge (kbo_amd/csrc/refset_best.hpp) on the CPU, by brute force: every
// list of (reference, strand) pairs over 3 references x 2 strands whose pairs are { no hit, a hit with n_match 0, 1, 2 } (4^6 lists;
// the 3^6 without the hit of no match among them), every contiguous cut of the list into 1 to 3 slabs (empty ones included), in
// the slabs' order and reversed, each slab and the table folded left to right and as a balanced tree - against the record made by
// SORTING the pairs by the stated order (larger n_match, smaller ref, '+' first).  All twelve words are compared: a pair's other
// extent words are its own, so a winner's extent cannot come from another pair.  No GPU, no library: a stand-alone program, meant to
// run under sanitizers.
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -I kbo_amd/csrc tools/refset_best_check.cpp -o refset_best_check
//   ./refset_best_check        prints the cases checked; exit status 1 at the first difference
#include "refset_best.hpp"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

namespace {

using namespace kbo::refbest;

constexpr uint32_t kSeq = 7;
constexpr uint32_t kRefIds[3] = {2, 5, 9}; // (ascending, as a slab has them, and not their positions)
constexpr int kPairs = 6;

struct PairIn {
    uint32_t ref, strand, ext[6];
};

// state 0: no hit; 1 .. 3: a hit with n_match = state - 1
PairIn make_pair(int at, int state)
{
    PairIn p;
    p.ref = kRefIds[at / 2];
    p.strand = 1u + (uint32_t)(at % 2);
    const uint32_t u = (uint32_t)at;
    const uint32_t hit[6] = {(uint32_t)state - 1u, 10u + u, 20u + u, 1u + u, 30u + u, 40u + u};
    const uint32_t miss[6] = {0u, 0u, 0u, 0u, 0u, 0u};
    std::memcpy(p.ext, state ? hit : miss, sizeof p.ext);
    return p;
}

Best by_sorting(const std::vector<PairIn> &pairs)
{
    std::vector<PairIn> hits;
    for (const PairIn &p : pairs)
        if (p.ext[3] > 0) hits.push_back(p);
    std::sort(hits.begin(), hits.end(), [](const PairIn &a, const PairIn &b) {
        if (a.ext[0] != b.ext[0]) return a.ext[0] > b.ext[0];
        if (a.ref != b.ref) return a.ref < b.ref;
        return a.strand < b.strand;
    });
    Best out{kSeq, kNone, 0, 0, 0, 0, 0, 0, 0, (uint32_t)hits.size(), kNone, 0};
    if (hits.empty()) return out;
    const PairIn &w = hits[0];
    out.ref = w.ref;
    out.strand = w.strand;
    out.n_match = w.ext[0]; out.n_mismatch = w.ext[1]; out.n_jump = w.ext[2]; out.n_runs = w.ext[3]; out.start = w.ext[4]; out.end = w.ext[5];
    for (const PairIn &p : hits)
        if (p.ref != w.ref) {
            out.second_ref = p.ref;
            out.second_match = p.ext[0];
            break;
        }
    return out;
}

Best fold_left(const std::vector<Best> &v)
{
    Best acc = empty(kSeq);
    for (const Best &b : v) acc = merge(acc, b);
    return acc;
}

Best fold_tree(const std::vector<Best> &v, size_t lo, size_t hi)
{
    if (lo == hi) return empty(kSeq);
    if (hi - lo == 1) return v[lo];
    const size_t mid = lo + (hi - lo) / 2;
    return merge(fold_tree(v, lo, mid), fold_tree(v, mid, hi));
}

bool same(const Best &a, const Best &b) { return std::memcmp(&a, &b, sizeof(Best)) == 0; }

void show(const char *what, const Best &b)
{
    std::printf("  %s: seq %u ref %u strand %u ext %u %u %u %u %u %u hits %u second %u %u\n", what, b.seq, b.ref, b.strand, b.n_match, b.n_mismatch,
                b.n_jump, b.n_runs, b.start, b.end, b.n_hits, b.second_ref, b.second_match);
}

} // namespace

int main()
{
    static_assert(sizeof(Best) == 4 * kWords, "twelve words, no padding");
    unsigned long long lists = 0, cases = 0;
    int total = 1;
    for (int i = 0; i < kPairs; i++) total *= 4;
    for (int code = 0; code < total; code++) {
        std::vector<PairIn> pairs;
        for (int at = 0, c = code; at < kPairs; at++, c /= 4) pairs.push_back(make_pair(at, c % 4));
        const Best want = by_sorting(pairs);
        std::vector<Best> recs;
        for (const PairIn &p : pairs) recs.push_back(from_pair(kSeq, p.ref, p.strand, p.ext));
        lists++;
        for (int i = 0; i <= kPairs; i++)
            for (int j = i; j <= kPairs; j++) { // slabs [0, i), [i, j), [j, 6): one slab when two are empty, two when one is
                const int cut[4] = {0, i, j, kPairs};
                for (int tree_in = 0; tree_in < 2; tree_in++)
                    for (int tree_out = 0; tree_out < 2; tree_out++)
                        for (int reversed = 0; reversed < 2; reversed++) {
                            std::vector<Best> slabs;
                            for (int s = 0; s < 3; s++) {
                                const std::vector<Best> part(recs.begin() + cut[s], recs.begin() + cut[s + 1]);
                                slabs.push_back(tree_in ? fold_tree(part, 0, part.size()) : fold_left(part));
                            }
                            if (reversed) std::reverse(slabs.begin(), slabs.end());
                            const Best got = tree_out ? fold_tree(slabs, 0, slabs.size()) : fold_left(slabs);
                            cases++;
                            if (!same(got, want)) {
                                std::printf("list %d cut %d %d tree %d %d reversed %d differs\n", code, i, j, tree_in, tree_out, reversed);
                                show("merged", got);
                                show("sorted", want);
                                return 1;
                            }
                        }
            }
    }
    // the sentinels, spelled out
    const Best none = empty(kSeq);
    if (none.ref != kNone || none.second_ref != kNone || none.strand || none.n_hits || none.n_match || none.second_match || none.seq != kSeq) return 1;
    std::printf("%llu lists, %llu cases agree\n", lists, cases);
    return 0;
}
