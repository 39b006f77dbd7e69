// refset_screen_check.cpp — the seed screen of a reference set (kbo_amd/csrc/refset_screen.hpp) on the CPU, against brute force: the
// seed of every position made right to left (step_left) against the bases read off the sequence, and the bucket scan over a table of
// related references - mutated copies of one ancestor, so that shared prefixes of every length between kSeedMin and kSeedMax occur,
// with a stretch shorter than kSeedMax, an N and a lower-case base among them - against sets of m-mers, for every m of
// kSeedMin .. kSeedMax: a (reference, query) pair is marked at m exactly when some m consecutive bases of the query are m consecutive
// bases of a stretch of the reference.  The table is read through an accessor that checks every index.  No GPU, no library: a
// stand-alone program, meant to run under sanitizers.
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -I kbo_amd/csrc tools/refset_screen_check.cpp -o refset_screen_check
//   ./refset_screen_check        prints the cases checked; exit status 1 at the first difference
#include "refset_screen.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <string>
#include <utility>
#include <vector>

namespace {

using namespace kbo::refscreen;

uint64_t g_rng = 0x9E3779B97F4A7C15ull;
uint32_t draw(uint32_t n)
{
    g_rng ^= g_rng << 13;
    g_rng ^= g_rng >> 7;
    g_rng ^= g_rng << 17;
    return (uint32_t)((g_rng >> 33) % n);
}

[[noreturn]] void fail(const char *what, size_t a, size_t b)
{
    std::printf("FAIL %s (%zu, %zu)\n", what, a, b);
    std::exit(1);
}

struct Table {
    std::vector<uint32_t> bucket_, ref_;
    std::vector<uint64_t> key_;
    uint32_t bucket(uint32_t b) const
    {
        if (b >= bucket_.size()) fail("bucket index", b, bucket_.size());
        return bucket_[b];
    }
    uint64_t key(uint32_t x) const
    {
        if (x >= key_.size()) fail("key index", x, key_.size());
        return key_[x];
    }
    uint32_t ref(uint32_t x) const
    {
        if (x >= ref_.size()) fail("ref index", x, ref_.size());
        return ref_[x];
    }
};

bool is_base(char c) { return c == 'A' || c == 'C' || c == 'G' || c == 'T'; }

// the maximal runs of bases of a sequence
std::vector<std::string> stretches(const std::string &s)
{
    std::vector<std::string> out;
    for (size_t i = 0; i < s.size();) {
        if (!is_base(s[i])) {
            i++;
            continue;
        }
        size_t j = i;
        while (j < s.size() && is_base(s[j])) j++;
        out.push_back(s.substr(i, j - i));
        i = j;
    }
    return out;
}

// the seed at position i by definition: the next up to kSeedMax bytes while they are bases
Seed seed_at(const std::string &s, size_t i)
{
    Seed d{0u, 0u};
    while (d.len < kSeedMax && i + d.len < s.size() && is_base(s[i + d.len])) {
        const uint64_t c = (uint64_t)std::string("ACGT").find(s[i + d.len]);
        d.code |= c << (46u - 2u * d.len);
        d.len++;
    }
    return d;
}

std::string mutate(std::string s, uint32_t every)
{
    for (size_t i = draw(every); i < s.size(); i += 1 + draw(2 * every)) s[i] = "ACGT"[draw(4)];
    return s;
}

} // namespace

int main()
{
    std::string ancestor;
    for (int i = 0; i < 400; i++) ancestor += "ACGT"[draw(4)];
    std::vector<std::string> refs;
    for (int r = 0; r < 6; r++) refs.push_back(mutate(ancestor, 8 + 6 * r));
    refs[1][100] = 'N';
    refs[1][117] = 'N'; // a stretch of 16 bases: shorter than a seed
    refs[2][200] = 'a';
    refs.push_back("ACGTACGTACGTACGTACGTACGTACGTACGTAC"); // a repeat: equal codes in one bucket
    refs.push_back("ACGTACGTAC");                         // shorter than kSeedMin: entries no seed can reach

    // the table, as refset.cpp builds it
    std::vector<std::pair<uint64_t, uint32_t>> entries;
    size_t n_seeds = 0;
    for (size_t r = 0; r < refs.size(); r++)
        for (const std::string &st : stretches(refs[r])) {
            Seed seed{0u, 0u};
            for (size_t i = st.size(); i-- > 0;) {
                seed = step_left(seed, (uint8_t)st[i]);
                const Seed want = seed_at(st, i);
                if (seed.code != want.code || seed.len != want.len) fail("reference seed", r, i);
                entries.emplace_back(key_of(seed), (uint32_t)r);
                n_seeds++;
            }
        }
    std::sort(entries.begin(), entries.end());
    Table t;
    t.bucket_.assign((size_t)kBuckets + 1, 0u);
    for (const auto &e : entries) {
        t.key_.push_back(e.first);
        t.ref_.push_back(e.second);
        t.bucket_[(size_t)bucket_of(e.first >> 16) + 1]++;
    }
    for (size_t b = 0; b < kBuckets; b++) t.bucket_[b + 1] += t.bucket_[b];

    std::vector<std::string> queries;
    for (int q = 0; q < 6; q++) queries.push_back(mutate(ancestor, 5 + 7 * q));
    queries[0][50] = 'N';
    queries[1][60] = 'c';
    queries.push_back(ancestor.substr(37, kSeedMin));      // exactly a bucket's bases
    queries.push_back(ancestor.substr(41, kSeedMin - 1));  // one fewer: nothing is looked up
    queries.push_back(ancestor.substr(300));               // ends where the ancestor ends
    queries.push_back("ACGTACGTACGTACGTACGTACGTACGTAC");
    queries.push_back("NNNN");
    queries.push_back("");

    size_t n_cases = 0, n_marked = 0;
    for (size_t q = 0; q < queries.size(); q++) {
        const std::string &s = queries[q];
        // got[m][r]: some position shares at least m bases with some entry of r
        std::vector<std::vector<char>> got(kSeedMax + 1, std::vector<char>(refs.size(), 0));
        Seed seed{0u, 0u};
        for (size_t i = s.size(); i-- > 0;) {
            seed = step_left(seed, (uint8_t)s[i]);
            const Seed want = seed_at(s, i);
            if (seed.code != want.code || seed.len != want.len) fail("query seed", q, i);
            n_seeds++;
            scan(t, seed, [&](uint32_t r, uint32_t shared) {
                if (r >= refs.size() || shared > kSeedMax || shared > seed.len) fail("hit", r, shared);
                for (uint32_t m = kSeedMin; m <= shared; m++) got[m][r] = 1;
            });
        }
        for (uint32_t m = kSeedMin; m <= kSeedMax; m++)
            for (size_t r = 0; r < refs.size(); r++) {
                std::set<std::string> mers;
                for (const std::string &st : stretches(refs[r]))
                    for (size_t i = 0; i + m <= st.size(); i++) mers.insert(st.substr(i, m));
                char want = 0;
                for (const std::string &st : stretches(s))
                    for (size_t i = 0; i + m <= st.size(); i++) want |= (char)mers.count(st.substr(i, m));
                if (want != got[m][r]) fail("candidate", q * 100 + m, r);
                n_cases++;
                n_marked += (size_t)want;
            }
    }
    std::printf("%zu seeds, %zu cases agree, %zu marked\n", n_seeds, n_cases, n_marked);
    return 0;
}
