// refset_cover_check.cpp — the arithmetic of the reference-set cover (kbo_amd/csrc/refset_cover.hpp) on the CPU: the count of a run's
// anchors into H, the in-place scan with its 64-wide tile and carry, and the reduce with its tile carries, through accessors that
// check every index against the size of H and of the profile: an index out of range is counted and fails the run.  The inputs are made
// here - references of lengths around k and around the tile, runs whose windows' entries are drawn at random (FWD, REV and MULTI
// entries, none, and entries that name no base of the reference) or planted (hit starts at 0 and at L - k, k and k + 1 apart, segment
// boundaries at 63|64 and 127|128) - and the yardstick is brute force over them, made here too: H by a loop, D by its definition's
// double loop, every field of the record from D.  No GPU, no library: a stand-alone program, meant to run under sanitizers.
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -I kbo_amd/csrc tools/refset_cover_check.cpp -o refset_cover_check
//   ./refset_cover_check
#include "refset_cover.hpp"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

namespace {

namespace lc = kbo::reflocate;
namespace cv = kbo::refcover;

uint64_t g_bad = 0, g_reads = 0, g_writes = 0;

struct CheckedWords {
    std::vector<uint32_t> *h; // exactly the words: the sanitizer sees an access behind them
    uint32_t get(uint64_t i) const
    {
        g_reads++;
        if (i >= h->size()) {
            g_bad++;
            return 0u;
        }
        return (*h)[(size_t)i];
    }
    void set(uint64_t i, uint32_t v)
    {
        g_writes++;
        if (i >= h->size()) g_bad++;
        else (*h)[(size_t)i] = v;
    }
    void add(uint64_t i)
    {
        g_writes++;
        if (i >= h->size()) g_bad++;
        else (*h)[(size_t)i]++;
    }
};
struct CheckedDepth {
    std::vector<uint32_t> *d;
    void put(uint64_t i, uint32_t v)
    {
        g_writes++;
        if (i >= d->size()) g_bad++;
        else (*d)[(size_t)i] = v;
    }
};

struct Run {
    uint32_t ref, start, end;
    std::vector<uint32_t> entries; // the entry of the window at start + i
};

// one world: references of the lengths given, back to back in H, and runs over them; true when the library's forms and brute force agree
bool check_world(const std::vector<uint32_t> &lens, uint32_t k, const std::vector<Run> &runs, bool with_depth, uint64_t *cases)
{
    const size_t n = lens.size();
    std::vector<uint64_t> off(n + 1, 0);
    for (size_t r = 0; r < n; r++) off[r + 1] = off[r] + lens[r];
    std::vector<uint32_t> h((size_t)off[n], 0u), depth(with_depth ? (size_t)off[n] : 0u, 0xA5A5A5A5u);
    h.shrink_to_fit();
    depth.shrink_to_fit();
    CheckedWords H{&h};
    CheckedDepth D{&depth};
    std::vector<uint64_t> anchors(n, 0), multi(n, 0), b_anchors(n, 0), b_multi(n, 0);
    std::vector<uint32_t> n_runs(n, 0);
    std::vector<std::vector<uint32_t>> b_h(n);
    for (size_t r = 0; r < n; r++) b_h[r].assign(lens[r], 0u);
    for (const Run &w : runs) {
        cv::count_serial(H, off[w.ref], lens[w.ref], w.start, w.end, k, [&](uint32_t i) { return w.entries.at(i - w.start); }, anchors[w.ref],
                         multi[w.ref]);
        n_runs[w.ref]++;
        if (w.end - w.start >= k)
            for (uint32_t i = 0; i + k <= w.end - w.start; i++) {
                const uint32_t e = w.entries[i], p = e & lc::kPosMask;
                if (e == lc::kPosNone || p >= lens[w.ref]) continue;
                b_h[w.ref][p]++;
                b_anchors[w.ref]++;
                if (e & lc::kMulti) b_multi[w.ref]++;
            }
    }
    uint64_t wrong = 0;
    for (size_t r = 0; r < n; r++) {
        const uint32_t L = lens[r];
        for (uint32_t p = 0; p < L; p++) wrong += h[(size_t)off[r] + p] != b_h[r][p];
        cv::scan_serial(H, off[r], L);
        uint32_t sum = 0;
        for (uint32_t p = 0; p < L; p++) {
            sum += b_h[r][p];
            wrong += h[(size_t)off[r] + p] != sum;
        }
        const cv::Tally t = cv::reduce_serial(H, off[r], L, k, with_depth ? &D : nullptr, off[r]);
        const cv::Cover got = cv::finish(L, t, n_runs[r], anchors[r], multi[r]);
        // brute force: D by the definition, the record from D
        std::vector<uint32_t> d(L, 0u);
        for (uint32_t j = 0; j < L; j++)
            for (uint32_t p = j + 1u >= k ? j + 1u - k : 0u; p <= j; p++) d[j] += b_h[r][p];
        cv::Cover exp{L, 0u, 0u, cv::kNone, cv::kNone, 0u, n_runs[r], 0u, b_anchors[r], b_multi[r]};
        uint64_t total = 0;
        for (uint32_t j = 0; j < L; j++) {
            total += d[j];
            if (!d[j]) continue;
            exp.covered++;
            if (j == 0 || !d[j - 1]) exp.n_segments++;
            if (exp.first == cv::kNone) exp.first = j;
            exp.last = j;
            exp.max_depth = std::max(exp.max_depth, d[j]);
        }
        wrong += std::memcmp(&got, &exp, sizeof got) != 0;
        wrong += total != (uint64_t)k * b_anchors[r] || (exp.covered == 0) != (b_anchors[r] == 0);
        if (with_depth)
            for (uint32_t j = 0; j < L; j++) wrong += depth[(size_t)off[r] + j] != d[j];
        if (cases) {
            cases[0] += L >= 65 && (d[63] != 0) != (d[64] != 0);
            cases[1] += L >= 129 && (d[127] != 0) != (d[128] != 0);
            cases[2] += L > 0 && b_h[r][0] != 0;
            cases[3] += L >= k && b_h[r][L - k] != 0;
            cases[4] += exp.n_segments >= 2;
            cases[5] += b_multi[r] != 0;
            cases[6] += exp.max_depth >= 2;
            cases[7] += exp.covered == L && L > 0;
        }
    }
    return wrong == 0;
}

Run planted(uint32_t ref, std::initializer_list<uint32_t> ps, uint32_t k)
{
    Run w{ref, 10u, 10u + k - 1u + (uint32_t)ps.size(), {}};
    for (uint32_t p : ps) w.entries.push_back(p);
    return w;
}

} // namespace

int main()
{
    uint64_t worlds = 0, failed = 0, cases[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    std::mt19937_64 rng(20240607u);
    for (uint32_t k : {1u, 5u, 31u, 64u, 96u}) {
        const std::vector<uint32_t> lens{k, k + 1u, 63u + k, 63u, 64u, 65u, 127u, 128u, 129u, 300u, 0u, 1000u};
        // random runs: up to 200 windows each, entries anywhere - also behind the reference's end, which must count nowhere
        for (int round = 0; round < 6; round++) {
            std::vector<Run> runs;
            for (int x = 0; x < 40; x++) {
                Run w;
                w.ref = (uint32_t)(rng() % lens.size());
                w.start = (uint32_t)(rng() % 1000u);
                const uint32_t windows = (uint32_t)(rng() % 200u);
                w.end = w.start + (windows ? windows + k - 1u : (uint32_t)(rng() % k)); // (no window: a run shorter than k)
                for (uint32_t i = 0; i < windows; i++) {
                    const uint64_t v = rng();
                    uint32_t e = lc::kPosNone;
                    if (v % 4u && lens[w.ref] >= k)
                        e = (uint32_t)((v >> 8) % (lens[w.ref] - k + 1u)) | ((v >> 40) & 1u ? lc::kRev : 0u) | ((v >> 41) % 4u == 0 ? lc::kMulti : 0u);
                    else if (v % 4u && (v >> 50) % 2u)
                        e = lens[w.ref] + (uint32_t)((v >> 8) % 70u); // names no base of the reference
                    w.entries.push_back(e);
                }
                if (round == 5 && x % 2) runs.push_back(w); // (the same record twice)
                runs.push_back(w);
            }
            worlds++;
            failed += !check_world(lens, k, runs, round % 2 == 0, nullptr);
        }
        // planted: reference 9 has 300 bases, reference 11 has 1000
        if (k <= 64) {
            std::vector<Run> runs{planted(9, {0u, 300u - k}, k),          planted(11, {100u, 100u + k}, k), planted(11, {400u, 400u + k + 1u}, k),
                                  planted(9, {64u}, k),                   planted(11, {128u - k + 600u}, k), planted(9, {128u - k}, k),
                                  planted(8, {(129u - k) | lc::kMulti}, k),    planted(7, {5u, 5u}, k),           planted(0, {0u}, k),
                                  planted(1, {0u, 1u | lc::kRev}, k)};
            if (k <= 63) runs.push_back(planted(3, {63u - k}, k)), runs.push_back(planted(5, {64u - k}, k));
            worlds++;
            failed += !check_world(lens, k, runs, true, cases);
        }
    }
    // a run without windows on a reference without bases, and nothing at all
    worlds += 2;
    failed += !check_world({0u, 7u}, 3u, {Run{0u, 5u, 5u, {}}, Run{1u, 0u, 2u, {}}}, true, nullptr);
    failed += !check_world({}, 3u, {}, true, nullptr);
    // the flags and the layout of the scratch
    const cv::Cover over = cv::finish(10u, cv::no_tally(), 1u, 1ull << 32, 0u), under = cv::finish(10u, cv::no_tally(), 1u, (1ull << 32) - 1u, 0u);
    const cv::Cover none = cv::no_entries(9u);
    if (over.flags != cv::kFlagOverflow || under.flags != 0u || none.flags != cv::kFlagNoEntries || none.ref_len != 9u || none.first != cv::kNone ||
        none.last != cv::kNone || none.covered || sizeof(cv::Cover) != 48u || cv::counter_bytes(1) != 32u || cv::counter_bytes(2) != 48u ||
        cv::work_bytes(3, 5) != 80u + 32u || cv::work_bytes(0, 0) != 0u)
        failed++;
    for (int c = 0; c < 8; c++)
        if (!cases[c]) {
            std::fprintf(stderr, "planted case %d did not occur\n", c);
            return 1;
        }
    if (failed) {
        std::fprintf(stderr, "%llu of %llu worlds differ from brute force\n", (unsigned long long)failed, (unsigned long long)worlds);
        return 1;
    }
    if (g_bad) {
        std::fprintf(stderr, "%llu indexes out of range\n", (unsigned long long)g_bad);
        return 1;
    }
    std::printf("refset_cover_check: %llu worlds agree with brute force; %llu reads and %llu writes in range\n", (unsigned long long)worlds,
                (unsigned long long)g_reads, (unsigned long long)g_writes);
    return 0;
}
