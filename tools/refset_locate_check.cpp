// refset_locate_check.cpp — the look-up of the reference-set locate (kbo_amd/csrc/refset_locate.hpp) on the CPU over a packed form and
// a position table read from files (kbo_refset_form's and kbo_refset_positions' bytes), through accessors that check every rank block,
// every byte of the batch and every row against the sizes: an index out of range is counted and fails the run.  The yardstick is brute
// force over the reference's bytes, made here: a map from every k-mer of every indexed stretch (and of its reverse complement with
// RC = 1) to its occurrences.  Checked against it: the entry of every k-mer's row, that no other row has one, and the first and last
// anchor, the flags and n_tested of runs over a query on both strands.  No GPU, no library: a stand-alone program, meant to run under
// sanitizers.
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -I kbo_amd/csrc tools/refset_locate_check.cpp -o refset_locate_check
//   ./refset_locate_check FORM POSITIONS REFERENCE QUERY ROWS K RC
#include "refset_locate.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <utility>
#include <vector>

namespace {

namespace lc = kbo::reflocate;

bool read_file(const char *path, std::vector<uint8_t> &out)
{
    std::FILE *f = std::fopen(path, "rb");
    if (!f) return false;
    uint8_t buf[1 << 16];
    for (size_t got; (got = std::fread(buf, 1, sizeof buf, f)) > 0;) out.insert(out.end(), buf, buf + got);
    std::fclose(f);
    return true;
}

// kernels.hpp refset_rank_units / refset_units, in 16-byte units
uint64_t rank_units(uint64_t n) { return 2u * (n / 32u + 1u); }
uint64_t units(uint64_t n) { return rank_units(n) + (n + 1u + 15u) / 16u; }

uint64_t g_bad = 0, g_ranks = 0, g_bytes = 0, g_rows = 0;

struct CheckedForm {
    const std::vector<uint8_t> *form; // exactly the form's bytes: the sanitizer sees a read behind them
    uint64_t n;
    kbo::refstep::Entry rank(uint32_t block, uint32_t c) const
    {
        g_ranks++;
        if (block > n / 32u || c > 3u) {
            g_bad++;
            return kbo::refstep::Entry{0u, 0u};
        }
        kbo::refstep::Entry e;
        std::memcpy(&e, form->data() + ((size_t)block * 4u + c) * 8u, 8);
        return e;
    }
};
struct CheckedSeq {
    const std::vector<uint8_t> *q;
    uint32_t byte(uint64_t i) const
    {
        g_bytes++;
        if (i >= q->size()) {
            g_bad++;
            return 'N';
        }
        return (*q)[(size_t)i];
    }
};
struct CheckedPos {
    const std::vector<uint8_t> *pos;
    uint64_t n;
    uint32_t entry(uint32_t row) const
    {
        g_rows++;
        if (row >= n) {
            g_bad++;
            return lc::kPosNone;
        }
        uint32_t e;
        std::memcpy(&e, pos->data() + (size_t)row * 4u, 4);
        return e;
    }
};

bool is_base(uint8_t b) { return b == 'A' || b == 'C' || b == 'G' || b == 'T'; }
uint8_t comp(uint8_t b) { return b == 'A' ? 'T' : b == 'C' ? 'G' : b == 'G' ? 'C' : b == 'T' ? 'A' : b; }
std::string revcomp(const std::string &s)
{
    std::string r(s.rbegin(), s.rend());
    for (char &c : r) c = (char)comp((uint8_t)c);
    return r;
}

using Occ = std::vector<std::pair<int, uint32_t>>; // (0: FWD, 1: REV; p)
uint32_t entry_of(const Occ &o)
{
    const auto m = *std::min_element(o.begin(), o.end());
    return m.second | (m.first ? lc::kRev : 0u) | (o.size() > 1 ? lc::kMulti : 0u);
}

} // namespace

int main(int argc, char **argv)
{
    if (argc != 8) {
        std::fprintf(stderr, "usage: %s FORM POSITIONS REFERENCE QUERY ROWS K RC\n", argv[0]);
        return 2;
    }
    std::vector<uint8_t> form, pos, ref, query;
    if (!read_file(argv[1], form) || !read_file(argv[2], pos) || !read_file(argv[3], ref) || !read_file(argv[4], query)) {
        std::fprintf(stderr, "cannot read an input\n");
        return 2;
    }
    const uint64_t n = std::strtoull(argv[5], nullptr, 10), k = std::strtoull(argv[6], nullptr, 10);
    const bool rc = std::atoi(argv[7]) != 0;
    if (n == 0 || n >= (1ull << 32) - 32u || k == 0 || k > 255 || form.size() != units(n) * 16u || pos.size() != n * 4u || ref.size() >= lc::kMaxRefLen) {
        std::fprintf(stderr, "the form or the table is not that of %llu rows, or k is outside 1 .. 255\n", (unsigned long long)n);
        return 2;
    }
    form.shrink_to_fit();
    pos.shrink_to_fit();
    query.shrink_to_fit();

    // brute force: the occurrences of every k-mer of every indexed stretch
    std::map<std::string, Occ> occ;
    for (size_t i = 0; i < ref.size();) {
        if (!is_base(ref[i])) {
            i++;
            continue;
        }
        size_t j = i;
        while (j < ref.size() && is_base(ref[j])) j++;
        if (j - i >= k)
            for (size_t p = i; p + k <= j; p++) {
                const std::string w(ref.begin() + p, ref.begin() + p + k);
                occ[w].emplace_back(0, (uint32_t)p);
                if (rc) occ[revcomp(w)].emplace_back(1, (uint32_t)p);
            }
        i = j;
    }

    const CheckedForm x{&form, n};
    const CheckedPos table{&pos, n};
    uint64_t wrong = 0;
    // the table: every k-mer's row holds its entry, and no other row holds one
    std::vector<uint8_t> seen(n, 0);
    for (const auto &kv : occ) {
        std::vector<uint8_t> km(kv.first.begin(), kv.first.end());
        km.shrink_to_fit();
        const CheckedSeq s{&km};
        const uint32_t row = lc::kmer_row(x, (uint32_t)n, (uint32_t)k, s, 0, k, false, 0);
        if (row == lc::kPosNone || row >= n || seen[row] || table.entry(row) != entry_of(kv.second)) wrong++;
        else seen[row] = 1;
        // ... and from the other strand: the reverse complement of the k-mer, read backwards, is the k-mer
        std::string other = revcomp(kv.first);
        std::vector<uint8_t> back(other.begin(), other.end());
        back.shrink_to_fit();
        const CheckedSeq s2{&back};
        if (lc::kmer_row(x, (uint32_t)n, (uint32_t)k, s2, 0, k, true, 0) != row) wrong++;
    }
    for (uint64_t row = 0; row < n; row++)
        if (!seen[row] && table.entry((uint32_t)row) != lc::kPosNone) wrong++;
    if (wrong) {
        std::fprintf(stderr, "%llu rows of the table differ from brute force\n", (unsigned long long)wrong);
        return 1;
    }

    // runs over the query on both strands: the whole sequence, and pieces at every phase of a group of windows
    const CheckedSeq q{&query};
    const uint64_t len = query.size();
    uint64_t runs = 0;
    for (int strand = 1; strand <= 2; strand++) {
        std::string s(query.begin(), query.end());
        if (strand == 2) s = revcomp(s);
        std::vector<uint32_t> hit(len, lc::kPosNone); // the entry of the window at i
        for (uint64_t i = 0; i + k <= len; i++) {
            const auto it = occ.find(s.substr(i, k));
            if (it != occ.end()) hit[i] = entry_of(it->second);
        }
        std::vector<std::pair<uint32_t, uint32_t>> spans{{0u, (uint32_t)len}, {(uint32_t)len, (uint32_t)len}, {0u, 0u}};
        for (uint32_t a = 0; a + 1 < len; a += 61)
            for (uint32_t n_b : {1u, (uint32_t)k - 1u, (uint32_t)k, (uint32_t)k + 1u, (uint32_t)k + 63u, (uint32_t)k + 64u, (uint32_t)k + 200u, 700u})
                if (a + n_b <= len) spans.emplace_back(a, a + n_b);
        for (const auto &sp : spans) {
            const uint32_t start = sp.first, end = sp.second;
            if (!lc::span_ok(0, len, len, start, end)) wrong++;
            const lc::Locus got = lc::locate_serial(start, end, (uint32_t)k, [&](uint32_t i) {
                return lc::kmer_entry(x, (uint32_t)n, (uint32_t)k, q, 0, len, strand == 2, table, i);
            });
            lc::Locus exp = lc::no_locus(0u);
            if (end - start >= k) {
                const uint32_t starts = end - start - (uint32_t)k + 1u;
                uint32_t first = lc::kPosNone, last = lc::kPosNone;
                for (uint32_t i = start; i < start + starts; i++)
                    if (hit[i] != lc::kPosNone) {
                        if (first == lc::kPosNone) first = i;
                        last = i;
                    }
                if (first == lc::kPosNone) exp.n_tested = starts;
                else {
                    lc::set_first(exp, first, hit[first]);
                    lc::set_last(exp, last, hit[last]);
                    const uint32_t a = ((first - start) / lc::kWindow + 1u) * lc::kWindow, b = ((start + starts - 1u - last) / lc::kWindow + 1u) * lc::kWindow;
                    exp.n_tested = std::min(a, starts) + std::min(b, starts);
                }
            }
            if (std::memcmp(&got, &exp, sizeof got) != 0) wrong++;
            runs++;
        }
    }
    if (lc::span_ok(5, 4, 10, 0, 0) || lc::span_ok(0, 11, 10, 0, 0) || lc::span_ok(0, 10, 10, 3, 2) || lc::span_ok(2, 10, 10, 0, 9)) wrong++;
    if (wrong) {
        std::fprintf(stderr, "%llu runs differ from brute force\n", (unsigned long long)wrong);
        return 1;
    }
    if (g_bad) {
        std::fprintf(stderr, "%llu indexes out of range\n", (unsigned long long)g_bad);
        return 1;
    }
    std::printf("refset_locate_check: %zu k-mers and %llu runs agree with brute force; %llu ranks, %llu bytes and %llu rows in range\n", occ.size(),
                (unsigned long long)runs, (unsigned long long)g_ranks, (unsigned long long)g_bytes, (unsigned long long)g_rows);
    return 0;
}
