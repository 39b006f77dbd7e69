// refset_step_check.cpp — the step of the reference-set walks (kbo_amd/csrc/refset_step.hpp) on the CPU over a packed form read from a
// file (kbo_refset_form's bytes), through an accessor that checks every rank block and every LCS index against the form's size: the
// depths of a query go to a file, and an index out of range is counted and fails the run.  No GPU, no library: a stand-alone
// program, meant to run under sanitizers.
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -I kbo_amd/csrc tools/refset_step_check.cpp -o refset_step_check
//   ./refset_step_check FORM QUERY ROWS K DEPTHS_OUT
#include "refset_step.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace {

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

struct CheckedForm {
    const std::vector<uint8_t> *form; // exactly the form's bytes: the sanitizer sees a read behind them
    uint64_t n;
    mutable uint64_t bad = 0, ranks = 0, lcs_reads = 0;
    kbo::refstep::Entry rank(uint32_t block, uint32_t c) const
    {
        ranks++;
        if (block > n / 32u || c > 3u) {
            bad++;
            return kbo::refstep::Entry{0u, 0u};
        }
        kbo::refstep::Entry e;
        std::memcpy(&e, form->data() + ((size_t)block * 4u + c) * 8u, 8);
        return e;
    }
    uint32_t lcs(uint32_t i) const
    {
        lcs_reads++;
        if (i > n) { // (l-- below row 0 wraps to 2^32 - 1: caught here too)
            bad++;
            return 0u;
        }
        return (*form)[(size_t)rank_units(n) * 16u + i];
    }
};

} // namespace

int main(int argc, char **argv)
{
    if (argc != 6) {
        std::fprintf(stderr, "usage: %s FORM QUERY ROWS K DEPTHS_OUT\n", argv[0]);
        return 2;
    }
    std::vector<uint8_t> form, query;
    if (!read_file(argv[1], form) || !read_file(argv[2], query)) {
        std::fprintf(stderr, "cannot read the form or the query\n");
        return 2;
    }
    const uint64_t n = std::strtoull(argv[3], nullptr, 10), k = std::strtoull(argv[4], nullptr, 10);
    if (n == 0 || n >= (1ull << 32) - 32u || k == 0 || k > 255 || form.size() != units(n) * 16u) {
        std::fprintf(stderr, "a form of %zu bytes is not that of %llu rows (%llu bytes), or k is outside 1 .. 255\n", form.size(),
                     (unsigned long long)n, (unsigned long long)(units(n) * 16u));
        return 2;
    }
    form.shrink_to_fit();
    CheckedForm x{&form, n};
    if (x.lcs(0) != 0 || x.lcs((uint32_t)n) != 0) {
        std::fprintf(stderr, "LCS[0] and the sentinel LCS[n] must be 0: the scans end at them\n");
        return 1;
    }
    std::vector<uint8_t> depths(query.size());
    uint32_t l = 0, r = (uint32_t)n, d = 0;
    for (size_t i = 0; i < query.size(); i++) {
        kbo::refstep::step(x, (uint32_t)n, (uint32_t)k, query[i], l, r, d);
        if (l >= r || r > n || d > k) x.bad++;
        depths[i] = (uint8_t)d;
    }
    std::FILE *f = std::fopen(argv[5], "wb");
    if (!f || std::fwrite(depths.data(), 1, depths.size(), f) != depths.size()) {
        std::fprintf(stderr, "cannot write the depths\n");
        return 2;
    }
    std::fclose(f);
    if (x.bad) {
        std::fprintf(stderr, "%llu indexes out of range\n", (unsigned long long)x.bad);
        return 1;
    }
    std::printf("refset_step_check: %zu bases, %llu ranks and %llu LCS reads in range\n", query.size(), (unsigned long long)x.ranks,
                (unsigned long long)x.lcs_reads);
    return 0;
}
