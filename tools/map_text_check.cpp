// map_text_check.cpp — the window arithmetic of map_reads_kernel's compare step (kbo_amd/csrc/map_text.hpp) on the CPU: the form over the
// interleaved text (pc_tm: digits and marks, what the kernel read before) against the form over the split arrays (pc_t, the summary bits
// pc_mu and the coarse summary pc_mc, with the marks of marked units alone from pc_tm), through accessors that check every index against
// the arrays' sizes: an index out of range is counted and fails the run.  The texts are made here - 50 to 2 000 positions with the
// padding of pack_text_kernel, marks planted nowhere, at one position, at the first and the last position of a unit, in two adjacent
// units and in every unit - and packed into both layouts here.  Compared: every word of the mismatch masks and their count for every
// diagonal from in front of the text to behind it (so every alignment 0 .. 15), every length 1 .. 160, and stage 2b's three-unit look
// with its verdict at both ends of every such window.  No GPU, no library: a stand-alone program, meant to run under sanitizers.
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -I kbo_amd/csrc tools/map_text_check.cpp -o map_text_check
//   ./map_text_check
#include "map_text.hpp"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

namespace {

namespace mt = kbo::maptext;

constexpr uint32_t kMapPad = 192; // == kbo::kMapPad (kernels.hpp needs the HIP headers; the values are compared in map_kernels.hip's build)
uint64_t pack_text_units(uint64_t n) { return (n + kMapPad + 256u) / 16u + 2u; }
uint64_t pack_text_mu_bytes(uint64_t n_units) { return (n_units + 255u) / 256u * 32u; }

uint64_t g_bad = 0, g_loads = 0;

struct Text { // both layouts, at exactly the sizes the device copy allocates
    uint64_t n_units = 0;
    std::vector<uint32_t> tm_d, tm_m; // pc_tm[u].x, .y: n_units (its slack is never read)
    std::vector<uint32_t> t;          // pc_t: n_units words + 16 of slack
    std::vector<uint8_t> mu;          // pc_mu: pack_text_mu_bytes + 64
    std::vector<uint32_t> mc;         // pc_mc: kCells bits
    uint32_t shift = 0;
};

struct CheckedUnits {
    const Text *x;
    bool ok(uint64_t u) const
    {
        g_loads++;
        if (u < x->n_units) return true;
        g_bad++;
        return false;
    }
    void pair(uint64_t u, uint32_t (&d)[2], uint32_t (&m)[2]) const
    {
        for (uint32_t i = 0; i < 2; i++) {
            const bool in = ok(u + i);
            d[i] = in ? x->tm_d[(size_t)(u + i)] : 0u;
            m[i] = in ? x->tm_m[(size_t)(u + i)] : 0u;
        }
    }
    void unit(uint64_t u, uint32_t &d, uint32_t &m) const
    {
        const bool in = ok(u);
        d = in ? x->tm_d[(size_t)u] : 0u;
        m = in ? x->tm_m[(size_t)u] : 0u;
    }
    uint32_t marks(uint64_t u) const { return ok(u) ? x->tm_m[(size_t)u] : 0u; }
};
struct CheckedDigits {
    const Text *x;
    uint32_t word(uint64_t u) const
    {
        g_loads++;
        if (u < x->t.size()) return x->t[(size_t)u];
        g_bad++;
        return 0u;
    }
    void quad(uint64_t u, uint32_t (&d)[4]) const
    {
        for (uint32_t i = 0; i < 4; i++) d[i] = word(u + i);
    }
};
struct CheckedBits {
    const Text *x;
    uint32_t from(uint64_t u) const
    {
        g_loads++;
        const uint64_t b = u >> 3;
        if (b + 4u > x->mu.size()) {
            g_bad++;
            return 0u;
        }
        uint32_t w;
        memcpy(&w, x->mu.data() + b, 4);
        return w >> (uint32_t)(u & 7u);
    }
};
struct HostAny {
    bool operator()(bool b) const { return b; }
};

// positions 0 .. n - 1 hold random digits; `mark[p]` plants a mark (a path start) at p; everything outside the text is padding
Text pack(const std::vector<uint8_t> &digit, const std::vector<uint8_t> &mark)
{
    Text x;
    const int64_t n = (int64_t)digit.size();
    x.n_units = pack_text_units((uint64_t)n);
    x.tm_d.assign(x.n_units, 0u);
    x.tm_m.assign(x.n_units, 0u);
    x.t.assign(x.n_units + 16u, 0u);
    const uint64_t mu_bytes = pack_text_mu_bytes(x.n_units);
    x.mu.assign(mu_bytes + 64u, 0xFFu);
    for (uint64_t b = 0; b < mu_bytes; b++) x.mu[b] = 0;
    for (uint64_t u = 0; u < mu_bytes * 8u; u++) {
        uint32_t d = 0, m = u < x.n_units ? 0u : 0x55555555u;
        if (u < x.n_units)
            for (uint32_t j = 0; j < 16u; j++) {
                const int64_t p = 16 * (int64_t)u - (int64_t)kMapPad + j;
                const bool in = p >= 0 && p < n;
                d = (d << 2) | (in ? digit[(size_t)p] : 0u);
                m = (m << 2) | ((!in || mark[(size_t)p]) ? 1u : 0u);
            }
        if (u < x.n_units) {
            x.tm_d[u] = d;
            x.tm_m[u] = m;
            x.t[u] = d;
        }
        if (m) x.mu[u >> 3] |= (uint8_t)(1u << (u & 7u));
    }
    x.shift = mt::cell_shift(x.n_units);
    x.mc.assign(mt::kCells / 32u, 0u);
    for (uint32_t c = 0; c < mt::kCells; c++)
        if (mt::cell_marked(CheckedBits{&x}, c, x.shift, x.n_units)) x.mc[c >> 5] |= 1u << (c & 31u);
    return x;
}

bool near_mark(const Text &x, uint64_t q)
{
    const uint32_t c = mt::cell_of(q >> 4, x.shift);
    if (c >= mt::kCells) {
        g_bad++;
        return true;
    }
    return (x.mc[c >> 5] >> (c & 31u)) & 1u;
}

} // namespace

int main()
{
    std::mt19937_64 rng(20261020);
    uint64_t windows = 0, looks = 0, differ = 0, marked_windows = 0, far_windows = 0;
    const char *pattern_name[5] = {"none", "one position", "first and last of a unit", "two adjacent units", "every unit"};
    for (uint32_t size_i = 0; size_i < 3u; size_i++) {
        const uint32_t n = size_i == 0 ? 50u : size_i == 1 ? 2000u : 50u + (uint32_t)(rng() % 1951u);
        for (uint32_t pattern = 0; pattern < 5u; pattern++) {
            std::vector<uint8_t> digit(n), mark(n, 0);
            for (auto &d : digit) d = (uint8_t)(rng() & 3u);
            // (unit u of the text holds positions 16 u - kMapPad ..: kMapPad is a multiple of 16, so positions 16 j .. 16 j + 15 share a unit)
            const uint32_t j = (uint32_t)(rng() % (n / 16u));
            if (pattern == 1) mark[rng() % n] = 1;
            if (pattern == 2) mark[16u * j] = mark[16u * j + 15u] = 1;
            if (pattern == 3 && n >= 48u) mark[16u * (j % (n / 16u - 1u)) + (uint32_t)(rng() % 16u)] = mark[16u * (j % (n / 16u - 1u)) + 16u + (uint32_t)(rng() % 16u)] = 1;
            if (pattern == 4)
                for (uint32_t u = 0; 16u * u < n; u++) mark[std::min(n - 1u, 16u * u + (uint32_t)(rng() % 16u))] = 1;
            const Text x = pack(digit, mark);
            const CheckedUnits tm{&x};
            const CheckedDigits tx{&x};
            const CheckedBits mu{&x};
            // diagonals: a seed places a read's base e < 160 on a text position, and stage 2b moves three bases to either side
            for (int64_t pd = -163; pd <= (int64_t)n + 3; pd++) {
                const uint64_t q0 = (uint64_t)(pd + (int64_t)kMapPad);
                for (uint32_t len = 1; len <= 160u; len++) {
                    // the read: the text on this diagonal with a few substitutions, or random bases
                    uint32_t qw[mt::kWords];
                    const uint32_t style = (uint32_t)(rng() % 4u);
                    for (uint32_t g = 0; g < mt::kWords; g++) {
                        uint32_t w = 0;
                        for (uint32_t b = 0; b < 16u; b++) {
                            const int64_t p = pd + 16 * (int64_t)g + b;
                            uint32_t d = (p >= 0 && p < (int64_t)n) ? digit[(size_t)p] : 0u;
                            if (style == 0 || (style == 1 && rng() % 50u == 0)) d = (uint32_t)(rng() & 3u);
                            w = (w << 2) | d;
                        }
                        qw[g] = 16u * g < len ? w : 0u;
                    }
                    uint32_t ma[mt::kWords], mb[mt::kWords];
                    const uint32_t ca = mt::compare_interleaved(tm, qw, q0, len, ma);
                    const bool near = near_mark(x, q0);
                    const uint32_t cb = mt::compare_split(tx, mu, tm, HostAny{}, near, qw, q0, len, mb);
                    windows++;
                    if (!near) far_windows++;
                    bool same = ca == cb;
                    for (uint32_t g = 0; g < mt::kWords; g++) same = same && ma[g] == mb[g];
                    if (!same) differ++;
                    // stage 2b: the read's last 16 bases around q0 + len - 19, its first 16 around q0 - 3
                    const uint64_t ends[2] = {q0 + len - 19u, q0 - 3u};
                    for (uint32_t e = 0; e < 2u; e++) {
                        uint32_t da[mt::kBeside], mka[mt::kBeside], db[mt::kBeside], mkb[mt::kBeside];
                        mt::beside_interleaved(tm, ends[e] >> 4, da, mka);
                        mt::beside_split(tx, mu, tm, HostAny{}, near_mark(x, ends[e]), ends[e] >> 4, db, mkb);
                        uint32_t ja, jb;
                        const uint32_t word = e ? qw[0] : (uint32_t)rng(), end8 = e ? 0xFFFF0000u : 0x0000FFFFu;
                        const uint32_t ba = mt::beside_best(da, mka, (uint32_t)ends[e], word, end8, ja), bb = mt::beside_best(db, mkb, (uint32_t)ends[e], word, end8, jb);
                        looks++;
                        bool s2 = ba == bb && ja == jb;
                        for (uint32_t i = 0; i < mt::kBeside; i++) {
                            s2 = s2 && da[i] == db[i] && mka[i] == mkb[i];
                            if (mka[i]) marked_windows++;
                        }
                        if (!s2) differ++;
                    }
                }
            }
            printf("text of %4u positions, marks: %-26s %u units, cells of %u units\n", n, pattern_name[pattern], (unsigned)x.n_units, 1u << x.shift);
        }
    }
    printf("%llu windows (%llu with no mark in sight by the coarse summary), %llu looks beside (%llu marked units seen), %llu loads: %s, %s\n",
           (unsigned long long)windows, (unsigned long long)far_windows, (unsigned long long)looks, (unsigned long long)marked_windows,
           (unsigned long long)g_loads, g_bad ? "INDEX OUT OF RANGE" : "every index in range", differ ? "THE FORMS DIFFER" : "both forms agree");
    if (g_bad) printf("%llu indexes out of range\n", (unsigned long long)g_bad);
    if (differ) printf("%llu windows differ\n", (unsigned long long)differ);
    return (g_bad || differ || far_windows == 0 || marked_windows == 0) ? 1 : 0;
}
