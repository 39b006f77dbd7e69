// map_subst_check.cpp — the bit per text position that settles a lone substitution in map_reads_kernel's stage 3
// (kbo_amd/csrc/map_subst.hpp) on the CPU, against a brute-force set of strings.  Random texts of 200 to 3 000 positions over 2 and 4
// letters (so that one-base neighbours that ARE in the set are common) with the padding of pack_text_kernel and marks planted as
// tools/map_text_check.cpp plants them; `order` 4 .. 9, thresholds order .. order + 8, with and without anchors.  The set holds every
// string of `order` bases of the text that crosses no mark.  The bitmap is made by the header's clean() at the size the device copy
// allocates, and looked up as the kernel does: bit_of(p0, m) through an accessor that checks the index.
//   (i)  for every position whose bit is set, every base b != the text's, every read length 3 .. 160 and the placements that put the
//        substitution at read base 0, 1, order - 2, order - 1, order, the middle and their mirror images at the read's end: the read is
//        made (the text on its diagonal with b at the position), its list of mismatches is made by comparing it with the text and its
//        marks, the entry must be eligible, and every window that stage 3 would ask - the header's offsets under the kernel's `use`
//        condition, the strings taken from the READ - must be absent from the set
//   (ii) eligible() accepts another list entry `order` bases away and rejects one order - 1 bases away, on either side
// --leave-out I makes the bitmap with window I of the proof left out of clean(): the program must then FAIL (i) - that the check can
// tell.  No GPU, no library: a stand-alone program, meant to run under sanitizers.
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -I kbo_amd/csrc tools/map_subst_check.cpp -o map_subst_check
//   ./map_subst_check
#include "map_subst.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

namespace {

namespace ms = kbo::mapsubst;

uint64_t pack_text_units(uint64_t n) { return (n + ms::kPad + 256u) / 16u + 2u; } // == kbo::pack_text_units (kernels.hpp needs the HIP headers)

uint64_t g_bad = 0, g_loads = 0;

struct Text { // pc_tm at the size the device copy allocates, and the set of strings
    uint64_t n_units = 0;
    std::vector<uint32_t> d, m; // pc_tm[u].x, .y
    uint32_t order = 0;
    std::vector<uint8_t> set;   // 4^order entries: the string is in the index
};
struct CheckedText {
    const Text *x;
    bool ok(uint64_t q) const
    {
        g_loads++;
        if ((q >> 4) < x->n_units) return true;
        g_bad++;
        return false;
    }
    uint64_t positions() const { return 16u * x->n_units; }
    bool marked(uint64_t q) const { return ok(q) ? (x->m[(size_t)(q >> 4)] >> (2u * (15u - (uint32_t)(q & 15u)))) & 1u : true; }
    uint32_t base(uint64_t q) const { return ok(q) ? (x->d[(size_t)(q >> 4)] >> (2u * (15u - (uint32_t)(q & 15u)))) & 3u : 0u; }
};
struct CheckedTable {
    const Text *x;
    bool present(uint64_t key) const
    {
        g_loads++;
        if (key < x->set.size()) return x->set[(size_t)key] != 0;
        g_bad++;
        return true;
    }
};
struct CheckedBits { // the device copy allocates bitmap_words(n_units) words + 64 bytes
    const std::vector<uint32_t> *w;
    uint32_t word(uint64_t i) const
    {
        g_loads++;
        if (i < w->size()) return (*w)[(size_t)i];
        g_bad++;
        return 0u;
    }
};

Text pack(const std::vector<uint8_t> &digit, const std::vector<uint8_t> &mark, uint32_t order)
{
    Text x;
    const int64_t n = (int64_t)digit.size();
    x.n_units = pack_text_units((uint64_t)n);
    x.d.assign(x.n_units, 0u);
    x.m.assign(x.n_units, 0u);
    for (uint64_t u = 0; u < x.n_units; u++)
        for (uint32_t j = 0; j < 16u; j++) {
            const int64_t p = 16 * (int64_t)u - (int64_t)ms::kPad + j;
            const bool in = p >= 0 && p < n;
            x.d[u] = (x.d[u] << 2) | (in ? digit[(size_t)p] : 0u);
            x.m[u] = (x.m[u] << 2) | ((!in || mark[(size_t)p]) ? 1u : 0u);
        }
    x.order = order;
    x.set.assign((size_t)1 << (2u * order), 0);
    for (int64_t s = 0; s + order <= n; s++) {
        uint64_t key = 0;
        bool whole = true;
        for (uint32_t j = 0; j < order; j++) {
            key = (key << 2) | digit[(size_t)(s + j)];
            whole = whole && !mark[(size_t)(s + j)];
        }
        if (whole) x.set[(size_t)key] = 1;
    }
    return x;
}

} // namespace

int main(int argc, char **argv)
{
    uint32_t leave_out = 0;
    if (argc == 3 && !strcmp(argv[1], "--leave-out")) leave_out = 1u << atoi(argv[2]);
    std::mt19937_64 rng(20261021);
    uint64_t clean_n = 0, dirty_n = 0, reads = 0, windows = 0, present = 0, not_eligible = 0, wrong_rule = 0, unadmitted_clean = 0, configs = 0;
    // (ii) the predicate itself
    for (uint32_t order = 4; order <= 9u; order++)
        for (uint32_t m = order; m < 100u; m += 7u) {
            const bool far = ms::eligible(false, false, false, true, m - order, m, true, m + order, order);
            const bool near_p = ms::eligible(false, false, false, true, m - (order - 1u), m, true, m + order, order);
            const bool near_n = ms::eligible(false, false, false, true, m - order, m, true, m + (order - 1u), order);
            const bool alone = ms::eligible(false, false, false, false, 0u, m, false, 0u, order);
            const bool never = ms::eligible(true, false, false, false, 0u, m, false, 0u, order) || ms::eligible(false, true, false, false, 0u, m, false, 0u, order) ||
                               ms::eligible(false, false, true, false, 0u, m, false, 0u, order);
            if (!far || near_p || near_n || !alone || never) wrong_rule++;
        }
    const char *pattern_name[5] = {"none", "one position", "first and last of a unit", "two adjacent units", "every third unit"};
    for (uint32_t trial = 0; trial < 24u; trial++) {
        const uint32_t letters = (trial & 1u) ? 4u : 2u, pattern = (trial >> 1) % 5u;
        const uint32_t n = trial < 2u ? 200u : trial < 4u ? 3000u : 200u + (uint32_t)(rng() % 2801u);
        const uint32_t order = 4u + (uint32_t)(rng() % 6u), thr = order + (trial < 10u ? trial % 9u : (uint32_t)(rng() % 9u));
        const bool anch_asked = (rng() & 1u) != 0, have_anch = anch_asked && thr > order; // (the kernel's have_anch: thr_gt)
        std::vector<uint8_t> digit(n), mark(n, 0);
        for (auto &d : digit) d = (uint8_t)(rng() % letters);
        const uint32_t j = (uint32_t)(rng() % (n / 16u));
        if (pattern == 1) mark[rng() % n] = 1;
        if (pattern == 2) mark[16u * j] = mark[16u * j + 15u] = 1;
        if (pattern == 3) mark[16u * (j % (n / 16u - 1u)) + (uint32_t)(rng() % 16u)] = mark[16u * (j % (n / 16u - 1u)) + 16u + (uint32_t)(rng() % 16u)] = 1;
        if (pattern == 4)
            for (uint32_t u = 0; 16u * u < n; u += 3u) mark[std::min(n - 1u, 16u * u + (uint32_t)(rng() % 16u))] = 1; // (every third: some positions stay clean)
        const Text x = pack(digit, mark, order);
        const CheckedText tx{&x};
        const CheckedTable tab{&x};
        // the bitmap, as the device makes it: a bit per position of every unit, slack of 64 bytes behind
        std::vector<uint32_t> bits((size_t)ms::bitmap_words(x.n_units) + 16u, 0u);
        for (uint64_t q = 0; q < 16u * x.n_units; q++)
            if (ms::clean(tx, tab, q, order, thr, have_anch, leave_out)) bits[(size_t)(q >> 5)] |= 1u << (q & 31u);
        const uint32_t cov = ms::window_step(order, thr, have_anch);
        // (the kernel takes the direct form only where the proof has at most kWindows windows: map_reads_direct)
        const bool admitted = (order - 1u + cov - 1u) / cov + 1u <= ms::kWindows;
        configs++;
        uint64_t clean_here = 0;
        for (int64_t p = -(int64_t)ms::kPad; p < (int64_t)n + 200; p++) {
            if ((uint64_t)(p + (int64_t)ms::kPad) >= 16u * x.n_units) break;
            // (what the kernel does: the diagonal and the read's base, mod 2^32)
            const bool is_clean = ms::clean_bit(CheckedBits{&bits}, ms::bit_of((uint32_t)(p - 5), 5u));
            if (!is_clean) {
                dirty_n++;
                continue;
            }
            clean_here++;
            if (!admitted) {
                unadmitted_clean++;
                continue;
            }
            if (p < 0 || p >= (int64_t)n) { // a clean position outside the text
                present++;
                continue;
            }
            for (uint32_t len = 3; len <= 160u; len++) {
                const uint32_t cand[11] = {0u, 1u, order - 2u, order - 1u, order, len / 2u, len - 1u, len - 2u, len - (order - 1u), len - order, len - order - 1u};
                for (uint32_t ci = 0; ci < 11u; ci++) {
                    const uint32_t m = cand[ci];
                    if (m >= len) continue; // (len - order .. wrap for short reads)
                    bool again = false;
                    for (uint32_t cj = 0; cj < ci; cj++) again = again || cand[cj] == m;
                    if (again) continue;
                    const int64_t p0 = p - (int64_t)m;
                    for (uint32_t b = 0; b < 4u; b++) {
                        if (b == digit[(size_t)p]) continue;
                        // the read, and its list as the compare step makes it: bases that differ from the text or stand on a mark
                        uint8_t read[160];
                        uint32_t list[160], cnt = 0, t_of_m = 0;
                        for (uint32_t i = 0; i < len; i++) {
                            const int64_t tp = p0 + i;
                            const bool in = tp >= 0 && tp < (int64_t)n;
                            read[i] = i == m ? (uint8_t)b : (in ? digit[(size_t)tp] : (uint8_t)0);
                            if (i == m || !in || mark[(size_t)tp]) {
                                if (i == m) t_of_m = cnt;
                                list[cnt++] = i;
                            }
                        }
                        reads++;
                        const bool has_prev = t_of_m > 0u, has_next = t_of_m + 1u < cnt;
                        if (!ms::eligible(false, false, false, has_prev, has_prev ? list[t_of_m - 1u] : 0u, m, has_next, has_next ? list[t_of_m + 1u] : 0u, order)) {
                            not_eligible++; // (a set bit with a mark within order - 1 bases: clean() (a) is wrong)
                            continue;
                        }
                        if (ms::bit_of((uint32_t)p0, m) != (uint64_t)(p + (int64_t)ms::kPad)) wrong_rule++;
                        for (uint32_t i = 0; i < ms::kWindows; i++) {
                            const uint32_t e = m + ms::window_offset(i, cov, order, 0u);
                            const bool use = e < len && e + 1u >= order && ms::window_used(i, cov, order, 0u); // (stage 3's own condition)
                            if (!use) continue;
                            uint64_t key = 0;
                            for (uint32_t jj = 0; jj < order; jj++) key = (key << 2) | read[e + 1u - order + jj];
                            windows++;
                            if (x.set[(size_t)key]) present++;
                        }
                    }
                }
            }
        }
        clean_n += clean_here;
        if (leave_out && present) break; // (the self-test has its answer)
        printf("text of %4u positions over %u letters, marks: %-26s order %u, threshold %2u, %s anchors%s: %llu clean positions\n", n, letters, pattern_name[pattern],
               order, thr, have_anch ? "with" : "no  ", admitted ? "" : " (not the direct form's)", (unsigned long long)clean_here);
    }
    const bool fail = g_bad || present || not_eligible || wrong_rule || unadmitted_clean || clean_n == 0 || dirty_n == 0 || windows == 0;
    printf("%llu configurations, %llu clean and %llu dirty positions, %llu reads, %llu windows, %llu loads: %s, %s, %s\n", (unsigned long long)configs,
           (unsigned long long)clean_n, (unsigned long long)dirty_n, (unsigned long long)reads, (unsigned long long)windows, (unsigned long long)g_loads,
           g_bad ? "INDEX OUT OF RANGE" : "every index in range", (present || not_eligible || unadmitted_clean) ? "A CLEAN POSITION HAS A PRESENT WINDOW" : "every window of a clean position is absent",
           wrong_rule ? "THE PREDICATE IS WRONG" : "the predicate holds");
    if (present) printf("%llu windows of clean positions are in the set\n", (unsigned long long)present);
    if (not_eligible) printf("%llu reads over a clean position are not eligible\n", (unsigned long long)not_eligible);
    if (unadmitted_clean) printf("%llu clean positions where the proof has more than %u windows\n", (unsigned long long)unadmitted_clean, ms::kWindows);
    return fail ? 1 : 0;
}
