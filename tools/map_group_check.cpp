// map_group_check.cpp — the clean groups of map_subst.hpp (sub_group: a bit per group of kGroup text positions, set where all of the
// group's bits of sub_clean are) on the CPU: the rule that makes them, the one load a read's window of them takes, and the dealing of
// what the owner lane leaves.  Random position bitmaps (mostly set, as the real ones are; mostly clear; half) and bitmaps with planted
// runs of set and clear bits, at the sizes the device copy allocates for texts of 200 to 3 000 positions.
//   (1) the group bits: bit G of group_word()'s array == the AND of the position bits kGroup G .. kGroup G + kGroup - 1 read the plain
//       way, for every group of the array, both of its ends included (positions behind the bitmap's last word read as clear)
//   (2) the in-window test: the array as the device holds it - bytes, kGroupSlack zeroed ones behind -, ONE load of 8 bytes at
//       group_load_byte(q0) through an accessor that checks every byte against array + slack and the offset against group_load_max();
//       for the first and the last possible diagonal and one between, every alignment q0 mod 32, every read length 3 .. 160 and every
//       base m of the read: group_in_window() == the plain bit of group (q0 + m) / kGroup
//   (3) the mapping: for every 13-bit mask of settled entries and every t below the number of entries left, nth_unsettled() == the
//       index found by counting
// --break makes the array with an OR where the rule says AND: the program must then FAIL (1) - that the check can tell.  No GPU, no library: a stand-alone program, meant to run under sanitizers.
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -I kbo_amd/csrc tools/map_group_check.cpp -o map_group_check
//   ./map_group_check
#include "map_subst.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

namespace {

namespace ms = kbo::mapsubst;

uint64_t pack_text_units(uint64_t n) { return (n + ms::kPad + 256u) / 16u + 2u; } // == kbo::pack_text_units (kernels.hpp needs the HIP headers)

uint64_t g_bad_index = 0, g_loads = 0;

struct CheckedBits { // sub_clean: bitmap_words(n_units) words (group_word() asks no word behind them)
    const std::vector<uint32_t> *w;
    uint32_t word(uint64_t i) const
    {
        g_loads++;
        if (i < w->size()) return (*w)[(size_t)i];
        g_bad_index++;
        return 0u;
    }
};

struct GroupArray { // sub_group as the device copy holds it: 4 group_words(n_units) bytes + kGroupSlack zeroed ones
    uint64_t n_units = 0;
    std::vector<uint8_t> bytes;
    uint64_t load8(uint64_t off) const // the kernel's load: 8 bytes at any byte address
    {
        g_loads++;
        if (off > ms::group_load_max(n_units) || off + 8u > bytes.size()) {
            g_bad_index++;
            return 0u;
        }
        uint64_t v;
        std::memcpy(&v, bytes.data() + off, 8);
        return v;
    }
    bool plain(uint64_t G) const { return (G >> 3) < bytes.size() ? (bytes[(size_t)(G >> 3)] >> (G & 7u)) & 1u : false; }
};

bool plain_bit(const std::vector<uint32_t> &w, uint64_t q) { return (q >> 5) < w.size() ? (w[(size_t)(q >> 5)] >> (q & 31u)) & 1u : false; }

} // namespace

int main(int argc, char **argv)
{
    bool brk = false;
    for (int i = 1; i < argc; i++)
        if (!std::strcmp(argv[i], "--break")) brk = true;
    std::mt19937_64 rng(20260421);
    uint64_t wrong_group = 0, wrong_window = 0, wrong_nth = 0, groups = 0, windows = 0, set_groups = 0;
    const uint32_t sizes[] = {200, 201, 333, 512, 1000, 1777, 2048, 3000};
    for (uint32_t n : sizes) {
        for (uint32_t kind = 0; kind < 5u; kind++) {
            const uint64_t units = pack_text_units(n), n_bw = ms::bitmap_words(units), n_gw = ms::group_words(units);
            std::vector<uint32_t> bits((size_t)n_bw, 0u);
            const uint64_t n_pos = 32u * n_bw;
            if (kind < 3u) { // random: 90 % set, 10 % set, half
                const uint32_t pct = kind == 0u ? 90u : kind == 1u ? 10u : 50u;
                for (uint64_t q = 0; q < n_pos; q++)
                    if (rng() % 100u < pct) bits[(size_t)(q >> 5)] |= 1u << (q & 31u);
            } else { // planted runs: set (kind 3) or clear (kind 4) everywhere but in runs of 1 .. 40 positions, both ends of the bitmap too
                if (kind == 3u) std::fill(bits.begin(), bits.end(), 0xFFFFFFFFu);
                auto plant = [&](uint64_t at, uint64_t len) {
                    for (uint64_t q = at; q < at + len && q < n_pos; q++) {
                        if (kind == 3u) bits[(size_t)(q >> 5)] &= ~(1u << (q & 31u));
                        else bits[(size_t)(q >> 5)] |= 1u << (q & 31u);
                    }
                };
                for (uint32_t r = 0; r < 40u; r++) plant(rng() % n_pos, 1u + rng() % 40u);
                plant(0, 1u + rng() % 9u);
                plant(n_pos - 1u - rng() % 9u, 12u);
            }
            GroupArray ga;
            ga.n_units = units;
            ga.bytes.assign((size_t)(4u * n_gw + ms::kGroupSlack), 0u);
            for (uint64_t W = 0; W < n_gw; W++) {
                const uint32_t v = ms::group_word(CheckedBits{&bits}, W, n_bw, brk);
                std::memcpy(ga.bytes.data() + 4u * W, &v, 4); // (little-endian, as the device)
            }
            // (1)
            for (uint64_t G = 0; G < 32u * n_gw; G++) {
                bool all = true;
                for (uint32_t j = 0; j < ms::kGroup; j++) all = all && plain_bit(bits, ms::kGroup * G + j);
                groups++;
                if (ga.plain(G)) set_groups++;
                if (ga.plain(G) != all) wrong_group++;
                if (ms::group_of(ms::kGroup * G) != G || ms::group_of(ms::kGroup * G + ms::kGroup - 1u) != G) wrong_group++;
            }
            // (2)
            const uint64_t last = 16u * units - 1u; // the last position a diagonal can start at
            for (uint32_t al = 0; al < 32u; al++) {
                const uint64_t mid = (rng() % (last / 32u)) * 32u + al;
                const uint64_t q0s[3] = {al, mid <= last ? mid : al, (last - al) / 32u * 32u + al};
                for (uint64_t q0 : q0s) {
                    const uint64_t loaded = ga.load8(ms::group_load_byte((uint32_t)q0));
                    for (uint32_t len = 3; len <= 160u; len++)
                        for (uint32_t m = 0; m < len; m++) {
                            windows++;
                            if (ms::group_in_window(loaded, (uint32_t)q0, m) != ga.plain(ms::group_of(q0 + m))) wrong_window++;
                        }
                }
            }
        }
    }
    // (3)
    uint64_t maps = 0;
    for (uint32_t mask = 0; mask < (1u << 13); mask++) {
        uint32_t left = 0;
        for (uint32_t i = 0; i < 13u; i++) {
            if ((mask >> i) & 1u) continue;
            maps++;
            if (ms::nth_unsettled(mask, left) != i) wrong_nth++;
            left++;
        }
    }
    std::printf("%llu groups (%llu set), %llu in-window tests over %llu loads, %llu mappings\n", (unsigned long long)groups, (unsigned long long)set_groups,
                (unsigned long long)windows, (unsigned long long)g_loads, (unsigned long long)maps);
    std::printf(g_bad_index == 0 ? "every index in range\n" : "AN INDEX OUT OF RANGE: %llu\n", (unsigned long long)g_bad_index);
    std::printf(wrong_group == 0 ? "every group bit is the AND of its position bits\n" : "A GROUP BIT IS NOT THE AND OF ITS POSITION BITS: %llu\n",
                (unsigned long long)wrong_group);
    std::printf(wrong_window == 0 ? "the in-window test reads the position's group bit\n" : "THE IN-WINDOW TEST READS ANOTHER BIT: %llu\n",
                (unsigned long long)wrong_window);
    std::printf(wrong_nth == 0 ? "the mapping finds the t-th entry left\n" : "THE MAPPING FINDS ANOTHER ENTRY: %llu\n", (unsigned long long)wrong_nth);
    return (g_bad_index || wrong_group || wrong_window || wrong_nth || set_groups == 0) ? 1 : 0;
}
