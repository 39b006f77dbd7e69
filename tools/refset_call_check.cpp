// refset_call_check.cpp — the first pass of kbo_call_refset (kbo_amd/csrc/refset_call.hpp) on the CPU over a packed form, a sequence
// and its matching statistics read from files (kbo_refset_form's and kbo_refset_ms_host's bytes), through accessors that check every
// rank block, every byte of the slab, every pair and every base against the sizes: an index out of range is counted and fails the run.
// Checked here:
//   spell   every row's k-mer by the inverse steps; walked forward again from the root, a full k-mer comes back to exactly its row and
//           the bases of a '$'-padded one to an interval that begins at it
//   scan    every byte of slabs laid out with explicit offsets - the sequence's pair behind filler pairs of 0 .. 257 bytes, sized so
//           that its first sites fall on the first and the last lane of a wave and of a workgroup of 256 in turn; pairs that were not kept and
//           whose last and first bytes would make a candidate across the pair boundary; depths made by hand for a candidate at i = 1;
//           pairs cut short behind a candidate so that the sequence end cuts the window of j - against the definition, written out
//           here pair by pair (variant_calling.rs:269-273)
//   match   the j and the row of every candidate against brute force over the spelled rows: the rows whose k-mer ends with the d[j]
//           bases that end at j, counted
// No GPU, no library: a stand-alone program, meant to run under sanitizers.
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -I kbo_amd/csrc tools/refset_call_check.cpp -o refset_call_check
//   ./refset_call_check FORM SEQUENCE MS ROWS K THRESHOLD
#include "refset_call.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace {

namespace rc = kbo::refcall;

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

uint64_t g_bad = 0, g_ranks = 0, g_bytes = 0, g_pairs = 0;

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
    const uint8_t *q;
    uint64_t len;
    uint32_t byte(uint32_t s) const
    {
        g_bytes++;
        if (s >= len) {
            g_bad++;
            return 'N';
        }
        return q[s];
    }
};
struct CheckedSlab {
    const std::vector<uint8_t> *ms_;
    const std::vector<uint64_t> *off_;
    const std::vector<uint32_t> *thr_;
    const std::vector<uint8_t> *kept_;
    uint32_t ms(uint64_t p) const
    {
        g_bytes++;
        if (p >= ms_->size()) {
            g_bad++;
            return 0;
        }
        return (*ms_)[(size_t)p];
    }
    uint64_t off(uint32_t x) const
    {
        g_pairs++;
        if (x >= off_->size()) {
            g_bad++;
            return 0;
        }
        return (*off_)[x];
    }
    uint32_t thr(uint32_t x) const
    {
        if (x >= thr_->size()) {
            g_bad++;
            return 2;
        }
        return (*thr_)[x];
    }
    bool kept(uint32_t x) const
    {
        if (x >= kept_->size()) {
            g_bad++;
            return false;
        }
        return (*kept_)[x] != 0;
    }
};
struct CheckedOut {
    std::vector<uint8_t> *w;
    void put(uint32_t t, uint32_t v)
    {
        if (t >= w->size()) {
            g_bad++;
            return;
        }
        (*w)[t] = (uint8_t)v;
    }
};

struct Pair { // one pair of a slab: its depths, whether the sequence is behind them (else: filler), kept, threshold
    std::vector<uint8_t> ms;
    bool real, kept;
    uint32_t thr;
};

} // namespace

int main(int argc, char **argv)
{
    if (argc != 7) {
        std::fprintf(stderr, "usage: %s FORM SEQUENCE MS ROWS K THRESHOLD\n", argv[0]);
        return 2;
    }
    std::vector<uint8_t> form, seq, ms;
    if (!read_file(argv[1], form) || !read_file(argv[2], seq) || !read_file(argv[3], ms)) {
        std::fprintf(stderr, "cannot read an input\n");
        return 2;
    }
    const uint64_t n = std::strtoull(argv[4], nullptr, 10);
    const uint32_t k = (uint32_t)std::strtoul(argv[5], nullptr, 10), t = (uint32_t)std::strtoul(argv[6], nullptr, 10);
    if (n == 0 || n >= (1ull << 32) - 32u || k == 0 || k > 255 || t < 2 || form.size() != units(n) * 16u || ms.size() != seq.size() || seq.size() < 4) {
        std::fprintf(stderr, "the form is not that of %llu rows, k is outside 1 .. 255, or the depths are not the sequence's\n", (unsigned long long)n);
        return 2;
    }
    form.shrink_to_fit();
    const CheckedForm x{&form, n};
    uint64_t wrong = 0;

    // ---- spell: every row, and forward again
    std::vector<std::string> rows(n);
    for (uint64_t row = 0; row < n; row++) {
        std::vector<uint8_t> km(k, 0);
        km.shrink_to_fit();
        CheckedOut out{&km};
        rc::spell_row(x, (uint32_t)n, k, (uint32_t)row, out);
        rows[row].assign(km.begin(), km.end());
        size_t dollars = 0;
        while (dollars < k && km[dollars] == '$') dollars++;
        for (size_t i = dollars; i < k; i++)
            if (km[i] != 'A' && km[i] != 'C' && km[i] != 'G' && km[i] != 'T') wrong++; // ('$' only in front)
        if ((row == 0) != (dollars == k)) wrong++;
        if (dollars == k) continue;
        const CheckedSeq s{km.data(), k};
        uint32_t l = 0, r = (uint32_t)n;
        for (size_t i = dollars; i < k; i++) {
            const uint32_t c = kbo::refstep::base_code(s.byte((uint32_t)i));
            l = kbo::refstep::rank_of(x, c, l);
            r = kbo::refstep::rank_of(x, c, r);
        }
        if (l != row || r <= l || (dollars == 0 && r - l != 1u)) wrong++;
    }
    if (wrong) {
        std::fprintf(stderr, "%llu rows do not spell a k-mer that leads back to them\n", (unsigned long long)wrong);
        return 1;
    }
    for (uint64_t row = 1; row < n; row++)
        if (!(rows[row - 1] != rows[row])) wrong++; // (distinct rows, distinct k-mers)

    // ---- the pairs: the sequence as it is, with a candidate made at i = 1, cut short behind its candidates; fillers in between
    std::vector<uint32_t> cand_at;
    for (uint32_t i = 1; i < ms.size(); i++)
        if (rc::is_candidate(ms[i - 1], ms[i], t)) cand_at.push_back(i);
    std::vector<std::vector<uint8_t>> variants{ms};
    {
        std::vector<uint8_t> v = ms;
        v[0] = (uint8_t)t; // (no walk makes this: d[0] <= 1.  The scan does not ask)
        v[1] = 0;
        variants.push_back(v);
    }
    for (size_t c = 0; c < cand_at.size() && c < 6; c++)
        for (uint32_t extra : {1u, 2u, k / 2u, k, k + 1u}) {
            const uint64_t len = (uint64_t)cand_at[c] + extra;
            if (len >= 3 && len <= ms.size()) variants.emplace_back(ms.begin(), ms.begin() + len);
        }
    uint64_t n_cands = 0, n_sites = 0, n_slabs = 0, lanes_seen[4] = {0, 0, 0, 0};
    // the first filler's bytes put a candidate of the first pair on byte 0 and on byte 255 of a workgroup's 256 in turn: the first and
    // the last lane of a wave too
    std::vector<uint32_t> fills{0u, 1u, 64u};
    for (size_t c = 0; c < cand_at.size() && c < 4; c++)
        for (uint32_t lane : {0u, 255u}) fills.push_back((lane + 256u - cand_at[c] % 256u) % 256u);
    for (uint32_t fill : fills) {
        std::vector<Pair> pairs;
        for (size_t v = 0; v < variants.size(); v++) {
            // a filler that is not kept and ends high, so that the next pair's first byte would be a candidate without the pair test
            Pair f{std::vector<uint8_t>(fill + (v % 3u), (uint8_t)k), false, v % 2u == 0u, t};
            if (!f.ms.empty() && f.kept) std::fill(f.ms.begin(), f.ms.end(), (uint8_t)0); // (a kept filler must hold no candidate of its own)
            pairs.push_back(f);
            pairs.push_back(Pair{variants[v], true, v % 5u != 4u, v % 4u == 3u ? t + 1u : t});
        }
        std::vector<uint8_t> slab, kept;
        std::vector<uint64_t> off{0};
        std::vector<uint32_t> thr;
        uint32_t min_thr = ~0u;
        for (const Pair &p : pairs) {
            slab.insert(slab.end(), p.ms.begin(), p.ms.end());
            off.push_back(slab.size());
            thr.push_back(p.thr);
            kept.push_back(p.kept);
            min_thr = std::min(min_thr, p.thr);
        }
        slab.shrink_to_fit();
        off.shrink_to_fit();
        thr.shrink_to_fit();
        kept.shrink_to_fit();
        const CheckedSlab s{&slab, &off, &thr, &kept};
        const uint32_t np = (uint32_t)pairs.size();
        // the definition, pair by pair
        std::vector<rc::Site> exp;
        std::vector<rc::Cand> exp_cands;
        for (uint32_t pi = 0; pi < np; pi++) {
            const Pair &p = pairs[pi];
            if (!p.kept) continue;
            const std::vector<uint8_t> &d = p.ms;
            for (uint32_t i = 1; i < d.size(); i++) {
                if (!(d[i] < d[i - 1] && d[i - 1] >= p.thr && d[i] < p.thr)) continue;
                exp_cands.push_back(rc::Cand{pi, i});
                if (!p.real) continue; // (fillers hold no candidate: see above)
                for (uint64_t j = i + 1u; j < std::min<uint64_t>((uint64_t)i + k + 1u, d.size()); j++) {
                    if (d[j] < p.thr || d[j] > j + 1u) continue;
                    const std::string tail(seq.begin() + (j + 1u - d[j]), seq.begin() + j + 1u);
                    uint32_t count = 0, row = 0;
                    for (uint64_t r = 0; r < n; r++)
                        if (rows[r].compare(k - d[j], d[j], tail) == 0) {
                            if (!count) row = (uint32_t)r;
                            count++;
                        }
                    if (count == 1u) {
                        exp.push_back(rc::Site{pi, i, (uint32_t)j, row});
                        break;
                    }
                }
            }
        }
        // the header's scan over every byte, and its match
        std::vector<rc::Site> got;
        std::vector<rc::Cand> got_cands;
        for (uint64_t p = 0; p < slab.size() + 2u; p++) {
            rc::Cand c{0, 0};
            if (!rc::scan_byte(s, np, slab.size(), min_thr, p, c)) continue;
            got_cands.push_back(c);
            if (c.pair >= np || !pairs[c.pair].real) continue;
            const uint64_t begin = off[c.pair], len = off[c.pair + 1u] - begin;
            const CheckedSeq q{seq.data(), len}; // (a pair cut short: the bases behind its end are not its own)
            uint32_t j = 0, row = 0;
            if (rc::match_serial(s, x, (uint32_t)n, q, begin, len, k, thr[c.pair], c.i, j, row)) {
                got.push_back(rc::Site{c.pair, c.i, j, row});
                if (p % 64u == 0u) lanes_seen[0]++;
                if (p % 64u == 63u) lanes_seen[1]++;
                if (p % 256u == 0u) lanes_seen[2]++;
                if (p % 256u == 255u) lanes_seen[3]++;
                std::vector<uint8_t> win(k, 0);
                win.shrink_to_fit();
                CheckedOut out{&win};
                rc::gather_depths(s, begin, j, k, out);
                for (uint32_t w = 0; w < k; w++) {
                    const int64_t pos = (int64_t)j - (int64_t)(k - 1u) + w;
                    if (win[w] != (pos >= 0 ? slab[(size_t)(begin + pos)] : rc::kNoDepth)) wrong++;
                }
            }
        }
        if (got_cands.size() != exp_cands.size() || got.size() != exp.size()) wrong++;
        else {
            for (size_t c = 0; c < exp_cands.size(); c++)
                if (std::memcmp(&got_cands[c], &exp_cands[c], sizeof(rc::Cand)) != 0) wrong++;
            for (size_t c = 0; c < exp.size(); c++)
                if (std::memcmp(&got[c], &exp[c], sizeof(rc::Site)) != 0) wrong++;
        }
        n_cands += got_cands.size();
        n_sites += got.size();
        n_slabs++;
    }
    if (wrong) {
        std::fprintf(stderr, "%llu slabs or windows differ from the definition\n", (unsigned long long)wrong);
        return 1;
    }
    if (g_bad) {
        std::fprintf(stderr, "%llu indexes out of range\n", (unsigned long long)g_bad);
        return 1;
    }
    std::printf("refset_call_check: %llu rows, %llu candidates and %llu sites of %llu slabs agree with the definition; lanes 0/63 of a wave %llu/%llu, "
                "0/255 of a workgroup %llu/%llu; %llu ranks, %llu bytes and %llu offsets in range\n",
                (unsigned long long)n, (unsigned long long)n_cands, (unsigned long long)n_sites, (unsigned long long)n_slabs,
                (unsigned long long)lanes_seen[0], (unsigned long long)lanes_seen[1], (unsigned long long)lanes_seen[2], (unsigned long long)lanes_seen[3],
                (unsigned long long)g_ranks, (unsigned long long)g_bytes, (unsigned long long)g_pairs);
    return 0;
}
