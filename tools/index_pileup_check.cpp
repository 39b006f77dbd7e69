// index_pileup_check.cpp — kbo_amd/csrc/index_pileup.hpp through accessors that check every index, against brute force of its own:
// the whole call's serial form (pileup_serial: the records taken, their spans, anchors, bridged bases, projection, columns) on
// randomized records in order and on records that hold anything; the rounds of 64 windows as a wave takes them (a lane per window, the
// ballot, gap_before, round_end, the tail) against the serial form; sites_serial against the rule in 128-bit arithmetic.
// A stand-alone program: c++ -std=c++17 -fsanitize=address,undefined -I kbo_amd/csrc tools/index_pileup_check.cpp
// (tests/test_index_pileup_host.py builds and runs it, plain and under the sanitizers).  Exit status 0 and "in range" / "agree" on
// stdout: all is well.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "index_pileup.hpp"

using namespace kbo::idxpile;

static uint64_t g_checked = 0;
[[noreturn]] static void fail(const char *what, uint64_t a = 0, uint64_t b = 0)
{
    std::printf("FAILED: %s (%llu, %llu)\n", what, (unsigned long long)a, (unsigned long long)b);
    std::exit(1);
}
template <typename T> struct Vec { // every access checked
    std::vector<T> v;
    const char *name;
    T &at(uint64_t i)
    {
        g_checked++;
        if (i >= v.size()) fail(name, i, v.size());
        return v[i];
    }
    const T &at(uint64_t i) const
    {
        g_checked++;
        if (i >= v.size()) fail(name, i, v.size());
        return v[i];
    }
};

// the accessors index_pileup.hpp names
struct Segs {
    const Vec<Segment> *s;
    Segment get(uint64_t x) const { return s->at(x); }
};
struct Off {
    const Vec<uint64_t> *o;
    uint64_t off(size_t s) const { return o->at(s); }
};
struct Bytes {
    const Vec<uint8_t> *b;
    uint32_t at(uint64_t i) const { return b->at(i); }
};
struct Words {
    const Vec<uint32_t> *w;
    uint32_t at(uint64_t i) const { return w->at(i); }
};
struct Pile {
    Vec<uint32_t> *p;
    void add(uint64_t word) { p->at(word)++; }
};
struct Sites {
    Vec<Site> *s;
    void set(uint64_t x, const Site &v) { s->at(x) = v; }
};

struct Batch {
    Vec<uint8_t> seq{{}, "concat"}, ms{{}, "ms"};
    Vec<uint64_t> off{{}, "offsets"};
    Vec<Segment> segs{{}, "segs"};
    uint32_t k;
    uint64_t source_bases;
};

// ---- brute force: the header's definitions with a mark per base and 64-bit signed arithmetic
static uint64_t brute(const Batch &b, bool skip_multi, std::vector<uint32_t> &pile)
{
    uint64_t bridged = 0;
    const uint64_t n_seqs = b.off.v.size() - 1, total = b.seq.v.size();
    for (const Segment &s : b.segs.v) {
        if (s.seq >= n_seqs || s.q_first > s.q_last) continue;
        if (skip_multi && (s.flags & 12u)) continue;
        const uint64_t o = b.off.v[s.seq], e = b.off.v[s.seq + 1];
        if (o > e || e > total || o + s.q_last + b.k > e) continue;
        std::vector<bool> covered((uint64_t)s.q_last + b.k - s.q_first, false); // a mark per base of the extent
        for (uint64_t w = s.q_first; w <= s.q_last; w++)
            if (b.ms.v[o + w + b.k - 1] == b.k)
                for (uint64_t x = w; x < w + b.k; x++) covered[x - s.q_first] = true;
        for (uint64_t x = s.q_first; x < (uint64_t)s.q_last + b.k; x++) {
            if (covered[x - s.q_first]) continue;
            bridged++;
            const bool rev = s.flags & 1u;
            const int64_t j = rev ? (int64_t)s.pos_first + b.k - 1 - (int64_t)(x - s.q_first) : (int64_t)s.pos_first + (int64_t)(x - s.q_first);
            const char *acgt = "ACGT", *tgca = "TGCA";
            int col = -1;
            for (int c = 0; c < 4; c++)
                if (b.seq.v[o + x] == (uint8_t)(rev ? tgca[c] : acgt[c])) col = c;
            if (col < 0 || j < 0 || (uint64_t)j >= b.source_bases) continue;
            pile[(uint64_t)j * 4 + col]++;
        }
    }
    return bridged;
}

// ---- a record as a wave takes it: 64 lanes a round, each with its own view of the ballot
static void wave_record(const Batch &b, const Segment &s, uint64_t o, Pile &pile)
{
    const Bytes ms{&b.ms}, seq{&b.seq};
    uint64_t word, end = s.q_first;
    for (uint64_t w0 = s.q_first; w0 <= s.q_last; w0 += kRound) {
        uint64_t mask = 0;
        for (uint32_t lane = 0; lane < kRound; lane++)
            if (w0 + lane <= s.q_last && is_anchor(ms.at(anchor_byte(o, (uint32_t)(w0 + lane), b.k)), b.k)) mask |= 1ull << lane;
        for (uint32_t lane = 0; lane < kRound; lane++) {
            if (!(mask >> lane & 1ull)) continue;
            uint64_t from;
            const uint32_t to = gap_before(mask, lane, (uint32_t)w0, end, b.k, &from);
            for (uint64_t x = from; x < to; x++)
                if (pile_word(s, (uint32_t)x, seq.at(o + x), b.k, b.source_bases, &word)) pile.add(word);
        }
        end = round_end(mask, (uint32_t)w0, end, b.k);
    }
    for (uint32_t lane = 0; lane < kRound; lane++)
        for (uint64_t x = end + lane; x < (uint64_t)s.q_last + b.k; x += kRound)
            if (pile_word(s, (uint32_t)x, seq.at(o + x), b.k, b.source_bases, &word)) pile.add(word);
}

static Batch make_batch(std::mt19937_64 &rng, bool wild)
{
    Batch b;
    static const uint32_t ks[5] = {3, 5, 31, 96, 200};
    b.k = ks[rng() % 5];
    b.source_bases = 1 + rng() % 3000;
    const uint32_t n_seqs = 1 + rng() % 12;
    b.off.v.push_back(0);
    const char *alphabet = "ACGTACGTACGTNacgt";
    for (uint32_t s = 0; s < n_seqs; s++) {
        const uint64_t len = rng() % 4 == 0 ? rng() % b.k : rng() % 900;
        for (uint64_t i = 0; i < len; i++) {
            b.seq.v.push_back((uint8_t)alphabet[rng() % 17]);
            // anchors in runs, gaps of every length up to a few rounds between them
            b.ms.v.push_back(rng() % 100 < 93 && !b.ms.v.empty() ? b.ms.v.back() : (rng() % 3 ? (uint8_t)b.k : (uint8_t)(rng() % 256)));
        }
        b.off.v.push_back(b.seq.v.size());
        if (len < b.k) continue;
        // records in order: stretches of the windows that start and end with an anchor (or do not, when wild)
        uint64_t w = 0;
        const uint64_t o = b.off.v[s], windows = len - b.k + 1;
        while (w < windows && b.segs.v.size() < 4000) {
            uint64_t first = w;
            while (first < windows && b.ms.v[o + first + b.k - 1] != b.k) first++;
            if (first >= windows) break;
            uint64_t last = first + rng() % (windows - first);
            while (b.ms.v[o + last + b.k - 1] != b.k) last--;
            const uint32_t flags = (rng() % 2 ? 1u : 0u) | (rng() % 8 == 0 ? 4u : 0u) | (rng() % 8 == 0 ? 8u : 0u);
            b.segs.v.push_back(Segment{s, 1u + (uint32_t)(rng() % 2), (uint32_t)first, (uint32_t)last, (uint32_t)(rng() % (b.source_bases + 40)), 0u, flags});
            w = last + 1 + rng() % 40;
        }
    }
    if (wild)
        for (Segment &s : b.segs.v) {
            switch (rng() % 8) {
            case 0: s.seq = rng() % 2 ? 0xFFFFFFFFu : n_seqs + (uint32_t)(rng() % 2); break;
            case 1: s.seq = (uint32_t)(rng() % n_seqs); break;
            case 2: s.q_last += (uint32_t)(rng() % 300); break;
            case 3: s.q_first = (uint32_t)rng(); break;
            case 4: s.q_first -= (uint32_t)(rng() % (s.q_first + 1u)); break;
            case 5: s.pos_first = (uint32_t)rng(); break;
            case 6: s.q_last = (uint32_t)rng(); s.flags = (uint32_t)rng(); break;
            default: break;
            }
        }
    return b;
}

int main()
{
    std::mt19937_64 rng(20261021);
    uint64_t records = 0, bridged_all = 0, long_gaps = 0, sites_all = 0;
    for (int trial = 0; trial < 120; trial++) {
        const Batch b = make_batch(rng, trial % 3 == 2);
        const uint32_t n_seqs = (uint32_t)(b.off.v.size() - 1);
        const uint64_t total = b.seq.v.size();
        for (int skip = 0; skip < 2; skip++) {
            Vec<uint32_t> got{std::vector<uint32_t>(b.source_bases * 4, 0), "pile"}, wave{std::vector<uint32_t>(b.source_bases * 4, 0), "pile (wave)"};
            std::vector<uint32_t> want(b.source_bases * 4, 0);
            Pile out{&got}, wout{&wave};
            const uint64_t n = pileup_serial(Segs{&b.segs}, b.segs.v.size(), Off{&b.off}, n_seqs, total, b.k, skip != 0, b.source_bases, Bytes{&b.ms},
                                             Bytes{&b.seq}, out);
            if (n != brute(b, skip != 0, want)) fail("bridged bases", n, trial);
            if (got.v != want) fail("pile differs from brute force", trial, skip);
            for (const Segment &s : b.segs.v) {
                if (!record_taken(s, n_seqs, skip != 0)) continue;
                const uint64_t o = b.off.at(s.seq);
                if (!record_span(s, o, b.off.at((uint64_t)s.seq + 1), total, b.k)) continue;
                wave_record(b, s, o, wout);
                records++;
                uint64_t run = 0;
                for (uint64_t w = s.q_first; w <= s.q_last; w++) {
                    run = b.ms.v[o + w + b.k - 1] == b.k ? 0 : run + 1;
                    long_gaps += run == kRound + 1;
                }
            }
            if (wave.v != want) fail("the rounds differ from brute force", trial, skip);
            bridged_all += n;
            // sites over this pile and a depth that makes the thresholds bite
            Vec<uint32_t> depth{std::vector<uint32_t>(b.source_bases), "depth"};
            for (uint64_t j = 0; j < b.source_bases; j++) {
                const uint64_t sum = (uint64_t)got.v[4 * j] + got.v[4 * j + 1] + got.v[4 * j + 2] + got.v[4 * j + 3];
                depth.v[j] = (uint32_t)(sum + rng() % 3);
                if (rng() % 50 == 0) got.v[4 * j + rng() % 4] = (uint32_t)rng(), depth.v[j] = (uint32_t)rng();
            }
            Vec<uint64_t> so{{0, b.source_bases / 3, b.source_bases / 3, b.source_bases}, "src_off"};
            const Thresholds t{1u + (uint32_t)(rng() % 3), rng() % 4 ? (uint32_t)(rng() % 5) : (uint32_t)rng(), rng() % 4 ? 1u + (uint32_t)(rng() % 4) : (uint32_t)rng() | 1u};
            std::vector<Site> ws;
            for (uint64_t j = 0; j < b.source_bases; j++) {
                bool any = false;
                for (int c = 0; c < 4; c++) {
                    const unsigned __int128 l = (unsigned __int128)got.v[4 * j + c] * t.frac_den, r = (unsigned __int128)t.frac_num * depth.v[j];
                    any |= got.v[4 * j + c] >= t.min_count && l >= r;
                }
                if (!any) continue;
                const uint32_t src = j >= b.source_bases / 3 ? 2u : 0u;
                ws.push_back(Site{(uint32_t)j, src, depth.v[j], {got.v[4 * j], got.v[4 * j + 1], got.v[4 * j + 2], got.v[4 * j + 3]}, 0u});
            }
            for (uint64_t cap : {(uint64_t)ws.size(), (uint64_t)ws.size() / 2, (uint64_t)0}) {
                Vec<Site> sites{std::vector<Site>(cap), "sites"};
                Sites sout{&sites};
                const uint64_t ns = sites_serial(Words{&got}, Words{&depth}, b.source_bases, Off{&so}, 3u, t, sout, cap);
                if (ns != ws.size()) fail("sites counted", ns, ws.size());
                for (uint64_t x = 0; x < cap; x++) {
                    const Site &g = sites.v[x], &w = ws[x];
                    if (g.pos != w.pos || g.source != w.source || g.depth != w.depth || g.count[0] != w.count[0] || g.count[1] != w.count[1] ||
                        g.count[2] != w.count[2] || g.count[3] != w.count[3] || g.reserved != 0u)
                        fail("a site differs", x, trial);
                }
            }
            sites_all += ws.size();
        }
    }
    if (!records || !bridged_all || !long_gaps || !sites_all) fail("the trials hold no record, bridged base, gap beyond a round or site");
    std::printf("%llu checked accesses in range\n", (unsigned long long)g_checked);
    std::printf("%llu records, %llu bridged bases, %llu gaps beyond a round, %llu sites: the serial form, the rounds and brute force agree\n",
                (unsigned long long)records, (unsigned long long)bridged_all, (unsigned long long)long_gaps, (unsigned long long)sites_all);
    return 0;
}
