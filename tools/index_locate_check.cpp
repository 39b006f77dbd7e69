// index_locate_check.cpp — kbo_amd/csrc/index_locate.hpp through accessors that check every index, against brute force of its own:
// the table's serial form (mark_serial / entry_from_minmax), the segments' serial form (segments_serial), the tile-and-halo decision as
// the kernels run it (tile_span, seq_of and the max-scan of the sequence marks, the anchor bits, decide) and the three-pass scan.
// A stand-alone program: c++ -std=c++17 -fsanitize=address,undefined -I kbo_amd/csrc tools/index_locate_check.cpp
// (tests/test_index_locate_host.py builds and runs it).  Exit status 0 and "in range" / "agree" on stdout: all is well.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <vector>

#include "index_locate.hpp"

using namespace kbo::idxlocate;

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

struct Batch {
    Vec<uint8_t> d{{}, "d"};
    Vec<uint32_t> lo{{}, "lo"};
    Vec<uint64_t> off{{}, "off"};
    // the accessors index_locate.hpp names
    struct In {
        const Batch *b;
        uint32_t d(uint64_t i) const { return b->d.at(i); }
        uint32_t lo(uint64_t i) const { return b->lo.at(i); }
        uint64_t off(size_t s) const { return b->off.at(s); }
    };
    In in() const { return In{this}; }
    size_t n_seqs() const { return off.v.size() - 1; }
    uint64_t total() const { return off.v.back(); }
};
struct Tab {
    Vec<uint32_t> *e;
    uint32_t get(uint32_t r) const { return e->at(r); }
    void set(uint32_t r, uint32_t x) { e->at(r) = x; }
};

struct Rec {
    uint32_t w[7];
    bool operator==(const Rec &o) const
    {
        for (int i = 0; i < 7; i++)
            if (w[i] != o.w[i]) return false;
        return true;
    }
};

// ---- brute force: the anchors of every sequence listed, then chained by the rule in plain 64-bit arithmetic
static std::vector<Rec> brute(const Batch &b, const std::vector<uint32_t> &entries, uint32_t k, uint32_t bridge, uint32_t strand,
                              std::vector<int64_t> &delta)
{
    std::vector<Rec> out;
    for (size_t s = 0; s + 1 < b.off.v.size(); s++) {
        struct A {
            int64_t q, p;
            bool rev, multi;
        };
        std::vector<A> as;
        for (uint64_t i = b.off.v[s]; i < b.off.v[s + 1]; i++)
            if (b.d.v[i] == k && i - b.off.v[s] + 1 >= k && b.lo.v[i] < entries.size()) {
                const uint32_t e = entries[b.lo.v[i]];
                as.push_back(A{(int64_t)(i - b.off.v[s]) + 1 - (int64_t)k, (int64_t)(e & kPosMask), (e & kRev) != 0, (e & kMulti) != 0});
            }
        size_t first = 0;
        for (size_t x = 0; x < as.size(); x++) {
            bool last = x + 1 == as.size();
            if (!last) {
                const A &a = as[x], &c = as[x + 1];
                const bool diag = a.rev ? a.p + a.q == c.p + c.q : a.p - a.q == c.p - c.q;
                last = !(c.q - a.q <= 1 + (int64_t)bridge && a.rev == c.rev && diag);
            }
            if (!last) continue;
            const A &f = as[first], &l = as[x];
            out.push_back(Rec{{(uint32_t)s, strand, (uint32_t)f.q, (uint32_t)l.q, (uint32_t)f.p, (uint32_t)l.p,
                               (f.rev ? 1u : 0u) | (f.multi ? 4u : 0u) | (l.multi ? 8u : 0u)}});
            const int64_t from = f.rev ? l.p : f.p, to = (f.rev ? f.p : l.p) + k;
            if (from < (int64_t)delta.size()) delta[from]++;
            if (to < (int64_t)delta.size()) delta[to]--;
            first = x + 1;
        }
    }
    return out;
}

// ---- the tiles as the kernels run them, one after the other
struct TileModel {
    const Vec<uint64_t> *bits;
    const Vec<uint32_t> *sseq, *sent;
    const Batch *b;
    const Tab *tab;
    TileSpan sp;
    uint64_t word(uint32_t w) const { return bits->at(w); }
    uint32_t seq(uint32_t j) const { return sseq->at(j); }
    uint32_t entry(uint32_t j) const
    {
        if (j - sp.head < sp.n_tile) return sent->at(j - sp.head);
        return tab->get(b->lo.at((uint64_t)sp.ext_lo + j));
    }
};
struct Boundary {
    uint32_t seq, q, e;
};
static void tiles(const Batch &b, const Tab &tab, uint32_t n_rows, uint32_t k, uint32_t bridge, std::vector<Boundary> &starts,
                  std::vector<Boundary> &ends)
{
    const Batch::In in = b.in();
    const uint64_t total = b.total();
    for (uint32_t tile = 0; tile < n_tiles(total); tile++) {
        const TileSpan sp = tile_span(tile, total);
        if (sp.n_ext > kExt || sp.head + sp.n_tile > sp.n_ext || sp.n_tile > kTile) fail("tile span", tile);
        Vec<uint32_t> sseq{std::vector<uint32_t>(sp.n_ext, 0), "sseq"}, sent{std::vector<uint32_t>(sp.n_tile, 0), "sent"};
        Vec<uint64_t> bits{std::vector<uint64_t>((sp.n_ext + 63) / 64, 0), "bits"};
        const uint32_t s0 = seq_of(in, (uint32_t)b.n_seqs(), sp.ext_lo);
        const uint64_t ext_hi = (uint64_t)sp.ext_lo + sp.n_ext;
        for (uint64_t s = (uint64_t)s0 + 1; s < b.n_seqs(); s++) {
            const uint64_t o = in.off(s);
            if (o >= ext_hi) break;
            if (o > sp.ext_lo && in.off(s + 1) > o) sseq.at(o - sp.ext_lo) = seq_mark((uint32_t)s);
        }
        uint32_t run = seq_mark(s0);
        for (uint32_t j = 0; j < sp.n_ext; j++) {
            run = sseq.at(j) > run ? sseq.at(j) : run;
            sseq.at(j) = run;
        }
        for (uint32_t j = 0; j < sp.n_ext; j++) {
            const uint64_t g = (uint64_t)sp.ext_lo + j;
            if (in.d(g) != k || !is_anchor(k, k, g, in.off(sseq.at(j) - 1u))) continue;
            const uint32_t row = in.lo(g);
            if (row >= n_rows) continue;
            bits.at(j >> 6) |= 1ull << (j & 63u);
            if (j - sp.head < sp.n_tile) sent.at(j - sp.head) = tab.get(row);
        }
        const TileModel tm{&bits, &sseq, &sent, &b, &tab, sp};
        for (uint32_t x = 0; x < sp.n_tile; x++) {
            const uint32_t j = sp.head + x;
            if (!(bits.at(j >> 6) >> (j & 63u) & 1ull)) continue;
            const uint32_t e = sent.at(x), f = decide(tm, j, sp.n_ext, bridge, e), s = sseq.at(j) - 1u;
            const Boundary at{s, (uint32_t)((uint64_t)sp.ext_lo + j - in.off(s)) + 1u - k, e};
            if (f & kStarts) starts.push_back(at);
            if (f & kEnds) ends.push_back(at);
        }
    }
}

static void compare(const char *what, const Batch &b, Vec<uint32_t> &entries, uint32_t k, uint32_t bridge, uint64_t n_delta)
{
    const Tab tab{&entries};
    const uint32_t n_rows = (uint32_t)entries.v.size();
    std::vector<int64_t> bd(n_delta, 0);
    const std::vector<Rec> want = brute(b, entries.v, k, bridge, 2, bd);
    // the serial form, with a capacity below the count as well
    for (uint64_t cap : {(uint64_t)want.size() + 3, (uint64_t)(want.size() / 2)}) {
        std::vector<Segment> segs(cap);
        std::vector<uint32_t> delta(n_delta, 0);
        const uint64_t n = segments_serial(b.in(), tab, n_rows, k, b.n_seqs(), bridge, 2u, segs.data(), cap, delta.data(), n_delta);
        if (n != want.size()) fail(what, n, want.size());
        for (uint64_t x = 0; x < n && x < cap; x++) {
            const Segment &g = segs[x];
            if (!(Rec{{g.seq, g.strand, g.q_first, g.q_last, g.pos_first, g.pos_last, g.flags}} == want[x])) fail("serial record", x, bridge);
        }
        for (uint64_t x = 0; x < n_delta; x++)
            if (delta[x] != (uint32_t)bd[x]) fail("serial delta", x, bridge);
    }
    // the tiles
    std::vector<Boundary> starts, ends;
    tiles(b, tab, n_rows, k, bridge, starts, ends);
    if (starts.size() != want.size() || ends.size() != want.size()) fail("tile counts", starts.size(), want.size());
    for (size_t x = 0; x < want.size(); x++) {
        const Boundary &s = starts[x], &e = ends[x];
        const Rec got{{s.seq, 2u, s.q, e.q, s.e & kPosMask, e.e & kPosMask, start_flags(s.e) | end_flags(e.e)}};
        if (s.seq != e.seq || !(got == want[x])) fail("tile record", x, bridge);
    }
}

// every position of one long sequence an anchor on one diagonal, then gaps and breaks put where the tiles' edges are
static void edges(std::mt19937_64 &rng)
{
    const uint32_t k = 31;
    const uint64_t len = 3 * kTile + 777;
    for (uint32_t bridge : {0u, 1u, 31u, 254u, 255u}) {
        Batch b;
        b.off.v = {0, 0, len, len, len + 40, len + 40 + 30};
        b.d.v.assign(b.total(), (uint8_t)k);
        b.lo.v.resize(b.total());
        Vec<uint32_t> entries{std::vector<uint32_t>(b.total() + 7, kPosNone), "entries"};
        for (uint64_t i = 0; i < b.total(); i++) {
            b.lo.v[i] = (uint32_t)i;
            entries.v[i] = i < 2 * kTile ? entry_of(1000u + (uint32_t)i, false) : entry_of(900000u - (uint32_t)i, true) | (i % 5 == 0 ? kMulti : 0u);
        }
        // gaps that end exactly at a tile's first position: of 1 + bridge (joined) and 2 + bridge (not), and the same in front of a halo's edge
        auto gap = [&](uint64_t last_anchor, uint64_t next_anchor) {
            for (uint64_t i = last_anchor + 1; i < next_anchor; i++) b.d.v[i] = (uint8_t)(k - 1);
        };
        gap(kTile - (1 + bridge), kTile);
        gap(2 * kTile - (2 + bridge), 2 * kTile);                        // (also where FWD turns into REV)
        gap(3 * kTile - kHalo - (1 + bridge), 3 * kTile - kHalo);
        gap(kTile + kHalo - 1, kTile + kHalo + bridge);                  // the successor exactly 1 + bridge behind the tile's last-but-halo anchor
        gap(3 * kTile + 5, 3 * kTile + 5 + 2 + bridge);
        entries.v[kTile + 700] = entry_of(5u, false);                   // a lone break of the diagonal
        b.lo.v[kTile - 1] = (uint32_t)entries.v.size() + 3;             // a row beyond the table: no anchor
        (void)rng;
        compare("edges", b, entries, k, bridge, 1u << 20);
    }
}

static void random_batches(std::mt19937_64 &rng)
{
    for (int round = 0; round < 40; round++) {
        const uint32_t k = 3 + (uint32_t)(rng() % 40);
        const uint32_t bridges[5] = {0, 1, k, 255, (uint32_t)(rng() % 256)};
        const uint32_t bridge = bridges[rng() % 5];
        Batch b;
        b.off.v = {0};
        const int n_seqs = 1 + (int)(rng() % 60);
        for (int s = 0; s < n_seqs; s++) {
            const uint64_t kind = rng() % 6;
            b.off.v.push_back(b.off.v.back() + (kind == 0 ? 0 : kind == 1 ? k - 1 : kind == 2 ? 3000 + rng() % 3000 : rng() % 300));
        }
        const uint64_t total = b.total();
        if (total == 0) continue;
        const uint32_t n_rows = 500;
        Vec<uint32_t> entries{std::vector<uint32_t>(n_rows), "entries"};
        for (auto &e : entries.v) e = (uint32_t)(rng() % 4000) | (rng() % 3 == 0 ? kRev : 0u) | (rng() % 7 == 0 ? kMulti : 0u);
        b.d.v.resize(total);
        b.lo.v.resize(total);
        // stretches on one diagonal (rows whose entries were made to continue it), single anchors, and noise
        uint64_t i = 0;
        while (i < total) {
            const uint64_t n = 1 + rng() % 200, kind = rng() % 4;
            const uint32_t r0 = (uint32_t)(rng() % (n_rows - 210));
            for (uint64_t j = 0; j < n && i < total; j++, i++) {
                b.d.v[i] = (uint8_t)(kind == 0 ? rng() % (k + 1) : (rng() % 50 == 0 ? k - 1 : k));
                b.lo.v[i] = kind == 1 ? (uint32_t)(rng() % (n_rows + 20)) : r0 + (uint32_t)j;
            }
            if (kind >= 2) {
                const bool rev = kind == 3;
                for (uint64_t j = 0; j < n; j++) entries.v[r0 + j] = rev ? entry_of(3000u - (uint32_t)j, true) : entry_of(100u + (uint32_t)j, false);
            }
        }
        compare("random", b, entries, k, bridge, 4000 + 256);
    }
}

static void table(std::mt19937_64 &rng)
{
    for (int round = 0; round < 50; round++) {
        const uint32_t k = 2 + (uint32_t)(rng() % 20), n_rows = 50, len = 1 + (uint32_t)(rng() % 400), base = (uint32_t)(rng() % 1000);
        Batch b;
        b.off.v = {0, len};
        b.d.v.resize(len);
        b.lo.v.resize(len);
        for (uint32_t i = 0; i < len; i++) {
            b.d.v[i] = (uint8_t)(rng() % 3 ? k : rng() % (k + 1));
            b.lo.v[i] = (uint32_t)(rng() % (n_rows + 5));
        }
        Vec<uint32_t> serial{std::vector<uint32_t>(n_rows, kPosNone), "entries"};
        std::vector<uint32_t> mn(n_rows, kPosNone), mx(n_rows, 0);
        std::map<uint32_t, std::vector<uint32_t>> occ;
        uint64_t full = 0, want_full = 0;
        for (int rev = 0; rev < 2; rev++) {
            Tab tab{&serial};
            full += mark_serial(b.in(), base, len, k, n_rows, rev != 0, tab);
            for (uint32_t i = 0; i < len; i++)
                if (b.d.v[i] == k && i + 1 >= k && b.lo.v[i] < n_rows) {
                    const uint32_t p = rev ? base + (len - 1 - i) : base + i + 1 - k, o = p | (rev ? kRev : 0u);
                    occ[b.lo.v[i]].push_back(o);
                    mn[b.lo.v[i]] = o < mn[b.lo.v[i]] ? o : mn[b.lo.v[i]];
                    mx[b.lo.v[i]] = o > mx[b.lo.v[i]] ? o : mx[b.lo.v[i]];
                    want_full++;
                }
        }
        if (full != want_full) fail("full depths", full, want_full);
        for (uint32_t r = 0; r < n_rows; r++) {
            uint32_t want = kPosNone;
            if (occ.count(r)) {
                want = occ[r][0];
                for (uint32_t o : occ[r]) want = o < want ? o : want;
                if (occ[r].size() > 1) want |= kMulti;
            }
            if (serial.v[r] != want || entry_from_minmax(mn[r], mx[r]) != want) fail("entry", r, want);
        }
    }
}

template <typename T> static void scan(std::mt19937_64 &rng, bool inclusive)
{
    for (uint64_t n : {1ull, 2047ull, 2048ull, 2049ull, 3ull * kScanChunk, 5ull * kScanChunk + 17ull}) {
        Vec<T> in{std::vector<T>(n), "scan in"}, out{std::vector<T>(n), "scan out"}, sums{std::vector<T>(scan_chunks(n)), "scan sums"};
        for (auto &v : in.v) v = (T)(rng() % 7 == 0 ? rng() : rng() % 3);
        struct A {
            Vec<T> *v;
            T get(uint64_t i) const { return v->at(i); }
            void set(uint64_t i, T x) { v->at(i) = x; }
        };
        A ain{&in}, aout{&out}, asum{&sums};
        for (uint64_t c = 0; c < scan_chunks(n); c++) sums.at(c) = scan_chunk_sum<T>(ain, n, c);
        const T total = scan_sums<T>(asum, scan_chunks(n));
        for (uint64_t c = 0; c < scan_chunks(n); c++) scan_chunk_apply<T>(ain, aout, n, c, sums.at(c), inclusive);
        T run = 0;
        for (uint64_t i = 0; i < n; i++) {
            const T want = inclusive ? (T)(run + in.v[i]) : run;
            if (out.v[i] != want) fail("scan", i, n);
            run = (T)(run + in.v[i]);
        }
        if (total != run) fail("scan total", n);
    }
}

int main()
{
    std::mt19937_64 rng(20240611);
    table(rng);
    edges(rng);
    random_batches(rng);
    scan<uint32_t>(rng, true);
    scan<uint64_t>(rng, false);
    if (seg_work(1).bytes != 16 + 16 + 16 || depth_work(2049) != 16 || seg_work(150u << 20).counts_off != (150u << 20)) fail("work figures");
    std::printf("%llu accesses, every one in range; the serial forms, the tiles and the scan agree with brute force\n", (unsigned long long)g_checked);
    return 0;
}
