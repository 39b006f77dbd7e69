// index_place_check.cpp — kbo_amd/csrc/index_place.hpp through accessors that check every index, against a chain builder of its own:
// the whole call's serial form (place_serial: ranges, sources, chains, records, merge) on lists in order and on lists that hold
// anything; the wave's form of a step (a lane per ring slot, the maximum, the ballot, winner_slot) against chain_step; the merge's
// algebra.  A stand-alone program: c++ -std=c++17 -fsanitize=address,undefined -I kbo_amd/csrc tools/index_place_check.cpp
// (tests/test_index_place_host.py builds and runs it, plain and under the sanitizers).  Exit status 0 and "in range" / "agree" on
// stdout: all is well.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "index_place.hpp"

using namespace kbo::idxplace;

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

// the accessors index_place.hpp names
struct Segs {
    const Vec<Segment> *s;
    Segment get(uint64_t x) const { return s->at(x); }
};
struct Off {
    const Vec<uint64_t> *o;
    uint64_t off(size_t s) const { return o->at(s); }
};
struct Work {
    Vec<uint32_t> b{{}, "begin"}, e{{}, "end"}, s{{}, "src"};
    uint32_t begin(uint32_t q) const { return b.at(q); }
    uint32_t end(uint32_t q) const { return e.at(q); }
    uint32_t src(uint32_t x) const { return s.at(x); }
    void set_begin(uint32_t q, uint32_t v) { b.at(q) = v; }
    void set_end(uint32_t q, uint32_t v) { e.at(q) = v; }
    void set_src(uint32_t x, uint32_t v) { s.at(x) = v; }
};
struct Ring {
    Vec<State> st{std::vector<State>(kWindow, no_state()), "ring"};
    State get(uint32_t slot) const { return st.at(slot); }
    void set(uint32_t slot, const State &v) { st.at(slot) = v; }
};
struct Out {
    Vec<Place> *p;
    Place get(uint32_t s) const { return p->at(s); }
    void set(uint32_t s, const Place &v) { p->at(s) = v; }
};

static bool same(const Place &a, const Place &b) { return std::memcmp(&a, &b, sizeof a) == 0; }

// ---- the chain builder: the header's definitions in plain 64-bit arithmetic, one sequence's records in list order
struct Lim {
    int64_t k, max_gap, max_indel;
};
static Place brute(const std::vector<Segment> &L, const std::vector<uint64_t> &so, const Lim &lim)
{
    const size_t n = L.size();
    if (n == 0) return no_place();
    struct X {
        int64_t len, diag, src;
        bool rev, multi;
    };
    std::vector<X> x(n);
    for (size_t i = 0; i < n; i++) {
        const Segment &s = L[i];
        x[i].len = (int64_t)s.q_last - s.q_first + lim.k;
        x[i].rev = s.flags & 1u;
        x[i].multi = (s.flags & 12u) != 0;
        x[i].diag = x[i].rev ? (int64_t)s.pos_first + s.q_first : (int64_t)s.pos_first - s.q_first;
        int64_t src = 0;
        for (size_t t = 0; t + 1 < so.size(); t++)
            if (so[t] <= s.pos_first) src = (int64_t)t;
        x[i].src = src;
    }
    std::vector<int64_t> f(n), root(n), ns(n), ind(n), nm(n);
    for (size_t i = 0; i < n; i++) {
        int64_t best = -1, bj = -1, bshift = 0;
        for (size_t j = i >= kWindow ? i - kWindow : 0; j < i; j++) {
            if (x[j].rev != x[i].rev || x[j].src != x[i].src) continue;
            const int64_t g = (int64_t)L[i].q_first - L[j].q_last, shift = x[i].rev ? x[j].diag - x[i].diag : x[i].diag - x[j].diag;
            if (g > lim.max_gap || std::llabs(shift) > lim.max_indel || g + shift < 1) continue;
            const int64_t d = (int64_t)L[i].q_last - L[j].q_last, v = f[j] + (x[i].len < d ? x[i].len : d);
            if (v >= best) best = v, bj = (int64_t)j, bshift = shift;
        }
        if (bj >= 0 && best > x[i].len) {
            f[i] = best, root[i] = root[bj], ns[i] = ns[bj] + 1, ind[i] = ind[bj] + std::llabs(bshift), nm[i] = nm[bj] + x[i].multi;
        } else {
            f[i] = x[i].len, root[i] = (int64_t)i, ns[i] = 1, ind[i] = 0, nm[i] = x[i].multi;
        }
    }
    size_t e = 0;
    for (size_t i = 1; i < n; i++)
        if (f[i] > f[e]) e = i;
    const size_t r = (size_t)root[e];
    int64_t second = 0;
    for (size_t i = 0; i < n; i++)
        if (root[i] != root[e] && f[i] > second) second = f[i];
    Place p = no_place();
    p.source = (uint32_t)x[r].src;
    p.strand = (uint16_t)L[e].strand;
    p.q_start = L[r].q_first;
    p.q_end = (uint32_t)(L[e].q_last + lim.k);
    p.pos_start = x[e].rev ? L[e].pos_last : L[r].pos_first;
    p.pos_end = (uint32_t)((x[e].rev ? L[r].pos_first : L[e].pos_last) + lim.k);
    p.flags = (uint16_t)((x[e].rev ? 1u : 0u) | (p.pos_end > so[(size_t)x[r].src + 1] ? 2u : 0u));
    p.score = (uint32_t)f[e];
    p.n_segs = (uint32_t)ns[e];
    p.indel = (uint32_t)ind[e];
    p.n_multi = (uint32_t)nm[e];
    p.second = (uint32_t)second;
    return p;
}

// ---- lists: sequences of 0 .. 200 segments that wander along a few diagonals of three sources (one of them empty), both strands
static std::vector<Segment> make_list(std::mt19937_64 &rng, uint32_t n_seqs, uint32_t k, std::vector<std::vector<Segment>> &per_seq)
{
    auto pick = [&](uint64_t n) { return (uint32_t)(rng() % n); };
    std::vector<Segment> all;
    per_seq.assign(n_seqs, {});
    for (uint32_t s = 0; s < n_seqs; s++) {
        const uint32_t shape = pick(8), count = shape == 0 ? 0 : shape < 4 ? 1 + pick(6) : shape < 7 ? 60 + pick(10) : 100 + pick(100);
        uint32_t q = pick(50);
        const uint32_t lanes[3] = {5000 + pick(2000), 30000 + pick(100), 61000 + pick(5000)};
        for (uint32_t i = 0; i < count; i++) {
            const uint32_t span = pick(4) ? pick(60) : 0, rev = pick(5) == 0, lane = pick(8) ? 0 : 1 + pick(2);
            const uint32_t jitter = pick(3) ? 0 : pick(41), base = lanes[lane] + jitter + (pick(50) ? 0 : 200);
            Segment g;
            g.seq = s;
            g.strand = 1 + pick(2);
            g.q_first = q;
            g.q_last = q + span;
            g.pos_first = rev ? base + 20000 - q : base + q;
            g.pos_last = rev ? g.pos_first - span : g.pos_first + span;
            g.flags = rev | (pick(6) ? 0 : 4u) | (pick(6) ? 0 : 8u);
            all.push_back(g);
            per_seq[s].push_back(g);
            q += span + 1 + pick(k + 40);
        }
    }
    return all;
}

int main()
{
    std::mt19937_64 rng(20240607);
    const std::vector<uint64_t> so = {0, 30050, 30050, 60000, 120000};
    const Vec<uint64_t> off{so, "src_off"};
    uint64_t n_lists = 0, n_chains = 0, n_long = 0, n_steps = 0;
    for (uint32_t trial = 0; trial < 60; trial++) {
        const uint32_t k = trial % 3 == 0 ? 5 : trial % 3 == 1 ? 31 : 96, n_seqs = 1 + (uint32_t)(rng() % 12);
        const Limits lim{k, 60 + (uint32_t)(rng() % 200), (uint32_t)(rng() % 45)};
        std::vector<std::vector<Segment>> per_seq;
        Vec<Segment> segs{make_list(rng, n_seqs, k, per_seq), "segs"};
        const uint32_t n = (uint32_t)segs.v.size();
        Work w;
        w.b.v.assign(n_seqs, 7u);
        w.e.v.assign(n_seqs, 7u);
        w.s.v.assign(n, 7u);
        Ring ring;
        Vec<Place> place{std::vector<Place>(n_seqs, no_place()), "place"};
        Out out{&place};
        place_serial(Segs{&segs}, n, n_seqs, Off{&off}, (uint32_t)so.size() - 1u, lim, false, w, ring, out);
        for (uint32_t s = 0; s < n_seqs; s++) {
            const Place want = brute(per_seq[s], so, Lim{k, lim.max_gap, lim.max_indel});
            if (!same(place.v[s], want)) fail("place_serial differs from the chain builder", trial, s);
            n_chains++;
            n_long += per_seq[s].size() > kWindow;
        }
        // merged into itself in a second call with other limits: the merge of the two, either way round
        Vec<Place> twice = place;
        Out out2{&twice};
        const Limits lim2{k, lim.max_gap / 2u, lim.max_indel + 9u};
        place_serial(Segs{&segs}, n, n_seqs, Off{&off}, (uint32_t)so.size() - 1u, lim2, true, w, ring, out2);
        for (uint32_t s = 0; s < n_seqs; s++) {
            const Place other = brute(per_seq[s], so, Lim{k, lim2.max_gap, lim2.max_indel});
            if (!same(twice.v[s], merged(place.v[s], other)) || !same(twice.v[s], merged(other, place.v[s]))) fail("merge differs", trial, s);
        }
        // the wave's form of every step of every sequence: a lane per slot, the maximum, the ballot, the winner
        for (uint32_t s = 0; s < n_seqs; s++) {
            const uint32_t b = w.begin(s), e = w.end(s);
            if (!has_range(b, e, n)) continue;
            Ring r2;
            for (uint32_t i = 0; i < e - b; i++) {
                const Seg c = seg_of(segs.at(b + i), k, w.src(b + i));
                const State want = chain_step(r2, i, c, lim);
                uint32_t best = 0;
                uint64_t mask = 0;
                bool ok[kWindow];
                uint32_t v[kWindow];
                for (uint32_t lane = 0; lane < kWindow; lane++) {
                    int64_t sh;
                    const State mine = r2.get(lane);
                    ok[lane] = lane < i && precedes(mine, c, lim, &sh);
                    v[lane] = ok[lane] ? value_through(mine, c) : 0u;
                    if (v[lane] > best) best = v[lane];
                }
                for (uint32_t lane = 0; lane < kWindow; lane++)
                    if (ok[lane] && v[lane] == best) mask |= 1ull << lane;
                State got;
                if (mask && best > c.len) {
                    const State p = r2.get(winner_slot(mask, i));
                    int64_t sh = 0;
                    (void)precedes(p, c, lim, &sh);
                    got = extend(c, i, true, p, best, sh);
                } else {
                    got = extend(c, i, false, no_state(), 0u, 0);
                }
                if (std::memcmp(&got.f, &want.f, 5 * sizeof(uint32_t)) != 0 || got.q_last != want.q_last || got.diag != want.diag || got.tag != want.tag ||
                    got.src != want.src)
                    fail("the wave's step differs from chain_step", s, i);
                r2.set(slot_of(i), want);
                n_steps++;
            }
        }
        // the same list with records that hold anything: in range, whatever comes out
        Vec<Segment> wild = segs;
        for (uint32_t t = 0; t < n / 4u + 1u && n; t++) {
            Segment &g = wild.v[rng() % n];
            switch (rng() % 6) {
            case 0: g.seq = 0xFFFFFFFFu; break;
            case 1: g.seq = (uint32_t)(rng() % (n_seqs + 2u)); break;
            case 2: g.q_first = (uint32_t)rng(); break;
            case 3: g.q_last = (uint32_t)rng(); break;
            case 4: g.pos_first = (uint32_t)rng(); break;
            default: g.pos_last = (uint32_t)rng(), g.flags = (uint32_t)rng(); break;
            }
        }
        place_serial(Segs{&wild}, n, n_seqs, Off{&off}, (uint32_t)so.size() - 1u, Limits{k, (uint32_t)rng(), (uint32_t)rng()}, (trial & 1u) != 0u, w, ring, out);
        n_lists++;
    }
    if (n_long < 20) fail("too few lists beyond the window", n_long);
    // the merge: commutative and associative over records that tie in every way
    std::vector<Place> recs;
    recs.push_back(no_place());
    for (uint32_t t = 0; t < 40; t++) {
        Place p = no_place();
        p.source = (uint32_t)(rng() % 3);
        p.strand = (uint16_t)(1 + rng() % 2);
        p.score = 40 + (uint32_t)(rng() % 3);
        p.second = (uint32_t)(rng() % 45);
        p.q_start = (uint32_t)(rng() % 2);
        recs.push_back(p);
    }
    for (const Place &a : recs)
        for (const Place &b : recs) {
            if (!same(merged(a, b), merged(b, a))) fail("the merge is not commutative");
            for (const Place &c : recs)
                if (!same(merged(merged(a, b), c), merged(a, merged(b, c)))) fail("the merge is not associative");
        }
    // the work layout: parts of whole 16 bytes that do not overlap
    for (uint64_t n_seqs : {(uint64_t)1, (uint64_t)3, (uint64_t)4, (uint64_t)5, (uint64_t)1000, (uint64_t)kMaxSeqs - 1u})
        for (uint64_t cap : {(uint64_t)0, (uint64_t)1, (uint64_t)4, (uint64_t)77, (uint64_t)kMaxSegs}) {
            const PlaceWork pw = place_work(n_seqs, cap);
            if (pw.end_off < 4u * n_seqs || pw.list_off - pw.end_off < 4u * n_seqs || pw.count_off - pw.list_off < 4u * n_seqs || pw.src_off - pw.count_off != 16u ||
                pw.bytes - pw.src_off < 4u * cap || (pw.end_off | pw.list_off | pw.count_off | pw.src_off | pw.bytes) % 16u)
                fail("the work layout", n_seqs, cap);
        }
    std::printf("%llu lists, %llu sequences (%llu beyond the window), %llu steps in the wave's form, %llu accesses: all in range\n", (unsigned long long)n_lists,
                (unsigned long long)n_chains, (unsigned long long)n_long, (unsigned long long)n_steps, (unsigned long long)g_checked);
    std::printf("place_serial, the chain builder, the wave's step and the merge agree\n");
    return 0;
}
