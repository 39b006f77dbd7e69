// index_indel_check.cpp — kbo_amd/csrc/index_indel.hpp through accessors that check every index, against brute force of its own:
// the whole call's serial form (events_serial: the pair rule, the intervals, the left-aligned pos, the bounds, an insertion's bytes and
// their code) on randomized records built around junctions and on records that hold anything, with capacities below the count; the
// code unpacked again (code_base) against the inserted string; event_key's rule and key_less's order against tuples; the grouping
// (sites_sorted_serial behind a sort of a shuffled list) against a map.
// A stand-alone program: c++ -std=c++17 -fsanitize=address,undefined -I kbo_amd/csrc tools/index_indel_check.cpp
// (tests/test_index_indel_host.py builds and runs it, plain and under the sanitizers).  Exit status 0 and "in range" / "agree" on
// stdout: all is well.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>
#include <string>
#include <tuple>
#include <vector>

#include "index_indel.hpp"

using namespace kbo::idxindel;

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

// the accessors index_indel.hpp names
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
struct Events {
    Vec<Event> *e;
    void set(uint64_t x, const Event &v) { e->at(x) = v; }
};
struct Sites {
    Vec<Site> *s;
    void set(uint64_t x, const Site &v) { s->at(x) = v; }
};
struct Keys {
    const Vec<std::pair<uint64_t, uint64_t>> *k;
    uint64_t w0(uint64_t i) const { return k->at(i).first; }
    uint64_t w1(uint64_t i) const { return k->at(i).second; }
};

struct Batch {
    Vec<uint8_t> seq{{}, "concat"};
    Vec<uint64_t> off{{}, "offsets"}, src_off{{}, "src_off"};
    Vec<Segment> segs{{}, "segs"};
    uint32_t k;
};

static bool same(const Event &a, const Event &b) { return a.pos == b.pos && a.kind_len == b.kind_len && a.code == b.code && a.flags == b.flags; }

// ---- brute force: the definitions with half-open intervals and strings
struct Iv {
    int64_t lo, hi;
};
static uint64_t source_of(const Batch &b, int64_t x)
{
    uint64_t s = 0;
    for (uint64_t i = 0; i + 1 < b.src_off.v.size(); i++)
        if ((int64_t)b.src_off.v[i] <= x) s = i;
    return s;
}
static uint64_t brute(const Batch &b, bool skip_multi, uint32_t max_indel, std::vector<Event> &out, std::vector<std::string> &strings, uint64_t *n_complex)
{
    const uint64_t n_seqs = b.off.v.size() - 1, total = b.seq.v.size();
    const int64_t bases = (int64_t)b.src_off.v.back(), k = b.k;
    auto holds = [&](const Segment &s) {
        if (s.seq >= n_seqs || s.q_first > s.q_last || (skip_multi && (s.flags & 12u))) return false;
        const uint64_t o = b.off.v[s.seq], e = b.off.v[s.seq + 1];
        return o <= e && e <= total && (uint64_t)s.q_last + b.k <= e - o;
    };
    auto S = [&](const Segment &s) { return (s.flags & 1u) ? Iv{s.pos_last, (int64_t)s.pos_first + k} : Iv{s.pos_first, (int64_t)s.pos_last + k}; };
    for (uint64_t x = 1; x < b.segs.v.size(); x++) {
        const Segment &A = b.segs.v[x - 1], &B = b.segs.v[x];
        if (!holds(A) || !holds(B) || A.seq != B.seq || ((A.flags ^ B.flags) & 1u) || A.q_last >= B.q_first) continue;
        const bool rev = A.flags & 1u;
        const Iv up = S(rev ? A : B), low = S(rev ? B : A);
        const int64_t gq = (int64_t)B.q_first - ((int64_t)A.q_last + k), gs = up.lo - low.hi, shift = gs - gq;
        const int64_t lim = max_indel < (1u << 30) - 1u ? max_indel : (1u << 30) - 1u;
        if (shift == 0 || shift > lim || -shift > lim) continue;
        if (gq > 0 && gs > 0) {
            ++*n_complex;
            continue;
        }
        const uint64_t o = b.off.v[A.seq], len_seq = b.off.v[A.seq + 1] - o;
        Event ev{0, 0, 0, rev != (B.strand == 2u) ? 1u : 0u};
        std::string ins;
        if (shift > 0) {
            if (up.lo - shift < 0 || up.lo > bases) continue;
            ev.pos = (uint32_t)(up.lo - shift);
            ev.kind_len = (uint32_t)shift;
        } else {
            const int64_t ln = -shift;
            if (up.lo > bases) continue;
            int64_t from = rev ? (int64_t)A.q_last + k : (int64_t)B.q_first - ln;
            if (from < 0 || (uint64_t)(from + ln) > len_seq) continue;
            for (int64_t i = 0; i < ln; i++) ins += (char)b.seq.v[o + from + i];
            if (rev) {
                std::reverse(ins.begin(), ins.end());
                for (char &c : ins) c = c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : c == 'T' ? 'A' : 'N';
            }
            if (ins.find_first_not_of("ACGT") != std::string::npos) continue;
            ev.pos = (uint32_t)up.lo;
            ev.kind_len = (uint32_t)ln | (1u << 31) | (ln > 16 ? 1u << 30 : 0u);
            if (ln <= 16)
                for (int64_t i = 0; i < ln; i++) ev.code |= (uint32_t)std::string("ACGT").find(ins[i]) << (2 * i);
        }
        if (source_of(b, up.lo) != source_of(b, low.hi - 1)) continue;
        out.push_back(ev);
        strings.push_back(ins);
    }
    return out.size();
}

// ---- batches
static std::mt19937_64 rng(20261021);
static uint64_t below(uint64_t n) { return n ? rng() % n : 0; }

static Batch random_batch(bool wild)
{
    Batch b;
    b.k = 3 + (uint32_t)below(38);
    const uint32_t n_src = 1 + (uint32_t)below(4);
    b.src_off.v.push_back(0);
    for (uint32_t s = 0; s < n_src; s++) b.src_off.v.push_back(b.src_off.v.back() + (below(4) ? 200 + below(600) : 0));
    const int64_t bases = (int64_t)b.src_off.v.back();
    const uint32_t n_seqs = 1 + (uint32_t)below(6);
    b.off.v.push_back(0);
    for (uint32_t s = 0; s < n_seqs; s++) {
        const uint64_t len = below(5) ? 4 * b.k + below(300) : below(b.k);
        for (uint64_t i = 0; i < len; i++) b.seq.v.push_back(below(60) ? (uint8_t)"ACGT"[below(4)] : (uint8_t)"Nacgt"[below(5)]);
        b.off.v.push_back(b.seq.v.size());
        // records around junctions: ascending windows, a shift and a query gap per junction
        const uint32_t rev = below(3) == 0, strand = 1 + (uint32_t)below(2);
        int64_t q = (int64_t)below(b.k), p = (int64_t)below((uint64_t)bases + 1);
        for (uint32_t r = 0, nr = (uint32_t)below(5); r < nr && len >= 4 * b.k; r++) {
            const int64_t run = (int64_t)below(b.k + 20), ql = q + run;
            if (ql + b.k > (int64_t)len) break;
            const int64_t pl = rev ? p - run : p + run;
            if (p < 0 || pl < 0 || p >= (1ll << 32) || pl >= (1ll << 32)) break;
            b.segs.v.push_back(Segment{s, strand, (uint32_t)q, (uint32_t)ql, (uint32_t)p, (uint32_t)pl, rev | (below(9) ? 0u : 4u << below(2))});
            const int64_t shift = below(4) ? (int64_t)below(41) - 20 : 0, gq = (int64_t)below(12) - 6;
            q = ql + b.k + gq; // the next record's q_first; its diagonal moves by `shift`
            p = rev ? pl - b.k - gq - shift : pl + b.k + gq + shift;
            if (q <= ql) q = ql + 1; // (windows ascend; the diagonal moves by whatever that leaves)
        }
    }
    if (wild)
        for (Segment &s : b.segs.v) {
            uint32_t w[7];
            std::memcpy(w, &s, sizeof w);
            if (below(3) == 0) w[below(7)] = below(2) ? (uint32_t)rng() : (uint32_t)below(2 * b.k + 2);
            if (below(20) == 0) w[0] = below(2) ? n_seqs : 0xFFFFFFFFu;
            std::memcpy(&s, w, sizeof w);
        }
    if (wild && below(3) == 0 && n_seqs > 1) b.off.v[1 + below(n_seqs - 1)] = below(2) ? b.seq.v.size() + 7 : 0; // offsets that descend or overrun
    return b;
}

int main()
{
    uint64_t n_events = 0, n_ins = 0, n_long = 0, n_complex_all = 0, n_rev = 0, n_cut = 0, n_sites = 0, n_invalid = 0;
    std::vector<Event> pool; // every event made: the lists of the second half
    for (int iter = 0; iter < 6000; iter++) {
        const Batch b = random_batch(iter % 3 == 2);
        const bool skip_multi = iter & 1;
        const uint32_t max_indel = iter % 7 == 0 ? 0xFFFFFFFFu : iter % 5 == 0 ? 1u : 1u + (uint32_t)below(24);
        std::vector<Event> want;
        std::vector<std::string> strings;
        uint64_t want_cx = 0;
        brute(b, skip_multi, max_indel, want, strings, &want_cx);
        // the list holds `base` events already; capacity below, at and above the count
        const uint64_t base = below(4), cap = below(3) == 0 ? below(base + want.size() + 1) : base + want.size() + below(3);
        Vec<Event> got{std::vector<Event>((size_t)cap, Event{7, 7, 7, 7}), "events"};
        Events out{&got};
        uint64_t cx = 0;
        const uint64_t made = events_serial(Segs{&b.segs}, b.segs.v.size(), Off{&b.off}, (uint32_t)(b.off.v.size() - 1), b.seq.v.size(), b.k, skip_multi, max_indel,
                                            b.src_off.v.back(), Off{&b.src_off}, (uint32_t)(b.src_off.v.size() - 1), Bytes{&b.seq}, out, base, cap, &cx);
        if (made != want.size() || cx != want_cx) fail("count", made, want.size());
        for (uint64_t i = 0; i < cap; i++) {
            const Event untouched{7, 7, 7, 7};
            const bool written = i >= base && i - base < want.size();
            if (!same(got.v[i], written ? want[i - base] : untouched)) fail("event", (uint64_t)iter, i);
        }
        if (cap < base + want.size()) n_cut++;
        n_complex_all += cx;
        for (size_t i = 0; i < want.size(); i++) {
            const Event &e = want[i];
            const uint32_t len = e.kind_len & kLenMask;
            n_events++;
            n_rev += e.flags;
            if (e.kind_len & kIns) n_ins++;
            if (e.kind_len & kLong) n_long++;
            // the code unpacked again
            if ((e.kind_len & kIns) && len <= kCodeLen)
                for (uint32_t j = 0; j < len; j++)
                    if (code_base(e.code, j) != (uint8_t)strings[i][j]) fail("code_base", (uint64_t)iter, j);
            uint64_t w0, w1;
            if (!event_key(e, b.src_off.v.back(), &w0, &w1)) fail("an event that events_serial wrote holds none", (uint64_t)iter, i);
            if (pool.size() < 4000) pool.push_back(e);
        }
    }
    if (!n_events || !n_ins || !n_long || !n_complex_all || !n_rev || !n_cut || n_ins == n_events) fail("a case did not occur", n_events, n_ins);

    // ---- keys: the rule, the order; sites from shuffled lists
    for (int iter = 0; iter < 300; iter++) {
        const uint64_t bases = 1 + below(1200);
        std::vector<Event> list;
        for (uint64_t i = 0, n = below(400); i < n; i++) {
            Event e = pool[below(pool.size())];
            if (below(4) == 0) e.pos = (uint32_t)below(bases + 2);
            if (below(8) == 0) {
                uint32_t w[4];
                std::memcpy(w, &e, sizeof w);
                w[below(4)] = below(2) ? (uint32_t)rng() : (uint32_t)below(20);
                std::memcpy(&e, w, sizeof w);
            }
            list.push_back(e);
        }
        Vec<uint32_t> depth{std::vector<uint32_t>((size_t)bases), "depth"};
        for (uint32_t &d : depth.v) d = (uint32_t)below(9);
        Vec<uint64_t> so{{0, below(bases + 1), bases}, "src_off"};
        if (so.v[1] > so.v[2]) fail("src_off");
        const Thresholds t{1 + (uint32_t)below(3), (uint32_t)below(3), 1 + (uint32_t)below(3)};
        // brute force: the rule as kbo_hip.h words it, a map from the tuple
        std::map<std::tuple<uint32_t, uint32_t, uint32_t>, std::pair<uint32_t, uint32_t>> groups;
        for (const Event &e : list) {
            const uint32_t len = e.kind_len & 0x3FFFFFFFu;
            const bool ins = e.kind_len >> 31, lng = (e.kind_len >> 30) & 1u;
            bool holds = e.flags <= 1u && len >= 1u && e.pos <= bases;
            if (ins) holds = holds && lng == (len > 16u) && !(lng && e.code) && !(len < 16u && (e.code >> (2u * len)));
            else holds = holds && !lng && e.code == 0u && (uint64_t)e.pos + len <= bases;
            uint64_t w0, w1;
            if (event_key(e, bases, &w0, &w1) != holds) fail("event_key", e.pos, e.kind_len);
            if (!holds) {
                n_invalid++;
                continue;
            }
            if (w0 == kPadKey) fail("a key that looks like the pad");
            auto &g = groups[std::make_tuple(e.pos, e.kind_len, e.code)];
            g.first++;
            g.second += e.flags;
        }
        std::vector<Site> want;
        for (const auto &g : groups) {
            const uint32_t pos = std::get<0>(g.first), d = depth.v[pos ? pos - 1 : 0], c = g.second.first;
            if (c >= t.min_count && (unsigned __int128)c * t.frac_den >= (unsigned __int128)t.frac_num * d)
                want.push_back(Site{pos, pos >= so.v[1] ? 1u : 0u, std::get<1>(g.first), std::get<2>(g.first), c, g.second.second, d, 0u});
        }
        // two shuffles of the list, each sorted by key_less: the same sites
        for (int round = 0; round < 2; round++) {
            std::shuffle(list.begin(), list.end(), rng);
            Vec<std::pair<uint64_t, uint64_t>> keys{{}, "keys"};
            for (const Event &e : list) {
                uint64_t w0, w1;
                if (event_key(e, bases, &w0, &w1)) keys.v.emplace_back(w0, w1);
            }
            std::sort(keys.v.begin(), keys.v.end(), [](const auto &a, const auto &b) { return key_less(a.first, a.second, b.first, b.second); });
            for (size_t i = 1; i < keys.v.size(); i++) { // the order is the tuples' order
                const auto &a = keys.v[i - 1], &b = keys.v[i];
                const auto ta = std::make_tuple((uint32_t)(a.first >> 32), (uint32_t)a.first, (uint32_t)(a.second >> 32));
                const auto tb = std::make_tuple((uint32_t)(b.first >> 32), (uint32_t)b.first, (uint32_t)(b.second >> 32));
                if (ta > tb || same_group(a.first, a.second, b.first, b.second) != (ta == tb)) fail("key order", i);
            }
            const uint64_t cap = below(3) == 0 ? below(want.size() + 1) : want.size() + below(2);
            Vec<Site> got{std::vector<Site>((size_t)cap), "sites"};
            Sites out{&got};
            const uint64_t n = sites_sorted_serial(Keys{&keys}, keys.v.size(), Words{&depth}, bases, Off{&so}, 2u, t, out, cap);
            if (n != want.size()) fail("sites", n, want.size());
            for (uint64_t i = 0; i < cap && i < n; i++) {
                const Site &a = got.v[i], &b = want[i];
                if (a.pos != b.pos || a.source != b.source || a.kind_len != b.kind_len || a.code != b.code || a.count != b.count || a.n_minus != b.n_minus ||
                    a.depth != b.depth || a.reserved != 0u)
                    fail("site", (uint64_t)iter, i);
            }
            n_sites += n;
        }
    }
    if (!n_sites || !n_invalid) fail("a case did not occur", n_sites, n_invalid);
    // the sort's passes cover the bits a key can set
    for (uint64_t bases : {0ull, 1ull, 2ull, 255ull, 256ull, (1ull << 30) - 1ull}) {
        const uint32_t first = sort_first_bit(bases);
        if (first > 32u || (first < 32u && (bases >> (32u - first)) != 0u) || (first < 32u && (bases >> (31u - first)) == 0u)) fail("sort_first_bit", bases, first);
        if (sort_passes(bases) * 8u < kSortEndBit - first || (sort_passes(bases) - 1u) * 8u >= kSortEndBit - first) fail("sort_passes", bases);
    }
    std::printf("%llu checked accesses in range\n", (unsigned long long)g_checked);
    std::printf("%llu events (%llu insertions, %llu long, %llu MINUS), %llu complex junctions, %llu lists cut by their capacity, %llu sites, %llu words that "
                "hold no event: serial forms and brute force agree\n",
                (unsigned long long)n_events, (unsigned long long)n_ins, (unsigned long long)n_long, (unsigned long long)n_rev,
                (unsigned long long)n_complex_all, (unsigned long long)n_cut, (unsigned long long)n_sites, (unsigned long long)n_invalid);
    return 0;
}
