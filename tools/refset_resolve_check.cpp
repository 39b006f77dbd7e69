// refset_resolve_check.cpp — the second pass of the device-resident variant calls (kbo_amd/csrc/refset_resolve.hpp) on the CPU over
// batches made here, through accessors that check every byte of the batch, every character of a k-mer and every word of the index
// against the sizes: an index out of range is counted and fails the run.
// Checked here:
//   index   the word of every start position against the definition (the q-mer inside a run of at least k bases of its own
//           sequence), and that the sorted list keeps the positions of a code ascending
//   depths  depth_at at every position of k-mers cut from the batch, from its reverse complement, across run boundaries, across
//           sequence boundaries and with '$' and 'N' in them, in the three modes, against brute force: the longest suffix that occurs
//           in a run of at least k bases of the sequence (in its reverse complement), searched with std::search
//   word    resolve_word for every (common suffix, query peak or none, reference peak or none) against resolve_variant
//           (variant_calling.rs:139-201) written out here with the reference's own panics
//   order   the radix passes of key_pass / key_digit over shuffled sites: sorted by (ref, seq, strand, i), a permutation; 5 000
//           sites in one pair
// No GPU, no library: a stand-alone program, meant to run under sanitizers.
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -I kbo_amd/csrc tools/refset_resolve_check.cpp -o refset_resolve_check
//   ./refset_resolve_check
#include "refset_resolve.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <tuple>
#include <vector>

namespace {

namespace rs = kbo::refresolve;

uint64_t g_bad = 0, g_reads = 0, g_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd(uint32_t n)
{
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)((g_state >> 33) % n);
}

struct CheckedSeq {
    const std::vector<uint8_t> *q;
    uint32_t byte(uint64_t p) const
    {
        g_reads++;
        if (p >= q->size()) {
            g_bad++;
            return 'N';
        }
        return (*q)[(size_t)p];
    }
};
struct CheckedKmer {
    const std::string *s;
    uint32_t byte(uint32_t t) const
    {
        g_reads++;
        if (t >= s->size()) {
            g_bad++;
            return '$';
        }
        return (uint8_t)(*s)[t];
    }
};
struct CheckedIndex {
    const std::vector<uint64_t> *w;
    uint64_t word(uint64_t x) const
    {
        g_reads++;
        if (x >= w->size()) {
            g_bad++;
            return rs::kInvalidWord;
        }
        return (*w)[(size_t)x];
    }
};

bool is_base(uint8_t c) { return c == 'A' || c == 'C' || c == 'G' || c == 'T'; }
char comp(char c) { return c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : 'A'; }

// the runs of at least k bases of one sequence, and their reverse complements
void runs_of(const std::vector<uint8_t> &q, uint64_t begin, uint64_t end, uint32_t k, std::vector<std::string> &fwd, std::vector<std::string> &rev)
{
    for (uint64_t p = begin; p < end;) {
        if (!is_base(q[p])) {
            p++;
            continue;
        }
        uint64_t e = p;
        while (e < end && is_base(q[e])) e++;
        if (e - p >= k) {
            fwd.emplace_back(q.begin() + p, q.begin() + e);
            std::string r(fwd.back().rbegin(), fwd.back().rend());
            for (char &c : r) c = comp(c);
            rev.push_back(r);
        }
        p = e;
    }
}

uint32_t brute_depth(const std::string &km, uint32_t t, uint32_t k, const std::vector<std::string> &fwd, const std::vector<std::string> &rev, uint32_t mode)
{
    for (uint32_t len = std::min(t + 1u, k); len > 0u; len--) {
        const std::string suffix = km.substr(t + 1u - len, len);
        if (!std::all_of(suffix.begin(), suffix.end(), [](char c) { return is_base((uint8_t)c); })) continue;
        auto in = [&](const std::vector<std::string> &runs) {
            for (const std::string &r : runs)
                if (r.find(suffix) != std::string::npos) return true;
            return false;
        };
        if (((mode & 1u) && in(fwd)) || ((mode & 2u) && in(rev))) return len;
    }
    return 0u;
}

uint64_t check_depths(uint32_t k, uint32_t q)
{
    // six sequences: runs of k - 1 and of k bases, 'N', lower case, a homopolymer and a dinucleotide repeat; the second and the third
    // share a stretch with the first, which must not count for them
    std::vector<uint8_t> b;
    std::vector<uint64_t> off{0};
    auto put = [&](const std::string &s) { b.insert(b.end(), s.begin(), s.end()); };
    auto random = [&](uint32_t n) {
        std::string s(n, 'A');
        for (char &c : s) c = "ACGT"[rnd(4)];
        return s;
    };
    const std::string shared = random(3u * k);
    put(random(k - 1u) + "N" + random(k) + "n" + shared + "acgt" + std::string(2u * k + 3u, 'A') + random(7) + "N");
    for (uint32_t x = 0; x < 2u * k; x++) put("AC");
    put(random(k + 2u));
    off.push_back(b.size());
    put(random(k / 2u) + shared.substr(k, k) + random(k));
    off.push_back(b.size());
    put(random(q) + "N" + random(k - 1u)); // no run of k bases: nothing of it is indexed
    off.push_back(b.size());
    put(shared + random(k));
    off.push_back(b.size());
    // homopolymers of T and of A behind sequences that hold positions without a word ('N', short runs, the last q - 1 bases): with
    // q = 12 the code of T x 12 is all ones, and a word that is no occurrence must not sort among its occurrences
    put(random(5) + "N" + std::string(2u * k + 5u, 'T') + random(k) + "N" + random(3) + "N" + std::string(k + 7u, 'T') + random(k));
    off.push_back(b.size());
    put(random(k) + "NN" + std::string(2u * k + 1u, 'A') + random(k) + "N" + std::string(k + 2u, 'A'));
    off.push_back(b.size());

    const CheckedSeq seq{&b};
    std::vector<uint64_t> ix(b.size());
    uint64_t n_valid = 0;
    for (size_t s = 0; s + 1 < off.size(); s++) {
        std::vector<std::string> fwd, rev;
        runs_of(b, off[s], off[s + 1], k, fwd, rev);
        for (uint64_t p = off[s]; p < off[s + 1]; p++) {
            const uint64_t w = ix[p] = rs::index_word(seq, off[s], off[s + 1], p, k, q);
            // the definition: the q bytes from p on lie inside one run of at least k bases of this sequence
            bool want = p + q <= off[s + 1];
            uint64_t lo = p, hi = p;
            if (want) {
                for (uint32_t m = 0; m < q; m++) want = want && is_base(b[p + m]);
                while (want && lo > off[s] && is_base(b[lo - 1])) lo--;
                while (want && hi < off[s + 1] && is_base(b[hi])) hi++;
                want = want && hi - lo >= k;
            }
            if (want != (w != rs::kInvalidWord) || (want && (uint32_t)w != p)) {
                std::printf("index word of position %llu: %016llx, expected %s\n", (unsigned long long)p, (unsigned long long)w, want ? "one" : "none");
                g_bad++;
            }
            n_valid += want;
        }
    }
    std::stable_sort(ix.begin(), ix.end(), [](uint64_t a, uint64_t c) { return (a >> 32) < (c >> 32); });
    for (size_t x = 1; x < ix.size(); x++)
        if (ix[x - 1] >= ix[x] && !(ix[x - 1] == rs::kInvalidWord && ix[x] == rs::kInvalidWord)) g_bad++; // (whole words ascend: what the bisection needs)
    const CheckedIndex index{&ix};

    uint64_t n_depths = 0;
    for (size_t s = 0; s + 1 < off.size(); s++) {
        std::vector<std::string> fwd, rev;
        runs_of(b, off[s], off[s + 1], k, fwd, rev);
        const uint64_t len = off[s + 1] - off[s];
        std::vector<std::string> kmers;
        for (uint64_t p = off[s]; p + k <= b.size(); p += 1u + rnd(5)) kmers.emplace_back(b.begin() + p, b.begin() + p + k); // (behind the sequence too)
        if (len >= k) {
            kmers.emplace_back(b.begin() + off[s], b.begin() + off[s] + k);          // at the sequence's first base
            kmers.emplace_back(b.begin() + off[s + 1] - k, b.begin() + off[s + 1]);  // at its last base
        }
        for (char c : {'A', 'T'}) { // homopolymers, alone and behind other bases: forwards and as reverse complements
            kmers.emplace_back(k, c);
            kmers.push_back(random(k / 2u) + std::string(k - k / 2u, c));
        }
        const size_t cut = kmers.size();
        for (size_t x = 0; x < cut; x += 3) { // reverse complements, '$' and 'N' in the k-mer, a k-mer of two runs' ends
            std::string r(kmers[x].rbegin(), kmers[x].rend());
            for (char &c : r) c = is_base((uint8_t)c) ? comp(c) : c;
            kmers.push_back(r);
            std::string d = kmers[x];
            d[rnd(k)] = x % 2 ? '$' : 'N';
            kmers.push_back(d);
        }
        if (fwd.size() >= 2) kmers.push_back(fwd[0].substr(fwd[0].size() - k / 2u) + fwd[1].substr(0, k - k / 2u));
        for (const std::string &km : kmers) {
            const CheckedKmer kmer{&km};
            for (uint32_t mode = 1; mode <= 3; mode++)
                for (uint32_t t = 0; t < k; t++) {
                    const uint32_t got = rs::depth_at(kmer, t, q, mode, seq, off[s], off[s + 1], index, ix.size());
                    const uint32_t exact = brute_depth(km, t, k, fwd, rev, mode), want = exact >= q ? exact : 0u;
                    if (got != want) {
                        std::printf("k %u q %u mode %u sequence %zu k-mer %s position %u: depth %u, expected %u\n", k, q, mode, s, km.c_str(), t, got, want);
                        g_bad++;
                    }
                    n_depths++;
                }
        }
    }
    if (!n_valid) g_bad++;
    return n_depths;
}

// resolve_variant (variant_calling.rs:139-201) on the three values: 0 Err(ResolveVariantErr), 1 a variant, 2 a panic
int reference_resolve(long k, long csl, bool hq, long qpeak, bool hr, long rpeak, long r[4])
{
    if (csl <= 0) return 2; // assert!(common_suffix_len > 0)
    if (!hq || !hr) return 0;
    const long sms = k - csl, query_gap = sms - qpeak - 1, ref_gap = sms - rpeak - 1;
    r[0] = r[1] = r[2] = r[3] = 0;
    if (query_gap > 0 && ref_gap > 0) {
        r[0] = qpeak + 1, r[1] = sms, r[2] = rpeak + 1, r[3] = sms;
        return 1;
    }
    const long qo = -query_gap, ro = -ref_gap;
    if (qo == ro) return 0;
    const long vlen = std::labs(qo - ro);
    if (qo > ro) {
        if (rpeak + 1 + vlen > k) return 2; // ref_kmer[..] out of range
        r[2] = rpeak + 1, r[3] = rpeak + 1 + vlen;
    } else {
        if (qpeak + 1 + vlen > k) return 2;
        r[0] = qpeak + 1, r[1] = qpeak + 1 + vlen;
    }
    return 1;
}

void check_words(uint32_t k, uint64_t counts[3])
{
    for (uint32_t csl = 0; csl <= k; csl++)
        for (uint32_t qx = 0; qx < k; qx++)
            for (uint32_t rx = 0; rx < k; rx++) {
                const bool hq = qx + 1u < k, hr = rx + 1u < k;
                const uint32_t word = rs::resolve_word(rs::site_code(csl, hq ? qx : rs::kNoPeak, hr ? rx : rs::kNoPeak), k);
                long r[4] = {0, 0, 0, 0};
                const int verdict = reference_resolve(k, csl, hq, qx, hr, rx, r);
                bool same = verdict == (word == rs::kPanic ? 2 : word == rs::kNoVariant ? 0 : 1);
                if (same && verdict == 1) {
                    const long ql = r[1] - r[0], rl = r[3] - r[2];
                    same = (long)((word >> 8) & 0xFFu) == ql && (long)(word >> 24) == rl && (ql == 0 || (long)(word & 0xFFu) == r[0]) &&
                           (rl == 0 || (long)((word >> 16) & 0xFFu) == r[2]) && r[1] <= (long)k && r[3] <= (long)k && rs::is_variant(word) &&
                           (long)rs::word_chars(word) == ql + rl;
                }
                if (!same) {
                    if (g_bad < 10) std::printf("k %u csl %u qpeak %u rpeak %u: word %08x, the reference %d\n", k, csl, qx, rx, word, verdict);
                    g_bad++;
                }
                counts[verdict]++;
            }
}

struct Site {
    uint32_t ref, seq, strand, i;
};
uint64_t check_order(uint64_t n_refs, uint64_t n_seqs, uint64_t total, size_t n, bool one_pair)
{
    std::vector<Site> sites;
    while (sites.size() < n) {
        Site s{one_pair ? (uint32_t)(n_refs - 1) : rnd((uint32_t)n_refs), one_pair ? (uint32_t)(n_seqs - 1) : rnd((uint32_t)n_seqs),
               one_pair ? 2u : 1u + rnd(2), rnd((uint32_t)total)};
        sites.push_back(s);
    }
    std::sort(sites.begin(), sites.end(), [](const Site &a, const Site &b) { return std::tie(a.ref, a.seq, a.strand, a.i) < std::tie(b.ref, b.seq, b.strand, b.i); });
    sites.erase(std::unique(sites.begin(), sites.end(), [](const Site &a, const Site &b) { return std::tie(a.ref, a.seq, a.strand, a.i) == std::tie(b.ref, b.seq, b.strand, b.i); }),
                sites.end()); // (a pair has one site at a position)
    for (size_t x = sites.size(); x > 1; x--) std::swap(sites[x - 1], sites[rnd((uint32_t)x)]);
    const rs::KeyShape shape = rs::key_shape(n_refs, n_seqs, total);
    const size_t m = sites.size();
    std::vector<uint64_t> hi(m), lo(m), hi2(m), lo2(m);
    for (size_t x = 0; x < m; x++) {
        hi[x] = rs::key_hi(shape, sites[x].ref, sites[x].seq, sites[x].strand);
        lo[x] = rs::key_lo(sites[x].i, (uint32_t)x);
    }
    for (uint32_t p = 0; p < rs::key_passes(shape); p++) {
        uint32_t a = 0, nb = 0;
        rs::key_pass(shape, p, a, nb);
        if (nb < 1u || nb > 8u || a + nb > 128u || (a < 64u && a + nb > 64u)) g_bad++;
        std::vector<size_t> first(257, 0);
        for (size_t x = 0; x < m; x++) first[rs::key_digit(hi[x], lo[x], a, nb) + 1u]++;
        for (size_t d = 0; d < 256; d++) first[d + 1] += first[d];
        for (size_t x = 0; x < m; x++) {
            const size_t to = first[rs::key_digit(hi[x], lo[x], a, nb)]++;
            hi2[to] = hi[x];
            lo2[to] = lo[x];
        }
        hi.swap(hi2);
        lo.swap(lo2);
    }
    std::vector<uint8_t> hit(m, 0);
    for (size_t p = 0; p < m; p++) {
        const uint32_t x = (uint32_t)lo[p];
        if (x >= m || hit[x]) {
            g_bad++;
            continue;
        }
        hit[x] = 1;
        if (p > 0) {
            const Site &a = sites[(uint32_t)lo[p - 1]], &b = sites[x];
            if (!(std::tie(a.ref, a.seq, a.strand, a.i) < std::tie(b.ref, b.seq, b.strand, b.i))) g_bad++;
        }
        if (hi[p] == ~0ull && lo[p] == ~0ull) g_bad++; // (what an unused slot of the device's list holds sorts behind every site)
    }
    return m;
}

} // namespace

int main()
{
    uint64_t depths = 0;
    for (uint32_t k : {5u, 9u, 31u})
        for (uint32_t q : {3u, 5u, 12u})
            if (q <= k) depths += check_depths(k, q);
    std::printf("%llu depths agree with the definition\n", (unsigned long long)depths);
    for (uint32_t k : {5u, 31u, 64u, 96u, 255u}) {
        uint64_t counts[3] = {0, 0, 0};
        check_words(k, counts);
        std::printf("k %u: %llu resolve words agree with the reference: %llu variants, %llu without one, %llu panics\n", k,
                    (unsigned long long)(counts[0] + counts[1] + counts[2]), (unsigned long long)counts[1], (unsigned long long)counts[0],
                    (unsigned long long)counts[2]);
    }
    uint64_t ordered = 0;
    ordered += check_order(1, 1, 3, 3, false);
    ordered += check_order(15, 8, 100000, 3000, false);
    ordered += check_order(2000, 1, 5000000, 20000, false);
    ordered += check_order(3, 300, (1ull << 32) - 17, 10000, false);
    ordered += check_order(7, 5, 200000, 5000, true);
    std::printf("%llu sites ordered by their keys\n", (unsigned long long)ordered);
    // the query-side depths and the peaks against their definitions
    for (uint32_t k : {5u, 41u})
        for (uint32_t j = 0; j < 3u * k; j += 1u + rnd(3))
            for (uint32_t t = 0; t < k; t++) {
                const long pos = (long)j - (long)(k - 1u) + (long)t;
                const uint32_t win = rnd(k + 1u), want = pos < 0 ? 0u : (uint32_t)std::min<long>(std::min<long>(win, t + 1), pos + 1);
                if (rs::query_depth(pos < 0 ? 0xFFu : win, t, j, k) != want || rs::in_front(t, j, k) != (pos < 0)) g_bad++;
            }
    for (uint32_t round = 0; round < 2000; round++) {
        const uint32_t k = 2u + rnd(40), thr = 1u + rnd(k);
        std::vector<uint32_t> d(k);
        for (uint32_t &v : d) v = rnd(k + 1u);
        uint32_t want = rs::kNoPeak;
        for (uint32_t i = 0; i + 1u < k; i++)
            if (d[i] >= thr && d[i] > d[i + 1u]) want = i;
        if (rs::rightmost_peak([&](uint32_t i) { return i < k ? d[i] : (g_bad++, 0u); }, k, thr) != want) g_bad++;
    }
    std::printf("%llu reads through the accessors, %llu out of range or wrong\n", (unsigned long long)g_reads, (unsigned long long)g_bad);
    if (g_bad) return 1;
    std::printf("every index in range\n");
    return 0;
}
