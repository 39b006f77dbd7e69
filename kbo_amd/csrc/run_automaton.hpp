// run_automaton.hpp — the reference-side walk of a call site without the index the reference builds of the sequence: what
// call_batch.cpp (kbo_call_batch) and refset_calls.cpp (kbo_call_refset) answer variant_calling.rs:280 with.  Host code only.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "host_util.hpp"

namespace kbo_host {

// ---- the reference-side walk of a site (variant_calling.rs:280: the matched row's k-mer against the index of the sequence
// itself, which the reference builds per call, lib.rs:553) without building that index.
// What resolve_variant reads of that walk are the depths only, and the depth at position t is the length of the longest
// suffix of kmer[0 ..= t] (at most k) that is a suffix of some row of the sequence's SBWT.  The ACGT suffixes of that index's
// rows are exactly the substrings (of at most k characters) of the sequence's ACGT-runs of at least k characters: a row is
// a k-mer of such a run or a $-padded prefix of one, and every substring of a run ends some k-mer or padded prefix of it
// (shorter runs contribute no rows; index.rs:73-94 / SURVEY.md section 8(a) A0).  With add_revcomp the reverse complements
// of those runs count as well.  So the depths are plain matching statistics of the k-mer against those runs: a suffix
// automaton of the runs (linear in the sequence, a few hundred KB for a 10 kbp read) answers them in k steps per site,
// where building, uploading and walking a one-sequence SBWT cost 2.8 ms of host time per sequence.
// tests: kbo_call_batch == the oracle's literal kbo::call (which builds that index) per sequence, and the reference's goldens.
class RunAutomaton {
public:
    void build(const uint8_t *seq, size_t len, uint32_t k, bool add_revcomp)
    {
        // (state numbers are 32-bit, two states per character and strand: 96 bytes per base with reverse complements - a
        // sequence this long is a genome, and kbo_call with it as ref_seq walks a real index of it: refine.cpp)
        KBO_REQUIRE((add_revcomp ? 2 : 1) * (uint64_t)len < (1ull << 29), KBO_E_UNSUPPORTED,
                    "kbo_call_batch: a sequence of 2^29 bases or more (2^28 with add_revcomp); call kbo_call for it");
        st_.clear();
        st_.reserve(2 * (add_revcomp ? 2 * len : len) + 2); // (at most two states per character)
        new_state(0, -1);
        size_t run = 0;
        for (size_t i = 0; i <= len; i++) {
            const int c = i < len ? code(seq[i]) : -1;
            if (c >= 0) { run++; continue; }
            if (run >= k) {
                last_ = 0;
                for (size_t t = i - run; t < i; t++) extend(code(seq[t]));
                if (add_revcomp) {
                    last_ = 0;
                    for (size_t t = i; t-- > i - run;) extend(3 - code(seq[t]));
                }
            }
            run = 0;
        }
    }
    // depths of the walk of `kmer` (k characters, '$' and other non-ACGT bytes reset it) -> out[0 .. k)
    void depths(const uint8_t *kmer, uint32_t k, uint32_t *out) const
    {
        int32_t v = 0;
        uint32_t l = 0;
        for (uint32_t t = 0; t < k; t++) {
            const int c = code(kmer[t]);
            if (c < 0) { v = 0; l = 0; out[t] = 0; continue; }
            while (v != 0 && st_[v].next[c] < 0) { v = st_[v].link; l = (uint32_t)st_[v].len; }
            if (st_[v].next[c] >= 0) { v = st_[v].next[c]; l++; }
            else { v = 0; l = 0; }
            out[t] = l < k ? l : k;
        }
    }

private:
    struct State { // 24 bytes: a state's transitions, suffix link and length share a cache line
        int32_t next[4], link, len;
    };
    static int code(uint8_t ch) { return ch == 'A' ? 0 : ch == 'C' ? 1 : ch == 'G' ? 2 : ch == 'T' ? 3 : -1; }
    int32_t new_state(int32_t length, int32_t link)
    {
        st_.push_back(State{{-1, -1, -1, -1}, link, length});
        return (int32_t)st_.size() - 1;
    }
    int32_t clone_of(int32_t q, int32_t length)
    {
        State c = st_[q];
        c.len = length;
        st_.push_back(c);
        return (int32_t)st_.size() - 1;
    }
    void extend(int c) // (generalised: `last_` may be the root again at the start of every run)
    {
        int32_t p = last_;
        if (st_[p].next[c] >= 0) {
            const int32_t q = st_[p].next[c];
            if (st_[p].len + 1 == st_[q].len) { last_ = q; return; }
            const int32_t cl = clone_of(q, st_[p].len + 1);
            while (p >= 0 && st_[p].next[c] == q) { st_[p].next[c] = cl; p = st_[p].link; }
            st_[q].link = cl;
            last_ = cl;
            return;
        }
        const int32_t cur = new_state(st_[p].len + 1, 0);
        while (p >= 0 && st_[p].next[c] < 0) { st_[p].next[c] = cur; p = st_[p].link; }
        if (p >= 0) {
            const int32_t q = st_[p].next[c];
            if (st_[p].len + 1 == st_[q].len) st_[cur].link = q;
            else {
                const int32_t cl = clone_of(q, st_[p].len + 1);
                while (p >= 0 && st_[p].next[c] == q) { st_[p].next[c] = cl; p = st_[p].link; }
                st_[q].link = cl;
                st_[cur].link = cl;
            }
        }
        last_ = cur;
    }
    std::vector<State> st_;
    int32_t last_ = 0;
};

} // namespace kbo_host
