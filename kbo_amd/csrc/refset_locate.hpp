// refset_locate.hpp — where a run of kbo_find_refset lies on its reference (kbo_hip.h "the locus of a run"), for host
// and device alike: refset_locate_kernels.hip runs it a wave per run, refset.cpp fills the position table with its encoding,
// refset_runs.cpp restates the call on the CPU (kbo_locate_refset_host), tools/refset_locate_check.cpp runs it through accessors that check every
// index.
//
// A noisy matching statistic equals k at query position i exactly when the k-mer that ends there is a row of the reference's SBWT,
// and a row of a one-sequence index stands for positions of that sequence.  The set keeps one ENTRY per row (opt-in, made at build
// time): of the k-mer's occurrences (p, strand) - FWD: the k-mer is ref[p, p + k); REV: its reverse complement is - the one with FWD
// before REV and then the smallest p, as
//   bits 0 .. 29  p        bit 30  REV        bit 31  the k-mer has more than one occurrence (MULTI)
// and kPosNone for a row that is no full k-mer.  The row of a k-mer is found by k rank steps from the root [0, n) over the packed
// form (refset_step.hpp's rank_of), leaving at the first empty interval or at a byte that is no base; at depth k the interval is one
// row.  An ANCHOR of a run [start, end) is a window [i, i + k) inside it whose k-mer has a row; the locus is the first and the last.
// Windows are looked up kWindow at a time, from the front until one holds an anchor, then from the back: n_tested counts the
// windows handed out that way, so the serial form here and the kernel's ballots agree on it.
// Accessors: Form as refset_step.hpp's (rank), and
//   Seq   uint32_t byte(uint64_t i)      byte i of the '+' batch (i < the batch's bases)
//   Pos   uint32_t entry(uint32_t row)   the entry of a row of this reference (row < n)
#pragma once
#include <stdint.h>

#include "refset_step.hpp"

namespace kbo {
namespace reflocate {

constexpr uint32_t kPosNone = 0xFFFFFFFFu;  // == KBO_POS_NONE == KBO_LOCUS_NONE
constexpr uint32_t kMulti = 1u << 31;       // == KBO_LOCUS_MULTI
constexpr uint32_t kRev = 1u << 30;
constexpr uint32_t kPosMask = kRev - 1u;
constexpr uint64_t kMaxRefLen = 1ull << 30; // p takes 30 bits
constexpr uint32_t kWindow = 64;            // windows looked up at a time: a wave's lanes
constexpr uint32_t kFlagFirstRev = 1u, kFlagLastRev = 2u, kFlagFirstMulti = 4u, kFlagLastMulti = 8u, kFlagUnusable = 16u;

struct Locus { // == kbo_ref_locus
    uint32_t q_first, ref_first, q_last, ref_last, flags, n_tested;
};

KBO_ST_FN Locus no_locus(uint32_t flags) { return Locus{kPosNone, kPosNone, kPosNone, kPosNone, flags, 0u}; }

// the entry of one occurrence, and the entry of a row that already has `have` when `occ` is found too
KBO_ST_FN uint32_t entry_of(uint32_t p, bool rev) { return p | (rev ? kRev : 0u); }
KBO_ST_FN uint32_t entry_merge(uint32_t have, uint32_t occ)
{
    if (have == kPosNone) return occ;
    const uint32_t a = have & ~kMulti; // (FWD before REV, then the smaller p: the order of the low 31 bits)
    return (a < occ ? a : occ) | kMulti;
}

// base j of a sequence of `len` bytes at `begin` on a strand, as refstep::base_code has it (4: no base).  '-' is the reverse
// complement as kbo_revcomp_batch makes it: byte j is the complement of byte len - 1 - j, and lower case is no base
template <typename Seq> KBO_ST_FN uint32_t strand_code(const Seq &q, uint64_t begin, uint64_t len, bool rev, uint32_t j)
{
    if (!rev) return refstep::base_code(q.byte(begin + j));
    const uint32_t c = refstep::base_code(q.byte(begin + (len - 1u - j)));
    return c > 3u ? 4u : 3u - c;
}

// the row of the k-mer at [i, i + k) of the strand's sequence (i + k <= len) in a form of n rows; kPosNone: it has none
template <typename Form, typename Seq>
KBO_ST_FN uint32_t kmer_row(const Form &x, uint32_t n, uint32_t k, const Seq &q, uint64_t begin, uint64_t len, bool rev, uint32_t i)
{
    uint32_t l = 0, r = n;
    for (uint32_t t = 0; t < k; t++) {
        const uint32_t c = strand_code(q, begin, len, rev, i + t);
        if (c > 3u) return kPosNone;
        l = refstep::rank_of(x, c, l);
        r = refstep::rank_of(x, c, r);
        if (l >= r) return kPosNone;
    }
    return l;
}

// the entry of that k-mer; kPosNone: the window is no anchor
template <typename Form, typename Seq, typename Pos>
KBO_ST_FN uint32_t kmer_entry(const Form &x, uint32_t n, uint32_t k, const Seq &q, uint64_t begin, uint64_t len, bool rev, const Pos &pos, uint32_t i)
{
    const uint32_t row = kmer_row(x, n, k, q, begin, len, rev, i);
    return row == kPosNone ? kPosNone : pos.entry(row);
}

// what the batch's offsets and a record's coordinates must satisfy for the windows to lie inside the batch
KBO_ST_FN bool span_ok(uint64_t begin, uint64_t seq_end, uint64_t total, uint32_t start, uint32_t end)
{
    return begin <= seq_end && seq_end <= total && start <= end && (uint64_t)end <= seq_end - begin;
}

KBO_ST_FN void set_first(Locus &L, uint32_t i, uint32_t e)
{
    L.q_first = i;
    L.ref_first = e & kPosMask;
    L.flags |= (e & kRev ? kFlagFirstRev : 0u) | (e & kMulti ? kFlagFirstMulti : 0u);
}
KBO_ST_FN void set_last(Locus &L, uint32_t i, uint32_t e)
{
    L.q_last = i;
    L.ref_last = e & kPosMask;
    L.flags |= (e & kRev ? kFlagLastRev : 0u) | (e & kMulti ? kFlagLastMulti : 0u);
}

// the windows of one group: kWindow, or what is left of the run's window starts
KBO_ST_FN uint32_t group_lanes(uint64_t left) { return left < kWindow ? (uint32_t)left : kWindow; } // left: starts not yet handed out

// the locus of the run [start, end), start <= end, one window after the other; entry_at(i): kmer_entry of the window at i
template <typename EntryAt> KBO_ST_FN Locus locate_serial(uint32_t start, uint32_t end, uint32_t k, EntryAt &&entry_at)
{
    Locus L = no_locus(0u);
    if (end - start < k) return L;
    const uint32_t starts = end - start - k + 1u;
    bool found = false;
    for (uint64_t done = 0; done < starts && !found; done += kWindow) {
        const uint32_t lanes = group_lanes(starts - done);
        L.n_tested += lanes;
        for (uint32_t j = 0; j < lanes && !found; j++) {
            const uint32_t i = start + (uint32_t)done + j, e = entry_at(i);
            if (e != kPosNone) {
                set_first(L, i, e);
                found = true;
            }
        }
    }
    if (!found) return L;
    found = false;
    for (uint64_t done = 0; done < starts && !found; done += kWindow) { // (ends at the first anchor at the latest)
        const uint32_t lanes = group_lanes(starts - done);
        L.n_tested += lanes;
        for (uint32_t j = 0; j < lanes && !found; j++) {
            const uint32_t i = start + (starts - 1u - (uint32_t)done - j), e = entry_at(i);
            if (e != kPosNone) {
                set_last(L, i, e);
                found = true;
            }
        }
    }
    return L;
}

} // namespace reflocate
} // namespace kbo
