// index_pileup.hpp — what the reads of a walked batch SAY at every source base (kbo_hip.h "Pileup"), for host and
// device alike: pileup_kernels.hip runs it a wave per record, index_pileup.cpp restates it on the CPU (kbo_pileup_from_segments_host,
// kbo_pileup_sites_host), tools/index_pileup_check.cpp runs it through accessors that check every index.
//
// Take the records of one kbo_segments_dev call, the batch as it was walked and the MS bytes of that walk.
//   a record      holds something when seq < n_seqs, q_first <= q_last and o + q_last + k <= off[seq + 1] <= total, o = off[seq]
//                 (record_span); skip_multi leaves out one with a MULTI bit at either end (record_taken).
//   anchors       a window w of [q_first, q_last] is an ANCHOR when the MS byte of its last base, ms[o + w + k - 1], is k (is_anchor).
//   bridged       a base x of [q_first, q_last + k) that no anchor's window [a, a + k) covers.  By ascending anchor with `end` = where
//                 the cover so far ends (q_first before the first anchor): the bases [end, a) are bridged, then end = a + k; behind the
//                 last anchor [end, q_last + k).  A record as kbo_segments_dev writes it starts and ends with an anchor, so only the gaps
//                 between anchors more than k apart hold any; a record that holds anything keeps to the same rule.
//   a round       64 windows, an anchor bit each: the anchor at bit l takes the gap in front of it - behind the nearest anchor below l in
//                 the word, or behind `end` as the rounds before left it (gap_before, round_end).  The serial form is the same rule one
//                 anchor after the other (pile_record_serial).
//   projection    FWD j = pos_first + (x - q_first), the base at x; REV j = pos_first + k - 1 - (x - q_first), its complement; 64 signed
//                 bits, a j outside [0, source_bases) is skipped (project, pile_code).  A, C, G, T = 0 .. 3 as kbo_pack_reads codes
//                 them; any other byte is counted in no column.
//   sites         base j is a SITE when a column holds at least min_count and count * frac_den >= frac_num * DEPTH[j] in 64 bits
//                 (is_site); its record is site_of().  Flag, scan, emit: the three-pass scan of index_locate.hpp over chunks of
//                 kScanChunk bases.
#pragma once
#include <stdint.h>

#include "index_locate.hpp"

namespace kbo {
namespace idxpile {

using idxlocate::kScanChunk;
using idxlocate::round16;
using idxlocate::scan_chunks;
using idxlocate::Segment;
using idxlocate::seq_of;

constexpr uint32_t kThreads = 256, kRound = 64, kWaves = kThreads / kRound;
constexpr uint32_t kNoColumn = 4;
constexpr uint32_t kMaxSeqs = 1u << 28;
constexpr uint64_t kMaxSegs = 0xFFFFFFFEull; // records a call looks at, as kbo_place_dev
static_assert(kRound == 64, "a wave's lanes are a round's windows");

struct Site { // == kbo_pile_site
    uint32_t pos, source, depth, count[4], reserved;
};
static_assert(sizeof(Site) == 32, "eight words");

struct Thresholds {
    uint32_t min_count, frac_num, frac_den;
};

// ---- a record
KBO_ST_FN bool record_taken(const Segment &s, uint32_t n_seqs, bool skip_multi)
{
    if (s.seq >= n_seqs || s.q_first > s.q_last) return false;
    return !(skip_multi && (s.flags & (idxlocate::kSegFirstMulti | idxlocate::kSegLastMulti)));
}
// ... of a sequence [o, seq_end) of a batch of `total` bases: every byte it names is the batch's
KBO_ST_FN bool record_span(const Segment &s, uint64_t o, uint64_t seq_end, uint64_t total, uint32_t k)
{
    return o <= seq_end && seq_end <= total && (uint64_t)s.q_last + k <= seq_end - o;
}
KBO_ST_FN bool is_anchor(uint32_t ms_byte, uint32_t k) { return ms_byte == k; }
// where window w's MS byte lies in the batch
KBO_ST_FN uint64_t anchor_byte(uint64_t o, uint32_t w, uint32_t k) { return o + w + k - 1u; }

// ---- a base
KBO_ST_FN uint32_t pile_code(uint32_t byte, bool rev)
{
    const uint32_t c = refstep::base_code(byte);
    return c > 3u ? kNoColumn : rev ? 3u - c : c;
}
KBO_ST_FN int64_t project(const Segment &s, uint32_t x, uint32_t k, bool rev)
{
    const int64_t d = (int64_t)x - (int64_t)s.q_first;
    return rev ? (int64_t)s.pos_first + (int64_t)k - 1 - d : (int64_t)s.pos_first + d;
}
// the word of the pile that base x of the record adds one to; false: none.  byte: the batch's byte at o + x
KBO_ST_FN bool pile_word(const Segment &s, uint32_t x, uint32_t byte, uint32_t k, uint64_t source_bases, uint64_t *word)
{
    const bool rev = (s.flags & idxlocate::kSegRev) != 0u;
    const uint32_t c = pile_code(byte, rev);
    const int64_t j = project(s, x, k, rev);
    if (c == kNoColumn || j < 0 || (uint64_t)j >= source_bases) return false;
    *word = (uint64_t)j * 4u + c;
    return true;
}

// ---- a round of 64 windows from w0: `mask` holds the anchors, `end` where the cover ended before the round
// the gap in front of the anchor at bit `lane`: the bases [*from, w0 + lane), empty when *from is not below
KBO_ST_FN uint32_t gap_before(uint64_t mask, uint32_t lane, uint32_t w0, uint64_t end, uint32_t k, uint64_t *from)
{
    const uint64_t below = lane ? mask & (~0ull >> (64u - lane)) : 0ull;
    *from = below ? (uint64_t)w0 + (63u - (uint32_t)__builtin_clzll(below)) + k : end;
    return w0 + lane;
}
KBO_ST_FN uint64_t round_end(uint64_t mask, uint32_t w0, uint64_t end, uint32_t k)
{
    return mask ? (uint64_t)w0 + (63u - (uint32_t)__builtin_clzll(mask)) + k : end;
}

// the serial form of one record that holds something (record_taken, record_span).  Ms, Seq: uint32_t at(uint64_t i) over the batch;
// Pile: void add(uint64_t word).  Returns the bridged bases, counted or not
template <typename Ms, typename Seq, typename Pile>
KBO_ST_FN uint64_t pile_record_serial(const Segment &s, uint64_t o, uint32_t k, uint64_t source_bases, const Ms &ms, const Seq &seq, Pile &pile)
{
    uint64_t end = s.q_first, n = 0, word;
    auto gap = [&](uint64_t from, uint64_t to) {
        for (uint64_t x = from; x < to; x++, n++)
            if (pile_word(s, (uint32_t)x, seq.at(o + x), k, source_bases, &word)) pile.add(word);
    };
    for (uint64_t w = s.q_first; w <= s.q_last; w++) {
        if (!is_anchor(ms.at(anchor_byte(o, (uint32_t)w, k)), k)) continue;
        gap(end, w);
        end = w + k;
    }
    gap(end, (uint64_t)s.q_last + k);
    return n;
}
// the whole call.  Segs: Segment get(uint64_t x); Off: uint64_t off(size_t s) with n_seqs + 1 values
template <typename Segs, typename Off, typename Ms, typename Seq, typename Pile>
KBO_ST_FN uint64_t pileup_serial(const Segs &segs, uint64_t n, const Off &off, uint32_t n_seqs, uint64_t total, uint32_t k, bool skip_multi,
                                 uint64_t source_bases, const Ms &ms, const Seq &seq, Pile &pile)
{
    uint64_t bridged = 0;
    for (uint64_t x = 0; x < n; x++) {
        const Segment s = segs.get(x);
        if (!record_taken(s, n_seqs, skip_multi)) continue;
        const uint64_t o = off.off(s.seq);
        if (!record_span(s, o, off.off((size_t)s.seq + 1u), total, k)) continue;
        bridged += pile_record_serial(s, o, k, source_bases, ms, seq, pile);
    }
    return bridged;
}

// ---- sites
KBO_ST_FN bool column_calls(uint32_t count, uint32_t depth, const Thresholds &t)
{
    return count >= t.min_count && (uint64_t)count * t.frac_den >= (uint64_t)t.frac_num * depth;
}
KBO_ST_FN bool is_site(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t depth, const Thresholds &t)
{
    return column_calls(c0, depth, t) || column_calls(c1, depth, t) || column_calls(c2, depth, t) || column_calls(c3, depth, t);
}
KBO_ST_FN Site site_of(uint32_t pos, uint32_t source, uint32_t depth, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3)
{
    return Site{pos, source, depth, {c0, c1, c2, c3}, 0u};
}
// the serial form.  PileIn: uint32_t at(uint64_t word); Depth: uint32_t at(uint64_t j); SrcOff: off(s) with n_src + 1 values;
// Out: void set(uint64_t x, Site).  Record x is written iff x < capacity; returns the full count
template <typename PileIn, typename Depth, typename SrcOff, typename Out>
KBO_ST_FN uint64_t sites_serial(const PileIn &pile, const Depth &depth, uint64_t source_bases, const SrcOff &so, uint32_t n_src, const Thresholds &t,
                                Out &out, uint64_t capacity)
{
    uint64_t n = 0;
    for (uint64_t j = 0; j < source_bases; j++) {
        const uint32_t c0 = pile.at(4u * j), c1 = pile.at(4u * j + 1u), c2 = pile.at(4u * j + 2u), c3 = pile.at(4u * j + 3u), d = depth.at(j);
        if (!is_site(c0, c1, c2, c3, d, t)) continue;
        if (n < capacity) out.set(n, site_of((uint32_t)j, seq_of(so, n_src, j), d, c0, c1, c2, c3));
        n++;
    }
    return n;
}

// ---- d_work of kbo_pileup_sites_dev: the scan's sums, 4 bytes per kScanChunk source bases rounded up to 16 (at least 16)
KBO_ST_FN uint64_t sites_work(uint64_t source_bases)
{
    const uint64_t b = round16(scan_chunks(source_bases) * 4u);
    return b < 16u ? 16u : b;
}

} // namespace idxpile
} // namespace kbo
