// index_locate.hpp — where a walked batch lies on the sequences an index was built from (kbo_hip.h "Positions, segments, depth";
// DESIGN.md 4.13), for host and device alike: locate_kernels.hip runs it a lane per base, index_locate.cpp restates it on the CPU
// (kbo_positions_from_ms_host, kbo_segments_from_ms_host), tools/index_locate_check.cpp runs it through accessors that check every index.
//
// The interval walk leaves, per base, the depth d and the interval's first row lo.  At d == k the interval is ONE row and the row's
// k-mer is the window that ends at the base, so one ENTRY per row (refset_locate.hpp's encoding: p, REV, MULTI, kPosNone) turns the
// walk into source coordinates - the coordinates of the sources concatenated without a separator.
//   the table     the sources are walked themselves, in slabs [a, b) of those coordinates (and each slab reversed and complemented
//                 as a whole, its sequence boundaries mirrored, for REV): a base i of the slab with d == k is the occurrence
//                 occ_of(a, b - a, i, k, rev) of row lo; a row keeps the smallest and the largest occurrence it was given (the order of
//                 the low 31 bits: FWD before REV, then p) and its entry is the smallest, MULTI when they differ: entry_from_minmax.
//                 The serial form gives the same by reflocate::entry_merge, one occurrence after the other.
//   anchors       base i of sequence s, off[s] <= i < off[s + 1], is an ANCHOR when d[i] == k, the window starts inside the sequence
//                 (i - off[s] + 1 >= k) and lo[i] is a row; its q is i - off[s] - (k - 1), its entry the table's word for lo[i].
//   segments      anchors a < b of one sequence with no anchor between them are JOINED when b.i - a.i <= 1 + bridge, both have the same
//                 REV bit and lie on one diagonal (joined()); a segment is a maximal chain.  An anchor STARTS one when it is not joined
//                 to its predecessor and ENDS one when it is not joined to its successor; segments are disjoint stretches of the anchor
//                 list, so the n-th start and the n-th end of the batch belong to the same record.
//   a tile        kTile positions and kHalo on each side (kHalo >= 1 + the largest bridge: what lies beyond cannot be joined): the
//                 sequence of every position by a max-scan over the marks of the sequence starts, the anchors as bits, 64 a word;
//                 decide() finds the nearest anchor on either side in those words and applies the rule.
//   the scan      three passes over chunks of kScanChunk values: each chunk's sum, the sums' exclusive scan by ONE workgroup, each
//                 chunk's own scan on top of its sum's prefix.  No pass waits for another workgroup of its own launch.
#pragma once
#include <stdint.h>

#include "refset_locate.hpp"

namespace kbo {
namespace idxlocate {

using reflocate::entry_merge;
using reflocate::entry_of;
using reflocate::kMulti;
using reflocate::kPosMask;
using reflocate::kPosNone;
using reflocate::kRev;

constexpr uint32_t kTile = 2048, kHalo = 256, kThreads = 256;
constexpr uint32_t kExt = kTile + 2u * kHalo, kPer = kExt / kThreads, kTilePer = kTile / kThreads, kWords = kExt / 64u;
constexpr uint32_t kMaxBridge = 255;
static_assert(kHalo >= 1u + kMaxBridge && kExt % (64u * (kThreads / 64u)) == 0 && kTilePer == 8u, "a wave's round is one word of anchor bits; a lane's flags are one 8-byte word");
constexpr uint64_t kMaxSourceBases = reflocate::kMaxRefLen;
constexpr uint32_t kScanChunk = 2048;                         // values a workgroup of the scan's outer passes takes
constexpr uint32_t kStarts = 1u, kEnds = 2u;                  // a position's flag byte
constexpr uint32_t kSegRev = 1u, kSegFirstMulti = 4u, kSegLastMulti = 8u;
constexpr uint32_t kNoPos = 0xFFFFFFFFu;

struct Segment { // == kbo_seq_segment
    uint32_t seq, strand, q_first, q_last, pos_first, pos_last, flags;
};

// ---- the table
// the occurrence that base i of a walked slab stands for: the slab holds the source bases [base, base + len), as they are (FWD) or
// reversed and complemented as a whole (REV)
KBO_ST_FN uint32_t occ_of(uint32_t base, uint32_t len, uint32_t i, uint32_t k, bool rev)
{
    return entry_of(rev ? base + (len - 1u - i) : base + (i + 1u - k), rev);
}
KBO_ST_FN bool full_depth(uint32_t d, uint32_t k, uint32_t i) { return d == k && i + 1u >= k; }
KBO_ST_FN uint32_t entry_from_minmax(uint32_t mn, uint32_t mx) { return mn == kPosNone ? kPosNone : mn | (mx != mn ? kMulti : 0u); }

// the serial form: every base of one strand's walk of a slab into `entries`; returns the bases with a full depth
// In: uint32_t d(uint64_t i), uint32_t lo(uint64_t i); Tab: uint32_t get(uint32_t row), void set(uint32_t row, uint32_t e)
template <typename In, typename Tab>
KBO_ST_FN uint64_t mark_serial(const In &in, uint32_t base, uint32_t len, uint32_t k, uint32_t n_rows, bool rev, Tab &tab)
{
    uint64_t n_full = 0;
    for (uint32_t i = 0; i < len; i++) {
        if (!full_depth(in.d(i), k, i)) continue;
        const uint32_t row = in.lo(i);
        if (row >= n_rows) continue;
        n_full++;
        tab.set(row, entry_merge(tab.get(row), occ_of(base, len, i, k, rev)));
    }
    return n_full;
}

// ---- segments
KBO_ST_FN bool is_anchor(uint32_t d, uint32_t k, uint64_t i, uint64_t seq_begin) { return d == k && i - seq_begin + 1u >= k; }
// anchors a before b, dist = b.q - a.q >= 1 (within reach already): one strand, one diagonal (FWD: p - q, REV: p + q)
KBO_ST_FN bool joined(uint32_t ea, uint32_t eb, uint32_t dist)
{
    if ((ea ^ eb) & kRev) return false;
    const uint32_t pa = ea & kPosMask, pb = eb & kPosMask;
    return (ea & kRev) ? pa - pb == dist : pb - pa == dist;
}
KBO_ST_FN uint32_t start_flags(uint32_t e) { return (e & kRev ? kSegRev : 0u) | (e & kMulti ? kSegFirstMulti : 0u); }
KBO_ST_FN uint32_t end_flags(uint32_t e) { return (e & kRev ? kSegRev : 0u) | (e & kMulti ? kSegLastMulti : 0u); }
// what the anchor that starts / ends a segment adds to delta, and where: FWD covers [pos_first, pos_last + k), REV [pos_last, pos_first + k)
KBO_ST_FN uint32_t delta_index(uint32_t e, uint32_t k, bool is_start) { return (e & kPosMask) + ((((e & kRev) != 0u) == is_start) ? k : 0u); }
KBO_ST_FN uint32_t delta_value(uint32_t e, bool is_start) { return (((e & kRev) != 0u) == is_start) ? 0xFFFFFFFFu : 1u; }

// the nearest set bit below / above position j of n_ext, at most `reach` away; kNoPos: none.  Bits: uint64_t word(uint32_t w)
template <typename Bits> KBO_ST_FN uint32_t prev_anchor(const Bits &b, uint32_t j, uint32_t reach)
{
    if (j == 0) return kNoPos;
    const uint32_t least = j > reach ? j - reach : 0u;
    uint32_t w = (j - 1u) >> 6;
    uint64_t m = b.word(w) & (~0ull >> (63u - ((j - 1u) & 63u)));
    for (;;) {
        if (m) {
            const uint32_t p = w * 64u + 63u - (uint32_t)__builtin_clzll(m);
            return p >= least ? p : kNoPos;
        }
        if (w * 64u <= least) return kNoPos;
        m = b.word(--w);
    }
}
template <typename Bits> KBO_ST_FN uint32_t next_anchor(const Bits &b, uint32_t j, uint32_t n_ext, uint32_t reach)
{
    if (j + 1u >= n_ext) return kNoPos;
    const uint32_t most = n_ext - 1u - j > reach ? j + reach : n_ext - 1u;
    uint32_t w = (j + 1u) >> 6;
    uint64_t m = b.word(w) & (~0ull << ((j + 1u) & 63u));
    for (;;) {
        if (m) {
            const uint32_t p = w * 64u + (uint32_t)__builtin_ctzll(m);
            return p <= most ? p : kNoPos;
        }
        if (w * 64u + 63u >= most) return kNoPos;
        m = b.word(++w);
    }
}
// kStarts | kEnds of the anchor at position j of a tile's n_ext positions, its entry e.
// Tile: word(w) as above, uint32_t seq(uint32_t j), uint32_t entry(uint32_t j) of an anchor
template <typename Tile> KBO_ST_FN uint32_t decide(const Tile &t, uint32_t j, uint32_t n_ext, uint32_t bridge, uint32_t e)
{
    uint32_t f = kStarts | kEnds;
    const uint32_t a = prev_anchor(t, j, 1u + bridge);
    if (a != kNoPos && t.seq(a) == t.seq(j) && joined(t.entry(a), e, j - a)) f &= ~kStarts;
    const uint32_t b = next_anchor(t, j, n_ext, 1u + bridge);
    if (b != kNoPos && t.seq(b) == t.seq(j) && joined(e, t.entry(b), b - j)) f &= ~kEnds;
    return f;
}
// the positions [ext_lo, ext_hi) a tile looks at, and where the tile begins among them
struct TileSpan {
    uint32_t ext_lo, n_ext, head, n_tile;
};
KBO_ST_FN TileSpan tile_span(uint32_t tile, uint64_t total)
{
    const uint64_t t0 = (uint64_t)tile * kTile, lo = t0 >= kHalo ? t0 - kHalo : 0u;
    const uint64_t hi = t0 + kTile + kHalo < total ? t0 + kTile + kHalo : total, t1 = t0 + kTile < total ? t0 + kTile : total;
    return TileSpan{(uint32_t)lo, (uint32_t)(hi - lo), (uint32_t)(t0 - lo), (uint32_t)(t1 - t0)};
}
KBO_ST_FN uint32_t n_tiles(uint64_t total) { return (uint32_t)((total + kTile - 1u) / kTile); }
// the sequence that holds position x < off(n_seqs): the last s with off(s) <= x.  Off: uint64_t off(size_t s)
template <typename Off> KBO_ST_FN uint32_t seq_of(const Off &o, uint32_t n_seqs, uint64_t x)
{
    uint32_t a = 0, b = n_seqs; // off(a) <= x (off(0) == 0), off(b) > x or b == n_seqs
    while (b - a > 1u) {
        const uint32_t m = a + (b - a) / 2u;
        if (o.off(m) <= x) a = m;
        else b = m;
    }
    return a;
}
// the mark of sequence s for the max-scan over a tile's positions: written where a sequence that is not empty starts
KBO_ST_FN uint32_t seq_mark(uint32_t s) { return s + 1u; }

// the serial form: the records of a batch, byte for byte what the kernels write.  In: d(i), lo(i), off(s); Tab: get(row).
// Records beyond `capacity` are counted and not written; delta (or null) has n_delta words.  Returns the number of segments.
template <typename In, typename Tab>
KBO_ST_FN uint64_t segments_serial(const In &in, const Tab &tab, uint32_t n_rows, uint32_t k, size_t n_seqs, uint32_t bridge, uint32_t strand,
                                   Segment *segs, uint64_t capacity, uint32_t *delta, uint64_t n_delta)
{
    uint64_t n = 0;
    auto add = [&](uint32_t e, bool is_start) {
        const uint32_t at = delta_index(e, k, is_start);
        if (delta && at < n_delta) delta[at] += delta_value(e, is_start);
    };
    for (size_t s = 0; s < n_seqs; s++) {
        const uint64_t begin = in.off(s), end = in.off(s + 1);
        bool open = false;
        uint64_t last_i = 0;
        uint32_t last_e = 0;
        auto close = [&]() {
            if (n < capacity) {
                segs[n].q_last = (uint32_t)(last_i - begin + 1u - k);
                segs[n].pos_last = last_e & kPosMask;
                segs[n].flags |= end_flags(last_e);
            }
            add(last_e, false);
            n++;
            open = false;
        };
        for (uint64_t i = begin; i < end; i++) {
            if (!is_anchor(in.d(i), k, i, begin)) continue;
            const uint32_t row = in.lo(i);
            if (row >= n_rows) continue;
            const uint32_t e = tab.get(row);
            if (open && !(i - last_i <= 1u + bridge && joined(last_e, e, (uint32_t)(i - last_i)))) close();
            if (!open) {
                if (n < capacity) segs[n] = Segment{(uint32_t)s, strand, (uint32_t)(i - begin + 1u - k), 0u, e & kPosMask, 0u, start_flags(e)};
                add(e, true);
                open = true;
            }
            last_i = i;
            last_e = e;
        }
        if (open) close();
    }
    return n;
}

// ---- the three-pass scan, one chunk / the sums at a time.  A: T get(uint64_t i), void set(uint64_t i, T v)
template <typename T, typename A> KBO_ST_FN T scan_chunk_sum(const A &in, uint64_t n, uint64_t chunk)
{
    T s = 0;
    for (uint64_t i = chunk * kScanChunk; i < n && i < (chunk + 1u) * kScanChunk; i++) s += in.get(i);
    return s;
}
template <typename T, typename A> KBO_ST_FN T scan_sums(A &sums, uint64_t n_chunks) // exclusive, in place; returns the total
{
    T run = 0;
    for (uint64_t c = 0; c < n_chunks; c++) {
        const T v = sums.get(c);
        sums.set(c, run);
        run += v;
    }
    return run;
}
template <typename T, typename A, typename B> KBO_ST_FN void scan_chunk_apply(const A &in, B &out, uint64_t n, uint64_t chunk, T prefix, bool inclusive)
{
    T run = prefix;
    for (uint64_t i = chunk * kScanChunk; i < n && i < (chunk + 1u) * kScanChunk; i++) {
        const T v = in.get(i);
        out.set(i, inclusive ? run + v : run);
        run += v;
    }
}
KBO_ST_FN uint64_t scan_chunks(uint64_t n) { return (n + kScanChunk - 1u) / kScanChunk; }

// ---- d_work of kbo_segments_dev: a flag byte per base | a tile's starts and ends (one 64-bit word) | the scan's sums; of
// kbo_depth_finish_dev: the scan's sums
KBO_ST_FN uint64_t round16(uint64_t v) { return (v + 15u) / 16u * 16u; }
struct SegWork {
    uint64_t counts_off, sums_off, bytes;
};
KBO_ST_FN SegWork seg_work(uint64_t total)
{
    SegWork w;
    w.counts_off = round16(total);
    w.sums_off = w.counts_off + round16((uint64_t)n_tiles(total) * 8u);
    w.bytes = w.sums_off + round16(scan_chunks(n_tiles(total)) * 8u);
    return w;
}
KBO_ST_FN uint64_t depth_work(uint64_t source_bases) { return round16(scan_chunks(source_bases) * 4u); }

} // namespace idxlocate
} // namespace kbo
