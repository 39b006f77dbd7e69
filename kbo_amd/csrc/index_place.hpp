// index_place.hpp — from the segments of a walked batch to ONE placement per sequence (kbo_hip.h "Placement"), for host
// and device alike: place_kernels.hip runs it a lane or a wave per sequence, index_place.cpp restates it on the CPU
// (kbo_place_from_segments_host), tools/index_place_check.cpp runs it through accessors that check every index.
//
// The segments of one sequence from one kbo_segments_dev call are s_0 .. s_{n-1} in list order, disjoint stretches of the anchor list.
//   a segment     len = q_last - q_first + k, rev = flag bit 0, diag = pos_first - q_first (FWD) / pos_first + q_first (REV) in 64 signed
//                 bits, src = the last source whose offset is <= pos_first (idxlocate::seq_of): seg_of().
//   j before i    i - kWindow <= j < i, one rev, one src, g = q_first_i - q_last_j <= max_gap, |shift| <= max_indel and g + shift >= 1,
//                 shift = diag_i - diag_j (FWD) / diag_j - diag_i (REV): precedes().  gain = min(len_i, q_last_i - q_last_j).
//   chains        f_i = max(len_i, max over j before i of f_j + gain): the predecessor with the largest value, ties to the larger j, none
//                 when len_i is at least that value.  A State is what the next kWindow steps need of a segment and what its chain
//                 carries: root, segments, the sum of |shift|, segments with a MULTI end.  chain_step() is one i against a ring of States.
//   the placement the end with the largest f, ties to the smaller i; second = the largest f of an end with another root: Top, top_add().
//   ranges        begin[s] = the smallest x with seq == s that starts a stretch of equal seq values, end[s] = 1 + the largest x that ends
//                 one (integer atomics on the device: the same words whatever the arrival order, and whatever the list holds).  Inside
//                 [begin, end) a record of another sequence takes its slot and is otherwise skipped.
//   routes        a list of at most kLaneMax segments is chained by one lane in registers, a longer one by a wave: lane l holds the
//                 State in slot l of the ring, the predecessor of step i that is congruent to l, and the maximum with its tie rule is a
//                 reduction over the lanes.  Both are chain_step()'s rule; place_serial() is the whole call, one sequence after the other.
#pragma once
#include <stdint.h>

#include "index_locate.hpp"

namespace kbo {
namespace idxplace {

using idxlocate::round16;
using idxlocate::Segment;
using idxlocate::seq_of;

constexpr uint32_t kWindow = 64;  // W: the predecessors a step looks at; a wave's lanes
constexpr uint32_t kLaneMax = 4;  // lists of at most this many segments take the lane route (LABNOTES "Placement": where it comes from)
constexpr uint32_t kThreads = 256;
constexpr uint32_t kPlaceNone = 0xFFFFFFFFu, kNoRange = 0xFFFFFFFFu;
constexpr uint32_t kPlaceRev = 1u, kPlaceSpills = 2u;
constexpr uint32_t kMaxSeqs = 1u << 28;
constexpr uint64_t kMaxSegs = 0xFFFFFFFEull; // records a call looks at: list indices are 32-bit, and kNoRange is none of them
static_assert(kWindow == 64 && kLaneMax < kWindow, "a wave's lanes are the window");

struct Place { // == kbo_seq_place
    uint32_t source;
    uint16_t strand, flags;
    uint32_t q_start, q_end, pos_start, pos_end, score, n_segs, indel, n_multi, second, reserved;
};
static_assert(sizeof(Place) == 48, "twelve words");

struct Limits {
    uint32_t k, max_gap, max_indel;
};

// ---- a segment as the chaining sees it
struct Seg {
    uint32_t len, q_first, q_last, src;
    bool rev, multi;
    int64_t diag;
};
KBO_ST_FN Seg seg_of(const Segment &s, uint32_t k, uint32_t src)
{
    Seg c;
    c.len = s.q_last - s.q_first + k;
    c.q_first = s.q_first;
    c.q_last = s.q_last;
    c.src = src;
    c.rev = (s.flags & idxlocate::kSegRev) != 0u;
    c.multi = (s.flags & (idxlocate::kSegFirstMulti | idxlocate::kSegLastMulti)) != 0u;
    c.diag = c.rev ? (int64_t)s.pos_first + (int64_t)s.q_first : (int64_t)s.pos_first - (int64_t)s.q_first;
    return c;
}

// ---- the state a segment leaves in the ring
constexpr uint32_t kTagValid = 1u, kTagRev = 2u;
struct State {
    uint32_t q_last, src, tag; // tag 0: no segment (a skipped record)
    int64_t diag;
    uint32_t f, root, n_segs, indel, n_multi;
};
KBO_ST_FN State no_state() { return State{0u, 0u, 0u, 0, 0u, 0u, 0u, 0u, 0u}; }

// may the segment that left p precede c?  *shift: the bases the source advances beyond the query (> 0 a deletion in the sequence)
KBO_ST_FN bool precedes(const State &p, const Seg &c, const Limits &lim, int64_t *shift)
{
    if (!(p.tag & kTagValid) || ((p.tag & kTagRev) != 0u) != c.rev || p.src != c.src) return false;
    const int64_t g = (int64_t)c.q_first - (int64_t)p.q_last; // (|diag| < 2^33: nothing below overflows)
    const int64_t sh = c.rev ? p.diag - c.diag : c.diag - p.diag;
    *shift = sh;
    return g <= (int64_t)lim.max_gap && (sh < 0 ? -sh : sh) <= (int64_t)lim.max_indel && g + sh >= 1;
}
KBO_ST_FN uint32_t gain(const State &p, const Seg &c)
{
    const uint32_t d = c.q_last - p.q_last;
    return c.len < d ? c.len : d;
}
// the value c's chain has through p (the arithmetic is modulo 2^32: a list in order never wraps, any other stays defined)
KBO_ST_FN uint32_t value_through(const State &p, const Seg &c) { return p.f + gain(p, c); }
// the state of segment i: on its own, or behind p with value v (taken: v > len)
KBO_ST_FN State extend(const Seg &c, uint32_t i, bool taken, const State &p, uint32_t v, int64_t shift)
{
    State n;
    n.q_last = c.q_last;
    n.src = c.src;
    n.tag = kTagValid | (c.rev ? kTagRev : 0u);
    n.diag = c.diag;
    n.f = taken ? v : c.len;
    n.root = taken ? p.root : i;
    n.n_segs = taken ? p.n_segs + 1u : 1u;
    n.indel = taken ? p.indel + (uint32_t)(shift < 0 ? -shift : shift) : 0u;
    n.n_multi = (taken ? p.n_multi : 0u) + (c.multi ? 1u : 0u);
    return n;
}
KBO_ST_FN uint32_t slot_of(uint32_t i) { return i & (kWindow - 1u); }
// one step, serial: segment i against the states of i - 1, i - 2, .. i - kWindow.  Ring: State get(uint32_t slot)
template <typename Ring> KBO_ST_FN State chain_step(const Ring &ring, uint32_t i, const Seg &c, const Limits &lim)
{
    bool any = false;
    uint32_t best_v = 0;
    int64_t best_sh = 0;
    State best = no_state();
    const uint32_t w = i < kWindow ? i : kWindow;
    for (uint32_t l = 0; l < w; l++) { // (ascending l = descending j: a later equal value does not replace an earlier one)
        const State p = ring.get(slot_of(i - 1u - l));
        int64_t sh;
        if (!precedes(p, c, lim, &sh)) continue;
        const uint32_t v = value_through(p, c);
        if (!any || v > best_v) {
            any = true;
            best_v = v;
            best_sh = sh;
            best = p;
        }
    }
    const bool taken = any && best_v > c.len;
    return extend(c, i, taken, best, best_v, best_sh);
}
// the wave's form of the same step picks its winner among the lanes that hold a predecessor with the largest value: lane x holds slot x,
// the segment i - 1 - l with l = (i - 1 - x) mod kWindow, and the smallest l wins.  mask: those lanes, not empty
KBO_ST_FN uint32_t winner_slot(uint64_t mask, uint32_t i)
{
    const uint32_t r = slot_of(i - 1u), rot = 63u - r;            // slot r (l = 0) to bit 63, r - 1 to bit 62, ..
    const uint64_t m = rot ? (mask << rot) | (mask >> (64u - rot)) : mask;
    const uint32_t l = (uint32_t)__builtin_clzll(m);
    return slot_of(r - l);
}

// ---- the best end and the runner-up with another root
struct Top {
    uint32_t any, f, i, root, n_segs, indel, n_multi, second;
};
KBO_ST_FN Top no_top() { return Top{0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u}; }
KBO_ST_FN void top_add(Top &t, const State &s, uint32_t i)
{
    if (!(s.tag & kTagValid)) return;
    const bool same = t.any && s.root == t.root;
    if (!t.any || s.f > t.f) { // (ties stay with the smaller i)
        if (t.any && !same) t.second = t.f; // (the best so far is at least every other end, and of another root than the new best)
        t.any = 1u;
        t.f = s.f;
        t.i = i;
        t.root = s.root;
        t.n_segs = s.n_segs;
        t.indel = s.indel;
        t.n_multi = s.n_multi;
    } else if (!same && s.f > t.second) {
        t.second = s.f;
    }
}

// ---- the record
KBO_ST_FN Place no_place() { return Place{kPlaceNone, 0, 0, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u}; }
// root, end: the records of the best chain's first and last segment; src: theirs; src_end = src_off[src + 1]
KBO_ST_FN Place place_of(const Top &t, const Segment &root, const Segment &end, uint32_t src, uint64_t src_end, uint32_t k)
{
    Place p = no_place();
    if (!t.any) return p;
    const bool rev = (end.flags & idxlocate::kSegRev) != 0u;
    p.source = src;
    p.strand = (uint16_t)end.strand;
    p.q_start = root.q_first;
    p.q_end = end.q_last + k;
    p.pos_start = rev ? end.pos_last : root.pos_first;
    p.pos_end = (rev ? root.pos_first : end.pos_last) + k;
    p.flags = (uint16_t)((rev ? kPlaceRev : 0u) | ((uint64_t)p.pos_end > src_end ? kPlaceSpills : 0u));
    p.score = t.f;
    p.n_segs = t.n_segs;
    p.indel = t.indel;
    p.n_multi = t.n_multi;
    p.second = t.second;
    return p;
}

// ---- the merge: associative and commutative, the record its own reduction state.  a wins over b: the larger score, then the smaller
// strand, then (two calls with one strand value) the smaller of the remaining fields in their order; kPlaceNone loses to anything
KBO_ST_FN bool wins(const Place &a, const Place &b)
{
    if (b.source == kPlaceNone) return true;
    if (a.source == kPlaceNone) return false;
    if (a.score != b.score) return a.score > b.score;
    if (a.strand != b.strand) return a.strand < b.strand;
    const uint32_t x[10] = {a.source, a.flags, a.q_start, a.q_end, a.pos_start, a.pos_end, a.n_segs, a.indel, a.n_multi, a.second};
    const uint32_t y[10] = {b.source, b.flags, b.q_start, b.q_end, b.pos_start, b.pos_end, b.n_segs, b.indel, b.n_multi, b.second};
    for (uint32_t w = 0; w < 10u; w++)
        if (x[w] != y[w]) return x[w] < y[w];
    return true;
}
KBO_ST_FN Place merged(const Place &a, const Place &b)
{
    const bool first = wins(a, b);
    Place w = first ? a : b;
    const Place &l = first ? b : a;
    const uint32_t s = l.second > l.score ? l.second : l.score;
    if (s > w.second) w.second = s;
    return w;
}

// ---- d_work of kbo_place_dev: begin[n_seqs] | end[n_seqs] | the sequences of the wave route [n_seqs] | their number (16 bytes) | the
// source of every record [capacity]; words of 32 bits, each part rounded up to 16 bytes
struct PlaceWork {
    uint64_t end_off, list_off, count_off, src_off, bytes;
};
KBO_ST_FN PlaceWork place_work(uint64_t n_seqs, uint64_t capacity)
{
    PlaceWork w;
    w.end_off = round16(n_seqs * 4u);
    w.list_off = 2u * w.end_off;
    w.count_off = 3u * w.end_off;
    w.src_off = w.count_off + 16u;
    w.bytes = w.src_off + round16(capacity * 4u);
    return w;
}

// ---- the stages, serial.  Segs: Segment get(uint64_t x); Off: uint64_t off(size_t s) with n_src + 1 values;
// Work: uint32_t begin(s), end(s), src(x) and set_begin, set_end, set_src; Ring: State get(slot), void set(slot, State)
template <typename Segs, typename Work> KBO_ST_FN void ranges_serial(const Segs &segs, uint32_t n, uint32_t n_seqs, Work &w)
{
    for (uint32_t s = 0; s < n_seqs; s++) {
        w.set_begin(s, kNoRange);
        w.set_end(s, 0u);
    }
    for (uint32_t x = 0; x < n; x++) {
        const uint32_t s = segs.get(x).seq;
        if (s >= n_seqs) continue;
        if ((x == 0 || segs.get(x - 1u).seq != s) && x < w.begin(s)) w.set_begin(s, x);
        if ((x + 1u == n || segs.get(x + 1u).seq != s) && x + 1u > w.end(s)) w.set_end(s, x + 1u);
    }
}
template <typename Segs, typename Off, typename Work> KBO_ST_FN void sources_serial(const Segs &segs, uint32_t n, const Off &so, uint32_t n_src, Work &w)
{
    for (uint32_t x = 0; x < n; x++) w.set_src(x, seq_of(so, n_src, segs.get(x).pos_first));
}
// the records [b, e) of sequence s, b < e <= the records of the call
template <typename Segs, typename Off, typename Work, typename Ring>
KBO_ST_FN Place chain_serial(const Segs &segs, const Off &so, const Work &w, Ring &ring, uint32_t s, uint32_t b, uint32_t e, const Limits &lim)
{
    Top top = no_top();
    for (uint32_t i = 0; i < e - b; i++) {
        const Segment sg = segs.get(b + i);
        State st = no_state();
        if (sg.seq == s) st = chain_step(ring, i, seg_of(sg, lim.k, w.src(b + i)), lim);
        ring.set(slot_of(i), st);
        top_add(top, st, i);
    }
    if (!top.any) return no_place();
    const uint32_t src = w.src(b + top.root);
    return place_of(top, segs.get(b + top.root), segs.get(b + top.i), src, so.off((size_t)src + 1u), lim.k);
}
KBO_ST_FN bool has_range(uint32_t b, uint32_t e, uint32_t n) { return b != kNoRange && b < e && e <= n; }
// the whole call.  Out: Place get(uint32_t s), void set(uint32_t s, Place)
template <typename Segs, typename Off, typename Work, typename Ring, typename Out>
KBO_ST_FN void place_serial(const Segs &segs, uint32_t n, uint32_t n_seqs, const Off &so, uint32_t n_src, const Limits &lim, bool merge, Work &w,
                            Ring &ring, Out &out)
{
    ranges_serial(segs, n, n_seqs, w);
    sources_serial(segs, n, so, n_src, w);
    for (uint32_t s = 0; s < n_seqs; s++) {
        const uint32_t b = w.begin(s), e = w.end(s);
        const Place p = has_range(b, e, n) ? chain_serial(segs, so, w, ring, s, b, e, lim) : no_place();
        out.set(s, merge ? merged(out.get(s), p) : p);
    }
}

} // namespace idxplace
} // namespace kbo
