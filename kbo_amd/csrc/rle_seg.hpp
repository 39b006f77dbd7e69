// rle_seg.hpp — the algebra of the segmented format::run_lengths_gapped (format.rs:143-193), for host and device alike:
// rle_seg_kernels.hip runs it a chunk per lane, rle_seg_host.cpp restates the same passes on the CPU at any chunk size.
//
// Every decision of the reference's loop is local once a '-' knows j, its 1-based place in its stretch of '-', and P, whether
// the byte in front of the stretch is in a run (not ' ', not the sequence's start):
//   in a run:   any byte but '-' and ' ' always; a '-' when P and j <= max_gap_len + 1; a ' ' never
//   a run ends: at the '-' with j == max_gap_len + 1 (that gap is taken back out), in front of a ' ', at the sequence's end
//               (a trailing '-' or 'D' takes the run's most recent gap back out when it has one)
// Two carries run along the chunks of a sequence, each with an associative combine: Dash (what a stretch of '-' that reaches
// into a chunk needs to know) and Part (the record so far of the run that is open where a chunk begins).  The number of runs
// that end in a chunk needs no carry of its own once the chunk knows its Dash: it is a plain sum.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define KBO_RS_FN __host__ __device__ __forceinline__
#else
#define KBO_RS_FN inline
#endif

namespace kbo {
namespace rleseg {

// ---- the dash carry: t '-' stand at the end of the stretch of positions it describes; kAll: it holds nothing else (t adds up);
// kP: the byte in front of those t - or, with t == 0, the last byte - is in a run
constexpr uint32_t kAll = 1u, kP = 2u;
struct Dash {
    uint32_t t, flags;
};
KBO_RS_FN Dash dash_identity() { return Dash{0u, kAll}; } // also a sequence's start: nothing in front, P unset
KBO_RS_FN Dash dash_combine(const Dash &a, const Dash &b) { return (b.flags & kAll) ? Dash{a.t + b.t, a.flags} : b; }
// summary of n >= 1 positions, c(q) = byte q of them
template <typename Get> KBO_RS_FN Dash dash_summary(Get c, uint32_t n)
{
    uint32_t t = 0;
    while (t < n && c(n - 1u - t) == (uint32_t)'-') t++;
    if (t == n) return Dash{n, kAll};
    return Dash{t, c(n - 1u - t) != (uint32_t)' ' ? kP : 0u};
}

// ---- the open run: a record in the making.  last = j of the run's most recent '-' (0: none yet)
struct Rec {
    uint32_t start, end, matches, mismatches, jumps, gap_bases, gap_opens, last;
};
// kOpen: a run is open behind the positions described; kFull: ALL of them belong to one run that none of them ends - so the
// run that was open in front of them goes on (kFull without kOpen: no positions at all, the identity)
constexpr uint32_t kOpen = 1u, kFull = 2u;
struct alignas(16) Part {
    Rec r;
    uint32_t flags, pad0, pad1, pad2;
};
KBO_RS_FN Rec rec_zero() { return Rec{0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u}; }
KBO_RS_FN Part part_identity() { return Part{rec_zero(), kFull, 0u, 0u, 0u}; }
KBO_RS_FN Rec rec_merge(const Rec &a, const Rec &b) // b continues a
{
    return Rec{a.start, b.end ? b.end : a.end, a.matches + b.matches, a.mismatches + b.mismatches, a.jumps + b.jumps,
               a.gap_bases + b.gap_bases, a.gap_opens + b.gap_opens, b.last ? b.last : a.last};
}
KBO_RS_FN Part part_combine(const Part &a, const Part &b)
{ // !kFull: b alone; kFull without kOpen: a alone; else b continues a's run, if a has one.  (Field by field: the records stay in registers)
    const bool only_a = (b.flags & (kFull | kOpen)) == kFull, joined = (b.flags & (kFull | kOpen)) == (kFull | kOpen) && (a.flags & kOpen);
    const Rec m = rec_merge(a.r, b.r);
    auto pick = [&](uint32_t va, uint32_t vb, uint32_t vm) { return only_a ? va : joined ? vm : vb; };
    return Part{Rec{pick(a.r.start, b.r.start, m.start), pick(a.r.end, b.r.end, m.end), pick(a.r.matches, b.r.matches, m.matches),
                    pick(a.r.mismatches, b.r.mismatches, m.mismatches), pick(a.r.jumps, b.r.jumps, m.jumps),
                    pick(a.r.gap_bases, b.r.gap_bases, m.gap_bases), pick(a.r.gap_opens, b.r.gap_opens, m.gap_opens),
                    pick(a.r.last, b.r.last, m.last)},
                only_a ? a.flags : (b.flags & kFull) ? (kOpen | (a.flags & kFull)) : b.flags, 0u, 0u, 0u};
}

// ---- one position.  t / P: the dash carry in front of it; open / r: the run in front of it
struct Walk {
    uint32_t t, P, open;
    Rec r;
};
KBO_RS_FN Walk walk_begin(const Dash &d, const Part &in)
{
    return Walk{d.t, (d.flags & kP) ? 1u : 0u, (in.flags & kOpen) ? 1u : 0u, in.r};
}
// c = the byte at position i of a sequence of len, prev = the byte in front of it (anything but 'R' at i == 0), next = the byte behind it
// (unused at i + 1 == len).  close(rec) is called with the finished record when a run ends here; `broke` is set when the position
// is in no run or ends one (a chunk that never sets it is kFull).  max_gap_len may be 2^32 - 1: j - 1 is compared, never j against gap + 1
template <typename Close>
KBO_RS_FN void walk_step(Walk &w, uint32_t c, uint32_t prev, uint32_t next, uint32_t i, uint32_t len, uint32_t max_gap_len, bool &broke,
                         Close &&close)
{
    const bool dash = c == (uint32_t)'-';
    w.t = dash ? w.t + 1u : 0u;
    const bool in_run = dash ? (w.P && w.t - 1u <= max_gap_len) : c != (uint32_t)' ';
    if (!dash) w.P = c != (uint32_t)' ';
    if (!in_run) {
        broke = true;
        return;
    }
    if (!w.open) { // format.rs:148-152
        w.open = 1u;
        w.r = rec_zero();
        w.r.start = i;
    }
    const bool is_match = c == (uint32_t)'M' || c == (uint32_t)'R' || c == (uint32_t)'I';
    const bool is_gap = dash || c == (uint32_t)'D';
    w.r.matches += is_match;
    w.r.gap_bases += is_gap;
    w.r.mismatches += (!is_match && !is_gap);
    if (!is_gap) w.r.end = i + 1u;
    w.r.jumps += (c == (uint32_t)'R' && i > 0u && prev == (uint32_t)'R'); // (guarded; the reference indexes aln[i - 1], format.rs:175)
    if (dash) {
        w.r.gap_opens += (w.t == 1u);
        w.r.last = w.t;
    }
    const bool overflow = dash && w.t - 1u == max_gap_len, at_end = i + 1u == len;
    if (overflow || at_end || next == (uint32_t)' ') { // (format.rs:154: a blank ends the run in front of it and is not consumed)
        if (overflow) {
            w.r.gap_opens -= 1u;
            w.r.gap_bases -= w.t;
        } else if (at_end && is_gap && w.r.gap_opens > 0u) { // (behind a 'D' `last` is stale: the reference does just that)
            w.r.gap_opens -= 1u;
            w.r.gap_bases -= w.r.last;
        }
        close(w.r);
        w.open = 0u;
        broke = true;
    }
}
// what a chunk leaves behind: the run open at its end, and whether it only continued the one in front of it
KBO_RS_FN Part walk_end(const Walk &w, bool broke)
{
    return Part{w.open ? w.r : rec_zero(), (w.open ? kOpen : 0u) | (broke ? 0u : kFull), 0u, 0u, 0u};
}

} // namespace rleseg
} // namespace kbo
