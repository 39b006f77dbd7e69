// index_indel.hpp — the insertions and deletions the reads of a walked batch carry, in source coordinates (kbo_hip.h "Indels";
// DESIGN.md 4.16), for host and device alike: indel_kernels.hip runs it a lane per pair of records and a lane per event,
// index_indel.cpp restates it on the CPU (kbo_indels_from_segments_host, kbo_indel_sites_host), tools/index_indel_check.cpp runs it
// through accessors that check every index.
//
// Take the records of one kbo_segments_dev call in list order and the batch as it was walked.
//   intervals     of a record s, rev = flag bit 0: Q(s) = [q_first, q_last + k); S(s) = [pos_first, pos_last + k) FWD,
//                 [pos_last, pos_first + k) REV.
//   a pair        records x - 1 = A and x = B count when both hold something (idxpile::record_taken, record_span), have one seq and
//                 one rev, and A.q_last < B.q_first.  FWD: lower = A, upper = B; REV: lower = B, upper = A.  In 64 signed bits:
//                 gq = B.q_first - (A.q_last + k), gs = S(upper).lo - S(lower).hi, shift = gs - gq (kbo_place_dev's shift).
//   the junction  shift == 0 or |shift| > max_indel: nothing.  gq > 0 and gs > 0: COMPLEX (an indel with a mismatch next to it),
//                 counted and not written.  Otherwise shift > 0 (then gq <= 0) is a DELETION of len = shift at pos = S(upper).lo -
//                 len, shift < 0 (then gs <= 0) an INSERTION of len = -shift in front of pos = S(upper).lo: pair_event().
//   left-aligned  the upper segment reaches down exactly as far as the read matches its diagonal, so pos is the leftmost placement and
//                 depends on `upper` and `shift` alone.
//   the bases     of an insertion in source orientation: FWD the bytes [B.q_first - len, B.q_first) of the sequence, REV the reverse
//                 complement of [A.q_last + k, A.q_last + k + len).  code packs base i (ascending source order) at bits [2i, 2i + 2)
//                 for len <= kCodeLen; beyond, code = 0 and LONG is set.  A byte that is no base: no event (insert_code).
//   no event      when the bytes would leave the sequence, pos < 0, pos (+ len for a deletion) > source_bases, or S(upper).lo and
//                 S(lower).hi - 1 lie in different sources.
//   a len         is below 2^30 (kLenMask): a max_indel above that counts as that.
//   sites         the events that hold an event (event_key: what pair_event can write) grouped by (pos, kind_len, code), ascending as
//                 unsigned words; a group is a site when count >= min_count and count * frac_den >= frac_num * depth, depth =
//                 DEPTH[pos - 1] (DEPTH[0] at pos 0): the base in front, which reads with and without the indel both cover.
#pragma once
#include <stdint.h>

#include "index_pileup.hpp"

namespace kbo {
namespace idxindel {

using idxlocate::kScanChunk;
using idxlocate::round16;
using idxlocate::scan_chunks;
using idxlocate::Segment;
using idxlocate::seq_of;
using idxpile::record_span;
using idxpile::record_taken;
using idxpile::Thresholds;

constexpr uint32_t kThreads = 256, kPer = kScanChunk / kThreads;
constexpr uint32_t kIns = 1u << 31, kLong = 1u << 30, kLenMask = kLong - 1u, kMinus = 1u, kCodeLen = 16;
constexpr uint32_t kStrandRev = 2u; // KBO_STRAND_REV
constexpr uint32_t kMaxSeqs = idxpile::kMaxSeqs;
constexpr uint64_t kMaxSegs = idxpile::kMaxSegs, kMaxEvents = 0xFFFFFFFEull;
constexpr uint32_t kNone = 0, kEvent = 1, kComplex = 2; // what a pair is

struct Event { // == kbo_indel_event
    uint32_t pos, kind_len, code, flags;
};
struct Site { // == kbo_indel_site
    uint32_t pos, source, kind_len, code, count, n_minus, depth, reserved;
};
static_assert(sizeof(Event) == 16 && sizeof(Site) == 32, "four and eight words");

// ---- a pair
struct Cand {
    uint32_t pos, len;
    bool ins, rev, minus;
    uint64_t bytes_at; // an insertion's bytes in the batch: [bytes_at, bytes_at + len)
};
// Off: uint64_t off(size_t s) with n_seqs + 1 values; SrcOff: the same with n_src + 1 values
template <typename Off, typename SrcOff>
KBO_ST_FN uint32_t pair_event(const Segment &A, const Segment &B, const Off &off, uint32_t n_seqs, uint64_t total, uint32_t k, bool skip_multi,
                              uint32_t max_indel, uint64_t source_bases, const SrcOff &so, uint32_t n_src, Cand *c)
{
    if (!record_taken(A, n_seqs, skip_multi) || !record_taken(B, n_seqs, skip_multi)) return kNone;
    if (A.seq != B.seq || ((A.flags ^ B.flags) & idxlocate::kSegRev)) return kNone;
    const uint64_t o = off.off(A.seq), e = off.off((size_t)A.seq + 1u);
    if (!record_span(A, o, e, total, k) || !record_span(B, o, e, total, k)) return kNone;
    if (!(A.q_last < B.q_first)) return kNone;
    const bool rev = (A.flags & idxlocate::kSegRev) != 0u;
    const Segment &lower = rev ? B : A, &upper = rev ? A : B;
    const int64_t up_lo = rev ? (int64_t)upper.pos_last : (int64_t)upper.pos_first;
    const int64_t low_hi = (rev ? (int64_t)lower.pos_first : (int64_t)lower.pos_last) + (int64_t)k;
    const int64_t gq = (int64_t)B.q_first - ((int64_t)A.q_last + (int64_t)k), gs = up_lo - low_hi, shift = gs - gq;
    if (shift == 0) return kNone;
    const int64_t mag = shift < 0 ? -shift : shift;
    if (mag > (int64_t)(max_indel < kLenMask ? max_indel : kLenMask)) return kNone;
    if (gq > 0 && gs > 0) return kComplex;
    const bool ins = shift < 0; // (shift > 0 leaves gq <= 0 here, shift < 0 gs <= 0)
    const int64_t pos = ins ? up_lo : up_lo - mag;
    if (pos < 0 || (uint64_t)up_lo > source_bases) return kNone;
    if (seq_of(so, n_src, (uint64_t)up_lo) != seq_of(so, n_src, (uint64_t)(low_hi - 1))) return kNone;
    uint64_t at = 0;
    if (ins) {
        if (rev) {
            at = (uint64_t)A.q_last + k;
            if (at + (uint64_t)mag > e - o) return kNone;
        } else {
            if ((int64_t)B.q_first < mag) return kNone;
            at = (uint64_t)B.q_first - (uint64_t)mag;
        }
    }
    c->pos = (uint32_t)pos;
    c->len = (uint32_t)mag;
    c->ins = ins;
    c->rev = rev;
    c->minus = rev != (B.strand == kStrandRev);
    c->bytes_at = o + at;
    return kEvent;
}
// the code of an insertion's bases; false: one of them is no base.  Seq: uint32_t at(uint64_t i) over the batch
template <typename Seq> KBO_ST_FN bool insert_code(const Seq &seq, const Cand &c, uint32_t *code)
{
    uint32_t v = 0;
    for (uint32_t i = 0; i < c.len; i++) { // i: ascending source order
        const uint32_t b = refstep::base_code(seq.at(c.bytes_at + (c.rev ? c.len - 1u - i : i)));
        if (b > 3u) return false;
        if (c.len <= kCodeLen) v |= (c.rev ? 3u - b : b) << (2u * i);
    }
    *code = v;
    return true;
}
// ... and back: base i of a code, as a byte
KBO_ST_FN uint32_t code_base(uint32_t code, uint32_t i) { return (0x54474341u >> (8u * ((code >> (2u * i)) & 3u))) & 0xFFu; }
KBO_ST_FN Event event_of(const Cand &c, uint32_t code)
{
    return Event{c.pos, c.len | (c.ins && c.len > kCodeLen ? kLong : 0u) | (c.ins ? kIns : 0u), code, c.minus ? kMinus : 0u};
}
// the pair (A, B) whole: kEvent with *ev, kComplex or kNone
template <typename Off, typename SrcOff, typename Seq>
KBO_ST_FN uint32_t pair_whole(const Segment &A, const Segment &B, const Off &off, uint32_t n_seqs, uint64_t total, uint32_t k, bool skip_multi,
                              uint32_t max_indel, uint64_t source_bases, const SrcOff &so, uint32_t n_src, const Seq &seq, Event *ev)
{
    Cand c;
    const uint32_t what = pair_event(A, B, off, n_seqs, total, k, skip_multi, max_indel, source_bases, so, n_src, &c);
    if (what != kEvent) return what;
    uint32_t code = 0;
    if (c.ins && !insert_code(seq, c, &code)) return kNone;
    *ev = event_of(c, code);
    return kEvent;
}
// the serial form of a call.  Segs: Segment get(uint64_t x); Out: void set(uint64_t n, Event).  Event number base + i is written iff it
// is below capacity; returns the events of the call
template <typename Segs, typename Off, typename SrcOff, typename Seq, typename Out>
KBO_ST_FN uint64_t events_serial(const Segs &segs, uint64_t n, const Off &off, uint32_t n_seqs, uint64_t total, uint32_t k, bool skip_multi,
                                 uint32_t max_indel, uint64_t source_bases, const SrcOff &so, uint32_t n_src, const Seq &seq, Out &out, uint64_t base,
                                 uint64_t capacity, uint64_t *n_complex)
{
    uint64_t made = 0;
    for (uint64_t x = 1; x < n; x++) {
        Event ev;
        const uint32_t what = pair_whole(segs.get(x - 1u), segs.get(x), off, n_seqs, total, k, skip_multi, max_indel, source_bases, so, n_src, seq, &ev);
        if (what == kComplex && n_complex) ++*n_complex;
        if (what != kEvent) continue;
        if (base + made < capacity) out.set(base + made, ev);
        made++;
    }
    return made;
}

// ---- sites
// the sort key of an event: (pos, kind_len) and (code, flags), most significant first; false: the words hold no event pair_event writes
KBO_ST_FN bool event_key(const Event &e, uint64_t source_bases, uint64_t *w0, uint64_t *w1)
{
    const uint32_t len = e.kind_len & kLenMask;
    const bool ins = (e.kind_len & kIns) != 0u, lng = (e.kind_len & kLong) != 0u;
    if (e.flags > kMinus || len == 0u || (uint64_t)e.pos > source_bases) return false;
    if (ins) {
        if (lng != (len > kCodeLen) || (lng && e.code != 0u)) return false;
        if (len < kCodeLen && (e.code >> (2u * len)) != 0u) return false;
    } else if (lng || e.code != 0u || (uint64_t)e.pos + len > source_bases) {
        return false;
    }
    *w0 = (uint64_t)e.pos << 32 | e.kind_len;
    *w1 = (uint64_t)e.code << 32 | e.flags;
    return true;
}
constexpr uint64_t kPadKey = ~0ull; // both words of a place that holds no event: behind every key, and no key's first word
KBO_ST_FN bool key_valid(uint64_t w0) { return w0 != kPadKey; }
// one group: keys a and b without the MINUS bit
KBO_ST_FN bool same_group(uint64_t a0, uint64_t a1, uint64_t b0, uint64_t b1) { return a0 == b0 && (a1 >> 32) == (b1 >> 32); }
KBO_ST_FN bool key_less(uint64_t a0, uint64_t a1, uint64_t b0, uint64_t b1) { return a0 != b0 ? a0 < b0 : (a1 >> 32) < (b1 >> 32); }
KBO_ST_FN uint32_t key_minus(uint64_t w1) { return (uint32_t)w1 & kMinus; }
// the key bits the sort goes over, counted from the most significant bit of word 0: the bits a pos <= source_bases can set, then all
// of kind_len and code
KBO_ST_FN uint32_t pos_bits(uint64_t source_bases)
{
    uint32_t b = 0;
    while (b < 32u && (source_bases >> b) != 0u) b++;
    return b;
}
KBO_ST_FN uint32_t sort_first_bit(uint64_t source_bases) { return 32u - pos_bits(source_bases); }
constexpr uint32_t kSortEndBit = 96;
KBO_ST_FN uint32_t sort_passes(uint64_t source_bases) { return (kSortEndBit - sort_first_bit(source_bases) + 7u) / 8u; }
KBO_ST_FN bool calls(uint32_t count, uint32_t depth, const Thresholds &t)
{
    return count >= t.min_count && (uint64_t)count * t.frac_den >= (uint64_t)t.frac_num * depth;
}
// where the depth of an event at pos is read; source_bases > 0
KBO_ST_FN uint64_t depth_at(uint32_t pos) { return pos > 0u ? pos - 1u : 0u; }
KBO_ST_FN Site site_of(uint64_t w0, uint64_t w1, uint32_t source, uint32_t count, uint32_t n_minus, uint32_t depth)
{
    return Site{(uint32_t)(w0 >> 32), source, (uint32_t)w0, (uint32_t)(w1 >> 32), count, n_minus, depth, 0u};
}
// the serial form over keys in key_less order, the n valid ones first.  Keys: uint64_t w0(uint64_t i), w1(uint64_t i);
// Depth: uint32_t at(uint64_t j); Out: void set(uint64_t x, Site).  Site x is written iff x < capacity; returns the full count
template <typename Keys, typename Depth, typename SrcOff, typename Out>
KBO_ST_FN uint64_t sites_sorted_serial(const Keys &keys, uint64_t n, const Depth &depth, uint64_t source_bases, const SrcOff &so, uint32_t n_src,
                                       const Thresholds &t, Out &out, uint64_t capacity)
{
    uint64_t made = 0;
    for (uint64_t i = 0; i < n;) {
        const uint64_t w0 = keys.w0(i), w1 = keys.w1(i);
        uint64_t j = i, minus = 0;
        for (; j < n && same_group(w0, w1, keys.w0(j), keys.w1(j)); j++) minus += key_minus(keys.w1(j));
        const uint32_t pos = (uint32_t)(w0 >> 32), d = source_bases ? depth.at(depth_at(pos)) : 0u;
        if (calls((uint32_t)(j - i), d, t)) {
            if (made < capacity) out.set(made, site_of(w0, w1, seq_of(so, n_src, pos), (uint32_t)(j - i), (uint32_t)minus, d));
            made++;
        }
        i = j;
    }
    return made;
}

// ---- d_work of kbo_indels_dev: the scan's sums, 4 bytes per kScanChunk records of capacity rounded up to 16 | the list's count
// before the call (16 bytes)
struct EventWork {
    uint64_t base_off, bytes;
};
KBO_ST_FN EventWork event_work(uint64_t capacity)
{
    EventWork w;
    w.base_off = round16(scan_chunks(capacity) * 4u);
    w.bytes = w.base_off + 16u;
    return w;
}
// ---- d_work of kbo_indel_sites_dev, n = event_capacity: the key words [2][n] twice (the sort's two buffers) | the radix passes'
// histogram, 256 words per tile of 4096 keys, and its sums, a word per 1024 of those + 2 | (first event, MINUS in front of it) of
// every group and of the end [n + 1] | the head scan's sums, 8 bytes per kScanChunk of n + 1 | the site scan's sums, 4 bytes per
// kScanChunk of n | the number of groups (16 bytes); each part rounded up to 16
constexpr uint32_t kRadixTile = 4096, kRadixSumBlock = 1024; // == kBuildTile, device_util.hpp's kScanBlock
struct SiteWork {
    uint64_t keys_b_off, hist_off, rsums_off, grp_off, hsums_off, ssums_off, count_off, bytes;
};
KBO_ST_FN uint64_t radix_tiles(uint64_t n) { return (n + kRadixTile - 1u) / kRadixTile; }
KBO_ST_FN SiteWork site_work(uint64_t n)
{
    SiteWork w;
    w.keys_b_off = round16(n * 16u);
    w.hist_off = 2u * w.keys_b_off;
    w.rsums_off = w.hist_off + round16(256u * radix_tiles(n) * 4u);
    w.grp_off = w.rsums_off + round16((256u * radix_tiles(n) / kRadixSumBlock + 2u) * 4u);
    w.hsums_off = w.grp_off + round16((n + 1u) * 8u);
    w.ssums_off = w.hsums_off + round16(scan_chunks(n + 1u) * 8u);
    w.count_off = w.ssums_off + round16(scan_chunks(n) * 4u);
    w.bytes = w.count_off + 16u;
    return w;
}

} // namespace idxindel
} // namespace kbo
