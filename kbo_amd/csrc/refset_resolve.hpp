// refset_resolve.hpp — the second pass of kbo::call against a set of references without an index or an automaton of the sequence
// (kbo_hip.h "The VARIANTS of a pair", kbo_call_refset_dev), for host and device alike:
// refset_resolve_kernels.hip runs it behind the last slab of a device-resident call, refset_calls.cpp restates it on the CPU
// (kbo_call_refset_host_indexed, kbo_refset_kmer_depths_host), tools/refset_resolve_check.cpp runs it through accessors that check
// every index.
//
// What resolve_variant (variant_calling.rs:139-201) reads of a site are three numbers: the common suffix of the query-side k-mer and
// the row's k-mer, and the rightmost significant peak of each of the two walks' depths.  The query-side depths come from the site's
// window.  The depth of the ROW's k-mer at position t is the longest suffix of kmer[0 ..= t] that occurs in an ACGT run of at least
// k bases of the sequence on the site's strand (run_automaton.hpp has the argument), and a peak needs it exactly only where it is
// at least q <= the smallest threshold.  So:
//   index   ONE list of words { q-mer code << 32 | start } over the '+' strand of the whole batch, a word per start position whose
//           q-mer lies inside a run of at least k bases of its own sequence (kInvalidWord, a code no q-mer has, for every other
//           position), sorted by code:
//           the occurrences of a q-mer are contiguous and ascend by position, so those of ONE sequence are a range found by bisection
//   probe   the q-mer that ends at t, looked up forwards (the '+' strand) or as its reverse complement (a string occurs in the runs
//           of revcomp(s) iff its reverse complement occurs in the runs of s), every occurrence inside the site's own sequence
//           extended base by base over bases only: an extension never leaves the occurrence's run
//   word    resolve_variant's case analysis on the three numbers; what the reference panics on is kPanic
//   order   the variants leave in the order (ref, seq, strand, i): two key words a site, radix-sorted
// Accessors:
//   Seq    uint32_t byte(uint64_t p)   byte p of the '+' batch          Kmer   uint32_t byte(uint32_t t)   character t of a k-mer
//   Index  uint64_t word(uint64_t x)   word x of the sorted list        Win    uint32_t byte(uint32_t t)   byte t of a window record
#pragma once
#include <stdint.h>

#include "refset_step.hpp"

namespace kbo {
namespace refresolve {

constexpr uint32_t kQMax = 12;                            // 24 bits of code
// a position without a word: bit 24 of the code field, which no code has (q = 12 uses all 24 bits below it: T x 12 is 0xFFFFFF), so
// the words that are no occurrence sort behind every occurrence of every code - the field is sorted as 25 bits, four radix passes
constexpr uint32_t kCodeBits = 2u * kQMax + 1u;
constexpr uint64_t kInvalidWord = 0x01FFFFFFFFFFFFFFull;
constexpr uint32_t kNoPeak = 0xFFu;
constexpr uint32_t kNoVariant = 0xFFFFFFFFu, kPanic = 0xFFFFFFFEu; // resolve words that are no slices (a slice begins below 0xFF)
constexpr uint32_t kModeFwd = 1, kModeRev = 2;            // kbo_refset_kmer_depths_host's mode bits

KBO_ST_FN uint32_t qmer_len(uint32_t min_thr, uint32_t k)
{
    const uint32_t q = min_thr < kQMax ? min_thr : kQMax;
    return q < 1u ? 1u : (q < k ? q : k);
}
// how a site probes: both ways with add_revcomp, else the way of its strand
KBO_ST_FN uint32_t probe_mode(uint32_t strand, bool add_revcomp) { return add_revcomp ? kModeFwd | kModeRev : (strand == 2u ? kModeRev : kModeFwd); }

// the word of start position p of a sequence that owns [begin, end) of the batch
template <typename Seq> KBO_ST_FN uint64_t index_word(const Seq &s, uint64_t begin, uint64_t end, uint64_t p, uint32_t k, uint32_t q)
{
    if (p < begin || p + q > end) return kInvalidWord;
    uint32_t right = 0, code = 0; // bases from p on, at most k of them
    for (uint64_t x = p; x < end && right < k; x++, right++) {
        const uint32_t c = refstep::base_code(s.byte(x));
        if (c > 3u) break;
        if (right < q) code = (code << 2) | c;
    }
    if (right < q) return kInvalidWord;
    uint32_t run = right; // ... and those in front of it until the run is known to hold k
    for (uint64_t x = p; x > begin && run < k; x--, run++)
        if (refstep::base_code(s.byte(x - 1u)) > 3u) break;
    return run >= k ? ((uint64_t)code << 32) | p : kInvalidWord;
}

// the first of n sorted words that is not below w
template <typename Index> KBO_ST_FN uint64_t lower_bound(const Index &ix, uint64_t n, uint64_t w)
{
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2u;
        if (ix.word(mid) < w) lo = mid + 1u;
        else hi = mid;
    }
    return lo;
}

// the depth of the k-mer at position t against the runs of the sequence that owns [begin, end), if it is at least q; else 0
template <typename Kmer, typename Seq, typename Index>
KBO_ST_FN uint32_t depth_at(const Kmer &km, uint32_t t, uint32_t q, uint32_t mode, const Seq &s, uint64_t begin, uint64_t end, const Index &ix,
                            uint64_t n)
{
    if (t + 1u < q || end - begin < q) return 0u;
    uint32_t code = 0, rcode = 0;
    for (uint32_t m = 0; m < q; m++) {
        const uint32_t c = refstep::base_code(km.byte(t + 1u - q + m));
        if (c > 3u) return 0u; // (a byte that is no base resets the depth: it is below q here)
        code = (code << 2) | c;
        rcode |= (3u - c) << (2u * m); // the reverse complement: the last base's complement first
    }
    uint32_t best = 0;
    if (mode & kModeFwd) // the q-mer at st .. st + q - 1: the match goes on backwards from st - 1 / t - q
        for (uint64_t x = lower_bound(ix, n, ((uint64_t)code << 32) | begin); x < n && best <= t; x++) {
            const uint64_t w = ix.word(x), st = w & 0xFFFFFFFFull;
            if ((uint32_t)(w >> 32) != code || st + q > end) break;
            uint32_t len = q;
            while (len <= t && st + q - 1u >= begin + len) {
                const uint32_t c = km.byte(t - len);
                if (refstep::base_code(c) > 3u || s.byte(st + q - 1u - len) != c) break;
                len++;
            }
            best = len > best ? len : best;
        }
    if (mode & kModeRev) // the complement of character t - m at st + m: the match goes on forwards from st + q / t - q
        for (uint64_t x = lower_bound(ix, n, ((uint64_t)rcode << 32) | begin); x < n && best <= t; x++) {
            const uint64_t w = ix.word(x), st = w & 0xFFFFFFFFull;
            if ((uint32_t)(w >> 32) != rcode || st + q > end) break;
            uint32_t len = q;
            while (len <= t && st + len < end) {
                const uint32_t c = refstep::base_code(km.byte(t - len));
                if (c > 3u || refstep::base_code(s.byte(st + len)) != 3u - c) break;
                len++;
            }
            best = len > best ? len : best;
        }
    return best;
}

// position t of the query-side walk of a site with match j: the depth resolve_variant sees there (refset_calls.cpp resolve_sites)
KBO_ST_FN uint32_t query_depth(uint32_t win_byte, uint32_t t, uint32_t j, uint32_t k)
{
    const int64_t pos = (int64_t)j - (int64_t)(k - 1u) + (int64_t)t;
    if (pos < 0) return 0u;
    uint32_t d = win_byte < t + 1u ? win_byte : t + 1u;
    return (int64_t)d < pos + 1 ? d : (uint32_t)(pos + 1);
}
KBO_ST_FN bool in_front(uint32_t t, uint32_t j, uint32_t k) { return (int64_t)j - (int64_t)(k - 1u) + (int64_t)t < 0; }

KBO_ST_FN bool is_peak(uint32_t here, uint32_t next, uint32_t thr) { return here >= thr && here > next; }
// rightmost i in [0, k - 2] with d(i) >= thr && d(i) > d(i + 1) (variant_calling.rs:73-83), or kNoPeak
template <typename Depth> KBO_ST_FN uint32_t rightmost_peak(const Depth &d, uint32_t k, uint32_t thr)
{
    for (uint32_t i = k - 1u; i-- > 0u;)
        if (is_peak(d(i), d(i + 1u), thr)) return i;
    return kNoPeak;
}

KBO_ST_FN uint32_t site_code(uint32_t csl, uint32_t qpeak, uint32_t rpeak) { return rpeak | (qpeak << 8) | ((csl < 255u ? csl : 255u) << 16); }

// resolve_variant on a site's code (k <= 255): the slices as { q_from | q_len << 8 | r_from << 16 | r_len << 24 }, kNoVariant for
// Err(ResolveVariantErr), kPanic where the reference panics (refine.cpp resolve_variant_peaks is the host's copy)
KBO_ST_FN uint32_t resolve_word(uint32_t code, uint32_t k)
{
    const uint32_t rp = code & 0xFFu, qp = (code >> 8) & 0xFFu, csl = (code >> 16) & 0xFFu;
    if (csl == 0u) return kPanic; // assert!(common_suffix_len > 0)
    if (rp == kNoPeak || qp == kNoPeak) return kNoVariant;
    const int32_t sms = (int32_t)(k - csl);
    const int32_t query_gap = sms - (int32_t)qp - 1, ref_gap = sms - (int32_t)rp - 1;
    if (query_gap > 0 && ref_gap > 0) return (qp + 1u) | ((uint32_t)query_gap << 8) | ((rp + 1u) << 16) | ((uint32_t)ref_gap << 24);
    const int32_t qo = -query_gap, ro = -ref_gap;
    if (qo == ro) return kNoVariant;
    const uint32_t vlen = (uint32_t)(qo > ro ? qo - ro : ro - qo);
    if (qo > ro) // deletion in the query
        return rp + 1u + vlen > k ? kPanic : ((rp + 1u) << 16) | (vlen << 24);
    return qp + 1u + vlen > k ? kPanic : (qp + 1u) | (vlen << 8);
}
KBO_ST_FN bool is_variant(uint32_t word) { return word != kNoVariant && word != kPanic; }
KBO_ST_FN uint32_t word_chars(uint32_t word) { return ((word >> 8) & 0xFFu) + (word >> 24); }

// ---- the order of the variants: two words a site.  hi = (ref, seq, strand - 1) in ref_bits + seq_bits + 1 bits, lo = i << 32 | the
// site's index; the digits that are sorted are lo's bits [32, 32 + i_bits) and hi's low bits
KBO_ST_FN uint32_t bits_for(uint64_t values) // the bits that hold 0 .. values - 1
{
    uint32_t b = 0;
    while (b < 64u && (values - 1u) >> b) b++;
    return values > 1u ? b : 0u;
}
struct KeyShape {
    uint32_t seq_bits, hi_bits, i_bits;
};
KBO_ST_FN KeyShape key_shape(uint64_t n_refs, uint64_t n_seqs, uint64_t total_bases)
{
    KeyShape s;
    s.seq_bits = bits_for(n_seqs);
    s.hi_bits = bits_for(n_refs) + s.seq_bits + 1u;
    s.i_bits = bits_for(total_bases + 1u);
    return s;
}
KBO_ST_FN uint32_t key_passes(const KeyShape &s) { return (s.i_bits + 7u) / 8u + (s.hi_bits + 7u) / 8u; }
KBO_ST_FN uint64_t key_hi(const KeyShape &s, uint32_t ref, uint32_t seq, uint32_t strand)
{
    return ((uint64_t)ref << (s.seq_bits + 1u)) | ((uint64_t)seq << 1) | (strand - 1u);
}
KBO_ST_FN uint64_t key_lo(uint32_t i, uint32_t site) { return ((uint64_t)i << 32) | site; }
// pass p of key_passes(): the digit's first bit counted from the most significant bit of word 0 = hi (word 1 = lo), and its width
KBO_ST_FN void key_pass(const KeyShape &s, uint32_t p, uint32_t &a, uint32_t &nb)
{
    const uint32_t i_passes = (s.i_bits + 7u) / 8u;
    const bool low = p < i_passes;
    const uint32_t field = low ? s.i_bits : s.hi_bits, d = low ? p : p - i_passes;
    const uint32_t from = 8u * d, to = from + 8u < field ? from + 8u : field; // bits [from, to) of the field, from its least significant
    nb = to - from;
    a = (low ? 96u : 64u) - to;
}
// the digit of that pass as the radix passes read it (build_kernels.hip digit_at): no digit spans both words
KBO_ST_FN uint32_t key_digit(uint64_t hi, uint64_t lo, uint32_t a, uint32_t nb)
{
    const uint64_t word = a < 64u ? hi : lo;
    return (uint32_t)(word >> (64u - (a & 63u) - nb)) & ((1u << nb) - 1u);
}

} // namespace refresolve
} // namespace kbo
