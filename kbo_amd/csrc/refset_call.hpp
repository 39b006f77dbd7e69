// refset_call.hpp — the first pass of kbo::call against a set of references (kbo_hip.h "The VARIANTS of a pair"), for
// host and device alike: refset_call_kernels.hip runs it over a slab of (reference, sequence, strand) pairs, refset_calls.cpp restates it on
// the CPU (kbo_call_refset_host), tools/refset_call_check.cpp runs it through accessors that check every index.
//
// A slab holds the matching statistics of its pairs back to back: pair x owns the bytes [off(x), off(x + 1)) and has the threshold
// t = thr(x) of its reference.  Three steps turn them into SITES (pair, i, j, row), the input of resolve_variant:
//   scan    byte p is a CANDIDATE when it is position i >= 1 of a kept pair with d[i] < d[i - 1], d[i - 1] >= t and d[i] < t
//           (variant_calling.rs:269).  A cheap test with the slab's smallest threshold comes first; the pair is found by bisection
//           over the offsets only for bytes that pass it.  A pair is KEPT when kbo_summary_refset has a record for it (has_hit)
//   match   the first j in i + 1 .. min(i + k + 1, len) with d[j] >= t whose interval is one row (:271-273).  The walk keeps no
//           intervals: the interval at j is that of the string seq[j - d[j] + 1 ..= j], d[j] rank steps from the root [0, n), none of
//           which contracts (one_row)
//   spell   the k-mer of that row (access_kmer, :276) by k inverse steps over the packed form: the last character of row x > 0 is the
//           largest c with C[c] <= x (C[c]: the count of entry c of rank block 0), its predecessor the row that holds set bit
//           x - C[c] of c - the last block whose count is <= x by bisection, then a select within its 32 bits.  Row 0 and everything
//           in front of it is '$'.  With it go the k depths that end at j (0xFF in front of the sequence's first base)
// Accessors: Form as refset_step.hpp's (rank), and
//   Slab  uint32_t ms(uint64_t p)     depth at byte p of the slab          uint64_t off(uint32_t x)   first byte of pair x (x <= pairs)
//         uint32_t thr(uint32_t x)    threshold of pair x                  bool kept(uint32_t x)
//   Seq   uint32_t byte(uint32_t s)   byte s of the pair's sequence on its strand
//   Out   void put(uint32_t t, uint32_t v)
#pragma once
#include <stdint.h>

#include "refset_step.hpp"

namespace kbo {
namespace refcall {

constexpr uint32_t kWindow = 64;     // positions j looked at at a time: a wave's lanes
constexpr uint32_t kNoDepth = 0xFFu; // a window byte in front of the sequence's first base

struct Cand { // a candidate: position i of a pair
    uint32_t pair, i;
};
struct Site { // == the four words of a site record
    uint32_t pair, i, j, row;
};

KBO_ST_FN uint32_t window_pad(uint32_t k) { return (k + 15u) / 16u * 16u; }
// a site's window record: [0, k) the depths ending at j, [pad, pad + k) the row's k-mer (call_kernels.hip call_finalize_kernel's layout)
KBO_ST_FN uint32_t window_stride(uint32_t k) { return 2u * window_pad(k); }

KBO_ST_FN bool is_candidate(uint32_t prev, uint32_t cur, uint32_t t) { return cur < prev && prev >= t && cur < t; }

// whether the derandomized depths of `len` noisy ones hold a positive value, which is when translate_ms_vec makes a character other
// than '-' and kbo_summary_refset a record: derandomize_ms_val starts a run at a depth of k or above t and only counts down from one
// otherwise, and the last position starts one only above t (derandomize.rs:221-247, :282)
template <typename Depth> KBO_ST_FN bool has_hit(const Depth &d, uint64_t len, uint32_t k, uint32_t t)
{
    for (uint64_t i = 0; i < len; i++) {
        const uint32_t v = d(i);
        if (v > t || (v == k && i + 1u < len)) return true;
    }
    return false;
}

// the pair that holds byte p: the largest x < pairs with off(x) <= p (pairs >= 1, p < off(pairs))
template <typename Slab> KBO_ST_FN uint32_t pair_of(const Slab &s, uint32_t pairs, uint64_t p)
{
    uint32_t lo = 0, hi = pairs;
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (s.off(mid) <= p) lo = mid;
        else hi = mid;
    }
    return lo;
}

// byte p of a slab of `bytes` bytes: whether it is a candidate, and which
template <typename Slab> KBO_ST_FN bool scan_byte(const Slab &s, uint32_t pairs, uint64_t bytes, uint32_t min_thr, uint64_t p, Cand &c)
{
    if (p < 1u || p >= bytes) return false;
    const uint32_t a = s.ms(p - 1u), b = s.ms(p);
    if (!(b < a && a >= min_thr)) return false;
    const uint32_t x = pair_of(s, pairs, p);
    const uint64_t begin = s.off(x);
    if (p <= begin || !s.kept(x) || !is_candidate(a, b, s.thr(x))) return false; // (i >= 1: p - 1 is the same pair's)
    if (p >= s.off(x + 1u)) return false; // (a slab cut on the device may end in front of `bytes`: a byte behind the last pair is no pair's)
    c.pair = x;
    c.i = (uint32_t)(p - begin);
    return true;
}

// whether the d bases that end at position j of the sequence have exactly one row in a form of n rows, and which
template <typename Form, typename Seq> KBO_ST_FN bool one_row(const Form &x, uint32_t n, const Seq &q, uint32_t j, uint32_t d, uint32_t &row)
{
    if (d == 0u || d > j + 1u) return false;
    uint32_t l = 0, r = n;
    for (uint32_t s = j + 1u - d; s <= j; s++) {
        const uint32_t c = refstep::base_code(q.byte(s));
        if (c > 3u) return false;
        l = refstep::rank_of(x, c, l);
        r = refstep::rank_of(x, c, r);
        if (l >= r) return false;
    }
    row = l;
    return r - l == 1u;
}

// one past the last j a candidate at i looks at
KBO_ST_FN uint32_t match_end(uint32_t i, uint32_t k, uint64_t len)
{
    const uint64_t e = (uint64_t)i + k + 1u;
    return (uint32_t)(e < len ? e : len);
}

// the match of the candidate at i of a pair of `len` bytes at `begin`, one j after the other
template <typename Slab, typename Form, typename Seq>
KBO_ST_FN bool match_serial(const Slab &s, const Form &x, uint32_t n, const Seq &q, uint64_t begin, uint64_t len, uint32_t k, uint32_t t, uint32_t i,
                            uint32_t &j_out, uint32_t &row)
{
    for (uint32_t j = i + 1u, e = match_end(i, k, len); j < e; j++) {
        const uint32_t d = s.ms(begin + j);
        if (d >= t && one_row(x, n, q, j, d, row)) {
            j_out = j;
            return true;
        }
    }
    return false;
}

// the last of nb rank blocks whose count of c is <= target (the count of block 0 is)
template <typename Form> KBO_ST_FN uint32_t block_of(const Form &x, uint32_t nb, uint32_t c, uint32_t target)
{
    uint32_t lo = 0, hi = nb;
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (x.rank(mid, c).count <= target) lo = mid;
        else hi = mid;
    }
    return lo;
}

// the k characters of row `row` (row < n) of a form of n rows -> out[0, k)
template <typename Form, typename Out> KBO_ST_FN void spell_row(const Form &x, uint32_t n, uint32_t k, uint32_t row, Out &out)
{
    const uint32_t nb = n / 32u + 1u;
    uint32_t C[4];
    for (uint32_t c = 0; c < 4u; c++) C[c] = x.rank(0u, c).count;
    uint32_t i = row;
    for (uint32_t t = k; t-- > 0u;) {
        if (i < C[0] || i == 0u) { // the root: everything to the left is '$'
            i = 0u;
            out.put(t, (uint32_t)'$');
            continue;
        }
        uint32_t c = 3u;
        while (c > 0u && C[c] > i) c--;
        out.put(t, (0x54474341u >> (8u * c)) & 0xFFu);
        const uint32_t b = block_of(x, nb, c, i);
        const refstep::Entry e = x.rank(b, c);
        uint32_t bits = e.bits;
        for (uint32_t skip = i - e.count; skip > 0u && bits; skip--) bits &= bits - 1u;
        i = bits ? b * 32u + (uint32_t)__builtin_ctz(bits) : 0u; // (no such bit: not a form the builder makes)
    }
}

// the k depths of a pair at `begin` that end at its position j -> out[0, k)
template <typename Slab, typename Out> KBO_ST_FN void gather_depths(const Slab &s, uint64_t begin, uint32_t j, uint32_t k, Out &out)
{
    for (uint32_t t = 0; t < k; t++) {
        const int64_t pos = (int64_t)j - (int64_t)(k - 1u) + (int64_t)t;
        out.put(t, pos >= 0 ? s.ms(begin + (uint64_t)pos) : kNoDepth);
    }
}

} // namespace refcall
} // namespace kbo
