// refset_resolve_kernels.hip — gfx950 (MI355X, CDNA4): the second pass of kbo::call for the device-resident reference-set calls
// (kbo_call_refset_dev, kbo_call_refset_screened_dev).  refset_resolve.hpp has the index word, the probe, the three
// values, the resolve word and the keys; this is their mapping onto lanes and waves.
//
// per slab, behind launch_refset_call
//   site_pairs   a lane per pair: its reference, where its sequence begins in the walk's buffer, its sequence and strand - from the
//                slab's plan (the unscreened form) or from the candidate list (the screened form); the one kernel the forms do not share
//   append       a lane per site of the slab: a wave takes its slots in the call's list with one atomic add on the call's site
//                count and writes the tag and the window of every site whose slot is in front of max_sites
// per call, behind the last slab
//   index        a lane per base of the '+' batch: its word; four radix passes (build_kernels.hip) sort the words by code, those
//                that are no occurrence behind all others
//   sites        a wave per site: the row's k-mer, the query-side depths and the two k-mers' last difference from the window, a lane
//                per position of the k-mer probing the index, the peaks by ballots, the resolve word by lane 0
//   keys, sort   a lane per slot of the list: two key words (all ones behind the sites), radix passes over the bits that can differ
//   counts       a lane per place of the order: a variant or none, its characters; two scans
//   write        a lane per place: the record and its characters, within the two capacities; lane 0 the totals
// Integer and byte work only: no MFMA.  Plain vector stores; the atomics are the adds on the site count and the panic count.  Every
// index is below a bound the kernel reads itself: a site's slot below max_sites, a probe's position inside the site's own sequence,
// a word of the index below `total`.
#include "device_util.hpp"
#include "refset_call.hpp"
#include "refset_cand.hpp"
#include "refset_resolve.hpp"

#include <algorithm>

namespace kbo {
namespace {

using namespace refresolve;

constexpr uint32_t kThreads = 256, kWaves = kThreads / 64u, kMaxK = 256;

struct DevSeq {
    const uint8_t *p_;
    __device__ __forceinline__ uint32_t byte(uint64_t x) const { return p_[x]; }
};
struct DevIndex {
    const uint64_t *w_;
    __device__ __forceinline__ uint64_t word(uint64_t x) const { return w_[x]; }
};
struct LdsKmer {
    const uint8_t *p_;
    __device__ __forceinline__ uint32_t byte(uint32_t t) const { return p_[t]; }
};

__device__ __forceinline__ uint32_t n_listed(const RefsetResolveArgs &a)
{
    const uint64_t have = a.stats[2];
    return have < a.max_sites ? (uint32_t)have : a.max_sites;
}
__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
}

__global__ __launch_bounds__(kThreads) void site_pairs_plan_kernel(RefsetPlan a, uint32_t first_q, uint32_t n_pairs, RefsetSitePairs out)
{
    const uint32_t p = blockIdx.x * kThreads + threadIdx.x;
    if (p >= n_pairs) return;
    const refplan::Pair pr = refplan::pair_of(a.g, p);
    const uint32_t strand = refplan::strand_of(a.g, pr.x);
    out.pref[p] = a.qref[first_q + pr.j];
    out.pq[p] = (uint32_t)((strand == 2u ? a.g.rev_base : 0u) + a.off[pr.s]);
    out.pseq[p] = pr.s << 1 | (strand - 1u);
}

__global__ __launch_bounds__(kThreads) void site_pairs_cand_kernel(RefsetCandArgs a, RefsetSitePairs out)
{
    const uint32_t p = blockIdx.x * kThreads + threadIdx.x;
    if (p >= a.max_pairs) return;
    uint32_t ref = a.safe_ref, pq = 0, pseq = 0; // (a pair behind the walked ones is empty: nothing reads its words)
    if (p < a.hdr[1]) {
        const refcand::PairId id = refcand::pair_of_bit(a.list[p], a.n_seqs);
        ref = id.ref;
        pq = (uint32_t)((id.strand == 2u ? a.rev_off : 0u) + a.off[id.seq]);
        pseq = id.seq << 1 | (id.strand - 1u);
    }
    out.pref[p] = ref;
    out.pq[p] = pq;
    out.pseq[p] = pseq;
}

__global__ __launch_bounds__(kThreads) void sites_append_kernel(RefsetCallArgs s, RefsetSitePairs pairs, RefsetResolveArgs a)
{
    const uint32_t cands = s.counts[0], found = s.counts[16], n = found < s.cap ? found : s.cap;
    const uint32_t stride = refcall::window_stride(a.k), lane = threadIdx.x & 63u;
    unsigned long long *total = reinterpret_cast<unsigned long long *>(a.stats + 2);
    // (whole waves take a turn: the ballot below is over all of a wave's lanes)
    for (uint64_t x0 = (uint64_t)blockIdx.x * kThreads + (threadIdx.x & ~63u); x0 < n; x0 += (uint64_t)gridDim.x * kThreads) {
        const uint64_t x = x0 + lane;
        const bool mine = x < n;
        const uint64_t mk = __ballot(mine);
        unsigned long long base = 0;
        if (lane == 0u) base = atomicAdd(total, (unsigned long long)__popcll(mk));
        base = __shfl(base, 0);
        const uint64_t slot = base + lane; // (the wave's sites are its first lanes)
        if (mine && slot < a.max_sites) {
            const uint4 site = s.sites[x];
            const uint32_t pair = site.x < s.n_pairs ? site.x : 0u, ps = pairs.pseq[pair];
            uint4 *tag = reinterpret_cast<uint4 *>(a.tags + slot * kRefsetSiteTagWords);
            tag[0] = make_uint4(pairs.pref[pair], ps >> 1, (ps & 1u) + 1u, s.pthr[pair]);
            tag[1] = make_uint4(site.y, site.z, pairs.pq[pair], 0u);
            const uint4 *src = reinterpret_cast<const uint4 *>(s.win + x * stride);
            uint4 *dst = reinterpret_cast<uint4 *>(a.wins + slot * stride);
            for (uint32_t t = 0; t < stride / 16u; t++) dst[t] = src[t];
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0 && a.stats[3] < cands) a.stats[3] = cands; // (slabs follow each other on the stream)
}

__global__ __launch_bounds__(kThreads) void resolve_index_kernel(RefsetResolveArgs a)
{
    const uint64_t p = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (p >= a.total) return;
    uint32_t lo = 0, hi = a.n_seqs; // the sequence that holds base p: the largest s with off[s] <= p
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (a.off[mid] <= p) lo = mid;
        else hi = mid;
    }
    a.ix[0][p] = index_word(DevSeq{a.concat}, a.off[lo], a.off[lo + 1u], p, a.k, a.qlen);
}

// rightmost peak of v[0, k) (LDS), one wave
__device__ __forceinline__ uint32_t wave_peak(const uint8_t *v, uint32_t k, uint32_t thr, uint32_t lane)
{
    for (int32_t base = (int32_t)((k - 2u) & ~63u); base >= 0; base -= 64) {
        const uint32_t i = (uint32_t)base + lane;
        const uint64_t m = __ballot(i + 1u < k && is_peak(v[i], v[i + 1u], thr));
        if (m) return (uint32_t)base + 63u - (uint32_t)__builtin_clzll(m);
    }
    return kNoPeak;
}

__global__ __launch_bounds__(kThreads) void resolve_sites_kernel(RefsetResolveArgs a, const uint64_t *__restrict__ ix)
{
    __shared__ uint8_t lds[kWaves][3 * kMaxK];
    const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t n = n_listed(a), k = a.k, pad = refcall::window_pad(k), stride = refcall::window_stride(k);
    uint8_t *rk = lds[wv], *dq = rk + kMaxK, *dr = dq + kMaxK;
    for (uint32_t x = blockIdx.x * kWaves + wv; x < n; x += gridDim.x * kWaves) {
        const uint4 *tag = reinterpret_cast<const uint4 *>(a.tags + (uint64_t)x * kRefsetSiteTagWords);
        const uint4 t0 = tag[0], t1 = tag[1]; // { ref, seq, strand, thr }, { i, j, pq, 0 }
        const uint32_t seq = t0.y < a.n_seqs ? t0.y : 0u, thr = t0.w, j = t1.y;
        const uint8_t *w = a.wins + (uint64_t)x * stride, *qs = a.q + t1.z;
        const uint64_t begin = a.off[seq], end = a.off[seq + 1u];
        uint32_t hi_diff = 0xFFFFFFFFu; // the rightmost position where the two k-mers differ
        for (uint32_t u0 = 0; u0 < k; u0 += 64u) {
            const uint32_t u = u0 + lane;
            bool differ = false;
            if (u < k) {
                const uint32_t ch = w[pad + u];
                rk[u] = (uint8_t)ch;
                dr[u] = (uint8_t)query_depth(w[u], u, j, k);
                const uint32_t qc = in_front(u, j, k) ? (uint32_t)'$' : (uint32_t)qs[(uint64_t)j + u - (k - 1u)];
                differ = qc != ch;
            }
            const uint64_t m = __ballot(differ);
            if (m) hi_diff = u0 + 63u - (uint32_t)__builtin_clzll(m);
        }
        wave_sync();
        const uint32_t mode = probe_mode(t0.z, a.add_revcomp != 0u);
        for (uint32_t u0 = 0; u0 < k; u0 += 64u) {
            const uint32_t u = u0 + lane;
            if (u < k) dq[u] = (uint8_t)depth_at(LdsKmer{rk}, u, a.qlen, mode, DevSeq{a.concat}, begin, end, DevIndex{ix}, a.total);
        }
        wave_sync();
        const uint32_t rpeak = wave_peak(dq, k, thr, lane), qpeak = wave_peak(dr, k, thr, lane);
        if (lane == 0u) {
            const uint32_t word = resolve_word(site_code(hi_diff == 0xFFFFFFFFu ? k : k - 1u - hi_diff, qpeak, rpeak), k);
            a.words[x] = word;
            if (word == kPanic) atomicAdd(reinterpret_cast<unsigned long long *>(a.stats + 4), 1ull);
        }
        wave_sync(); // (the next site's k-mer goes where this one's is)
    }
}

__global__ __launch_bounds__(kThreads) void resolve_keys_kernel(RefsetResolveArgs a)
{
    const uint32_t x = blockIdx.x * kThreads + threadIdx.x;
    if (x >= a.max_sites) return;
    uint64_t hi = ~0ull, lo = ~0ull;
    if (x < n_listed(a)) {
        const uint4 *tag = reinterpret_cast<const uint4 *>(a.tags + (uint64_t)x * kRefsetSiteTagWords);
        const uint4 t0 = tag[0];
        hi = key_hi(KeyShape{a.key_seq_bits, a.key_hi_bits, a.key_i_bits}, t0.x, t0.y, t0.z);
        lo = key_lo(tag[1].x, x);
    }
    a.keys[0][x] = hi;
    a.keys[0][(uint64_t)a.max_sites + x] = lo;
}

__device__ __forceinline__ uint32_t scanned(const uint32_t *data, const uint32_t *sums, uint32_t i) { return sums[i / kScanBlock] + data[i]; }

// place p of the order holds the site whose index is the low word of the p-th sorted key
__global__ __launch_bounds__(kThreads) void resolve_counts_kernel(RefsetResolveArgs a, const uint64_t *__restrict__ sorted)
{
    const uint32_t p = blockIdx.x * kThreads + threadIdx.x;
    if (p > a.max_sites) return;
    uint32_t v = 0, c = 0;
    if (p < n_listed(a)) {
        const uint32_t x = (uint32_t)sorted[(uint64_t)a.max_sites + p];
        const uint32_t word = x < a.max_sites ? a.words[x] : kNoVariant;
        if (is_variant(word)) {
            v = 1u;
            c = word_chars(word);
        }
    }
    a.vcnt[p] = v;
    a.ccnt[p] = c;
}

__global__ __launch_bounds__(kThreads) void resolve_write_kernel(RefsetResolveArgs a, const uint64_t *__restrict__ sorted)
{
    const uint32_t p = blockIdx.x * kThreads + threadIdx.x;
    if (p == 0u) {
        a.stats[0] = scanned(a.vcnt, a.vsums, a.max_sites);
        a.stats[1] = scanned(a.ccnt, a.csums, a.max_sites);
    }
    if (p >= n_listed(a)) return;
    const uint32_t x = (uint32_t)sorted[(uint64_t)a.max_sites + p];
    if (x >= a.max_sites) return;
    const uint32_t word = a.words[x];
    if (!is_variant(word)) return;
    const uint32_t v = scanned(a.vcnt, a.vsums, p), c = scanned(a.ccnt, a.csums, p);
    const uint4 *tag = reinterpret_cast<const uint4 *>(a.tags + (uint64_t)x * kRefsetSiteTagWords);
    const uint4 t0 = tag[0], t1 = tag[1];
    const uint32_t qf = word & 0xFFu, ql = (word >> 8) & 0xFFu, rf = (word >> 16) & 0xFFu, rl = word >> 24;
    if (v < a.max_variants) {
        uint32_t *rec = a.variants + (uint64_t)v * 6u;
        rec[0] = t0.x;
        rec[1] = t0.y;
        rec[2] = t0.z;
        rec[3] = t1.x;
        rec[4] = c;
        rec[5] = ql | (rl << 16);
    }
    if ((uint64_t)c + ql + rl > a.max_chars) return;
    // the query-side k-mer: the k characters of the sequence on its strand that end at j, '$' in front of it; the row's from the window
    const uint8_t *qs = a.q + t1.z, *rk = a.wins + (uint64_t)x * refcall::window_stride(a.k) + refcall::window_pad(a.k);
    uint8_t *o = a.chars + c;
    for (uint32_t t = 0; t < ql; t++) o[t] = in_front(qf + t, t1.y, a.k) ? (uint8_t)'$' : qs[(uint64_t)t1.y + qf + t - (a.k - 1u)];
    for (uint32_t t = 0; t < rl; t++) o[ql + t] = rk[rf + t];
}

dim3 blocks_for(uint64_t n) { return dim3((uint32_t)std::max<uint64_t>((n + kThreads - 1u) / kThreads, 1u)); }

} // namespace

hipError_t launch_refset_site_pairs_plan(const RefsetPlan &a, uint32_t first_q, uint32_t n_pairs, const RefsetSitePairs &out, hipStream_t stream)
{
    hipLaunchKernelGGL(site_pairs_plan_kernel, blocks_for(n_pairs), dim3(kThreads), 0, stream, a, first_q, n_pairs, out);
    return hipGetLastError();
}

hipError_t launch_refset_site_pairs_cand(const RefsetCandArgs &a, const RefsetSitePairs &out, hipStream_t stream)
{
    hipLaunchKernelGGL(site_pairs_cand_kernel, blocks_for(a.max_pairs), dim3(kThreads), 0, stream, a, out);
    return hipGetLastError();
}

hipError_t launch_refset_sites_append(const RefsetCallArgs &slab, const RefsetSitePairs &pairs, const RefsetResolveArgs &a, hipStream_t stream)
{
    if (slab.cap == 0 || a.max_sites == 0 || a.k < 2u || a.k >= kMaxK) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sites_append_kernel, dim3(std::min<uint32_t>(blocks_for(slab.cap).x, 1024u)), dim3(kThreads), 0, stream, slab, pairs, a);
    return hipGetLastError();
}

hipError_t launch_refset_resolve(const RefsetResolveArgs &a, hipStream_t stream)
{
    if (a.max_sites == 0 || a.total == 0 || a.n_seqs == 0 || a.k < 2u || a.k >= kMaxK || a.qlen < 1u || a.qlen > kQMax) return hipErrorInvalidValue;
    hipLaunchKernelGGL(resolve_index_kernel, blocks_for(a.total), dim3(kThreads), 0, stream, a);
    uint32_t at = 0;
    for (uint32_t p = 0; p < 4u; p++, at ^= 1u) { // the 25 bits of the code field, eight at a time from the least significant
        const RadixPass ps{p < 3u ? 24u - 8u * p : 32u - kCodeBits, p < 3u ? 8u : kCodeBits - 24u, 0u};
        const hipError_t e = launch_build_radix_pass(a.ix[at], a.ix[at ^ 1u], 1u, a.total, nullptr, nullptr, a.total, ps, a.hist, a.sums, stream);
        if (e != hipSuccess) return e;
    }
    const uint32_t site_blocks = std::min<uint32_t>((a.max_sites + kWaves - 1u) / kWaves, 4096u);
    hipLaunchKernelGGL(resolve_sites_kernel, dim3(site_blocks), dim3(kThreads), 0, stream, a, a.ix[at]);
    hipLaunchKernelGGL(resolve_keys_kernel, blocks_for(a.max_sites), dim3(kThreads), 0, stream, a);
    const KeyShape shape{a.key_seq_bits, a.key_hi_bits, a.key_i_bits};
    uint32_t kat = 0;
    for (uint32_t p = 0; p < key_passes(shape); p++, kat ^= 1u) {
        RadixPass ps{0u, 0u, 0u};
        key_pass(shape, p, ps.a, ps.nb);
        const hipError_t e =
            launch_build_radix_pass(a.keys[kat], a.keys[kat ^ 1u], 2u, a.max_sites, nullptr, nullptr, a.max_sites, ps, a.hist, a.sums, stream);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(resolve_counts_kernel, blocks_for((uint64_t)a.max_sites + 1u), dim3(kThreads), 0, stream, a, a.keys[kat]);
    hipError_t e = launch_scan(a.vcnt, a.max_sites + 1u, a.vsums, stream);
    if (e != hipSuccess) return e;
    e = launch_scan(a.ccnt, a.max_sites + 1u, a.csums, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(resolve_write_kernel, blocks_for(a.max_sites), dim3(kThreads), 0, stream, a, a.keys[kat]);
    return hipGetLastError();
}

} // namespace kbo
