// indel_kernels.hip — insertion and deletion events from the segments of a walked batch, and the events of any number of batches
// counted into sites (kbo_hip.h "Indels"; the arithmetic: index_indel.hpp).
//   event_count_kernel   a workgroup per chunk of kScanChunk records: a lane evaluates the pairs (x - 1, x) of its kPer records - the
//                        rule, the bisections, an insertion's bytes - and the events are counted
//   event_sums_kernel    ONE workgroup: the counts' exclusive scan in place; the list's count before the call is kept in d_work and
//                        *n_events grows by the total
//   event_emit_kernel    the same chunks behind that scan: the n-th event of the call is written at base + n when that is below capacity
//   key_kernel           a lane per place of the list: the sort key of event i < min(*n_events, capacity) that holds an event, else
//                        (and for the places up to event_capacity) the pad key of all ones
//   (the sort)           launch_build_radix_pass over the key bits a pos <= source_bases, kind_len and code can set: stable, LSD
//   head_count_kernel    per chunk of kScanChunk places: heads (a key that differs from the one in front) and MINUS bits, summed in ONE
//                        64-bit word, heads low
//   sums64_kernel        ONE workgroup: those sums' exclusive scan, the number of groups to d_work
//   head_apply_kernel    every head writes (its place, the MINUS bits in front of it) at its group's number, the first place that holds
//                        no key (or event_capacity) the same at the number of groups: count and n_minus are differences at the next head
//   site_count_kernel    per chunk of kScanChunk groups: the threshold, counted
//   site_sums_kernel     ONE workgroup: the counts' exclusive scan, the total to *n_sites
//   site_emit_kernel     the n-th site writes record n when n < capacity
// No pass waits for another workgroup of its own launch.  Every count is read on the device; every grid is sized by a capacity.
#include "device_util.hpp"
#include "index_indel.hpp"

namespace kbo {
namespace {

using namespace idxindel;
constexpr uint32_t kWave = 64, kWaves = kThreads / kWave;

struct DevOff {
    const uint64_t *p;
    __device__ uint64_t off(size_t s) const { return p[s]; }
};
struct DevBytes {
    const uint8_t *p;
    __device__ uint32_t at(uint64_t i) const { return p[i]; }
};

// the inclusive scan of v over the workgroup's kThreads lanes (sh: kThreads values); every lane calls it
template <typename T> __device__ __forceinline__ T block_incl_scan(T v, T *sh)
{
    const uint32_t t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (uint32_t step = 1; step < kThreads; step <<= 1) {
        const T x = t >= step ? sh[t - step] : (T)0;
        __syncthreads();
        sh[t] += x;
        __syncthreads();
    }
    const T r = sh[t];
    __syncthreads();
    return r;
}
// ONE workgroup: the exclusive scan of sums[0, n_chunks) in place; returns the total (to every lane)
template <typename T> __device__ __forceinline__ T sums_scan(T *__restrict__ sums, uint64_t n_chunks, T *sh)
{
    const uint32_t t = threadIdx.x;
    T run = 0;
    for (uint64_t c0 = 0; c0 < n_chunks; c0 += kThreads) {
        const uint64_t c = c0 + t;
        const T v = c < n_chunks ? sums[c] : (T)0;
        const T incl = block_incl_scan(v, sh);
        if (c < n_chunks) sums[c] = run + incl - v;
        __syncthreads();
        sh[t] = incl;
        __syncthreads();
        run += sh[kThreads - 1u];
        __syncthreads();
    }
    return run;
}

// ---- events
struct EArgs {
    const uint32_t *segs; // records of 7 words
    const uint64_t *n_segs;
    const uint8_t *concat;
    const uint64_t *off, *src_off;
    uint32_t *sums;
    uint64_t *base;       // d_work: the list's count before the call
    uint4 *events;
    uint64_t *n_events;
    uint64_t capacity, total, source_bases, event_capacity;
    uint32_t n_seqs, n_src, k, skip_multi, max_indel;
};
__device__ __forceinline__ Segment load_record(const uint32_t *segs, uint64_t x)
{
    const uint32_t *p = segs + x * 7u;
    return Segment{p[0], p[1], p[2], p[3], p[4], p[5], p[6]};
}
// the pair that ends at record x, 1 <= x < the records of the call: its event, or none
__device__ __forceinline__ bool pair_at(const EArgs &a, uint64_t x, Event *e)
{
    return pair_whole(load_record(a.segs, x - 1u), load_record(a.segs, x), DevOff{a.off}, a.n_seqs, a.total, a.k, a.skip_multi != 0u, a.max_indel,
                      a.source_bases, DevOff{a.src_off}, a.n_src, DevBytes{a.concat}, e) == kEvent;
}
// the events among the pairs that end at the kPer records of this lane, a bit each
__device__ __forceinline__ uint32_t lane_events(const EArgs &a, uint64_t at)
{
    const uint64_t n_all = *a.n_segs, n = n_all < a.capacity ? n_all : a.capacity;
    uint32_t f = 0;
    for (uint32_t u = 0; u < kPer; u++) {
        const uint64_t x = at + u;
        Event e;
        if (x >= 1u && x < n && pair_at(a, x, &e)) f |= 1u << u;
    }
    return f;
}

__global__ void __launch_bounds__(kThreads) event_count_kernel(EArgs a)
{
    __shared__ uint32_t sh[kWaves];
    const uint32_t t = threadIdx.x;
    const uint32_t mine = wave_sum((uint32_t)__popc(lane_events(a, (uint64_t)blockIdx.x * kScanChunk + (uint64_t)t * kPer)));
    if ((t & (kWave - 1u)) == 0) sh[t / kWave] = mine;
    __syncthreads();
    if (t == 0) {
        uint32_t v = 0;
        for (uint32_t w = 0; w < kWaves; w++) v += sh[w];
        a.sums[blockIdx.x] = v;
    }
}

__global__ void __launch_bounds__(kThreads) event_sums_kernel(uint32_t *__restrict__ sums, uint64_t n_chunks, uint64_t *__restrict__ base,
                                                              uint64_t *__restrict__ n_events)
{
    __shared__ uint32_t sh[kThreads];
    const uint32_t total = sums_scan(sums, n_chunks, sh);
    if (threadIdx.x == 0) {
        const uint64_t before = *n_events;
        *base = before;
        *n_events = before + total;
    }
}

__global__ void __launch_bounds__(kThreads) event_emit_kernel(EArgs a)
{
    __shared__ uint32_t sh[kThreads];
    const uint32_t t = threadIdx.x;
    const uint64_t at = (uint64_t)blockIdx.x * kScanChunk + (uint64_t)t * kPer;
    const uint32_t f = lane_events(a, at), mine = (uint32_t)__popc(f);
    const uint32_t incl = block_incl_scan(mine, sh);
    uint64_t x = *a.base + a.sums[blockIdx.x] + (incl - mine);
    for (uint32_t u = 0; u < kPer; u++) { // (few lanes hold an event: the pair is evaluated again where one is written)
        if (!(f >> u & 1u)) continue;
        Event e;
        if (x < a.event_capacity && pair_at(a, at + u, &e)) a.events[x] = make_uint4(e.pos, e.kind_len, e.code, e.flags);
        x++;
    }
}

// ---- sites
struct SArgs {
    const uint4 *events;
    const uint64_t *n_events;
    const uint32_t *depth;
    const uint64_t *src_off;
    uint64_t *keys;      // the sorted keys: word j of key i at keys[j * n + i]
    uint2 *grp;          // n + 1
    uint64_t *hsums;
    uint32_t *ssums;
    uint64_t *n_groups;
    uint4 *sites;
    uint64_t *n_sites;
    uint64_t n, source_bases, capacity; // n: event_capacity
    uint32_t n_src;
    Thresholds t;
};

__global__ void __launch_bounds__(kThreads) key_kernel(SArgs a, uint64_t *__restrict__ keys)
{
    const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= a.n) return;
    uint64_t w0 = kPadKey, w1 = kPadKey;
    if (i < *a.n_events) {
        const uint4 e = a.events[i];
        uint64_t k0, k1;
        if (event_key(Event{e.x, e.y, e.z, e.w}, a.source_bases, &k0, &k1)) {
            w0 = k0;
            w1 = k1;
        }
    }
    keys[i] = w0;
    keys[a.n + i] = w1;
}

// heads (low word) and MINUS bits (high word) among the kPer places of this lane; i in [0, n]: place n holds no key
__device__ __forceinline__ bool place_valid(const SArgs &a, uint64_t i) { return i < a.n && key_valid(a.keys[i]); }
__device__ __forceinline__ bool place_head(const SArgs &a, uint64_t i)
{
    if (i == 0) return true;
    return !same_group(a.keys[i - 1u], a.keys[a.n + i - 1u], a.keys[i], a.keys[a.n + i]);
}
__device__ __forceinline__ uint64_t lane_heads(const SArgs &a, uint64_t at, uint32_t *heads)
{
    uint64_t v = 0;
    uint32_t f = 0;
    for (uint32_t u = 0; u < kPer; u++) {
        const uint64_t i = at + u;
        if (!place_valid(a, i)) break; // (the keys that hold an event are a prefix of the sorted places)
        if (place_head(a, i)) {
            f |= 1u << u;
            v += 1u;
        }
        v += (uint64_t)key_minus(a.keys[a.n + i]) << 32;
    }
    *heads = f;
    return v;
}

__global__ void __launch_bounds__(kThreads) head_count_kernel(SArgs a)
{
    __shared__ uint64_t sh[kThreads];
    uint32_t f;
    const uint64_t v = lane_heads(a, (uint64_t)blockIdx.x * kScanChunk + (uint64_t)threadIdx.x * kPer, &f);
    const uint64_t incl = block_incl_scan(v, sh);
    if (threadIdx.x == kThreads - 1u) a.hsums[blockIdx.x] = incl;
}

__global__ void __launch_bounds__(kThreads) sums64_kernel(uint64_t *__restrict__ sums, uint64_t n_chunks, uint64_t *__restrict__ n_groups)
{
    __shared__ uint64_t sh[kThreads];
    const uint64_t total = sums_scan(sums, n_chunks, sh);
    if (threadIdx.x == 0) *n_groups = total & 0xFFFFFFFFull;
}

__global__ void __launch_bounds__(kThreads) head_apply_kernel(SArgs a)
{
    __shared__ uint64_t sh[kThreads];
    const uint64_t at = (uint64_t)blockIdx.x * kScanChunk + (uint64_t)threadIdx.x * kPer;
    uint32_t f;
    const uint64_t v = lane_heads(a, at, &f);
    const uint64_t incl = block_incl_scan(v, sh);
    uint64_t run = a.hsums[blockIdx.x] + incl - v; // heads and MINUS bits in front of this lane's places
    for (uint32_t u = 0; u < kPer; u++) {
        const uint64_t i = at + u;
        if (i > a.n) break;
        const bool valid = place_valid(a, i);
        // a head, or the end: the first place without a key
        if (valid ? (f >> u & 1u) != 0u : (i == 0 || place_valid(a, i - 1u))) a.grp[(uint32_t)run] = make_uint2((uint32_t)i, (uint32_t)(run >> 32));
        if (!valid) break;
        run += (f >> u & 1u) + ((uint64_t)key_minus(a.keys[a.n + i]) << 32);
    }
}

// group g < *n_groups as a site, or not
__device__ __forceinline__ bool group_site(const SArgs &a, uint64_t g, Site *s)
{
    if (g >= *a.n_groups) return false;
    const uint2 h = a.grp[g], next = a.grp[g + 1u];
    const uint64_t w0 = a.keys[h.x], w1 = a.keys[a.n + h.x];
    const uint32_t pos = (uint32_t)(w0 >> 32), count = next.x - h.x;
    const uint32_t d = a.source_bases ? a.depth[depth_at(pos)] : 0u; // (event_key: pos <= source_bases)
    if (!calls(count, d, a.t)) return false;
    *s = site_of(w0, w1, seq_of(DevOff{a.src_off}, a.n_src, pos), count, next.y - h.y, d);
    return true;
}
__device__ __forceinline__ uint32_t lane_sites(const SArgs &a, uint64_t at)
{
    uint32_t f = 0;
    for (uint32_t u = 0; u < kPer; u++) {
        Site s;
        if (group_site(a, at + u, &s)) f |= 1u << u;
    }
    return f;
}

__global__ void __launch_bounds__(kThreads) site_count_kernel(SArgs a)
{
    __shared__ uint32_t sh[kThreads];
    const uint32_t mine = (uint32_t)__popc(lane_sites(a, (uint64_t)blockIdx.x * kScanChunk + (uint64_t)threadIdx.x * kPer));
    const uint32_t incl = block_incl_scan(mine, sh);
    if (threadIdx.x == kThreads - 1u) a.ssums[blockIdx.x] = incl;
}

__global__ void __launch_bounds__(kThreads) site_sums_kernel(uint32_t *__restrict__ sums, uint64_t n_chunks, uint64_t *__restrict__ n_sites)
{
    __shared__ uint32_t sh[kThreads];
    const uint32_t total = sums_scan(sums, n_chunks, sh);
    if (threadIdx.x == 0) *n_sites = total;
}

__global__ void __launch_bounds__(kThreads) site_emit_kernel(SArgs a)
{
    __shared__ uint32_t sh[kThreads];
    const uint64_t at = (uint64_t)blockIdx.x * kScanChunk + (uint64_t)threadIdx.x * kPer;
    const uint32_t f = lane_sites(a, at), mine = (uint32_t)__popc(f);
    const uint32_t incl = block_incl_scan(mine, sh);
    uint64_t x = (uint64_t)a.ssums[blockIdx.x] + (incl - mine);
    for (uint32_t u = 0; u < kPer; u++) {
        if (!(f >> u & 1u)) continue;
        Site s;
        if (x < a.capacity && group_site(a, at + u, &s)) {
            a.sites[2u * x] = make_uint4(s.pos, s.source, s.kind_len, s.code);
            a.sites[2u * x + 1u] = make_uint4(s.count, s.n_minus, s.depth, 0u);
        }
        x++;
    }
}

} // namespace

hipError_t launch_indel_events(const IndelEventArgs &x, hipStream_t stream)
{
    if (x.n_seqs == 0 || x.n_seqs >= kMaxSeqs || x.capacity > kMaxSegs || x.event_capacity > kMaxEvents || x.k == 0 || x.n_src == 0 ||
        x.max_indel == 0 || x.total + 16u > (1ull << 32))
        return hipErrorInvalidValue;
    const EventWork w = event_work(x.capacity);
    EArgs a;
    a.segs = x.segs;
    a.n_segs = x.n_segs;
    a.concat = x.concat;
    a.off = x.off;
    a.src_off = x.src_off;
    a.sums = static_cast<uint32_t *>(x.work);
    a.base = reinterpret_cast<uint64_t *>(static_cast<uint8_t *>(x.work) + w.base_off);
    a.events = static_cast<uint4 *>(x.events);
    a.n_events = x.n_events;
    a.capacity = x.capacity;
    a.total = x.total;
    a.source_bases = x.source_bases;
    a.event_capacity = x.event_capacity;
    a.n_seqs = x.n_seqs;
    a.n_src = x.n_src;
    a.k = x.k;
    a.skip_multi = x.skip_multi ? 1u : 0u;
    a.max_indel = x.max_indel;
    const uint32_t chunks = (uint32_t)scan_chunks(x.capacity);
    if (!chunks) return hipSuccess; // (no record, no event: *n_events stays)
    hipLaunchKernelGGL(event_count_kernel, dim3(chunks), dim3(kThreads), 0, stream, a);
    hipLaunchKernelGGL(event_sums_kernel, dim3(1), dim3(kThreads), 0, stream, a.sums, (uint64_t)chunks, a.base, a.n_events);
    hipLaunchKernelGGL(event_emit_kernel, dim3(chunks), dim3(kThreads), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_indel_sites(const IndelSitesArgs &x, hipStream_t stream)
{
    if (x.n_src == 0 || x.min_count == 0 || x.frac_den == 0 || x.source_bases >= idxlocate::kMaxSourceBases || x.event_capacity > kMaxEvents)
        return hipErrorInvalidValue;
    static_assert(kRadixTile == kBuildTile && kRadixSumBlock == kScanBlock, "site_work()'s figures are the radix pass's");
    const uint64_t n = x.event_capacity;
    const SiteWork w = site_work(n);
    uint8_t *wk = static_cast<uint8_t *>(x.work);
    uint64_t *ka = reinterpret_cast<uint64_t *>(wk), *kb = reinterpret_cast<uint64_t *>(wk + w.keys_b_off);
    SArgs a;
    a.events = static_cast<const uint4 *>(x.events);
    a.n_events = x.n_events;
    a.depth = x.depth;
    a.src_off = x.src_off;
    a.grp = reinterpret_cast<uint2 *>(wk + w.grp_off);
    a.hsums = reinterpret_cast<uint64_t *>(wk + w.hsums_off);
    a.ssums = reinterpret_cast<uint32_t *>(wk + w.ssums_off);
    a.n_groups = reinterpret_cast<uint64_t *>(wk + w.count_off);
    a.sites = static_cast<uint4 *>(x.sites);
    a.n_sites = x.n_sites;
    a.n = n;
    a.source_bases = x.source_bases;
    a.capacity = x.capacity;
    a.n_src = x.n_src;
    a.t = Thresholds{x.min_count, x.frac_num, x.frac_den};
    a.keys = ka;
    if (n) {
        hipLaunchKernelGGL(key_kernel, dim3((uint32_t)((n + kThreads - 1u) / kThreads)), dim3(kThreads), 0, stream, a, ka);
        const uint32_t first = sort_first_bit(x.source_bases);
        for (uint32_t end = kSortEndBit; end > first;) { // LSD: the least significant digit first
            const uint32_t nb = end - first < 8u ? end - first : 8u;
            const RadixPass ps{end - nb, nb, 0u};
            const hipError_t e = launch_build_radix_pass(ka, kb, 2u, n, nullptr, nullptr, n, ps, reinterpret_cast<uint32_t *>(wk + w.hist_off),
                                                         reinterpret_cast<uint32_t *>(wk + w.rsums_off), stream);
            if (e != hipSuccess) return e;
            uint64_t *t = ka;
            ka = kb;
            kb = t;
            end -= nb;
        }
        a.keys = ka;
    }
    const uint32_t hchunks = (uint32_t)scan_chunks(n + 1u), schunks = (uint32_t)scan_chunks(n);
    hipLaunchKernelGGL(head_count_kernel, dim3(hchunks), dim3(kThreads), 0, stream, a);
    hipLaunchKernelGGL(sums64_kernel, dim3(1), dim3(kThreads), 0, stream, a.hsums, (uint64_t)hchunks, a.n_groups);
    hipLaunchKernelGGL(head_apply_kernel, dim3(hchunks), dim3(kThreads), 0, stream, a);
    if (schunks) hipLaunchKernelGGL(site_count_kernel, dim3(schunks), dim3(kThreads), 0, stream, a);
    hipLaunchKernelGGL(site_sums_kernel, dim3(1), dim3(kThreads), 0, stream, a.ssums, (uint64_t)schunks, x.n_sites);
    if (schunks) hipLaunchKernelGGL(site_emit_kernel, dim3(schunks), dim3(kThreads), 0, stream, a);
    return hipGetLastError();
}

} // namespace kbo
