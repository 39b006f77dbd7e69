// place_kernels.hip — one placement per sequence from the segments of a walked batch (kbo_hip.h "Placement"; the arithmetic, the
// ring and the d_work layout: index_place.hpp).
//   place_init_kernel    a lane per sequence: no range yet, and the list of the wave route empty
//   place_range_kernel   a lane per record: its source by a bisection of the source offsets, and where a stretch of equal seq values
//                        starts or ends one integer atomic into the sequence's range
//   place_lane_kernel    a lane per sequence: kPlaceNone without a range, a list of at most kLaneMax segments chained in registers, a
//                        longer one appended to the list of the wave route
//   place_wave_kernel    a wave per listed sequence: the steps over i are serial, lane l holds slot l of the LDS ring - the one
//                        predecessor of the step that is congruent to l - and the winner is a maximum over the lanes and a ballot
// Every launch reads the number of records on the device: min(*d_n_segs, capacity).  A sequence is written by one lane of one launch.
#include "device_util.hpp"
#include "index_place.hpp"

namespace kbo {
namespace {

using namespace idxplace;

struct PArgs {
    const uint32_t *segs; // records of 7 words
    const uint64_t *n_segs;
    const uint64_t *src_off;
    uint32_t *begin, *end, *list, *n_long, *src;
    uint4 *place;
    uint64_t capacity;
    uint32_t n_seqs, n_src, merge;
    Limits lim;
};

__device__ __forceinline__ uint32_t n_records(const PArgs &a)
{
    const uint64_t n = *a.n_segs;
    return (uint32_t)(n < a.capacity ? n : a.capacity);
}
__device__ __forceinline__ Segment load_segment(const uint32_t *__restrict__ segs, uint32_t x)
{
    const uint32_t *p = segs + (uint64_t)x * 7u;
    return Segment{p[0], p[1], p[2], p[3], p[4], p[5], p[6]};
}
struct DevSegs {
    const uint32_t *p;
    __device__ Segment get(uint64_t x) const { return load_segment(p, (uint32_t)x); }
};
struct DevSrcOff {
    const uint64_t *p;
    __device__ uint64_t off(size_t s) const { return p[s]; }
};

// the record of sequence s: merged into what is there, or written over it
__device__ __forceinline__ void store_place(const PArgs &a, uint32_t s, const Place &p)
{
    union {
        Place rec;
        uint4 q[3];
    } u, old;
    u.rec = p;
    uint4 *o = a.place + (uint64_t)s * 3u;
    if (a.merge) {
        old.q[0] = o[0];
        old.q[1] = o[1];
        old.q[2] = o[2];
        u.rec = merged(old.rec, p);
    }
    o[0] = u.q[0];
    o[1] = u.q[1];
    o[2] = u.q[2];
}

__global__ void __launch_bounds__(kThreads) place_init_kernel(PArgs a)
{
    const uint32_t s = blockIdx.x * kThreads + threadIdx.x;
    if (s == 0) *a.n_long = 0;
    if (s >= a.n_seqs) return;
    a.begin[s] = kNoRange;
    a.end[s] = 0;
}

__global__ void __launch_bounds__(kThreads) place_range_kernel(PArgs a)
{
    const uint32_t n = n_records(a);
    for (uint64_t x = (uint64_t)blockIdx.x * kThreads + threadIdx.x; x < n; x += (uint64_t)gridDim.x * kThreads) {
        const uint32_t *p = a.segs + x * 7u;
        const uint32_t s = p[0];
        a.src[x] = seq_of(DevSrcOff{a.src_off}, a.n_src, p[4]);
        if (s >= a.n_seqs) continue;
        if (x == 0 || p[-7] != s) atomicMin(a.begin + s, (uint32_t)x);
        if (x + 1u == n || p[7] != s) atomicMax(a.end + s, (uint32_t)x + 1u);
    }
}

// the lane route's ring: the states of a list of at most kLaneMax segments, in registers once the loops are unrolled
struct LaneRing {
    State st[kLaneMax];
    __device__ __forceinline__ State get(uint32_t slot) const { return st[slot]; }
};

__global__ void __launch_bounds__(kThreads) place_lane_kernel(PArgs a)
{
    const uint32_t s = blockIdx.x * kThreads + threadIdx.x;
    if (s >= a.n_seqs) return;
    const uint32_t n = n_records(a), b = a.begin[s], e = a.end[s];
    Place out = no_place();
    if (has_range(b, e, n)) {
        const uint32_t count = e - b;
        if (count > kLaneMax) { // (the wave route writes the record)
            a.list[atomicAdd(a.n_long, 1u)] = s;
            return;
        }
        LaneRing ring;
        Top top = no_top();
#pragma unroll
        for (uint32_t i = 0; i < kLaneMax; i++) {
            if (i < count) {
                const Segment sg = load_segment(a.segs, b + i);
                State st = no_state();
                if (sg.seq == s) st = chain_step(ring, i, seg_of(sg, a.lim.k, a.src[b + i]), a.lim);
                ring.st[i] = st;
                top_add(top, st, i);
            }
        }
        if (top.any) {
            const uint32_t src = a.src[b + top.root];
            out = place_of(top, load_segment(a.segs, b + top.root), load_segment(a.segs, b + top.i), src, a.src_off[(uint64_t)src + 1u], a.lim.k);
        }
    }
    store_place(a, s, out);
}

// ---- the wave route
constexpr uint32_t kStateWords = 10;
struct LdsRing { // a word of every state side by side: lane l reads slot l without a bank conflict
    uint32_t (*w)[kWindow];
    __device__ __forceinline__ State get(uint32_t slot) const
    {
        State s;
        s.q_last = w[0][slot];
        s.src = w[1][slot];
        s.tag = w[2][slot];
        s.diag = (int64_t)((uint64_t)w[3][slot] | (uint64_t)w[4][slot] << 32);
        s.f = w[5][slot];
        s.root = w[6][slot];
        s.n_segs = w[7][slot];
        s.indel = w[8][slot];
        s.n_multi = w[9][slot];
        return s;
    }
    __device__ __forceinline__ void set(uint32_t slot, const State &s) const
    {
        w[0][slot] = s.q_last;
        w[1][slot] = s.src;
        w[2][slot] = s.tag;
        w[3][slot] = (uint32_t)(uint64_t)s.diag;
        w[4][slot] = (uint32_t)((uint64_t)s.diag >> 32);
        w[5][slot] = s.f;
        w[6][slot] = s.root;
        w[7][slot] = s.n_segs;
        w[8][slot] = s.indel;
        w[9][slot] = s.n_multi;
    }
};
__device__ __forceinline__ uint32_t wave_max(uint32_t v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t x = __shfl_xor(v, o);
        v = x > v ? x : v;
    }
    return v;
}

__global__ void __launch_bounds__(kWindow) place_wave_kernel(PArgs a)
{
    __shared__ uint32_t words[kStateWords][kWindow];
    const LdsRing ring{words};
    const uint32_t lane = threadIdx.x, n = n_records(a);
    uint32_t n_long = *a.n_long;
    n_long = n_long < a.n_seqs ? n_long : a.n_seqs;
    for (uint32_t at = blockIdx.x; at < n_long; at += gridDim.x) { // (uniform: every lane of the wave takes every turn)
        const uint32_t s = a.list[at];
        if (s >= a.n_seqs) continue;
        const uint32_t b = a.begin[s], e = a.end[s];
        if (!has_range(b, e, n)) continue;
        const uint32_t count = e - b;
        Top top = no_top();
        Segment next = load_segment(a.segs, b);
        uint32_t next_src = a.src[b];
        for (uint32_t i = 0; i < count; i++) {
            const Segment sg = next;
            const uint32_t sg_src = next_src;
            if (i + 1u < count) { // (the next record is on its way while this one is chained)
                next = load_segment(a.segs, b + i + 1u);
                next_src = a.src[b + i + 1u];
            }
            State st = no_state();
            if (sg.seq == s) { // (uniform)
                const Seg c = seg_of(sg, a.lim.k, sg_src);
                const State mine = ring.get(lane); // segment i - 1 - l, l = (i - 1 - lane) mod kWindow: there once i > lane
                int64_t sh = 0;
                const bool ok = lane < i && precedes(mine, c, a.lim, &sh);
                const uint32_t v = ok ? value_through(mine, c) : 0u;
                const uint32_t best = wave_max(v);
                const uint64_t mask = __ballot(ok && v == best);
                if (mask && best > c.len) {
                    const State p = ring.get(winner_slot(mask, i)); // (one slot for all lanes: a broadcast)
                    (void)precedes(p, c, a.lim, &sh);
                    st = extend(c, i, true, p, best, sh);
                } else {
                    st = extend(c, i, false, no_state(), 0u, 0);
                }
            }
            __syncthreads(); // (one wave a workgroup: every lane has read its slot before the slot of i - kWindow is written over ...
            if (lane == slot_of(i)) ring.set(lane, st);
            __syncthreads(); // ... and the next step reads what this one wrote)
            top_add(top, st, i);
        }
        if (lane == 0) {
            Place out = no_place();
            if (top.any) {
                const uint32_t src = a.src[b + top.root];
                out = place_of(top, load_segment(a.segs, b + top.root), load_segment(a.segs, b + top.i), src, a.src_off[(uint64_t)src + 1u], a.lim.k);
            }
            store_place(a, s, out);
        }
    }
}

} // namespace

hipError_t launch_place(const PlaceArgs &x, hipStream_t stream)
{
    if (x.n_seqs == 0 || x.n_seqs >= kMaxSeqs || x.capacity > kMaxSegs || x.n_src == 0 || x.k == 0) return hipErrorInvalidValue;
    const PlaceWork w = place_work(x.n_seqs, x.capacity);
    uint8_t *work = static_cast<uint8_t *>(x.work);
    PArgs a;
    a.segs = x.segs;
    a.n_segs = x.n_segs;
    a.src_off = x.src_off;
    a.begin = reinterpret_cast<uint32_t *>(work);
    a.end = reinterpret_cast<uint32_t *>(work + w.end_off);
    a.list = reinterpret_cast<uint32_t *>(work + w.list_off);
    a.n_long = reinterpret_cast<uint32_t *>(work + w.count_off);
    a.src = reinterpret_cast<uint32_t *>(work + w.src_off);
    a.place = static_cast<uint4 *>(x.place);
    a.capacity = x.capacity;
    a.n_seqs = x.n_seqs;
    a.n_src = x.n_src;
    a.merge = x.merge ? 1u : 0u;
    a.lim = Limits{x.k, x.max_gap, x.max_indel};
    const uint32_t seq_blocks = (x.n_seqs + kThreads - 1u) / kThreads;
    const uint64_t rec_blocks = (x.capacity + kThreads - 1u) / kThreads;
    // the wave route's sequences are known on the device alone: a wave per sequence it can hold, at most 16 a compute unit's worth
    const uint64_t most_long = x.capacity / (kLaneMax + 1u) < x.n_seqs ? x.capacity / (kLaneMax + 1u) : x.n_seqs;
    hipLaunchKernelGGL(place_init_kernel, dim3(seq_blocks), dim3(kThreads), 0, stream, a);
    if (rec_blocks) hipLaunchKernelGGL(place_range_kernel, dim3((uint32_t)(rec_blocks < 4096u ? rec_blocks : 4096u)), dim3(kThreads), 0, stream, a);
    hipLaunchKernelGGL(place_lane_kernel, dim3(seq_blocks), dim3(kThreads), 0, stream, a);
    if (most_long) hipLaunchKernelGGL(place_wave_kernel, dim3((uint32_t)(most_long < 4096u ? most_long : 4096u)), dim3(kWindow), 0, stream, a);
    return hipGetLastError();
}

} // namespace kbo
