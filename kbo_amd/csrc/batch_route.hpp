// batch_route.hpp — the kernel route of a batch over one index, stated once for the device-resident calls (device_batch.cpp) and
// the slabs of a host batch (host_batch.cpp): map_long_kernel, map_reads_kernel with its second pass (bytes, packed-native and summary
// forms) or the walk over every shard - and the WalkArgs of each.  Both sides describe their batch as a BatchView and call this.
#pragma once
#include "capi_internal.hpp"

// (shared by two units of the library, no part of what it exports: hidden)
namespace kbo_host __attribute__((visibility("hidden"))) {

// one index's copy on the current device, asked for once per call: device_view() counts the batch's bases for the copy's lazy plan
// structures
struct CopyView {
    kbo::DevIndexView ix{};
    DevCopy::PlanState *plan = nullptr;
};
inline CopyView copy_view(kbo_index *idx, uint64_t total_bases)
{
    CopyView c;
    c.ix = device_view(idx, current_device(), &c.plan, total_bases);
    return c;
}

// memory a route may need: the caller's own (a region of d_work) or a pooled buffer that grows when the route first takes it (a slab's)
struct Scratch {
    void *p = nullptr;
    DevBuf *grow = nullptr;
    void *get(size_t bytes) const { return grow ? (grow->ensure(bytes), grow->p) : p; }
};

// A batch as it lies on the device.  The device entry points fill it from d_work, a slab from its BatchOnDevice.
struct BatchView {
    // the queries: bytes where the walk reads them and / or 2-bit words (pack_kernels.hip) with their non-ACGT list.  have_bytes = false:
    // a packed batch none of whose bytes are in `q` yet (need_bytes unpacks them all; a packed-native second pass those of its reads)
    const uint8_t *q = nullptr;
    uint8_t *bytes_out = nullptr; // == q where the batch came as words: where their bytes are unpacked
    bool have_bytes = true;
    const uint32_t *qp = nullptr;
    size_t n_words = 0;
    uint32_t wps = 0;               // words per sequence, or 0 and ...
    const uint32_t *pscr = nullptr; // ... the scanned words per sequence (launch_packed_prefix)
    const uint64_t *exc_pos = nullptr; // ... their non-ACGT list: positions, ...
    const uint8_t *exc_byte = nullptr; // ... bytes, ...
    uint32_t n_exc = 0;
    uint64_t exc_base = 0; // ... and the batch's first base in the positions' coordinates
    Scratch exc_flag;      // n_seqs + 16 bytes: one per read of a packed-native launch
    const uint64_t *offsets = nullptr;
    uint32_t n_seqs = 0;
    uint64_t total = 0;
    uint32_t longest = 0; // longest sequence, 0 = not known
    // the work items: one per sequence, or chunks of `chunk` bases with their warm-up bases.  reads_seq_off: what
    // map_reads_kernel takes as WalkArgs::seq_off - the offsets where no item list is made for it (the device calls), null where the
    // list exists (a slab: launch_make_items has run) and only its second pass reads the offsets
    kbo::WalkItem *items = nullptr;
    uint32_t n_items = 0;
    uint32_t chunk = 0; // (0: one item per sequence)
    const uint64_t *reads_seq_off = nullptr;
    Scratch plan; // kbo::plan_work_bytes(n_items, total)
    uint8_t *ms = nullptr, *ms_shard = nullptr;
    Scratch long_work; // kbo::long_work_bytes(n_seqs, total, k)
};

// what the walk is to leave besides the MS values: intervals, or the call mode's sites
struct WalkAsk {
    uint32_t *lo = nullptr, *hi = nullptr;
    const CallSink *call = nullptr;
};

// sequences of more than 160 bases (or of a length not known): not map_reads_kernel's
inline bool long_seqs(const BatchView &v) { return v.longest == 0 || v.longest > 160u; }

// the WalkArgs of a launch over `v` and the copy `c`: the batch, the call mode, the longest item, the plan work (attach_plan: one call
// per launch - it counts the copy's hold-off) and, with `map` (capi_internal.hpp FusedMap: what kbo::matches / map / find / the
// summaries ask), map_reads_kernel's fields.  c.plan = null: planned whatever the hold-off
kbo::WalkArgs walk_args(const BatchView &v, const CopyView &c, uint8_t *ms_out, const WalkAsk &w, const FusedMap *map);

// the packed-native fields of `a`, the flags of the reads that hold a listed byte made on `s`
void packed_native_args(const BatchView &v, kbo::WalkArgs &a, uint32_t *packed_out, hipStream_t s);

// The reads map_reads_kernel left, on `t`, in whatever form `a` describes (one_wave_groups: launch_map_reads_finish as workgroups of
// one wave)
void second_pass(const BatchView &v, const kbo::WalkArgs &a, hipStream_t t, bool one_wave_groups);
// How a caller launches map_reads_kernel with its second pass behind it: both on `s`, or then(v, a, L), which enqueues the kernel on
// `s` and second_pass on a stream of its choice, which it returns
struct ReadsLaunch {
    hipStream_t s = nullptr, tail = nullptr; // (tail == s: no stream of its own for second passes)
    bool one_wave_tail = false;              // launch_map_reads_finish on a tail of its own as workgroups of one wave
    hipStream_t (*then)(const BatchView &, kbo::WalkArgs &, const ReadsLaunch &) = nullptr;
};
// what `s` holds so far is waited for by `tail`, which is returned (tail == s: nothing to do).  `a`: a batch of reads' second pass
hipStream_t fork_tail(hipStream_t s, hipStream_t tail, kbo::WalkArgs *a);

// map_reads_kernel over `a` and the second pass over the reads it leaves, whatever form `a` describes; returns the stream the result
// is complete on.  a.host_bailed is the caller's: unset, the launch reports a plan given up by plan_after_launch
hipStream_t run_reads(const BatchView &v, kbo::WalkArgs &a, DevCopy::PlanState *plan, const ReadsLaunch &L);

// the walk over every shard of `idx` on `s`, the maximum kept in v.ms.  given: the copy of the one index where the caller has asked
// for it already (else every shard's is asked for here); filled: its WalkArgs where the caller has made them for this launch already
void walk_shards(BatchView &v, kbo_index *idx, const CopyView *given, const WalkAsk &w, hipStream_t s, const kbo::WalkArgs *filled = nullptr);

// kbo::matches / map over a batch and the copy `c` of an unsharded index: sequences of any length by map_long_kernel, reads by
// map_reads_kernel in its summary, packed-native or bytes form - or nothing: the caller walks and derandomizes (two kernels).  What
// it did is left in `m` (done and which of the extras; when done, ts: where the result is complete).  `a`: walk_args with `m`, or empty
// where the caller made none
void route_map(BatchView &v, const CopyView &c, kbo::WalkArgs &a, FusedMap &m, const ReadsLaunch &L);

} // namespace kbo_host
