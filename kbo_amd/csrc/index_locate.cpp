// index_locate.cpp — kbo_hip.h "Positions, segments, depth": the position table of an index made on the device from a walk of its
// own sources (kbo_index_add_positions and its getters), the segments of a walked batch and the depth of the sources over device
// buffers (kbo_segments_dev, kbo_depth_finish_dev), the host batch that composes them (kbo_segments_batch) and the CPU restatements
// (kbo_positions_from_ms_host, kbo_segments_from_ms_host).  The arithmetic is index_locate.hpp's, the kernels locate_kernels.hip's.
#include "../../include/kbo_hip.h"
#include "../../include/kbo_hip_tuning.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstring>
#include <mutex>
#include <vector>

#include "capi_internal.hpp"
#include "index_locate.hpp"

using namespace kbo_host;
namespace loc = kbo::idxlocate;

static_assert(sizeof(kbo_seq_segment) == 28 && sizeof(loc::Segment) == 28, "the kernels write records of seven words");
static_assert(loc::kTile == KBO_SEGMENTS_TILE && loc::kHalo == KBO_SEGMENTS_HALO && loc::kMaxBridge == KBO_SEGMENTS_MAX_BRIDGE,
              "kbo_hip_tuning.h states the kernels' constants");
static_assert(loc::kPosNone == KBO_POS_NONE && loc::kMulti == KBO_LOCUS_MULTI, "one entry encoding");

namespace {

std::atomic<uint64_t> g_slab_bases{0}; // kbo_set_positions_slab_bases: source bases a slab of kbo_index_add_positions adds (0 = the default)
constexpr uint64_t kDefaultSlabBases = 32ull << 20;

void ok(int rc)
{
    if (rc != KBO_OK) throw KboError(rc, last_error());
}

bool has_positions(const kbo_index *idx)
{
    std::lock_guard<std::mutex> g(const_cast<kbo_index *>(idx)->mu);
    return !idx->src_off.empty();
}

void drop_positions(kbo_index *idx)
{
    std::lock_guard<std::mutex> g(idx->mu);
    idx->positions.clear();
    idx->src_off.clear();
    for (auto &kv : idx->dev) {
        kv.second->positions.release();
        kv.second->src_off.release();
    }
}

// the source offsets beside a copy's table (mu held, the copy's device current)
void upload_src_off(kbo_index *idx, DevCopy *copy)
{
    if (copy->src_off.p) return;
    copy->src_off.alloc(idx->src_off.size() * sizeof(uint64_t));
    HIP_OK(hipMemcpy(copy->src_off.p, idx->src_off.data(), idx->src_off.size() * sizeof(uint64_t), hipMemcpyHostToDevice));
}

// the table of the copy on `dev`, or null; make: uploaded when the copy has none (the device current)
const uint32_t *positions_on(kbo_index *idx, int dev, bool make)
{
    if (make) (void)device_view(idx, dev);
    std::lock_guard<std::mutex> g(idx->mu);
    auto it = idx->dev.find(dev);
    if (it == idx->dev.end() || idx->src_off.empty()) return nullptr;
    DevBuf &b = it->second->positions;
    if (!b.p && make) {
        b.alloc(idx->positions.size() * sizeof(uint32_t));
        if (!idx->positions.empty())
            HIP_OK(hipMemcpy(b.p, idx->positions.data(), idx->positions.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    }
    if (make) upload_src_off(idx, it->second.get());
    return b.as<uint32_t>();
}

bool is_base(uint8_t c) { return c == 'A' || c == 'C' || c == 'G' || c == 'T'; }

void add_positions(kbo_index *idx, const uint8_t *const *seqs, const size_t *lens, size_t n_seqs, bool rc, int device)
{
    const uint32_t k = (uint32_t)idx->host.k;
    const uint64_t n_rows = idx->host.n_sets;
    std::vector<uint64_t> src_off(n_seqs + 1, 0);
    uint64_t windows = 0; // the windows of the indexed stretches: every one must reach depth k
    for (size_t s = 0; s < n_seqs; s++) {
        KBO_REQUIRE(seqs[s] || lens[s] == 0, KBO_E_BAD_ARG, "null sequence");
        src_off[s + 1] = src_off[s] + lens[s];
        KBO_REQUIRE(src_off[s + 1] < loc::kMaxSourceBases, KBO_E_UNSUPPORTED, "sources of 2^30 bases or more (an entry's position has 30 bits)");
    }
    for (size_t s = 0; s < n_seqs; s++) {
        uint64_t run = 0;
        for (size_t j = 0; j < lens[s]; j++) {
            run = is_base(seqs[s][j]) ? run + 1 : 0;
            windows += run >= k;
        }
    }
    KBO_REQUIRE(n_rows < 0xFFFFFFFFull && k > 0, KBO_E_UNSUPPORTED, "an index of 2^32 - 1 rows or more");
    const uint64_t total = src_off[n_seqs];
    // ---- the device from here on
    DeviceScope scope(device);
    const int dev = current_device();
    drop_positions(idx);
    (void)device_view(idx, dev);
    DevBuf mn(n_rows * 4), mx(n_rows * 4), cnt(16);
    HIP_OK(hipMemset(mn.p, 0xFF, n_rows * 4));
    HIP_OK(hipMemset(mx.p, 0, n_rows * 4));
    HIP_OK(hipMemset(cnt.p, 0, 16));
    const uint64_t want = g_slab_bases.load(), slab = std::max<uint64_t>(1, want ? want : kDefaultSlabBases);
    const uint64_t most = std::min<uint64_t>(total, slab + k - 1);
    const size_t pad = (size_t)loc::round16(most) + 64;
    DevBuf q(pad), qr(rc ? pad : 16), ms(pad), lo(most * 4 + 16), hi(most * 4 + 16), off, work;
    HIP_OK(hipMemset(q.p, 0, pad));
    if (rc) HIP_OK(hipMemset(qr.p, 0, pad));
    std::vector<uint8_t> bytes;
    std::vector<uint64_t> cuts, up;
    for (uint64_t b0 = 0; b0 < total; b0 += slab) {
        const uint64_t a = b0 >= k - 1 ? b0 - (k - 1) : 0, b1 = std::min(total, b0 + slab), len = b1 - a;
        bytes.resize(len);
        cuts.assign(1, 0);
        size_t s = (size_t)(std::upper_bound(src_off.begin(), src_off.end(), a) - src_off.begin()) - 1; // the sequence that holds base a
        for (; s < n_seqs && src_off[s] < b1; s++) {
            const uint64_t x0 = std::max(a, src_off[s]), x1 = std::min(b1, src_off[s + 1]);
            if (x1 <= x0) continue;
            std::memcpy(bytes.data() + (x0 - a), seqs[s] + (x0 - src_off[s]), x1 - x0);
            if (x0 - a != cuts.back()) cuts.push_back(x0 - a);
        }
        cuts.push_back(len);
        const size_t ns = cuts.size() - 1;
        // the slab's offsets | the same mirrored (the slab reversed as a whole) | the slab as one sequence
        up = cuts;
        for (size_t t = 0; t <= ns; t++) up.push_back(len - cuts[ns - t]);
        up.push_back(0);
        up.push_back(len);
        off.ensure(up.size() * 8);
        HIP_OK(hipMemcpy(off.p, up.data(), up.size() * 8, hipMemcpyHostToDevice));
        HIP_OK(hipMemcpy(q.p, bytes.data(), len, hipMemcpyHostToDevice));
        const size_t wb = kbo_ms_work_bytes(ns, len, 0, k);
        work.ensure(wb);
        for (int rev = 0; rev < (rc ? 2 : 1); rev++) {
            const uint64_t *d_off = off.as<uint64_t>() + (rev ? ns + 1 : 0);
            if (rev) ok(kbo_revcomp_batch_dev(q.as<uint8_t>(), off.as<uint64_t>() + 2 * (ns + 1), 1, len, 0, qr.as<uint8_t>(), nullptr));
            ok(kbo_ms_batch_dev(idx, rev ? qr.as<uint8_t>() : q.as<uint8_t>(), d_off, ns, len, 0, ms.as<uint8_t>(), lo.as<uint32_t>(),
                                hi.as<uint32_t>(), work.p, wb, nullptr));
            HIP_OK(kbo::launch_locate_mark(ms.as<uint8_t>(), lo.as<uint32_t>(), (uint32_t)len, k, (uint32_t)n_rows, (uint32_t)a, rev != 0,
                                           mn.as<uint32_t>(), mx.as<uint32_t>(), cnt.as<uint64_t>(), nullptr));
        }
    }
    HIP_OK(kbo::launch_locate_entries(mn.as<uint32_t>(), mx.as<uint32_t>(), (uint32_t)n_rows, cnt.as<uint64_t>() + 1, nullptr));
    uint64_t got[2];
    HIP_OK(hipMemcpy(got, cnt.p, 16, hipMemcpyDeviceToHost));
    KBO_REQUIRE(got[0] == windows * (rc ? 2 : 1), KBO_E_BAD_ARG,
                "a window of the sequences does not reach depth k in this index: these are not the sequences it was built from (or add_revcomp differs)");
    KBO_REQUIRE(got[1] == idx->host.n_kmers, KBO_E_BAD_ARG,
                "the index holds k-mers that the sequences lack: these are not all the sequences it was built from (or add_revcomp differs)");
    std::vector<uint32_t> host(n_rows);
    if (n_rows) HIP_OK(hipMemcpy(host.data(), mn.p, n_rows * 4, hipMemcpyDeviceToHost));
    std::lock_guard<std::mutex> g(idx->mu);
    idx->positions = std::move(host);
    idx->src_off = std::move(src_off);
    DevBuf &keep = idx->dev.at(dev)->positions;
    keep.release();
    std::swap(keep.p, mn.p);
    std::swap(keep.cap, mn.cap);
    std::swap(keep.dev, mn.dev);
    upload_src_off(idx, idx->dev.at(dev).get());
}

struct HostIn {
    const uint8_t *d_;
    const uint32_t *lo_;
    const uint64_t *off_;
    uint64_t shift;
    uint32_t d(uint64_t i) const { return d_[shift + i]; }
    uint32_t lo(uint64_t i) const { return lo_[shift + i]; }
    uint64_t off(size_t s) const { return off_[s]; }
};
struct HostTab {
    uint32_t *p;
    uint32_t get(uint32_t r) const { return p[r]; }
    void set(uint32_t r, uint32_t e) { p[r] = e; }
};

void require_offsets(const uint64_t *offsets, size_t n_seqs)
{
    KBO_REQUIRE(offsets[0] == 0, KBO_E_BAD_ARG, "offsets[0] must be 0");
    for (size_t s = 0; s < n_seqs; s++) KBO_REQUIRE(offsets[s + 1] >= offsets[s], KBO_E_BAD_ARG, "offsets not monotone");
}

size_t segments_work_bytes(size_t n_seqs, uint64_t total_bases)
{
    if (n_seqs == 0 || n_seqs >= (1ull << 28) || total_bases + 16 > (1ull << 32)) return 0;
    return total_bases ? (size_t)loc::seg_work(total_bases).bytes : 16;
}

// kbo_segments_dev behind its checks
void segments_enqueue(const uint32_t *d_entries, uint32_t n_rows, uint32_t k, uint32_t n_delta, const uint8_t *d_ms, const uint32_t *d_lo,
                      const uint64_t *d_offsets, size_t n_seqs, uint64_t total, uint32_t bridge, uint32_t strand, kbo_seq_segment *d_segs,
                      size_t capacity, uint64_t *d_n_segs, uint32_t *d_delta, void *d_work, hipStream_t s)
{
    if (total == 0) { // (nothing but empty sequences)
        HIP_OK(hipMemsetAsync(d_n_segs, 0, 8, s));
        return;
    }
    kbo::SegmentArgs a;
    a.ms = d_ms;
    a.lo = d_lo;
    a.off = d_offsets;
    a.entries = d_entries;
    a.n_seqs = (uint32_t)n_seqs;
    a.n_rows = n_rows;
    a.k = k;
    a.bridge = bridge;
    a.strand = strand;
    a.n_delta = n_delta;
    a.total = total;
    a.capacity = capacity;
    a.segs = reinterpret_cast<uint32_t *>(d_segs);
    a.n_segs = d_n_segs;
    a.delta = d_delta;
    a.work = d_work;
    HIP_OK(kbo::launch_segments(a, s));
}

} // namespace

const uint64_t *kbo_host::source_offsets_on(kbo_index *idx, int dev, uint32_t *n_src)
{
    std::lock_guard<std::mutex> g(idx->mu);
    auto it = idx->dev.find(dev);
    if (it == idx->dev.end() || idx->src_off.empty() || !it->second->positions.p || !it->second->src_off.p) return nullptr;
    *n_src = (uint32_t)(idx->src_off.size() - 1);
    return it->second->src_off.as<uint64_t>();
}

int kbo_set_positions_slab_bases(uint64_t bases)
{
    g_slab_bases.store(bases);
    return KBO_OK;
}

int kbo_segments_geometry(uint32_t *tile, uint32_t *halo, uint32_t *scan_chunk)
{
    if (tile) *tile = loc::kTile;
    if (halo) *halo = loc::kHalo;
    if (scan_chunk) *scan_chunk = loc::kScanChunk;
    return KBO_OK;
}

int kbo_index_add_positions(kbo_index_t *idx, const uint8_t *const *seqs, const size_t *lens, size_t n_seqs, int add_revcomp, int device)
{
    return guarded([&] {
        KBO_REQUIRE(idx && seqs && lens && n_seqs > 0, KBO_E_BAD_ARG, "null argument or no sequence");
        require_unsharded(idx, "kbo_index_add_positions");
        try {
            add_positions(idx, seqs, lens, n_seqs, add_revcomp != 0, device);
        } catch (...) {
            drop_positions(idx); // (a failure leaves the handle without positions)
            throw;
        }
    });
}

int kbo_index_has_positions(const kbo_index_t *idx) { return idx && !idx->sharded() && has_positions(idx) ? 1 : 0; }

uint64_t kbo_index_positions_bytes(const kbo_index_t *idx)
{
    if (!kbo_index_has_positions(idx)) return 0;
    std::lock_guard<std::mutex> g(const_cast<kbo_index_t *>(idx)->mu);
    return idx->positions.size() * sizeof(uint32_t) + idx->src_off.size() * sizeof(uint64_t);
}

int kbo_index_positions(const kbo_index_t *idx, uint32_t *out, size_t *n_rows)
{
    return guarded([&] {
        KBO_REQUIRE(idx && n_rows, KBO_E_BAD_ARG, "null argument");
        KBO_REQUIRE(kbo_index_has_positions(idx), KBO_E_BAD_ARG, "the handle has no positions (kbo_index_add_positions)");
        std::lock_guard<std::mutex> g(const_cast<kbo_index_t *>(idx)->mu);
        *n_rows = idx->positions.size();
        if (out && !idx->positions.empty()) std::memcpy(out, idx->positions.data(), idx->positions.size() * sizeof(uint32_t));
    });
}

int kbo_index_source_offsets(const kbo_index_t *idx, uint64_t *out, size_t *n)
{
    return guarded([&] {
        KBO_REQUIRE(idx && n, KBO_E_BAD_ARG, "null argument");
        KBO_REQUIRE(kbo_index_has_positions(idx), KBO_E_BAD_ARG, "the handle has no positions (kbo_index_add_positions)");
        std::lock_guard<std::mutex> g(const_cast<kbo_index_t *>(idx)->mu);
        *n = idx->src_off.size();
        if (out) std::memcpy(out, idx->src_off.data(), idx->src_off.size() * sizeof(uint64_t));
    });
}

uint64_t kbo_index_source_bases(const kbo_index_t *idx)
{
    if (!kbo_index_has_positions(idx)) return 0;
    std::lock_guard<std::mutex> g(const_cast<kbo_index_t *>(idx)->mu);
    return idx->src_off.back();
}

int kbo_index_positions_to_device(kbo_index_t *idx, int device)
{
    return guarded([&] {
        KBO_REQUIRE(idx, KBO_E_BAD_ARG, "null index");
        require_unsharded(idx, "kbo_index_positions_to_device");
        KBO_REQUIRE(has_positions(idx), KBO_E_BAD_ARG, "the handle has no positions (kbo_index_add_positions)");
        DeviceScope scope(device);
        (void)positions_on(idx, current_device(), true);
    });
}

int kbo_positions_from_ms_host(uint32_t k, uint64_t n_sets, const uint8_t *d, const uint32_t *lo, const uint64_t *offsets, size_t n_seqs,
                               const uint64_t *src_off, int rev, uint32_t *entries_inout, uint64_t *n_not_full)
{
    return guarded([&] {
        KBO_REQUIRE(d && lo && offsets && src_off && entries_inout && n_seqs > 0 && k > 0, KBO_E_BAD_ARG, "null argument");
        KBO_REQUIRE(n_sets < 0xFFFFFFFFull, KBO_E_UNSUPPORTED, "2^32 - 1 rows or more");
        require_offsets(offsets, n_seqs);
        KBO_REQUIRE(src_off[n_seqs] < loc::kMaxSourceBases, KBO_E_UNSUPPORTED, "sources of 2^30 bases or more");
        HostTab tab{entries_inout};
        uint64_t missing = 0;
        for (size_t s = 0; s < n_seqs; s++) {
            const uint64_t len = offsets[s + 1] - offsets[s];
            KBO_REQUIRE(src_off[s + 1] - src_off[s] == len, KBO_E_BAD_ARG, "a sequence of the walk and its source differ in length");
            const HostIn in{d, lo, offsets, offsets[s]};
            const uint64_t full = loc::mark_serial(in, (uint32_t)src_off[s], (uint32_t)len, k, (uint32_t)n_sets, rev != 0, tab);
            missing += (len >= k ? len - k + 1 : 0) - full;
        }
        if (n_not_full) *n_not_full = missing;
    });
}

int kbo_segments_from_ms_host(const uint32_t *entries, uint64_t n_rows, uint32_t k, const uint8_t *d, const uint32_t *lo,
                              const uint64_t *offsets, size_t n_seqs, uint32_t bridge, uint32_t strand, kbo_seq_segment *segs, size_t capacity,
                              uint64_t *n_segs, uint32_t *delta, uint64_t source_bases)
{
    return guarded([&] {
        KBO_REQUIRE(entries && d && lo && offsets && n_segs && (segs || capacity == 0) && k > 0, KBO_E_BAD_ARG, "null argument");
        KBO_REQUIRE(bridge <= loc::kMaxBridge, KBO_E_BAD_ARG, "bridge above 255");
        KBO_REQUIRE(n_seqs > 0, KBO_E_EMPTY_QUERY, "no sequences");
        require_offsets(offsets, n_seqs);
        KBO_REQUIRE(offsets[n_seqs] + 16 <= (1ull << 32) && n_seqs < (1ull << 28) && n_rows < 0xFFFFFFFFull && source_bases < loc::kMaxSourceBases,
                    KBO_E_UNSUPPORTED, "a batch of 2^32 - 16 bases or 2^28 sequences, or more");
        const HostIn in{d, lo, offsets, 0};
        const HostTab tab{const_cast<uint32_t *>(entries)};
        *n_segs = loc::segments_serial(in, tab, (uint32_t)n_rows, k, n_seqs, bridge, strand, reinterpret_cast<loc::Segment *>(segs), capacity, delta,
                                       source_bases + 1);
    });
}

size_t kbo_segments_work_bytes(size_t n_seqs, uint64_t total_bases) { return segments_work_bytes(n_seqs, total_bases); }

int kbo_segments_dev(kbo_index_t *idx, const uint8_t *d_ms, const uint32_t *d_lo, const uint64_t *d_offsets, size_t n_seqs, uint64_t total_bases,
                     uint32_t bridge, uint32_t strand, kbo_seq_segment *d_segs, size_t capacity, uint64_t *d_n_segs, uint32_t *d_delta,
                     void *d_work, size_t work_bytes, void *stream)
{
    return guarded([&] {
        KBO_REQUIRE(idx && d_ms && d_lo && d_offsets && d_n_segs && d_work && (d_segs || capacity == 0), KBO_E_BAD_ARG, "null argument");
        KBO_REQUIRE((((uintptr_t)d_lo | (uintptr_t)d_segs | (uintptr_t)d_delta) & 3) == 0 && (((uintptr_t)d_offsets | (uintptr_t)d_n_segs) & 7) == 0 &&
                        ((uintptr_t)d_work & 15) == 0,
                    KBO_E_BAD_ARG, "d_lo, d_segs and d_delta 4-byte, d_offsets and d_n_segs 8-byte, d_work 16-byte aligned");
        KBO_REQUIRE(bridge <= loc::kMaxBridge, KBO_E_BAD_ARG, "bridge above 255");
        KBO_REQUIRE(n_seqs > 0, KBO_E_EMPTY_QUERY, "empty batch");
        KBO_REQUIRE(total_bases + 16 <= (1ull << 32) && n_seqs < (1ull << 28), KBO_E_UNSUPPORTED, "a batch of 2^32 - 16 bases or 2^28 sequences, or more");
        require_unsharded(idx, "kbo_segments_dev");
        KBO_REQUIRE(has_positions(idx), KBO_E_BAD_ARG, "the handle has no positions (kbo_index_add_positions)");
        KBO_REQUIRE(work_bytes >= segments_work_bytes(n_seqs, total_bases), KBO_E_BAD_ARG, "work_bytes is smaller than kbo_segments_work_bytes()");
        const uint32_t *d_entries = positions_on(idx, current_device(), false);
        KBO_REQUIRE(d_entries, KBO_E_BAD_ARG, "the handle has no positions on the current device (kbo_index_positions_to_device)");
        segments_enqueue(d_entries, (uint32_t)idx->host.n_sets, (uint32_t)idx->host.k, (uint32_t)(kbo_index_source_bases(idx) + 1), d_ms, d_lo,
                         d_offsets, n_seqs, total_bases, bridge, strand, d_segs, capacity, d_n_segs, d_delta, d_work, static_cast<hipStream_t>(stream));
    });
}

size_t kbo_depth_work_bytes(const kbo_index_t *idx) { return kbo_index_has_positions(idx) ? (size_t)std::max<uint64_t>(16, loc::depth_work(kbo_index_source_bases(idx))) : 0; }

int kbo_depth_finish_dev(kbo_index_t *idx, const uint32_t *d_delta, uint32_t *d_depth, void *d_work, size_t work_bytes, void *stream)
{
    return guarded([&] {
        KBO_REQUIRE(idx && d_delta && d_depth && d_work, KBO_E_BAD_ARG, "null argument");
        KBO_REQUIRE((((uintptr_t)d_delta | (uintptr_t)d_depth) & 3) == 0 && ((uintptr_t)d_work & 15) == 0, KBO_E_BAD_ARG,
                    "d_delta and d_depth 4-byte, d_work 16-byte aligned");
        KBO_REQUIRE(kbo_index_has_positions(idx), KBO_E_BAD_ARG, "the handle has no positions (kbo_index_add_positions)");
        KBO_REQUIRE(work_bytes >= kbo_depth_work_bytes(idx), KBO_E_BAD_ARG, "work_bytes is smaller than kbo_depth_work_bytes()");
        HIP_OK(kbo::launch_depth_finish(d_delta, d_depth, kbo_index_source_bases(idx), d_work, static_cast<hipStream_t>(stream)));
    });
}

int kbo_segments_batch(kbo_index_t *idx, const uint8_t *concat, const uint64_t *offsets, size_t n_seqs, uint32_t bridge, int strands,
                       kbo_seq_segment **segs, uint64_t *n_segs, uint32_t *depth_out)
{
    return guarded([&] {
        KBO_REQUIRE(strands >= 1 && strands <= 3, KBO_E_BAD_ARG, "strands: KBO_STRAND_FWD, KBO_STRAND_REV or both");
        KBO_REQUIRE(idx && segs && n_segs, KBO_E_BAD_ARG, "null argument");
        KBO_REQUIRE(bridge <= loc::kMaxBridge, KBO_E_BAD_ARG, "bridge above 255");
        require_unsharded(idx, "kbo_segments_batch");
        KBO_REQUIRE(has_positions(idx), KBO_E_BAD_ARG, "the handle has no positions (kbo_index_add_positions)");
        check_batch(concat, offsets, n_seqs);
        const uint64_t total = offsets[n_seqs];
        KBO_REQUIRE(total + 16 <= (1ull << 32) && n_seqs < (1ull << 28), KBO_E_UNSUPPORTED, "a batch of 2^32 - 16 bases or 2^28 sequences, or more");
        // ---- the device from here on
        const int dev = current_device();
        const uint32_t *d_entries = positions_on(idx, dev, true);
        const uint32_t k = (uint32_t)idx->host.k, n_rows = (uint32_t)idx->host.n_sets;
        const uint64_t bases = kbo_index_source_bases(idx);
        const size_t pad = (size_t)loc::round16(total) + 64, wb = kbo_ms_work_bytes(n_seqs, total, 0, k), sb = segments_work_bytes(n_seqs, total);
        DevBuf q(pad), off((n_seqs + 1) * 8), hi(total * 4 + 16), work(wb), swork(sb), cnt(16), delta, depth, dwork, qr, ms[2], lo[2];
        HIP_OK(hipMemset(q.p, 0, pad));
        HIP_OK(hipMemcpy(q.p, concat, total, hipMemcpyHostToDevice));
        HIP_OK(hipMemcpy(off.p, offsets, (n_seqs + 1) * 8, hipMemcpyHostToDevice));
        if (depth_out) {
            delta.alloc((bases + 1) * 4);
            depth.alloc(bases * 4);
            dwork.alloc(kbo_depth_work_bytes(idx));
            HIP_OK(hipMemset(delta.p, 0, (bases + 1) * 4));
        }
        // the walk of every strand asked for, and its segments counted
        for (int st = 0; st < 2; st++) {
            if (!(strands & (1 << st))) continue;
            const uint8_t *d_q = q.as<uint8_t>();
            if (st) {
                qr.alloc(pad);
                HIP_OK(hipMemset(qr.p, 0, pad));
                ok(kbo_revcomp_batch_dev(q.as<uint8_t>(), off.as<uint64_t>(), n_seqs, total, 0, qr.as<uint8_t>(), nullptr));
                d_q = qr.as<uint8_t>();
            }
            ms[st].alloc(pad);
            lo[st].alloc(total * 4 + 16);
            ok(kbo_ms_batch_dev(idx, d_q, off.as<uint64_t>(), n_seqs, total, 0, ms[st].as<uint8_t>(), lo[st].as<uint32_t>(), hi.as<uint32_t>(), work.p,
                                wb, nullptr));
            segments_enqueue(d_entries, n_rows, k, (uint32_t)(bases + 1), ms[st].as<uint8_t>(), lo[st].as<uint32_t>(), off.as<uint64_t>(), n_seqs, total,
                             bridge, st + 1, nullptr, 0, cnt.as<uint64_t>() + st, nullptr, swork.p, nullptr);
        }
        uint64_t n[2] = {0, 0}, got[2];
        HIP_OK(hipMemcpy(got, cnt.p, 16, hipMemcpyDeviceToHost));
        for (int st = 0; st < 2; st++)
            if (strands & (1 << st)) n[st] = got[st];
        // the records, and the depth
        DevBuf recs((n[0] + n[1]) * sizeof(kbo_seq_segment));
        for (int st = 0; st < 2; st++) {
            if (!(strands & (1 << st))) continue;
            segments_enqueue(d_entries, n_rows, k, (uint32_t)(bases + 1), ms[st].as<uint8_t>(), lo[st].as<uint32_t>(), off.as<uint64_t>(), n_seqs, total,
                             bridge, st + 1, recs.as<kbo_seq_segment>() + (st ? n[0] : 0), n[st], cnt.as<uint64_t>() + st, delta.as<uint32_t>(), swork.p,
                             nullptr);
        }
        if (depth_out && bases) {
            HIP_OK(kbo::launch_depth_finish(delta.as<uint32_t>(), depth.as<uint32_t>(), bases, dwork.p, nullptr));
            HIP_OK(hipMemcpy(depth_out, depth.p, bases * 4, hipMemcpyDeviceToHost));
        }
        std::vector<kbo_seq_segment> both(n[0] + n[1]);
        if (!both.empty()) HIP_OK(hipMemcpy(both.data(), recs.p, both.size() * sizeof(kbo_seq_segment), hipMemcpyDeviceToHost));
        // (seq, '+' before '-', q_first): either strand's records are in (seq, q_first) order already
        MallocPtr<kbo_seq_segment> out = malloc_array<kbo_seq_segment>(both.size());
        std::merge(both.begin(), both.begin() + n[0], both.begin() + n[0], both.end(), out.get(),
                   [](const kbo_seq_segment &x, const kbo_seq_segment &y) { return x.seq != y.seq ? x.seq < y.seq : x.strand < y.strand; });
        *n_segs = both.size();
        *segs = out.release();
    });
}
