// index_place.cpp — kbo_hip.h "Placement": one record per sequence from the segments of a walked batch over device buffers
// (kbo_place_dev), its CPU restatement (kbo_place_from_segments_host) and the host batch that composes the interval walk, the segments
// and the placement per strand (kbo_place_batch).  The arithmetic is index_place.hpp's, the kernels place_kernels.hip's.
#include "../../include/kbo_hip.h"

#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "capi_internal.hpp"
#include "index_place.hpp"

using namespace kbo_host;
namespace plc = kbo::idxplace;

static_assert(sizeof(kbo_seq_place) == 48 && sizeof(plc::Place) == 48 && sizeof(kbo_seq_segment) == sizeof(plc::Segment), "the kernels' records");
static_assert(plc::kPlaceNone == KBO_PLACE_NONE && plc::kWindow == KBO_PLACE_WINDOW && plc::kLaneMax == KBO_PLACE_LANE_MAX &&
                  plc::kPlaceRev == KBO_PLACE_REV && plc::kPlaceSpills == KBO_PLACE_SPILLS,
              "kbo_hip.h states the kernels' constants");

namespace {

void ok(int rc)
{
    if (rc != KBO_OK) throw KboError(rc, last_error());
}

size_t place_work_bytes(size_t n_seqs, uint64_t capacity)
{
    if (n_seqs == 0 || n_seqs >= plc::kMaxSeqs || capacity > plc::kMaxSegs) return 0;
    return (size_t)plc::place_work(n_seqs, capacity).bytes;
}

// the accessors index_place.hpp names, over host arrays
struct HostSegs {
    const kbo_seq_segment *p;
    plc::Segment get(uint64_t x) const
    {
        const kbo_seq_segment &s = p[x];
        return plc::Segment{s.seq, s.strand, s.q_first, s.q_last, s.pos_first, s.pos_last, s.flags};
    }
};
struct HostOff {
    const uint64_t *p;
    uint64_t off(size_t s) const { return p[s]; }
};
struct HostWork {
    std::vector<uint32_t> b, e, s;
    uint32_t begin(uint32_t q) const { return b[q]; }
    uint32_t end(uint32_t q) const { return e[q]; }
    uint32_t src(uint32_t x) const { return s[x]; }
    void set_begin(uint32_t q, uint32_t v) { b[q] = v; }
    void set_end(uint32_t q, uint32_t v) { e[q] = v; }
    void set_src(uint32_t x, uint32_t v) { s[x] = v; }
};
struct HostRing {
    plc::State st[plc::kWindow];
    plc::State get(uint32_t slot) const { return st[slot]; }
    void set(uint32_t slot, const plc::State &v) { st[slot] = v; }
};
struct HostPlaces {
    kbo_seq_place *p;
    plc::Place get(uint32_t s) const
    {
        plc::Place v;
        std::memcpy(&v, p + s, sizeof v);
        return v;
    }
    void set(uint32_t s, const plc::Place &v) { std::memcpy(p + s, &v, sizeof v); }
};

void place_enqueue(const uint64_t *d_src_off, uint32_t n_src, uint32_t k, const kbo_seq_segment *d_segs, const uint64_t *d_n_segs, size_t capacity,
                   size_t n_seqs, uint32_t max_gap, uint32_t max_indel, bool merge, kbo_seq_place *d_place, void *d_work, hipStream_t s)
{
    kbo::PlaceArgs a;
    a.segs = reinterpret_cast<const uint32_t *>(d_segs);
    a.n_segs = d_n_segs;
    a.capacity = capacity;
    a.src_off = d_src_off;
    a.n_seqs = (uint32_t)n_seqs;
    a.n_src = n_src;
    a.k = k;
    a.max_gap = max_gap;
    a.max_indel = max_indel;
    a.merge = merge;
    a.place = d_place;
    a.work = d_work;
    HIP_OK(kbo::launch_place(a, s));
}

} // namespace

size_t kbo_place_work_bytes(size_t n_seqs, size_t n_segs_capacity) { return place_work_bytes(n_seqs, n_segs_capacity); }

int kbo_place_dev(kbo_index_t *idx, const kbo_seq_segment *d_segs, const uint64_t *d_n_segs, size_t capacity, size_t n_seqs, uint32_t max_gap,
                  uint32_t max_indel, int merge, kbo_seq_place *d_place, void *d_work, size_t work_bytes, void *stream)
{
    return guarded([&] {
        KBO_REQUIRE(idx && d_n_segs && d_place && d_work && (d_segs || capacity == 0), KBO_E_BAD_ARG, "null argument");
        KBO_REQUIRE(((uintptr_t)d_segs & 3) == 0 && ((uintptr_t)d_n_segs & 7) == 0 && (((uintptr_t)d_place | (uintptr_t)d_work) & 15) == 0, KBO_E_BAD_ARG,
                    "d_segs 4-byte, d_n_segs 8-byte, d_place and d_work 16-byte aligned");
        KBO_REQUIRE(n_seqs > 0, KBO_E_EMPTY_QUERY, "empty batch");
        KBO_REQUIRE(n_seqs < plc::kMaxSeqs && capacity <= plc::kMaxSegs, KBO_E_UNSUPPORTED, "2^28 sequences or 2^32 - 1 records, or more");
        require_unsharded(idx, "kbo_place_dev");
        KBO_REQUIRE(kbo_index_has_positions(idx), KBO_E_BAD_ARG, "the handle has no positions (kbo_index_add_positions)");
        uint32_t n_src = 0;
        const uint64_t *d_src_off = source_offsets_on(idx, current_device(), &n_src);
        KBO_REQUIRE(d_src_off && n_src, KBO_E_BAD_ARG, "the handle has no positions on the current device (kbo_index_positions_to_device)");
        KBO_REQUIRE(work_bytes >= place_work_bytes(n_seqs, capacity), KBO_E_BAD_ARG, "work_bytes is smaller than kbo_place_work_bytes()");
        place_enqueue(d_src_off, n_src, (uint32_t)idx->host.k, d_segs, d_n_segs, capacity, n_seqs, max_gap, max_indel, merge != 0, d_place, d_work,
                      static_cast<hipStream_t>(stream));
    });
}

int kbo_place_from_segments_host(const kbo_seq_segment *segs, uint64_t n_segs, size_t n_seqs, const uint64_t *src_off, size_t n_src, uint32_t k,
                                 uint32_t max_gap, uint32_t max_indel, int merge, kbo_seq_place *place)
{
    return guarded([&] {
        KBO_REQUIRE(src_off && place && (segs || n_segs == 0) && k > 0 && n_src > 0, KBO_E_BAD_ARG, "null argument, k == 0 or no source");
        KBO_REQUIRE(n_seqs > 0, KBO_E_EMPTY_QUERY, "no sequences");
        KBO_REQUIRE(n_seqs < plc::kMaxSeqs && n_segs <= plc::kMaxSegs && n_src < 0xFFFFFFFFull, KBO_E_UNSUPPORTED,
                    "2^28 sequences, 2^32 - 1 records or sources, or more");
        KBO_REQUIRE(src_off[0] == 0, KBO_E_BAD_ARG, "src_off[0] must be 0");
        for (size_t s = 0; s < n_src; s++) KBO_REQUIRE(src_off[s + 1] >= src_off[s], KBO_E_BAD_ARG, "src_off not monotone");
        HostWork w;
        w.b.resize(n_seqs);
        w.e.resize(n_seqs);
        w.s.resize(n_segs);
        HostRing ring;
        HostPlaces out{place};
        plc::place_serial(HostSegs{segs}, (uint32_t)n_segs, (uint32_t)n_seqs, HostOff{src_off}, (uint32_t)n_src, plc::Limits{k, max_gap, max_indel},
                          merge != 0, w, ring, out);
    });
}

int kbo_place_batch(kbo_index_t *idx, const uint8_t *concat, const uint64_t *offsets, size_t n_seqs, uint32_t bridge, int strands, uint32_t max_gap,
                    uint32_t max_indel, kbo_seq_place *place_out)
{
    return guarded([&] {
        KBO_REQUIRE(strands >= 1 && strands <= 3, KBO_E_BAD_ARG, "strands: KBO_STRAND_FWD, KBO_STRAND_REV or both");
        KBO_REQUIRE(idx && place_out, KBO_E_BAD_ARG, "null argument");
        KBO_REQUIRE(bridge <= kbo::idxlocate::kMaxBridge, KBO_E_BAD_ARG, "bridge above 255");
        require_unsharded(idx, "kbo_place_batch");
        KBO_REQUIRE(kbo_index_has_positions(idx), KBO_E_BAD_ARG, "the handle has no positions (kbo_index_add_positions)");
        check_batch(concat, offsets, n_seqs);
        const uint64_t total = offsets[n_seqs];
        KBO_REQUIRE(total + 16 <= (1ull << 32) && n_seqs < plc::kMaxSeqs, KBO_E_UNSUPPORTED, "a batch of 2^32 - 16 bases or 2^28 sequences, or more");
        // ---- the device from here on
        ok(kbo_index_positions_to_device(idx, -1));
        uint32_t n_src = 0;
        const uint64_t *d_src_off = source_offsets_on(idx, current_device(), &n_src);
        KBO_REQUIRE(d_src_off && n_src, KBO_E_HIP, "the source offsets did not reach the device");
        const uint32_t k = (uint32_t)idx->host.k;
        const size_t pad = (size_t)plc::round16(total) + 64, wb = kbo_ms_work_bytes(n_seqs, total, 0, k), sb = kbo_segments_work_bytes(n_seqs, total);
        DevBuf q(pad), off((n_seqs + 1) * 8), ms(pad), lo(total * 4 + 16), hi(total * 4 + 16), work(wb), swork(sb), cnt(16), place(n_seqs * sizeof(kbo_seq_place)), qr,
            recs, pwork;
        HIP_OK(hipMemset(q.p, 0, pad));
        if (total) HIP_OK(hipMemcpy(q.p, concat, total, hipMemcpyHostToDevice));
        HIP_OK(hipMemcpy(off.p, offsets, (n_seqs + 1) * 8, hipMemcpyHostToDevice));
        bool merge = false;
        for (int st = 0; st < 2; st++) {
            if (!(strands & (1 << st))) continue;
            const uint8_t *d_q = q.as<uint8_t>();
            if (st) {
                qr.alloc(pad);
                HIP_OK(hipMemset(qr.p, 0, pad));
                ok(kbo_revcomp_batch_dev(q.as<uint8_t>(), off.as<uint64_t>(), n_seqs, total, 0, qr.as<uint8_t>(), nullptr));
                d_q = qr.as<uint8_t>();
            }
            // the walk, its segments counted, then written at their number
            ok(kbo_ms_batch_dev(idx, d_q, off.as<uint64_t>(), n_seqs, total, 0, ms.as<uint8_t>(), lo.as<uint32_t>(), hi.as<uint32_t>(), work.p, wb, nullptr));
            ok(kbo_segments_dev(idx, ms.as<uint8_t>(), lo.as<uint32_t>(), off.as<uint64_t>(), n_seqs, total, bridge, (uint32_t)st + 1u, nullptr, 0,
                                cnt.as<uint64_t>(), nullptr, swork.p, sb, nullptr));
            uint64_t n = 0;
            HIP_OK(hipMemcpy(&n, cnt.p, 8, hipMemcpyDeviceToHost));
            KBO_REQUIRE(n <= plc::kMaxSegs, KBO_E_UNSUPPORTED, "2^32 - 1 segments or more");
            recs.ensure((size_t)n * sizeof(kbo_seq_segment));
            ok(kbo_segments_dev(idx, ms.as<uint8_t>(), lo.as<uint32_t>(), off.as<uint64_t>(), n_seqs, total, bridge, (uint32_t)st + 1u,
                                recs.as<kbo_seq_segment>(), (size_t)n, cnt.as<uint64_t>(), nullptr, swork.p, sb, nullptr));
            pwork.ensure(place_work_bytes(n_seqs, n));
            place_enqueue(d_src_off, n_src, k, recs.as<kbo_seq_segment>(), cnt.as<uint64_t>(), (size_t)n, n_seqs, max_gap, max_indel, merge,
                          place.as<kbo_seq_place>(), pwork.p, nullptr);
            merge = true;
        }
        HIP_OK(hipMemcpy(place_out, place.p, n_seqs * sizeof(kbo_seq_place), hipMemcpyDeviceToHost));
    });
}
