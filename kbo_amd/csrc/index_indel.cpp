// index_indel.cpp — kbo_hip.h "Indels": insertion and deletion events from the segments of a walked batch over device buffers
// (kbo_indels_dev), the events of any number of batches counted into sites (kbo_indel_sites_dev), their CPU restatements
// (kbo_indels_from_segments_host, kbo_indel_sites_host) and the host batch that composes the interval walk, the segments, the events,
// the depth and the sites (kbo_indels_batch).  The arithmetic is index_indel.hpp's, the kernels indel_kernels.hip's.
#include "../../include/kbo_hip.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <utility>
#include <vector>

#include "capi_internal.hpp"
#include "index_indel.hpp"

using namespace kbo_host;
namespace ind = kbo::idxindel;

static_assert(sizeof(kbo_indel_event) == sizeof(ind::Event) && sizeof(kbo_indel_site) == sizeof(ind::Site) && KBO_STRAND_REV == ind::kStrandRev &&
                  KBO_INDEL_INS == ind::kIns && KBO_INDEL_LONG == ind::kLong && KBO_INDEL_MINUS == ind::kMinus && KBO_INDEL_CODE_LEN == ind::kCodeLen,
              "the kernels' records");

namespace {

void ok(int rc)
{
    if (rc != KBO_OK) throw KboError(rc, last_error());
}

// the accessors index_indel.hpp names, over host arrays
struct HostSegs {
    const kbo_seq_segment *p;
    ind::Segment get(uint64_t x) const
    {
        const kbo_seq_segment &s = p[x];
        return ind::Segment{s.seq, s.strand, s.q_first, s.q_last, s.pos_first, s.pos_last, s.flags};
    }
};
struct HostOff {
    const uint64_t *p;
    uint64_t off(size_t s) const { return p[s]; }
};
struct HostBytes {
    const uint8_t *p;
    uint32_t at(uint64_t i) const { return p[i]; }
};
struct HostWords {
    const uint32_t *p;
    uint32_t at(uint64_t i) const { return p[i]; }
};
struct HostEvents {
    kbo_indel_event *p;
    void set(uint64_t x, const ind::Event &v) { std::memcpy(p + x, &v, sizeof v); }
};
struct HostSites {
    kbo_indel_site *p;
    void set(uint64_t x, const ind::Site &v) { std::memcpy(p + x, &v, sizeof v); }
};
struct HostKeys {
    const std::pair<uint64_t, uint64_t> *p;
    uint64_t w0(uint64_t i) const { return p[i].first; }
    uint64_t w1(uint64_t i) const { return p[i].second; }
};

struct OnDevice {
    const uint64_t *d_src_off;
    uint32_t n_src;
};
// the checks every device call ends with: unsharded, positions, positions on the current device
OnDevice require_positions_here(kbo_index *idx, const char *what)
{
    require_unsharded(idx, what);
    KBO_REQUIRE(kbo_index_has_positions(idx), KBO_E_BAD_ARG, "the handle has no positions (kbo_index_add_positions)");
    OnDevice d{nullptr, 0};
    d.d_src_off = source_offsets_on(idx, current_device(), &d.n_src);
    KBO_REQUIRE(d.d_src_off && d.n_src, KBO_E_BAD_ARG, "the handle has no positions on the current device (kbo_index_positions_to_device)");
    return d;
}

void events_enqueue(const OnDevice &d, uint32_t k, uint64_t source_bases, const uint8_t *d_concat, const uint64_t *d_offsets, size_t n_seqs, uint64_t total,
                    const kbo_seq_segment *d_segs, const uint64_t *d_n_segs, size_t capacity, bool skip_multi, uint32_t max_indel, kbo_indel_event *d_events,
                    size_t event_capacity, uint64_t *d_n_events, void *d_work, hipStream_t s)
{
    kbo::IndelEventArgs a;
    a.segs = reinterpret_cast<const uint32_t *>(d_segs);
    a.n_segs = d_n_segs;
    a.capacity = capacity;
    a.concat = d_concat;
    a.off = d_offsets;
    a.src_off = d.d_src_off;
    a.n_seqs = (uint32_t)n_seqs;
    a.n_src = d.n_src;
    a.k = k;
    a.max_indel = max_indel;
    a.total = total;
    a.source_bases = source_bases;
    a.skip_multi = skip_multi;
    a.events = d_events;
    a.event_capacity = event_capacity;
    a.n_events = d_n_events;
    a.work = d_work;
    HIP_OK(kbo::launch_indel_events(a, s));
}

void sites_enqueue(const OnDevice &d, uint64_t source_bases, const kbo_indel_event *d_events, const uint64_t *d_n_events, size_t event_capacity,
                   const uint32_t *d_depth, const ind::Thresholds &t, kbo_indel_site *d_sites, size_t capacity, uint64_t *d_n_sites, void *d_work,
                   hipStream_t s)
{
    kbo::IndelSitesArgs a;
    a.events = d_events;
    a.n_events = d_n_events;
    a.event_capacity = event_capacity;
    a.depth = d_depth;
    a.src_off = d.d_src_off;
    a.n_src = d.n_src;
    a.min_count = t.min_count;
    a.frac_num = t.frac_num;
    a.frac_den = t.frac_den;
    a.source_bases = source_bases;
    a.capacity = capacity;
    a.sites = d_sites;
    a.n_sites = d_n_sites;
    a.work = d_work;
    HIP_OK(kbo::launch_indel_sites(a, s));
}

void check_src_off(const uint64_t *src_off, size_t n_src)
{
    KBO_REQUIRE(src_off[0] == 0, KBO_E_BAD_ARG, "src_off[0] must be 0");
    for (size_t s = 0; s < n_src; s++) KBO_REQUIRE(src_off[s + 1] >= src_off[s], KBO_E_BAD_ARG, "src_off not monotone");
    KBO_REQUIRE(src_off[n_src] < kbo::idxlocate::kMaxSourceBases, KBO_E_UNSUPPORTED, "sources of 2^30 bases or more");
}

} // namespace

size_t kbo_indels_work_bytes(size_t n_segs_capacity) { return n_segs_capacity > ind::kMaxSegs ? 0 : (size_t)ind::event_work(n_segs_capacity).bytes; }

int kbo_indels_dev(kbo_index_t *idx, const uint8_t *d_concat, const uint64_t *d_offsets, size_t n_seqs, uint64_t total_bases, const kbo_seq_segment *d_segs,
                   const uint64_t *d_n_segs, size_t capacity, int skip_multi, uint32_t max_indel, kbo_indel_event *d_events, size_t event_capacity,
                   uint64_t *d_n_events, void *d_work, size_t work_bytes, void *stream)
{
    return guarded([&] {
        KBO_REQUIRE(idx && d_concat && d_offsets && d_n_segs && d_n_events && d_work && (d_segs || capacity == 0) && (d_events || event_capacity == 0),
                    KBO_E_BAD_ARG, "null argument");
        KBO_REQUIRE(((uintptr_t)d_segs & 3) == 0 && (((uintptr_t)d_offsets | (uintptr_t)d_n_segs | (uintptr_t)d_n_events) & 7) == 0 &&
                        (((uintptr_t)d_events | (uintptr_t)d_work) & 15) == 0,
                    KBO_E_BAD_ARG, "d_segs 4-byte, d_offsets, d_n_segs and d_n_events 8-byte, d_events and d_work 16-byte aligned");
        KBO_REQUIRE(max_indel > 0, KBO_E_BAD_ARG, "max_indel == 0");
        KBO_REQUIRE(n_seqs > 0, KBO_E_EMPTY_QUERY, "empty batch");
        KBO_REQUIRE(total_bases + 16 <= (1ull << 32) && n_seqs < ind::kMaxSeqs && capacity <= ind::kMaxSegs && event_capacity <= ind::kMaxEvents,
                    KBO_E_UNSUPPORTED, "a batch of 2^32 - 16 bases, 2^28 sequences, 2^32 - 1 records or 2^32 - 1 events, or more");
        const OnDevice d = require_positions_here(idx, "kbo_indels_dev");
        KBO_REQUIRE(work_bytes >= ind::event_work(capacity).bytes, KBO_E_BAD_ARG, "work_bytes is smaller than kbo_indels_work_bytes()");
        events_enqueue(d, (uint32_t)idx->host.k, kbo_index_source_bases(idx), d_concat, d_offsets, n_seqs, total_bases, d_segs, d_n_segs, capacity,
                       skip_multi != 0, max_indel, d_events, event_capacity, d_n_events, d_work, static_cast<hipStream_t>(stream));
    });
}

size_t kbo_indel_sites_work_bytes(size_t event_capacity) { return event_capacity > ind::kMaxEvents ? 0 : (size_t)ind::site_work(event_capacity).bytes; }

int kbo_indel_sites_dev(kbo_index_t *idx, const kbo_indel_event *d_events, const uint64_t *d_n_events, size_t event_capacity, const uint32_t *d_depth,
                        uint32_t min_count, uint32_t frac_num, uint32_t frac_den, kbo_indel_site *d_sites, size_t site_capacity, uint64_t *d_n_sites,
                        void *d_work, size_t work_bytes, void *stream)
{
    return guarded([&] {
        KBO_REQUIRE(idx && d_n_events && d_depth && d_n_sites && d_work && (d_events || event_capacity == 0) && (d_sites || site_capacity == 0), KBO_E_BAD_ARG,
                    "null argument");
        KBO_REQUIRE(((uintptr_t)d_depth & 3) == 0 && (((uintptr_t)d_n_events | (uintptr_t)d_n_sites) & 7) == 0 &&
                        (((uintptr_t)d_events | (uintptr_t)d_sites | (uintptr_t)d_work) & 15) == 0,
                    KBO_E_BAD_ARG, "d_depth 4-byte, d_n_events and d_n_sites 8-byte, d_events, d_sites and d_work 16-byte aligned");
        KBO_REQUIRE(min_count > 0 && frac_den > 0, KBO_E_BAD_ARG, "min_count == 0 or frac_den == 0");
        KBO_REQUIRE(event_capacity <= ind::kMaxEvents, KBO_E_UNSUPPORTED, "2^32 - 1 events or more");
        const OnDevice d = require_positions_here(idx, "kbo_indel_sites_dev");
        KBO_REQUIRE(work_bytes >= ind::site_work(event_capacity).bytes, KBO_E_BAD_ARG, "work_bytes is smaller than kbo_indel_sites_work_bytes()");
        sites_enqueue(d, kbo_index_source_bases(idx), d_events, d_n_events, event_capacity, d_depth, ind::Thresholds{min_count, frac_num, frac_den}, d_sites,
                      site_capacity, d_n_sites, d_work, static_cast<hipStream_t>(stream));
    });
}

int kbo_indels_from_segments_host(const kbo_seq_segment *segs, uint64_t n_segs, const uint8_t *concat, const uint64_t *offsets, size_t n_seqs,
                                  uint64_t total_bases, uint32_t k, int skip_multi, uint32_t max_indel, const uint64_t *src_off, size_t n_src,
                                  kbo_indel_event *events, size_t event_capacity, uint64_t *n_events, uint64_t *n_complex)
{
    return guarded([&] {
        KBO_REQUIRE(offsets && src_off && n_events && (segs || n_segs == 0) && (concat || total_bases == 0) && (events || event_capacity == 0) && k > 0 &&
                        n_src > 0,
                    KBO_E_BAD_ARG, "null argument, k == 0 or no source");
        KBO_REQUIRE(max_indel > 0, KBO_E_BAD_ARG, "max_indel == 0");
        KBO_REQUIRE(n_seqs > 0, KBO_E_EMPTY_QUERY, "no sequences");
        KBO_REQUIRE(total_bases + 16 <= (1ull << 32) && n_seqs < ind::kMaxSeqs && n_segs <= ind::kMaxSegs && event_capacity <= ind::kMaxEvents &&
                        n_src < 0xFFFFFFFFull,
                    KBO_E_UNSUPPORTED, "a batch of 2^32 - 16 bases, 2^28 sequences, 2^32 - 1 records, events or sources, or more");
        check_src_off(src_off, n_src);
        HostEvents out{events};
        *n_events += ind::events_serial(HostSegs{segs}, n_segs, HostOff{offsets}, (uint32_t)n_seqs, total_bases, k, skip_multi != 0, max_indel, src_off[n_src],
                                        HostOff{src_off}, (uint32_t)n_src, HostBytes{concat}, out, *n_events, event_capacity, n_complex);
    });
}

int kbo_indel_sites_host(const kbo_indel_event *events, uint64_t n_events, size_t event_capacity, const uint32_t *depth, const uint64_t *src_off,
                         size_t n_src, uint32_t min_count, uint32_t frac_num, uint32_t frac_den, kbo_indel_site *sites, size_t site_capacity,
                         uint64_t *n_sites)
{
    return guarded([&] {
        KBO_REQUIRE(src_off && n_sites && n_src > 0 && (events || event_capacity == 0) && (sites || site_capacity == 0), KBO_E_BAD_ARG,
                    "null argument or no source");
        KBO_REQUIRE(min_count > 0 && frac_den > 0, KBO_E_BAD_ARG, "min_count == 0 or frac_den == 0");
        KBO_REQUIRE(event_capacity <= ind::kMaxEvents && n_src < 0xFFFFFFFFull, KBO_E_UNSUPPORTED, "2^32 - 1 events or sources, or more");
        check_src_off(src_off, n_src);
        const uint64_t bases = src_off[n_src], n = std::min<uint64_t>(n_events, event_capacity);
        KBO_REQUIRE(depth || bases == 0, KBO_E_BAD_ARG, "null argument");
        std::vector<std::pair<uint64_t, uint64_t>> keys;
        keys.reserve((size_t)n);
        for (uint64_t i = 0; i < n; i++) {
            uint64_t w0, w1;
            if (ind::event_key(ind::Event{events[i].pos, events[i].kind_len, events[i].code, events[i].flags}, bases, &w0, &w1)) keys.emplace_back(w0, w1);
        }
        std::stable_sort(keys.begin(), keys.end(), [](const auto &a, const auto &b) { return ind::key_less(a.first, a.second, b.first, b.second); });
        HostSites out{sites};
        *n_sites = ind::sites_sorted_serial(HostKeys{keys.data()}, keys.size(), HostWords{depth}, bases, HostOff{src_off}, (uint32_t)n_src,
                                            ind::Thresholds{min_count, frac_num, frac_den}, out, site_capacity);
    });
}

int kbo_indels_batch(kbo_index_t *idx, const uint8_t *concat, const uint64_t *offsets, size_t n_seqs, uint32_t bridge, int strands, int skip_multi,
                     uint32_t max_indel, uint32_t min_count, uint32_t frac_num, uint32_t frac_den, kbo_indel_site **sites, uint64_t *n_sites,
                     uint32_t *depth_out)
{
    return guarded([&] {
        KBO_REQUIRE(strands >= 1 && strands <= 3, KBO_E_BAD_ARG, "strands: KBO_STRAND_FWD, KBO_STRAND_REV or both");
        KBO_REQUIRE(idx && sites && n_sites, KBO_E_BAD_ARG, "null argument");
        KBO_REQUIRE(bridge <= kbo::idxlocate::kMaxBridge, KBO_E_BAD_ARG, "bridge above 255");
        KBO_REQUIRE(max_indel > 0 && min_count > 0 && frac_den > 0, KBO_E_BAD_ARG, "max_indel == 0, min_count == 0 or frac_den == 0");
        require_unsharded(idx, "kbo_indels_batch");
        KBO_REQUIRE(kbo_index_has_positions(idx), KBO_E_BAD_ARG, "the handle has no positions (kbo_index_add_positions)");
        check_batch(concat, offsets, n_seqs);
        const uint64_t total = offsets[n_seqs];
        KBO_REQUIRE(total + 16 <= (1ull << 32) && n_seqs < ind::kMaxSeqs, KBO_E_UNSUPPORTED, "a batch of 2^32 - 16 bases or 2^28 sequences, or more");
        // ---- the device from here on
        ok(kbo_index_positions_to_device(idx, -1));
        const OnDevice d = require_positions_here(idx, "kbo_indels_batch");
        const uint32_t k = (uint32_t)idx->host.k;
        const uint64_t bases = kbo_index_source_bases(idx);
        const size_t pad = (size_t)ind::round16(total) + 64, wb = kbo_ms_work_bytes(n_seqs, total, 0, k), sb = kbo_segments_work_bytes(n_seqs, total);
        DevBuf q(pad), off((n_seqs + 1) * 8), ms(pad), lo(total * 4 + 16), hi(total * 4 + 16), work(wb), swork(sb), cnt(16), ecnt(16), delta((bases + 1) * 4),
            depth(bases * 4 + 16), dwork(kbo_depth_work_bytes(idx)), qr, recs[2], ework, events, twork, out;
        uint64_t n_recs[2] = {0, 0};
        HIP_OK(hipMemset(q.p, 0, pad));
        if (total) HIP_OK(hipMemcpy(q.p, concat, total, hipMemcpyHostToDevice));
        HIP_OK(hipMemcpy(off.p, offsets, (n_seqs + 1) * 8, hipMemcpyHostToDevice));
        HIP_OK(hipMemset(delta.p, 0, (bases + 1) * 4));
        HIP_OK(hipMemset(ecnt.p, 0, 16));
        if (strands & 2) {
            qr.alloc(pad);
            HIP_OK(hipMemset(qr.p, 0, pad));
            if (total) ok(kbo_revcomp_batch_dev(q.as<uint8_t>(), off.as<uint64_t>(), n_seqs, total, 0, qr.as<uint8_t>(), nullptr));
        }
        // per strand: the walk, its segments counted, then written at their number with the strand's delta.  A pair of records gives
        // at most one event, so the list is sized by the records: events are written once
        for (int st = 0; st < 2 && total; st++) {
            if (!(strands & (1 << st))) continue;
            const uint8_t *d_q = st ? qr.as<uint8_t>() : q.as<uint8_t>();
            ok(kbo_ms_batch_dev(idx, d_q, off.as<uint64_t>(), n_seqs, total, 0, ms.as<uint8_t>(), lo.as<uint32_t>(), hi.as<uint32_t>(), work.p, wb, nullptr));
            ok(kbo_segments_dev(idx, ms.as<uint8_t>(), lo.as<uint32_t>(), off.as<uint64_t>(), n_seqs, total, bridge, (uint32_t)st + 1u, nullptr, 0,
                                cnt.as<uint64_t>(), nullptr, swork.p, sb, nullptr));
            uint64_t n = 0;
            HIP_OK(hipMemcpy(&n, cnt.p, 8, hipMemcpyDeviceToHost));
            KBO_REQUIRE(n <= ind::kMaxSegs, KBO_E_UNSUPPORTED, "2^32 - 1 segments or more");
            recs[st].alloc((size_t)n * sizeof(kbo_seq_segment) + 16);
            ok(kbo_segments_dev(idx, ms.as<uint8_t>(), lo.as<uint32_t>(), off.as<uint64_t>(), n_seqs, total, bridge, (uint32_t)st + 1u,
                                recs[st].as<kbo_seq_segment>(), (size_t)n, cnt.as<uint64_t>(), delta.as<uint32_t>(), swork.p, sb, nullptr));
            n_recs[st] = n;
        }
        const uint64_t cap = n_recs[0] + n_recs[1];
        KBO_REQUIRE(cap <= ind::kMaxEvents, KBO_E_UNSUPPORTED, "2^32 - 1 segments or more");
        events.alloc((size_t)cap * sizeof(kbo_indel_event) + 16);
        ework.alloc((size_t)ind::event_work(std::max(n_recs[0], n_recs[1])).bytes);
        for (int st = 0; st < 2; st++) {
            if (!n_recs[st]) continue;
            HIP_OK(hipMemcpy(cnt.p, &n_recs[st], 8, hipMemcpyHostToDevice));
            events_enqueue(d, k, bases, st ? qr.as<uint8_t>() : q.as<uint8_t>(), off.as<uint64_t>(), n_seqs, total, recs[st].as<kbo_seq_segment>(),
                           cnt.as<uint64_t>(), (size_t)n_recs[st], skip_multi != 0, max_indel, events.as<kbo_indel_event>(), (size_t)cap, ecnt.as<uint64_t>(),
                           ework.p, nullptr);
            HIP_OK(hipStreamSynchronize(nullptr)); // (cnt is written again for the next strand)
        }
        ok(kbo_depth_finish_dev(idx, delta.as<uint32_t>(), depth.as<uint32_t>(), dwork.p, kbo_depth_work_bytes(idx), nullptr));
        // the list cut to its count, the sites counted, then written at their number
        uint64_t n_ev = 0;
        HIP_OK(hipMemcpy(&n_ev, ecnt.p, 8, hipMemcpyDeviceToHost));
        twork.alloc((size_t)ind::site_work(n_ev).bytes);
        const ind::Thresholds t{min_count, frac_num, frac_den};
        sites_enqueue(d, bases, events.as<kbo_indel_event>(), ecnt.as<uint64_t>(), (size_t)n_ev, depth.as<uint32_t>(), t, nullptr, 0, cnt.as<uint64_t>(), twork.p,
                      nullptr);
        uint64_t n = 0;
        HIP_OK(hipMemcpy(&n, cnt.p, 8, hipMemcpyDeviceToHost));
        out.alloc((size_t)n * sizeof(kbo_indel_site) + 16);
        sites_enqueue(d, bases, events.as<kbo_indel_event>(), ecnt.as<uint64_t>(), (size_t)n_ev, depth.as<uint32_t>(), t, out.as<kbo_indel_site>(), (size_t)n,
                      cnt.as<uint64_t>(), twork.p, nullptr);
        MallocPtr<kbo_indel_site> host = malloc_array<kbo_indel_site>((size_t)n);
        if (n) HIP_OK(hipMemcpy(host.get(), out.p, (size_t)n * sizeof(kbo_indel_site), hipMemcpyDeviceToHost));
        if (depth_out && bases) HIP_OK(hipMemcpy(depth_out, depth.p, bases * 4, hipMemcpyDeviceToHost));
        *n_sites = n;
        *sites = host.release();
    });
}
