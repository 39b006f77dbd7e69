// index_pileup.cpp — kbo_hip.h "Pileup": allele counts per source base from the segments of a walked batch over device buffers
// (kbo_pileup_dev), the candidate sites of a pile (kbo_pileup_sites_dev), their CPU restatements (kbo_pileup_from_segments_host,
// kbo_pileup_sites_host) and the host batch that composes the interval walk, the segments, the pile, the depth and the sites
// (kbo_pileup_batch).  The arithmetic is index_pileup.hpp's, the kernels pileup_kernels.hip's.
#include "../../include/kbo_hip.h"

#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "capi_internal.hpp"
#include "index_pileup.hpp"

using namespace kbo_host;
namespace pil = kbo::idxpile;

static_assert(sizeof(kbo_pile_site) == 32 && sizeof(pil::Site) == 32 && sizeof(kbo_seq_segment) == sizeof(pil::Segment), "the kernels' records");

namespace {

void ok(int rc)
{
    if (rc != KBO_OK) throw KboError(rc, last_error());
}

size_t sites_work_bytes(const kbo_index *idx) { return kbo_index_has_positions(idx) ? (size_t)pil::sites_work(kbo_index_source_bases(idx)) : 0; }

// the accessors index_pileup.hpp names, over host arrays
struct HostSegs {
    const kbo_seq_segment *p;
    pil::Segment get(uint64_t x) const
    {
        const kbo_seq_segment &s = p[x];
        return pil::Segment{s.seq, s.strand, s.q_first, s.q_last, s.pos_first, s.pos_last, s.flags};
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
struct HostPile {
    uint32_t *p;
    void add(uint64_t word) { p[word]++; }
};
struct HostSites {
    kbo_pile_site *p;
    void set(uint64_t x, const pil::Site &v) { std::memcpy(p + x, &v, sizeof v); }
};

void pileup_enqueue(uint32_t k, uint64_t source_bases, const uint8_t *d_concat, const uint8_t *d_ms, const uint64_t *d_offsets, size_t n_seqs,
                    uint64_t total, const kbo_seq_segment *d_segs, const uint64_t *d_n_segs, size_t capacity, bool skip_multi, uint32_t *d_pile,
                    hipStream_t s)
{
    kbo::PileupArgs a;
    a.segs = reinterpret_cast<const uint32_t *>(d_segs);
    a.n_segs = d_n_segs;
    a.capacity = capacity;
    a.concat = d_concat;
    a.ms = d_ms;
    a.off = d_offsets;
    a.n_seqs = (uint32_t)n_seqs;
    a.k = k;
    a.total = total;
    a.source_bases = source_bases;
    a.skip_multi = skip_multi;
    a.pile = d_pile;
    HIP_OK(kbo::launch_pileup(a, s));
}

void sites_enqueue(const uint64_t *d_src_off, uint32_t n_src, uint64_t source_bases, const uint32_t *d_pile, const uint32_t *d_depth,
                   const pil::Thresholds &t, kbo_pile_site *d_sites, size_t capacity, uint64_t *d_n_sites, void *d_work, hipStream_t s)
{
    kbo::PileupSitesArgs a;
    a.pile = d_pile;
    a.depth = d_depth;
    a.src_off = d_src_off;
    a.n_src = n_src;
    a.min_count = t.min_count;
    a.frac_num = t.frac_num;
    a.frac_den = t.frac_den;
    a.source_bases = source_bases;
    a.capacity = capacity;
    a.sites = d_sites;
    a.n_sites = d_n_sites;
    a.work = d_work;
    HIP_OK(kbo::launch_pileup_sites(a, s));
}

} // namespace

int kbo_pileup_dev(kbo_index_t *idx, const uint8_t *d_concat, const uint8_t *d_ms, const uint64_t *d_offsets, size_t n_seqs, uint64_t total_bases,
                   const kbo_seq_segment *d_segs, const uint64_t *d_n_segs, size_t capacity, int skip_multi, uint32_t *d_pile, void *stream)
{
    return guarded([&] {
        KBO_REQUIRE(idx && d_concat && d_ms && d_offsets && d_n_segs && d_pile && (d_segs || capacity == 0), KBO_E_BAD_ARG, "null argument");
        KBO_REQUIRE(((uintptr_t)d_segs & 3) == 0 && (((uintptr_t)d_offsets | (uintptr_t)d_n_segs) & 7) == 0 && ((uintptr_t)d_pile & 15) == 0, KBO_E_BAD_ARG,
                    "d_segs 4-byte, d_offsets and d_n_segs 8-byte, d_pile 16-byte aligned");
        KBO_REQUIRE(n_seqs > 0, KBO_E_EMPTY_QUERY, "empty batch");
        KBO_REQUIRE(total_bases + 16 <= (1ull << 32) && n_seqs < pil::kMaxSeqs && capacity <= pil::kMaxSegs, KBO_E_UNSUPPORTED,
                    "a batch of 2^32 - 16 bases, 2^28 sequences or 2^32 - 1 records, or more");
        require_unsharded(idx, "kbo_pileup_dev");
        KBO_REQUIRE(kbo_index_has_positions(idx), KBO_E_BAD_ARG, "the handle has no positions (kbo_index_add_positions)");
        uint32_t n_src = 0;
        KBO_REQUIRE(source_offsets_on(idx, current_device(), &n_src) && n_src, KBO_E_BAD_ARG,
                    "the handle has no positions on the current device (kbo_index_positions_to_device)");
        pileup_enqueue((uint32_t)idx->host.k, kbo_index_source_bases(idx), d_concat, d_ms, d_offsets, n_seqs, total_bases, d_segs, d_n_segs, capacity,
                       skip_multi != 0, d_pile, static_cast<hipStream_t>(stream));
    });
}

size_t kbo_pileup_sites_work_bytes(const kbo_index_t *idx) { return sites_work_bytes(idx); }

int kbo_pileup_sites_dev(kbo_index_t *idx, const uint32_t *d_pile, const uint32_t *d_depth, uint32_t min_count, uint32_t frac_num, uint32_t frac_den,
                         kbo_pile_site *d_sites, size_t capacity, uint64_t *d_n_sites, void *d_work, size_t work_bytes, void *stream)
{
    return guarded([&] {
        KBO_REQUIRE(idx && d_pile && d_depth && d_n_sites && d_work && (d_sites || capacity == 0), KBO_E_BAD_ARG, "null argument");
        KBO_REQUIRE(((uintptr_t)d_depth & 3) == 0 && ((uintptr_t)d_n_sites & 7) == 0 && (((uintptr_t)d_pile | (uintptr_t)d_sites | (uintptr_t)d_work) & 15) == 0,
                    KBO_E_BAD_ARG, "d_depth 4-byte, d_n_sites 8-byte, d_pile, d_sites and d_work 16-byte aligned");
        KBO_REQUIRE(min_count > 0 && frac_den > 0, KBO_E_BAD_ARG, "min_count == 0 or frac_den == 0");
        require_unsharded(idx, "kbo_pileup_sites_dev");
        KBO_REQUIRE(kbo_index_has_positions(idx), KBO_E_BAD_ARG, "the handle has no positions (kbo_index_add_positions)");
        uint32_t n_src = 0;
        const uint64_t *d_src_off = source_offsets_on(idx, current_device(), &n_src);
        KBO_REQUIRE(d_src_off && n_src, KBO_E_BAD_ARG, "the handle has no positions on the current device (kbo_index_positions_to_device)");
        KBO_REQUIRE(work_bytes >= sites_work_bytes(idx), KBO_E_BAD_ARG, "work_bytes is smaller than kbo_pileup_sites_work_bytes()");
        sites_enqueue(d_src_off, n_src, kbo_index_source_bases(idx), d_pile, d_depth, pil::Thresholds{min_count, frac_num, frac_den}, d_sites, capacity,
                      d_n_sites, d_work, static_cast<hipStream_t>(stream));
    });
}

int kbo_pileup_from_segments_host(const kbo_seq_segment *segs, uint64_t n_segs, const uint8_t *concat, const uint8_t *ms, const uint64_t *offsets,
                                  size_t n_seqs, uint64_t total_bases, uint32_t k, int skip_multi, uint32_t *pile, uint64_t source_bases,
                                  uint64_t *n_bridged)
{
    return guarded([&] {
        KBO_REQUIRE(offsets && (segs || n_segs == 0) && ((concat && ms) || total_bases == 0) && (pile || source_bases == 0) && k > 0, KBO_E_BAD_ARG,
                    "null argument or k == 0");
        KBO_REQUIRE(n_seqs > 0, KBO_E_EMPTY_QUERY, "no sequences");
        KBO_REQUIRE(total_bases + 16 <= (1ull << 32) && n_seqs < pil::kMaxSeqs && n_segs <= pil::kMaxSegs && source_bases < kbo::idxlocate::kMaxSourceBases,
                    KBO_E_UNSUPPORTED, "a batch of 2^32 - 16 bases, 2^28 sequences or 2^32 - 1 records, sources of 2^30 bases, or more");
        HostPile out{pile};
        const uint64_t n = pil::pileup_serial(HostSegs{segs}, n_segs, HostOff{offsets}, (uint32_t)n_seqs, total_bases, k, skip_multi != 0, source_bases,
                                              HostBytes{ms}, HostBytes{concat}, out);
        if (n_bridged) *n_bridged = n;
    });
}

int kbo_pileup_sites_host(const uint32_t *pile, const uint32_t *depth, uint64_t source_bases, const uint64_t *src_off, size_t n_src, uint32_t min_count,
                          uint32_t frac_num, uint32_t frac_den, kbo_pile_site *sites, size_t capacity, uint64_t *n_sites)
{
    return guarded([&] {
        KBO_REQUIRE(((pile && depth) || source_bases == 0) && src_off && n_sites && (sites || capacity == 0) && n_src > 0, KBO_E_BAD_ARG,
                    "null argument or no source");
        KBO_REQUIRE(min_count > 0 && frac_den > 0, KBO_E_BAD_ARG, "min_count == 0 or frac_den == 0");
        KBO_REQUIRE(source_bases < kbo::idxlocate::kMaxSourceBases && n_src < 0xFFFFFFFFull, KBO_E_UNSUPPORTED, "sources of 2^30 bases or 2^32 - 1 sources, or more");
        KBO_REQUIRE(src_off[0] == 0, KBO_E_BAD_ARG, "src_off[0] must be 0");
        for (size_t s = 0; s < n_src; s++) KBO_REQUIRE(src_off[s + 1] >= src_off[s], KBO_E_BAD_ARG, "src_off not monotone");
        HostSites out{sites};
        *n_sites = pil::sites_serial(HostWords{pile}, HostWords{depth}, source_bases, HostOff{src_off}, (uint32_t)n_src,
                                     pil::Thresholds{min_count, frac_num, frac_den}, out, capacity);
    });
}

int kbo_pileup_batch(kbo_index_t *idx, const uint8_t *concat, const uint64_t *offsets, size_t n_seqs, uint32_t bridge, int strands, int skip_multi,
                     uint32_t min_count, uint32_t frac_num, uint32_t frac_den, kbo_pile_site **sites, uint64_t *n_sites, uint32_t *depth_out,
                     uint32_t *pile_out)
{
    return guarded([&] {
        KBO_REQUIRE(strands >= 1 && strands <= 3, KBO_E_BAD_ARG, "strands: KBO_STRAND_FWD, KBO_STRAND_REV or both");
        KBO_REQUIRE(idx && sites && n_sites, KBO_E_BAD_ARG, "null argument");
        KBO_REQUIRE(bridge <= kbo::idxlocate::kMaxBridge, KBO_E_BAD_ARG, "bridge above 255");
        KBO_REQUIRE(min_count > 0 && frac_den > 0, KBO_E_BAD_ARG, "min_count == 0 or frac_den == 0");
        require_unsharded(idx, "kbo_pileup_batch");
        KBO_REQUIRE(kbo_index_has_positions(idx), KBO_E_BAD_ARG, "the handle has no positions (kbo_index_add_positions)");
        check_batch(concat, offsets, n_seqs);
        const uint64_t total = offsets[n_seqs];
        KBO_REQUIRE(total + 16 <= (1ull << 32) && n_seqs < pil::kMaxSeqs, KBO_E_UNSUPPORTED, "a batch of 2^32 - 16 bases or 2^28 sequences, or more");
        // ---- the device from here on
        ok(kbo_index_positions_to_device(idx, -1));
        uint32_t n_src = 0;
        const uint64_t *d_src_off = source_offsets_on(idx, current_device(), &n_src);
        KBO_REQUIRE(d_src_off && n_src, KBO_E_HIP, "the source offsets did not reach the device");
        const uint32_t k = (uint32_t)idx->host.k;
        const uint64_t bases = kbo_index_source_bases(idx);
        const size_t pad = (size_t)pil::round16(total) + 64, wb = kbo_ms_work_bytes(n_seqs, total, 0, k), sb = kbo_segments_work_bytes(n_seqs, total);
        DevBuf q(pad), off((n_seqs + 1) * 8), ms(pad), lo(total * 4 + 16), hi(total * 4 + 16), work(wb), swork(sb), cnt(16), delta((bases + 1) * 4),
            depth(bases * 4 + 16), pile(bases * 16 + 16), dwork(kbo_depth_work_bytes(idx)), twork(sites_work_bytes(idx)), qr, recs, out;
        HIP_OK(hipMemset(q.p, 0, pad));
        if (total) HIP_OK(hipMemcpy(q.p, concat, total, hipMemcpyHostToDevice));
        HIP_OK(hipMemcpy(off.p, offsets, (n_seqs + 1) * 8, hipMemcpyHostToDevice));
        HIP_OK(hipMemset(delta.p, 0, (bases + 1) * 4));
        HIP_OK(hipMemset(pile.p, 0, bases * 16 + 16));
        for (int st = 0; st < 2 && total; st++) {
            if (!(strands & (1 << st))) continue;
            const uint8_t *d_q = q.as<uint8_t>();
            if (st) {
                qr.alloc(pad);
                HIP_OK(hipMemset(qr.p, 0, pad));
                ok(kbo_revcomp_batch_dev(q.as<uint8_t>(), off.as<uint64_t>(), n_seqs, total, 0, qr.as<uint8_t>(), nullptr));
                d_q = qr.as<uint8_t>();
            }
            // the walk, its segments counted, then written at their number with the strand's delta, and piled
            ok(kbo_ms_batch_dev(idx, d_q, off.as<uint64_t>(), n_seqs, total, 0, ms.as<uint8_t>(), lo.as<uint32_t>(), hi.as<uint32_t>(), work.p, wb, nullptr));
            ok(kbo_segments_dev(idx, ms.as<uint8_t>(), lo.as<uint32_t>(), off.as<uint64_t>(), n_seqs, total, bridge, (uint32_t)st + 1u, nullptr, 0,
                                cnt.as<uint64_t>(), nullptr, swork.p, sb, nullptr));
            uint64_t n = 0;
            HIP_OK(hipMemcpy(&n, cnt.p, 8, hipMemcpyDeviceToHost));
            KBO_REQUIRE(n <= pil::kMaxSegs, KBO_E_UNSUPPORTED, "2^32 - 1 segments or more");
            recs.ensure((size_t)n * sizeof(kbo_seq_segment) + 16);
            ok(kbo_segments_dev(idx, ms.as<uint8_t>(), lo.as<uint32_t>(), off.as<uint64_t>(), n_seqs, total, bridge, (uint32_t)st + 1u,
                                recs.as<kbo_seq_segment>(), (size_t)n, cnt.as<uint64_t>(), delta.as<uint32_t>(), swork.p, sb, nullptr));
            pileup_enqueue(k, bases, d_q, ms.as<uint8_t>(), off.as<uint64_t>(), n_seqs, total, recs.as<kbo_seq_segment>(), cnt.as<uint64_t>(), (size_t)n,
                           skip_multi != 0, pile.as<uint32_t>(), nullptr);
        }
        ok(kbo_depth_finish_dev(idx, delta.as<uint32_t>(), depth.as<uint32_t>(), dwork.p, kbo_depth_work_bytes(idx), nullptr));
        // the sites counted, then written at their number
        const pil::Thresholds t{min_count, frac_num, frac_den};
        sites_enqueue(d_src_off, n_src, bases, pile.as<uint32_t>(), depth.as<uint32_t>(), t, nullptr, 0, cnt.as<uint64_t>(), twork.p, nullptr);
        uint64_t n = 0;
        HIP_OK(hipMemcpy(&n, cnt.p, 8, hipMemcpyDeviceToHost));
        out.alloc((size_t)n * sizeof(kbo_pile_site) + 16);
        sites_enqueue(d_src_off, n_src, bases, pile.as<uint32_t>(), depth.as<uint32_t>(), t, out.as<kbo_pile_site>(), (size_t)n, cnt.as<uint64_t>(), twork.p,
                      nullptr);
        MallocPtr<kbo_pile_site> host = malloc_array<kbo_pile_site>((size_t)n);
        if (n) HIP_OK(hipMemcpy(host.get(), out.p, (size_t)n * sizeof(kbo_pile_site), hipMemcpyDeviceToHost));
        if (depth_out && bases) HIP_OK(hipMemcpy(depth_out, depth.p, bases * 4, hipMemcpyDeviceToHost));
        if (pile_out && bases) HIP_OK(hipMemcpy(pile_out, pile.p, bases * 16, hipMemcpyDeviceToHost));
        *n_sites = n;
        *sites = host.release();
    });
}
