// refset_runs.cpp — what the runs of a find say about the references (kbo_hip.h), over a set built with positions:
// kbo_locate_refset turns the runs into anchors on the references with one kernel (refset_locate.hpp; refset_locate_kernels.hip);
// kbo_cover_refset counts every anchor of the runs on the base its entry names and reduces along each reference to its depth and
// breadth (refset_cover.hpp; refset_cover_kernels.hip).  Each as a host call, on the CPU (*_host) and device-resident (*_dev).
#include "refset_internal.hpp"
#include "refset_cover.hpp"
#include "refset_locate.hpp"

using namespace kbo_host;

static_assert(kbo::reflocate::kPosNone == KBO_POS_NONE && kbo::reflocate::kPosNone == KBO_LOCUS_NONE && kbo::reflocate::kMulti == KBO_LOCUS_MULTI &&
                  sizeof(kbo_ref_locus) == 24 && sizeof(kbo_ref_locus) == sizeof(kbo::reflocate::Locus),
              "kbo_hip.h states the position table's constants and the six words of a locus");
static_assert(sizeof(kbo_ref_cover) == 48 && sizeof(kbo_ref_cover) == sizeof(kbo::refcover::Cover) && KBO_COVER_NO_ENTRIES == kbo::refcover::kFlagNoEntries &&
                  KBO_COVER_OVERFLOW == kbo::refcover::kFlagOverflow,
              "kbo_hip.h states the twelve words of a cover and its flags");

namespace {
namespace lc = kbo::reflocate;

// the batch and the runs of a host call on the device.  (The count is copied from here: it lives until the call's one wait.)
struct RunsOnDevice {
    DevBuf q, off, runs, n;
    uint64_t n_runs;
    RunsOnDevice(const uint8_t *concat, const uint64_t *offsets, size_t n_seqs, uint64_t total, const kbo_ref_run *src, uint64_t n_runs_, hipStream_t st)
        : q(up16((size_t)total) + 16), off((n_seqs + 1) * sizeof(uint64_t)), runs((size_t)n_runs_ * sizeof(kbo_ref_run)), n(16), n_runs(n_runs_)
    {
        HIP_OK(hipMemcpyAsync(q.p, concat, total, hipMemcpyHostToDevice, st));
        HIP_OK(hipMemcpyAsync(off.p, offsets, (n_seqs + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, st));
        HIP_OK(hipMemcpyAsync(runs.p, src, (size_t)n_runs * sizeof(kbo_ref_run), hipMemcpyHostToDevice, st));
        HIP_OK(hipMemcpyAsync(n.p, &n_runs, sizeof(uint64_t), hipMemcpyHostToDevice, st));
    }
};

// the batch and the runs in the arguments of the locate or the cover kernel, which name them alike
template <typename Args>
void put_runs(Args &a, const uint8_t *q, const uint64_t *off, const uint32_t *runs, const uint64_t *n_runs, uint64_t capacity, uint64_t total, size_t n_seqs)
{
    a.q = q;
    a.off = off;
    a.runs = runs;
    a.n_runs = n_runs;
    a.capacity = capacity;
    a.total = total;
    a.n_seqs = (uint32_t)n_seqs;
}

// the checks the device-resident forms make behind their null arguments and alignments
void check_runs_dev(const kbo_refset *set, size_t n_seqs)
{
    KBO_REQUIRE(set->positions, KBO_E_BAD_ARG, "the set has no positions (kbo_refset_build_opts)");
    KBO_REQUIRE(n_seqs > 0, KBO_E_EMPTY_QUERY, "empty batch");
    KBO_REQUIRE(n_seqs < 0xFFFFFFFFull, KBO_E_UNSUPPORTED, "more than 2^32-1 sequences per call");
}

// what kbo_locate_refset, kbo_cover_refset and their host forms check behind their null arguments, all before any work: the set has
// positions, the batch, then every record; the batch's bases
uint64_t check_runs_host(const kbo_refset *set, const uint8_t *concat, const uint64_t *offsets, size_t n_seqs, const kbo_ref_run *runs,
                         uint64_t n_runs)
{
    KBO_REQUIRE(set->positions, KBO_E_BAD_ARG, "the set has no positions (kbo_refset_build_opts)");
    const uint64_t total = check_refset_batch(set, concat, offsets, n_seqs);
    for (uint64_t x = 0; x < n_runs; x++) {
        const kbo_ref_run &w = runs[x];
        KBO_REQUIRE(w.ref < set->descs.size() && packed_ok(set->descs[w.ref]), KBO_E_BAD_ARG,
                    "a run of a reference that is not in the set, has a status or takes the single-index route");
        KBO_REQUIRE(w.seq < n_seqs && (w.strand == KBO_STRAND_FWD || w.strand == KBO_STRAND_REV), KBO_E_BAD_ARG,
                    "a run of a sequence that is not in the batch, or of no strand");
        KBO_REQUIRE(lc::span_ok(offsets[w.seq], offsets[w.seq + 1], total, w.run.start, w.run.end), KBO_E_BAD_ARG,
                    "a run with start > end, or end beyond its sequence");
    }
    return total;
}

kbo::RefsetLocateArgs locate_args(const kbo_refset *set, const DevSet *ds)
{
    kbo::RefsetLocateArgs a{};
    a.descs = ds->descs.as<kbo::RefsetDesc>();
    a.arena = ds->arena.as<uint4>();
    a.positions = ds->pos.as<uint32_t>();
    a.pos_off = ds->pos_off.as<uint64_t>();
    a.n_refs = (uint32_t)set->descs.size();
    a.k = set->k;
    return a;
}
} // namespace

extern "C" {

int kbo_refset_has_positions(const kbo_refset_t *set) { return set && set->positions ? 1 : 0; }

uint64_t kbo_refset_positions_bytes(const kbo_refset_t *set)
{
    if (!set || !set->positions) return 0;
    return (uint64_t)set->pos.size() * sizeof(uint32_t) + (uint64_t)set->pos_off.size() * sizeof(uint64_t);
}

int kbo_refset_positions(const kbo_refset_t *set, size_t r, uint32_t *out, size_t *n_rows)
{
    if (!set || !set->positions || r >= set->descs.size() || !n_rows) return KBO_E_BAD_ARG;
    *n_rows = (size_t)(set->pos_off[r + 1] - set->pos_off[r]);
    if (out && *n_rows) std::memcpy(out, set->pos.data() + set->pos_off[r], *n_rows * sizeof(uint32_t));
    return KBO_OK;
}

uint64_t kbo_refset_ref_len(const kbo_refset_t *set, size_t r) { return set && r < set->ref_len.size() ? set->ref_len[r] : 0; }

int kbo_locate_refset_host(const kbo_refset_t *set, const uint8_t *concat, const uint64_t *offsets, size_t n_seqs, const kbo_ref_run *runs,
                           uint64_t n_runs, kbo_ref_locus *loci_out)
{
    return guarded([&] {
        KBO_REQUIRE(set && concat && offsets && (n_runs == 0 || (runs && loci_out)), KBO_E_BAD_ARG, "null argument");
        (void)check_runs_host(set, concat, offsets, n_seqs, runs, n_runs);
        const HostSeq q{concat};
        for (uint64_t x = 0; x < n_runs; x++) {
            const kbo_ref_run &w = runs[x];
            const kbo::RefsetDesc &d = set->descs[w.ref];
            const HostForm form = host_form(set, d);
            const HostPos pos{set->pos.data() + set->pos_off[w.ref]};
            const uint64_t begin = offsets[w.seq], len = offsets[w.seq + 1] - begin;
            const bool rev = w.strand == KBO_STRAND_REV;
            const lc::Locus L = lc::locate_serial(w.run.start, w.run.end, set->k, [&](uint32_t i) {
                return lc::kmer_entry(form, d.n_sets, set->k, q, begin, len, rev, pos, i);
            });
            std::memcpy(&loci_out[x], &L, sizeof L);
        }
    });
}

int kbo_locate_refset(kbo_refset_t *set, const uint8_t *concat, const uint64_t *offsets, size_t n_seqs, const kbo_ref_run *runs,
                      uint64_t n_runs, kbo_ref_locus *loci_out)
{
    return guarded([&] {
        KBO_REQUIRE(set && concat && offsets && (n_runs == 0 || (runs && loci_out)), KBO_E_BAD_ARG, "null argument");
        const uint64_t total = check_runs_host(set, concat, offsets, n_seqs, runs, n_runs);
        if (n_runs == 0) return;
        DevSet *ds = device_set(set, current_device());
        StreamScope stream;
        DevBuf d_loci((size_t)n_runs * sizeof(kbo_ref_locus));
        RunsOnDevice in(concat, offsets, n_seqs, total, runs, n_runs, stream.s);
        kbo::RefsetLocateArgs a = locate_args(set, ds);
        put_runs(a, in.q.as<uint8_t>(), in.off.as<uint64_t>(), in.runs.as<uint32_t>(), in.n.as<uint64_t>(), n_runs, total, n_seqs);
        a.loci = d_loci.as<uint32_t>();
        HIP_OK(kbo::launch_refset_locate(a, stream.s));
        HIP_OK(hipMemcpyAsync(loci_out, d_loci.p, (size_t)n_runs * sizeof(kbo_ref_locus), hipMemcpyDeviceToHost, stream.s));
        HIP_OK(hipStreamSynchronize(stream.s)); // the call's one wait
    });
}

int kbo_locate_refset_dev(kbo_refset_t *set, const uint8_t *d_concat, const uint64_t *d_offsets, size_t n_seqs, uint64_t total_bases,
                          const kbo_ref_run *d_runs, const uint64_t *d_n_runs, size_t capacity, kbo_ref_locus *d_loci, void *stream)
{
    return guarded([&] {
        KBO_REQUIRE(set && d_concat && d_offsets && d_n_runs && (capacity == 0 || (d_runs && d_loci)), KBO_E_BAD_ARG, "null argument");
        KBO_REQUIRE(((uintptr_t)d_concat & 15) == 0 && ((uintptr_t)d_offsets & 7) == 0 && ((uintptr_t)d_n_runs & 7) == 0 &&
                        ((uintptr_t)d_runs & 3) == 0 && ((uintptr_t)d_loci & 3) == 0,
                    KBO_E_BAD_ARG, "d_concat 16-byte, d_offsets and the count 8-byte, the records 4-byte aligned");
        check_runs_dev(set, n_seqs);
        kbo::RefsetLocateArgs a = locate_args(set, require_device_set(set, true));
        put_runs(a, d_concat, d_offsets, reinterpret_cast<const uint32_t *>(d_runs), d_n_runs, capacity, total_bases, n_seqs);
        a.loci = reinterpret_cast<uint32_t *>(d_loci);
        HIP_OK(kbo::launch_refset_locate(a, static_cast<hipStream_t>(stream)));
    });
}

// ---- depth and breadth of every reference (refset_cover.hpp; refset_cover_kernels.hip)
} // extern "C"

namespace {
namespace cv = kbo::refcover;

struct HostWords { // refset_cover.hpp's accessors over H and the profile on the host
    uint32_t *h_;
    uint32_t get(uint64_t i) const { return h_[i]; }
    void set(uint64_t i, uint32_t v) { h_[i] = v; }
    void add(uint64_t i) { h_[i]++; }
};
struct HostDepth {
    uint32_t *d_;
    void put(uint64_t i, uint32_t v) { d_[i] = v; }
};

// the call on the CPU: count, scan and reduce as refset_cover.hpp's serial forms have them
void cover_host(const kbo_refset *set, const uint8_t *concat, const uint64_t *offsets, const kbo_ref_run *runs, uint64_t n_runs,
                kbo_ref_cover *covers_out, uint32_t *depth_out)
{
    const size_t n_refs = set->descs.size();
    std::vector<uint32_t> h((size_t)set->cov_off[n_refs], 0u), ref_runs(n_refs, 0u);
    std::vector<uint64_t> anchors(n_refs, 0), multi(n_refs, 0);
    HostWords H{h.data()};
    const HostSeq q{concat};
    for (uint64_t x = 0; x < n_runs; x++) {
        const kbo_ref_run &w = runs[x];
        const kbo::RefsetDesc &d = set->descs[w.ref];
        const HostForm form = host_form(set, d);
        const HostPos pos{set->pos.data() + set->pos_off[w.ref]};
        const uint64_t begin = offsets[w.seq], len = offsets[w.seq + 1] - begin;
        const bool rev = w.strand == KBO_STRAND_REV;
        cv::count_serial(
            H, set->cov_off[w.ref], (uint32_t)set->ref_len[w.ref], w.run.start, w.run.end, set->k,
            [&](uint32_t i) { return lc::kmer_entry(form, d.n_sets, set->k, q, begin, len, rev, pos, i); }, anchors[w.ref], multi[w.ref]);
        ref_runs[w.ref]++;
    }
    HostDepth depth{depth_out};
    for (size_t r = 0; r < n_refs; r++) {
        const uint32_t len = (uint32_t)set->ref_len[r];
        cv::Cover c = cv::no_entries(len);
        if (packed_ok(set->descs[r])) {
            cv::scan_serial(H, set->cov_off[r], len);
            c = cv::finish(len, cv::reduce_serial(H, set->cov_off[r], len, set->k, depth_out ? &depth : nullptr, set->cov_off[r]), ref_runs[r], anchors[r],
                           multi[r]);
        }
        std::memcpy(&covers_out[r], &c, sizeof c);
    }
}

kbo::RefsetCoverArgs cover_args(const kbo_refset *set, const DevSet *ds)
{
    kbo::RefsetCoverArgs a{};
    const size_t n_refs = set->descs.size();
    a.descs = ds->descs.as<kbo::RefsetDesc>();
    a.arena = ds->arena.as<uint4>();
    a.positions = ds->pos.as<uint32_t>();
    a.pos_off = ds->pos_off.as<uint64_t>();
    a.base_off = ds->cov.as<uint64_t>();
    a.ref_len = reinterpret_cast<const uint32_t *>(ds->cov.as<uint64_t>() + n_refs + 1);
    a.n_refs = (uint32_t)n_refs;
    a.bases = set->cov_off[n_refs];
    a.k = set->k;
    return a;
}
} // namespace

extern "C" {

uint64_t kbo_refset_cover_bases(const kbo_refset_t *set) { return set && set->positions ? set->cov_off.back() : 0; }

int kbo_refset_cover_offsets(const kbo_refset_t *set, uint64_t *out)
{
    if (!set || !set->positions || !out) return KBO_E_BAD_ARG;
    std::memcpy(out, set->cov_off.data(), set->cov_off.size() * sizeof(uint64_t));
    return KBO_OK;
}

size_t kbo_cover_refset_dev_work_bytes(const kbo_refset_t *set)
{
    if (!set || !set->positions) return 0;
    return (size_t)cv::work_bytes(set->descs.size(), set->cov_off.back());
}

int kbo_cover_refset_host(const kbo_refset_t *set, const uint8_t *concat, const uint64_t *offsets, size_t n_seqs, const kbo_ref_run *runs,
                          uint64_t n_runs, kbo_ref_cover *covers_out, uint32_t *depth_out)
{
    return guarded([&] {
        KBO_REQUIRE(set && concat && offsets && covers_out && (n_runs == 0 || runs), KBO_E_BAD_ARG, "null argument");
        (void)check_runs_host(set, concat, offsets, n_seqs, runs, n_runs);
        cover_host(set, concat, offsets, runs, n_runs, covers_out, depth_out);
    });
}

int kbo_cover_refset(kbo_refset_t *set, const uint8_t *concat, const uint64_t *offsets, size_t n_seqs, const kbo_ref_run *runs, uint64_t n_runs,
                     kbo_ref_cover *covers_out, uint32_t *depth_out)
{
    return guarded([&] {
        KBO_REQUIRE(set && concat && offsets && covers_out && (n_runs == 0 || runs), KBO_E_BAD_ARG, "null argument");
        const uint64_t total = check_runs_host(set, concat, offsets, n_seqs, runs, n_runs);
        if (n_runs == 0) { // (no device: the records of references nothing was found on, and a profile of zeros)
            cover_host(set, concat, offsets, runs, 0, covers_out, depth_out);
            return;
        }
        DevSet *ds = device_set(set, current_device());
        StreamScope stream;
        const size_t n_refs = set->descs.size(), bases = (size_t)set->cov_off[n_refs], work_bytes = (size_t)cv::work_bytes(n_refs, bases);
        DevBuf d_covers(n_refs * sizeof(kbo_ref_cover)), d_work(work_bytes), d_depth(depth_out ? bases * sizeof(uint32_t) + 16 : 0);
        RunsOnDevice in(concat, offsets, n_seqs, total, runs, n_runs, stream.s);
        kbo::RefsetCoverArgs a = cover_args(set, ds);
        put_runs(a, in.q.as<uint8_t>(), in.off.as<uint64_t>(), in.runs.as<uint32_t>(), in.n.as<uint64_t>(), n_runs, total, n_seqs);
        a.covers = d_covers.as<uint32_t>();
        a.depth = depth_out ? d_depth.as<uint32_t>() : nullptr;
        a.work = d_work.as<uint8_t>();
        HIP_OK(kbo::launch_refset_cover(a, stream.s));
        HIP_OK(hipMemcpyAsync(covers_out, d_covers.p, n_refs * sizeof(kbo_ref_cover), hipMemcpyDeviceToHost, stream.s));
        if (depth_out && bases) HIP_OK(hipMemcpyAsync(depth_out, d_depth.p, bases * sizeof(uint32_t), hipMemcpyDeviceToHost, stream.s));
        HIP_OK(hipStreamSynchronize(stream.s)); // the call's one wait
    });
}

int kbo_cover_refset_dev(kbo_refset_t *set, const uint8_t *d_concat, const uint64_t *d_offsets, size_t n_seqs, uint64_t total_bases,
                         const kbo_ref_run *d_runs, const uint64_t *d_n_runs, size_t capacity, kbo_ref_cover *d_covers, uint32_t *d_depth,
                         void *d_work, size_t work_bytes, void *stream)
{
    return guarded([&] {
        KBO_REQUIRE(set && d_concat && d_offsets && d_n_runs && d_covers && d_work && (capacity == 0 || d_runs), KBO_E_BAD_ARG, "null argument");
        KBO_REQUIRE(((uintptr_t)d_concat & 15) == 0 && ((uintptr_t)d_work & 15) == 0 && ((uintptr_t)d_offsets & 7) == 0 &&
                        ((uintptr_t)d_n_runs & 7) == 0 && ((uintptr_t)d_runs & 3) == 0 && ((uintptr_t)d_covers & 3) == 0 && ((uintptr_t)d_depth & 3) == 0,
                    KBO_E_BAD_ARG, "d_concat and d_work 16-byte, d_offsets and the count 8-byte, the records and d_depth 4-byte aligned");
        check_runs_dev(set, n_seqs);
        KBO_REQUIRE(work_bytes >= kbo_cover_refset_dev_work_bytes(set), KBO_E_BAD_ARG, "work_bytes below the figure of kbo_cover_refset_dev_work_bytes");
        kbo::RefsetCoverArgs a = cover_args(set, require_device_set(set, true));
        put_runs(a, d_concat, d_offsets, reinterpret_cast<const uint32_t *>(d_runs), d_n_runs, capacity, total_bases, n_seqs);
        a.covers = reinterpret_cast<uint32_t *>(d_covers);
        a.depth = d_depth;
        a.work = static_cast<uint8_t *>(d_work);
        HIP_OK(kbo::launch_refset_cover(a, static_cast<hipStream_t>(stream)));
    });
}

} // extern "C"
