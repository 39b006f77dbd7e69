// map_batch_opts.cpp — kbo::map with any MapOpts (lib.rs:720-761) and gap_filling::fill_gaps over a batch
// (kbo_map_batch_opts, kbo_fill_gaps_batch in include/kbo_hip.h).
//
// Per slab of the batch: the walk with intervals and the translation on the device (run_walk_host,
// derand_translate_host_offsets), then the gaps on the device (gap_kernels.hip: their starts one lane per base, one wave
// per gap), and the sequences the gap kernel left behind redone whole on the host by kbo::fill_gaps from their own
// MS values and translation.  Then, for call_variants, the variants of the whole batch from kbo_call_batch_flat, applied
// in the reference's order (translate.rs:350-386) and relative_to_ref, on host threads: both are one pass over the bytes
// of a sequence, and the characters are on the host by then.
//
// A sequence kbo_map would refuse on its own gets that code in status[] and is left out of every device pass; sequences
// too short for the batched call (no more than 2k + 2 bases) take kbo_map's own route, so that the status of every
// sequence is the one kbo_map returns for it.
#include "../../include/kbo_hip.h"
#include "../../include/kbo_hip_tuning.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <memory>
#include <vector>

#include "capi_internal.hpp"

using namespace kbo_host;

namespace {

struct GapRun {
    uint64_t stats[4] = {0, 0, 0, 0}; // gaps found, finished on the device, sequences redone on the host, extension steps
    double phase[6] = {0, 0, 0, 0, 0, 0}; // seconds: walk, translate, gap kernels, host fallback, call, apply + format
};
thread_local GapRun t_last;

using clk = std::chrono::steady_clock;
double since(clk::time_point t) { return std::chrono::duration<double>(clk::now() - t).count(); }

// the batch shape every entry point here requires (status is per sequence: empty sequences are allowed)
void check_shape(const uint8_t *concat, const uint64_t *offsets, size_t n_seqs)
{
    KBO_REQUIRE(concat && offsets, KBO_E_BAD_ARG, "null concat/offsets");
    KBO_REQUIRE(n_seqs > 0, KBO_E_EMPTY_QUERY, "no sequences");
    KBO_REQUIRE(n_seqs < 0xFFFFFFFFull, KBO_E_UNSUPPORTED, "more than 2^32-1 sequences per call");
    KBO_REQUIRE(offsets[0] == 0, KBO_E_BAD_ARG, "offsets[0] must be 0");
    for (size_t s = 0; s < n_seqs; s++) {
        KBO_REQUIRE(offsets[s + 1] >= offsets[s], KBO_E_BAD_ARG, "offsets not monotone");
        KBO_REQUIRE(offsets[s + 1] - offsets[s] < 0xFFFFFFFFull, KBO_E_UNSUPPORTED, "sequence longer than 2^32-1");
    }
}

// a sub-batch: the sequences `pick` of (concat, offsets) back to back (no copy when it is all of them)
struct SubBatch {
    std::vector<size_t> pick;
    std::vector<uint8_t> bytes;
    std::vector<uint64_t> off;
    const uint8_t *concat = nullptr;
    SubBatch(const uint8_t *c, const uint64_t *o, size_t n, std::vector<size_t> p) : pick(std::move(p))
    {
        off.assign(pick.size() + 1, 0);
        for (size_t i = 0; i < pick.size(); i++) off[i + 1] = off[i] + (o[pick[i] + 1] - o[pick[i]]);
        if (pick.size() == n) {
            concat = c;
            return;
        }
        bytes.resize(off.back());
        for (size_t i = 0; i < pick.size(); i++) std::memcpy(bytes.data() + off[i], c + o[pick[i]], off[i + 1] - off[i]);
        concat = bytes.data();
    }
    size_t size() const { return pick.size(); }
};

// gap_filling::fill_gaps after the walk and the translation, for a batch whose sequences are all more than 2 and at least
// `threshold` bases long: out (offsets[n_seqs] bytes) = the refined translation, status[s] = 0 or KBO_E_REF_PANIC
void fill_gaps_core(kbo_index *idx, const uint8_t *concat, const uint64_t *offsets, size_t n_seqs, size_t threshold,
                    double max_err_prob, uint8_t *out, int32_t *status, GapRun &run)
{
    const uint32_t k = idx->host.k;
    KBO_REQUIRE(threshold < 0xFFFFFFF0ull, KBO_E_UNSUPPORTED, "threshold above 2^32");
    const uint32_t t = (uint32_t)threshold;
    const int dev = current_device();
    // the path cover spells the candidate rows; it is made now if the copy has none yet (plan structures are lazy), and a handle
    // whose plan option is off spells every row on the host
    kbo::DevIndexView ix;
    const bool plan_on = plan_enabled(idx);
    try {
        ix = device_view(idx, dev, nullptr, offsets[n_seqs], plan_on);
    } catch (const KboError &) {
        ix = device_view(idx, dev, nullptr, 0, false); // (could not be made: the copy walks plainly and the host spells)
    }
    if (!plan_on) {
        ix.pc_text = nullptr;
        ix.pc_pos = nullptr;
        ix.pc_node = nullptr;
    }
    std::vector<double> tab(kbo::kGapFillLds, 0.0); // log_rm_max_cdf(c + 1, 4, 1): the fill_overlaps test (gap_filling.rs:500-509)
    for (size_t c = 1; c < tab.size(); c++) tab[c] = kbo::log_rm_max_cdf_host(c + 1, 4, 1);
    const double log_thr = std::log1p(-max_err_prob);
    hipStream_t stream = nullptr;
    DevBuf d_tab(tab.size() * sizeof(double));
    HIP_OK(hipMemcpy(d_tab.p, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice));
    DevBuf d_cnt(64), d_stats(64), d_tr, d_out, d_flag, d_gaps, piece;
    size_t gap_cap = 0;
    BatchOnDevice B;
    std::unique_ptr<kbo::HostNav> nav;
    const std::vector<Slab> slabs = make_slabs(offsets, n_seqs, slab_bytes_for(idx));
    for (const Slab &sl : slabs) {
        const size_t ns = sl.s1 - sl.s0;
        const uint64_t total = sl.b1 - sl.b0;
        std::vector<uint64_t> loff(ns + 1);
        for (size_t i = 0; i <= ns; i++) loff[i] = offsets[sl.s0 + i] - sl.b0;
        clk::time_point t0 = clk::now();
        run_walk_host(idx, concat + sl.b0, loff.data(), ns, true, B, stream); // (synchronised)
        run.phase[0] += since(t0);
        t0 = clk::now();
        const size_t chars_bytes = (total + 15) / 16 * 16 + 16;
        d_tr.ensure(chars_bytes);
        d_out.ensure(chars_bytes);
        derand_translate_host_offsets(B.ms.as<uint8_t>(), B.off.as<uint64_t>(), loff.data(), ns, k, t, nullptr, d_tr.as<uint8_t>(),
                                      nullptr, stream, 0, &piece);
        HIP_OK(hipMemcpyAsync(d_out.p, d_tr.p, total, hipMemcpyDeviceToDevice, stream));
        HIP_OK(hipStreamSynchronize(stream));
        run.phase[1] += since(t0);
        // ---- the gaps
        t0 = clk::now();
        d_flag.ensure(ns + 16);
        HIP_OK(hipMemsetAsync(d_flag.p, 0, ns, stream));
        HIP_OK(hipMemsetAsync(d_stats.p, 0, 16, stream));
        const size_t want_cap = std::max<size_t>(1024, total / 64);
        if (gap_cap < want_cap) {
            gap_cap = want_cap;
            d_gaps.ensure(gap_cap * 8);
        }
        uint32_t n_gaps = 0;
        for (int attempt = 0; attempt < 2; attempt++) {
            HIP_OK(hipMemsetAsync(d_cnt.p, 0, 4, stream));
            HIP_OK(kbo::launch_gap_starts(d_tr.as<uint8_t>(), B.off.as<uint64_t>(), (uint32_t)ns, total, t, d_gaps.p, (uint32_t)gap_cap,
                                          d_cnt.as<uint32_t>(), stream));
            HIP_OK(hipMemcpyAsync(&n_gaps, d_cnt.p, 4, hipMemcpyDeviceToHost, stream));
            HIP_OK(hipStreamSynchronize(stream));
            if (n_gaps <= gap_cap) break;
            gap_cap = n_gaps; // overflowed: again with room for all of them
            d_gaps.ensure(gap_cap * 8);
        }
        KBO_REQUIRE(n_gaps <= gap_cap, KBO_E_HIP, "gap list overflowed twice");
        HIP_OK(kbo::launch_gap_fill(B.q.as<uint8_t>(), d_tr.as<uint8_t>(), d_out.as<uint8_t>(), B.lo.as<uint32_t>(), B.hi.as<uint32_t>(),
                                    B.off.as<uint64_t>(), d_gaps.p, n_gaps, k, t, d_tab.as<double>(), log_thr, d_flag.as<uint8_t>(),
                                    d_stats.as<unsigned long long>(), ix, stream));
        std::vector<uint8_t> flag(ns);
        uint64_t st[2] = {0, 0};
        HIP_OK(hipMemcpyAsync(out + sl.b0, d_out.p, total, hipMemcpyDeviceToHost, stream));
        HIP_OK(hipMemcpyAsync(flag.data(), d_flag.p, ns, hipMemcpyDeviceToHost, stream));
        HIP_OK(hipMemcpyAsync(st, d_stats.p, 16, hipMemcpyDeviceToHost, stream));
        HIP_OK(hipStreamSynchronize(stream));
        run.phase[2] += since(t0);
        run.stats[0] += n_gaps;
        run.stats[1] += st[0];
        run.stats[3] += st[1];
        // ---- the sequences left to the host: kbo::fill_gaps from their own values, as kbo_fill_gaps runs it
        t0 = clk::now();
        std::vector<size_t> redo;
        for (size_t i = 0; i < ns; i++)
            if (flag[i]) redo.push_back(i);
        if (!redo.empty()) {
            run.stats[2] += redo.size();
            if (!nav) nav.reset(new kbo::HostNav(idx->host));
            std::vector<uint8_t> d(total), tr(total);
            std::vector<uint32_t> lo(total), hi(total);
            HIP_OK(hipMemcpy(d.data(), B.ms.p, total, hipMemcpyDeviceToHost));
            HIP_OK(hipMemcpy(lo.data(), B.lo.p, total * 4, hipMemcpyDeviceToHost));
            HIP_OK(hipMemcpy(hi.data(), B.hi.p, total * 4, hipMemcpyDeviceToHost));
            HIP_OK(hipMemcpy(tr.data(), d_tr.p, total, hipMemcpyDeviceToHost));
            HostTeam::get().run(redo.size(), [&](size_t r) {
                const size_t i = redo[r];
                const uint64_t a = loff[i], len = loff[i + 1] - loff[i];
                std::vector<kbo::MsVal> ms(len);
                for (uint64_t x = 0; x < len; x++) ms[x] = kbo::MsVal{d[a + x], lo[a + x], hi[a + x]};
                const std::vector<uint8_t> tv(tr.begin() + a, tr.begin() + a + len);
                try {
                    const std::vector<uint8_t> refined = kbo::fill_gaps(tv, ms, concat + sl.b0 + a, len, *nav, threshold, max_err_prob);
                    std::memcpy(out + sl.b0 + a, refined.data(), len);
                } catch (const kbo::RefPanic &) {
                    status[sl.s0 + i] = KBO_E_REF_PANIC;
                }
            });
        }
        run.phase[3] += since(t0);
    }
}

void fill_gaps_batch_impl(kbo_index *idx, const uint8_t *concat, const uint64_t *offsets, size_t n_seqs, size_t threshold,
                          double max_err_prob, uint8_t *out, int32_t *status, GapRun &run)
{
    KBO_REQUIRE(idx && out && status, KBO_E_BAD_ARG, "null argument");
    check_shape(concat, offsets, n_seqs);
    require_unsharded(idx, "kbo_fill_gaps_batch");
    KBO_REQUIRE(idx->host.k > 0, KBO_E_BAD_ARG, "k > 0 (derandomize.rs:274)");
    KBO_REQUIRE(threshold > 1, KBO_E_THRESHOLD_LE_1, "threshold > 1 (derandomize.rs:275, translate.rs:269)");
    std::vector<size_t> pick;
    for (size_t s = 0; s < n_seqs; s++) {
        const uint64_t len = offsets[s + 1] - offsets[s];
        status[s] = len == 0 ? KBO_E_EMPTY_QUERY             // index.rs:248
                    : len <= 2 ? KBO_E_LEN_LE_2               // derandomize.rs:276, translate.rs:270
                    : len < threshold ? KBO_E_REF_PANIC       // refined.len() - threshold (gap_filling.rs:467)
                                      : KBO_OK;
        if (status[s] == KBO_OK) pick.push_back(s);
    }
    if (pick.empty()) return;
    SubBatch sub(concat, offsets, n_seqs, std::move(pick));
    if (sub.size() == n_seqs) {
        fill_gaps_core(idx, concat, offsets, n_seqs, threshold, max_err_prob, out, status, run);
        return;
    }
    std::vector<uint8_t> o(sub.off.back());
    std::vector<int32_t> st(sub.size(), KBO_OK);
    fill_gaps_core(idx, sub.concat, sub.off.data(), sub.size(), threshold, max_err_prob, o.data(), st.data(), run);
    for (size_t i = 0; i < sub.size(); i++) {
        const size_t s = sub.pick[i];
        status[s] = st[i];
        std::memcpy(out + offsets[s], o.data() + sub.off[i], sub.off[i + 1] - sub.off[i]);
    }
}

void map_batch_opts_impl(kbo_index *idx, const uint8_t *concat, const uint64_t *offsets, size_t n_seqs, const kbo_map_opts *opts,
                         uint8_t *out, int32_t *status, GapRun &run)
{
    KBO_REQUIRE(idx && out && status, KBO_E_BAD_ARG, "null argument");
    kbo_map_opts o;
    if (opts) o = *opts; else kbo_map_opts_default(&o);
    if (o.call_variants)
        KBO_REQUIRE(idx->host.k == o.sbwt_build_opts.k, KBO_E_K_MISMATCH, "assert!(sbwt.k() == map_opts.sbwt_build_opts.k) (lib.rs:729)");
    check_shape(concat, offsets, n_seqs);
    const bool refine = o.fill_gaps || o.call_variants;
    if (refine) require_unsharded(idx, "kbo_map_batch_opts with fill_gaps / call_variants");
    const size_t k = idx->host.k;
    const size_t threshold = random_match_threshold(k, idx->host.n_kmers, 4, o.max_error_prob); // lib.rs:731
    KBO_REQUIRE(threshold > 1, KBO_E_THRESHOLD_LE_1, "threshold > 1 (derandomize.rs:275, translate.rs:269)");
    // ---- per sequence: what kbo_map refuses at once, and the sequences that take kbo_map's own route
    std::vector<size_t> pick;
    for (size_t s = 0; s < n_seqs; s++) {
        const uint64_t len = offsets[s + 1] - offsets[s];
        status[s] = len == 0 ? KBO_E_EMPTY_QUERY : len <= 2 ? KBO_E_LEN_LE_2 : (o.fill_gaps && len < threshold) ? KBO_E_REF_PANIC : KBO_OK;
        if (status[s] != KBO_OK) continue;
        if (o.call_variants && len <= 2 * k + 2) status[s] = kbo_map(idx, concat + offsets[s], len, &o, out + offsets[s]);
        else pick.push_back(s);
    }
    if (pick.empty()) return;
    SubBatch sub(concat, offsets, n_seqs, std::move(pick));
    const size_t m = sub.size();
    const uint64_t *soff = sub.off.data();
    std::vector<uint8_t> own;
    uint8_t *res = out; // the sub-batch's characters (out itself when the sub-batch is the whole batch)
    if (m != n_seqs) {
        own.resize(sub.off.back());
        res = own.data();
    }
    std::vector<int32_t> st(m, KBO_OK);
    // ---- the translation, gap-filled (lib.rs:735-747)
    if (o.fill_gaps) fill_gaps_core(idx, sub.concat, soff, m, threshold, o.max_error_prob, res, st.data(), run);
    else {
        clk::time_point t0 = clk::now();
        matches_batch_impl(idx, sub.concat, soff, m, o.max_error_prob, HostOut::chars(res, nullptr, o.format != 0 && !o.call_variants));
        run.phase[0] += since(t0);
    }
    // ---- variants (lib.rs:749-754): the whole batch through kbo_call_batch_flat, then add_variants per sequence
    kbo_call_flat calls;
    std::memset(&calls, 0, sizeof(calls));
    std::vector<uint64_t> var_off;
    std::vector<size_t> called; // indexes into the sub-batch
    if (o.call_variants) {
        clk::time_point t0 = clk::now();
        for (size_t i = 0; i < m; i++)
            if (st[i] == KBO_OK) called.push_back(i);
        if (!called.empty()) {
            SubBatch cb(sub.concat, soff, m, called);
            kbo_call_opts co;
            co.max_error_prob = o.max_error_prob;
            co.sbwt_build_opts = o.sbwt_build_opts;
            var_off.assign(cb.size() + 1, 0);
            const int rc = kbo_call_batch_flat(idx, cb.concat, cb.off.data(), cb.size(), &co, &calls, var_off.data());
            if (rc != KBO_OK) throw KboError(rc, last_error());
        }
        run.phase[4] += since(t0);
    }
    std::unique_ptr<kbo_call_flat, void (*)(kbo_call_flat *)> calls_guard(&calls, kbo_call_flat_free);
    // ---- add_variants (translate.rs:350-386) and relative_to_ref (lib.rs:756-760), host threads
    clk::time_point t0 = clk::now();
    const bool host_format = o.format != 0 && refine;
    if (o.call_variants || host_format) {
        std::vector<uint64_t> char_off; // where the characters of each called sequence's variants start
        if (!called.empty()) {
            char_off.assign(called.size() + 1, 0);
            for (size_t c = 0; c < called.size(); c++) {
                uint64_t sum = 0;
                for (uint64_t v = var_off[c]; v < var_off[c + 1]; v++) sum += (uint64_t)calls.query_len[v] + calls.ref_len[v];
                char_off[c + 1] = char_off[c] + sum;
            }
        }
        std::vector<size_t> call_slot(m, ~(size_t)0);
        for (size_t c = 0; c < called.size(); c++) call_slot[called[c]] = c;
        HostTeam::get().run(m, [&](size_t i) {
            if (st[i] != KBO_OK) return;
            const uint64_t len = soff[i + 1] - soff[i];
            uint8_t *aln = res + soff[i];
            const size_t c = call_slot[i];
            if (c != ~(size_t)0 && var_off[c + 1] > var_off[c]) {
                std::vector<kbo::Variant> vars(var_off[c + 1] - var_off[c]);
                const uint8_t *cp = calls.chars + char_off[c];
                for (size_t v = 0; v < vars.size(); v++) {
                    const uint64_t g = var_off[c] + v;
                    vars[v].query_pos = calls.query_pos[g];
                    vars[v].query_chars.assign(cp, cp + calls.query_len[g]);
                    cp += calls.query_len[g];
                    vars[v].ref_chars.assign(cp, cp + calls.ref_len[g]);
                    cp += calls.ref_len[g];
                }
                std::vector<uint8_t> tv(aln, aln + len);
                try {
                    kbo::add_variants(tv, vars);
                } catch (const kbo::RefPanic &) {
                    st[i] = KBO_E_REF_PANIC;
                    return;
                }
                std::memcpy(aln, tv.data(), len);
            }
            if (host_format) {
                std::vector<uint8_t> f(len);
                const int rc = kbo_relative_to_ref(sub.concat + soff[i], aln, len, f.data());
                if (rc != KBO_OK) st[i] = rc;
                else std::memcpy(aln, f.data(), len);
            }
        });
    }
    run.phase[5] += since(t0);
    for (size_t i = 0; i < m; i++) {
        const size_t s = sub.pick[i];
        status[s] = st[i];
        if (res != out) std::memcpy(out + offsets[s], res + soff[i], soff[i + 1] - soff[i]);
    }
}

} // namespace

extern "C" int kbo_map_batch_opts(kbo_index_t *idx, const uint8_t *concat, const uint64_t *offsets, size_t n_seqs,
                                  const kbo_map_opts *opts, uint8_t *out, int32_t *status)
{
    t_last = GapRun();
    return guarded([&] { map_batch_opts_impl(idx, concat, offsets, n_seqs, opts, out, status, t_last); });
}

extern "C" int kbo_fill_gaps_batch(kbo_index_t *idx, const uint8_t *concat, const uint64_t *offsets, size_t n_seqs, size_t threshold,
                                   double max_err_prob, uint8_t *out, int32_t *status)
{
    t_last = GapRun();
    return guarded([&] { fill_gaps_batch_impl(idx, concat, offsets, n_seqs, threshold, max_err_prob, out, status, t_last); });
}

extern "C" int kbo_fill_gaps_stats(uint64_t out[4])
{
    if (!out) return KBO_E_BAD_ARG;
    for (int i = 0; i < 4; i++) out[i] = t_last.stats[i];
    return KBO_OK;
}

extern "C" int kbo_map_batch_opts_phases(double out[6])
{
    if (!out) return KBO_E_BAD_ARG;
    for (int i = 0; i < 6; i++) out[i] = t_last.phase[i];
    return KBO_OK;
}
