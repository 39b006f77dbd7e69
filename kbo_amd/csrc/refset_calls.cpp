// refset_calls.cpp — the variants of a pair (kbo_hip.h "The VARIANTS of a pair"): kbo_call_refset runs the first
// pass of kbo::call behind the summary's stages of every slab of refset_internal.hpp's host pipeline (refset_call.hpp;
// refset_call_kernels.hip): the sites and their windows come back, and the host resolves them as call_batch.cpp resolves a site left
// to it - one suffix automaton per (sequence, strand) with a site.  kbo_call_refset_host is the same pipeline on the CPU, and
// kbo_call_refset_host_indexed that with the second pass as the device-resident forms run it (refset_resolve.hpp).
#include "refset_internal.hpp"
#include "refine.hpp"
#include "refset_call.hpp"
#include "refset_resolve.hpp"
#include "run_automaton.hpp"

#include <thread>

using namespace kbo_host;

namespace {
namespace rc = kbo::refcall;

struct CallSite { // a site as the second pass takes it; its window record has the same index
    uint32_t ref, seq, strand, thr, i, j;
};
struct CallSites {
    uint32_t k = 0, stride = 0, pad = 0;
    std::vector<CallSite> sites;
    std::vector<uint8_t> wins;
    void init(uint32_t k_)
    {
        k = k_;
        stride = rc::window_stride(k_);
        pad = rc::window_pad(k_);
    }
};

// the checks of kbo_call_refset and its host form, all before any work: the options, the thresholds, the batch's bases
struct CallCheck {
    kbo_call_opts o;
    std::vector<uint32_t> thr;
    uint64_t total = 0;
};
CallCheck check_call(const kbo_refset *set, const uint8_t *concat, const uint64_t *offsets, size_t n_seqs, const kbo_call_opts *opts, int strands,
                     kbo_ref_calls *out)
{
    static_assert(sizeof(kbo_ref_variant) == 24 && sizeof(rc::Site) == 16, "kbo_ref_variant is 24 bytes, a site record four words");
    require_strands(strands);
    KBO_REQUIRE(set && out, KBO_E_BAD_ARG, "null argument");
    *out = kbo_ref_calls{0, 0, nullptr, nullptr};
    CallCheck c;
    if (opts) c.o = *opts; else kbo_call_opts_default(&c.o);
    KBO_REQUIRE(c.o.sbwt_build_opts.k == set->k, KBO_E_K_MISMATCH, "assert!(sbwt_ref.k() == sbwt_query.k()) (lib.rs:559)");
    KBO_REQUIRE(packed_only(set), KBO_E_UNSUPPORTED,
                "a reference of the single-index route: kbo_call_batch on an index of it (kbo_refset_packed_only)");
    c.thr = refset_thresholds(set, c.o.max_error_prob);
    c.total = check_refset_batch(set, concat, offsets, n_seqs);
    const uint64_t per_base = c.o.sbwt_build_opts.add_revcomp ? 2 : 1;
    for (size_t s = 0; s < n_seqs; s++) // (what RunAutomaton::build refuses)
        KBO_REQUIRE(per_base * (offsets[s + 1] - offsets[s]) < (1ull << 29), KBO_E_UNSUPPORTED,
                    "a sequence of 2^29 bases or more (2^28 with add_revcomp)");
    return c;
}

// The second pass (variant_calling.rs:275-284), as call_batch.cpp does it for a site left to the host: the query-side k-mer and its
// depths from the sequence and the window, the depths of the row's k-mer against the sequence's own index from a suffix automaton of
// the sequence on its strand - one per (sequence, strand) with a site - and resolve_variant with the pair's threshold.  The records
// in the order (reference, sequence, strand, position).
void resolve_sites(const CallSites &S, const uint8_t *concat, const uint64_t *offsets, bool add_revcomp, uint32_t num_threads, kbo_ref_calls *out)
{
    struct Rec {
        uint32_t site, group, chars;
        uint16_t q_len, r_len;
    };
    const uint32_t k = S.k;
    const size_t n = S.sites.size();
    std::vector<uint32_t> order(n);
    for (size_t x = 0; x < n; x++) order[x] = (uint32_t)x;
    auto key = [&](uint32_t x) { return (uint64_t)S.sites[x].seq * 2u + (S.sites[x].strand - 1u); };
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return key(a) != key(b) ? key(a) < key(b) : a < b; });
    std::vector<size_t> first; // the groups: the sites of one (sequence, strand)
    for (size_t x = 0; x < n; x++)
        if (x == 0 || key(order[x]) != key(order[x - 1])) first.push_back(x);
    first.push_back(n);
    const size_t n_groups = first.size() - 1;
    std::vector<std::vector<Rec>> recs(n_groups);
    std::vector<std::vector<uint8_t>> chars(n_groups);
    std::atomic<size_t> next{0};
    std::atomic<int> failed{KBO_OK};
    auto work = [&] {
        RunAutomaton sam;
        std::vector<uint32_t> dq(k), dr(k);
        std::vector<uint8_t> qk(k), rev;
        try {
            for (size_t g; (g = next.fetch_add(1)) < n_groups;) {
                const CallSite &head = S.sites[order[first[g]]];
                const size_t len = (size_t)(offsets[head.seq + 1] - offsets[head.seq]);
                const uint8_t *seq = concat + offsets[head.seq];
                if (head.strand == KBO_STRAND_REV) {
                    revcomp_host(seq, len, rev);
                    seq = rev.data();
                }
                sam.build(seq, len, k, add_revcomp);
                for (size_t y = first[g]; y < first[g + 1]; y++) {
                    const CallSite &w = S.sites[order[y]];
                    const uint8_t *win = S.wins.data() + (size_t)order[y] * S.stride, *rk = win + S.pad;
                    for (uint32_t t = 0; t < k; t++) { // (call_batch.cpp call_slow: variant_calling.rs:46-58, 275, 279)
                        const int64_t pos = (int64_t)w.j - (int64_t)(k - 1u) + t;
                        if (pos < 0) {
                            qk[t] = '$';
                            dr[t] = 0;
                            continue;
                        }
                        qk[t] = seq[pos];
                        dr[t] = std::min<uint32_t>(win[t], (uint32_t)std::min<int64_t>(t + 1u, pos + 1));
                    }
                    sam.depths(rk, k, dq.data()); // (:280)
                    size_t qf, qt, rf, rt;
                    if (!kbo::resolve_variant_ranges(qk.data(), rk, dq.data(), dr.data(), k, w.thr, qf, qt, rf, rt)) continue; // (:282-284)
                    recs[g].push_back(Rec{order[y], (uint32_t)g, (uint32_t)chars[g].size(), (uint16_t)(qt - qf), (uint16_t)(rt - rf)});
                    chars[g].insert(chars[g].end(), qk.begin() + qf, qk.begin() + qt);
                    chars[g].insert(chars[g].end(), rk + rf, rk + rt);
                }
            }
        } catch (const KboError &e) {
            failed = e.code;
        } catch (const std::exception &) {
            failed = KBO_E_NOMEM;
        }
    };
    std::vector<std::thread> team;
    try {
        for (uint32_t t = 1; t < std::min<size_t>(num_threads, n_groups); t++) team.emplace_back(work);
    } catch (const std::exception &) { // (no further thread: those that started and this one share the groups)
    }
    work();
    for (auto &t : team) t.join();
    KBO_REQUIRE(failed.load() == KBO_OK, failed.load(), "the second pass of kbo_call_refset failed");

    std::vector<Rec> all;
    uint64_t n_chars = 0;
    for (size_t g = 0; g < n_groups; g++) {
        all.insert(all.end(), recs[g].begin(), recs[g].end());
        n_chars += chars[g].size();
    }
    KBO_REQUIRE(n_chars < 0xFFFFFFFFull, KBO_E_UNSUPPORTED, "2^32 - 1 characters of variants or more");
    auto less = [&](const Rec &a, const Rec &b) {
        const CallSite &x = S.sites[a.site], &y = S.sites[b.site];
        if (x.ref != y.ref) return x.ref < y.ref;
        if (x.seq != y.seq) return x.seq < y.seq;
        if (x.strand != y.strand) return x.strand < y.strand;
        return x.i < y.i;
    };
    std::sort(all.begin(), all.end(), less);
    t_call[3] = all.size();
    if (all.empty()) return; // (none: the pointers stay NULL)
    MallocPtr<kbo_ref_variant> vars = malloc_array<kbo_ref_variant>(all.size());
    MallocPtr<uint8_t> bytes = malloc_array<uint8_t>((size_t)n_chars);
    uint32_t at = 0;
    for (size_t x = 0; x < all.size(); x++) {
        const Rec &r = all[x];
        const CallSite &w = S.sites[r.site];
        vars.get()[x] = kbo_ref_variant{w.ref, w.seq, w.strand, w.i, at, r.q_len, r.r_len};
        const uint32_t nc = (uint32_t)r.q_len + r.r_len;
        if (nc) std::memcpy(bytes.get() + at, chars[r.group].data() + r.chars, nc);
        at += nc;
    }
    out->n_variants = all.size();
    out->n_chars = n_chars;
    out->variants = vars.release();
    out->chars = n_chars ? bytes.release() : nullptr;
}

uint32_t call_threads() { return std::max(1u, std::min(16u, std::thread::hardware_concurrency())); }

// kbo_call_refset: behind the summary's stages of a slab, the candidates of its kept pairs, their sites and the sites' windows
struct Caller : SlabWalker {
    DevBuf d_ext, d_pref, d_pq, d_counts, d_cands, d_sites, d_win;
    size_t cap = 0;
    CallSites S;
    std::vector<uint32_t> pq;
    std::vector<rc::Site> got;

    void run_slab(const SlabPlan &P)
    {
        const size_t np = P.pairs();
        d_ext.ensure(np * sizeof(kbo_aln_extent));
        d_pref.ensure(np * sizeof(uint32_t));
        d_pq.ensure(np * sizeof(uint32_t));
        d_counts.ensure(kbo::kRefsetCallCountBytes);
        pq.resize(np);
        for (size_t p = 0; p < np; p++) pq[p] = (uint32_t)((P.strand[p] == KBO_STRAND_REV ? rev_base : 0) + offsets[P.seq[p]]);
        walk_slab(P);
        upload(d_pref.p, P.ref.data(), np * sizeof(uint32_t));
        upload(d_pq.p, pq.data(), np * sizeof(uint32_t));
        summarize(P, d_ext);
        if (!cap) cap = g_record_capacity.load();
        uint32_t counts[32];
        for (;;) { // (once, unless the slab has more candidates than the lists hold: then once more, with room for the count)
            KBO_REQUIRE(cap < 0xFFFFFFFFull, KBO_E_UNSUPPORTED, "2^32 - 1 candidates or more in a slab");
            d_cands.ensure(cap * sizeof(rc::Cand));
            d_sites.ensure(cap * sizeof(rc::Site));
            d_win.ensure(cap * (size_t)S.stride);
            kbo::RefsetCallArgs a{};
            a.descs = ds->descs.as<kbo::RefsetDesc>();
            a.arena = ds->arena.as<uint4>();
            a.q = d_q.as<uint8_t>();
            a.ms = d_ms.as<uint8_t>();
            a.poff = d_poff.as<uint64_t>();
            a.pthr = d_pthr.as<uint32_t>();
            a.ext = d_ext.as<uint32_t>();
            a.pref = d_pref.as<uint32_t>();
            a.pq = d_pq.as<uint32_t>();
            a.counts = d_counts.as<uint32_t>();
            a.cands = d_cands.as<uint2>();
            a.sites = d_sites.as<uint4>();
            a.win = d_win.as<uint8_t>();
            a.bytes = P.bytes();
            a.n_pairs = (uint32_t)np;
            a.k = k;
            a.min_thr = min_thr;
            a.cap = (uint32_t)cap;
            HIP_OK(kbo::launch_refset_call(a, st));
            HIP_OK(hipMemcpyAsync(counts, d_counts.p, sizeof counts, hipMemcpyDeviceToHost, st));
            HIP_OK(hipStreamSynchronize(st));
            if (counts[0] <= cap) break;
            cap = (size_t)counts[0] + counts[0] / 4 + 16;
        }
        const size_t n_sites = counts[16];
        KBO_REQUIRE(n_sites <= counts[0], KBO_E_HIP, "more sites than candidates");
        t_call[0] += np;
        t_call[1] += counts[0];
        t_call[2] += n_sites;
        t_routes[3]++;
        if (!n_sites) return;
        got.resize(n_sites);
        const size_t w0 = S.wins.size();
        S.wins.resize(w0 + n_sites * S.stride);
        HIP_OK(hipMemcpyAsync(got.data(), d_sites.p, n_sites * sizeof(rc::Site), hipMemcpyDeviceToHost, st));
        HIP_OK(hipMemcpyAsync(S.wins.data() + w0, d_win.p, n_sites * (size_t)S.stride, hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
        for (const rc::Site &w : got) {
            KBO_REQUIRE(w.pair < np, KBO_E_HIP, "a site of no pair of the slab");
            S.sites.push_back(CallSite{P.ref[w.pair], P.seq[w.pair], P.strand[w.pair], P.thr[w.pair], w.i, w.j});
        }
    }
};

struct HostPairSlab { // refset_call.hpp's Slab over the depths of ONE pair on the host
    const uint8_t *ms_;
    uint64_t len_;
    uint32_t thr_;
    uint32_t ms(uint64_t p) const { return ms_[p]; }
    uint64_t off(uint32_t x) const { return x ? len_ : 0u; }
    uint32_t thr(uint32_t) const { return thr_; }
    bool kept(uint32_t) const { return true; }
};
struct HostStrandSeq {
    const uint8_t *q_;
    uint32_t byte(uint32_t s) const { return q_[s]; }
};
struct HostBytes {
    uint8_t *w_;
    void put(uint32_t t, uint32_t v) { w_[t] = (uint8_t)v; }
};

// the first pass on the CPU, a pair at a time (refset_call.hpp): the sites and their windows, the counters of kbo_refset_last_call
void host_first_pass(const kbo_refset *set, const uint8_t *concat, const uint64_t *offsets, size_t n_seqs, int strands, const CallCheck &c, CallSites &S)
{
    std::fill(t_call, t_call + 4, 0);
    const uint32_t k = set->k;
    S.init(k);
    std::vector<uint8_t> rev, ms;
    for (size_t s = 0; s < n_seqs; s++) {
        const size_t len = (size_t)(offsets[s + 1] - offsets[s]);
        ms.resize(len);
        for (uint32_t strand = 1; strand <= 2; strand++) {
            if (!(strands & strand)) continue;
            const uint8_t *q = concat + offsets[s];
            if (strand == KBO_STRAND_REV) {
                revcomp_host(q, len, rev);
                q = rev.data();
            }
            const HostStrandSeq seq{q};
            for (size_t r = 0; r < set->descs.size(); r++) {
                const kbo::RefsetDesc &d = set->descs[r];
                if (!packed_ok(d)) continue;
                KBO_REQUIRE(kbo_refset_ms_host(set, r, q, len, ms.data()) == KBO_OK, KBO_E_BAD_ARG, "kbo_refset_ms_host");
                t_call[0]++;
                const uint32_t t = c.thr[r];
                if (!rc::has_hit([&](uint64_t i) { return (uint32_t)ms[i]; }, len, k, t)) continue; // (no summary record: nothing)
                const HostPairSlab slab{ms.data(), len, t};
                const HostForm form = host_form(set, d);
                for (uint64_t p = 1; p < len; p++) {
                    rc::Cand cand{0, 0};
                    if (!rc::scan_byte(slab, 1u, len, t, p, cand)) continue;
                    t_call[1]++;
                    uint32_t j = 0, row = 0;
                    if (!rc::match_serial(slab, form, d.n_sets, seq, 0u, len, k, t, cand.i, j, row)) continue;
                    t_call[2]++;
                    S.sites.push_back(CallSite{(uint32_t)r, (uint32_t)s, strand, t, cand.i, j});
                    S.wins.resize(S.wins.size() + S.stride, 0);
                    uint8_t *w = S.wins.data() + S.wins.size() - S.stride;
                    HostBytes depths{w}, kmer{w + S.pad};
                    rc::gather_depths(slab, 0u, j, k, depths);
                    rc::spell_row(form, d.n_sets, k, row, kmer);
                }
            }
        }
    }
}

// ---- the second pass as the device-resident forms run it (refset_resolve.hpp; refset_resolve_kernels.hip), on the CPU
namespace rs = kbo::refresolve;
struct HostWords {
    const uint64_t *w_;
    uint64_t word(uint64_t x) const { return w_[x]; }
};
struct HostKmer {
    const uint8_t *p_;
    uint32_t byte(uint32_t t) const { return p_[t]; }
};

// the index of a batch on its '+' strand: a word per base, sorted by code (the positions of a code ascend: the sort is stable)
std::vector<uint64_t> batch_index(const uint8_t *concat, const uint64_t *offsets, size_t n_seqs, uint32_t k, uint32_t q)
{
    std::vector<uint64_t> ix((size_t)offsets[n_seqs]);
    const HostSeq s{concat};
    for (size_t x = 0; x < n_seqs; x++)
        for (uint64_t p = offsets[x]; p < offsets[x + 1]; p++) ix[(size_t)p] = rs::index_word(s, offsets[x], offsets[x + 1], p, k, q);
    std::stable_sort(ix.begin(), ix.end(), [](uint64_t a, uint64_t b) { return (a >> 32) < (b >> 32); });
    return ix;
}

// the sites' places by their keys: LSD passes over the digits the device's radix passes read, each a stable counting sort
std::vector<uint32_t> order_by_keys(const std::vector<CallSite> &sites, uint64_t n_refs, uint64_t n_seqs, uint64_t total)
{
    const rs::KeyShape shape = rs::key_shape(n_refs, n_seqs, total);
    const size_t n = sites.size();
    std::vector<uint64_t> hi(n), lo(n), hi2(n), lo2(n);
    for (size_t x = 0; x < n; x++) {
        hi[x] = rs::key_hi(shape, sites[x].ref, sites[x].seq, sites[x].strand);
        lo[x] = rs::key_lo(sites[x].i, (uint32_t)x);
    }
    for (uint32_t p = 0; p < rs::key_passes(shape); p++) {
        uint32_t a = 0, nb = 0;
        rs::key_pass(shape, p, a, nb);
        size_t first[257] = {0};
        for (size_t x = 0; x < n; x++) first[rs::key_digit(hi[x], lo[x], a, nb) + 1u]++;
        for (size_t d = 0; d < 256; d++) first[d + 1] += first[d];
        for (size_t x = 0; x < n; x++) {
            const size_t to = first[rs::key_digit(hi[x], lo[x], a, nb)]++;
            hi2[to] = hi[x];
            lo2[to] = lo[x];
        }
        hi.swap(hi2);
        lo.swap(lo2);
    }
    std::vector<uint32_t> order(n);
    for (size_t x = 0; x < n; x++) order[x] = (uint32_t)lo[x];
    return order;
}

// resolve_variant_peaks on a site's three values: 0 no variant, 1 a variant (its ranges in r), 2 a panic
uint32_t host_verdict(uint32_t k, uint32_t csl, uint32_t qpeak, uint32_t rpeak, size_t r[4])
{
    try {
        return kbo::resolve_variant_peaks(k, csl, qpeak != rs::kNoPeak, qpeak, rpeak != rs::kNoPeak, rpeak, r[0], r[1], r[2], r[3]) ? 1u : 0u;
    } catch (const kbo::RefPanic &) {
        return 2u;
    }
}

void resolve_sites_indexed(const CallSites &S, const uint8_t *concat, const uint64_t *offsets, size_t n_seqs, size_t n_refs, uint32_t min_thr,
                           bool add_revcomp, kbo_ref_calls *out)
{
    const uint32_t k = S.k, q = rs::qmer_len(min_thr, k);
    const size_t n = S.sites.size();
    if (!n) return;
    const uint64_t total = offsets[n_seqs];
    const std::vector<uint64_t> ix = batch_index(concat, offsets, n_seqs, k, q);
    const HostSeq plus{concat};
    const HostWords words{ix.data()};
    std::vector<uint8_t> minus(total), rev; // the '-' strand, a sequence at a time, where a site needs it
    std::vector<uint8_t> have(n_seqs, 0);
    std::vector<uint32_t> word(n), dq(k), dr(k);
    std::vector<uint8_t> qk(k);
    for (size_t x = 0; x < n; x++) {
        const CallSite &w = S.sites[x];
        const uint64_t begin = offsets[w.seq], end = offsets[w.seq + 1];
        if (w.strand == KBO_STRAND_REV && !have[w.seq]) {
            revcomp_host(concat + begin, (size_t)(end - begin), rev);
            std::copy(rev.begin(), rev.end(), minus.begin() + begin);
            have[w.seq] = 1;
        }
        const uint8_t *seq = (w.strand == KBO_STRAND_REV ? minus.data() : concat) + begin;
        const uint8_t *win = S.wins.data() + x * S.stride, *rk = win + S.pad;
        const HostKmer km{rk};
        const uint32_t mode = rs::probe_mode(w.strand, add_revcomp);
        uint32_t csl = 0;
        for (uint32_t t = 0; t < k; t++) {
            qk[t] = rs::in_front(t, w.j, k) ? (uint8_t)'$' : seq[(size_t)w.j + t - (k - 1u)];
            dr[t] = rs::query_depth(win[t], t, w.j, k);
            dq[t] = rs::depth_at(km, t, q, mode, plus, begin, end, words, ix.size());
        }
        while (csl < k && qk[k - 1u - csl] == rk[k - 1u - csl]) csl++;
        const uint32_t qpeak = rs::rightmost_peak([&](uint32_t i) { return dr[i]; }, k, w.thr);
        const uint32_t rpeak = rs::rightmost_peak([&](uint32_t i) { return dq[i]; }, k, w.thr);
        word[x] = rs::resolve_word(rs::site_code(csl, qpeak, rpeak), k);
        KBO_REQUIRE(word[x] != rs::kPanic, KBO_E_REF_PANIC, "resolve_variant panics at a site (common suffix 0, or a slice beyond the k-mer)");
    }
    const std::vector<uint32_t> order = order_by_keys(S.sites, n_refs, n_seqs, total);
    uint64_t n_vars = 0, n_chars = 0;
    for (size_t x = 0; x < n; x++)
        if (rs::is_variant(word[x])) {
            n_vars++;
            n_chars += rs::word_chars(word[x]);
        }
    KBO_REQUIRE(n_chars < 0xFFFFFFFFull, KBO_E_UNSUPPORTED, "2^32 - 1 characters of variants or more");
    t_call[3] = n_vars;
    if (!n_vars) return;
    MallocPtr<kbo_ref_variant> vars = malloc_array<kbo_ref_variant>((size_t)n_vars);
    MallocPtr<uint8_t> bytes = malloc_array<uint8_t>((size_t)std::max<uint64_t>(n_chars, 1));
    uint32_t at = 0;
    size_t v = 0;
    for (size_t p = 0; p < n; p++) {
        const uint32_t x = order[p], wd = word[x];
        if (!rs::is_variant(wd)) continue;
        const CallSite &w = S.sites[x];
        const uint32_t qf = wd & 0xFFu, ql = (wd >> 8) & 0xFFu, rf = (wd >> 16) & 0xFFu, rl = wd >> 24;
        vars.get()[v++] = kbo_ref_variant{w.ref, w.seq, w.strand, w.i, at, (uint16_t)ql, (uint16_t)rl};
        const uint8_t *seq = (w.strand == KBO_STRAND_REV ? minus.data() : concat) + offsets[w.seq];
        const uint8_t *rk = S.wins.data() + (size_t)x * S.stride + S.pad;
        for (uint32_t t = 0; t < ql; t++) bytes.get()[at + t] = rs::in_front(qf + t, w.j, k) ? (uint8_t)'$' : seq[(size_t)w.j + qf + t - (k - 1u)];
        for (uint32_t t = 0; t < rl; t++) bytes.get()[at + ql + t] = rk[rf + t];
        at += ql + rl;
    }
    out->n_variants = n_vars;
    out->n_chars = n_chars;
    out->variants = vars.release();
    if (n_chars) out->chars = bytes.release();
}
} // namespace

extern "C" {

int kbo_refset_last_call(uint64_t out[4]) { return read_counters(t_call, 4, out); }

int kbo_refset_spell_row(const kbo_refset_t *set, size_t r, uint32_t row, uint8_t *out)
{
    const kbo::RefsetDesc *d = packed_desc(set, r);
    if (!d || !out || row >= d->n_sets) return KBO_E_BAD_ARG;
    HostBytes o{out};
    rc::spell_row(host_form(set, *d), d->n_sets, set->k, row, o);
    return KBO_OK;
}

void kbo_ref_calls_free(kbo_ref_calls *calls)
{
    if (!calls) return;
    std::free(calls->variants);
    std::free(calls->chars);
    *calls = kbo_ref_calls{0, 0, nullptr, nullptr};
}

int kbo_call_refset(kbo_refset_t *set, const uint8_t *concat, const uint64_t *offsets, size_t n_seqs, const kbo_call_opts *opts, int strands,
                    kbo_ref_calls *out)
{
    return guarded([&] {
        const CallCheck c = check_call(set, concat, offsets, n_seqs, opts, strands, out);
        reset_call_counters();
        std::fill(t_call, t_call + 4, 0);
        Caller F;
        F.S.init(set->k);
        StreamScope stream;
        upload_batch(F, set, concat, offsets, n_seqs, c.total, strands, stream.s);
        Screen scr;
        run_slabs(F, c.thr, n_seqs, strands, screen_call(F, c.thr, n_seqs, c.total, strands, scr));
        resolve_sites(F.S, concat, offsets, c.o.sbwt_build_opts.add_revcomp != 0, call_threads(), out);
    });
}

int kbo_call_refset_host(const kbo_refset_t *set, const uint8_t *concat, const uint64_t *offsets, size_t n_seqs, const kbo_call_opts *opts,
                         int strands, kbo_ref_calls *out)
{
    return guarded([&] {
        const CallCheck c = check_call(set, concat, offsets, n_seqs, opts, strands, out);
        CallSites S;
        host_first_pass(set, concat, offsets, n_seqs, strands, c, S);
        resolve_sites(S, concat, offsets, c.o.sbwt_build_opts.add_revcomp != 0, call_threads(), out);
    });
}

int kbo_call_refset_host_indexed(const kbo_refset_t *set, const uint8_t *concat, const uint64_t *offsets, size_t n_seqs,
                                 const kbo_call_opts *opts, int strands, kbo_ref_calls *out)
{
    return guarded([&] {
        const CallCheck c = check_call(set, concat, offsets, n_seqs, opts, strands, out);
        CallSites S;
        host_first_pass(set, concat, offsets, n_seqs, strands, c, S);
        uint32_t min_thr = set->k;
        for (size_t r = 0; r < set->descs.size(); r++)
            if (packed_ok(set->descs[r])) min_thr = std::min(min_thr, c.thr[r]);
        resolve_sites_indexed(S, concat, offsets, n_seqs, set->descs.size(), min_thr, c.o.sbwt_build_opts.add_revcomp != 0, out);
    });
}

int kbo_refset_kmer_depths_host(const uint8_t *seq, size_t len, uint32_t k, uint32_t q, int mode, const uint8_t *kmer, uint32_t *out)
{
    return guarded([&] {
        KBO_REQUIRE(seq && kmer && out && mode >= 1 && mode <= 3 && q >= 1 && q <= rs::kQMax && q <= k && k <= 255 && len < 0xFFFFFFFFull,
                    KBO_E_BAD_ARG, "kbo_refset_kmer_depths_host: arguments");
        const uint64_t off[2] = {0, len};
        const std::vector<uint64_t> ix = batch_index(seq, off, 1, k, q);
        const HostSeq s{seq};
        const HostWords words{ix.data()};
        const HostKmer km{kmer};
        for (uint32_t t = 0; t < k; t++) out[t] = rs::depth_at(km, t, q, (uint32_t)mode, s, 0u, len, words, ix.size());
    });
}

int kbo_refset_resolve_word_host(uint32_t k, uint32_t csl, uint32_t qpeak, uint32_t rpeak, uint32_t out[6])
{
    if (!out || k < 2 || k > 255 || csl > k || (qpeak != rs::kNoPeak && qpeak + 2 > k) || (rpeak != rs::kNoPeak && rpeak + 2 > k)) return KBO_E_BAD_ARG;
    out[0] = rs::resolve_word(rs::site_code(csl, qpeak, rpeak), k);
    size_t r[4] = {0, 0, 0, 0};
    out[1] = host_verdict(k, csl, qpeak, rpeak, r);
    for (int x = 0; x < 4; x++) out[2 + x] = (uint32_t)r[x];
    return KBO_OK;
}

int kbo_refset_resolve_words_check(uint32_t k, uint64_t out[4])
{
    if (!out || k < 2 || k > 255) return KBO_E_BAD_ARG;
    std::fill(out, out + 4, 0);
    auto peak = [&](uint32_t x) { return x + 1u < k ? x : rs::kNoPeak; }; // (x = k - 1: none)
    for (uint32_t csl = 0; csl <= k; csl++)
        for (uint32_t qx = 0; qx < k; qx++)
            for (uint32_t rx = 0; rx < k; rx++) {
                const uint32_t qp = peak(qx), rp = peak(rx), word = rs::resolve_word(rs::site_code(csl, qp, rp), k);
                size_t r[4] = {0, 0, 0, 0};
                const uint32_t verdict = host_verdict(k, csl, qp, rp, r);
                bool same = verdict == (word == rs::kPanic ? 2u : word == rs::kNoVariant ? 0u : 1u);
                if (same && verdict == 1u)
                    same = (word & 0xFFu) == (r[1] > r[0] ? r[0] : 0u) && ((word >> 8) & 0xFFu) == r[1] - r[0] &&
                           ((word >> 16) & 0xFFu) == (r[3] > r[2] ? r[2] : 0u) && (word >> 24) == r[3] - r[2];
                out[0]++;
                out[1] += !same;
                out[2] += verdict == 2u;
                out[3] += verdict == 1u;
            }
    return KBO_OK;
}

int kbo_refset_order_sites_host(size_t n, const uint32_t *refs, const uint32_t *seqs, const uint32_t *strands, const uint32_t *is,
                                uint64_t n_refs, uint64_t n_seqs, uint64_t total_bases, uint32_t *order_out)
{
    return guarded([&] {
        KBO_REQUIRE((n == 0 || (refs && seqs && strands && is && order_out)) && n < 0xFFFFFFFFull && n_refs >= 1 && n_refs <= 0xFFFFFFFFull &&
                        n_seqs >= 1 && n_seqs < (1ull << 28) && total_bases < (1ull << 32),
                    KBO_E_BAD_ARG, "kbo_refset_order_sites_host: arguments");
        std::vector<CallSite> sites(n);
        for (size_t x = 0; x < n; x++) {
            KBO_REQUIRE(refs[x] < n_refs && seqs[x] < n_seqs && strands[x] >= 1 && strands[x] <= 2 && is[x] < total_bases, KBO_E_BAD_ARG,
                        "kbo_refset_order_sites_host: a site outside the shape");
            sites[x] = CallSite{refs[x], seqs[x], strands[x], 0u, is[x], 0u};
        }
        const std::vector<uint32_t> order = order_by_keys(sites, n_refs, n_seqs, total_bases);
        std::copy(order.begin(), order.end(), order_out);
    });
}

} // extern "C"
