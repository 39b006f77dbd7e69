// refset_calls.cpp — the variants of a pair (kbo_hip.h "The VARIANTS of a pair"): kbo_call_refset runs the first
// pass of kbo::call behind the summary's stages of every slab of refset_internal.hpp's host pipeline (refset_call.hpp;
// refset_call_kernels.hip): the sites and their windows come back, and the host resolves them as call_batch.cpp resolves a site left
// to it - one suffix automaton per (sequence, strand) with a site.  kbo_call_refset_host is the same pipeline on the CPU.
#include "refset_internal.hpp"
#include "refset_call.hpp"
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
        std::fill(t_call, t_call + 4, 0);
        const uint32_t k = set->k;
        CallSites S;
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
        resolve_sites(S, concat, offsets, c.o.sbwt_build_opts.add_revcomp != 0, call_threads(), out);
    });
}

} // extern "C"
