// kbo_capi.cpp — the extern "C" boundary declared in include/kbo_hip.h.
//
// Host logic only: argument checks mirroring the reference's asserts, index ownership,
// device-memory plumbing and kernel launches.  All matching-statistics / derandomize /
// translate / run-length compute happens in the *_kernels.hip files; nothing here falls back to the CPU.
#include "../../include/kbo_hip.h"
#include "../../include/kbo_hip_tuning.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdlib>
#include <chrono>
#include <cstdio>
#include <condition_variable>
#include <functional>
#include <memory>
#include <cstring>
#include <deque>
#include <map>
#include <mutex>
#include <new>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "capi_internal.hpp"

using namespace kbo_host;

namespace kbo_host {

// rows the index would have, at most: one per base and strand (+ dummies).  Beyond 32-bit row numbers (a human genome with its reverse
// complements) - or when a test asks for it - kbo_index_build builds the index as shards (capi_internal.hpp)
size_t shards_wanted(uint64_t bases, bool add_revcomp)
{
    const uint64_t est_rows = bases * (add_revcomp ? 2u : 1u);
    const uint64_t kShardRows = 0xE0000000ull; // (3.76 * 10^9: leaves room for the dummy rows)
    const int forced = g_index_shards.load();
    return forced > 0 ? (size_t)forced : (size_t)((est_rows + kShardRows - 1) / kShardRows);
}

// ---- A3: derandomize.rs:91-145, f64, identical operation order -------------------------
double powi_f64(double a, int b) // Rust f64::powi == llvm.powi == compiler-rt __powidf2
{
    const bool recip = b < 0;
    double r = 1;
    for (;;) {
        if (b & 1) r *= a;
        b /= 2;
        if (b == 0) break;
        a *= a;
    }
    return recip ? 1 / r : r;
}

double log_rm_max_cdf(size_t t, size_t alphabet_size, size_t n_kmers)
{
    KBO_REQUIRE(n_kmers > 0, KBO_E_BAD_ARG, "n_kmers > 0 (derandomize.rs:96)");
    KBO_REQUIRE(alphabet_size > 0, KBO_E_BAD_ARG, "alphabet_size > 0 (derandomize.rs:97)");
    return (double)n_kmers *
           std::log1p(-powi_f64(std::exp(std::log(1.0) - std::log((double)alphabet_size)), (int)t + 1));
}

size_t random_match_threshold(size_t k, size_t n_kmers, size_t alphabet_size, double p)
{
    KBO_REQUIRE(k > 0, KBO_E_BAD_ARG, "k > 0 (derandomize.rs:133)");
    KBO_REQUIRE(n_kmers > 0, KBO_E_BAD_ARG, "n_kmers > 0 (derandomize.rs:134)");
    KBO_REQUIRE(alphabet_size > 0, KBO_E_BAD_ARG, "alphabet_size > 0 (derandomize.rs:135)");
    KBO_REQUIRE(p <= 1.0 && p > 0.0, KBO_E_BAD_ARG, "0 < max_error_prob <= 1 (derandomize.rs:136-137)");
    for (size_t i = 1; i < k; i++)
        if (log_rm_max_cdf(i, alphabet_size, n_kmers) > std::log1p(-p)) return i;
    return k;
}

} // namespace kbo_host

namespace {

// matching statistics with intervals of a list of sequences, batched on the GPU
kbo::MsFn make_ms_fn(kbo_index *idx)
{
    return [idx](const std::vector<std::vector<uint8_t>> &seqs, std::vector<std::vector<kbo::MsVal>> &out) {
        out.assign(seqs.size(), {});
        if (seqs.empty()) return;
        std::vector<uint64_t> off(seqs.size() + 1, 0);
        for (size_t s = 0; s < seqs.size(); s++) off[s + 1] = off[s] + seqs[s].size();
        std::vector<uint8_t> concat(off.back());
        for (size_t s = 0; s < seqs.size(); s++) std::memcpy(concat.data() + off[s], seqs[s].data(), seqs[s].size());
        hipStream_t stream = nullptr;
        BatchOnDevice B;
        run_walk_host(idx, concat.data(), off.data(), seqs.size(), true, B, stream);
        std::vector<uint8_t> d(B.total);
        std::vector<uint32_t> lo(B.total), hi(B.total);
        HIP_OK(hipMemcpy(d.data(), B.ms.p, B.total, hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(lo.data(), B.lo.p, B.total * 4, hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(hi.data(), B.hi.p, B.total * 4, hipMemcpyDeviceToHost));
        for (size_t s = 0; s < seqs.size(); s++) {
            out[s].resize(seqs[s].size());
            for (size_t i = 0; i < seqs[s].size(); i++) out[s][i] = kbo::MsVal{d[off[s] + i], lo[off[s] + i], hi[off[s] + i]};
        }
    };
}

// lib.rs:735-738 for one sequence with an explicit threshold: MS (with intervals) + A5 + A6 on the GPU
void ms_and_translation(kbo_index *idx, const uint8_t *seq, size_t len, size_t threshold, std::vector<kbo::MsVal> &ms,
                        std::vector<uint8_t> &chars)
{
    KBO_REQUIRE(len > 0, KBO_E_EMPTY_QUERY, "assert!(!query.is_empty()) (index.rs:248)");
    const uint64_t off[2] = {0, len};
    check_len_threshold(off, 1, idx->host.k, threshold);
    hipStream_t stream = nullptr;
    BatchOnDevice B;
    run_walk_host(idx, seq, off, 1, true, B, stream);
    DevBuf dch(((len + 15) / 16) * 16 + 16);
    derand_translate_host_offsets(B.ms.as<uint8_t>(), B.off.as<uint64_t>(), off, 1, idx->host.k, (uint32_t)threshold,
                                  nullptr, dch.as<uint8_t>(), nullptr, stream);
    std::vector<uint8_t> d(len);
    std::vector<uint32_t> lo(len), hi(len);
    chars.resize(len);
    HIP_OK(hipMemcpy(d.data(), B.ms.p, len, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(lo.data(), B.lo.p, len * 4, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(hi.data(), B.hi.p, len * 4, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(chars.data(), dch.p, len, hipMemcpyDeviceToHost));
    ms.resize(len);
    for (size_t i = 0; i < len; i++) ms[i] = kbo::MsVal{d[i], lo[i], hi[i]};
}

// kbo::call (lib.rs:547-573)
std::vector<kbo::Variant> call_impl(kbo_index *query_idx, const uint8_t *ref_seq, size_t len, const kbo_call_opts &o)
{
    kbo_index ref_idx; // lib.rs:553: an index of ref_seq is built on every call
    kbo::BuildParams p;
    p.k = o.sbwt_build_opts.k;
    p.add_revcomp = o.sbwt_build_opts.add_revcomp != 0;
    p.num_threads = std::max(1u, o.sbwt_build_opts.num_threads);
    const uint8_t *seqs[1] = {ref_seq};
    const size_t lens[1] = {len};
    kbo::build_host_index(seqs, lens, 1, p, ref_idx.host);
    KBO_REQUIRE(ref_idx.host.k == query_idx->host.k, KBO_E_K_MISMATCH, "assert!(sbwt_ref.k() == sbwt_query.k()) (lib.rs:559)");
    // variant_calling.rs:260 — callee's sbwt_ref is kbo's query index (lib.rs:561-568)
    const size_t d = random_match_threshold(query_idx->host.k, query_idx->host.n_kmers, 4, o.max_error_prob);
    kbo::HostNav nav(query_idx->host);
    return kbo::call_variants(nav, make_ms_fn(query_idx), make_ms_fn(&ref_idx), query_idx->host.k, ref_seq, len, d);
}

kbo_variant *pack_variants(const std::vector<kbo::Variant> &v)
{
    size_t chars = 0;
    for (const auto &x : v) chars += x.query_chars.size() + x.ref_chars.size();
    const size_t head = std::max<size_t>(1, v.size()) * sizeof(kbo_variant);
    MallocPtr<uint8_t> mem = malloc_array<uint8_t>(head + chars + 1);
    kbo_variant *out = reinterpret_cast<kbo_variant *>(mem.get());
    uint8_t *cp = mem.get() + head;
    for (size_t i = 0; i < v.size(); i++) {
        out[i].query_pos = v[i].query_pos;
        out[i].query_chars = cp;
        out[i].query_len = v[i].query_chars.size();
        std::memcpy(cp, v[i].query_chars.data(), v[i].query_chars.size());
        cp += v[i].query_chars.size();
        out[i].ref_chars = cp;
        out[i].ref_len = v[i].ref_chars.size();
        std::memcpy(cp, v[i].ref_chars.data(), v[i].ref_chars.size());
        cp += v[i].ref_chars.size();
    }
    return reinterpret_cast<kbo_variant *>(mem.release());
}

// format.rs:143-193, statement for statement (sequential, variable-length output: host).  Returns false where the reference
// panics: an 'R' at position 0 that starts a run makes format.rs:175 evaluate aln[i - 1] with i = 0 (usize underflow).
bool run_lengths_gapped_impl(const uint8_t *aln, size_t len, size_t max_gap_len, std::vector<kbo_rle> &out)
{
    size_t i = 0;
    bool match_start = false;
    while (i < len) {
        match_start = (aln[i] != '-' && aln[i] != ' ') && !match_start;
        if (match_start) {
            kbo_rle rle{(uint64_t)i, 0, 0, 0, 0, 0, 0};
            size_t within_gap_bases = 0;
            bool within_gap_start = false;
            while (i < len && aln[i] != ' ') {
                const bool is_true_gap = aln[i] == '-';
                if (is_true_gap && !within_gap_start) {
                    within_gap_start = true;
                    rle.gap_opens += 1;
                    within_gap_bases = 0;
                }
                if (!is_true_gap && within_gap_start) within_gap_start = false;
                const bool is_match = aln[i] == 'M' || aln[i] == 'R' || aln[i] == 'I';
                const bool is_gap = is_true_gap || aln[i] == 'D';
                rle.matches += is_match;
                rle.gap_bases += is_gap;
                rle.mismatches += (!is_match && !is_gap);
                rle.end = (is_match || !is_gap) ? i + 1 : rle.end;
                if (aln[i] == 'R' && i == 0) return false; // (format.rs:175: aln[i - 1] with i = 0)
                rle.jumps += (aln[i] == 'R' && aln[i - 1] == 'R');
                within_gap_bases += (aln[i] == '-');
                i += 1;
                if (within_gap_bases > max_gap_len || (is_gap && i == len && rle.gap_opens > 0)) {
                    rle.gap_opens -= 1;
                    rle.gap_bases -= within_gap_bases;
                    break;
                }
            }
            out.push_back(rle);
            match_start = false;
        } else {
            i += 1;
        }
    }
    return true;
}

kbo_rle *copy_rles(const std::vector<kbo_rle> &v)
{
    MallocPtr<kbo_rle> p = malloc_array<kbo_rle>(v.size());
    if (!v.empty()) std::memcpy(p.get(), v.data(), v.size() * sizeof(kbo_rle));
    return p.release();
}

// kbo::find over a batch (lib.rs:815-820: matches, then run_lengths_gapped per sequence; both on the device, slab by slab): the
// caller's sink - its record array library-allocated, or the caller's buffer (use_buffer) - made ready from the options (null:
// the defaults).  Returns their max_error_prob.
template <typename T> double prepare_find(RleSink<T> &sink, const kbo_find_opts *opts, uint64_t *rle_offsets)
{
    kbo_find_opts o;
    if (opts) o = *opts; else kbo_find_opts_default(&o);
    sink.max_gap_len = o.max_gap_len;
    sink.rle_offsets = rle_offsets;
    return o.max_error_prob;
}

} // namespace


extern "C" {

const char *kbo_last_error(void) { return last_error().c_str(); }
const char *kbo_version(void) { return "kbo-hip 0.1.0 (gfx950)"; }

void kbo_build_opts_default(kbo_build_opts *o)
{
    if (!o) return;
    o->k = 31; o->add_revcomp = 0; o->num_threads = 1; o->prefix_precalc = 8;
    o->build_select = 0; o->mem_gb = 4; o->dedup_batches = 0; o->temp_dir = nullptr;
}
void kbo_find_opts_default(kbo_find_opts *o)
{
    if (!o) return;
    o->max_error_prob = 0.0000001; o->max_gap_len = 0;
}
void kbo_call_opts_default(kbo_call_opts *o)
{
    if (!o) return;
    o->max_error_prob = 0.0000001;
    kbo_build_opts_default(&o->sbwt_build_opts);
    o->sbwt_build_opts.build_select = 1;
}
void kbo_map_opts_default(kbo_map_opts *o)
{
    if (!o) return;
    o->max_error_prob = 0.0000001; o->fill_gaps = 1; o->call_variants = 1; o->format = 1;
    kbo_build_opts_default(&o->sbwt_build_opts);
    o->sbwt_build_opts.build_select = 1;
}

namespace {
// A sharded index (capi_internal.hpp kbo_index::shards): `want` shards or more over disjoint parts of the input - groups of
// whole sequences of about equal size, and with add_revcomp the forward and the reverse-complement strand of every group
// apart.  The set of strings (of at most k characters) that are suffixes of rows of an SBWT is the set of substrings of its
// input's ACGT-runs of at least k characters - a property of the runs, hence of the sequences one by one - so the depth of a
// walk against the index of everything is the maximum of the depths against the shards.  The threshold of the derandomisation
// needs the number of distinct k-mers of the union: every shard hands back its sorted k-mers and a merge counts them once.
void build_sharded(const uint8_t *const *seqs, const size_t *lens, size_t n_seqs, const kbo::BuildParams &p, size_t want, kbo_index &out)
{
    const size_t strands = p.add_revcomp ? 2 : 1;
    const size_t groups = std::max<size_t>(1, std::min(n_seqs, (want + strands - 1) / strands));
    uint64_t bases = 0;
    for (size_t s = 0; s < n_seqs; s++) bases += lens[s];
    // contiguous groups of sequences with about bases / groups bases each
    std::vector<size_t> first(groups + 1, n_seqs);
    first[0] = 0;
    {
        uint64_t acc = 0;
        size_t g = 1;
        for (size_t s = 0; s < n_seqs && g < groups; s++) {
            acc += lens[s];
            if (acc >= bases * g / groups && s + 1 < n_seqs) first[g++] = s + 1;
        }
    }
    std::vector<std::vector<uint64_t>> keys;
    uint32_t key_words = 0;
    uint64_t n_sets = 0;
    for (size_t g = 0; g < groups; g++) {
        if (first[g] >= first[g + 1]) continue;
        for (size_t st = 0; st < strands; st++) {
            kbo::BuildParams q = p;
            q.add_revcomp = false;
            q.revcomp_only = st == 1;
            keys.emplace_back();
            q.keys_out = &keys.back();
            q.key_words_out = &key_words;
            std::unique_ptr<kbo_index> sh(new kbo_index());
            try {
                kbo::build_host_index(seqs + first[g], lens + first[g], first[g + 1] - first[g], q, sh->host);
            } catch (const std::runtime_error &e) { // (a shard that is itself too large: sequences are never cut)
                throw KboError(KBO_E_UNSUPPORTED,
                               std::string("sharded build: shard ") + std::to_string(out.shards.size()) + " (sequences " + std::to_string(first[g]) + " .. " +
                               std::to_string(first[g + 1] - 1) + ", " + (st ? "reverse-complement" : "forward") + " strand) failed: " + e.what() +
                               " - shards hold whole sequences, so one sequence with 2^32 or more distinct k-mers cannot be indexed");
            }
            n_sets += sh->host.n_sets;
            out.shards.push_back(std::move(sh));
        }
    }
    // distinct k-mers of the union: a merge over the shards' sorted key lists (equal k-mers have equal keys everywhere)
    const size_t W = key_words ? key_words : 1;
    std::vector<size_t> at(keys.size(), 0);
    uint64_t distinct = 0;
    auto less = [&](const uint64_t *a, const uint64_t *b) {
        for (size_t j = 0; j < W; j++)
            if (a[j] != b[j]) return a[j] < b[j];
        return false;
    };
    uint64_t cur[8]; // (k <= 255: at most 8 words a key)
    KBO_REQUIRE(W <= 8, KBO_E_UNSUPPORTED, "k-mer keys wider than 8 words");
    for (;;) {
        const uint64_t *best = nullptr;
        for (size_t x = 0; x < keys.size(); x++) {
            if (at[x] * W >= keys[x].size()) continue;
            const uint64_t *c = keys[x].data() + at[x] * W;
            if (!best || less(c, best)) best = c;
        }
        if (!best) break;
        distinct++;
        std::copy(best, best + W, cur); // (advance every list past this k-mer)
        for (size_t x = 0; x < keys.size(); x++)
            while (at[x] * W < keys[x].size() && std::equal(cur, cur + W, keys[x].data() + at[x] * W)) at[x]++;
    }
    out.host.k = p.k;
    out.host.n_kmers = distinct;
    out.host.n_sets = n_sets; // (rows over all shards; the index of the union would have fewer dummy rows)
}
} // namespace

int kbo_index_build(const uint8_t *const *seqs, const size_t *lens, size_t n_seqs,
                    const kbo_build_opts *opts, kbo_index_t **out)
{
    return guarded([&] {
        KBO_REQUIRE(out, KBO_E_BAD_ARG, "null out");
        *out = nullptr;
        KBO_REQUIRE(seqs && lens && n_seqs > 0, KBO_E_BAD_ARG, "assert!(!slices.is_empty()) (index.rs:60)");
        kbo_build_opts o;
        if (opts) o = *opts; else kbo_build_opts_default(&o);
        kbo::BuildParams p;
        p.k = o.k; p.add_revcomp = o.add_revcomp != 0; p.num_threads = std::max(1u, o.num_threads);
        // rows the index would have, at most: one per base and strand (+ dummies).  Beyond 32-bit row numbers (a human genome
        // with its reverse complements) - or when a test asks for it - the index is built as shards (capi_internal.hpp)
        uint64_t bases = 0;
        for (size_t s = 0; s < n_seqs; s++) bases += lens[s];
        const size_t want = shards_wanted(bases, p.add_revcomp);
        std::unique_ptr<kbo_index> idx(new kbo_index());
        if (want <= 1) kbo::build_host_index(seqs, lens, n_seqs, p, idx->host);
        else build_sharded(seqs, lens, n_seqs, p, want, *idx);
        *out = idx.release();
    });
}

int kbo_index_from_parts(uint32_t k, uint64_t n_sets, uint64_t n_kmers, const uint64_t *const rows[4],
                         const uint64_t C[4], const uint8_t *lcs, kbo_index_t **out)
{
    return guarded([&] {
        KBO_REQUIRE(out, KBO_E_BAD_ARG, "null out");
        *out = nullptr;
        KBO_REQUIRE(rows && C && lcs && k > 0 && k <= 255 && n_sets > 0, KBO_E_BAD_ARG, "bad index parts");
        kbo_index *idx = new kbo_index();
        idx->host.k = k; idx->host.n_sets = n_sets; idx->host.n_kmers = n_kmers;
        const size_t nw = (n_sets + 63) / 64;
        for (int c = 0; c < 4; c++) {
            idx->host.C[c] = C[c];
            idx->host.rows[c].assign(rows[c], rows[c] + nw);
            if (n_sets & 63) idx->host.rows[c][nw - 1] &= (1ull << (n_sets & 63)) - 1;
        }
        idx->host.lcs.assign(lcs, lcs + n_sets);
        idx->host.lcs[0] = 0;
        try {
            kbo::validate_host_index(idx->host); // C[] vs edge bits, LCS < k: the kernels trust them
        } catch (...) {
            delete idx;
            throw;
        }
        *out = idx;
    });
}

int kbo_index_export_parts(const kbo_index_t *idx, uint64_t *const rows[4], uint64_t C[4], uint8_t *lcs)
{
    return guarded([&] {
        KBO_REQUIRE(idx && rows && C && lcs, KBO_E_BAD_ARG, "null argument");
        require_unsharded(idx, "kbo_index_export_parts");
        const size_t nw = (idx->host.n_sets + 63) / 64;
        for (int c = 0; c < 4; c++) {
            C[c] = idx->host.C[c];
            std::memcpy(rows[c], idx->host.rows[c].data(), nw * sizeof(uint64_t));
        }
        std::memcpy(lcs, idx->host.lcs.data(), idx->host.n_sets);
    });
}

void kbo_index_free(kbo_index_t *idx) { delete idx; }
size_t kbo_index_k(const kbo_index_t *idx) { return idx ? idx->host.k : 0; }
uint64_t kbo_index_n_kmers(const kbo_index_t *idx) { return idx ? idx->host.n_kmers : 0; }
uint64_t kbo_index_n_sets(const kbo_index_t *idx) { return idx ? idx->host.n_sets : 0; }

int kbo_index_save(const kbo_index_t *idx_c, const char *path)
{
    kbo_index_t *idx = const_cast<kbo_index_t *>(idx_c); // (the handle's cache of its path cover is filled in under its mutex)
    int rc = guarded([&] {
        KBO_REQUIRE(idx && path, KBO_E_BAD_ARG, "null argument");
        std::lock_guard<std::mutex> g(idx->mu);
        require_unsharded(idx, "kbo_index_save");
        if (plan_enabled(idx) && !idx->cover && !idx->transient && idx->host.n_sets < 0xFFFFFFF0ull) {
            idx->cover.reset(new kbo::PathCover());
            kbo::make_path_cover(idx->host, *idx->cover);
        }
        kbo::save_host_index(idx->host, path, plan_enabled(idx) ? idx->cover.get() : nullptr);
    });
    return rc == KBO_E_BAD_ARG && idx && path ? KBO_E_IO : rc;
}

int kbo_index_load(const char *path, kbo_index_t **out)
{
    int rc = guarded([&] {
        KBO_REQUIRE(path && out, KBO_E_BAD_ARG, "null argument");
        *out = nullptr;
        kbo_index *idx = new kbo_index();
        try {
            std::unique_ptr<kbo::PathCover> pc(new kbo::PathCover());
            bool have = false;
            kbo::load_host_index(path, idx->host, pc.get(), &have);
            if (have) idx->cover = std::move(pc);
        } catch (...) {
            delete idx;
            throw;
        }
        *out = idx;
    });
    return rc == KBO_E_BAD_ARG && path && out ? KBO_E_IO : rc;
}

int kbo_index_save_sbwt(const kbo_index_t *idx, const char *prefix)
{
    int rc = guarded([&] {
        KBO_REQUIRE(idx && prefix, KBO_E_BAD_ARG, "null argument");
        require_unsharded(idx, "kbo_index_save_sbwt");
        kbo::save_sbwt_pair(idx->host, prefix);
    });
    return rc == KBO_E_BAD_ARG && idx && prefix ? KBO_E_IO : rc;
}

int kbo_index_load_sbwt(const char *prefix, kbo_index_t **out)
{
    int rc = guarded([&] {
        KBO_REQUIRE(prefix && out, KBO_E_BAD_ARG, "null argument");
        *out = nullptr;
        kbo_index *idx = new kbo_index();
        bool own = false;
        try {
            own = kbo::load_sbwt_pair(prefix, idx->host);
        } catch (...) {
            delete idx;
            throw;
        }
        if (!own) {
            delete idx;
            throw KboError(KBO_E_UNSUPPORTED,
                           std::string(prefix) + ".sbwt was written by the sbwt crate: its field layout behind the SubsetMatrix tag is not "
                           "pinned by the reference (index.rs:143); hand the index over with kbo_index_from_parts");
        }
        *out = idx;
    });
    return rc == KBO_E_BAD_ARG && prefix && out ? KBO_E_IO : rc;
}

int kbo_index_to_device(kbo_index_t *idx, int device)
{
    return guarded([&] {
        KBO_REQUIRE(idx, KBO_E_BAD_ARG, "null index");
        for (kbo_index *sh : shards_of(idx)) (void)device_view(sh, resolve_device(device), nullptr, 0, true);
    });
}

int kbo_index_device_bytes(const kbo_index_t *idx, uint64_t *rank_bytes, uint64_t *lcs_bytes)
{
    return guarded([&] {
        KBO_REQUIRE(idx, KBO_E_BAD_ARG, "null index");
        uint64_t rb = 0, lb = 0; // (a sharded index: over all shards)
        for (kbo_index *sh : shards_of(const_cast<kbo_index *>(idx))) {
            rb += (sh->host.n_sets / kbo::kRankRowsPerBlock + 2) * 16 * 4;
            lb += (3 * (sh->host.n_sets + 1) + 4) * sizeof(uint32_t);
        }
        if (rank_bytes) *rank_bytes = rb;
        if (lcs_bytes) *lcs_bytes = lb;
    });
}

uint64_t kbo_index_device_pair_bytes(const kbo_index_t *idx)
{
    if (!idx) return 0;
    uint64_t total = 0; // what the device copies actually carry (none for the 64-bit entry layout)
    for (kbo_index *sh : shards_of(const_cast<kbo_index *>(idx))) {
        uint64_t bytes = 0;
        std::lock_guard<std::mutex> g(sh->mu);
        for (const auto &kv : sh->dev)
            if (kv.second->pair_off) bytes = std::max<uint64_t>(bytes, (kv.second->n_blocks) * 16ull * 16ull);
        total += bytes;
    }
    return total;
}

int kbo_log_rm_max_cdf(size_t t, size_t alphabet_size, size_t n_kmers, double *out)
{
    return guarded([&] {
        KBO_REQUIRE(out, KBO_E_BAD_ARG, "null out");
        *out = log_rm_max_cdf(t, alphabet_size, n_kmers);
    });
}

int kbo_random_match_threshold(size_t k, size_t n_kmers, size_t alphabet_size, double max_error_prob,
                               size_t *out)
{
    return guarded([&] {
        KBO_REQUIRE(out, KBO_E_BAD_ARG, "null out");
        *out = random_match_threshold(k, n_kmers, alphabet_size, max_error_prob);
    });
}

int kbo_ms_batch(kbo_index_t *idx, const uint8_t *concat, const uint64_t *offsets, size_t n_seqs,
                 uint8_t *d_out, uint32_t *lo_out, uint32_t *hi_out)
{
    return guarded([&] { ms_batch_impl(idx, concat, offsets, n_seqs, d_out, lo_out, hi_out); });
}

int kbo_matching_statistics(kbo_index_t *idx, const uint8_t *query, size_t len, uint64_t *d, uint64_t *lo,
                            uint64_t *hi)
{
    return guarded([&] {
        KBO_REQUIRE(idx && query && d, KBO_E_BAD_ARG, "null argument");
        KBO_REQUIRE(len > 0, KBO_E_EMPTY_QUERY, "assert!(!query.is_empty()) (index.rs:248)");
        KBO_REQUIRE((lo == nullptr) == (hi == nullptr), KBO_E_BAD_ARG, "lo/hi must come together");
        const uint64_t off[2] = {0, len};
        std::vector<uint8_t> d8(len);
        std::vector<uint32_t> lo32, hi32;
        if (lo) { lo32.resize(len); hi32.resize(len); }
        int rc = kbo_ms_batch(idx, query, off, 1, d8.data(), lo ? lo32.data() : nullptr,
                              lo ? hi32.data() : nullptr);
        if (rc) throw KboError(rc, last_error());
        for (size_t i = 0; i < len; i++) d[i] = d8[i]; // widen to the reference's usize
        if (lo)
            for (size_t i = 0; i < len; i++) { lo[i] = lo32[i]; hi[i] = hi32[i]; }
    });
}

int kbo_derandomize_ms_val(size_t curr, int64_t next, size_t threshold, size_t k, int64_t *out)
{
    return guarded([&] {
        KBO_REQUIRE(out, KBO_E_BAD_ARG, "null out");
        KBO_REQUIRE(k > 0, KBO_E_BAD_ARG, "k > 0 (derandomize.rs:227)");
        KBO_REQUIRE(threshold > 1, KBO_E_THRESHOLD_LE_1, "threshold > 1 (derandomize.rs:228)");
        KBO_REQUIRE(curr <= k, KBO_E_MS_RANGE, "curr_noisy_ms <= k (derandomize.rs:229)");
        KBO_REQUIRE(next <= (int64_t)k, KBO_E_MS_RANGE, "next_derand_ms <= k (derandomize.rs:230)");
        int64_t run = next - 1;
        if (curr == k) run = (int64_t)k;
        if (curr > threshold && next < (int64_t)curr) run = (int64_t)curr;
        *out = run;
    });
}

int kbo_derandomize_ms_vec(const uint64_t *noisy, size_t len, size_t k, size_t threshold, int64_t *out)
{
    return guarded([&] {
        KBO_REQUIRE(noisy && out, KBO_E_BAD_ARG, "null argument");
        KBO_REQUIRE(k > 0, KBO_E_BAD_ARG, "k > 0 (derandomize.rs:274)");
        KBO_REQUIRE(threshold > 1, KBO_E_THRESHOLD_LE_1, "threshold > 1 (derandomize.rs:275)");
        KBO_REQUIRE(len > 2, KBO_E_LEN_LE_2, "len > 2 (derandomize.rs:276)");
        KBO_REQUIRE(k <= 255, KBO_E_UNSUPPORTED, "k > 255");
        std::vector<uint8_t> n8(((len + 15) / 16) * 16 + 16, 0);
        for (size_t i = 0; i < len; i++) {
            KBO_REQUIRE(noisy[i] <= k, KBO_E_MS_RANGE, "curr_noisy_ms <= k (derandomize.rs:229)");
            n8[i] = (uint8_t)noisy[i]; // narrow usize -> u8 (values <= k <= 255)
        }
        hipStream_t stream = nullptr;
        const uint64_t off[2] = {0, len};
        DevBuf dms(n8.size()), doff(sizeof(off)), dch(n8.size()), dder(len * sizeof(int32_t));
        HIP_OK(hipMemcpyAsync(dms.p, n8.data(), n8.size(), hipMemcpyHostToDevice, stream));
        HIP_OK(hipMemcpyAsync(doff.p, off, sizeof(off), hipMemcpyHostToDevice, stream));
        derand_translate_host_offsets(dms.as<uint8_t>(), doff.as<uint64_t>(), off, 1, (uint32_t)k,
                                      (uint32_t)std::min<size_t>(threshold, 0x7FFFFFFF), nullptr,
                                      dch.as<uint8_t>(), dder.as<int32_t>(), stream);
        std::vector<int32_t> d32(len);
        HIP_OK(hipMemcpyAsync(d32.data(), dder.p, len * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
        HIP_OK(hipStreamSynchronize(stream));
        for (size_t i = 0; i < len; i++) out[i] = d32[i];
    });
}

int kbo_translate_ms_val(int64_t curr, int64_t next, int64_t prev, size_t threshold, uint32_t *aln_curr,
                         uint32_t *aln_next)
{
    return guarded([&] {
        KBO_REQUIRE(aln_curr && aln_next, KBO_E_BAD_ARG, "null out");
        KBO_REQUIRE(threshold > 1, KBO_E_THRESHOLD_LE_1, "threshold > 1 (translate.rs:186)");
        *aln_next = ' ';
        const int64_t t = (int64_t)threshold;
        if (curr > t && next > 0 && next < t) { *aln_curr = 'R'; *aln_next = 'R'; }
        else if (curr <= 0) *aln_curr = (next == 1 && prev > 0) ? 'X' : '-';
        else *aln_curr = 'M';
    });
}

int kbo_translate_ms_vec(const int64_t *derand, size_t len, size_t k, size_t threshold, uint32_t *out)
{
    return guarded([&] {
        KBO_REQUIRE(derand && out, KBO_E_BAD_ARG, "null argument");
        KBO_REQUIRE(k > 0, KBO_E_BAD_ARG, "k > 0 (translate.rs:268)");
        KBO_REQUIRE(threshold > 1, KBO_E_THRESHOLD_LE_1, "threshold > 1 (translate.rs:269)");
        KBO_REQUIRE(len > 2, KBO_E_LEN_LE_2, "len > 2 (translate.rs:270)");
        KBO_REQUIRE(len < 0xFFFFFFFFull, KBO_E_UNSUPPORTED, "vector longer than 2^32-1");
        // the stencil only compares values with 0, 1, threshold and k: clamping i64 -> i32
        // preserves every comparison as long as threshold and k fit in i32
        const int64_t lim = 0x7FFFFFF0;
        std::vector<int32_t> x(len);
        for (size_t i = 0; i < len; i++) x[i] = (int32_t)std::max<int64_t>(-lim, std::min<int64_t>(lim, derand[i]));
        const uint32_t t32 = (uint32_t)std::min<size_t>(threshold, (size_t)lim - 1);
        const uint32_t k32 = (uint32_t)std::min<size_t>(k, (size_t)lim - 1);
        hipStream_t stream = nullptr;
        DevBuf dx(len * sizeof(int32_t)), dch(len);
        HIP_OK(hipMemcpyAsync(dx.p, x.data(), len * sizeof(int32_t), hipMemcpyHostToDevice, stream));
        HIP_OK(kbo::launch_translate(dx.as<int32_t>(), len, k32, t32, dch.as<uint8_t>(), stream));
        std::vector<uint8_t> ch(len);
        HIP_OK(hipMemcpyAsync(ch.data(), dch.p, len, hipMemcpyDeviceToHost, stream));
        HIP_OK(hipStreamSynchronize(stream));
        for (size_t i = 0; i < len; i++) out[i] = ch[i]; // widen u8 -> Rust char
    });
}

int kbo_matches_batch(kbo_index_t *idx, const uint8_t *concat, const uint64_t *offsets, size_t n_seqs,
                      double max_error_prob, uint8_t *chars_out)
{
    return guarded([&] { matches_batch_impl(idx, concat, offsets, n_seqs, max_error_prob, HostOut::chars(chars_out, nullptr, false)); });
}

int kbo_summary_batch(kbo_index_t *idx, const uint8_t *concat, const uint64_t *offsets, size_t n_seqs, double max_error_prob,
                      kbo_aln_summary *summary_out)
{
    return guarded([&] {
        KBO_REQUIRE(summary_out, KBO_E_BAD_ARG, "null argument");
        matches_batch_impl(idx, concat, offsets, n_seqs, max_error_prob, HostOut::summary(summary_out));
    });
}

int kbo_map_batch(kbo_index_t *idx, const uint8_t *concat, const uint64_t *offsets, size_t n_seqs,
                  double max_error_prob, int format, uint8_t *out)
{
    return guarded([&] { matches_batch_impl(idx, concat, offsets, n_seqs, max_error_prob, HostOut::chars(out, nullptr, format != 0)); });
}

int kbo_matches(kbo_index_t *idx, const uint8_t *query, size_t len, double max_error_prob, uint32_t *chars_out)
{
    return guarded([&] {
        KBO_REQUIRE(idx && query && chars_out, KBO_E_BAD_ARG, "null argument");
        KBO_REQUIRE(len > 0, KBO_E_EMPTY_QUERY, "assert!(!query.is_empty()) (index.rs:248)");
        const uint64_t off[2] = {0, len};
        std::vector<uint8_t> ch(len);
        matches_batch_impl(idx, query, off, 1, max_error_prob, HostOut::chars(ch.data(), nullptr, false));
        for (size_t i = 0; i < len; i++) chars_out[i] = ch[i];
    });
}

int kbo_map(kbo_index_t *idx, const uint8_t *ref_seq, size_t len, const kbo_map_opts *opts, uint8_t *out)
{
    return guarded([&] {
        KBO_REQUIRE(idx && ref_seq && out, KBO_E_BAD_ARG, "null argument");
        kbo_map_opts o;
        if (opts) o = *opts; else kbo_map_opts_default(&o);
        if (o.call_variants)
            KBO_REQUIRE(idx->host.k == o.sbwt_build_opts.k, KBO_E_K_MISMATCH,
                        "assert!(sbwt.k() == map_opts.sbwt_build_opts.k) (lib.rs:729)");
        KBO_REQUIRE(len > 0, KBO_E_EMPTY_QUERY, "assert!(!query.is_empty()) (index.rs:248)");
        if (!o.fill_gaps && !o.call_variants) { // everything on the GPU, incl. relative_to_ref
            const uint64_t off[2] = {0, len};
            matches_batch_impl(idx, ref_seq, off, 1, o.max_error_prob, HostOut::chars(out, nullptr, o.format != 0));
            return;
        }
        require_unsharded(idx, "kbo_map with fill_gaps / call_variants");
        const size_t threshold = random_match_threshold(idx->host.k, idx->host.n_kmers, 4, o.max_error_prob); // lib.rs:731
        std::vector<kbo::MsVal> ms;
        std::vector<uint8_t> refined;
        ms_and_translation(idx, ref_seq, len, threshold, ms, refined);                                       // lib.rs:735-738
        if (o.fill_gaps) {                                                                                   // lib.rs:743-747
            kbo::HostNav nav(idx->host);
            refined = kbo::fill_gaps(refined, ms, ref_seq, len, nav, threshold, o.max_error_prob);
        }
        if (o.call_variants) {                                                                               // lib.rs:749-754
            kbo_call_opts co;
            co.max_error_prob = o.max_error_prob;
            co.sbwt_build_opts = o.sbwt_build_opts;
            kbo::add_variants(refined, call_impl(idx, ref_seq, len, co));
        }
        if (o.format) {                                                                                      // lib.rs:756-760
            int rc = kbo_relative_to_ref(ref_seq, refined.data(), len, out);
            if (rc) throw KboError(rc, last_error());
        } else {
            std::memcpy(out, refined.data(), len);
        }
    });
}

int kbo_call(kbo_index_t *query_idx, const uint8_t *ref_seq, size_t len, const kbo_call_opts *opts, kbo_variant **out,
             size_t *n_out)
{
    return guarded([&] {
        KBO_REQUIRE(query_idx && ref_seq && out && n_out, KBO_E_BAD_ARG, "null argument");
        *out = nullptr;
        *n_out = 0;
        require_unsharded(query_idx, "kbo_call");
        KBO_REQUIRE(len > 0, KBO_E_EMPTY_QUERY, "assert!(!query.is_empty()) (index.rs:248)");
        kbo_call_opts o;
        if (opts) o = *opts; else kbo_call_opts_default(&o);
        std::vector<kbo::Variant> v = call_impl(query_idx, ref_seq, len, o);
        *out = pack_variants(v);
        *n_out = v.size();
    });
}

int kbo_add_variants(uint32_t *translation, size_t len, const kbo_variant *variants, size_t n_variants)
{
    return guarded([&] {
        KBO_REQUIRE(translation && (variants || n_variants == 0), KBO_E_BAD_ARG, "null argument");
        std::vector<uint8_t> t(len);
        for (size_t i = 0; i < len; i++) t[i] = (uint8_t)translation[i];
        std::vector<kbo::Variant> v(n_variants);
        for (size_t i = 0; i < n_variants; i++) {
            v[i].query_pos = variants[i].query_pos;
            v[i].query_chars.assign(variants[i].query_chars, variants[i].query_chars + variants[i].query_len);
            v[i].ref_chars.assign(variants[i].ref_chars, variants[i].ref_chars + variants[i].ref_len);
        }
        kbo::add_variants(t, v);
        for (size_t i = 0; i < len; i++) translation[i] = t[i];
    });
}

int kbo_fill_gaps(kbo_index_t *idx, const uint8_t *ref_seq, size_t len, size_t threshold, double max_err_prob,
                  uint32_t *out)
{
    return guarded([&] {
        KBO_REQUIRE(idx && ref_seq && out, KBO_E_BAD_ARG, "null argument");
        std::vector<kbo::MsVal> ms;
        require_unsharded(idx, "kbo_fill_gaps");
        std::vector<uint8_t> tr;
        ms_and_translation(idx, ref_seq, len, threshold, ms, tr);
        kbo::HostNav nav(idx->host);
        std::vector<uint8_t> refined = kbo::fill_gaps(tr, ms, ref_seq, len, nav, threshold, max_err_prob);
        for (size_t i = 0; i < len; i++) out[i] = refined[i];
    });
}

int kbo_nearest_unique_context(kbo_index_t *idx, const uint8_t *ref_seq, size_t len, size_t range_start,
                               size_t range_end, size_t *kmer_idx, uint8_t *kmer_out, size_t *kmer_len)
{
    return guarded([&] {
        KBO_REQUIRE(idx && ref_seq && kmer_idx && kmer_out && kmer_len, KBO_E_BAD_ARG, "null argument");
        require_unsharded(idx, "kbo_nearest_unique_context");
        std::vector<std::vector<uint8_t>> one(1, std::vector<uint8_t>(ref_seq, ref_seq + len));
        std::vector<std::vector<kbo::MsVal>> ms;
        make_ms_fn(idx)(one, ms);
        kbo::HostNav nav(idx->host);
        auto r = kbo::nearest_unique_context(ms[0], nav, range_start, range_end);
        *kmer_idx = r.first;
        *kmer_len = r.second.size();
        std::memcpy(kmer_out, r.second.data(), r.second.size());
    });
}

int kbo_run_lengths_gapped(const uint8_t *aln, size_t len, size_t max_gap_len, kbo_rle **out, size_t *n_out)
{
    return guarded([&] {
        KBO_REQUIRE((aln || len == 0) && out && n_out, KBO_E_BAD_ARG, "null argument");
        std::vector<kbo_rle> v;
        KBO_REQUIRE(run_lengths_gapped_impl(aln, len, max_gap_len, v), KBO_E_REF_PANIC,
                    "an 'R' at position 0: the reference indexes aln[i - 1] there (format.rs:175) and panics");
        *out = copy_rles(v);
        *n_out = v.size();
    });
}

int kbo_run_lengths_gapped_batch(const uint8_t *aln_concat, const uint64_t *offsets, size_t n_seqs, size_t max_gap_len,
                                 kbo_rle **rles, uint64_t *rle_offsets)
{
    return guarded([&] {
        KBO_REQUIRE(aln_concat && offsets && rles && rle_offsets, KBO_E_BAD_ARG, "null argument");
        KBO_REQUIRE(n_seqs > 0 && n_seqs < (1ull << 31), KBO_E_BAD_ARG, "1 .. 2^31-1 sequences");
        KBO_REQUIRE(offsets[0] == 0, KBO_E_BAD_ARG, "offsets[0] must be 0");
        const OffsetScan scan = scan_offsets(offsets, n_seqs);
        KBO_REQUIRE(scan.monotone, KBO_E_BAD_ARG, "offsets not monotone");
        KBO_REQUIRE(scan.longest < 0xFFFFFFFFull, KBO_E_UNSUPPORTED, "sequence longer than 2^32-1");
        const uint64_t total = offsets[n_seqs];
        hipStream_t st = nullptr;
        DevBuf chars(total + 64), off((n_seqs + 1) * sizeof(uint64_t)), count(16);
        DevBuf scratch(kbo::chunk_items_scratch_words((uint32_t)n_seqs) * sizeof(uint32_t));
        HIP_OK(hipMemsetAsync(static_cast<uint8_t *>(chars.p) + total, 0, 64, st));
        if (total) HIP_OK(hipMemcpyAsync(chars.p, aln_concat, total, hipMemcpyHostToDevice, st));
        HIP_OK(hipMemcpyAsync(off.p, offsets, (n_seqs + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, st));
        const uint32_t gap = (uint32_t)std::min<size_t>(max_gap_len, 0xFFFFFFFFu);
        const uint32_t longest = (uint32_t)scan.longest;
        HIP_OK(kbo::launch_rle_count(chars.as<uint8_t>(), off.as<uint64_t>(), (uint32_t)n_seqs, gap, scratch.as<uint32_t>(),
                                     count.as<uint32_t>(), st, longest));
        uint32_t n_runs = 0;
        HIP_OK(hipMemcpy(&n_runs, count.p, sizeof(uint32_t), hipMemcpyDeviceToHost));
        DevBuf d_runs(std::max<size_t>(16, (size_t)n_runs * kRleWords * sizeof(uint32_t)));
        HIP_OK(kbo::launch_rle_emit(chars.as<uint8_t>(), off.as<uint64_t>(), (uint32_t)n_seqs, gap, scratch.as<uint32_t>(),
                                    d_runs.as<uint32_t>(), n_runs, st, longest));
        std::vector<uint32_t> compact((size_t)n_runs * kRleWords + 1), words(kbo::chunk_items_scratch_words((uint32_t)n_seqs));
        if (n_runs) HIP_OK(hipMemcpy(compact.data(), d_runs.p, (size_t)n_runs * kRleWords * sizeof(uint32_t), hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(words.data(), scratch.p, words.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
        MallocPtr<kbo_rle> all = malloc_array<kbo_rle>(n_runs);
        widen_rles(all.get(), compact.data(), n_runs, HostTeam::get());
        const uint32_t *local = words.data(), *sums = local + n_seqs + 1;
        for (size_t q = 0; q <= n_seqs; q++) rle_offsets[q] = (uint64_t)sums[q / 1024] + local[q];
        *rles = all.release();
    });
}

int kbo_relative_to_ref(const uint8_t *ref_seq, const uint8_t *aln, size_t len, uint8_t *out)
{
    return guarded([&] {
        KBO_REQUIRE(ref_seq && aln && out, KBO_E_BAD_ARG, "null argument");
        for (size_t i = 0; i < len; i++) { // format.rs:270-286
            const uint8_t a = aln[i];
            if (a == 'M' || a == 'R' || a == 'I') out[i] = ref_seq[i];
            else if (a == 'X' || a == 'D') out[i] = '-';
            else if (a != '-') out[i] = a;
            else out[i] = '-';
        }
    });
}

int kbo_find_batch(kbo_index_t *idx, const uint8_t *concat, const uint64_t *offsets, size_t n_seqs,
                   const kbo_find_opts *opts, kbo_rle **rles, uint64_t *rle_offsets)
{
    return guarded([&] {
        KBO_REQUIRE(idx && rles && rle_offsets, KBO_E_BAD_ARG, "null argument");
        RleSink<kbo_rle> sink;
        const double max_error_prob = prepare_find(sink, opts, rle_offsets);
        matches_batch_impl(idx, concat, offsets, n_seqs, max_error_prob, HostOut::runs(&sink));
        sink.take(rles);
    });
}

int kbo_find_batch_into(kbo_index_t *idx, const uint8_t *concat, const uint64_t *offsets, size_t n_seqs,
                        const kbo_find_opts *opts, kbo_rle *rles, size_t capacity, uint64_t *rle_offsets, size_t *n_runs)
{
    return guarded([&] {
        KBO_REQUIRE(idx && (rles || capacity == 0) && rle_offsets && n_runs, KBO_E_BAD_ARG, "null argument");
        RleSink<kbo_rle> sink;
        sink.records.use_buffer(rles, capacity); // (no record is written beyond it)
        const double max_error_prob = prepare_find(sink, opts, rle_offsets);
        matches_batch_impl(idx, concat, offsets, n_seqs, max_error_prob, HostOut::runs(&sink));
        *n_runs = sink.take(nullptr);
        KBO_REQUIRE(*n_runs <= capacity, KBO_E_NOMEM, "rles holds fewer records than the batch has runs (*n_runs says how many)");
    });
}

// ---- 2-bit packed batches (pack_kernels.hip has the layout) ------------------------------------------------------------

size_t kbo_packed_words(const uint64_t *offsets, size_t n_seqs)
{
    if (!offsets) return 0;
    size_t w = 0;
    for (size_t s = 0; s < n_seqs; s++) w += (size_t)((offsets[s + 1] - offsets[s] + 15) / 16);
    return w;
}

int kbo_pack_reads(const uint8_t *concat, const uint64_t *offsets, size_t n_seqs, uint32_t *words_out, uint64_t *exc_pos,
                   uint8_t *exc_byte, size_t exc_cap, size_t *n_exc)
{
    return guarded([&] {
        KBO_REQUIRE(concat && offsets && words_out && n_exc && (exc_cap == 0 || (exc_pos && exc_byte)), KBO_E_BAD_ARG, "null argument");
        std::vector<uint64_t> pw(n_seqs + 1, 0);
        for (size_t s = 0; s < n_seqs; s++) {
            KBO_REQUIRE(offsets[s + 1] >= offsets[s], KBO_E_BAD_ARG, "offsets not monotone");
            pw[s + 1] = pw[s] + (offsets[s + 1] - offsets[s] + 15) / 16;
        }
        const size_t piece = 4096, n_tasks = (n_seqs + piece - 1) / piece;
        std::vector<std::vector<std::pair<uint64_t, uint8_t>>> exc(n_tasks); // (in order inside a task, tasks in order)
        HostTeam::get().run(n_tasks, [&](size_t t) {
            for (size_t s = t * piece; s < std::min(n_seqs, (t + 1) * piece); s++) {
                const uint64_t b0 = offsets[s], len = offsets[s + 1] - b0;
                uint32_t *w = words_out + pw[s];
                for (uint64_t i0 = 0; i0 < len; i0 += 16) {
                    uint32_t v = 0;
                    const uint64_t nb = std::min<uint64_t>(16, len - i0);
                    for (uint64_t i = 0; i < nb; i++) {
                        const uint8_t ch = concat[b0 + i0 + i];
                        const uint32_t c = ch == 'A' ? 0u : ch == 'C' ? 1u : ch == 'G' ? 2u : ch == 'T' ? 3u : 4u;
                        if (c == 4u) exc[t].emplace_back(b0 + i0 + i, ch);
                        v |= (c & 3u) << (2 * i);
                    }
                    w[i0 / 16] = v;
                }
            }
        });
        size_t total = 0;
        for (const auto &e : exc) total += e.size();
        *n_exc = total;
        KBO_REQUIRE(total <= exc_cap, KBO_E_NOMEM, "more non-ACGT bases than the exception list holds (*n_exc says how many)");
        size_t x = 0;
        for (const auto &e : exc)
            for (const auto &pr : e) {
                exc_pos[x] = pr.first;
                exc_byte[x++] = pr.second;
            }
    });
}

int kbo_unpack_matches(const uint32_t *words, const uint64_t *offsets, size_t n_seqs, uint8_t *chars_out)
{
    return guarded([&] {
        KBO_REQUIRE(words && offsets && chars_out, KBO_E_BAD_ARG, "null argument");
        std::vector<uint64_t> pw(n_seqs + 1, 0);
        for (size_t s = 0; s < n_seqs; s++) pw[s + 1] = pw[s] + (offsets[s + 1] - offsets[s] + 15) / 16;
        const size_t piece = 4096;
        HostTeam::get().run((n_seqs + piece - 1) / piece, [&](size_t t) {
            for (size_t s = t * piece; s < std::min(n_seqs, (t + 1) * piece); s++) {
                const uint64_t b0 = offsets[s], len = offsets[s + 1] - b0;
                const uint32_t *w = words + pw[s];
                for (uint64_t i = 0; i < len; i++) chars_out[b0 + i] = (uint8_t)"M-XR"[(w[i / 16] >> (2 * (i % 16))) & 3u];
            }
        });
    });
}

int kbo_matches_batch_packed(kbo_index_t *idx, const uint32_t *words, const uint64_t *offsets, size_t n_seqs, const uint64_t *exc_pos,
                             const uint8_t *exc_byte, size_t n_exc, double max_error_prob, uint32_t *words_out)
{
    return guarded([&] {
        KBO_REQUIRE(idx && words && words_out, KBO_E_BAD_ARG, "null argument");
        const PackedBatch in{words, exc_pos, exc_byte, n_exc};
        matches_batch_packed_impl(idx, in, offsets, n_seqs, max_error_prob, HostOut::words(words_out, nullptr));
    });
}

int kbo_summary_batch_packed(kbo_index_t *idx, const uint32_t *words, const uint64_t *offsets, size_t n_seqs, const uint64_t *exc_pos,
                             const uint8_t *exc_byte, size_t n_exc, double max_error_prob, kbo_aln_summary *summary_out)
{
    return guarded([&] {
        KBO_REQUIRE(idx && words && summary_out, KBO_E_BAD_ARG, "null argument");
        const PackedBatch in{words, exc_pos, exc_byte, n_exc};
        matches_batch_packed_impl(idx, in, offsets, n_seqs, max_error_prob, HostOut::summary(summary_out));
    });
}

int kbo_find_batch_packed(kbo_index_t *idx, const uint32_t *words, const uint64_t *offsets, size_t n_seqs, const uint64_t *exc_pos,
                          const uint8_t *exc_byte, size_t n_exc, const kbo_find_opts *opts, kbo_rle32 **rles, uint64_t *rle_offsets)
{
    return guarded([&] {
        KBO_REQUIRE(idx && words && rles && rle_offsets, KBO_E_BAD_ARG, "null argument");
        static_assert(sizeof(kbo_rle32) == kRleWords * sizeof(uint32_t), "kbo_rle32 is the device's record");
        RleSink<kbo_rle32> sink;
        const double max_error_prob = prepare_find(sink, opts, rle_offsets);
        const PackedBatch in{words, exc_pos, exc_byte, n_exc};
        matches_batch_packed_impl(idx, in, offsets, n_seqs, max_error_prob, HostOut::runs32(&sink));
        sink.take(rles);
    });
}

int kbo_matches_batch_sparse(kbo_index_t *idx, const uint32_t *words, const uint64_t *offsets, size_t n_seqs, const uint64_t *exc_pos,
                             const uint8_t *exc_byte, size_t n_exc, double max_error_prob, kbo_aln_run **runs, uint64_t *n_runs)
{
    return guarded([&] {
        KBO_REQUIRE(idx && words && runs && n_runs, KBO_E_BAD_ARG, "null argument");
        static_assert(sizeof(kbo_aln_run) == 12, "kbo_aln_run is the device's record");
        RecordSink<kbo_aln_run> sink; // (records carry the sequence's index in the whole batch: nothing is rewritten)
        const PackedBatch in{words, exc_pos, exc_byte, n_exc};
        matches_batch_packed_impl(idx, in, offsets, n_seqs, max_error_prob, HostOut::sparse(&sink));
        *n_runs = sink.take(runs);
    });
}

int kbo_sparse_expand(const kbo_aln_run *runs, uint64_t n_runs, const uint64_t *offsets, size_t n_seqs, const uint8_t *ref_concat,
                      uint8_t *out)
{
    return guarded([&] {
        KBO_REQUIRE(offsets && out && (runs || n_runs == 0), KBO_E_BAD_ARG, "null argument");
        for (size_t s = 0; s < n_seqs; s++) KBO_REQUIRE(offsets[s + 1] >= offsets[s], KBO_E_BAD_ARG, "offsets not monotone");
        // every record inside its sequence and behind the one before it (same sequence: at or past its end)
        const size_t piece = 1u << 16;
        HostTeam &team = HostTeam::get();
        std::atomic<bool> bad{false};
        team.run((size_t)((n_runs + piece - 1) / piece), [&](size_t t) {
            const uint64_t a = t * piece, b = std::min<uint64_t>(n_runs, a + piece);
            for (uint64_t r = a; r < b && !bad.load(std::memory_order_relaxed); r++) {
                const kbo_aln_run &x = runs[r];
                const uint64_t len = x.len_code >> 2, code = x.len_code & 3u;
                bool ok = x.seq < n_seqs && len > 0 && code != 0 && x.start + len <= offsets[x.seq + 1] - offsets[x.seq];
                if (ok && r > 0) {
                    const kbo_aln_run &p = runs[r - 1];
                    ok = p.seq < x.seq || (p.seq == x.seq && (uint64_t)p.start + (p.len_code >> 2) <= x.start);
                }
                if (!ok) bad.store(true, std::memory_order_relaxed);
            }
        });
        KBO_REQUIRE(!bad.load(), KBO_E_BAD_ARG, "records out of (seq, start) order, overlapping, empty, of code 0 or outside their sequence");
        // sequences in pieces; a piece's records by binary search over seq (they are in order)
        const size_t spiece = 4096;
        team.run((n_seqs + spiece - 1) / spiece, [&](size_t t) {
            const size_t s0 = t * spiece, s1 = std::min(n_seqs, s0 + spiece);
            const uint64_t b0 = offsets[s0], b1 = offsets[s1];
            if (ref_concat) std::memcpy(out + b0, ref_concat + b0, b1 - b0); // format.rs:270-286: 'M' and 'R' take the read's base
            else std::memset(out + b0, 'M', b1 - b0);
            auto by_seq = [](const kbo_aln_run &x, size_t s) { return x.seq < s; };
            const kbo_aln_run *r = std::lower_bound(runs, runs + n_runs, s0, by_seq), *e = std::lower_bound(r, runs + n_runs, s1, by_seq);
            for (; r < e; r++) {
                const uint32_t code = r->len_code & 3u;
                if (ref_concat && code == 3u) continue;
                std::memset(out + offsets[r->seq] + r->start, ref_concat ? '-' : "M-XR"[code], r->len_code >> 2);
            }
        });
    });
}

int kbo_find(kbo_index_t *idx, const uint8_t *query, size_t len, const kbo_find_opts *opts, kbo_rle **out,
             size_t *n_out)
{
    return guarded([&] {
        KBO_REQUIRE(idx && query && out && n_out, KBO_E_BAD_ARG, "null argument");
        KBO_REQUIRE(len > 0, KBO_E_EMPTY_QUERY, "assert!(!query.is_empty()) (index.rs:248)");
        const uint64_t off[2] = {0, len};
        uint64_t ro[2];
        int rc = kbo_find_batch(idx, query, off, 1, opts, out, ro);
        if (rc) throw KboError(rc, last_error());
        *n_out = ro[1];
    });
}

void kbo_free(void *p) { std::free(p); }

int kbo_set_devices(const int *devices, int n)
{
    return guarded([&] {
        KBO_REQUIRE(n >= 0 && (devices || n == 0), KBO_E_BAD_ARG, "bad device list");
        int count = 0;
        if (n > 0) HIP_OK(hipGetDeviceCount(&count)); // (n == 0, back to the current device, needs no device at all)
        for (int i = 0; i < n; i++) KBO_REQUIRE(devices[i] >= 0 && devices[i] < count, KBO_E_BAD_ARG, "no such device");
        std::lock_guard<std::mutex> g(g_devices_mu);
        g_devices.assign(devices, devices + n);
    });
}

// ---- per-handle options
int kbo_index_opts_default(kbo_index_opts_t *opts)
{
    return guarded([&] {
        KBO_REQUIRE(opts, KBO_E_BAD_ARG, "null argument");
        std::memset(opts, 0, sizeof *opts);
        opts->struct_size = (uint32_t)sizeof *opts;
        opts->plan = opts->depth_table = opts->depth_table_anchors = KBO_OPT_INHERIT;
        opts->n_devices = -1;
    });
}

namespace {
void apply_opts(kbo_index *idx, const kbo_index_opts_t &o)
{
    idx->opts.plan = o.plan == KBO_OPT_INHERIT ? kOptInherit : (o.plan != 0 ? 1 : 0);
    idx->opts.depth_table = o.depth_table == KBO_OPT_INHERIT ? kOptInherit : (o.depth_table < 0 ? -1 : std::min(o.depth_table, 17));
    idx->opts.depth_table_anchors =
        o.depth_table_anchors == KBO_OPT_INHERIT ? kOptInherit : (o.depth_table_anchors < 0 ? -1 : (o.depth_table_anchors != 0 ? 1 : 0));
    idx->opts.slab_bytes = o.slab_bytes ? std::max<size_t>(1u << 16, std::min<size_t>(o.slab_bytes, 0xF0000000ull)) : 0;
    {
        std::lock_guard<std::mutex> g(idx->mu);
        idx->opts.n_devices = o.n_devices;
        idx->opts.devices.assign(o.devices, o.devices + std::max(0, o.n_devices));
    }
    if (o.plan != KBO_OPT_INHERIT && o.plan != 0) plan_reset_holdoff();
    for (auto &sh : idx->shards) apply_opts(sh.get(), o); // (a sharded index: its shards are what gets copied and walked)
}
} // namespace

int kbo_index_set_opts(kbo_index_t *idx, const kbo_index_opts_t *opts)
{
    return guarded([&] {
        KBO_REQUIRE(idx && opts, KBO_E_BAD_ARG, "null argument");
        KBO_REQUIRE(opts->struct_size == sizeof *opts, KBO_E_BAD_ARG, "kbo_index_opts_t: struct_size is not this library's (fill it with kbo_index_opts_default)");
        KBO_REQUIRE(opts->n_devices >= -1 && opts->n_devices <= KBO_OPT_MAX_DEVICES, KBO_E_BAD_ARG, "n_devices: -1 .. KBO_OPT_MAX_DEVICES");
        if (opts->n_devices > 0) {
            int count = 0;
            HIP_OK(hipGetDeviceCount(&count));
            for (int i = 0; i < opts->n_devices; i++) KBO_REQUIRE(opts->devices[i] >= 0 && opts->devices[i] < count, KBO_E_BAD_ARG, "no such device");
        }
        apply_opts(idx, *opts);
    });
}

int kbo_index_get_opts(const kbo_index_t *idx_c, kbo_index_opts_t *opts)
{
    return guarded([&] {
        KBO_REQUIRE(idx_c && opts, KBO_E_BAD_ARG, "null argument");
        kbo_index *idx = const_cast<kbo_index *>(idx_c);
        std::memset(opts, 0, sizeof *opts);
        opts->struct_size = (uint32_t)sizeof *opts;
        auto out = [](int v) { return v == kOptInherit ? KBO_OPT_INHERIT : v; };
        opts->plan = out(idx->opts.plan.load());
        opts->depth_table = out(idx->opts.depth_table.load());
        opts->depth_table_anchors = out(idx->opts.depth_table_anchors.load());
        opts->slab_bytes = idx->opts.slab_bytes.load();
        std::lock_guard<std::mutex> g(idx->mu);
        opts->n_devices = idx->opts.n_devices;
        for (int i = 0; i < idx->opts.n_devices; i++) opts->devices[i] = idx->opts.devices[(size_t)i];
    });
}

int kbo_set_host_threads(int n)
{
    HostTeam::get().set_threads(n < 1 ? 1u : (unsigned)n);
    HostTeam::out().set_threads(n < 1 ? 1u : (unsigned)n);
    return KBO_OK;
}

int kbo_release_scratch(void)
{
    return guarded([&] {
        release_host_scratch();
    });
}

int kbo_index_recovery_lines(const kbo_index_t *idx, uint8_t *lines, size_t *n_bytes)
{
    return guarded([&] {
        KBO_REQUIRE(idx && n_bytes, KBO_E_BAD_ARG, "null argument");
        require_unsharded(idx, "kbo_index_recovery_lines");
        const size_t need = (idx->host.n_sets / kbo::kFatRows + 3) * 128;
        if (lines) {
            KBO_REQUIRE(*n_bytes >= need, KBO_E_BAD_ARG, "buffer smaller than the lines");
            std::vector<uint8_t> v;
            kbo::make_recovery_lines(idx->host, v);
            std::memcpy(lines, v.data(), v.size());
        }
        *n_bytes = need;
    });
}

int kbo_index_path_cover(const kbo_index_t *idx, uint8_t *text, uint32_t *pos, uint32_t *node_at)
{
    return guarded([&] {
        KBO_REQUIRE(idx && text && pos && node_at, KBO_E_BAD_ARG, "null argument");
        require_unsharded(idx, "kbo_index_path_cover");
        kbo_index_t *ix = const_cast<kbo_index_t *>(idx); // (fills the handle's cache of its cover, under its mutex)
        std::lock_guard<std::mutex> g(ix->mu);
        if (!ix->cover) {
            ix->cover.reset(new kbo::PathCover());
            kbo::make_path_cover(ix->host, *ix->cover);
        }
        const kbo::PathCover &pc = *ix->cover;
        std::memcpy(text, pc.text.data() + kbo::PathCover::kPad, idx->host.n_sets);
        std::memcpy(pos, pc.pos.data(), idx->host.n_sets * 4);
        std::memcpy(node_at, pc.node_at.data(), idx->host.n_sets * 4);
    });
}

int kbo_index_shards(const kbo_index_t *idx) { return idx ? (idx->sharded() ? (int)idx->shards.size() : 1) : 0; }

int kbo_index_device_layout(kbo_index_t *idx, int device, kbo_device_layout *out)
{
    return guarded([&] {
        KBO_REQUIRE(idx && out, KBO_E_BAD_ARG, "null argument");
        require_unsharded(idx, "kbo_index_device_layout");
        std::lock_guard<std::mutex> g(idx->mu);
        const DevCopy &dc = copy_on(idx, device);
        *out = kbo_device_layout{};
        out->rank_bytes = dc.setup.rank_bytes;
        out->entry_bytes = dc.setup.entry_bytes;
        out->pair_bytes = dc.setup.pair_bytes;
        out->cover_bytes = dc.setup.cover_bytes;
        out->lines_bytes = dc.setup.lines_bytes;
        out->seed_bytes = dc.setup.seed_bytes;
        out->dtab_bytes = dc.setup.dtab_bytes;
        out->anchor_bytes = dc.setup.anchor_bytes;
        out->entries_64bit = dc.big ? 1u : 0u;
        out->seed_depth = dc.seed_d;
        out->dtab_order = dc.dtab_order;
        out->dtab_grouped = dc.dtab_grouped ? 1u : 0u;
        out->layout_seconds = dc.setup.layout_s;
        out->upload_seconds = dc.setup.upload_s;
        out->cover_seconds = dc.setup.cover_s;
        out->lines_seconds = dc.setup.lines_s;
        out->seed_seconds = dc.setup.seed_s;
        out->dtab_seconds = dc.setup.dtab_s;
    });
}

uint64_t kbo_index_device_plan_bytes(const kbo_index_t *idx)
{
    if (!idx) return 0;
    uint64_t b = 0;
    for (kbo_index *sh : shards_of(const_cast<kbo_index *>(idx))) b += sh->plan_bytes;
    return b;
}

int kbo_set_slab_bytes(size_t bytes)
{
    g_slab_bytes = std::max<size_t>(1u << 16, std::min<size_t>(bytes, 0xF0000000ull));
    return KBO_OK;
}

} // extern "C"

// ---- both strands (revcomp_kernels.hip; host_batch.cpp doubles every slab on the device) ---------------------------------------

namespace {
inline uint8_t complement_byte(uint8_t c)
{
    switch (c) {
    case 'A': return 'T';
    case 'T': return 'A';
    case 'C': return 'G';
    case 'G': return 'C';
    case 'a': return 't';
    case 't': return 'a';
    case 'c': return 'g';
    case 'g': return 'c';
    default: return c;
    }
}
bool ranges_overlap(const void *a, const void *b, uint64_t n)
{
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return x < y + n && y < x + n;
}
void require_strands(int strands) { KBO_REQUIRE(strands >= 1 && strands <= 3, KBO_E_BAD_ARG, "strands: KBO_STRAND_FWD, KBO_STRAND_REV or both"); }
} // namespace

int kbo_revcomp_batch(const uint8_t *concat, const uint64_t *offsets, size_t n_seqs, uint8_t *out)
{
    return guarded([&] {
        KBO_REQUIRE(concat && offsets && out, KBO_E_BAD_ARG, "null argument");
        for (size_t s = 0; s < n_seqs; s++) KBO_REQUIRE(offsets[s + 1] >= offsets[s], KBO_E_BAD_ARG, "offsets not monotone");
        KBO_REQUIRE(offsets[0] == 0, KBO_E_BAD_ARG, "offsets[0] must be 0");
        const uint64_t total = offsets[n_seqs];
        KBO_REQUIRE(!ranges_overlap(concat, out, total), KBO_E_BAD_ARG, "out overlaps concat");
        // pieces of the OUTPUT, so that a few long sequences keep every thread as busy as many short ones
        const uint64_t piece = 1u << 18;
        HostTeam::get().run((size_t)((total + piece - 1) / piece), [&](size_t t) {
            const uint64_t a = t * piece, b = std::min(total, a + piece);
            size_t s = std::upper_bound(offsets, offsets + n_seqs + 1, a) - offsets - 1; // the sequence that holds base a
            for (uint64_t p = a; p < b;) {
                while (p >= offsets[s + 1]) s++;
                const uint64_t e = std::min(b, offsets[s + 1]), mirror = offsets[s] + offsets[s + 1] - 1;
                for (; p < e; p++) out[p] = complement_byte(concat[mirror - p]);
            }
        });
    });
}

int kbo_matches_batch_strands(kbo_index_t *idx, const uint8_t *concat, const uint64_t *offsets, size_t n_seqs, double max_error_prob,
                              int format, int strands, uint8_t *out_fwd, uint8_t *out_rev)
{
    return guarded([&] {
        require_strands(strands);
        matches_batch_impl(idx, concat, offsets, n_seqs, max_error_prob, HostOut::chars(out_fwd, out_rev, format != 0), strands);
    });
}

int kbo_find_batch_strands(kbo_index_t *idx, const uint8_t *concat, const uint64_t *offsets, size_t n_seqs, const kbo_find_opts *opts,
                           int strands, kbo_rle **rles, uint64_t *rle_offsets)
{
    return guarded([&] {
        require_strands(strands);
        KBO_REQUIRE(idx && rles && rle_offsets, KBO_E_BAD_ARG, "null argument");
        RleSink<kbo_rle> sink;
        const double max_error_prob = prepare_find(sink, opts, rle_offsets);
        matches_batch_impl(idx, concat, offsets, n_seqs, max_error_prob, HostOut::runs(&sink), strands);
        sink.take(rles);
    });
}

int kbo_matches_batch_packed_strands(kbo_index_t *idx, const uint32_t *words, const uint64_t *offsets, size_t n_seqs, const uint64_t *exc_pos,
                                     const uint8_t *exc_byte, size_t n_exc, double max_error_prob, int strands, uint32_t *words_fwd,
                                     uint32_t *words_rev)
{
    return guarded([&] {
        require_strands(strands);
        KBO_REQUIRE(idx && words, KBO_E_BAD_ARG, "null argument");
        const PackedBatch in{words, exc_pos, exc_byte, n_exc};
        matches_batch_packed_impl(idx, in, offsets, n_seqs, max_error_prob, HostOut::words(words_fwd, words_rev), strands);
    });
}

int kbo_find_batch_packed_strands(kbo_index_t *idx, const uint32_t *words, const uint64_t *offsets, size_t n_seqs, const uint64_t *exc_pos,
                                  const uint8_t *exc_byte, size_t n_exc, const kbo_find_opts *opts, int strands, kbo_rle32 **rles,
                                  uint64_t *rle_offsets)
{
    return guarded([&] {
        require_strands(strands);
        KBO_REQUIRE(idx && words && rles && rle_offsets, KBO_E_BAD_ARG, "null argument");
        RleSink<kbo_rle32> sink;
        const double max_error_prob = prepare_find(sink, opts, rle_offsets);
        const PackedBatch in{words, exc_pos, exc_byte, n_exc};
        matches_batch_packed_impl(idx, in, offsets, n_seqs, max_error_prob, HostOut::runs32(&sink), strands);
        sink.take(rles);
    });
}
