// build_device.cpp — kbo_index_build_device: kbo::build (reference lib.rs:501-506, index.rs:56-99) by the device.  The passes of
// build_kernels.hip follow the five steps of sbwt_build.cpp's build_impl over the same colex keys, so the index is the host
// builder's bit for bit; this file uploads the sequences, runs the passes, checks the device's counters as the host builder checks
// its own, downloads the rows and LCS into the handle's host copy, and makes the handle's device copy from the rows and LCS the device
// built (device_view: the one layout path kbo_index_to_device takes too).
#include "capi_internal.hpp"

#include <chrono>
#include <cstring>

using namespace kbo_host;

namespace {

// where the last build of the calling thread spent its time (kbo_index_build_device_phases)
constexpr int kPhases = 9;
thread_local double t_phase[kPhases];

constexpr size_t kScanValuesPerBlock = 1024; // (values per block of launch_scan: device_util.hpp kScanBlock)

uint32_t key_words(uint32_t k) { return k <= 32 ? 1u : k <= 64 ? 2u : k <= 128 ? 4u : 8u; }

// Peak device bytes of a build over `bases` bases, with E = bases x strands k-mers at most, W key words each.  The peak is the merge
// (step 3): the sorted k-mers (8 W E), the dummy rows ((8 W + 1) E: an ACGT run of L >= k bases adds at most k - 1 <= L of them) and
// the rows they merge into ((8 W + 1) 2 E), plus the merge's 4-byte search results: 32 W + 7 bytes per k-mer, 32 W + 8 with the
// sort's histograms and the flags.  The sequences (1 byte per base) are freed once the k-mers are out.
uint64_t peak_bytes(uint64_t bases, size_t n_seqs, uint32_t k, bool add_revcomp)
{
    const uint64_t E = bases * (add_revcomp ? 2u : 1u);
    return E * (32u * key_words(k) + 8u) + bases + n_seqs + (64ull << 20);
}

struct Keys { // W word arrays of `stride` words (+ one real byte per key)
    DevBuf w, r;
    uint64_t stride = 0;
    void alloc(uint64_t n, uint32_t W, bool real)
    {
        stride = std::max<uint64_t>(n, 1);
        w.alloc(stride * W * 8 + 64);
        if (real) r.alloc(stride + 64);
    }
    void release()
    {
        w.release();
        r.release();
    }
    uint64_t *k() const { return w.as<uint64_t>(); }
    uint8_t *re() const { return r.as<uint8_t>(); }
};
void swap_buf(DevBuf &a, DevBuf &b)
{
    std::swap(a.p, b.p);
    std::swap(a.cap, b.cap);
    std::swap(a.dev, b.dev);
}
void swap_keys(Keys &a, Keys &b)
{
    swap_buf(a.w, b.w);
    swap_buf(a.r, b.r);
    std::swap(a.stride, b.stride);
}

struct Events {
    hipEvent_t e[kPhases + 1] = {};
    Events()
    {
        for (auto &x : e) HIP_OK(hipEventCreate(&x));
    }
    ~Events()
    {
        for (auto &x : e)
            if (x) (void)hipEventDestroy(x);
    }
};

// the sequences back to back, each followed by one 0 byte (not ACGT: no k-mer spans two sequences), through two pinned chunks
void upload(const uint8_t *const *seqs, const size_t *lens, size_t n_seqs, uint64_t n_bytes, uint8_t *d_seq, hipStream_t s)
{
    const size_t chunk = (size_t)std::min<uint64_t>(n_bytes, 64ull << 20);
    PinBuf pin[2];
    pin[0].ensure(chunk);
    pin[1].ensure(chunk);
    Events ev;
    bool pending[2] = {false, false};
    int cur = 0;
    size_t fill = 0;
    uint64_t dst = 0;
    auto flush = [&] {
        if (!fill) return;
        HIP_OK(hipMemcpyAsync(d_seq + dst, pin[cur].p, fill, hipMemcpyHostToDevice, s));
        HIP_OK(hipEventRecord(ev.e[cur], s));
        pending[cur] = true;
        dst += fill;
        fill = 0;
        cur ^= 1;
        if (pending[cur]) HIP_OK(hipEventSynchronize(ev.e[cur]));
        pending[cur] = false;
    };
    for (size_t q = 0; q < n_seqs; q++) {
        for (size_t off = 0; off < lens[q];) {
            const size_t t = std::min(lens[q] - off, chunk - fill);
            std::memcpy(pin[cur].as<uint8_t>() + fill, seqs[q] + off, t);
            fill += t;
            off += t;
            if (fill == chunk) flush();
        }
        pin[cur].as<uint8_t>()[fill++] = 0;
        if (fill == chunk) flush();
    }
    flush();
    HIP_OK(hipStreamSynchronize(s));
}

uint64_t read_u64(const unsigned long long *d, hipStream_t s)
{
    uint64_t v = 0;
    HIP_OK(hipMemcpyAsync(&v, d, 8, hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    return v;
}

// LSD radix sort of keys [0, n) of `a` by (key over its 2k significant bits[, real]); `b` (same stride) is the other buffer.  The
// result is in `a`.
void sort_keys(Keys &a, Keys &b, uint64_t n, uint32_t W, uint32_t k, bool real, hipStream_t s)
{
    const size_t tiles = kbo::build_tiles(n);
    if (!tiles) return;
    DevBuf hist(256 * tiles * 4 + 64), sums((256 * tiles / kScanValuesPerBlock + 2) * 4 + 64);
    std::vector<kbo::RadixPass> passes;
    if (real) passes.push_back(kbo::RadixPass{0, 8, 1});
    for (int hi = 2 * (int)k; hi > 0; hi -= 8) {
        const int lo = std::max(0, hi - 8);
        passes.push_back(kbo::RadixPass{(uint32_t)lo, (uint32_t)(hi - lo), 0});
    }
    for (const kbo::RadixPass &ps : passes) {
        HIP_OK(kbo::launch_build_radix_pass(a.k(), b.k(), W, a.stride, real ? a.re() : nullptr, real ? b.re() : nullptr, n, ps, hist.as<uint32_t>(),
                                            sums.as<uint32_t>(), s));
        swap_keys(a, b);
    }
}

// the flagged keys of `in` [0, n) into `out`, in order; returns their number
uint64_t compact(const Keys &in, Keys &out, uint32_t W, bool real, const uint8_t *d_flags, uint64_t n, unsigned long long *d_total, hipStream_t s)
{
    const size_t tiles = kbo::build_tiles(n);
    if (!tiles) return 0;
    DevBuf counts(tiles * 4 + 64), sums((tiles / kScanValuesPerBlock + 2) * 4 + 64);
    HIP_OK(hipMemsetAsync(d_total, 0, 8, s));
    HIP_OK(kbo::launch_build_compact(in.k(), in.stride, out.k(), out.stride, W, real ? in.re() : nullptr, real ? out.re() : nullptr, d_flags, n,
                                     counts.as<uint32_t>(), sums.as<uint32_t>(), d_total, s));
    return read_u64(d_total, s);
}

// steps 1-5; leaves the rows (4 x nw words) and LCS (n bytes) in d_rows / d_lcs and the rest of the index in h
void build_on_device(const uint8_t *const *seqs, const size_t *lens, size_t n_seqs, uint64_t bases, uint32_t k, bool add_revcomp,
                     kbo::HostIndex &h, DevBuf &d_rows, DevBuf &d_lcs, Events &ev, hipStream_t s)
{
    const uint32_t W = key_words(k);
    const uint64_t E = bases * (add_revcomp ? 2u : 1u), n_bytes = bases + n_seqs;
    DevBuf ctr(16 * 8);
    unsigned long long *d_ctr = ctr.as<unsigned long long>();
    HIP_OK(hipMemsetAsync(d_ctr, 0, 16 * 8, s));
    HIP_OK(hipEventRecord(ev.e[0], s));
    // ---- 1. the k-mers of every ACGT run of >= k bases
    Keys a, b;
    uint64_t R = 0;
    {
        DevBuf d_seq(n_bytes + 64);
        upload(seqs, lens, n_seqs, n_bytes, d_seq.as<uint8_t>(), s);
        HIP_OK(hipEventRecord(ev.e[1], s));
        a.alloc(E, W, false);
        HIP_OK(kbo::launch_build_extract(W, d_seq.as<uint8_t>(), n_bytes, k, true, add_revcomp, a.k(), a.stride, d_ctr, s));
        R = read_u64(d_ctr, s);
        if (R > E) throw KboError(KBO_E_HIP, "device build: more k-mers than bases");
    }
    HIP_OK(hipEventRecord(ev.e[2], s));
    // ---- sort + dedup
    b.alloc(E, W, false);
    sort_keys(a, b, R, W, k, false, s);
    HIP_OK(hipEventRecord(ev.e[3], s));
    DevBuf flags(std::max<uint64_t>(R, 1) + 64);
    HIP_OK(kbo::launch_build_flag_distinct(W, a.k(), a.stride, nullptr, R, flags.as<uint8_t>(), s));
    const uint64_t N = compact(a, b, W, false, flags.as<uint8_t>(), R, d_ctr + 1, s);
    swap_keys(a, b); // (the k-mers in a, b free)
    HIP_OK(hipEventRecord(ev.e[4], s));
    // ---- 2. k-mers without a predecessor -> their $-padded prefixes + the root, sorted by (key, real), deduplicated
    HIP_OK(kbo::launch_build_flag_orphan(W, a.k(), a.stride, N, k, flags.as<uint8_t>(), s));
    const uint64_t n_orph = compact(a, b, W, false, flags.as<uint8_t>(), N, d_ctr + 2, s);
    flags.release();
    const uint64_t D_raw = 1 + n_orph * (k - 1);
    Keys da, db;
    da.alloc(D_raw, W, true);
    HIP_OK(kbo::launch_build_dummies(W, b.k(), b.stride, n_orph, k, da.k(), da.stride, da.re(), s));
    HIP_OK(hipStreamSynchronize(s));
    b.release();
    db.alloc(D_raw, W, true);
    sort_keys(da, db, D_raw, W, k, true, s);
    uint64_t D = 0;
    {
        DevBuf dflags(D_raw + 64);
        HIP_OK(kbo::launch_build_flag_distinct(W, da.k(), da.stride, da.re(), D_raw, dflags.as<uint8_t>(), s));
        D = compact(da, db, W, true, dflags.as<uint8_t>(), D_raw, d_ctr + 3, s);
    }
    swap_keys(da, db);
    db.release();
    HIP_OK(hipEventRecord(ev.e[5], s));
    // ---- 3. merge into colex row order
    const uint64_t n = N + D;
    if (n >= 0xFFFFFFF0ull) throw std::runtime_error("n_sets >= 2^32: 64-bit positions not built yet");
    Keys rm;
    rm.alloc(n, W, true);
    {
        DevBuf lb(D * 4 + 64);
        HIP_OK(kbo::launch_build_merge(W, a.k(), a.stride, N, k, da.k(), da.stride, da.re(), D, lb.as<uint32_t>(), rm.k(), rm.stride, rm.re(), s));
        HIP_OK(hipStreamSynchronize(s));
    }
    a.release();
    da.release();
    HIP_OK(hipEventRecord(ev.e[6], s));
    // ---- 4. edge bits, C[] and its checks; 5. LCS
    const uint64_t nw = (n + 63) / 64;
    d_rows.alloc(4 * nw * 8 + 64);
    d_lcs.alloc(n + 64);
    HIP_OK(hipMemsetAsync(d_rows.p, 0, 4 * nw * 8 + 64, s));
    HIP_OK(hipMemsetAsync(d_ctr + 4, 0, 9 * 8, s));
    HIP_OK(kbo::launch_build_edges_lcs(W, rm.k(), rm.stride, rm.re(), n, k, d_rows.as<uint64_t>(), nw, d_lcs.as<uint8_t>(), d_ctr + 4, s));
    uint64_t c9[9];
    HIP_OK(hipMemcpyAsync(c9, d_ctr + 4, sizeof c9, hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    rm.release();
    HIP_OK(hipEventRecord(ev.e[7], s));
    if (c9[0]) throw std::runtime_error("sbwt build: row without incoming edge");
    uint64_t first[5], acc = 1;
    first[0] = 1;
    for (int c = 1; c <= 4; c++) first[c] = first[c - 1] + c9[c];
    first[4] = n;
    for (int c = 0; c < 4; c++) {
        h.C[c] = acc;
        acc += c9[5 + c];
    }
    if (acc != n) throw std::runtime_error("sbwt build: edge count != n_sets - 1");
    for (int c = 0; c < 4; c++)
        if (first[c] != h.C[c] && first[c] < first[c + 1]) throw std::runtime_error("sbwt build: C array inconsistent with row order");
    // ---- the host copy
    h.k = k;
    h.n_sets = n;
    h.n_kmers = N;
    for (int c = 0; c < 4; c++) {
        h.rows[c].resize(nw);
        HIP_OK(hipMemcpyAsync(h.rows[c].data(), d_rows.as<uint64_t>() + c * nw, nw * 8, hipMemcpyDeviceToHost, s));
    }
    h.lcs.resize(n);
    HIP_OK(hipMemcpyAsync(h.lcs.data(), d_lcs.p, n, hipMemcpyDeviceToHost, s));
    HIP_OK(hipEventRecord(ev.e[8], s));
    HIP_OK(hipStreamSynchronize(s));
}

} // namespace

extern "C" int kbo_index_build_device(const uint8_t *const *seqs, const size_t *lens, size_t n_seqs, const kbo_build_opts *opts, int device,
                                      kbo_index_t **out)
{
    return guarded([&] {
        // (argument checks as kbo_index_build's, before any HIP call)
        KBO_REQUIRE(out, KBO_E_BAD_ARG, "null out");
        *out = nullptr;
        KBO_REQUIRE(seqs && lens && n_seqs > 0, KBO_E_BAD_ARG, "assert!(!slices.is_empty()) (index.rs:60)");
        kbo_build_opts o;
        if (opts) o = *opts; else kbo_build_opts_default(&o);
        if (o.k == 0 || o.k > 255) throw std::runtime_error("k must be in 1..255");
        const bool rc = o.add_revcomp != 0;
        uint64_t bases = 0;
        for (size_t q = 0; q < n_seqs; q++) {
            KBO_REQUIRE(seqs[q] || lens[q] == 0, KBO_E_BAD_ARG, "null sequence");
            bases += lens[q];
        }
        KBO_REQUIRE(shards_wanted(bases, rc) <= 1, KBO_E_UNSUPPORTED,
                    "kbo_index_build_device: this input would be built as a sharded index; sharded builds run on the host (kbo_index_build)");
        KBO_REQUIRE(bases * (rc ? 2u : 1u) < 0xFFFFFFF0ull, KBO_E_UNSUPPORTED,
                    "kbo_index_build_device: 2^32 or more k-mers; build it with kbo_index_build");
        for (double &t : t_phase) t = 0;
        DeviceScope scope(device);
        const int dev = device < 0 ? scope.prev : device;
        size_t free_b = 0, total_b = 0;
        HIP_OK(hipMemGetInfo(&free_b, &total_b));
        const uint64_t need = peak_bytes(bases, n_seqs, o.k, rc);
        KBO_REQUIRE(need <= free_b, KBO_E_NOMEM,
                    "kbo_index_build_device: needs " + std::to_string(need >> 20) + " MiB of device memory, " + std::to_string(free_b >> 20) +
                        " MiB are free");
        std::unique_ptr<kbo_index> idx(new kbo_index());
        DevBuf d_rows, d_lcs;
        hipStream_t s = nullptr;
        HIP_OK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
        try {
            Events ev;
            build_on_device(seqs, lens, n_seqs, bases, o.k, rc, idx->host, d_rows, d_lcs, ev, s);
            for (int i = 0; i < 8; i++) {
                float ms = 0;
                HIP_OK(hipEventElapsedTime(&ms, ev.e[i], ev.e[i + 1]));
                t_phase[i] = ms * 1e-3;
            }
        } catch (...) {
            (void)hipStreamSynchronize(s);
            (void)hipStreamDestroy(s);
            throw;
        }
        HIP_OK(hipStreamDestroy(s));
        // the device copy, from the rows and LCS the device built (build scratch is gone by now)
        const auto t0 = std::chrono::steady_clock::now();
        const DeviceRowsLcs built{d_rows.as<uint64_t>(), d_lcs.as<uint8_t>()};
        (void)device_view(idx.get(), dev, nullptr, 0, true, &built);
        t_phase[8] = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        *out = idx.release();
    });
}

extern "C" int kbo_index_build_device_phases(double out[9])
{
    if (!out) return KBO_E_BAD_ARG;
    for (int i = 0; i < kPhases; i++) out[i] = t_phase[i];
    return KBO_OK;
}
