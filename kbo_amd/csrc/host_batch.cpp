// host_batch.cpp — host batches: work decomposition, slabs, pinned staging with helper threads, the
// three-stage (upload / kernels / download) pipeline with pooled per-device scratch and one output
// stage per mode.  No compute here: kernels live in the *_kernels.hip files.
#include "batch_route.hpp"

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <memory>

namespace kbo_host {

std::vector<int> g_devices;
std::mutex g_devices_mu;
std::vector<int> devices_snapshot()
{
    std::lock_guard<std::mutex> g(g_devices_mu);
    return g_devices;
}
std::vector<int> devices_for(kbo_index *idx)
{
    if (idx) {
        std::lock_guard<std::mutex> g(idx->mu);
        if (idx->opts.n_devices >= 0) return idx->opts.devices;
    }
    return devices_snapshot();
}

// ---- work decomposition ------------------------------------------------------------------
// Reads become one item each.  Longer sequences are cut into chunks that restart the walk
// k-1 bases upstream from the empty state (MS depends only on the last k bases).
uint32_t max_len(const uint64_t *offsets, size_t n_seqs)
{
    uint64_t m = 0;
    for (size_t s = 0; s < n_seqs; s++) m = std::max(m, offsets[s + 1] - offsets[s]);
    return (uint32_t)std::min<uint64_t>(m, 0xFFFFFFFFu);
}

// emitted bases per chunk: aim for about 130 k items when the input allows it, 256..4096 bases
// (every chunk after the first re-walks k-1 warm-up bases); a batch that already has enough
// sequences to fill the device is only cut where a sequence is very long
uint64_t walk_chunk(uint64_t total, size_t n_seqs, uint32_t k)
{
    // (measured on 100 Mbp of 10 kbp reads, call mode: 192 / 256 / 384 / 512 / 768 / 1024 / 1536 / 2048 bases per chunk ->
    // 39.9 / 41.9 / 42.9 / 43.6 / 46.0 / 42.5 / 32.1 / 26.0 Gbp/s: about 130 k items, a quarter of the lanes, is the best
    // trade between the k warm-up bases every chunk re-walks and the number of chains in flight)
    // Not above 768: the plan-guided walk keeps at most 29 mismatches of an item (13 for reads), which chunks of 800 bases
    // at 1 % substitutions rarely exceed and chunks of 4000 always do (500 Mbp of 10 kbp reads, call mode: 46.5 Gbp/s with
    // chunks of 3814 bases, every one of them walked as an item without a plan); 30 warm-up bases per 768 cost the plain
    // walk 4 %.
    (void)n_seqs;
    // (a multiple of 64: tools/dbg_call_chunk.py - with chunks of 457 bases, what a slab of 60 Mbp used to get, the call mode of the
    // plan-guided walk gave different sites from run to run; 448, 460, 464, 300, 1000 are exact.  Slabs were 32 MiB until round 4,
    // whose chunks are 256 bases, so nothing ever ran that way; chunk boundaries now stay 4-byte aligned relative to the sequence)
    uint64_t chunk = std::min<uint64_t>(768, std::max<uint64_t>(256, (total >> 17) & ~63ull));
    static const int env_chunk = std::getenv("KBO_WALK_CHUNK") ? std::atoi(std::getenv("KBO_WALK_CHUNK")) : 0; // experiments
    if (env_chunk > 0) chunk = ((uint64_t)env_chunk + 3u) & ~3ull;
    return std::max<uint64_t>(chunk, 4ull * k);
}

// call = true: items for the call mode of the walk (k warm-up bases so that the MS value in front of the first owned
// base is exact up to min(., k); up to k more bases behind the chunk, walked only to finish the search to the right)
void make_items_host(const uint64_t *offsets, size_t n_seqs, uint32_t k, std::vector<kbo::WalkItem> &items, bool call = false)
{
    const uint64_t total = offsets[n_seqs] - offsets[0];
    const uint64_t chunk = walk_chunk(total, n_seqs, k);
    KBO_REQUIRE(!call || (chunk & 3u) == 0, KBO_E_BAD_ARG, "call mode: chunks of a multiple of four bases (kernels.hpp launch_make_chunk_items)");
    items.clear();
    for (size_t s = 0; s < n_seqs; s++) {
        const uint64_t b = offsets[s], e = offsets[s + 1];
        for (uint64_t c0 = b; c0 < e; c0 += chunk) {
            const uint64_t c1 = std::min(e, c0 + chunk);
            const uint64_t warm = std::min<uint64_t>(c0 - b, call ? k : (k > 0 ? k - 1 : 0));
            const uint64_t tail = call ? std::min<uint64_t>(e - c1, k) : 0;
            kbo::WalkItem it;
            it.start = c0 - warm;
            it.len = (uint32_t)(c1 - c0 + warm + tail);
            it.warm = (uint32_t)warm | ((uint32_t)tail << 16);
            items.push_back(it);
        }
    }
}

void check_batch(const void *concat, const uint64_t *offsets, size_t n_seqs)
{
    KBO_REQUIRE(concat && offsets, KBO_E_BAD_ARG, "null concat/offsets");
    KBO_REQUIRE(n_seqs > 0, KBO_E_EMPTY_QUERY, "no sequences");
    KBO_REQUIRE(n_seqs < 0xFFFFFFFFull, KBO_E_UNSUPPORTED, "more than 2^32-1 sequences per call");
    for (size_t s = 0; s < n_seqs; s++) {
        KBO_REQUIRE(offsets[s + 1] >= offsets[s], KBO_E_BAD_ARG, "offsets not monotone");
        KBO_REQUIRE(offsets[s + 1] > offsets[s], KBO_E_EMPTY_QUERY,
                    "empty query (index.rs:248 assert!(!query.is_empty()))");
        KBO_REQUIRE(offsets[s + 1] - offsets[s] < 0xFFFFFFFFull, KBO_E_UNSUPPORTED,
                    "sequence longer than 2^32-1");
    }
    KBO_REQUIRE(offsets[0] == 0, KBO_E_BAD_ARG, "offsets[0] must be 0");
}


// The upload of a host batch (on `copy_stream` where given, `stream` waiting for it) and what is made of it on the device: the
// other strand, the offsets, the work items, a packed batch's scanned words.  Returns the queries, offsets and items of the batch's
// view (batch_route.hpp); the bytes of a packed batch are unpacked only when a route needs them
static BatchView stage_walk_host(kbo_index *idx, const uint8_t *concat, const uint64_t *offsets, size_t n_seqs, BatchOnDevice &B,
                                 std::vector<kbo::WalkItem> &items_keep, hipStream_t stream, const WalkHostAsk &ask)
{
    const PackedIn *packed = ask.packed;
    const HostStage *hs = ask.stage;
    // strands (HostStage): what is uploaded is the first n_up sequences' up_total bases; `rev` = a reverse complement is made of it
    const int strands = hs ? hs->strands : 1;
    const bool both = strands == 3, rev = (strands & 2) != 0;
    const size_t n_up = both ? n_seqs / 2 : n_seqs;
    const uint64_t up_total = both ? offsets[n_up] : offsets[n_seqs];
    BatchView v;
    v.n_seqs = (uint32_t)n_seqs;
    v.total = B.total = offsets[n_seqs];
    // reads (nothing to chunk): the item list is derived from the offsets on the device;
    // otherwise it is built here (chunks with k-1 warm-up bases) and uploaded
    v.longest = ask.longest ? ask.longest : max_len(offsets, n_seqs);
    const uint64_t chunk = walk_chunk(v.total, n_seqs, idx->host.k);
    if (v.longest > chunk) v.chunk = (uint32_t)chunk;
    if (v.chunk) make_items_host(offsets, n_seqs, idx->host.k, items_keep, ask.call != nullptr);
    const size_t n_items = v.chunk ? items_keep.size() : n_seqs;
    KBO_REQUIRE(n_items < (1ull << 28), KBO_E_UNSUPPORTED, "more than 2^28 work items per launch");
    KBO_REQUIRE(v.total < 0xFFFFFF00ull, KBO_E_UNSUPPORTED, "4 GiB or more of query in one launch");
    v.n_items = (uint32_t)n_items;

    const size_t padded = ((v.total + 15) / 16) * 16 + 16;
    B.q.ensure(padded);
    B.off.ensure((n_seqs + 1) * sizeof(uint64_t));
    B.items.ensure(n_items * sizeof(kbo::WalkItem));
    B.ms.ensure(padded);
    v.q = v.bytes_out = B.q.as<uint8_t>();
    v.offsets = B.off.as<uint64_t>();
    v.items = B.items.as<kbo::WalkItem>();
    hipStream_t up = ask.copy_stream ? ask.copy_stream : stream;
    auto upload = [&](void *dst, const void *src, size_t n) {
        HIP_OK(hipMemcpyAsync(dst, src, n, hipMemcpyHostToDevice, up));
        if (hs && hs->staged) hs->staged->fetch_add(n, std::memory_order_relaxed);
    };
    const bool uniform = packed && packed->uniform_len != 0;
    // the '-' strand alone: the upload goes to B.raw and its reverse complement where the walk reads; both: the upload is the
    // first half of the walk's buffers and its reverse complement the second
    const size_t up_words = packed ? packed->n_words : 0, up_exc = packed ? packed->n_exc : 0;
    if (strands == 2) B.raw.ensure(packed ? up_words * 4 + 16 : ((up_total + 15) / 16) * 16 + 16);
    if (packed) { // a quarter of the bytes: 2-bit words + the non-ACGT list; unpacked into B.q below
        B.packed.ensure((both ? 2 : 1) * up_words * 4 + 16);
        upload(strands == 2 ? B.raw.p : B.packed.p, packed->words, up_words * 4);
        if (up_exc) {
            B.exc_pos.ensure((rev ? 2 : 1) * up_exc * 8);
            B.exc_byte.ensure((rev ? 2 : 1) * up_exc);
            upload(B.exc_pos.p, packed->exc_pos, up_exc * 8);
            upload(B.exc_byte.p, packed->exc_byte, up_exc);
        }
    } else {
        upload(strands == 2 ? B.raw.p : B.q.p, concat, up_total);
    }
    if (!uniform) upload(B.off.p, offsets, (n_up + 1) * sizeof(uint64_t));
    if (v.chunk) upload(B.items.p, items_keep.data(), items_keep.size() / (both ? 2 : 1) * sizeof(kbo::WalkItem));
    if (ask.copy_stream) {
        HIP_OK(hipEventRecord(ask.copied, ask.copy_stream));
        HIP_OK(hipStreamWaitEvent(stream, ask.copied, 0));
    }
    if (both && !uniform) HIP_OK(kbo::launch_double_offsets(B.off.as<uint64_t>(), (uint32_t)n_up, stream));
    if (both && v.chunk) // (a sequence's chunks depend on its length alone: the second half's items are the first's, up_total on)
        HIP_OK(kbo::launch_double_items(B.items.as<kbo::WalkItem>(), (uint32_t)(items_keep.size() / 2), up_total, stream));
    if (packed) {
        if (uniform) HIP_OK(kbo::launch_uniform_offsets(B.off.as<uint64_t>(), (uint32_t)n_seqs, packed->uniform_len, stream));
        else {
            B.pscr.ensure(kbo::chunk_items_scratch_words((uint32_t)n_seqs) * sizeof(uint32_t));
            HIP_OK(kbo::launch_packed_prefix(B.off.as<uint64_t>(), (uint32_t)n_seqs, B.pscr.as<uint32_t>(), stream));
        }
    }
    if (packed) { // what the kernels see of a packed slab: its words and its list, with the '-' strand where asked for
        v.have_bytes = false;
        v.qp = B.packed.as<uint32_t>();
        v.n_words = (both ? 2 : 1) * up_words;
        v.wps = uniform ? (packed->uniform_len + 15u) / 16u : 0u;
        v.pscr = uniform ? nullptr : B.pscr.as<uint32_t>();
        v.exc_pos = B.exc_pos.as<uint64_t>() + (strands == 2 ? up_exc : 0);
        v.exc_byte = B.exc_byte.as<uint8_t>() + (strands == 2 ? up_exc : 0);
        v.n_exc = (uint32_t)((both ? 2 : 1) * up_exc);
        v.exc_base = packed->base;
    }
    if (rev && packed) {
        HIP_OK(kbo::launch_revcomp_packed(strands == 2 ? B.raw.as<uint32_t>() : B.packed.as<uint32_t>(), (uint32_t)up_words, B.off.as<uint64_t>(),
                                          (uint32_t)n_up, v.wps, v.pscr, v.pscr ? v.pscr + n_seqs + 1u : nullptr,
                                          B.packed.as<uint32_t>() + (both ? up_words : 0), stream));
        HIP_OK(kbo::launch_revcomp_exceptions(B.exc_pos.as<uint64_t>(), B.exc_byte.as<uint8_t>(), (uint32_t)up_exc, packed->base, B.off.as<uint64_t>(),
                                              (uint32_t)n_up, packed->base + (both ? up_total : 0), B.exc_pos.as<uint64_t>() + up_exc,
                                              B.exc_byte.as<uint8_t>() + up_exc, stream));
    } else if (rev) {
        HIP_OK(kbo::launch_revcomp_bytes(strands == 2 ? B.raw.as<uint8_t>() : B.q.as<uint8_t>(), B.off.as<uint64_t>(), (uint32_t)n_up, up_total,
                                         B.q.as<uint8_t>() + (both ? up_total : 0), stream));
    }
    if (!v.chunk) HIP_OK(kbo::launch_make_items(B.off.as<uint64_t>(), (uint32_t)n_seqs, B.items.as<kbo::WalkItem>(), stream));
    return v;
}

// upload + A1 over a host batch (asynchronous on `stream`); leaves ms (and lo/hi) on the device.
// `items_keep` must stay alive until the stream has been synchronised.
void enqueue_walk_host(kbo_index *idx, const uint8_t *concat, const uint64_t *offsets, size_t n_seqs, BatchOnDevice &B,
                       std::vector<kbo::WalkItem> &items_keep, hipStream_t stream, const WalkHostAsk &ask)
{
    const bool want_ival = ask.want_ival;
    const CallSink *call = ask.call;
    FusedMap *map = ask.map;
    KBO_REQUIRE(idx->host.k <= 255, KBO_E_UNSUPPORTED, "k > 255");
    KBO_REQUIRE(!ask.stage || ask.stage->strands != 3 || n_seqs % 2 == 0, KBO_E_BAD_ARG, "both strands: a doubled slab");
    const std::vector<kbo_index *> shards = shards_of(idx);
    KBO_REQUIRE(shards.size() == 1 || (!want_ival && !call), KBO_E_UNSUPPORTED,
                "intervals and the call mode need the rows of one index; this handle is a sharded index");
    BatchView v = stage_walk_host(idx, concat, offsets, n_seqs, B, items_keep, stream, ask);
    // the slab's own buffers for what the routes leave or need on the way; those not every route takes grow when one does
    for (DevBuf *b : {&B.lo, &B.hi})
        if (want_ival) b->ensure(v.total * sizeof(uint32_t));
    if (shards.size() > 1) B.ms_shard.ensure(((v.total + 15) / 16) * 16 + 16);
    v.exc_flag.grow = &B.exc_flag;
    v.plan.grow = &B.plan;
    v.ms = B.ms.as<uint8_t>();
    v.ms_shard = B.ms_shard.as<uint8_t>();
    v.long_work.grow = &B.longw;
    const WalkAsk wask{want_ival ? B.lo.as<uint32_t>() : nullptr, want_ival ? B.hi.as<uint32_t>() : nullptr, call};
    if (shards.size() > 1) return walk_shards(v, idx, nullptr, wask, stream); // (every shard is walked, the maximum kept)
    const CopyView c = copy_view(shards[0], v.total);
    kbo::WalkArgs a = walk_args(v, c, v.ms, wask, !v.chunk && !call ? map : nullptr);
    if (map && !call && !want_ival) route_map(v, c, a, *map, ReadsLaunch{stream, stream}); // kbo::matches / map: the one kernel where it applies
    if (!map || !map->done) walk_shards(v, idx, &c, wask, stream, &a); // (A1 alone: the caller runs A5 / A6)
}

void run_walk_host(kbo_index *idx, const uint8_t *concat, const uint64_t *offsets, size_t n_seqs,
                   bool want_ival, BatchOnDevice &B, hipStream_t stream)
{
    check_batch(concat, offsets, n_seqs);
    std::vector<kbo::WalkItem> items;
    WalkHostAsk ask;
    ask.want_ival = want_ival;
    enqueue_walk_host(idx, concat, offsets, n_seqs, B, items, stream, ask);
    HIP_OK(hipStreamSynchronize(stream)); // the items vector must outlive the async copy
}

// ---- slabs: a host batch is processed in pieces of at most g_slab_bytes of query so that
// (a) one launch stays below the 32-bit offset limits and (b) the H2D copy of slab i+1 and
// the D2H copy of slab i-1 overlap the kernels of slab i (two streams, user buffers pinned
// in place with hipHostRegister when that succeeds).
std::atomic<int> g_host_in_place{std::getenv("KBO_HOST_INPLACE") ? std::atoi(std::getenv("KBO_HOST_INPLACE")) : 0};
std::atomic<size_t> g_slab_bytes{16ull << 20}; // tools/bench_host.py, 600 Mbp of C2 reads through the one kernel: 16 / 24 / 32 / 64 MiB 39 / 36 / 32-39 / 31 Gbp/s (bytes), 121 / 89 / 104 Gbp/s (packed)


std::vector<Slab> make_slabs(const uint64_t *offsets, size_t n_seqs, size_t max_bytes)
{
    std::vector<Slab> slabs;
    size_t s0 = 0;
    while (s0 < n_seqs) {
        // last s1 with offsets[s1] - offsets[s0] <= max_bytes (at least one sequence per slab)
        size_t s1 = std::upper_bound(offsets + s0 + 1, offsets + n_seqs + 1, offsets[s0] + max_bytes) - offsets - 1;
        s1 = std::max(s1, s0 + 1);
        slabs.push_back(Slab{s0, s1, offsets[s0], offsets[s1]});
        s0 = s1;
    }
    // the last slab in halves and quarters: what the pipeline cannot hide is the last slab's way through it (upload, kernels,
    // download, copy out - 1.1 ms of a 4.8 ms call over 600 Mbp of packed reads), and that way is shorter for a smaller slab
    static const int env_taper = std::getenv("KBO_SLAB_TAPER") ? std::atoi(std::getenv("KBO_SLAB_TAPER")) : 1; // experiments
    if (env_taper && slabs.size() >= 3) {
        const Slab last = slabs.back();
        const size_t n = last.s1 - last.s0;
        if (n >= 64) {
            slabs.pop_back();
            const size_t cut[4] = {last.s0, last.s0 + n / 2, last.s0 + n / 2 + n / 4, last.s1};
            for (int i = 0; i < 3; i++) slabs.push_back(Slab{cut[i], cut[i + 1], offsets[cut[i]], offsets[cut[i + 1]]});
        }
    }
    return slabs;
}

// Slabs of a packed batch: four times the bases of a byte slab (the same bytes over PCIe).  Large on purpose: the guided
// walk has a fixed cost of about 0.19 ms per launch whatever the slab holds (its longest chain of units; a slab of 56 k reads
// spends 0.4 ms in kernels, 21 Gbp/s, one of 894 k reads 1.1 ms, 122 Gbp/s), so slabs that start small and grow - tried, to
// shorten the pipeline's unhidden first upload and last download - lose more than they hide (tools/bench_host.py PACKED=1,
// 600 Mbp: equal slabs of 32 / 64 / 128 MiB of bases 58 / 72 / 81 Gbp/s, ramped 8 .. 128 MiB 69).
size_t slab_bytes_for(const kbo_index *idx)
{
    const size_t v = idx ? idx->opts.slab_bytes.load() : 0;
    return v ? v : g_slab_bytes.load();
}
size_t packed_slab_bytes(const kbo_index *idx) { return std::min<size_t>(4 * slab_bytes_for(idx), 0xC0000000ull); }

// one pass over the offsets of a batch: order, emptiness, shortest and longest sequence
OffsetScan scan_offsets(const uint64_t *offsets, size_t n_seqs)
{
    const size_t piece = 1u << 18;
    const size_t n_tasks = (n_seqs + piece - 1) / piece;
    std::vector<OffsetScan> part(n_tasks);
    HostTeam::get().run(n_tasks, [&](size_t t) {
        OffsetScan r;
        const size_t a = t * piece, b = std::min(n_seqs, a + piece);
        for (size_t s = a; s < b; s++) {
            r.monotone &= offsets[s + 1] >= offsets[s];
            const uint64_t len = offsets[s + 1] - offsets[s];
            r.shortest = std::min(r.shortest, len);
            r.longest = std::max(r.longest, len);
        }
        part[t] = r;
    });
    OffsetScan r;
    for (const OffsetScan &x : part) {
        r.monotone &= x.monotone;
        r.shortest = std::min(r.shortest, x.shortest);
        r.longest = std::max(r.longest, x.longest);
    }
    return r;
}

bool is_pinned_host(const void *ptr) // memory the DMA engines can reach without staging
{
    // (off by default: on the MI355X boxes here the copies between a caller's large pinned buffers and the device run at 28 GB/s
    // each way, those between the slots' small staging buffers and the device at 38 - the host team's copies included: 600 Mbp
    // of pinned reads 27.7 in place against 34.9 Gbp/s staged, packed 104 against 123.  kbo_set_host_in_place(1) / KBO_HOST_INPLACE=1)
    if (!g_host_in_place.load()) return false;
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, ptr) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return attr.type == hipMemoryTypeHost;
}

// ---- per-device scratch of the host batch entry points, kept between calls: slabs rotate
// through kHostSlots slots, each with its own stream, device buffers and pinned staging, so
// that the staging copy + H2D of slab i+1 and the D2H + copy-out of slab i-1 overlap the
// kernels of slab i.
constexpr int kHostSlots = 4;
struct HostSlot {
    BatchOnDevice B;
    DevBuf chars;
    PinBuf in, out, off, lo_pin, hi_pin;
    std::vector<kbo::WalkItem> items;
    hipEvent_t copied = nullptr, computed = nullptr, done = nullptr;
    bool busy = false;     // a slab is in flight in this slot
    size_t slab_id = 0, n_seqs = 0; // which slab, its sequences ...
    uint32_t longest = 0;           // ... and the longest of them
    // run-length output (kbo_find_batch): per-sequence first-run indices + block sums, the records,
    // the number of runs (device word and its pinned copy), what the slab holds
    DevBuf rle_scratch, rles, rle_total, dt_work;
    PinBuf rle_total_pin, rle_first_pin;
    size_t rle_capacity = 0, rle_count = 0; // records the emit has room for / the slab has (known once its kernels are done)
    // sparse output (kbo_matches_batch_sparse): runs per workgroup + scan, the records, their number (device word, pinned copy)
    DevBuf sp_scratch, sp_runs, sp_total;
    DevBuf summary; // kbo_summary_batch[_packed]: the slab's records
    PinBuf sp_total_pin;
    size_t sp_capacity = 0, sp_spec = 0; // records the emit has room for / the download took behind the count, unasked
    uint32_t sp_blocks = 0;
};
struct HostCtx {
    int dev = 0;
    HostSlot slot[kHostSlots];
    // one stream per stage, so that every stage runs one slab at a time, in order, next to the
    // other two stages: upload (copy engine), kernels, download (copy kernel)
    hipStream_t st_up = nullptr, st_run = nullptr, st_down = nullptr;
    explicit HostCtx(int d) : dev(d)
    {
        for (hipStream_t *st : {&st_up, &st_run, &st_down}) HIP_OK(hipStreamCreateWithFlags(st, hipStreamNonBlocking));
        for (HostSlot &S : slot)
            for (hipEvent_t *e : {&S.copied, &S.computed, &S.done}) HIP_OK(hipEventCreateWithFlags(e, hipEventDisableTiming));
    }
    ~HostCtx()
    {
        int prev = 0;
        (void)hipGetDevice(&prev);
        (void)hipSetDevice(dev);
        for (hipStream_t st : {st_up, st_run, st_down})
            if (st) { (void)hipStreamSynchronize(st); (void)hipStreamDestroy(st); }
        for (HostSlot &S : slot)
            for (hipEvent_t e : {S.copied, S.computed, S.done})
                if (e) (void)hipEventDestroy(e);
        for (HostSlot &S : slot) { // buffers belong to `dev`
            S.B.release();
            for (DevBuf *b : {&S.chars, &S.rle_scratch, &S.rles, &S.rle_total, &S.dt_work, &S.sp_scratch, &S.sp_runs, &S.sp_total}) b->release();
        }
        (void)hipSetDevice(prev);
    }
};
std::mutex g_ctx_mu;
// leaked on purpose: destroying streams from a static destructor would run after the HIP runtime is gone
std::vector<std::unique_ptr<HostCtx>> &g_ctx_pool = *new std::vector<std::unique_ptr<HostCtx>>();

struct CtxLease { // takes a context of the device out of the pool (or makes one), puts it back
    std::unique_ptr<HostCtx> ctx;
    explicit CtxLease(int dev)
    {
        {
            std::lock_guard<std::mutex> g(g_ctx_mu);
            for (size_t i = 0; i < g_ctx_pool.size(); i++)
                if (g_ctx_pool[i]->dev == dev) {
                    ctx = std::move(g_ctx_pool[i]);
                    g_ctx_pool.erase(g_ctx_pool.begin() + i);
                    break;
                }
        }
        if (!ctx) ctx.reset(new HostCtx(dev));
    }
    ~CtxLease()
    {
        bool busy = false; // an error may have left work in flight
        for (HostSlot &S : ctx->slot) {
            busy |= S.busy;
            S.busy = false;
        }
        if (busy)
            for (hipStream_t st : {ctx->st_up, ctx->st_run, ctx->st_down}) (void)hipStreamSynchronize(st);
        // keep at most kPooledPerDevice contexts per device (each holds ~0.8 GB of device and ~0.3 GB of
        // pinned memory at the default slab size); the scratch of further concurrent callers is freed
        std::unique_lock<std::mutex> g(g_ctx_mu);
        size_t same = 0;
        for (const auto &c : g_ctx_pool) same += c->dev == ctx->dev;
        if (same < kPooledPerDevice) {
            g_ctx_pool.push_back(std::move(ctx));
            return;
        }
        g.unlock();
        ctx.reset(); // ~HostCtx switches to its device and back
    }
    static constexpr size_t kPooledPerDevice = 2;
};

void check_len_threshold(const uint64_t *offsets, size_t n_seqs, size_t k, size_t threshold)
{
    KBO_REQUIRE(k > 0, KBO_E_BAD_ARG, "k > 0 (derandomize.rs:274)");
    KBO_REQUIRE(threshold > 1, KBO_E_THRESHOLD_LE_1, "threshold > 1 (derandomize.rs:275, translate.rs:269)");
    for (size_t s = 0; s < n_seqs; s++)
        KBO_REQUIRE(offsets[s + 1] - offsets[s] > 2, KBO_E_LEN_LE_2,
                    "len > 2 (derandomize.rs:276, translate.rs:270)");
}

// A5+A6 over a batch whose offsets are known on the host: reads -> LDS kernel, medium
// sequences -> one lane each, very long sequences -> chunked scan (one at a time).
void derand_translate_host_offsets(const uint8_t *d_ms, const uint64_t *d_off, const uint64_t *offsets, size_t n_seqs,
                                   uint32_t k, uint32_t threshold, const uint8_t *d_ref, uint8_t *d_chars,
                                   int32_t *d_derand, hipStream_t stream, uint32_t longest, DevBuf *piece_work)
{
    const uint32_t mx = longest ? longest : max_len(offsets, n_seqs);
    void *work = nullptr;
    size_t work_bytes = 0;
    if (piece_work && mx > 480 && !d_derand) {
        work_bytes = kbo::derand_piece_work_bytes((uint32_t)n_seqs, offsets[n_seqs]);
        piece_work->ensure(work_bytes);
        work = piece_work->p;
    }
    HIP_OK(kbo::launch_derand_translate(d_ms, d_off, (uint32_t)n_seqs, k, threshold, d_ref, d_chars, d_derand, mx,
                                        kbo::kLongSeq, stream, offsets[n_seqs], work, work_bytes));
    if (mx <= kbo::kLongSeq) return;
    size_t need = 0;
    for (size_t s = 0; s < n_seqs; s++) {
        const uint64_t len = offsets[s + 1] - offsets[s];
        if (len > kbo::kLongSeq) need = std::max(need, kbo::derand_long_scratch_bytes(len, k, threshold));
    }
    DevBuf scratch(need);
    for (size_t s = 0; s < n_seqs; s++) {
        const uint64_t b = offsets[s], len = offsets[s + 1] - offsets[s];
        if (len <= kbo::kLongSeq) continue;
        HIP_OK(kbo::launch_derand_long(d_ms + b, (uint32_t)len, k, threshold, d_ref ? d_ref + b : nullptr, d_chars + b,
                                       d_derand ? d_derand + b : nullptr, scratch.p, stream));
    }
    HIP_OK(hipStreamSynchronize(stream)); // scratch is released on return
}

void widen_rles(kbo_rle *dst, const uint32_t *src, size_t n, HostTeam &team)
{
    const size_t piece = 1u << 14;
    team.run((n + piece - 1) / piece, [&](size_t t) {
        const size_t a = t * piece, b = std::min(n, a + piece);
        for (size_t q = a; q < b; q++) {
            const uint32_t *r = src + q * kRleWords;
            dst[q] = kbo_rle{r[0], r[1], r[2], r[3], r[4], r[5], r[6]};
        }
    });
}


// ---- the slab pipeline of kbo::matches / map / find / the MS values over a host batch (lib.rs:618-627; relative_to_ref
// lib.rs:756-757; run lengths lib.rs:816-820): every slab is staged, walked, and leaves by its mode's output stage
thread_local uint64_t t_last_staged = 0;

namespace {

// slabs of kbo_summary_batch[_packed] by the route they took (kbo_hip_tuning.h kbo_summary_slab_routes)
std::atomic<uint64_t> g_summary_kernel_slabs{0}, g_summary_reducer_slabs{0};

// what a batch call hands to its per-device workers
struct BatchJob {
    HostOut out; // the mode and its destination
    kbo_index *idx;
    const uint8_t *concat = nullptr; // nullptr for a packed batch
    const uint64_t *offsets;
    uint32_t k, threshold = 0;
    bool in_pinned = false, out_pinned = false; // user buffers the DMA engines reach directly are used in place
    std::vector<Slab> slabs;
    std::vector<int> devices;
    size_t n_workers = 1; // one per device of the list, as far as there are slabs
    PhaseClock *clk;      // phase timing (worker 0 only)
    size_t max_gap_len = 0;                        // Rle, Rle32: FindOpts' max_gap_len
    // a packed batch (kbo_matches_batch_packed / kbo_find_batch_packed / kbo_matches_batch_sparse): 2-bit words in
    const PackedBatch *packed = nullptr;
    std::vector<uint64_t> pw;       // first word of every sequence (n_seqs + 1), empty when ...
    uint32_t uniform_len = 0;       // ... all sequences have this many bases
    uint64_t word_of(size_t s) const { return pw.empty() ? (uint64_t)s * ((uniform_len + 15u) / 16u) : pw[s]; }
    uint32_t words_per_seq() const { return uniform_len ? (uniform_len + 15u) / 16u : 0u; }
    bool rle_mode() const { return out.mode == OutMode::Rle || out.mode == OutMode::Rle32; }
    // the strands the batch is compared in (KBO_STRAND_*; Chars, Words, Rle, Rle32).  With both, every slab is doubled on the
    // device (HostStage): uploaded once, walked as 2 ns sequences, and its two halves leave for out.chars_out / packed_out ('+')
    // and out.chars_rev / packed_rev ('-'); a sink puts the records in (sequence, strand) order.  One strand: that destination only.
    int strands = 1;
    std::atomic<uint64_t> *staged = nullptr; // host -> device bytes of the whole batch
    template <typename T, typename F> void for_strands(T *fwd, T *rev, size_t half, F f) const // f(destination, where the strand begins in the slab's output)
    {
        if (strands & 1) f(fwd, (size_t)0);
        if (strands & 2) f(rev, strands == 3 ? half : (size_t)0);
    }
};

// One device's share of a batch: slabs `first`, `first + stride`, ... rotate through the slots of a
// leased HostCtx.  The calling thread stages and submits slabs; a second thread completes them in
// submission order (downloads, copies the staged output to the user's memory), so the two host
// copies of a slab never queue behind each other.
class SlabWorker {
public:
    SlabWorker(const BatchJob &job, int device, size_t first, size_t stride, bool timed)
        : job_(job), device_(device), first_(first), stride_(stride), timed_(timed)
    {
    }

    void run()
    {
        HIP_OK(hipSetDevice(device_));
        CtxLease lease(device_);
        C_ = lease.ctx.get();
        std::thread drainer([this] { drain_loop(); });
        auto join_drainer = [&] {
            {
                std::lock_guard<std::mutex> g(mu_);
                stop_ = true;
            }
            cv_.notify_all();
            if (drainer.joinable()) drainer.join();
        };
        try {
            size_t turn = 0;
            for (size_t i = first_; i < job_.slabs.size(); i += stride_, turn++) {
                {
                    std::unique_lock<std::mutex> g(mu_);
                    cv_.wait(g, [&] { return turn < drained_ + kHostSlots; }); // the slot is free again
                    if (drain_code_ != KBO_OK) break;
                }
                lap("  wait for a free slot");
                submit(turn, i);
                {
                    std::lock_guard<std::mutex> g(mu_);
                    submitted_++;
                }
                cv_.notify_all();
                lap("  enqueue");
            }
        } catch (...) {
            join_drainer();
            throw;
        }
        join_drainer();
        if (drain_code_ != KBO_OK) throw KboError(drain_code_, drain_error_);
        lap("drain");
    }

private:
    void lap(const char *what)
    {
        if (timed_) job_.clk->lap(what);
    }
    HostSlot &slot(size_t turn) { return C_->slot[turn % kHostSlots]; }

    // a slab as stage() leaves it: what the walk reads and what the mode's output stage needs to know of it
    struct SlabIn {
        const Slab *sl;
        size_t ns;           // sequences ...
        uint64_t bytes;      // ... and bases as the device sees them: twice the slab's own (hns, hbytes) when both strands run
        size_t hns;
        uint64_t hbytes;
        const uint64_t *off; // slab-relative offsets (pinned), ns + 1
        uint32_t longest;    // longest sequence
        const uint8_t *src;  // the bases (the caller's pinned memory or the slot's staging copy), nullptr for a packed batch ...
        PackedIn pin;        // ... which has this
        uint64_t w0, n_words, hwords; // a packed batch: the slab's first word in the batch's, its words on the device / of its own
    };

    // ---- submitting thread: stage the slab, enqueue upload, kernels and the mode's output stage
    void submit(size_t turn, size_t slab_id)
    {
        HostSlot &S = slot(turn);
        S.busy = true; // from the first enqueue on: if anything below throws, ~CtxLease drains the streams before the
                       // context (and the caller's pinned buffers the copies read) can be reused
        const SlabIn in = stage(S, slab_id);
        lap("  offsets + copy in");
        switch (job_.out.mode) {
        case OutMode::Ms: submit_ms(S, in); break;
        case OutMode::Chars: submit_chars(S, in); break;
        case OutMode::Words: submit_words(S, in); break;
        case OutMode::Rle:
        case OutMode::Rle32: submit_rle(S, in); break;
        case OutMode::Sparse: submit_sparse(S, in); break;
        case OutMode::Summary: submit_summary(S, in); break;
        }
    }

    // slab-relative offsets (and the longest sequence of the slab), query bytes or words
    SlabIn stage(HostSlot &S, size_t slab_id)
    {
        const Slab &sl = job_.slabs[slab_id];
        HostTeam &team = HostTeam::get();
        SlabIn in{};
        const bool both = job_.strands == 3;
        in.sl = &sl;
        in.hns = sl.s1 - sl.s0;
        in.hbytes = sl.b1 - sl.b0;
        in.ns = both ? 2 * in.hns : in.hns;
        in.bytes = both ? 2 * in.hbytes : in.hbytes;
        S.slab_id = slab_id;
        S.n_seqs = in.ns;
        const size_t ns = in.hns;
        S.off.ensure((in.ns + 1) * sizeof(uint64_t));
        uint64_t *off = S.off.as<uint64_t>();
        const uint64_t *offsets = job_.offsets;
        if (job_.packed && job_.uniform_len && job_.uniform_len <= 255u) { // (reads: below every chunk length, walk_chunk() >= 256)
            // equally long reads, packed: the offsets are made on the device and nothing below reads more of the host
            // copy than its last entry (one item per read, A5/A6 by the longest length)
            off[0] = 0;
            off[ns] = in.hbytes;
            off[in.ns] = in.bytes;
            in.longest = job_.uniform_len;
        } else {
            const size_t piece = 1u << 15, n_tasks = (ns + 1 + piece - 1) / piece;
            std::vector<uint64_t> longest(n_tasks, 0);
            team.run(n_tasks, [&](size_t t) {
                const size_t a = t * piece, b = std::min(ns + 1, a + piece);
                uint64_t m = 0;
                for (size_t j = a; j < b; j++) {
                    off[j] = offsets[sl.s0 + j] - sl.b0;
                    if (both && j) off[ns + j] = in.hbytes + off[j]; // (the '-' strands behind the '+' strands)
                    if (j < ns) m = std::max(m, offsets[sl.s0 + j + 1] - offsets[sl.s0 + j]);
                }
                longest[t] = m;
            });
            in.longest = (uint32_t)*std::max_element(longest.begin(), longest.end());
        }
        in.off = off;
        S.longest = in.longest;
        if (job_.packed) {
            PackedIn &pin = in.pin;
            in.w0 = job_.word_of(sl.s0);
            in.hwords = job_.word_of(sl.s1) - in.w0;
            in.n_words = both ? 2 * in.hwords : in.hwords;
            pin.words = job_.packed->words + in.w0;
            pin.n_words = (size_t)in.hwords;
            if (!job_.in_pinned) {
                S.in.ensure(pin.n_words * 4 + 16);
                team.copy(S.in.p, pin.words, pin.n_words * 4);
                pin.words = S.in.as<uint32_t>();
            }
            const uint64_t *e0 = std::lower_bound(job_.packed->exc_pos, job_.packed->exc_pos + job_.packed->n_exc, sl.b0);
            const uint64_t *e1 = std::lower_bound(e0, job_.packed->exc_pos + job_.packed->n_exc, sl.b1);
            pin.exc_pos = e0;
            pin.exc_byte = job_.packed->exc_byte + (e0 - job_.packed->exc_pos);
            pin.n_exc = (size_t)(e1 - e0);
            pin.base = sl.b0;
            pin.uniform_len = job_.uniform_len;
        } else {
            in.src = job_.concat + sl.b0;
            if (!job_.in_pinned) {
                S.in.ensure(in.hbytes);
                team.copy(S.in.p, in.src, in.hbytes);
                in.src = S.in.as<uint8_t>();
            }
        }
        return in;
    }

    // upload + A1 (or, with `fm`, the one kernel where it applies) on the slot's streams
    void walk(HostSlot &S, const SlabIn &in, FusedMap *fm)
    {
        const HostStage hs{job_.strands, job_.staged};
        WalkHostAsk ask;
        ask.want_ival = job_.out.lo_out != nullptr;
        ask.longest = in.longest;
        ask.copy_stream = C_->st_up;
        ask.copied = S.copied;
        ask.packed = job_.packed ? &in.pin : nullptr;
        ask.map = fm;
        ask.stage = &hs;
        enqueue_walk_host(job_.idx, in.src, in.off, in.ns, S.B, S.items, C_->st_run, ask);
    }
    // kbo::matches / map / find: the characters' buffer (and, words = true, that of their 2-bit words) before the walk, so
    // that the one kernel can write into it
    FusedMap fused_map(HostSlot &S, const SlabIn &in, bool words)
    {
        FusedMap fm{nullptr, job_.threshold, job_.out.format};
        S.chars.ensure(((in.bytes + 15) / 16) * 16 + 32);
        fm.d_chars = S.chars.as<uint8_t>();
        if (words) {
            S.B.packed_out.ensure((size_t)in.n_words * 4 + 16);
            fm.d_packed_out = S.B.packed_out.as<uint32_t>();
        }
        return fm;
    }
    // A5/A6 behind the walk where the one kernel has not left the characters already
    void chars_after_walk(HostSlot &S, const SlabIn &in, const FusedMap &fm)
    {
        if (fm.done) return;
        derand_translate_host_offsets(S.B.ms.as<uint8_t>(), S.B.off.as<uint64_t>(), in.off, in.ns, job_.k, job_.threshold,
                                      job_.out.format ? S.B.q.as<uint8_t>() : nullptr, S.chars.as<uint8_t>(), nullptr, C_->st_run,
                                      in.longest, &S.dt_work);
    }
    // ... and their 2-bit words (a quarter of the bytes) where the packed-native kernel has not written them itself
    void words_after_walk(HostSlot &S, const SlabIn &in, const FusedMap &fm)
    {
        chars_after_walk(S, in, fm);
        if (fm.packed_done) return;
        HIP_OK(kbo::launch_pack2(S.chars.as<uint8_t>(), (uint32_t)in.n_words, S.B.off.as<uint64_t>(), (uint32_t)in.ns,
                                 job_.words_per_seq(), job_.uniform_len ? nullptr : S.B.pscr.as<uint32_t>(),
                                 S.B.packed_out.as<uint32_t>(), C_->st_run));
    }
    void download_waits_for_kernels(HostSlot &S)
    {
        HIP_OK(hipEventRecord(S.computed, C_->st_run));
        HIP_OK(hipStreamWaitEvent(C_->st_down, S.computed, 0));
    }

    // A1 only: MS values (and intervals) straight back
    void submit_ms(HostSlot &S, const SlabIn &in)
    {
        HostCtx &C = *C_;
        const uint64_t bytes = in.bytes;
        walk(S, in, nullptr);
        download_waits_for_kernels(S);
        uint8_t *dst = job_.out.ms_out + in.sl->b0;
        uint32_t *dlo = job_.out.lo_out ? job_.out.lo_out + in.sl->b0 : nullptr, *dhi = job_.out.hi_out ? job_.out.hi_out + in.sl->b0 : nullptr;
        if (!job_.out_pinned) {
            S.out.ensure(bytes + 32);
            dst = S.out.as<uint8_t>();
            if (dlo) {
                S.lo_pin.ensure(bytes * sizeof(uint32_t));
                S.hi_pin.ensure(bytes * sizeof(uint32_t));
                dlo = S.lo_pin.as<uint32_t>();
                dhi = S.hi_pin.as<uint32_t>();
            }
        }
        HIP_OK(hipMemcpyAsync(dst, S.B.ms.p, bytes, hipMemcpyDeviceToHost, C.st_down));
        if (dlo) {
            HIP_OK(hipMemcpyAsync(dlo, S.B.lo.p, bytes * sizeof(uint32_t), hipMemcpyDeviceToHost, C.st_down));
            HIP_OK(hipMemcpyAsync(dhi, S.B.hi.p, bytes * sizeof(uint32_t), hipMemcpyDeviceToHost, C.st_down));
        }
        HIP_OK(hipEventRecord(S.done, C.st_down));
    }

    // one character per base.  D2H leg: hipMemcpyAsync on the download stream.  With one stream per stage the copy
    // engines carry both directions at once (tools/bench_host.py: 37-40 Gbp/s host->host; a small kernel storing
    // into pinned memory, or A5/A6 storing there themselves, gave 28 and 26 Gbp/s).
    void submit_chars(HostSlot &S, const SlabIn &in)
    {
        FusedMap fm = fused_map(S, in, false);
        walk(S, in, &fm);
        if (!job_.out_pinned) S.out.ensure(in.bytes + 32);
        chars_after_walk(S, in, fm);
        download_waits_for_kernels(S);
        job_.for_strands(job_.out.chars_out, job_.out.chars_rev, in.hbytes, [&](uint8_t *user, size_t at) {
            uint8_t *dst = job_.out_pinned ? user + in.sl->b0 : S.out.as<uint8_t>() + at;
            HIP_OK(hipMemcpyAsync(dst, S.chars.as<uint8_t>() + at, in.hbytes, hipMemcpyDeviceToHost, C_->st_down));
        });
        HIP_OK(hipEventRecord(S.done, C_->st_down));
    }

    // the characters as 2-bit words
    void submit_words(HostSlot &S, const SlabIn &in)
    {
        FusedMap fm = fused_map(S, in, true);
        walk(S, in, &fm);
        words_after_walk(S, in, fm);
        download_waits_for_kernels(S);
        if (!job_.out_pinned) S.out.ensure((size_t)in.n_words * 4 + 32);
        job_.for_strands(job_.out.packed_out, job_.out.packed_rev, (size_t)in.hwords, [&](uint32_t *user, size_t at) {
            uint32_t *dst = job_.out_pinned ? user + in.w0 : S.out.as<uint32_t>() + at;
            HIP_OK(hipMemcpyAsync(dst, S.B.packed_out.as<uint32_t>() + at, (size_t)in.hwords * 4, hipMemcpyDeviceToHost, C_->st_down));
        });
        HIP_OK(hipEventRecord(S.done, C_->st_down));
    }

    // run lengths: the characters stay on the device; their runs are counted, scanned and (speculatively, into
    // the room the slot has) emitted right behind A5/A6; the completing thread downloads them (start_download)
    void submit_rle(HostSlot &S, const SlabIn &in)
    {
        hipStream_t st = C_->st_run;
        const size_t ns = in.ns;
        const uint32_t gap = (uint32_t)std::min<size_t>(job_.max_gap_len, 0xFFFFFFFFu);
        FusedMap fm = fused_map(S, in, false);
        S.rle_scratch.ensure(kbo::chunk_items_scratch_words((uint32_t)ns) * sizeof(uint32_t));
        if (job_.max_gap_len == 0) fm.run_counts = S.rle_scratch.as<uint32_t>(); // FindOpts' default: the one kernel counts the runs itself
        walk(S, in, &fm);
        chars_after_walk(S, in, fm);
        S.rle_total.ensure(16);
        S.rle_total_pin.ensure(16);
        if (S.rle_capacity < 2 * ns + 16) {
            S.rle_capacity = 2 * ns + 16;
            S.rles.ensure(S.rle_capacity * kRleWords * sizeof(uint32_t));
        }
        if (fm.done && fm.counted) // (counts are there: scan + total)
            HIP_OK(kbo::launch_rle_scan_counts((uint32_t)ns, S.rle_scratch.as<uint32_t>(), S.rle_total.as<uint32_t>(), st));
        else
            HIP_OK(kbo::launch_rle_count(S.chars.as<uint8_t>(), S.B.off.as<uint64_t>(), (uint32_t)ns, gap,
                                         S.rle_scratch.as<uint32_t>(), S.rle_total.as<uint32_t>(), st, in.longest, true));
        HIP_OK(hipMemcpyAsync(S.rle_total_pin.p, S.rle_total.p, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        HIP_OK(kbo::launch_rle_emit(S.chars.as<uint8_t>(), S.B.off.as<uint64_t>(), (uint32_t)ns, gap,
                                    S.rle_scratch.as<uint32_t>(), S.rles.as<uint32_t>(), (uint32_t)S.rle_capacity,
                                    st, in.longest, true)); // (the characters are the kernels' own: M - X R)
        download_waits_for_kernels(S);
    }

    // one record per sequence: the characters (bytes; a packed batch's reads go through the packed-native kernel that writes bytes) are
    // counted where they are (summary_kernels.hip) and 16 bytes a sequence leave
    void submit_summary(HostSlot &S, const SlabIn &in)
    {
        FusedMap fm = fused_map(S, in, false);
        S.summary.ensure(in.ns * sizeof(kbo_aln_summary));
        fm.d_summary = S.summary.as<uint4>();
        walk(S, in, &fm);
        (fm.summarized ? g_summary_kernel_slabs : g_summary_reducer_slabs).fetch_add(1);
        if (!fm.summarized) { // (longer sequences, no depth table, a sharded index, a held-off copy: characters, then the reducer)
            chars_after_walk(S, in, fm);
            HIP_OK(kbo::launch_summary_bytes(S.chars.as<uint8_t>(), S.B.off.as<uint64_t>(), (uint32_t)in.ns, in.bytes, S.summary.as<uint4>(), C_->st_run));
        }
        download_waits_for_kernels(S);
        kbo_aln_summary *dst = job_.out.summary_out + in.sl->s0;
        if (!job_.out_pinned) {
            S.out.ensure(in.ns * sizeof(kbo_aln_summary));
            dst = S.out.as<kbo_aln_summary>();
        }
        HIP_OK(hipMemcpyAsync(dst, S.summary.p, in.ns * sizeof(kbo_aln_summary), hipMemcpyDeviceToHost, C_->st_down));
        HIP_OK(hipEventRecord(S.done, C_->st_down));
    }

    // only the runs of characters other than 'M': counted, scanned and (speculatively, into the room the slot has) emitted
    // behind the words, and downloaded with their number as many as the slabs before had (no round trip per slab); the
    // completing thread fetches the rest, if any (fetch_sparse_rest)
    void submit_sparse(HostSlot &S, const SlabIn &in)
    {
        HostCtx &C = *C_;
        const size_t ns = in.ns;
        FusedMap fm = fused_map(S, in, true);
        walk(S, in, &fm);
        words_after_walk(S, in, fm);
        S.sp_scratch.ensure(kbo::kSparseScratchWords * sizeof(uint32_t));
        S.sp_total.ensure(16);
        S.sp_total_pin.ensure(16);
        if (S.sp_capacity < 2 * ns + 16) {
            S.sp_capacity = 2 * ns + 16;
            S.sp_runs.ensure(S.sp_capacity * sizeof(kbo_aln_run));
        }
        S.sp_blocks = kbo::sparse_blocks((size_t)in.n_words);
        const uint32_t wps = job_.words_per_seq();
        const uint32_t *pre = job_.uniform_len ? nullptr : S.B.pscr.as<uint32_t>();
        HIP_OK(kbo::launch_sparse_count(S.B.packed_out.as<uint32_t>(), S.B.off.as<uint64_t>(), (uint32_t)ns, wps, pre, S.sp_blocks,
                                        S.sp_scratch.as<uint32_t>(), C.st_run));
        HIP_OK(kbo::launch_sparse_emit(S.B.packed_out.as<uint32_t>(), S.B.off.as<uint64_t>(), (uint32_t)ns, wps, pre, S.sp_blocks,
                                       S.sp_scratch.as<uint32_t>(), (uint32_t)in.sl->s0, S.sp_runs.as<uint32_t>(),
                                       (uint32_t)S.sp_capacity, S.sp_total.as<uint32_t>(), C.st_run));
        download_waits_for_kernels(S);
        const uint64_t per_kseq = sp_runs_per_kseq_.load(std::memory_order_relaxed); // (0: no slab finished yet)
        S.sp_spec = per_kseq ? std::min<size_t>(S.sp_capacity, (size_t)(ns * per_kseq / 1024 * 5 / 4) + 1024) : S.sp_capacity;
        S.out.ensure(S.sp_capacity * sizeof(kbo_aln_run));
        HIP_OK(hipMemcpyAsync(S.sp_total_pin.p, S.sp_total.p, sizeof(uint32_t), hipMemcpyDeviceToHost, C.st_down));
        HIP_OK(hipMemcpyAsync(S.out.p, S.sp_runs.p, S.sp_spec * sizeof(kbo_aln_run), hipMemcpyDeviceToHost, C.st_down));
        HIP_OK(hipEventRecord(S.done, C.st_down));
    }

    // ---- completing thread
    // run lengths: the number of records of a slab is known once its kernels are done, so the download
    // is issued here; it is issued for the next slab before the previous one is copied out, so that the
    // copy engine and the host copy work on different slabs
    void start_download(size_t turn)
    {
        HostSlot &S = slot(turn);
        HostCtx &C = *C_;
        HIP_OK(hipEventSynchronize(S.computed));
        const uint32_t total = *S.rle_total_pin.as<uint32_t>();
        if (total > S.rle_capacity) { // more runs than the speculative emit had room for
            S.rle_capacity = (size_t)total + total / 4 + 16;
            S.rles.ensure(S.rle_capacity * kRleWords * sizeof(uint32_t));
            HIP_OK(kbo::launch_rle_emit(S.chars.as<uint8_t>(), S.B.off.as<uint64_t>(), (uint32_t)S.n_seqs,
                                        (uint32_t)std::min<size_t>(job_.max_gap_len, 0xFFFFFFFFu),
                                        S.rle_scratch.as<uint32_t>(), S.rles.as<uint32_t>(), (uint32_t)S.rle_capacity,
                                        C.st_down, S.longest, true));
        }
        const size_t words = kbo::chunk_items_scratch_words((uint32_t)S.n_seqs);
        S.out.ensure(std::max<size_t>(16, (size_t)total * kRleWords * sizeof(uint32_t)));
        S.rle_first_pin.ensure(words * sizeof(uint32_t));
        if (total)
            HIP_OK(hipMemcpyAsync(S.out.p, S.rles.p, (size_t)total * kRleWords * sizeof(uint32_t), hipMemcpyDeviceToHost,
                                  C.st_down));
        HIP_OK(hipMemcpyAsync(S.rle_first_pin.p, S.rle_scratch.p, words * sizeof(uint32_t), hipMemcpyDeviceToHost, C.st_down));
        HIP_OK(hipEventRecord(S.done, C.st_down));
        S.rle_count = total;
    }

    // sparse records: those the speculative download did not take (more runs than the slabs before had: the rest of the emitted
    // ones; more than the emit had room for: emitted again into a larger buffer, all of them)
    void fetch_sparse_rest(HostSlot &S, uint32_t total)
    {
        HostCtx &C = *C_;
        size_t from = S.sp_spec;
        if (total > S.sp_capacity) {
            S.sp_capacity = (size_t)total + total / 4 + 16;
            S.sp_runs.ensure(S.sp_capacity * sizeof(kbo_aln_run));
            HIP_OK(kbo::launch_sparse_emit(S.B.packed_out.as<uint32_t>(), S.B.off.as<uint64_t>(), (uint32_t)S.n_seqs, job_.words_per_seq(),
                                           job_.uniform_len ? nullptr : S.B.pscr.as<uint32_t>(), S.sp_blocks, S.sp_scratch.as<uint32_t>(),
                                           (uint32_t)job_.slabs[S.slab_id].s0, S.sp_runs.as<uint32_t>(), (uint32_t)S.sp_capacity,
                                           S.sp_total.as<uint32_t>(), C.st_down));
            S.out.ensure((size_t)total * sizeof(kbo_aln_run)); // (a new buffer: everything comes again)
            from = 0;
        }
        HIP_OK(hipMemcpyAsync(S.out.as<kbo_aln_run>() + from, S.sp_runs.as<kbo_aln_run>() + from, (total - from) * sizeof(kbo_aln_run),
                              hipMemcpyDeviceToHost, C.st_down));
        HIP_OK(hipEventRecord(S.done, C.st_down));
        HIP_OK(hipEventSynchronize(S.done));
    }

    void finish(size_t turn)
    {
        HostSlot &S = slot(turn);
        HIP_OK(hipEventSynchronize(S.done));
        switch (job_.out.mode) {
        case OutMode::Ms: finish_ms(S); break;
        case OutMode::Chars: finish_chars(S); break;
        case OutMode::Words: finish_words(S); break;
        case OutMode::Rle: finish_rle(S, *job_.out.rle); break;
        case OutMode::Rle32: finish_rle(S, *job_.out.rle32); break;
        case OutMode::Sparse: finish_sparse(S); break;
        case OutMode::Summary: finish_summary(S); break;
        }
        S.busy = false;
        {
            std::lock_guard<std::mutex> g(mu_);
            drained_++;
        }
        cv_.notify_all();
    }

    // (the first three: a pinned destination took the download itself; otherwise the staged output is copied out)
    void finish_ms(HostSlot &S)
    {
        if (job_.out_pinned) return;
        const Slab &sl = job_.slabs[S.slab_id];
        const uint64_t bytes = sl.b1 - sl.b0;
        HostTeam::out().copy(job_.out.ms_out + sl.b0, S.out.p, bytes);
        if (job_.out.lo_out) {
            HostTeam::out().copy(job_.out.lo_out + sl.b0, S.lo_pin.p, bytes * sizeof(uint32_t));
            HostTeam::out().copy(job_.out.hi_out + sl.b0, S.hi_pin.p, bytes * sizeof(uint32_t));
        }
    }
    void finish_chars(HostSlot &S)
    {
        const Slab &sl = job_.slabs[S.slab_id];
        if (job_.out_pinned) return;
        job_.for_strands(job_.out.chars_out, job_.out.chars_rev, (size_t)(sl.b1 - sl.b0), [&](uint8_t *user, size_t at) {
            HostTeam::out().copy(user + sl.b0, S.out.as<uint8_t>() + at, sl.b1 - sl.b0);
        });
    }
    void finish_words(HostSlot &S)
    {
        const Slab &sl = job_.slabs[S.slab_id];
        const uint64_t w0 = job_.word_of(sl.s0), w1 = job_.word_of(sl.s1);
        if (job_.out_pinned) return;
        job_.for_strands(job_.out.packed_out, job_.out.packed_rev, (size_t)(w1 - w0), [&](uint32_t *user, size_t at) {
            HostTeam::out().copy(user + w0, S.out.as<uint32_t>() + at, (size_t)(w1 - w0) * 4);
        });
    }
    void finish_summary(HostSlot &S)
    {
        const Slab &sl = job_.slabs[S.slab_id];
        if (job_.out_pinned) return;
        HostTeam::out().copy(job_.out.summary_out + sl.s0, S.out.p, (sl.s1 - sl.s0) * sizeof(kbo_aln_summary));
    }
    template <typename T> void finish_rle(HostSlot &S, RleSink<T> &sink)
    {
        sink.append(S.slab_id, S.out.p, S.rle_count, S.rle_first_pin.as<uint32_t>(), HostTeam::out());
    }
    void finish_sparse(HostSlot &S)
    {
        const uint32_t total = *S.sp_total_pin.as<uint32_t>();
        if (total > S.sp_spec) fetch_sparse_rest(S, total);
        sp_runs_per_kseq_.store(std::max<uint64_t>(1, (uint64_t)total * 1024 / std::max<size_t>(1, S.n_seqs)), std::memory_order_relaxed);
        job_.out.sparse_runs->append(S.slab_id, S.out.p, total, HostTeam::out());
    }

    void drain_loop()
    {
        auto fail = [&](int code, const char *what) {
            std::lock_guard<std::mutex> g(mu_);
            drain_code_ = code;
            drain_error_ = what;
            drained_ = ~size_t(0) / 2; // releases the submitting thread
            cv_.notify_all();
        };
        try {
            HIP_OK(hipSetDevice(device_));
            const size_t none = ~size_t(0);
            size_t started = 0, pending = none;
            for (;;) {
                bool can_start;
                {
                    std::unique_lock<std::mutex> g(mu_);
                    cv_.wait(g, [&] { return started < submitted_ || pending != none || stop_; });
                    can_start = started < submitted_;
                    if (!can_start && pending == none) return;
                }
                const size_t prev = pending;
                pending = none;
                if (can_start) {
                    if (job_.rle_mode()) start_download(started);
                    pending = started++;
                }
                if (prev != none) finish(prev);
            }
        } catch (const KboError &e) {
            fail(e.code, e.what());
        } catch (const std::bad_alloc &) {
            fail(KBO_E_NOMEM, "out of host memory");
        } catch (const std::exception &e) {
            fail(KBO_E_HIP, e.what());
        }
    }

    const BatchJob &job_;
    const int device_;
    const size_t first_, stride_;
    const bool timed_;
    HostCtx *C_ = nullptr;
    std::mutex mu_;
    std::condition_variable cv_;
    size_t submitted_ = 0, drained_ = 0;
    std::atomic<uint64_t> sp_runs_per_kseq_{0}; // runs per 1024 sequences of the last sparse slab finished (sizes the next downloads)
    bool stop_ = false;
    int drain_code_ = KBO_OK;
    std::string drain_error_;
};

// one worker per device (index replicated on each, slabs dealt round-robin, disjoint output slices: no
// exchange between devices); a single device runs on the calling thread
void run_on_devices(const BatchJob &job)
{
    const size_t nd = job.n_workers;
    if (nd == 1) {
        DeviceScope scope(job.devices[0]); // (restores also when run() throws)
        SlabWorker(job, job.devices[0], 0, 1, true).run();
        return;
    }
    std::vector<std::thread> threads;
    std::vector<std::string> errors(nd);
    std::vector<int> codes(nd, KBO_OK);
    for (size_t w = 0; w < nd; w++)
        threads.emplace_back([&, w] {
            try {
                SlabWorker(job, job.devices[w], w, nd, w == 0).run();
            } catch (const KboError &e) {
                codes[w] = e.code;
                errors[w] = e.what();
            } catch (const std::exception &e) {
                codes[w] = KBO_E_HIP;
                errors[w] = e.what();
            }
        });
    for (auto &t : threads) t.join();
    for (size_t w = 0; w < nd; w++)
        if (codes[w] != KBO_OK) throw KboError(codes[w], errors[w]);
}

// The checks the host batch entry points share, in the order the tests pin (which error a doubly wrong call gets), and the
// scan of the offsets they are made from.  matches = true: + what derandomize / translate assert (kbo::matches, map, find).
// (k > 0 cannot fire, for the byte forms no more than for the packed ones: random_match_threshold has refused k = 0 before,
// and no handle has it - kbo_index_from_parts, the builders and the loader all refuse it; it stays as the reference's assert.)
OffsetScan checked_scan(const uint64_t *offsets, size_t n_seqs, bool matches, size_t k = 0, size_t threshold = 0)
{
    KBO_REQUIRE(n_seqs > 0, KBO_E_EMPTY_QUERY, "no sequences");
    KBO_REQUIRE(n_seqs < 0xFFFFFFFFull, KBO_E_UNSUPPORTED, "more than 2^32-1 sequences per call");
    KBO_REQUIRE(offsets[0] == 0, KBO_E_BAD_ARG, "offsets[0] must be 0");
    const OffsetScan scan = scan_offsets(offsets, n_seqs);
    KBO_REQUIRE(scan.monotone, KBO_E_BAD_ARG, "offsets not monotone");
    KBO_REQUIRE(scan.shortest > 0, KBO_E_EMPTY_QUERY, "empty query (index.rs:248 assert!(!query.is_empty()))");
    KBO_REQUIRE(scan.longest < 0xFFFFFFFFull, KBO_E_UNSUPPORTED, "sequence longer than 2^32-1");
    if (!matches) return scan;
    KBO_REQUIRE(k > 0, KBO_E_BAD_ARG, "k > 0 (derandomize.rs:274)");
    KBO_REQUIRE(threshold > 1, KBO_E_THRESHOLD_LE_1, "threshold > 1 (derandomize.rs:275, translate.rs:269)");
    KBO_REQUIRE(scan.shortest > 2, KBO_E_LEN_LE_2, "len > 2 (derandomize.rs:276, translate.rs:270)");
    return scan;
}

// the strands of a job (0: a single-strand entry point); slabs of half the bytes when they are doubled
size_t strand_slab_bytes(size_t bytes, int strands) { return strands == 3 ? std::max<size_t>(bytes / 2, 1u << 15) : bytes; }

// the slab list, the devices and their workers, and the destination: its sink begun, or whether the DMA engines reach it
BatchJob make_job(const HostOut &out, int strands, kbo_index *idx, const uint64_t *offsets, size_t n_seqs, size_t slab_bytes, size_t threshold,
                  PhaseClock &clk)
{
    BatchJob job;
    job.out = out;
    job.strands = strands ? strands : 1;
    job.idx = idx;
    job.offsets = offsets;
    job.k = idx->host.k;
    job.threshold = (uint32_t)threshold;
    job.slabs = make_slabs(offsets, n_seqs, strand_slab_bytes(slab_bytes, strands));
    job.devices = devices_for(idx);
    if (job.devices.empty()) job.devices.push_back(current_device());
    job.n_workers = std::min(job.devices.size(), std::max<size_t>(1, job.slabs.size()));
    job.clk = &clk;
    auto pinned = [&](const void *fwd, const void *rev) { return (!(job.strands & 1) || is_pinned_host(fwd)) && (!(job.strands & 2) || is_pinned_host(rev)); };
    auto begin_runs = [&](auto *sink) {
        job.max_gap_len = sink->max_gap_len;
        sink->strands = strands;
        sink->begin(job.slabs, n_seqs, job.n_workers == 1);
    };
    switch (out.mode) {
    case OutMode::Ms: job.out_pinned = is_pinned_host(out.ms_out) && (!out.lo_out || (is_pinned_host(out.lo_out) && is_pinned_host(out.hi_out))); break;
    case OutMode::Chars: job.out_pinned = pinned(out.chars_out, out.chars_rev); break;
    case OutMode::Words: job.out_pinned = pinned(out.packed_out, out.packed_rev); break;
    case OutMode::Rle: begin_runs(out.rle); break;
    case OutMode::Rle32: begin_runs(out.rle32); break;
    case OutMode::Sparse: out.sparse_runs->begin(job.slabs.size(), n_seqs, job.n_workers == 1); break;
    case OutMode::Summary: job.out_pinned = is_pinned_host(out.summary_out); break;
    }
    return job;
}

void run_counted(BatchJob &job) // ... and the count of what it uploads
{
    std::atomic<uint64_t> staged{0};
    job.staged = &staged;
    run_on_devices(job);
    t_last_staged = staged.load();
}

const char *const kBadStrands = "strands: KBO_STRAND_FWD, KBO_STRAND_REV or both";

} // namespace

void matches_batch_impl(kbo_index *idx, const uint8_t *concat, const uint64_t *offsets, size_t n_seqs, double max_error_prob, const HostOut &out,
                        int strands)
{
    KBO_REQUIRE(strands >= 0 && strands <= 3 && (!strands || out.takes_strands()), KBO_E_BAD_ARG, kBadStrands);
    KBO_REQUIRE(idx && out.complete(strands ? strands : 1), KBO_E_BAD_ARG, "null argument");
    PhaseClock clk;
    const size_t threshold = random_match_threshold(idx->host.k, idx->host.n_kmers, 4, max_error_prob); // lib.rs:620
    KBO_REQUIRE(concat && offsets, KBO_E_BAD_ARG, "null concat/offsets");
    checked_scan(offsets, n_seqs, true, idx->host.k, threshold);
    clk.lap("argument checks");
    BatchJob job = make_job(out, strands, idx, offsets, n_seqs, slab_bytes_for(idx), threshold, clk);
    job.concat = concat;
    job.in_pinned = is_pinned_host(concat);
    clk.lap("slab list");
    run_counted(job);
}

// kbo::matches / kbo::find over a batch of 2-bit packed reads: the same pipeline, a quarter of the bytes over PCIe each way
void matches_batch_packed_impl(kbo_index *idx, const PackedBatch &in, const uint64_t *offsets, size_t n_seqs, double max_error_prob,
                               const HostOut &out, int strands)
{
    KBO_REQUIRE(strands >= 0 && strands <= 3 && (!strands || out.takes_strands()), KBO_E_BAD_ARG, kBadStrands);
    KBO_REQUIRE(idx && in.words && out.complete(strands ? strands : 1), KBO_E_BAD_ARG, "null argument");
    KBO_REQUIRE(in.n_exc == 0 || (in.exc_pos && in.exc_byte), KBO_E_BAD_ARG, "null exception list");
    PhaseClock clk;
    const size_t threshold = random_match_threshold(idx->host.k, idx->host.n_kmers, 4, max_error_prob); // lib.rs:620
    KBO_REQUIRE(offsets, KBO_E_BAD_ARG, "null offsets");
    const OffsetScan scan = checked_scan(offsets, n_seqs, true, idx->host.k, threshold);
    KBO_REQUIRE(out.mode != OutMode::Sparse || scan.longest < (1ull << 30), KBO_E_UNSUPPORTED, "sequence of 2^30 bases or more (kbo_aln_run has 30 bits of length)");
    for (size_t x = 0; x < in.n_exc; x++) // (ascending, inside the batch: the slabs cut the list by binary search)
        KBO_REQUIRE(in.exc_pos[x] < offsets[n_seqs] && (x == 0 || in.exc_pos[x] > in.exc_pos[x - 1]), KBO_E_BAD_ARG,
                    "exception positions must ascend and lie inside the batch");
    clk.lap("argument checks");
    BatchJob job = make_job(out, strands, idx, offsets, n_seqs, packed_slab_bytes(idx), threshold, clk);
    job.packed = &in;
    job.in_pinned = is_pinned_host(in.words);
    if (scan.shortest == scan.longest) {
        job.uniform_len = (uint32_t)scan.longest;
    } else { // first word of every sequence
        job.pw.resize(n_seqs + 1);
        job.pw[0] = 0;
        for (size_t s = 0; s < n_seqs; s++) job.pw[s + 1] = job.pw[s] + (offsets[s + 1] - offsets[s] + 15) / 16;
    }
    clk.lap("slab list");
    run_counted(job);
}

// A1 over a host batch: MS values (and intervals) only
void ms_batch_impl(kbo_index *idx, const uint8_t *concat, const uint64_t *offsets, size_t n_seqs, uint8_t *d_out,
                   uint32_t *lo_out, uint32_t *hi_out)
{
    KBO_REQUIRE(idx && d_out, KBO_E_BAD_ARG, "null argument");
    KBO_REQUIRE((lo_out == nullptr) == (hi_out == nullptr), KBO_E_BAD_ARG, "lo/hi must come together");
    KBO_REQUIRE(concat && offsets, KBO_E_BAD_ARG, "null concat/offsets");
    checked_scan(offsets, n_seqs, false);
    PhaseClock clk;
    // intervals cost 8 more bytes per base on the device and on the way back: smaller slabs
    const size_t slab_bytes = lo_out ? std::max<size_t>(1u << 16, slab_bytes_for(idx) / 4) : slab_bytes_for(idx);
    BatchJob job = make_job(HostOut::ms(d_out, lo_out, hi_out), 0, idx, offsets, n_seqs, slab_bytes, 0, clk);
    job.concat = concat;
    job.in_pinned = is_pinned_host(concat);
    run_counted(job);
}

void summary_slab_routes(uint64_t *kernel_slabs, uint64_t *reducer_slabs)
{
    if (kernel_slabs) *kernel_slabs = g_summary_kernel_slabs.load();
    if (reducer_slabs) *reducer_slabs = g_summary_reducer_slabs.load();
}

void release_host_scratch()
{
    {
        std::lock_guard<std::mutex> g(g_ctx_mu);
        g_ctx_pool.clear();
    }
    // the calling thread's own caches (kbo_call / kbo_call_batch keep a transient-index arena and a small batch's device
    // buffers per host thread; pool threads free theirs when they exit)
    release_transient_arena();
}

} // namespace kbo_host
