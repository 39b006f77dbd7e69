// kbo_tuning.cpp — the knobs, experiment setters and test hooks declared in include/kbo_hip_tuning.h, as far as they are
// not a pipeline's own: host logic only, like kbo_capi.cpp.
#include "../../include/kbo_hip_tuning.h"

#include <algorithm>
#include <cstdlib>
#include <vector>

#include "capi_internal.hpp"
#include "map_subst.hpp"
#include "map_text.hpp"

using namespace kbo_host;

extern "C" {

int kbo_summary_slab_routes(uint64_t *kernel_slabs, uint64_t *reducer_slabs)
{
    summary_slab_routes(kernel_slabs, reducer_slabs);
    return KBO_OK;
}

int kbo_set_map_long(int mode)
{
    kbo::set_map_long(mode);
    return KBO_OK;
}

int kbo_walk_geometry(int *blocks, int *threads)
{
    return guarded([&] {
        if (blocks) *blocks = walk_max_waves();
        if (threads) *threads = kbo::kWalkThreads;
    });
}

int kbo_set_pair_steps(uint64_t min_rows, int min_depth)
{
    g_pair_min_rows = min_rows; // applies to device copies made after the call
    if (min_depth >= 0) kbo::set_pair_min_depth(min_depth);
    return KBO_OK;
}

int kbo_set_plan(int enabled, int seed_depth, int seed_cap)
{
    if (enabled >= 0) g_plan_enabled = enabled != 0; // launches from now on; path covers of device copies made from now on
    if (enabled > 0) plan_reset_holdoff();
    kbo::set_plan_params(seed_depth, seed_cap); // (<= 0 keeps a value)
    if (const char *e = std::getenv("KBO_PLAN_GAP")) kbo::set_plan_params(0, 0, std::atoi(e), 0);   // experiments
    if (const char *e = std::getenv("KBO_PLAN_BAIL")) kbo::set_plan_bail(std::atoi(e));
    if (const char *e = std::getenv("KBO_PLAN_CHUNK")) kbo::set_plan_params(0, 0, 0, std::atoi(e));
    return KBO_OK;
}

int kbo_index_depth_table(kbo_index_t *idx, int device, int view, uint8_t *table, size_t *n_bytes, int *order)
{
    return guarded([&] {
        KBO_REQUIRE(idx && n_bytes && order && view >= 0 && view < 3, KBO_E_BAD_ARG, "null argument / view not in 0..2");
        const int dev = resolve_device(device);
        const kbo::DevIndexView v = device_view(idx, dev, nullptr, 0, true); // (no table while kbo_set_depth_table(-1) is in force)
        const size_t need = v.dtab ? (size_t)1 << (2u * v.dtab_order) : 0;
        if (table && need) {
            KBO_REQUIRE(*n_bytes >= need, KBO_E_BAD_ARG, "buffer smaller than the table");
            KBO_REQUIRE(v.dtab_order <= 14u, KBO_E_UNSUPPORTED, "tables of more than 14 bases are not handed back (a test hook: GiBs through a host copy)");
            DeviceScope scope(dev);
            if (!v.dtab_grouped) HIP_OK(hipMemcpy(table, v.dtab, need, hipMemcpyDeviceToHost));
            else { // the grouped table holds every entry three times: the copy `view` of them, put back in key order
                std::vector<uint8_t> g(kbo::dtab_bytes(v.dtab_order, true));
                HIP_OK(hipMemcpy(g.data(), v.dtab, g.size(), hipMemcpyDeviceToHost));
                const uint32_t cb = 2u * (v.dtab_order - 2u);
                const uint64_t cm = (1ull << cb) - 1ull;
                for (uint64_t key = 0; key < need; key++) {
                    const uint64_t a = view == 0 ? ((key & cm) << 6) + (key >> cb)
                                     : view == 1 ? (((key >> 2) & cm) << 6) + 16u + ((key >> (cb + 2u)) << 2) + (key & 3u)
                                                 : ((key >> 4) << 6) + 32u + (key & 15u);
                    table[key] = g[a];
                }
            }
        }
        *n_bytes = need;
        *order = (int)v.dtab_order;
    });
}

// test hook (kbo_hip_tuning.h): one of the plan structures the copy on `device` made for itself, as it lies there, slack included
int kbo_index_plan_part(kbo_index_t *idx, int device, int part, void *out, size_t *n_bytes, uint32_t info[4])
{
    return guarded([&] {
        KBO_REQUIRE(idx && n_bytes && info && part >= 0 && part < KBO_PLAN_PARTS, KBO_E_BAD_ARG, "null argument / part not in 0 .. KBO_PLAN_PARTS - 1");
        const int dev = resolve_device(device);
        (void)device_view(idx, dev, nullptr, 0, true); // (makes the copy and its plan structures if there are none yet)
        std::lock_guard<std::mutex> g(idx->mu);
        const DevCopy &dc = copy_on(idx, dev);
        const uint64_t units = kbo::pack_text_units(idx->host.n_sets);
        const uint32_t shift = kbo::maptext::cell_shift(units);
        const bool seed_on_device = dc.dtab_order != 0 && dc.seed_d != 0 && dc.seed_d <= dc.dtab_order; // (build_plan_structures' rule)
        const DevBuf *buf = nullptr;
        size_t need = 0;
        uint32_t inf[4] = {0, 0, 0, 0};
        switch (part) {
        case KBO_PLAN_PART_PC_TM: buf = &dc.pc_tm, need = units * 8, inf[0] = (uint32_t)units, inf[1] = shift; break;
        case KBO_PLAN_PART_PC_T: buf = &dc.pc_t, need = units * 4 + 16, inf[0] = (uint32_t)units, inf[1] = shift; break;
        case KBO_PLAN_PART_PC_MU: buf = &dc.pc_mu, need = kbo::pack_text_mu_bytes(units) + 4, inf[0] = (uint32_t)units, inf[1] = shift; break;
        case KBO_PLAN_PART_PC_MC: buf = &dc.pc_mc, need = kbo::maptext::kCells / 8u, inf[0] = (uint32_t)units, inf[1] = shift; break;
        case KBO_PLAN_PART_SEED_TAB: buf = &dc.seed_tab, need = dc.seed_d ? (size_t)8 << (2u * dc.seed_d) : 0, inf[0] = dc.seed_d, inf[1] = seed_on_device; break;
        case KBO_PLAN_PART_SEED_POS: buf = &dc.seed_pos, need = (size_t)4 << (2u * dc.seed_d), inf[0] = dc.seed_d, inf[1] = seed_on_device; break;
        case KBO_PLAN_PART_DFILT: buf = &dc.dfilt, need = dc.dfilt_bases ? ((size_t)1 << (2u * dc.dfilt_bases)) / 8u : 0, inf[0] = dc.dfilt_bases, inf[1] = dc.dtab_order; break;
        case KBO_PLAN_PART_ANCHOR: buf = &dc.anchor, need = dc.anchor_bits ? (size_t)8 << dc.anchor_bits : 0, inf[0] = dc.anchor_bits, inf[1] = dc.dtab_order; break;
        case KBO_PLAN_PART_SUB_GROUP: buf = &dc.sub_group, need = kbo::mapsubst::group_words(units) * 4 + kbo::mapsubst::kGroupSlack, inf[0] = (uint32_t)units, inf[1] = dc.dtab_order, inf[2] = dc.sub_thr, inf[3] = dc.sub_anch ? 1u : 0u; break;
        default: buf = &dc.sub_clean, need = kbo::mapsubst::bitmap_words(units) * 4, inf[0] = (uint32_t)units, inf[1] = dc.dtab_order, inf[2] = dc.sub_thr, inf[3] = dc.sub_anch ? 1u : 0u; break;
        }
        if (!buf->p) need = 0; // (a part this copy does not have)
        if (out && need) {
            KBO_REQUIRE(*n_bytes >= need, KBO_E_BAD_ARG, "buffer smaller than the part");
            DeviceScope scope(dev);
            HIP_OK(hipMemcpy(out, buf->p, need, hipMemcpyDeviceToHost));
        }
        *n_bytes = need;
        for (int i = 0; i < 4; i++) info[i] = need ? inf[i] : 0u;
    });
}

int kbo_set_walk_experiment(int lane_limit, int dummy_lds_bytes)
{
    kbo::set_walk_experiment(lane_limit, dummy_lds_bytes);
    return KBO_OK;
}

int kbo_set_plan_tuning(int gap, int chunk, int bail_x16)
{
    kbo::set_plan_params(0, 0, gap, chunk);
    if (bail_x16 >= 0) kbo::set_plan_bail(bail_x16);
    return KBO_OK;
}

int kbo_set_plan_unit_cap_divisor(int divisor)
{
    g_plan_cap_div = std::max(1, divisor);
    return KBO_OK;
}

int kbo_set_index_shards(int shards)
{
    g_index_shards = std::max(0, shards);
    return KBO_OK;
}

const kbo_index_t *kbo_index_shard(const kbo_index_t *idx, int i)
{
    if (!idx || i < 0) return nullptr;
    if (!idx->sharded()) return i == 0 ? idx : nullptr;
    return (size_t)i < idx->shards.size() ? idx->shards[(size_t)i].get() : nullptr;
}

int kbo_set_plan_stats(int on)
{
    g_plan_stats = on != 0;
    return KBO_OK;
}

int kbo_set_plan_table_budget(uint64_t bytes)
{
    g_plan_table_budget = bytes;
    return KBO_OK;
}

int kbo_set_plan_lazy(int64_t bases)
{
    g_plan_lazy_bases = bases < 0 ? -1 : bases;
    return KBO_OK;
}

int kbo_set_depth_table(int order)
{
    g_depth_table = order < 0 ? -1 : std::min(order, 17);
    return KBO_OK;
}

int kbo_set_depth_table_anchors(int mode)
{
    g_depth_table_anchors = mode < 0 ? -1 : (mode != 0 ? 1 : 0);
    return KBO_OK;
}

int kbo_set_seed_table_depth(int bases)
{
    g_seed_table_depth = std::max(0, std::min(bases, 14));
    return KBO_OK;
}

int kbo_index_plan_holdoff(kbo_index_t *idx, int device, uint32_t *bails, int *holdoff)
{
    return guarded([&] {
        KBO_REQUIRE(idx, KBO_E_BAD_ARG, "null index");
        require_unsharded(idx, "kbo_index_plan_holdoff");
        std::lock_guard<std::mutex> g(idx->mu);
        const DevCopy &dc = copy_on(idx, device);
        if (bails) *bails = dc.plan.bails.load();
        if (holdoff) *holdoff = dc.plan.holdoff.load();
    });
}

// test hook (kbo_hip_tuning.h): the rank blocks, contraction entries and two-base blocks of the copy on `device` (made on the device:
// layout_kernels.hip) against the host's make_device_layout -> *n_diff = bytes that differ (0: the same layout)
int kbo_index_layout_check(kbo_index_t *idx, int device, uint64_t *n_diff)
{
    return guarded([&] {
        KBO_REQUIRE(idx && n_diff, KBO_E_BAD_ARG, "null argument");
        require_unsharded(idx, "kbo_index_layout_check");
        std::lock_guard<std::mutex> g(idx->mu);
        const DevCopy &dc = copy_on(idx, device);
        kbo::DeviceLayout lay;
        kbo::make_device_layout(idx->host, lay, dc.pair_off != 0);
        KBO_REQUIRE(lay.n_blocks == dc.n_blocks, KBO_E_BAD_ARG, "block counts differ");
        const size_t per = lay.n_blocks * 16, ent_bytes = lay.ent.size() * 4, pair_bytes = lay.pair.size() * 4;
        uint64_t diff = 0;
        auto compare = [&](const void *d_ptr, const void *h_ptr, size_t bytes) {
            std::vector<uint8_t> got(bytes);
            HIP_OK(hipMemcpy(got.data(), d_ptr, bytes, hipMemcpyDeviceToHost));
            const uint8_t *want = static_cast<const uint8_t *>(h_ptr);
            for (size_t i = 0; i < bytes; i++) diff += got[i] != want[i];
        };
        for (int c = 0; c < 4; c++) compare(dc.arena.as<uint8_t>() + per * c, lay.rank[c].data(), per);
        compare(dc.big ? dc.ent.as<uint8_t>() : dc.arena.as<uint8_t>() + per * 4 + 16, lay.ent.data(), ent_bytes);
        if (dc.pair_off) compare(dc.arena.as<uint8_t>() + (size_t)dc.pair_off * 16, lay.pair.data(), pair_bytes);
        *n_diff = diff;
    });
}

// test hook (kbo_hip_tuning.h): the handle's path cover (laid out on the device when its first copy made it: cover_kernels.hip) against
// the host's make_path_cover -> *n_diff = positions of text / pos / node_at that differ (0: the same layout); KBO_E_BAD_ARG without a cover
int kbo_index_cover_check(kbo_index_t *idx, uint64_t *n_diff)
{
    return guarded([&] {
        KBO_REQUIRE(idx && n_diff, KBO_E_BAD_ARG, "null argument");
        require_unsharded(idx, "kbo_index_cover_check");
        std::lock_guard<std::mutex> g(idx->mu);
        KBO_REQUIRE((bool)idx->cover, KBO_E_BAD_ARG, "the handle has no path cover yet (kbo_index_to_device makes it)");
        kbo::PathCover want;
        kbo::make_path_cover(idx->host, want);
        const kbo::PathCover &got = *idx->cover;
        KBO_REQUIRE(got.text.size() == want.text.size() && got.pos.size() == want.pos.size() && got.node_at.size() == want.node_at.size(),
                    KBO_E_BAD_ARG, "sizes differ");
        uint64_t diff = 0;
        for (size_t i = 0; i < want.text.size(); i++) diff += got.text[i] != want.text[i];
        for (size_t i = 0; i < want.pos.size(); i++) diff += (got.pos[i] != want.pos[i]) + (got.node_at[i] != want.node_at[i]);
        *n_diff = diff;
    });
}

int kbo_set_force_big_layout(int on)
{
    g_force_big = on != 0; // applies to device copies made after the call
    return KBO_OK;
}

int kbo_set_host_in_place(int on)
{
    g_host_in_place = on != 0;
    return KBO_OK;
}

int kbo_set_walk_rare(int period)
{
    kbo::set_walk_rare(period);
    return KBO_OK;
}

int kbo_set_walk_threads(int threads)
{
    kbo::set_walk_threads(threads);
    return KBO_OK;
}

int kbo_set_guided_walk(int waves_per_cu, int recovery_lines)
{
    kbo::set_guided_walk(waves_per_cu, recovery_lines);
    return KBO_OK;
}

int kbo_set_walk_waves_per_cu(int waves_per_cu)
{
    g_waves_per_cu = waves_per_cu > 0 ? waves_per_cu : 0;
    return KBO_OK;
}

uint64_t kbo_last_batch_staged_bytes(void) { return t_last_staged; }

// test hook (kbo_hip_tuning.h): the router of the slab pipeline's derandomize + translate stage over host MS bytes of any content
int kbo_derand_translate_host(const uint8_t *ms, const uint64_t *offsets, size_t n_seqs, size_t k, size_t threshold, const uint8_t *ref,
                              uint8_t *chars_out)
{
    return guarded([&] {
        KBO_REQUIRE(ms && offsets && chars_out, KBO_E_BAD_ARG, "null argument");
        KBO_REQUIRE(n_seqs > 0 && n_seqs < 0xFFFFFFFFull, KBO_E_EMPTY_QUERY, "empty batch");
        KBO_REQUIRE(k > 0 && k <= 255, KBO_E_BAD_ARG, "k in 1..255");
        KBO_REQUIRE(threshold > 1, KBO_E_THRESHOLD_LE_1, "threshold > 1 (derandomize.rs:275)");
        KBO_REQUIRE(offsets[0] == 0, KBO_E_BAD_ARG, "offsets[0] == 0");
        for (size_t s = 0; s < n_seqs; s++) KBO_REQUIRE(offsets[s] <= offsets[s + 1], KBO_E_BAD_ARG, "offsets ascend");
        const uint64_t total = offsets[n_seqs];
        KBO_REQUIRE(total > 0 && total + 16 <= (1ull << 32), KBO_E_UNSUPPORTED, "an empty batch, or one of 2^32 - 16 bases or more");
        hipStream_t stream = nullptr;
        const size_t bytes = (size_t)total + 16; // what kbo_derand_translate_dev documents for its per-base buffers
        DevBuf dms(bytes), doff((n_seqs + 1) * sizeof(uint64_t)), dch(bytes), dref, piece;
        HIP_OK(hipMemsetAsync(dms.p, 0, bytes, stream));
        HIP_OK(hipMemsetAsync(dch.p, 0, bytes, stream));
        HIP_OK(hipMemcpyAsync(dms.p, ms, total, hipMemcpyHostToDevice, stream));
        HIP_OK(hipMemcpyAsync(doff.p, offsets, (n_seqs + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, stream));
        if (ref) {
            dref.alloc(bytes);
            HIP_OK(hipMemsetAsync(dref.p, 0, bytes, stream));
            HIP_OK(hipMemcpyAsync(dref.p, ref, total, hipMemcpyHostToDevice, stream));
        }
        derand_translate_host_offsets(dms.as<uint8_t>(), doff.as<uint64_t>(), offsets, n_seqs, (uint32_t)k,
                                      (uint32_t)std::min<size_t>(threshold, 0x7FFFFFFF), ref ? dref.as<uint8_t>() : nullptr,
                                      dch.as<uint8_t>(), nullptr, stream, 0, &piece);
        HIP_OK(hipMemcpyAsync(chars_out, dch.p, total, hipMemcpyDeviceToHost, stream));
        HIP_OK(hipStreamSynchronize(stream));
    });
}

} // extern "C"
