// rle_seg_host.cpp — kbo_run_lengths_seq_host (kbo_hip_tuning.h): the passes of rle_seg_kernels.hip restated on the CPU over
// rle_seg.hpp's algebra, with the chunk and the group of any size, so that every boundary case is a few bytes long.  No HIP call.
#include "../../include/kbo_hip_tuning.h"
#include "rle_seg.hpp"

#include <algorithm>
#include <vector>

using namespace kbo::rleseg;

namespace {

struct Chunk {
    uint64_t byte0;      // first byte in the batch
    uint32_t p0, n, len; // first position in its sequence, positions, the sequence's length
};
struct Group {
    size_t c0, nc; // its chunks
};

// the walk of one chunk, as the count and the emit kernels make it
template <typename Close>
Part walk_chunk(const uint8_t *aln, const Chunk &c, uint32_t gap, const Dash &dash_in, const Part &part_in, Close &&close)
{
    const uint8_t *row = aln + c.byte0;
    Walk w = walk_begin(dash_in, part_in);
    bool broke = false;
    for (uint32_t q = 0; q < c.n; q++) {
        const uint32_t i = c.p0 + q;
        walk_step(w, row[q], i > 0 ? row[(int64_t)q - 1] : 0u, i + 1u < c.len ? row[q + 1u] : 0u, i, c.len, gap, broke, close);
    }
    return walk_end(w, broke);
}

} // namespace

extern "C" int kbo_run_lengths_seq_host(const uint8_t *aln, const uint64_t *offsets, size_t n_seqs, size_t max_gap_len, size_t chunk,
                                        size_t group, size_t min_len, uint32_t *records, size_t capacity, uint32_t *first)
{
    if (!offsets || !first || (!records && capacity) || n_seqs == 0 || chunk == 0 || group == 0 || group % chunk != 0 ||
        chunk > 0xFFFFFFFFull)
        return KBO_E_BAD_ARG;
    if ((!aln && offsets[n_seqs] > offsets[0]) || offsets[n_seqs] - offsets[0] >= (1ull << 32)) return KBO_E_BAD_ARG;
    const uint32_t gap = (uint32_t)std::min<size_t>(max_gap_len, 0xFFFFFFFFu);
    const size_t gchunks = group / chunk;
    // the lists: chunks and groups, neither spanning two sequences; a sequence below min_len has none
    std::vector<Chunk> chunks;
    std::vector<Group> groups;
    std::vector<size_t> seq_c0(n_seqs + 1), seq_g0(n_seqs + 1);
    for (size_t s = 0; s < n_seqs; s++) {
        seq_c0[s] = chunks.size();
        seq_g0[s] = groups.size();
        const uint64_t len = offsets[s + 1] - offsets[s];
        if (len < min_len) continue;
        for (uint64_t p = 0; p < len; p += chunk) {
            if ((chunks.size() - seq_c0[s]) % gchunks == 0) groups.push_back(Group{chunks.size(), 0});
            chunks.push_back(Chunk{offsets[s] + p, (uint32_t)p, (uint32_t)std::min<uint64_t>(chunk, len - p), (uint32_t)len});
            groups.back().nc++;
        }
    }
    seq_c0[n_seqs] = chunks.size();
    seq_g0[n_seqs] = groups.size();
    const size_t nc = chunks.size(), ng = groups.size();
    // two levels, the same for both carries: summaries of the chunks, of the groups; one pass per sequence over its groups leaves
    // what enters each group where its summary was; one pass per group over its chunks does the same a level down
    auto carry = [&](auto &csum, auto &gsum, auto identity, auto combine) {
        for (size_t g = 0; g < ng; g++) {
            auto acc = identity();
            for (size_t c = groups[g].c0; c < groups[g].c0 + groups[g].nc; c++) acc = combine(acc, csum[c]);
            gsum[g] = acc;
        }
        for (size_t s = 0; s < n_seqs; s++) {
            auto state = identity();
            for (size_t g = seq_g0[s]; g < seq_g0[s + 1]; g++) {
                const auto own = gsum[g];
                gsum[g] = state;
                state = combine(state, own);
            }
        }
        for (size_t g = 0; g < ng; g++) {
            auto state = gsum[g];
            for (size_t c = groups[g].c0; c < groups[g].c0 + groups[g].nc; c++) {
                const auto own = csum[c];
                csum[c] = state;
                state = combine(state, own);
            }
        }
    };
    std::vector<Dash> cdash(nc), gdash(ng);
    for (size_t c = 0; c < nc; c++) {
        const uint8_t *row = aln + chunks[c].byte0;
        cdash[c] = dash_summary([&](uint32_t q) { return (uint32_t)row[q]; }, chunks[c].n);
    }
    carry(cdash, gdash, dash_identity, dash_combine);
    std::vector<Part> cpart(nc), gpart(ng);
    std::vector<uint32_t> count(nc + 1, 0);
    for (size_t c = 0; c < nc; c++) {
        uint32_t n = 0;
        cpart[c] = walk_chunk(aln, chunks[c], gap, cdash[c], part_identity(), [&](const Rec &) { n++; });
        count[c] = n;
    }
    carry(cpart, gpart, part_identity, part_combine);
    uint32_t run = 0;
    for (size_t c = 0; c <= nc; c++) { // exclusive scan; a sequence's first run is its first chunk's
        const uint32_t v = count[c];
        count[c] = run;
        run += v;
    }
    for (size_t s = 0; s <= n_seqs; s++) first[s] = count[seq_c0[s]];
    for (size_t c = 0; c < nc; c++) {
        uint32_t slot = count[c];
        walk_chunk(aln, chunks[c], gap, cdash[c], cpart[c], [&](const Rec &r) {
            if (slot < capacity) {
                const uint32_t rec[7] = {r.start, r.end, r.matches, r.mismatches, r.jumps, r.gap_bases, r.gap_opens};
                std::copy(rec, rec + 7, records + (size_t)slot * 7u);
            }
            slot++;
        });
    }
    return KBO_OK;
}

// every sequence of the batch as a batch of ONE, in a buffer of exactly its length (nothing in front of it and nothing behind);
// records and first as the batch call gives them
extern "C" int kbo_run_lengths_seq_host_each(const uint8_t *aln, const uint64_t *offsets, size_t n_seqs, size_t max_gap_len, size_t chunk,
                                             size_t group, size_t min_len, uint32_t *records, size_t capacity, uint32_t *first)
{
    if (!offsets || !first || (!records && capacity) || n_seqs == 0) return KBO_E_BAD_ARG;
    size_t run = 0;
    for (size_t s = 0; s < n_seqs; s++) {
        if (offsets[s + 1] < offsets[s] || (!aln && offsets[s + 1] > offsets[s])) return KBO_E_BAD_ARG;
        const std::vector<uint8_t> own(aln + offsets[s], aln + offsets[s + 1]);
        const uint64_t off[2] = {0, own.size()};
        uint32_t f[2] = {0, 0};
        const size_t room = capacity > run ? capacity - run : 0;
        const int rc = kbo_run_lengths_seq_host(own.empty() ? nullptr : own.data(), off, 1, max_gap_len, chunk, group, min_len,
                                                room ? records + run * 7u : nullptr, room, f);
        if (rc != KBO_OK) return rc;
        first[s] = (uint32_t)run;
        run += f[1];
    }
    first[n_seqs] = (uint32_t)run;
    return KBO_OK;
}
