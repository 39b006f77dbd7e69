/*
 * kbo_hip.h — C ABI of the MI355X-native k-bounded matching-statistics path of kbo.
 *
 * This is the drop-in boundary: every entry point below is what a binding of the
 * reference crate (tmaklin/kbo v0.5.1, Rust) would call instead of its CPU path.
 * Each declaration cites the reference interface it replaces (file:line under the
 * reference's src/).  Plain pointers and sizes only; no C++ or torch types.
 *
 * Conventions
 *   - return 0 (KBO_OK) or a negative KBO_E_* code; each code mirrors one of the
 *     reference's assert!/panic! sites.  kbo_last_error() gives a thread-local text.
 *   - the caller owns all in/out buffers; the index handle is immutable after
 *     construction, so concurrent calls on one handle are allowed.
 *   - "host" entry points take host pointers and do H2D/D2H themselves;
 *     "*_dev" entry points take pointers that are already resident in the HBM of
 *     the current HIP device plus a hipStream_t (passed as void*), enqueue their
 *     kernels on that stream and return without synchronising.
 *   - ALL matching-statistics work runs in the HIP kernels (gfx950).  There is no
 *     CPU fallback: without a usable GPU the compute entry points fail with KBO_E_HIP.
 */
#ifndef KBO_HIP_H
#define KBO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KBO_OK 0
#define KBO_E_EMPTY_QUERY (-1)    /* index.rs:248   assert!(!query.is_empty())          */
#define KBO_E_LEN_LE_2 (-2)       /* derandomize.rs:276, translate.rs:270  len > 2      */
#define KBO_E_THRESHOLD_LE_1 (-3) /* derandomize.rs:275, translate.rs:269  threshold > 1*/
#define KBO_E_BAD_ARG (-4)        /* derandomize.rs:96-97,133-137,274; null/invalid arg */
#define KBO_E_NOMEM (-5)
#define KBO_E_K_MISMATCH (-6)     /* lib.rs:559,729  k of index != k of opts            */
#define KBO_E_HIP (-7)            /* HIP runtime error / no device / kernel image missing */
#define KBO_E_UNSUPPORTED (-8)    /* valid in the reference, not (yet) built here        */
#define KBO_E_MS_RANGE (-9)       /* derandomize.rs:229-230  noisy/derand value > k     */
#define KBO_E_IO (-10)            /* index.rs:137,202 file open/read/write failure      */
#define KBO_E_REF_PANIC (-11)     /* the reference would panic here (index/usize underflow, assert!) */

const char *kbo_last_error(void);
const char *kbo_version(void);

/* ------------------------------------------------------------------ options */

/* kbo::BuildOpts (lib.rs:259-313).  Only k and add_revcomp change the index content;
 * the remaining fields steer the sbwt crate's construction algorithm and are accepted
 * for signature compatibility (num_threads is honoured by this builder too). */
typedef struct {
    uint32_t k;              /* 31    */
    int32_t add_revcomp;     /* false */
    uint32_t num_threads;    /* 1     */
    uint32_t prefix_precalc; /* 8     */
    int32_t build_select;    /* false */
    uint32_t mem_gb;         /* 4     */
    int32_t dedup_batches;   /* false */
    const char *temp_dir;    /* NULL  */
} kbo_build_opts;
void kbo_build_opts_default(kbo_build_opts *o); /* lib.rs:300-313 */

/* kbo::FindOpts (lib.rs:358-382) */
typedef struct {
    double max_error_prob; /* 1e-7 */
    size_t max_gap_len;    /* 0    */
} kbo_find_opts;
void kbo_find_opts_default(kbo_find_opts *o);

/* kbo::MapOpts (lib.rs:412-466).  fill_gaps / call_variants select the host-side
 * refinement stages that follow the hot path (lib.rs:743-754). */
typedef struct {
    double max_error_prob; /* 1e-7 */
    int32_t fill_gaps;     /* true */
    int32_t call_variants; /* true */
    int32_t format;        /* true */
    kbo_build_opts sbwt_build_opts; /* build_select = true */
} kbo_map_opts;
void kbo_map_opts_default(kbo_map_opts *o);

/* kbo::CallOpts (lib.rs:318-353) */
typedef struct {
    double max_error_prob;          /* 1e-7 */
    kbo_build_opts sbwt_build_opts; /* build_select = true */
} kbo_call_opts;
void kbo_call_opts_default(kbo_call_opts *o);

/* kbo::variant_calling::Variant (variant_calling.rs:8-26).  Arrays returned by kbo_call live
 * in one allocation: release the whole result with a single kbo_free(variants). */
typedef struct {
    uint64_t query_pos;
    const uint8_t *query_chars;
    size_t query_len;
    const uint8_t *ref_chars;
    size_t ref_len;
} kbo_variant;

/* kbo::format::RLE (format.rs:18-33) */
typedef struct {
    uint64_t start, end, matches, mismatches, jumps, gap_bases, gap_opens;
} kbo_rle;

/* ------------------------------------------------------------------ index
 * Opaque stand-in for (sbwt::SbwtIndexVariant, sbwt::LcsArray) — the pair returned by
 * kbo::build (lib.rs:501-506) and consumed by every query function.  Owns the host
 * copy and one device-resident copy per GPU it has been used on. */
typedef struct kbo_index kbo_index_t;

/* kbo::build / index::build_sbwt_from_vecs (lib.rs:501-506, index.rs:56-99). */
int kbo_index_build(const uint8_t *const *seqs, const size_t *lens, size_t n_seqs,
                    const kbo_build_opts *opts, kbo_index_t **out);

/* kbo::build on HIP device `device` (-1 = current): the same index as kbo_index_build(seqs, lens, n_seqs, opts) - equal
 * k, n_kmers, n_sets, C, subset-matrix rows and LCS - built by the device, with that device's copy made from the rows
 * the device built (no host -> device copy of rows or LCS); the host copy is filled too (export / save / host stages).
 * The copy equals what kbo_index_to_device(idx, device) makes of a host-built handle.  The current device is unchanged
 * on return; num_threads is accepted and ignored.  Errors: those of kbo_index_build (checked before any HIP call),
 * KBO_E_UNSUPPORTED for an input kbo_index_build would build as shards (kbo_index_build builds those), KBO_E_NOMEM when
 * the build's peak does not fit the device's free memory: (32 W + 8) bytes per base and strand (W = 1 / 2 / 4 / 8 key
 * words for k <= 32 / 64 / 128 / 255; e.g. 72 bytes per base at k = 63 without add_revcomp) + 1 byte per base. */
int kbo_index_build_device(const uint8_t *const *seqs, const size_t *lens, size_t n_seqs,
                           const kbo_build_opts *opts, int device, kbo_index_t **out);

/* Adopt an index built elsewhere (e.g. by the sbwt crate on the Rust side): the four
 * SubsetMatrix rows as little-endian 64-bit words (bit i of word i/64 = row i), the C
 * array and the LCS array as bytes.  Replaces handing &SbwtIndexVariant/&LcsArray to
 * index::query_sbwt (index.rs:243-247). */
int kbo_index_from_parts(uint32_t k, uint64_t n_sets, uint64_t n_kmers,
                         const uint64_t *const rows[4], const uint64_t C[4],
                         const uint8_t *lcs, kbo_index_t **out);
/* Inverse of the above; rows[c] must hold ceil(n_sets/64) words, lcs n_sets bytes. */
int kbo_index_export_parts(const kbo_index_t *idx, uint64_t *const rows[4], uint64_t C[4],
                           uint8_t *lcs);
void kbo_index_free(kbo_index_t *idx);

size_t kbo_index_k(const kbo_index_t *idx);         /* SbwtIndex::k()       lib.rs:620 */
uint64_t kbo_index_n_kmers(const kbo_index_t *idx); /* SbwtIndex::n_kmers() lib.rs:620 */
uint64_t kbo_index_n_sets(const kbo_index_t *idx);  /* SbwtIndex::n_sets()             */

/* index::serialize_sbwt / load_sbwt (index.rs:128-151, 195-212) — own flat,
 * device-ready file format "<prefix>.kbohip" (NOT the sbwt crate's .sbwt/.lcs).  While the plan-guided walk is enabled
 * (default) the file also carries the index's path cover (9 bytes per row; computed by the save if the handle has none
 * yet): laying it out is the one slow, serial part of making a device copy (26 s per 10^8 rows), so a loaded index uploads
 * in the time of a few streaming passes.  A cover read from a file is validated against the subset matrix (KBO_E_IO). */
int kbo_index_save(const kbo_index_t *idx, const char *path);
int kbo_index_load(const char *path, kbo_index_t **out);
/* index::serialize_sbwt / load_sbwt (index.rs:128-151, 195-212).  The reference writes <prefix>.sbwt + <prefix>.lcs: a
 * u64-LE length and the tag "SubsetMatrix" (index.rs:139-140), then the sbwt crate's own serialize() payload, which
 * nothing in the reference tree pins: PARITY UNPINNED.  These functions therefore keep their
 * own payload (pinned header + second tag "KBOSBWT1") under their OWN names, <prefix>.sbwt.kbohip + <prefix>.lcs.kbohip,
 * so that kbo-cli never mistakes the pair for a crate-written index; kbo_index_load_sbwt reads that pair and returns
 * KBO_E_UNSUPPORTED (not a guess at the crate's fields) when all it finds is a crate-written <prefix>.sbwt: such an index
 * comes in through kbo_index_from_parts (INTEGRATION.md has the Rust side).  KBO_E_IO when a file is missing, truncated
 * or inconsistent. */
int kbo_index_save_sbwt(const kbo_index_t *idx, const char *prefix);
int kbo_index_load_sbwt(const char *prefix, kbo_index_t **out);

/* Sharded indexes.  Row numbers are 32 bits on the device, so an index of 2^32 rows or more - a human genome WITH its reverse
 * complements, 6.2 * 10^9 rows - cannot be one index here.  kbo_index_build builds such an input as SHARDS: ordinary indexes
 * over groups of whole sequences, the forward and the reverse-complement strand of every group apart.  The strings (of at
 * most k characters) that are suffixes of an SBWT's rows are the substrings of its input's ACGT-runs of at least k characters
 * - a property of the sequences one by one - so the DEPTH of the walk against the index of everything is the maximum of the
 * depths against the shards, and n_kmers (what the threshold of the derandomisation needs) is counted over the union.
 * Everything that only needs depths therefore gives the union index's results, bit for bit, by walking every shard:
 * kbo_matches[_batch][_packed], kbo_map[_batch] without fill_gaps / call_variants, kbo_find[_batch][_packed], kbo_ms_batch /
 * kbo_matching_statistics without intervals, and the device-resident entry points (d_work: kbo_index_work_bytes).  What needs
 * ROWS of the union - intervals, kbo_call*, kbo_fill_gaps, full kbo_map, export / save, the path-cover getters - returns
 * KBO_E_UNSUPPORTED for such a handle.  kbo_index_shards: 1 for an ordinary index; kbo_index_n_sets counts the rows of all
 * shards. */
int kbo_index_shards(const kbo_index_t *idx);

/* Upload (idempotent) the device layout to HIP device `device` (-1 = current). */
int kbo_index_to_device(kbo_index_t *idx, int device);
/* Bytes of the device-resident layout: rank blocks / contraction entries {lcs,psv,nsv}. */
int kbo_index_device_bytes(const kbo_index_t *idx, uint64_t *rank_bytes, uint64_t *lcs_bytes);
/* bytes of two-base extension blocks a device copy of this index carries (0 = none, see kbo_set_pair_steps) */
uint64_t kbo_index_device_pair_bytes(const kbo_index_t *idx);
/* What the copy of `idx` on `device` (-1 = current) holds and what making it cost - the index is built once and queried many
 * times (index.rs:56-99 is not part of any query), but the plan structures are sized by log4(rows), not by the index, so a
 * caller that serves few queries per index wants to see the bill.  Bytes by part; entries_64bit = the contraction entries sit
 * in their own allocation behind 64-bit offsets (rank blocks + entries >= 4 GiB); seconds of host work + upload by part
 * (cover: laying out the path cover, 0 when the handle had one already - from an index file or an earlier copy).
 * KBO_E_BAD_ARG when there is no such copy, KBO_E_UNSUPPORTED for a sharded handle (ask its shards). */
typedef struct {
    uint64_t rank_bytes, entry_bytes, pair_bytes;                           /* what every walk needs */
    uint64_t cover_bytes, lines_bytes, seed_bytes, dtab_bytes, anchor_bytes; /* the plan structures (0: the copy has none) */
    uint32_t entries_64bit, seed_depth, dtab_order, dtab_grouped;
    double layout_seconds, upload_seconds, cover_seconds, lines_seconds, seed_seconds, dtab_seconds;
} kbo_device_layout;
int kbo_index_device_layout(kbo_index_t *idx, int device, kbo_device_layout *out);

/* ------------------------------------------------------------------ A3 (host, f64)
 * derandomize::log_rm_max_cdf (derandomize.rs:91-100) and
 * derandomize::random_match_threshold (derandomize.rs:127-145). */
int kbo_log_rm_max_cdf(size_t t, size_t alphabet_size, size_t n_kmers, double *out);
int kbo_random_match_threshold(size_t k, size_t n_kmers, size_t alphabet_size,
                               double max_error_prob, size_t *out);

/* ------------------------------------------------------------------ single-sequence
 * parity entry points with the reference's element widths (host pointers). */

/* index::query_sbwt -> Vec<(usize, Range<usize>)> (index.rs:243-256).
 * d/lo/hi each hold len elements; lo/hi may both be NULL. */
int kbo_matching_statistics(kbo_index_t *idx, const uint8_t *query, size_t len, uint64_t *d,
                            uint64_t *lo, uint64_t *hi);
/* derandomize::derandomize_ms_vec (derandomize.rs:269-288). */
int kbo_derandomize_ms_vec(const uint64_t *noisy_ms, size_t len, size_t k, size_t threshold,
                           int64_t *out);
/* derandomize::derandomize_ms_val (derandomize.rs:221-247) — scalar, host. */
int kbo_derandomize_ms_val(size_t curr_noisy_ms, int64_t next_derand_ms, size_t threshold,
                           size_t k, int64_t *out);
/* translate::translate_ms_vec (translate.rs:263-293); chars as Rust `char` (u32). */
int kbo_translate_ms_vec(const int64_t *derand_ms, size_t len, size_t k, size_t threshold,
                         uint32_t *out);
/* translate::translate_ms_val (translate.rs:180-216) — scalar, host. */
int kbo_translate_ms_val(int64_t ms_curr, int64_t ms_next, int64_t ms_prev, size_t threshold,
                         uint32_t *aln_curr, uint32_t *aln_next);
/* kbo::matches (lib.rs:612-628): chars as Rust `char` (u32), len elements. */
int kbo_matches(kbo_index_t *idx, const uint8_t *query, size_t len, double max_error_prob,
                uint32_t *chars_out);
/* kbo::map (lib.rs:720-761): out holds len bytes. */
int kbo_map(kbo_index_t *query_idx, const uint8_t *ref_seq, size_t len, const kbo_map_opts *opts,
            uint8_t *out);
/* kbo::call (lib.rs:547-573): builds an index of ref_seq, runs variant_calling::call_variants
 * (variant_calling.rs:249-294; all MS passes on the GPU, k-mer walks of the sites batched). */
int kbo_call(kbo_index_t *query_idx, const uint8_t *ref_seq, size_t len, const kbo_call_opts *opts,
             kbo_variant **out, size_t *n_out);
/* kbo::call over a batch: every sequence of (concat, offsets) plays ref_seq against the same query index.  The first
 * pass of call_variants (MS walk + the breakpoint scan, variant_calling.rs:266-273) runs on the device for the whole
 * batch and only the sites come back; the second pass walks all query-side k-mers in one batch and, per sequence, the
 * reference-side k-mers against that sequence's own index (lib.rs:553).  *out holds var_offsets[n_seqs] variants, those
 * of sequence s at [var_offsets[s], var_offsets[s+1]); one allocation, kbo_free(*out).  opts->sbwt_build_opts.k must
 * equal the index's k (lib.rs:559). */
int kbo_call_batch(kbo_index_t *query_idx, const uint8_t *concat, const uint64_t *offsets, size_t n_seqs,
                   const kbo_call_opts *opts, kbo_variant **out, uint64_t *var_offsets /* n_seqs + 1 */);
/* The same with the variants as flat arrays in the order of (sequence, query position) - the form they leave the device in
 * (call_emit_kernels.hip: the device sorts a slab's sites, runs resolve_variant's case analysis, variant_calling.rs:139-201, and slices
 * the characters; 10 bytes per variant cross PCIe instead of 164 per site): no record with two pointers per variant to fill, nothing for
 * a binding to copy.  Variant v of sequence s (v in [var_offsets[s], var_offsets[s + 1])) has query_pos[v], query_len[v] query characters
 * followed by ref_len[v] reference characters in `chars`, the variants' characters back to back in variant order.  Released by
 * kbo_call_flat_free(result).  kbo_call_batch is this + the reference's records made from it. */
typedef struct {
    uint64_t n_variants, n_chars;
    uint32_t *query_pos;
    uint16_t *query_len, *ref_len;
    uint8_t *chars;
} kbo_call_flat;
int kbo_call_batch_flat(kbo_index_t *query_idx, const uint8_t *concat, const uint64_t *offsets, size_t n_seqs,
                        const kbo_call_opts *opts, kbo_call_flat *result, uint64_t *var_offsets /* n_seqs + 1 */);
void kbo_call_flat_free(kbo_call_flat *result);
/* The first pass of call_variants in one go, device-resident: the walk of kbo_ms_batch_dev (MS values to d_ms_out, no
 * intervals) whose lanes run the breakpoint scan on the values they produce.  Sites are 16-byte records {offset of i in
 * d_concat, offset of j, row of ms[j], 0} in KBO_CALL_LISTS lists as below; d_count needs KBO_CALL_LISTS * 64 + 64 bytes:
 * the last counter is non-zero when some read had more than four breakpoints waiting within k bases - then (and when a
 * list overflowed) use kbo_ms_batch_dev with intervals + kbo_call_sites_dev instead.  A record whose first word is
 * 0xFFFFFFFF is void and to be skipped (plan-guided walk: a site of a read that was afterwards scanned again in full,
 * where the same site appears once more).  Asynchronous on `stream`. */
int kbo_call_walk_dev(kbo_index_t *idx, const uint8_t *d_concat, const uint64_t *d_offsets, size_t n_seqs,
                      uint64_t total_bases, size_t max_seq_len, size_t threshold, uint8_t *d_ms_out, void *d_sites,
                      size_t capacity, uint32_t *d_count, void *d_work, size_t work_bytes, void *stream);
/* The breakpoint scan alone, device-resident: d_ms / d_lo / d_hi as kbo_ms_batch_dev wrote them (intervals requested).
 * Sites are 16-byte records {sequence, i, j, row of ms[j]} in KBO_CALL_LISTS lists (one counter would serialise the
 * appends): list g occupies d_sites[g * (capacity / KBO_CALL_LISTS) ...] and has d_count[16 g] records, in arrival
 * order; d_count is KBO_CALL_LISTS counters 64 bytes apart (16 KiB).  A counter above capacity / KBO_CALL_LISTS means
 * that list overflowed: repeat with more room.  Asynchronous on `stream`. */
#define KBO_CALL_LISTS 256
int kbo_call_sites_dev(const uint8_t *d_ms, const uint32_t *d_lo, const uint32_t *d_hi, const uint64_t *d_offsets,
                       size_t n_seqs, uint64_t total_bases, size_t k, size_t threshold, void *d_sites, size_t capacity,
                       uint32_t *d_count, void *stream);
/* translate::add_variants (translate.rs:350-386) on Rust-char (u32) alignment strings, in place. */
int kbo_add_variants(uint32_t *translation, size_t len, const kbo_variant *variants, size_t n_variants);
/* gap_filling::fill_gaps (gap_filling.rs:444-526) preceded by the steps its callers run
 * (lib.rs:735-747): query_sbwt, derandomize_ms_vec and translate_ms_vec with the GIVEN threshold
 * on the GPU, then the host-side gap filling.  out holds len Rust chars. */
int kbo_fill_gaps(kbo_index_t *query_idx, const uint8_t *ref_seq, size_t len, size_t threshold,
                  double max_err_prob, uint32_t *out);
/* gap_filling::nearest_unique_context (gap_filling.rs:127-151): kmer_out holds k bytes;
 * *kmer_len is 0 when no unique interval was found. */
int kbo_nearest_unique_context(kbo_index_t *idx, const uint8_t *ref_seq, size_t len, size_t range_start,
                               size_t range_end, size_t *kmer_idx, uint8_t *kmer_out, size_t *kmer_len);
/* kbo::find (lib.rs:808-821): *out is allocated by the library (kbo_free). */
int kbo_find(kbo_index_t *idx, const uint8_t *query, size_t len, const kbo_find_opts *opts,
             kbo_rle **out, size_t *n_out);
/* format::run_lengths_gapped (format.rs:143-193) and relative_to_ref (format.rs:266-287)
 * on byte-wide alignment strings (host; sequential variable-length output).  KBO_E_REF_PANIC for an alignment that starts
 * with 'R': the reference evaluates aln[i - 1] with i = 0 there (format.rs:175) and panics; translate_ms_vec never produces
 * one (an 'R' needs a derandomised value above the threshold, the first base's is at most 1), so the pipeline's entry points
 * cannot run into it. */
int kbo_run_lengths_gapped(const uint8_t *aln, size_t len, size_t max_gap_len, kbo_rle **out,
                           size_t *n_out);
/* format::run_lengths_gapped over a batch of alignments on the GPU (one lane per alignment): runs of
 * all sequences concatenated, rle_offsets[i]..[i+1] = alignment i (n_seqs+1 entries, caller-allocated;
 * *rles library-allocated, release with kbo_free).  Same records as kbo_run_lengths_gapped. */
int kbo_run_lengths_gapped_batch(const uint8_t *aln_concat, const uint64_t *offsets, size_t n_seqs,
                                 size_t max_gap_len, kbo_rle **rles, uint64_t *rle_offsets);
int kbo_relative_to_ref(const uint8_t *ref_seq, const uint8_t *aln, size_t len, uint8_t *out);
void kbo_free(void *p);

/* ------------------------------------------------------------------ batched entry points
 * (new surface: the reference takes ONE sequence per call, lib.rs:612-617; batching over
 * reads/contigs lives in kbo-cli).  `concat` holds all sequences back to back,
 * offsets[i]..offsets[i+1] delimits sequence i (n_seqs+1 entries).  Compact element
 * widths: d as u8 (d <= k <= 255), intervals as u32 (n_sets < 2^32), chars as u8. */
int kbo_ms_batch(kbo_index_t *idx, const uint8_t *concat, const uint64_t *offsets, size_t n_seqs,
                 uint8_t *d_out, uint32_t *lo_out, uint32_t *hi_out);
int kbo_matches_batch(kbo_index_t *idx, const uint8_t *concat, const uint64_t *offsets,
                      size_t n_seqs, double max_error_prob, uint8_t *chars_out);
/* map with fill_gaps=false, call_variants=false (lib.rs:735-738, 756-760) over a batch. */
int kbo_map_batch(kbo_index_t *idx, const uint8_t *concat, const uint64_t *offsets, size_t n_seqs,
                  double max_error_prob, int format, uint8_t *out);
/* kbo::map (lib.rs:720-761) with any MapOpts over a batch: out[offsets[s] .. offsets[s+1]) is what kbo_map(idx, seq s, opts)
 * writes.  status[s] (n_seqs entries) = 0, or the KBO_E_* code kbo_map returns for sequence s alone (its bytes of `out` are
 * then unspecified).  Whole-call errors (null args, KBO_E_K_MISMATCH, KBO_E_THRESHOLD_LE_1, sharded index -> KBO_E_UNSUPPORTED
 * as kbo_map) are returned as the call's code.  Gap filling runs on the device (a sequence the device cannot finish is redone
 * on the host), the variants of the whole batch come from kbo_call_batch_flat's passes. */
int kbo_map_batch_opts(kbo_index_t *idx, const uint8_t *concat, const uint64_t *offsets, size_t n_seqs,
                       const kbo_map_opts *opts, uint8_t *out, int32_t *status);
/* gap_filling::fill_gaps over a batch, as kbo_fill_gaps per sequence (same threshold argument); out holds u8 characters. */
int kbo_fill_gaps_batch(kbo_index_t *idx, const uint8_t *concat, const uint64_t *offsets, size_t n_seqs,
                        size_t threshold, double max_err_prob, uint8_t *out, int32_t *status);
/* find over a batch: RLEs of all sequences concatenated, rle_offsets[i]..[i+1] = sequence i
 * (rle_offsets has n_seqs+1 entries, caller-allocated; *rles library-allocated, kbo_free).  The
 * run lengths are computed on the device (the translated characters never leave it). */
int kbo_find_batch(kbo_index_t *idx, const uint8_t *concat, const uint64_t *offsets, size_t n_seqs,
                   const kbo_find_opts *opts, kbo_rle **rles, uint64_t *rle_offsets);
/* The same into caller-owned memory (buffers reused from call to call cost no page faults): `rles`
 * holds `capacity` records; *n_runs receives the number of runs of the batch.  When that exceeds
 * `capacity` the call fails with KBO_E_NOMEM after filling rle_offsets and *n_runs (records beyond
 * the capacity are not written), so a second call with a large enough buffer succeeds. */
int kbo_find_batch_into(kbo_index_t *idx, const uint8_t *concat, const uint64_t *offsets, size_t n_seqs,
                        const kbo_find_opts *opts, kbo_rle *rles, size_t capacity, uint64_t *rle_offsets,
                        size_t *n_runs);

/* ------------------------------------------------------------------ packed batches
 * The batch entry points above move one byte per base over PCIe in each direction, which is what bounds them (about
 * 40 Gbp/s host -> host against 140 Gbp/s on the device).  Reads carry 2 bits per base and the alphabet of kbo::matches is
 * exactly { M, -, X, R } (translate.rs:180-216), so these entry points take and return 2-bit words: a quarter of the bytes,
 * the same kernels in between (the words are unpacked and packed on the device).
 * Layout, input and output alike: sequence s of len_s bases occupies ceil(len_s / 16) little-endian u32 words, the
 * sequences back to back in order (kbo_packed_words() in all); base i of a sequence sits in bits 2 (i mod 16), + 1 of its
 * word i / 16.  Input: A, C, G, T = 0 .. 3; every other byte of the reads (N, lower case, ...: they break matches like in
 * the reference) travels in a side list { position in base coordinates (offsets[] space), byte }, positions ascending,
 * and the 2 bits at such a position are ignored.  Output: M, -, X, R = 0 .. 3.
 * offsets[] counts BASES as everywhere else (n_seqs + 1 entries).  kbo_pack_reads / kbo_unpack_matches are host helpers
 * (threaded) for callers that hold bytes; KBO_E_NOMEM from kbo_pack_reads when the reads hold more than exc_cap
 * non-ACGT bases (*n_exc is set to their number). */
size_t kbo_packed_words(const uint64_t *offsets, size_t n_seqs);
int kbo_pack_reads(const uint8_t *concat, const uint64_t *offsets, size_t n_seqs, uint32_t *words_out, uint64_t *exc_pos,
                   uint8_t *exc_byte, size_t exc_cap, size_t *n_exc);
int kbo_unpack_matches(const uint32_t *words, const uint64_t *offsets, size_t n_seqs, uint8_t *chars_out);
/* kbo::matches (lib.rs:612-628) over a packed batch */
int kbo_matches_batch_packed(kbo_index_t *idx, const uint32_t *words, const uint64_t *offsets, size_t n_seqs,
                             const uint64_t *exc_pos, const uint8_t *exc_byte, size_t n_exc, double max_error_prob,
                             uint32_t *words_out);
/* kbo::find (lib.rs:808-821) over a packed batch.  The run lengths come back as the seven u32 the device writes (the fields of
 * format::RLE, format.rs:18-33; a sequence is shorter than 2^32 bases): 28 bytes per run instead of kbo_rle's 56, and no
 * widening pass on the host - at about 1.15 runs per 150-base read the records are as many bytes as the packed alignments
 * themselves.  *rles is library-allocated (kbo_free); rle_offsets as for kbo_find_batch. */
typedef struct {
    uint32_t start, end, matches, mismatches, jumps, gap_bases, gap_opens;
} kbo_rle32;
int kbo_find_batch_packed(kbo_index_t *idx, const uint32_t *words, const uint64_t *offsets, size_t n_seqs,
                          const uint64_t *exc_pos, const uint8_t *exc_byte, size_t n_exc, const kbo_find_opts *opts,
                          kbo_rle32 **rles, uint64_t *rle_offsets);
/* kbo::matches over a packed batch in its SPARSE form: only the runs of characters other than 'M'.  A run is a maximal stretch
 * of one character other than 'M' inside one sequence's kbo::matches output (never across sequences; "-X" is two runs).
 * Records are ordered by (seq, start); a sequence without one is all 'M', and one of fewer than 3 bases (no alignment) has
 * none.  12 bytes a run and nothing per sequence: at 1 % substitutions a small fraction of the dense words' bytes.  Lossless:
 * kbo_sparse_expand rebuilds kbo_matches_batch's characters, and with the reads kbo_map_batch(..., format = 1)'s
 * (format::relative_to_ref, format.rs:266-287).  Inputs, checks and error codes are kbo_matches_batch_packed's; sequences must
 * be shorter than 2^30 bases (KBO_E_UNSUPPORTED).  *runs is library-allocated (kbo_free), *n_runs records. */
typedef struct {
    uint32_t seq;      /* index of the sequence in the batch (0 .. n_seqs-1) */
    uint32_t start;    /* first position of the run within that sequence (0-based) */
    uint32_t len_code; /* (length << 2) | code; code as in the packed alphabet: 1 = '-', 2 = 'X', 3 = 'R' (0 = 'M' never occurs) */
} kbo_aln_run;
int kbo_matches_batch_sparse(kbo_index_t *idx, const uint32_t *words, const uint64_t *offsets, size_t n_seqs,
                             const uint64_t *exc_pos, const uint8_t *exc_byte, size_t n_exc, double max_error_prob,
                             kbo_aln_run **runs, uint64_t *n_runs);
/* Host helper (threaded): sparse records -> one byte per base, offsets[n_seqs] bytes at `out`.  ref_concat == NULL: kbo::matches'
 * characters (M - X R, what kbo_matches_batch returns); ref_concat = the reads: format::relative_to_ref of them (the read's base for
 * 'M' and 'R', '-' for 'X' and '-': what kbo_map_batch(..., format = 1) returns).  KBO_E_BAD_ARG for records out of (seq, start)
 * order, overlapping, of length 0, with code 0 or outside their sequence. */
int kbo_sparse_expand(const kbo_aln_run *runs, uint64_t n_runs, const uint64_t *offsets, size_t n_seqs, const uint8_t *ref_concat,
                      uint8_t *out);

/* ------------------------------------------------------------------ per-sequence alignment summaries
 * Read screening, decontamination, presence / absence and identity / coverage tables reduce kbo::matches' characters to a few
 * counts per sequence; these entry points do that on the device, and 16 bytes per sequence leave it instead of a character (or two
 * bits) per base.  The record of one sequence describes the characters kbo_matches_batch returns for it: n_match, n_mismatch and
 * n_jump are its numbers of 'M', 'X' and 'R'; n_runs is the number of maximal stretches without '-' (what kbo_find_batch counts
 * with max_gap_len = 0); the number of '-' is len - (n_match + n_mismatch + n_jump).  A sequence of fewer than 3 bases has no
 * alignment (the reference asserts, derandomize.rs:274-276): the device-resident entry points give it an all-zero record, the host
 * entry points refuse the batch as kbo_matches_batch does.  Both strands: kbo_revcomp_batch_dev / kbo_revcomp_packed_dev, then a
 * summary of each.  There is no relative_to_ref form: the summary is of kbo::matches' characters. */
typedef struct {
    uint32_t n_match, n_mismatch, n_jump, n_runs;
} kbo_aln_summary; /* 16 bytes */
/* The same counts with the extent of the alignment, of the characters c = translate_ms_vec(derandomize_ms_vec(ms, k, t), k, t) of one
 * sequence: start is the 0-based position of the first character other than '-', end one past the last such character, both 0 when
 * there is none.  A sequence of fewer than 3 bases gets an all-zero record.  What kbo_derand_summary_seq_dev writes and
 * kbo_summary_refset returns per pair. */
typedef struct {
    uint32_t n_match, n_mismatch, n_jump, n_runs, start, end;
} kbo_aln_extent; /* 24 bytes */
/* kbo_matches_batch / kbo_matches_batch_packed with the records as output: summary_out holds n_seqs records (the caller's; the library
 * allocates nothing).  Inputs, checks and error codes are those of kbo_matches_batch / kbo_matches_batch_packed; the same slab
 * pipeline, over the devices of kbo_set_devices and over sharded indexes alike; a slab downloads 16 bytes per sequence.  A slab of reads
 * (at most 160 bases, a copy with a depth table) goes through map_reads_kernel's summary form - bytes in, or the words as they are - and
 * makes no character at all; any other slab keeps its characters on the device and a reducer counts them there. */
int kbo_summary_batch(kbo_index_t *idx, const uint8_t *concat, const uint64_t *offsets, size_t n_seqs, double max_error_prob,
                      kbo_aln_summary *summary_out);
int kbo_summary_batch_packed(kbo_index_t *idx, const uint32_t *words, const uint64_t *offsets, size_t n_seqs, const uint64_t *exc_pos,
                             const uint8_t *exc_byte, size_t n_exc, double max_error_prob, kbo_aln_summary *summary_out);

/* ------------------------------------------------------------------ both strands
 * A read comes from either strand of what the index was built of, a gene lies on either strand of an assembly.  Instead of an
 * index built with add_revcomp (twice the rows and plan structures; a human-scale index then has 2^32 rows or more and becomes
 * a sharded one, see above) or a second call with sequences the host has reverse-complemented (every base crosses PCIe twice),
 * these entry points compare every sequence AND its reverse complement with the index as it is.  The batch is staged to the
 * device ONCE; the '-' strand is made there (kbo_amd/csrc/revcomp_kernels.hip).
 * Reverse complement, per sequence and never across a boundary: output base i = complement of input base len - 1 - i;
 * A <-> T, C <-> G, a <-> t, c <-> g, every other byte unchanged (N stays N and breaks matches as ever).
 * strands: KBO_STRAND_FWD, KBO_STRAND_REV or both (3); 0 or anything else -> KBO_E_BAD_ARG.  The '-' result of sequence s is
 * exactly what the single-strand entry point returns for revcomp(sequence s), and it is IN THE COORDINATES OF THE
 * REVERSE-COMPLEMENTED SEQUENCE: position i of a '-' output (a character, a run's start / end) is base len - 1 - i of the
 * sequence as given.  Errors, limits and the behaviour for sharded indexes are the single-strand entry point's; the output of a
 * strand that is not asked for may be NULL and is not touched. */
#define KBO_STRAND_FWD 1
#define KBO_STRAND_REV 2
/* host helper (threaded): out[offsets[s] .. offsets[s+1]) = revcomp(sequence s).  Sequences may be empty.  KBO_E_BAD_ARG for
 * null arguments, offsets that do not ascend from 0, and an `out` that overlaps `concat`. */
int kbo_revcomp_batch(const uint8_t *concat, const uint64_t *offsets, size_t n_seqs, uint8_t *out);
/* kbo_matches_batch (format = 0) / kbo_map_batch (format != 0: format::relative_to_ref of the '-' strand takes the
 * reverse-complemented read) per strand; out_fwd / out_rev hold offsets[n_seqs] bytes each. */
int kbo_matches_batch_strands(kbo_index_t *idx, const uint8_t *concat, const uint64_t *offsets, size_t n_seqs, double max_error_prob,
                              int format, int strands, uint8_t *out_fwd, uint8_t *out_rev);
/* kbo_find_batch per strand: rle_offsets has 2 * n_seqs + 1 entries (caller-allocated); the runs of sequence s are
 * [rle_offsets[2 s], rle_offsets[2 s + 1]) for '+' and [rle_offsets[2 s + 1], rle_offsets[2 s + 2]) for '-'; a strand that is
 * not asked for has none.  *rles is library-allocated (kbo_free). */
int kbo_find_batch_strands(kbo_index_t *idx, const uint8_t *concat, const uint64_t *offsets, size_t n_seqs, const kbo_find_opts *opts,
                           int strands, kbo_rle **rles, uint64_t *rle_offsets);
/* the same over the packed input of kbo_matches_batch_packed / kbo_find_batch_packed; words_fwd / words_rev hold
 * kbo_packed_words() words each, with kbo_matches_batch_packed's conventions (M - X R = 0 .. 3; kbo_unpack_matches) */
int kbo_matches_batch_packed_strands(kbo_index_t *idx, const uint32_t *words, const uint64_t *offsets, size_t n_seqs, const uint64_t *exc_pos,
                                     const uint8_t *exc_byte, size_t n_exc, double max_error_prob, int strands, uint32_t *words_fwd,
                                     uint32_t *words_rev);
int kbo_find_batch_packed_strands(kbo_index_t *idx, const uint32_t *words, const uint64_t *offsets, size_t n_seqs, const uint64_t *exc_pos,
                                  const uint8_t *exc_byte, size_t n_exc, const kbo_find_opts *opts, int strands, kbo_rle32 **rles,
                                  uint64_t *rle_offsets);
/* The reverse complement of a device-resident batch, enqueued on `stream` (a hipStream_t); the library never synchronises.
 * Alignment and SLACK as for the device-resident path below: d_concat 16-byte aligned with 16 readable bytes behind its last
 * base, d_offsets 8-byte, d_out 4-byte aligned.  Exactly [d_out, d_out + total_bases) is written - d_out needs no slack of its own
 * for this call.  Sequences may be empty; max_seq_len (0 = unknown) is accepted for symmetry and changes nothing: the work is cut
 * by 4 KiB of output, so millions of reads and a handful of Mbp contigs fill the device alike.  KBO_E_BAD_ARG for null or
 * misaligned arguments and for a d_out that overlaps the input, KBO_E_UNSUPPORTED for total_bases + 16 > 2^32. */
int kbo_revcomp_batch_dev(const uint8_t *d_concat, const uint64_t *d_offsets, size_t n_seqs, uint64_t total_bases, size_t max_seq_len,
                          uint8_t *d_out, void *stream);
/* ... of a device-resident PACKED batch (the layout of kbo_matches_batch_packed; total_words = kbo_packed_words()): a
 * sequence's words reversed in 2-bit groups, complemented and shifted by (16 - len mod 16) mod 16 groups across word boundaries,
 * the padding bits of its last word zero; the exception list mirrored within each sequence (p -> offsets[s] + offsets[s+1] - 1 - p,
 * the byte complemented) and ascending again.  The 2 bits at a listed position are unspecified, as on input.  d_scratch:
 * kbo_revcomp_packed_scratch_bytes(n_seqs) bytes, 16-byte aligned (0 from it: too many sequences for one launch).  No output may
 * overlap its input (KBO_E_BAD_ARG). */
size_t kbo_revcomp_packed_scratch_bytes(size_t n_seqs);
int kbo_revcomp_packed_dev(const uint32_t *d_words, const uint64_t *d_offsets, size_t n_seqs, uint64_t total_words, const uint64_t *d_exc_pos,
                           const uint8_t *d_exc_byte, size_t n_exc, uint32_t *d_words_out, uint64_t *d_exc_pos_out, uint8_t *d_exc_byte_out,
                           void *d_scratch, void *stream);

/* ------------------------------------------------------------------ find against a set of references
 * kbo::find over a file of reference sequences - a resistance-gene or virulence-factor database: hundreds to thousands of sequences
 * of 0.3 - 5 kbp - is one index PER REFERENCE in the reference crate (kbo::build on that one sequence, lib.rs:501-506; kbo::find for
 * every (reference, query contig) pair, lib.rs:808-821), and no single index of all of them gives the same runs: the derandomisation
 * threshold comes from each index's own n_kmers (derandomize.rs:127-145), and the matching statistics against the union are the
 * maximum over the references.  A kbo_refset_t is N such indexes - index r exactly what kbo_index_build of sequence r alone builds:
 * the same rows, C, LCS, n_kmers and k - in ONE packed device layout without plan structures (2 bytes a row), and kbo_find_refset
 * queries all of them in one call: the query batch is uploaded once, its '-' strand is made on the device, and a kernel that keeps a
 * whole reference in a compute unit's LDS walks (reference, query chunk) pairs (kbo_amd/csrc/refset_kernels.hip).  A reference of
 * more than 16 384 rows does not fit that form; the set keeps an ordinary index handle for it and the call takes it through the
 * single-index pipeline, one such reference at a time, with the same results (kbo_refset_build_wide, below, keeps references of up
 * to 2^20 rows in the packed layout instead).
 * A reference without a k-mer - shorter than k, or without a run of k bases A, C, G, T - cannot be queried (kbo_find on its own
 * handle fails in random_match_threshold, derandomize.rs:134); the set still builds, kbo_refset_status says so (KBO_E_BAD_ARG, the
 * code that call returns) and the reference contributes no runs.  Whole-call errors of the build (null arguments, n_refs == 0, k
 * outside 1 .. 255) are kbo_index_build's, checked before any HIP call; opts->num_threads threads build the references. */
typedef struct kbo_refset kbo_refset_t;
int kbo_refset_build(const uint8_t *const *seqs, const size_t *lens, size_t n_refs, const kbo_build_opts *opts, kbo_refset_t **out);
void kbo_refset_free(kbo_refset_t *set);
size_t kbo_refset_size(const kbo_refset_t *set);                /* N */
size_t kbo_refset_k(const kbo_refset_t *set);
uint64_t kbo_refset_n_kmers(const kbo_refset_t *set, size_t r); /* 0 for r >= N */
int kbo_refset_status(const kbo_refset_t *set, size_t r);       /* 0, or the KBO_E_* of building / querying r alone */
int kbo_refset_to_device(kbo_refset_t *set, int device);        /* idempotent, -1 = current */
/* The same set with references of more than 16 384 rows kept in the packed layout too.  kbo_refset_build_wide behaves as
 * kbo_refset_build does, with one difference in routing: a reference of more than KBO_REFSET_MAX_ROWS (16 384) and at most
 * max_wide_rows rows keeps its packed form - the same 2 bytes a row - in the set's arena and takes the WIDE route: a kernel that reads
 * the form from memory where the LDS kernel reads it from LDS (kbo_amd/csrc/refset_wide_kernels.hip), in the same slabs as the small
 * references.  It gets no index handle and no plan structures.  A reference of at most KBO_REFSET_MAX_ROWS rows keeps the LDS route, one of
 * more than max_wide_rows rows the single-index route.  max_wide_rows must lie in [KBO_REFSET_MAX_ROWS, KBO_REFSET_WIDE_MAX_ROWS]
 * (KBO_E_BAD_ARG otherwise, checked before any work); max_wide_rows == KBO_REFSET_MAX_ROWS gives exactly kbo_refset_build's set.
 * The cap is 2^20 rows because the form is then 2 MiB, half of one XCD's 4 MiB L2: the workgroups of a reference's tasks re-read it
 * from L2 while the query and the MS bytes stream through the other half; above it the single-index pipeline with its plan
 * structures is the tool.  A contraction scans LCS bytes linearly, as in the LDS form: a reference that is mostly one long repeat
 * makes the walk slow, never wrong.  That, and that the route is measured on one workload only, is why it is chosen per set and kbo_refset_build
 * does not take it.  Results do not depend on the route: fields, order, '-' strand coordinates and the thresholds from each
 * reference's own n_kmers are the same. */
#define KBO_REFSET_WIDE_MAX_ROWS (1u << 20)
#define KBO_REFSET_ROUTE_NONE (-1)   /* the reference has a status */
#define KBO_REFSET_ROUTE_LDS 0
#define KBO_REFSET_ROUTE_INDEX 1     /* the single-index pipeline */
#define KBO_REFSET_ROUTE_WIDE 2      /* packed form, walked from memory */
int kbo_refset_build_wide(const uint8_t *const *seqs, const size_t *lens, size_t n_refs, const kbo_build_opts *opts, size_t max_wide_rows,
                          kbo_refset_t **out);
int kbo_refset_route(const kbo_refset_t *set, size_t r);   /* KBO_REFSET_ROUTE_*; KBO_E_BAD_ARG for r >= N or a null set */
int kbo_refset_packed_only(const kbo_refset_t *set);       /* 1: no reference takes the single-index route */
/* A set with a PREFILTER: an opt-in screen of the (reference, sequence, strand) pairs by shared seeds, for the packed routes (LDS
 * and wide).  More than 99 % of the pairs of a gene database against an assembly produce nothing, and the walk of all of them is the
 * cost of a call; the screen is exact.  From derandomize_ms_vec (derandomize.rs:221-247, 282-285) and translate_ms_val
 * (translate.rs:190-213): when no noisy matching statistic of a sequence is > threshold or == k, every derandomised value is below 1
 * and every character '-' - the pair has no run and no summary record.  So a pair can have a record only if, with t_r the threshold
 * of reference r at this call's max_error_prob and w_r = min(t_r + 1, k), some w_r consecutive bases of the sequence on that strand
 * occur in an indexed stretch of r.  The screen tests that with m_r = min(w_r, KBO_REFSET_SEED_MAX) bases.
 * kbo_refset_build_opts(..., refset_opts, out) with refset_opts->prefilter = 0 is exactly kbo_refset_build_wide(max_wide_rows); with
 * prefilter = 1 the set also carries a seed table, made on the host while the sequences are at hand: one entry for every start
 * position of every indexed stretch - a maximal run of A, C, G, T of at least k bases, and its reverse complement when
 * opts->add_revcomp is set - of every reference of a packed route that can be queried.  An entry holds the 2-bit code of the next
 * KBO_REFSET_SEED_MAX bases (fewer at the stretch's end, and then how many) and the reference; entries are sorted by code, and an
 * array of 4^KBO_REFSET_SEED_MIN + 1 offsets addresses them by their first KBO_REFSET_SEED_MIN bases.  Entries carry their reference
 * and their length, so one table serves every max_error_prob.  12 bytes an entry + 16 MiB (kbo_refset_prefilter_bytes);
 * kbo_refset_to_device uploads it with the arena.  References of the single-index route and references with a status have no entries.
 *   KBO_REFSET_SEED_MAX = 24: the default thresholds (max_error_prob 1e-7) are 15 .. 18 for references of 0.3 .. 16 kbp and reach 21
 *     at 2^20 rows, so m_r = w_r there; a stricter max_error_prob than the cap covers is screened with 24 bases - weaker, never
 *     wrong.  The figure is reasoning, not measurement.
 *   KBO_REFSET_SEED_MIN = 11: a reference with m_r below it cannot be screened at that max_error_prob - all its pairs are candidates
 *     - so it should not exceed the m_r in use (max_error_prob 1e-4 gives m_r = 11 for a reference of 300 bases), and the offsets should stay
 *     small against the 256 MiB Infinity Cache next to the entries: 16 MiB, where 12 bases would take 64 MiB and buy a bucket a
 *     quarter as long - 0.5 entries a look-up instead of 0.12 for 2 x 10^6 entries, either of which is one cache line.
 * kbo_find_refset, kbo_summary_refset and kbo_best_refset on such a set run ONE more kernel behind the upload
 * (kbo_amd/csrc/refset_screen_kernels.hip) that marks the pairs sharing a seed of m_r bases, read the bitmap back (one more copy and
 * one more synchronisation per call), and plan, upload and walk only the marked pairs.  Records are byte-identical with and without
 * the prefilter.  References of the single-index route go through their pipeline unscreened.  A call whose bitmap would exceed 2^31
 * bits (n_refs x n_seqs x 2) runs unscreened, with the same records.  kbo_best_refset's merge kernel finds a slab's pairs by
 * arithmetic and cannot skip any: on a set with a prefilter the call runs kbo_summary_refset's slabs over the candidate pairs -
 * their per-slab waits come back - and folds the kept records into the table on the host, by the merge of refset_best.hpp; the table
 * is the same.  The device forms (kbo_*_refset_dev) IGNORE the prefilter: they plan on the device from closed forms over all pairs;
 * kbo_*_refset_screened_dev, below them, plan from the bitmap.
 * kbo_refset_candidates runs the screen alone: bits_out receives ceil(n_refs x n_seqs x 2 / 32) words, bit
 * (r x n_seqs + s) x 2 + (strand - 1); *n_candidates (may be NULL) the bits set.  For a reference that can be screened the bit is 1 if
 * and only if sequence s on that strand holds m_r consecutive bytes that lie within the sequence, are all bases and occur as m_r
 * consecutive bases of an indexed stretch of r - so every pair with a record has its bit set; a reference that cannot be screened at
 * this max_error_prob has the bits of all its pairs set.  Bits of strands not asked for, and of references without entries, are 0.
 * Errors: those of kbo_summary_refset; KBO_E_BAD_ARG for a set without a prefilter; KBO_E_UNSUPPORTED above 2^31 bits. */
#define KBO_REFSET_SEED_MAX 24
#define KBO_REFSET_SEED_MIN 11
typedef struct {
    size_t max_wide_rows; /* KBO_REFSET_MAX_ROWS: as kbo_refset_build; up to KBO_REFSET_WIDE_MAX_ROWS: as kbo_refset_build_wide */
    int32_t prefilter;    /* 0 */
    int32_t positions;    /* 0; 1: the set also carries a position table ("the locus of a run", below).  In what was tail padding:
                           * sizeof(kbo_refset_opts) is unchanged */
} kbo_refset_opts;
void kbo_refset_opts_default(kbo_refset_opts *o);
int kbo_refset_build_opts(const uint8_t *const *seqs, const size_t *lens, size_t n_refs, const kbo_build_opts *opts,
                          const kbo_refset_opts *refset_opts, kbo_refset_t **out);
int kbo_refset_has_prefilter(const kbo_refset_t *set);        /* 1 or 0 */
uint64_t kbo_refset_prefilter_bytes(const kbo_refset_t *set); /* the seed table's bytes; 0 without one */
int kbo_refset_candidates(kbo_refset_t *set, const uint8_t *concat, const uint64_t *offsets, size_t n_seqs, double max_error_prob,
                          int strands, uint32_t *bits_out, uint64_t *n_candidates);
/* The records with (ref = r, seq = s, strand) are, in order, exactly the runs kbo_find returns for sequence s - strand
 * KBO_STRAND_REV: for its reverse complement, in the coordinates of the reverse-complemented sequence as for kbo_find_batch_strands -
 * against reference r's own index: derandomised with the threshold of that index's n_kmers and opts->max_error_prob, run lengths
 * with opts->max_gap_len.  Records are ordered by (ref, seq, strand with '+' first, start); a pair without a hit has no record, and
 * there is no cap on their number.  *runs is library-allocated (kbo_free), *n_runs records.  Only runs leave the device.
 * Errors, all checked before the first HIP call: strands outside 1 .. 3 and null arguments KBO_E_BAD_ARG, offsets as for
 * kbo_find_batch_strands, a sequence of fewer than 3 bases refuses the batch with KBO_E_LEN_LE_2, KBO_E_THRESHOLD_LE_1 when some
 * reference's threshold is (kbo_find on its handle fails so), KBO_E_UNSUPPORTED for a batch of 2^31 bases or more. */
typedef struct {
    uint32_t ref, seq, strand; /* strand: KBO_STRAND_FWD or KBO_STRAND_REV */
    kbo_rle32 run;
} kbo_ref_run; /* 40 bytes */
int kbo_find_refset(kbo_refset_t *set, const uint8_t *concat, const uint64_t *offsets, size_t n_seqs, const kbo_find_opts *opts,
                    int strands, kbo_ref_run **runs, uint64_t *n_runs);
/* The summary of the same pairs: which references are present, on which strand, with what identity and coverage - one record per
 * (reference, sequence, strand) pair whose alignment holds at least one character other than '-', a pair without a hit has none.
 * aln (kbo_aln_extent, above) describes kbo::matches of sequence s - strand KBO_STRAND_REV: of its reverse complement, in the
 * coordinates of the reverse-complemented sequence - against reference r's own index, with the threshold of that index's n_kmers and
 * max_error_prob: the pairs, thresholds and coordinates of kbo_find_refset, and aln.n_runs is the number of records
 * kbo_find_refset(max_gap_len = 0) has for the pair.  Records are ordered by (ref, seq, strand with '+' first).  *records is
 * library-allocated (kbo_free); *n_records == 0 leaves it NULL.  The slabs, the upload, the '-' strand and the walk are
 * kbo_find_refset's; behind the walk a slab runs kbo_derand_summary_seq_dev's stage with the pairs' thresholds and keeps the records
 * with n_runs > 0 on the device, in pair order: one count and the kept records leave the device per slab - no character buffer, no
 * run-length stage.  A reference of more than KBO_REFSET_MAX_ROWS rows goes through the single-index pipeline, whose characters are
 * counted on the host.  Errors, all checked before the first HIP call: those of kbo_find_refset, max_error_prob as
 * opts->max_error_prob there.  References with a status set contribute nothing.  kbo_refset_last_routes reports this call's routes
 * as it does kbo_find_refset's. */
typedef struct {
    uint32_t ref, seq, strand; /* strand: KBO_STRAND_FWD or KBO_STRAND_REV */
    kbo_aln_extent aln;
} kbo_ref_summary; /* 36 bytes */
int kbo_summary_refset(kbo_refset_t *set, const uint8_t *concat, const uint64_t *offsets, size_t n_seqs, double max_error_prob,
                       int strands, kbo_ref_summary **records, uint64_t *n_records);
/* The two calls for a batch that is already in the HBM of the current device: the same records, in the same order, written to the
 * caller's device buffer; everything is enqueued on `stream` (a hipStream_t) and the call returns.  No hipStreamSynchronize, no
 * device-to-host copy, no allocation: all scratch is d_work, and the one host-to-device upload of a call is the references' thresholds
 * (n_refs uint32_t - only the host can compute them, from n_kmers and max_error_prob).  Launches: 6 a call (7 with the '-' strand, and
 * a device-to-device copy of the batch when both strands are asked for) + 34 a slab (find) or 22 a slab (summary), whatever the batch
 * holds; one more for a slab that holds both LDS and wide references (a walk kernel each).
 * Inputs: the set has a copy on the current device (kbo_refset_to_device; KBO_E_BAD_ARG when it has none); d_concat holds
 * total_bases + 16 readable bytes and is 16-byte aligned; d_offsets holds n_seqs + 1 uint64_t on the device, 8-byte aligned, ascending
 * from 0 to total_bases, which the caller knows: nothing about the batch is read back, so nothing about it is checked.
 * Records: exactly those kbo_find_refset / kbo_summary_refset return for the same set, batch, options and strands - fields, the
 * coordinates of the '-' strand and the order (ref, seq, strand with '+' first, start) - from d_runs[0] / d_records[0] on (4-byte
 * aligned).  *d_n_runs / *d_n_records (on the device, 8-byte aligned; the call writes it and does not require it to be zero) receives
 * the number of records, those beyond `capacity` included: they are counted and not written, nothing is written at or behind element
 * `capacity`, and the output pointer may be NULL when capacity == 0.
 * A sequence of fewer than 3 bases, an empty one included, contributes no record and disturbs no other pair: the device form cannot
 * refuse the batch with KBO_E_LEN_LE_2 as the host form does, because it does not know the lengths.  A reference with a status
 * contributes nothing, as there.  A set that holds a reference of the single-index route (more than KBO_REFSET_MAX_ROWS rows in a set of
 * kbo_refset_build, more than max_wide_rows in one of kbo_refset_build_wide) is refused with KBO_E_UNSUPPORTED - that route is a host
 * pipeline; kbo_refset_packed_only() is 1 when the set holds none, else 0, and the *_work_bytes of a refused set are 0.  Wide references
 * lie in the slabs next to LDS ones and need no scratch of their own: the figures do not depend on the routes.  kbo_refset_lds_only()
 * is 1 when every reference that can be queried takes the LDS route.
 * Slabs: a slab is a range of consecutive queryable references against the WHOLE batch on the strands asked for, refs x n_strands x
 * total_bases bytes, planned on the device (kbo_amd/csrc/refset_plan_kernels.hip).  *_work_bytes(..., refs_per_slab) is the exact figure
 * for slabs of that many references - 0: as many as one slab may hold (all queryable ones unless 2^32 - 16 bytes or 2^28 pairs come
 * first), larger values count as that - and grows with refs_per_slab and with capacity; 0 for arguments the call refuses.  The call
 * uses the largest refs_per_slab whose figure fits work_bytes and touches no byte of d_work (16-byte aligned) behind that figure.
 * d_work holds, per call, the '-' strand of the batch (behind a copy of the '+' strand when both are asked for: the walk addresses one
 * buffer), the chunks of every sequence with their scan, the thresholds and the list of the queryable references; per slab, pair
 * offsets and thresholds, the walk's items and tasks, the MS bytes, the characters (find), the scratch of
 * kbo_derand_translate_seq_dev's stage - for the lowest threshold there is, 2: the figure does not know max_error_prob - and of
 * kbo_run_lengths_seq_dev's (find) or the extents and the kept list (summary), and a slab-local buffer of min(capacity, the most runs
 * a slab can have) seven-word records (find).
 * Errors, all before anything is enqueued: KBO_E_BAD_ARG for null arguments, misaligned ones, strands outside 1 .. 3, a max_error_prob
 * outside (0, 1] and a work_bytes below the figure for one reference a slab; KBO_E_EMPTY_QUERY for n_seqs == 0; KBO_E_THRESHOLD_LE_1 as
 * the host calls; KBO_E_UNSUPPORTED for a reference of the single-index route, a slab of one reference of 2^32 - 16 bytes or more, and
 * n_seqs x n_strands >= 2^28.  kbo_refset_last_routes is not touched by these calls. */
int kbo_refset_lds_only(const kbo_refset_t *set);
size_t kbo_find_refset_dev_work_bytes(const kbo_refset_t *set, size_t n_seqs, uint64_t total_bases, int strands, size_t capacity,
                                      size_t refs_per_slab);
int kbo_find_refset_dev(kbo_refset_t *set, const uint8_t *d_concat, const uint64_t *d_offsets, size_t n_seqs, uint64_t total_bases,
                        const kbo_find_opts *opts, int strands, void *d_work, size_t work_bytes, kbo_ref_run *d_runs, size_t capacity,
                        uint64_t *d_n_runs, void *stream);
size_t kbo_summary_refset_dev_work_bytes(const kbo_refset_t *set, size_t n_seqs, uint64_t total_bases, int strands, size_t capacity,
                                         size_t refs_per_slab);
int kbo_summary_refset_dev(kbo_refset_t *set, const uint8_t *d_concat, const uint64_t *d_offsets, size_t n_seqs, uint64_t total_bases,
                           double max_error_prob, int strands, void *d_work, size_t work_bytes, kbo_ref_summary *d_records, size_t capacity,
                           uint64_t *d_n_records, void *stream);
/* Which reference does each sequence belong to, and how clear is that choice: ONE record per query sequence, always, in sequence
 * order (seq == its index) - typing a contig against an allele database, assigning a plasmid to its closest relative, binning reads by
 * gene.  It is the reduction over references of kbo_summary_refset's pairs, made on the device: n_seqs records leave it per call where
 * the summary sends up to N x n_seqs x 2.
 * A pair (ref, strand) of a sequence has a HIT when its aln.n_runs > 0 - the pairs kbo_summary_refset has a record for.  Pairs with a
 * hit are ordered by: larger aln.n_match first, then smaller ref, then '+' (KBO_STRAND_FWD) before '-'.
 *   ref, strand, aln         the first pair in that order, aln as kbo_summary_refset's record of it has it ('-': in the coordinates
 *                            of the reverse-complemented sequence)
 *   n_hits                   the pairs of this sequence with a hit (kbo_summary_refset's records with this seq)
 *   second_ref, second_match ref and aln.n_match of the first pair in that order among the pairs of ANOTHER reference than ref: the
 *                            runner-up; the winner's own other strand is never it
 * A sequence without a hit: ref = second_ref = KBO_REF_NONE, strand = 0, aln and the counts 0.  Only one reference hit: second_ref =
 * KBO_REF_NONE, second_match = 0.  second_match == aln.n_match says that another reference ties (two identical references: the lower
 * one is ref, the other second_ref).
 * kbo_best_refset: *out is library-allocated (kbo_free), n_seqs records.  The slabs, the upload, the '-' strand, the walk and the
 * summary stage are kbo_summary_refset's; behind them a slab runs ONE kernel that merges its extents into a table of n_seqs records on
 * the device (kbo_amd/csrc/refset_best_kernels.hip) - no compaction, no record stage, nothing read back and nothing waited for per
 * slab; the table comes back in one copy behind the last slab, the call's one synchronisation.  References of the single-index route
 * go through that pipeline as in kbo_summary_refset and are merged into the table on the host, by the same merge
 * (kbo_amd/csrc/refset_best.hpp).  Errors, all checked before the first HIP call: those of kbo_summary_refset, and KBO_E_UNSUPPORTED
 * for 2^28 sequences or more.  References with a status contribute nothing.  kbo_refset_last_routes / kbo_refset_last_wide report this
 * call as they do the summary's.
 * kbo_best_refset_dev: kbo_summary_refset_dev's contract - the set is kbo_refset_packed_only() and has a copy on the current device,
 * the inputs, alignments and slack of the batch, d_work (16-byte aligned) of kbo_best_refset_dev_work_bytes(..., refs_per_slab) bytes
 * with the same meaning of refs_per_slab, everything enqueued on `stream`, nothing synchronised, read back or allocated, the same
 * errors before anything is enqueued.  d_out (4-byte aligned, n_seqs records) IS the running table: the call sets it to the empty
 * records and every slab merges into it, so it is complete when the stream reaches the end of the call; there is no capacity and no
 * count.  Sequences of fewer than 3 bases get the record without a hit (the host form refuses the batch, as kbo_summary_refset does).
 * Launches: 7 a call (8 with the '-' strand, and the device-to-device copy when both strands are asked for) - the summary form's 6 and
 * the table's fill - + 17 a slab where the summary form has 22: its compaction (4) and its record append (2) are not launched, the merge (1) is;
 * one more for a slab with both LDS and wide references.  d_work holds what kbo_summary_refset_dev's does without the scan and the kept
 * list. */
#define KBO_REF_NONE 0xFFFFFFFFu
typedef struct {
    uint32_t seq, ref, strand; /* strand: KBO_STRAND_FWD or KBO_STRAND_REV; 0 without a hit */
    kbo_aln_extent aln;
    uint32_t n_hits, second_ref, second_match;
} kbo_ref_best; /* 48 bytes */
int kbo_best_refset(kbo_refset_t *set, const uint8_t *concat, const uint64_t *offsets, size_t n_seqs, double max_error_prob, int strands,
                    kbo_ref_best **out);
size_t kbo_best_refset_dev_work_bytes(const kbo_refset_t *set, size_t n_seqs, uint64_t total_bases, int strands, size_t refs_per_slab);
int kbo_best_refset_dev(kbo_refset_t *set, const uint8_t *d_concat, const uint64_t *d_offsets, size_t n_seqs, uint64_t total_bases,
                        double max_error_prob, int strands, void *d_work, size_t work_bytes, kbo_ref_best *d_out, void *stream);
/* The SCREENED device forms: the device-resident calls above over a set built with a prefilter, walking only the pairs the seed screen
 * marks.  They are opt-in; kbo_*_refset_dev keep ignoring the prefilter.  Everything those promise holds: all work is enqueued on
 * `stream`, no synchronisation, no device-to-host copy, no allocation, all scratch in d_work (16-byte aligned) and nothing written
 * behind the figure of *_work_bytes, the same inputs, alignments and 16 bytes of slack behind d_concat.  The call's ONE host-to-device
 * upload is 5 bytes a reference: the thresholds and the seed lengths m_r, which only the host can compute.
 * kbo_refset_candidates_dev is kbo_refset_candidates for a batch on the device: d_bits (4-byte aligned, ceil(n_refs x n_seqs x 2 / 32)
 * words, zeroed by the call) receives the same bitmap bit for bit - a reference that cannot be screened at this max_error_prob has
 * all its pairs on the strands asked for set - and d_stats (8-byte aligned) n_candidates and candidate_bases (the bases of the
 * candidate pairs, a pair counting its sequence's length), n_walked = walked_bases = 0.  5 launches, 6 with the '-' strand.
 * kbo_find / summary / best_refset_screened_dev run that screen into d_work, list the set bits in ascending order - the records' own
 * order (ref, seq, strand with '+' first) - and walk ONE slab: the longest prefix of that list with at most max_pairs pairs and at
 * most max_pair_bases bases.  d_stats receives the four figures; the caller reads it when it likes, and n_walked == n_candidates says
 * that the call is complete.  A caller that sizes the caps from kbo_refset_candidates_dev's figures always is.  Records: byte for byte
 * those of the host forms restricted to the walked pairs, in the same order; capacity and *d_n_runs / *d_n_records as in the
 * unscreened forms; for best, d_out is the complete table of n_seqs records over the walked pairs.  Several slabs are out of scope:
 * ONE slab holds at most 2^28 - 1 pairs and 2^32 - 17 bytes, and a caller with more candidates than that uses the unscreened form.
 * Launches, whatever the batch and the bitmap hold: find 46, summary 34, best 31; one more with the '-' strand (and a device-to-device
 * copy of the batch when both strands are asked for), one more for a set with both LDS and wide references.  Grids are sized by the
 * caps - max_pair_bases / chunk + max_pairs item slots, that / 256 + min(queryable references, max_pairs) + 1 workgroups of the walk -
 * and lanes behind the device-side counts return, so generous caps cost time as well as scratch.
 * *_work_bytes are exact, grow with max_pairs, max_pair_bases and capacity, and are 0 for arguments the call refuses.
 * Errors, all before anything is enqueued: those of the unscreened device forms; KBO_E_BAD_ARG for a set without a prefilter, for
 * max_pairs == 0 and for a work_bytes below the figure; KBO_E_UNSUPPORTED for a bitmap of more than 2^31 bits, a reference of the
 * single-index route, a batch of 2^31 bases or more, and caps beyond what one slab may hold. */
typedef struct {
    uint64_t n_candidates, candidate_bases, n_walked, walked_bases;
} kbo_refset_screen_stats; /* 32 bytes, on the device */
size_t kbo_refset_candidates_dev_work_bytes(const kbo_refset_t *set, size_t n_seqs, uint64_t total_bases, int strands);
int kbo_refset_candidates_dev(kbo_refset_t *set, const uint8_t *d_concat, const uint64_t *d_offsets, size_t n_seqs, uint64_t total_bases,
                              double max_error_prob, int strands, void *d_work, size_t work_bytes, uint32_t *d_bits,
                              kbo_refset_screen_stats *d_stats, void *stream);
size_t kbo_find_refset_screened_dev_work_bytes(const kbo_refset_t *set, size_t n_seqs, uint64_t total_bases, int strands, size_t capacity,
                                               size_t max_pairs, uint64_t max_pair_bases);
int kbo_find_refset_screened_dev(kbo_refset_t *set, const uint8_t *d_concat, const uint64_t *d_offsets, size_t n_seqs, uint64_t total_bases,
                                 const kbo_find_opts *opts, int strands, void *d_work, size_t work_bytes, kbo_ref_run *d_runs, size_t capacity,
                                 uint64_t *d_n_runs, size_t max_pairs, uint64_t max_pair_bases, kbo_refset_screen_stats *d_stats, void *stream);
size_t kbo_summary_refset_screened_dev_work_bytes(const kbo_refset_t *set, size_t n_seqs, uint64_t total_bases, int strands, size_t capacity,
                                                  size_t max_pairs, uint64_t max_pair_bases);
int kbo_summary_refset_screened_dev(kbo_refset_t *set, const uint8_t *d_concat, const uint64_t *d_offsets, size_t n_seqs, uint64_t total_bases,
                                    double max_error_prob, int strands, void *d_work, size_t work_bytes, kbo_ref_summary *d_records,
                                    size_t capacity, uint64_t *d_n_records, size_t max_pairs, uint64_t max_pair_bases,
                                    kbo_refset_screen_stats *d_stats, void *stream);
size_t kbo_best_refset_screened_dev_work_bytes(const kbo_refset_t *set, size_t n_seqs, uint64_t total_bases, int strands, size_t max_pairs,
                                               uint64_t max_pair_bases);
int kbo_best_refset_screened_dev(kbo_refset_t *set, const uint8_t *d_concat, const uint64_t *d_offsets, size_t n_seqs, uint64_t total_bases,
                                 double max_error_prob, int strands, void *d_work, size_t work_bytes, kbo_ref_best *d_out, size_t max_pairs,
                                 uint64_t max_pair_bases, kbo_refset_screen_stats *d_stats, void *stream);
/* The LOCUS of a run: which part of its reference a kbo_ref_run covers.  Every coordinate of a run is one of the query sequence; a
 * set built with kbo_refset_opts.positions = 1 also answers where on the reference the run lies - which half of the gene, forward or
 * reverse - exactly and without a second alignment.  With positions = 0 (the default) the set is byte for byte what it is without the
 * field: arena, descs, device copy and every *_work_bytes figure; values other than 0 and 1 give KBO_E_BAD_ARG.
 * The table: one uint32_t per row of every reference of a packed route (LDS or wide) that can be queried, made on the host at build
 * time by walking every indexed stretch - a maximal run of A, C, G, T of at least k bases, as for the seed table - and, with
 * opts->add_revcomp, its reverse complement through the reference's own packed form.  An OCCURRENCE of a k-mer x in reference r is
 * (p, FWD) when x equals ref[p, p + k) and (p, REV) when the reverse complement of x does (REV only with add_revcomp), the window
 * inside an indexed stretch, p 0-based on the reference as given.  The entry of x's row holds, of x's occurrences, the one with FWD
 * before REV and then the smallest p: bits 0 .. 29 p, bit 30 set for REV, bit 31 (KBO_LOCUS_MULTI) set when x has more than one
 * occurrence; a row that is no full k-mer (a dummy row) holds KBO_POS_NONE.  References of the single-index route and references
 * with a status have no entries.  A reference of 2^30 bases or more makes the build fail with KBO_E_UNSUPPORTED, before any work.
 * (KBO_E_UNSUPPORTED too, behind the walk, should an indexed k-mer ever lack a row of its own in the packed form: the table cannot be made.)
 * kbo_refset_to_device uploads the table with the arena (4 bytes a row + 8 a reference: kbo_refset_positions_bytes).
 * kbo_refset_positions copies the entries of reference r (out may be NULL: *n_rows alone; 0 rows for a reference without entries;
 * KBO_E_BAD_ARG for a set without positions or r >= N); kbo_refset_ref_len is a reference's length as given, kept for every set.
 *
 * A run covers the half-open 0-based range [run.start, run.end) of the sequence on its strand (format.rs:154,175: start is the index
 * of the run's first character and end one past its last character that is no gap - as oracle/kbo_oracle.c's
 * ora_run_lengths_gapped states it and the find tests compare it).  An ANCHOR of the run is a position i with run.start <= i and
 * i + k <= run.end whose k bytes [i, i + k) of the strand's sequence are all A, C, G, T and are a k-mer of reference run.ref.  For
 * strand == KBO_STRAND_REV the strand's sequence is the reverse complement as kbo_revcomp_batch defines it: byte j is the complement
 * of byte len - 1 - j as given, and lower case is no base.  The first anchor is the smallest such i, the last anchor the largest;
 * they may be the same.  A run without one - a run shorter than k included - has all four positions KBO_LOCUS_NONE and flags 0.
 * Bit 4 of flags, with all positions KBO_LOCUS_NONE and n_tested 0, marks a record the call cannot use: ref >= N, a reference with a
 * status or of the single-index route, seq >= n_seqs, a strand that is not 1 or 2, start > end, or end beyond the sequence.
 *
 * kbo_locate_refset: the batch is kbo_find_refset's ('+' as given), runs any n_runs records with (ref, seq, strand, run.start,
 * run.end) set - kbo_find_refset's, on either or both strands - and loci_out receives n_runs records, same index.  It uploads the
 * batch and the runs, launches ONE kernel (kbo_amd/csrc/refset_locate_kernels.hip: a wave per run, 64 windows a step, the packed form
 * read from the arena) and downloads the loci: one synchronisation.  Errors, all before the first HIP call and in this order:
 * KBO_E_BAD_ARG for null arguments (runs and loci_out may be NULL when n_runs == 0) and for a set without positions; the offsets as
 * kbo_find_refset checks them; KBO_E_BAD_ARG for a record that bit 4 describes.  n_runs == 0 succeeds and touches no device.
 * kbo_locate_refset_host is the same call restated on the CPU (no device; a test hook and a yardstick): byte-identical records.
 * kbo_locate_refset_dev: kbo_find_refset_dev's contract for the batch (d_concat 16-byte aligned with 16 readable bytes behind
 * total_bases, d_offsets 8-byte aligned) and d_runs / d_n_runs (4- / 8-byte aligned) exactly as kbo_find_refset_dev and
 * kbo_find_refset_screened_dev leave them, so the calls compose on one stream with nothing read back.  It writes
 * min(*d_n_runs, capacity) records to d_loci (4-byte aligned) and nothing at or behind element `capacity` (d_runs and d_loci may be
 * NULL when capacity == 0); one launch, no synchronisation, no allocation, no scratch.  The kernel checks every record itself from
 * the descs and the offsets and reads nothing outside the batch, the arena and the table: a record that bit 4 describes - or an
 * offset pair that is descending or beyond total_bases - gets bit 4, never a fault.  KBO_E_BAD_ARG before anything is enqueued for
 * null or misaligned pointers, a set without positions and a set without a copy on the current device; KBO_E_EMPTY_QUERY for
 * n_seqs == 0.
 * n_tested counts the k-mer windows handed to lanes for this run, 64 at a time from the front until a group holds an anchor and
 * then from the back (both directions; the last group of a direction counts the windows that are left): a work count. */
#define KBO_POS_NONE 0xFFFFFFFFu
#define KBO_LOCUS_MULTI 0x80000000u
#define KBO_LOCUS_NONE 0xFFFFFFFFu
typedef struct {
    uint32_t q_first, ref_first; /* first anchor: position in the sequence on the run's strand of the k-mer's first base; the table's p */
    uint32_t q_last, ref_last;   /* last anchor */
    uint32_t flags;              /* bit 0 / 1: first / last anchor is a REV occurrence; bit 2 / 3: it is MULTI; bit 4: the record was not usable */
    uint32_t n_tested;           /* k-mer windows looked up for this run (both directions) */
} kbo_ref_locus; /* 24 bytes, one per kbo_ref_run, same index */
int kbo_refset_has_positions(const kbo_refset_t *set);        /* 1 or 0 */
uint64_t kbo_refset_positions_bytes(const kbo_refset_t *set); /* the position table's bytes; 0 without one */
int kbo_refset_positions(const kbo_refset_t *set, size_t r, uint32_t *out, size_t *n_rows);
uint64_t kbo_refset_ref_len(const kbo_refset_t *set, size_t r); /* 0 for r >= N */
int kbo_locate_refset(kbo_refset_t *set, const uint8_t *concat, const uint64_t *offsets, size_t n_seqs, const kbo_ref_run *runs,
                      uint64_t n_runs, kbo_ref_locus *loci_out);
int kbo_locate_refset_dev(kbo_refset_t *set, const uint8_t *d_concat, const uint64_t *d_offsets, size_t n_seqs, uint64_t total_bases,
                          const kbo_ref_run *d_runs, const uint64_t *d_n_runs, size_t capacity, kbo_ref_locus *d_loci, void *stream);
int kbo_locate_refset_host(const kbo_refset_t *set, const uint8_t *concat, const uint64_t *offsets, size_t n_seqs, const kbo_ref_run *runs,
                           uint64_t n_runs, kbo_ref_locus *loci_out);
/* The COVER of a reference: how much of reference r the whole batch covers, how deep and in how many pieces - the one reduction
 * along REFERENCE coordinates; every other record is keyed by a query sequence.  The set is built with positions = 1.  Reference r
 * HAS ENTRIES when it is of a packed route (LDS or wide) and its status is 0; anchors and usable records are those of "The LOCUS of a
 * run" above.  For a reference with entries of L_r bases (kbo_refset_ref_len):
 *   H_r[p], 0 <= p < L_r: the number of (record, anchor) pairs with the record one of the usable records given to the call with
 *     ref == r and the entry of the anchor's k-mer holding position p (its low 30 bits; FWD and REV alike: both say that
 *     ref[p, p + k) is matched).  A record given twice counts twice.  A MULTI k-mer counts at its one stored occurrence (FWD before
 *     REV, then the smallest p) and nowhere else: an exact repeat of k or more bases inside a reference leaves its second copy
 *     uncovered - n_multi says how many anchors that concerns.  Marking every occurrence needs an occurrence list that the set does
 *     not keep; it is out of scope.
 *   D_r[j] = sum of H_r[p] over max(0, j - k + 1) <= p <= j, 0 <= j < L_r: the DEPTH at base j.
 * kbo_ref_cover holds, per reference, index = reference: ref_len = L_r as given (set for every reference); covered = the number of j
 * with D[j] > 0; n_segments = the maximal intervals of such j; first / last = the smallest / largest such j (KBO_LOCUS_NONE when
 * covered == 0); max_depth = the largest D[j]; n_runs = the usable records with ref == r; n_anchors = the sum of H; n_multi = the
 * anchors among them whose entry has MULTI.  flags bit 0 (KBO_COVER_NO_ENTRIES): the reference has no entries (the single-index
 * route, or a status) - every field but ref_len is 0 and first / last are KBO_LOCUS_NONE.  Bit 1 (KBO_COVER_OVERFLOW): n_anchors >=
 * 2^32; H and D are 32-bit, so every field but ref_len, n_runs, n_anchors and n_multi is unspecified.  With bit 1 clear the sum of D
 * is k * n_anchors, covered <= ref_len, and covered == 0 exactly when n_anchors == 0.
 * The DEPTH PROFILE (optional) is D_r as uint32_t for every reference with entries, concatenated in reference order:
 * kbo_refset_cover_offsets copies the N + 1 offsets (made at build time; a reference without entries owns no element; KBO_E_BAD_ARG
 * for a set without positions), kbo_refset_cover_bases is their last, B (0 without positions).  kbo_refset_to_device uploads the
 * offsets as a small allocation of their own; kbo_refset_positions_bytes does not count them.
 *
 * kbo_cover_refset: batch and runs as for kbo_locate_refset; covers_out receives N records, depth_out (or NULL) B words.  It uploads
 * the batch and the runs, clears its scratch, launches three kernels (kbo_amd/csrc/refset_cover_kernels.hip: count - a wave per run,
 * every window looked up, an integer atomic add per anchor; scan - a prefix sum per reference; reduce - D, the record, the profile)
 * and downloads the records, and the profile when asked: one synchronisation.  The result does not depend on the order of the runs.
 * Errors, all before the first HIP call and in this order: KBO_E_BAD_ARG for null arguments (runs may be NULL when n_runs == 0,
 * depth_out always) and for a set without positions; the offsets as kbo_find_refset checks them; KBO_E_BAD_ARG for a record that
 * bit 4 of a locus describes.  n_runs == 0 succeeds and touches no device: records with ref_len, bit 0 where due and zeros, and a
 * profile of zeros.
 * kbo_cover_refset_host is the same call restated on the CPU (no device; a test hook and a yardstick): byte-identical records and
 * profile.
 * kbo_cover_refset_dev: kbo_locate_refset_dev's contract for the batch and for d_runs / d_n_runs, so it composes on one stream
 * behind kbo_find_refset_dev and kbo_find_refset_screened_dev with nothing read back.  It reads min(*d_n_runs, capacity) records
 * (d_runs may be NULL when capacity == 0) and checks every one itself as the locate kernel does; an unusable record is skipped: it
 * contributes nothing and cannot fault.  It writes N records to d_covers (4-byte aligned) and, when d_depth is given (4-byte
 * aligned), B words there; nothing outside them and d_work[0, work_bytes).  No synchronisation, no allocation, no scratch memory.
 * d_work: 16-byte aligned, work_bytes at least kbo_cover_refset_dev_work_bytes(set) - 24 bytes a reference for the counters and 4
 * bytes a base of B for H, each part rounded up to 16; it does not depend on the batch and is 0 for a set the call refuses.
 * KBO_E_BAD_ARG before anything is enqueued for null or misaligned pointers, a set without positions, a short d_work and a set
 * without a copy on the current device; KBO_E_EMPTY_QUERY for n_seqs == 0. */
#define KBO_COVER_NO_ENTRIES 1u
#define KBO_COVER_OVERFLOW 2u
typedef struct {
    uint32_t ref_len;     /* L_r as given */
    uint32_t covered;     /* bases with D > 0 */
    uint32_t n_segments;  /* maximal intervals of them */
    uint32_t first, last; /* the smallest and the largest covered base; KBO_LOCUS_NONE without one */
    uint32_t max_depth;
    uint32_t n_runs;      /* usable records of this reference */
    uint32_t flags;       /* KBO_COVER_NO_ENTRIES, KBO_COVER_OVERFLOW */
    uint64_t n_anchors;   /* the sum of H */
    uint64_t n_multi;     /* the anchors among them whose entry has MULTI */
} kbo_ref_cover; /* 48 bytes, one per reference of the set, index = reference */
uint64_t kbo_refset_cover_bases(const kbo_refset_t *set);
int kbo_refset_cover_offsets(const kbo_refset_t *set, uint64_t *out /* N + 1 */);
int kbo_cover_refset(kbo_refset_t *set, const uint8_t *concat, const uint64_t *offsets, size_t n_seqs, const kbo_ref_run *runs,
                     uint64_t n_runs, kbo_ref_cover *covers_out, uint32_t *depth_out);
int kbo_cover_refset_host(const kbo_refset_t *set, const uint8_t *concat, const uint64_t *offsets, size_t n_seqs, const kbo_ref_run *runs,
                          uint64_t n_runs, kbo_ref_cover *covers_out, uint32_t *depth_out);
size_t kbo_cover_refset_dev_work_bytes(const kbo_refset_t *set);
int kbo_cover_refset_dev(kbo_refset_t *set, const uint8_t *d_concat, const uint64_t *d_offsets, size_t n_seqs, uint64_t total_bases,
                         const kbo_ref_run *d_runs, const uint64_t *d_n_runs, size_t capacity, kbo_ref_cover *d_covers, uint32_t *d_depth,
                         void *d_work, size_t work_bytes, void *stream);
/* The VARIANTS of a pair: what differs between reference r and its copy in sequence s - kbo::call (lib.rs:547-573) against every
 * reference of the set that has a hit, in one call.  kbo_call_refset returns records for every (reference r, sequence s, strand) pair
 * that kbo_summary_refset has a record for with the same set, batch, strands and max_error_prob, and for no other: a pair without a
 * summary record contributes nothing, by definition.  (That is what makes the prefilter exact for this call: a site needs a depth of
 * at least the threshold, the screen proves the absence of one above it, and a pair whose depths only reach the threshold has no
 * summary record.)  The records of a pair are exactly the variants kbo_call(an index of reference r alone, sequence s, opts)
 * returns - for KBO_STRAND_REV with the reverse complement of s as kbo_revcomp_batch makes it, in the coordinates of the reverse
 * complement, as everywhere in this family.  The threshold is that of reference r's own n_kmers (lib.rs:620).  Field roles are the
 * reference crate's: query_chars are characters of the walked sequence s, ref_chars those of the matched row of reference r's index,
 * so a contig with 'A' where the gene has 'G' gives (pos, "A", "G").  An insertion in s has ref_len 0, a deletion query_len 0.
 * Useful calls need k of about twice the threshold or more: resolve_variant (variant_calling.rs:139-201) needs a significant match
 * on either side of the site inside one k-mer, so with thresholds of 15 - 18 (references of 300 - 20 000 bases) k = 41 and above
 * resolve substitutions, insertions and deletions alike and k = 31 resolves little but deletions.
 * Records are in the order (ref, seq, strand with KBO_STRAND_FWD first, pos).  `chars` of a record is the offset of its characters
 * in kbo_ref_calls.chars: query_len characters of the sequence, then ref_len of the reference.  Without a variant n_variants is 0
 * and both pointers are NULL.  kbo_ref_calls_free releases both arrays (malloc'ed) and clears the struct; NULL is allowed.
 *
 * opts->sbwt_build_opts.k must equal the set's k.  opts->sbwt_build_opts.add_revcomp applies to the index of the sequence itself
 * (lib.rs:553), as in kbo_call_batch, and is independent of how the set was built; the other build options are not used.  NULL opts:
 * the defaults.  The set must be kbo_refset_packed_only(); references with a status contribute nothing.
 * Errors, all before the first HIP call and in this order: KBO_E_BAD_ARG for strands outside 1 .. 3 and for a null set or out (out
 * is cleared from here on); KBO_E_K_MISMATCH, as kbo_call_batch; KBO_E_UNSUPPORTED for a set with a reference of the single-index
 * route, as the device forms; then kbo_summary_refset's for max_error_prob, the thresholds and the batch, in its order and with its
 * codes; KBO_E_UNSUPPORTED for a sequence of 2^29 bases or more (2^28 with add_revcomp), as kbo_call_batch.
 *
 * kbo_call_refset runs kbo_summary_refset's slabs - on a set with a prefilter over the candidate pairs alone, with the same bytes
 * returned - and behind the walk and the counting derandomize of every slab three more kernels
 * (kbo_amd/csrc/refset_call_kernels.hip): scan, a lane per byte of the slab's matching statistics, finds the positions i >= 1 of
 * kept pairs with d[i] < d[i-1], d[i-1] >= t and d[i] < t (variant_calling.rs:269); match, a wave per candidate, finds the first j
 * in i + 1 .. min(i + k + 1, len) with d[j] >= t whose interval is one row, the interval recomputed by d[j] rank steps over the
 * packed form; spell, a lane per site, reads the row's k-mer off the packed form by k inverse steps and gathers the k depths that
 * end at j.  Two counts, the site records and the windows come back per slab.  The host then resolves every site as kbo_call_batch
 * resolves a site left to it (variant_calling.rs:275-284), with one suffix automaton per (sequence, strand) that has a site.
 * kbo_call_refset_host is the same call restated on the CPU (no HIP call; a test hook and a yardstick): byte-identical records and
 * characters.  Open: references of the single-index route.
 *
 * kbo_call_refset_dev and kbo_call_refset_screened_dev are the device-resident forms.  Everything kbo_summary_refset_dev and
 * kbo_summary_refset_screened_dev promise holds: the inputs, alignments and 16 bytes of slack of the batch, a set that is
 * kbo_refset_packed_only() with a copy on the current device, everything enqueued on `stream`, nothing synchronised, read back or
 * allocated, all scratch in d_work (16-byte aligned) and nothing written behind the figure of *_work_bytes; refs_per_slab, max_pairs
 * and max_pair_bases mean what they mean there (the screened form walks ONE slab; n_walked == n_candidates of d_screen_stats says
 * that it held every candidate).  The call's only upload is the thresholds (and, screened, the seed lengths).  opts as in
 * kbo_call_refset, add_revcomp included.
 * Records: byte for byte the kbo_ref_variant records and characters of kbo_call_refset for the same set, batch, options and strands,
 * in its order; the screened form returns those of the walked pairs.  Record x is written iff x < max_variants, its characters iff
 * chars + query_len + ref_len <= max_chars; d_stats->n_variants and n_chars are the full totals, and nothing at or behind either
 * capacity is touched (d_variants may be NULL when max_variants == 0, d_chars when max_chars == 0).  d_variants is 4-byte, d_stats
 * 8-byte aligned.
 * max_sites bounds three lists in d_work: a slab's candidates, a slab's sites, and the sites of the whole call.  The host form enlarges
 * its lists and repeats a slab; the device form cannot, so it counts what it could not store: the call is COMPLETE iff
 * max_slab_candidates <= max_sites and n_sites <= max_sites.  The records of the stored sites are exact either way.
 * A site at which the reference would panic (resolve_variant: common suffix 0, a slice beyond the k-mer) makes kbo_call_refset fail
 * with KBO_E_REF_PANIC; the device forms count it in n_panics and emit nothing for it.  Sequences of fewer than 3 bases contribute
 * nothing.  Limits: those of the device forms (strands x bases below 2^32 - 16; 2^31 bases screened) and max_sites <= 2^23; the host
 * form's 2^29 bases a sequence do not apply, and a sequence may be as long as the batch.
 * The second pass (kbo_amd/csrc/refset_resolve_kernels.hip; the arithmetic: refset_resolve.hpp) runs behind the last slab: ONE
 * index of the '+' strand of the batch - a word { q-mer code, start } per base whose q-mer, q = min(12, the smallest threshold), lies
 * inside a run of at least k bases, every other base a word with a code that no q-mer has, radix-sorted by code in four passes, in
 * time linear in the batch whatever repeats it holds - then a wave per
 * site that probes it for the depths of the row's k-mer (forwards, as reverse complements, or both: the site's strand and
 * add_revcomp), the resolve word, a radix sort of the sites' keys (ref, seq, strand, pos), two scans and one write.  d_work holds
 * 16 bytes a base for the index and its sort, 1/4 byte a base for the sort's histograms, 4 k + 100 bytes (k rounded up to 16) a
 * site of max_sites and 12 bytes a pair of a slab, behind what the best form holds; the figure is never below the summary form's.
 * Launches, whatever the batch holds: per slab the summary form's without its compaction and record append, + 1 (the pairs' words) +
 * 3 and a clear (the first pass) + 1 (the append); per call 25 + 4 P behind the last slab, P = ceil(bits(total_bases + 1) / 8) +
 * ceil((bits(N) + bits(n_seqs) + 1) / 8) the passes over the sites' keys (bits(v): the bits that hold 0 .. v - 1), and the clear of
 * d_stats.
 * Errors, all before anything is enqueued and in this order: those of kbo_summary_refset_dev / _screened_dev for the same arguments
 * (d_stats null or misaligned among them); KBO_E_K_MISMATCH; KBO_E_BAD_ARG for max_sites == 0, KBO_E_UNSUPPORTED for max_sites above
 * 2^23; then a short work_bytes and a set without a copy on the current device, as there.  *_work_bytes are exact, grow with
 * max_sites and refs_per_slab (max_pairs, max_pair_bases), are at least the summary form's, and are 0 for arguments the call refuses. */
typedef struct {
    uint64_t n_variants, n_chars; /* what there is, those beyond the capacities included */
    uint64_t n_sites;             /* sites found in the whole call, those beyond max_sites included; the sites of candidates that a
                                     slab could not store are never found, so not counted: max_slab_candidates says that there are such */
    uint64_t max_slab_candidates; /* the most candidates one slab had */
    uint64_t n_panics;            /* sites at which the reference panics */
    uint64_t reserved[3];
} kbo_ref_calls_stats;            /* 64 bytes, on the device */
typedef struct {
    uint32_t ref, seq, strand;   /* as kbo_ref_run */
    uint32_t pos;                /* Variant::query_pos: in sequence s on that strand */
    uint32_t chars;              /* offset into kbo_ref_calls.chars: query_len characters of the sequence, then ref_len of reference r */
    uint16_t query_len, ref_len; /* 0 = none: an insertion has ref_len 0, a deletion query_len 0 */
} kbo_ref_variant;               /* 24 bytes */
typedef struct {
    uint64_t n_variants, n_chars;
    kbo_ref_variant *variants;
    uint8_t *chars;
} kbo_ref_calls;
int kbo_call_refset(kbo_refset_t *set, const uint8_t *concat, const uint64_t *offsets, size_t n_seqs, const kbo_call_opts *opts, int strands,
                    kbo_ref_calls *out);
int kbo_call_refset_host(const kbo_refset_t *set, const uint8_t *concat, const uint64_t *offsets, size_t n_seqs, const kbo_call_opts *opts,
                         int strands, kbo_ref_calls *out);
void kbo_ref_calls_free(kbo_ref_calls *calls);
size_t kbo_call_refset_dev_work_bytes(const kbo_refset_t *set, size_t n_seqs, uint64_t total_bases, int strands, size_t max_sites,
                                      size_t refs_per_slab);
int kbo_call_refset_dev(kbo_refset_t *set, const uint8_t *d_concat, const uint64_t *d_offsets, size_t n_seqs, uint64_t total_bases,
                        const kbo_call_opts *opts, int strands, void *d_work, size_t work_bytes, kbo_ref_variant *d_variants, size_t max_variants,
                        uint8_t *d_chars, size_t max_chars, size_t max_sites, kbo_ref_calls_stats *d_stats, void *stream);
size_t kbo_call_refset_screened_dev_work_bytes(const kbo_refset_t *set, size_t n_seqs, uint64_t total_bases, int strands, size_t max_sites,
                                               size_t max_pairs, uint64_t max_pair_bases);
int kbo_call_refset_screened_dev(kbo_refset_t *set, const uint8_t *d_concat, const uint64_t *d_offsets, size_t n_seqs, uint64_t total_bases,
                                 const kbo_call_opts *opts, int strands, void *d_work, size_t work_bytes, kbo_ref_variant *d_variants,
                                 size_t max_variants, uint8_t *d_chars, size_t max_chars, size_t max_sites, kbo_ref_calls_stats *d_stats,
                                 size_t max_pairs, uint64_t max_pair_bases, kbo_refset_screen_stats *d_screen_stats, void *stream);

/* ------------------------------------------------------------------ device-resident path
 * Everything already in the HBM of the current device; kernels are enqueued on `stream`
 * (a hipStream_t) and the call returns immediately.  d_concat must be 16-byte aligned,
 * the other buffers 4-byte aligned.
 * SLACK: the kernels move bytes in 16-byte blocks relative to each sequence, so every per-base
 * buffer handed to these entry points - d_concat, d_ms_out / d_ms, d_ref, d_chars_out / d_chars -
 * must have at least 16 readable (for outputs: writable) bytes behind its last base, i.e. be
 * allocated with total_bases + 16 bytes or more (the in-repo callers round up to 16 and add 64).
 * The calls check what they can: they refuse total_bases + 16 > 2^32.  Sequences shorter than 3 are skipped by the fused
 * derandomize/translate kernel (the host entry points reject them like the reference).
 * d_work is device scratch of at least kbo_work_bytes(...) bytes for the batch (16-byte aligned).  Since round 5 that figure holds, for
 * batches with sequences of more than 160 bases (max_seq_len 0 or > 160), the regions of the kernels for long sequences as well (about
 * 0.5 B per base more): what kbo_map_batch_dev[_tail], kbo_find_batch_dev and kbo_map_stream_* check.  The walks alone - kbo_ms_batch_dev,
 * kbo_call_walk_dev - never touch those regions and check kbo_ms_work_bytes(...) only (the round-4 figure; <= kbo_work_bytes). */
size_t kbo_work_bytes(size_t n_seqs, uint64_t total_bases, size_t max_seq_len, uint32_t k);
size_t kbo_ms_work_bytes(size_t n_seqs, uint64_t total_bases, size_t max_seq_len, uint32_t k);
/* the same for a given index: kbo_work_bytes() for an ordinary index; for a sharded index (kbo_index_shards() > 1) that plus one
 * further shard's MS values, round16(total_bases) + 16 <= total_bases + 32 bytes.  What a SHARDED index needs as d_work:
 *   kbo_ms_batch_dev                                   kbo_ms_work_bytes() + round16(total_bases) + 16 (the walk's figure + one shard's
 *                                                      values, which sit right behind the walk's own region)
 *   kbo_map_batch_dev[_tail], kbo_find_batch_dev,      kbo_index_work_bytes() - NOT kbo_work_bytes(): both are refused with KBO_E_BAD_ARG
 *   kbo_map_stream_* (sizes its slots itself)          (kbo_call_walk_dev and kbo_matches_packed_dev refuse a sharded index) */
size_t kbo_index_work_bytes(const kbo_index_t *idx, size_t n_seqs, uint64_t total_bases, size_t max_seq_len);
/* A1 over a batch.  total_bases = offsets[n_seqs] (known to the caller; avoids a device read-back);
 * max_seq_len = length of the longest sequence if the caller knows it, 0 = unknown.  Batches of reads
 * get one work item per sequence; when max_seq_len is unknown or long, the item list is built on the
 * device from the offsets: sequences are cut into chunks that restart the walk k-1 bases upstream
 * (the MS of a base depends only on the k bases ending at it), so a few long sequences still fill the
 * device.  Same results either way - provided max_seq_len, when given, is not SMALLER than the longest sequence: the
 * kernels size their work items (16-bit lengths) and LDS stretches from it; pass 0 when in doubt.
 * Reads (max_seq_len <= 160) over a copy with a depth table, intervals not asked for: ONE kernel puts the values together (k where
 * nothing happened, the ramps behind the mismatches, the table's values behind them) and a second kernel walks the reads it leaves -
 * 305 Gbp/s at C2, 392 with resident batches in turn on two streams of the caller's (the plan-guided walk it replaces there: 242);
 * every other batch - chunks of long sequences, intervals (d_lo_out / d_hi_out: the colexicographic intervals, index.rs:243-256),
 * sharded indexes - takes the plan-guided walk. */
int kbo_ms_batch_dev(kbo_index_t *idx, const uint8_t *d_concat, const uint64_t *d_offsets,
                     size_t n_seqs, uint64_t total_bases, size_t max_seq_len, uint8_t *d_ms_out,
                     uint32_t *d_lo_out, uint32_t *d_hi_out, void *d_work, size_t work_bytes, void *stream);
/* A5+A6 fused (+ optional format::relative_to_ref when d_ref != NULL): u8 MS -> u8 chars.
 * max_seq_len = length of the longest sequence in the batch if the caller knows it (selects
 * the LDS-staged kernel for short reads), 0 = unknown.  d_work (optional, NULL = none): scratch of
 * kbo_derand_work_bytes() bytes, 16-byte aligned; with it long reads / contigs are processed in
 * pieces of 132 positions, one lane each, instead of one lane per sequence (a smaller work_bytes is not an error: one lane per
 * sequence, the same characters).  d_ms, d_ref, d_chars_out: total_bases + 16 bytes, 4-byte aligned.  d_chars_out must NOT be d_ms
 * (KBO_E_BAD_ARG) nor overlap it: a piece reads MS bytes up to 1024 positions above itself, which belong to other workgroups, and
 * sequences it cannot finish that way are read again by a second launch after their other pieces' characters were written.
 * Sequences of fewer than 3 bases are skipped (their bytes of d_chars_out are unspecified). */
size_t kbo_derand_work_bytes(size_t n_seqs, uint64_t total_bases);
int kbo_derand_translate_dev(const uint8_t *d_ms, const uint64_t *d_offsets, size_t n_seqs,
                             uint64_t total_bases, size_t k, size_t threshold, const uint8_t *d_ref,
                             uint8_t *d_chars_out, size_t max_seq_len, void *d_work, size_t work_bytes,
                             void *stream);
/* The same stage for a batch in which every sequence has a threshold of its own, at any length: d_thresholds[s] (on the device) is
 * sequence s's threshold and min_threshold (known on the host) a lower bound of them that sizes the tables; a looser bound costs
 * scratch and time, never a character.  For every sequence of >= 3 bases with min_threshold <= d_thresholds[s] <= k the characters
 * are exactly translate_ms_vec(derandomize_ms_vec(ms_s, k, t_s), k, t_s) - for ANY MS bytes <= k, not only those a walk produces,
 * with no look-ahead heuristic and no fallback launch - and with d_ref != NULL format::relative_to_ref of that.  Sequences of fewer
 * than 3 bases are skipped (their bytes of d_chars_out stay as they were); a threshold outside [min_threshold, k] gives that sequence
 * unspecified characters and nothing else.  The call enqueues 11 kernel launches and no memset on `stream`, whatever n_seqs, the
 * lengths and the thresholds are, reads nothing back and returns: chunks of KBO_DERAND_SEQ_CHUNK positions and groups of
 * KBO_DERAND_SEQ_GROUP positions (kbo_hip_tuning.h), neither ever spanning two sequences, are listed on the device from d_offsets;
 * every chunk and every group gets a table of k - min_threshold + 1 states that says what it does to the value entering it, one
 * lane per sequence runs over that sequence's groups, and a last pass per chunk writes the characters.
 * d_ms, d_ref, d_chars_out: total_bases + 16 bytes, 4-byte aligned; d_chars_out must NOT be d_ms (a chunk reads the MS byte below
 * it, which belongs to another workgroup).  d_work: required, 16-byte aligned, kbo_derand_seq_work_bytes() bytes - about
 * total_bases * (k - min_threshold + 6) / 32 + n_seqs * (8 (k - min_threshold) + 64) bytes: 4 (k - min_threshold + 1) bytes of table per
 * chunk of 128 bases, 1/64 of that per group, 20 bytes of descriptor and value per chunk, and a chunk and a group more per sequence
 * (0.7 bytes a base at k = 31, t >= 14; 8.1 at k = 255, t >= 2).
 * No byte of d_work beyond that figure is touched.  n_seqs < 2^28.
 * Errors, before anything is enqueued: KBO_E_BAD_ARG (null argument, k outside 1..255, min_threshold > k, work_bytes too small,
 * alignment), KBO_E_EMPTY_QUERY (n_seqs == 0), KBO_E_THRESHOLD_LE_1 (min_threshold <= 1, derandomize.rs:275), KBO_E_UNSUPPORTED
 * (total_bases + 16 > 2^32, n_seqs >= 2^28). */
size_t kbo_derand_seq_work_bytes(size_t n_seqs, uint64_t total_bases, size_t k, size_t min_threshold);
int kbo_derand_translate_seq_dev(const uint8_t *d_ms, const uint64_t *d_offsets, size_t n_seqs, uint64_t total_bases,
                                 size_t k, const uint32_t *d_thresholds, size_t min_threshold, const uint8_t *d_ref,
                                 uint8_t *d_chars_out, void *d_work, size_t work_bytes, void *stream);
/* The summary form of that stage: the same inputs, the same contract - any MS bytes <= k, a threshold per sequence, any length,
 * exact - and one kbo_aln_extent record per sequence instead of a character per base.  The passes up to the value entering every
 * chunk are the character form's, called as they are; the last one counts the characters of a chunk where the character form packs
 * them, in LDS, and the lanes of a wave that sit on one sequence are summed before its record is added to - so no character buffer
 * exists.  The call enqueues 13 kernel launches and no memset on `stream`, whatever n_seqs, the lengths and the thresholds are,
 * reads nothing back and returns.  d_out: n_seqs records (24 n_seqs bytes), 4-byte aligned, every one written: a sequence of fewer
 * than 3 bases gets zeros.  d_ms: total_bases + 16 bytes, 4-byte aligned, not written.  d_work: required, 16-byte aligned,
 * kbo_derand_summary_seq_work_bytes() bytes (the figure of kbo_derand_seq_work_bytes()); no byte beyond it is touched.
 * Errors and limits are kbo_derand_translate_seq_dev's, checked before anything is enqueued. */
size_t kbo_derand_summary_seq_work_bytes(size_t n_seqs, uint64_t total_bases, size_t k, size_t min_threshold);
int kbo_derand_summary_seq_dev(const uint8_t *d_ms, const uint64_t *d_offsets, size_t n_seqs, uint64_t total_bases, size_t k,
                               const uint32_t *d_thresholds, size_t min_threshold, kbo_aln_extent *d_out, void *d_work,
                               size_t work_bytes, void *stream);
/* kbo::map with fill_gaps = false and call_variants = false (lib.rs:726-738; format != 0: + relative_to_ref, lib.rs:756-757) or
 * kbo::matches (lib.rs:612-628; format = 0) over a device-resident batch, the whole chain MS -> derandomize_ms_vec ->
 * translate_ms_vec enqueued on `stream`; the threshold comes from the index and max_error_prob (lib.rs:620, 731).  Batches of
 * reads (max_seq_len <= 160) over an index copy that carries a depth table run as ONE kernel (kbo_amd/csrc/map_kernels.hip): the
 * MS values never leave the chip unless want_ms != 0.  Batches with LONGER sequences - contigs, whole reference sequences, long reads:
 * what kbo::map / matches / find are called with (lib.rs:612-628, 720-761) - run as one kernel too when want_ms == 0 (one wave per
 * piece of a sequence, kbo_amd/csrc/long_kernels.hip: max_seq_len > 160 or 0 = unknown; any length below 4 GiB per launch).  Other
 * batches run as kbo_ms_batch_dev + kbo_derand_translate_dev (d_work carries the scratch of both).
 * d_ms: total_bases bytes + 16, 4-byte aligned: the MS value of every base when want_ms != 0 or the batch takes the two-kernel
 * route, otherwise scratch (unspecified contents).  d_work / work_bytes as for
 * kbo_ms_batch_dev; d_concat needs 16 readable bytes of slack behind the batch.  Sequences of fewer than 3 bases (the
 * reference asserts, derandomize.rs:276) have no alignment: their bytes of d_chars_out (and d_ms) are unspecified - left unwritten by the
 * two-kernel route, overwritten by the one kernel, whose stores are whole lines - and kbo_find_batch_dev reports no run for them.  *fused (optional) = 1 when the
 * batch took the one kernel. */
int kbo_map_batch_dev(kbo_index_t *idx, const uint8_t *d_concat, const uint64_t *d_offsets, size_t n_seqs, uint64_t total_bases,
                      size_t max_seq_len, double max_error_prob, int format, int want_ms, uint8_t *d_ms, uint8_t *d_chars_out,
                      void *d_work, size_t work_bytes, void *stream, int *fused);
/* The same with the second pass - one kernel that walks the few reads the first leaves (two in ten thousand at 1 % substitutions), a wave
 * a read: a chain of dependent look-ups that takes 0.07 ms however few they are - enqueued on `tail_stream`, ordered behind the kernel on `stream` by an
 * event: a caller with several batches in flight (own d_ms / d_chars_out / d_work each) keeps `stream` busy with the next batch's
 * kernel meanwhile.  The batch's outputs are complete when BOTH streams have reached this point; whatever touches this batch's
 * buffers next - on either stream - has to be ordered behind `tail_stream`.  tail_stream == stream: kbo_map_batch_dev.  The two-kernel
 * route (*fused = 0) runs on `stream` alone.  Two such pairs of streams that take the batches in turn, two batches in flight on
 * each, keep the device fuller still (INTEGRATION.md "Several batches in flight"; bench.py: 1 034 against 679 Gbp/s at C2). */
int kbo_map_batch_dev_tail(kbo_index_t *idx, const uint8_t *d_concat, const uint64_t *d_offsets, size_t n_seqs, uint64_t total_bases,
                           size_t max_seq_len, double max_error_prob, int format, int want_ms, uint8_t *d_ms, uint8_t *d_chars_out,
                           void *d_work, size_t work_bytes, void *stream, void *tail_stream, int *fused);
/* A (stream, tail_stream) pair for kbo_map_batch_dev_tail / kbo_find_batch_dev made the way kbo_map_stream_* makes its own: `stream` -
 * the kernels' - kept off `tail_cus` compute units of the current device (-1: the library's default, 32; 0: two plain streams), the tail
 * stream a plain one: a second pass is a chain of dependent look-ups by a few hundred waves that otherwise waits for wave slots behind
 * kernels that hold them all; with units the kernels cannot take its workgroups start at once (C2, two such pairs: 757 -> 967 Gbp/s),
 * and a second pass that is work still has the whole device.  hipStream_t values; kbo_stream_pair_destroy when they are idle. */
int kbo_stream_pair_create(int tail_cus, void **stream, void **tail_stream);
void kbo_stream_pair_destroy(void *stream, void *tail_stream);
/* ---- several batches in flight, the library's own arrangement (what bench.py's headline is measured with): `pipelines` pairs of
 * (kernel stream, second-pass stream) that take the batches in turn, two slots - work and MS buffers, a completion event - per
 * pipeline, so that a batch's second pass runs beside the next batches' kernels.  When max_seq_len is 1 .. 160 over an unsharded index
 * (batches of reads) the kernels' stream is a plain one on every compute unit and the second-pass stream one of the device's highest
 * priority, the second pass in workgroups of one wave; else the pair is kbo_stream_pair_create(-1, ..)'s.  max_* size the slots' buffers: a batch may not
 * exceed them.  The batch's own buffers (d_concat, d_offsets, d_chars_out) stay the caller's and must stay valid and untouched
 * until the batch is complete.
 *   kbo_map_stream_submit   enqueues kbo::map (format != 0) / kbo::matches of one device-resident batch and returns at once;
 *                           d_ms_out (optional, padded as d_chars_out): the matching statistics of every base too, one byte a base, as
 *                           kbo_ms_batch_dev gives them (index.rs:243-256: the raw k-bounded values, NOT derandomized);
 *                           ready_stream (optional): the stream whose work so far produces the batch's inputs - the pipeline waits
 *                           for it on the device; *ticket (optional) names the batch; *fused (optional) as kbo_map_batch_dev's
 *   kbo_map_stream_wait     blocks the calling thread until that batch is complete (submit never blocks, so more batches than the
 *                           pipelines have slots may be queued: a ticket whose slot a later batch has taken is waited for through the
 *                           next batch of its pipeline that still holds one - a pipeline's batches complete in order);
 *                           kbo_map_stream_wait_on makes `stream` wait for it on the device instead;  kbo_map_stream_sync: every
 *                           batch submitted so far */
typedef struct kbo_map_stream kbo_map_stream_t;
int kbo_map_stream_create(kbo_index_t *idx, int pipelines, size_t max_seqs, uint64_t max_bases, size_t max_seq_len, kbo_map_stream_t **out);
int kbo_map_stream_submit(kbo_map_stream_t *ms, const uint8_t *d_concat, const uint64_t *d_offsets, size_t n_seqs, uint64_t total_bases,
                          size_t max_seq_len, double max_error_prob, int format, uint8_t *d_ms_out, uint8_t *d_chars_out, void *ready_stream,
                          uint64_t *ticket, int *fused);
int kbo_map_stream_wait(kbo_map_stream_t *ms, uint64_t ticket);
int kbo_map_stream_wait_on(kbo_map_stream_t *ms, uint64_t ticket, void *stream);
int kbo_map_stream_sync(kbo_map_stream_t *ms);
void kbo_map_stream_free(kbo_map_stream_t *ms);
/* kbo::find (lib.rs:808-821) over a device-resident batch: kbo_map_batch_dev_tail with format = 0, then format::run_lengths_gapped
 * (format.rs:143-193) of the characters - kbo_run_lengths_dev's buffers and record layout (d_rle_work: kbo_run_lengths_work_bytes()) -
 * enqueued behind the second pass on `tail_stream` (pass `stream` for one stream).  With max_gap_len = 0 (FindOpts' default) the one
 * kernel counts the runs of every read it finishes while the characters are in LDS, and the run lengths are ONE pass over the
 * characters instead of two (count, then emit). */
int kbo_find_batch_dev(kbo_index_t *idx, const uint8_t *d_concat, const uint64_t *d_offsets, size_t n_seqs, uint64_t total_bases,
                       size_t max_seq_len, double max_error_prob, size_t max_gap_len, uint8_t *d_ms, uint8_t *d_chars_out, void *d_work,
                       size_t work_bytes, void *d_rle_work, uint32_t *d_records, size_t capacity, void *stream, void *tail_stream, int *fused);
/* kbo::matches (lib.rs:612-628) over a device-resident PACKED batch of reads (the layout of kbo_matches_batch_packed: kbo_packed_words()
 * words, every read starts a word; d_offsets counts bases), through the one kernel's packed-native form: the words go into the kernel
 * as they are and the characters leave it as words (M, -, X, R = 0 .. 3) - a quarter of a byte per base each way; only the reads it
 * leaves to the second pass are ever unpacked.  uniform_len = the length of every read if they are all equally long, else 0;
 * d_exc_pos / d_exc_byte / n_exc: the non-ACGT list on the device (positions in base coordinates, ascending) or NULL / 0;
 * d_scratch: kbo_matches_packed_dev_scratch_bytes() bytes, 16-byte aligned; d_work / work_bytes as for kbo_ms_batch_dev;
 * tail_stream as for kbo_map_batch_dev_tail (pass `stream` for one stream).  KBO_E_UNSUPPORTED when the batch or this copy of
 * the index cannot take that kernel (reads longer than 160 bases, no depth table, a threshold below the table's order):
 * kbo_matches_batch_packed takes any batch. */
size_t kbo_matches_packed_dev_scratch_bytes(size_t n_seqs, uint64_t total_bases);
int kbo_matches_packed_dev(kbo_index_t *idx, const uint32_t *d_words, const uint64_t *d_offsets, size_t n_seqs, uint64_t total_bases,
                           size_t max_seq_len, size_t uniform_len, const uint64_t *d_exc_pos, const uint8_t *d_exc_byte, size_t n_exc,
                           double max_error_prob, uint32_t *d_words_out, void *d_scratch, void *d_work, size_t work_bytes, void *stream,
                           void *tail_stream);
/* format::run_lengths_gapped over device-resident characters (the output of kbo_derand_translate_dev
 * without d_ref), enqueued on `stream`.  d_work: kbo_run_lengths_work_bytes(n_seqs) bytes; afterwards
 * word s of d_work plus word (n_seqs + 1 + s / 1024) is the index of sequence s's first run, and the
 * last word of d_work the total number of runs.  Records are seven u32 {start, end, matches,
 * mismatches, jumps, gap_bases, gap_opens}; runs beyond `capacity` are counted but not written.
 * max_seq_len = length of the longest sequence if known (reads take LDS-staged kernels), 0 = unknown.
 * Sequences of more than 480 characters, and every sequence when max_gap_len > 0, cost one lane a sequence here, a step per
 * character: long sequences belong to kbo_run_lengths_seq_dev, below. */
size_t kbo_run_lengths_work_bytes(size_t n_seqs);
int kbo_run_lengths_dev(const uint8_t *d_chars, const uint64_t *d_offsets, size_t n_seqs, size_t max_seq_len,
                        size_t max_gap_len, void *d_work, uint32_t *d_records, size_t capacity, void *stream);
/* The same records in the same order - ordered by (sequence, start), start and end relative to the sequence - for a batch of
 * sequences of any length, any byte values and any max_gap_len (2^32 - 1 and more: no gap is too long), segmented: chunks of
 * KBO_RLE_SEG_CHUNK positions and groups of KBO_RLE_SEG_GROUP positions (kbo_hip_tuning.h), neither ever spanning two sequences,
 * are listed on the device from d_offsets; a lane per chunk steps over its characters, staged in LDS, a lane per group over its
 * chunks' summaries and a lane per sequence over that sequence's groups only.  The call enqueues 18 kernel launches and no memset
 * on `stream` whatever the batch holds, reads nothing back and returns.  Sequences of length 0 are legal.
 * d_first (n_seqs + 1 u32): d_first[s] = index of sequence s's first run, d_first[n_seqs] = the number of runs of the batch, those
 * beyond `capacity` included - a plain exclusive prefix.  Runs beyond `capacity` are counted, not written; nothing is written at or
 * behind d_records[7 * capacity] (d_records may be NULL when capacity == 0).
 * d_chars: total_bases + 16 readable bytes; d_offsets 8-byte, d_records and d_first 4-byte aligned.  d_work: required, 16-byte
 * aligned, kbo_run_lengths_seq_work_bytes() bytes - about total_bases * 77 / 128 + n_seqs * 158 bytes: per chunk of 128 positions
 * 16 bytes of descriptor, 8 of dash carry, 48 of open run and 4 of count, per group (1/64 of the chunks) 72 more, and a chunk, a
 * group and 8 bytes of listing more per sequence (0.6 bytes a position).  No byte of d_work beyond that figure is touched.
 * Errors, before anything is enqueued: KBO_E_BAD_ARG (null argument, alignment, work_bytes too small), KBO_E_EMPTY_QUERY
 * (n_seqs == 0), KBO_E_UNSUPPORTED (total_bases + 16 > 2^32, n_seqs >= 2^28). */
size_t kbo_run_lengths_seq_work_bytes(size_t n_seqs, uint64_t total_bases);
int kbo_run_lengths_seq_dev(const uint8_t *d_chars, const uint64_t *d_offsets, size_t n_seqs, uint64_t total_bases,
                            size_t max_gap_len, void *d_work, size_t work_bytes, uint32_t *d_records, size_t capacity,
                            uint32_t *d_first /* n_seqs + 1 */, void *stream);
/* The sparse form (kbo_aln_run, above) of a device-resident packed batch of kbo::matches characters - what kbo_matches_packed_dev
 * writes: kbo_packed_words() words, every sequence starts a word, M - X R = 0 .. 3; the padding bits of a sequence's last word
 * are ignored - enqueued on `stream`; the library never synchronises.  d_offsets counts bases (n_seqs + 1 entries, 8-byte
 * aligned); d_words 4-byte aligned, no slack needed.  max_seq_len = the longest sequence if known: it bounds the work (0 =
 * unknown: as many workgroups as for the largest batch), and 2^30 or more is refused (KBO_E_UNSUPPORTED; every sequence must be shorter than 2^30 bases, the batch hold fewer
 * than 2^32 - 256 words and 2^32 bases).  d_work: kbo_sparse_runs_work_bytes(n_seqs, total words) bytes, 16-byte aligned
 * (0 from it: the batch is too large).  d_runs: `capacity` records (12 bytes each, 4-byte aligned); runs beyond capacity are
 * counted but not written, and nothing past d_runs[capacity] is.  *d_n_runs (one u32, 4-byte aligned) receives the number
 * of runs of the batch; a sequence of fewer than 3 bases has none.  seq in the records = the index in this batch. */
size_t kbo_sparse_runs_work_bytes(size_t n_seqs, uint64_t total_words);
int kbo_sparse_runs_dev(const uint32_t *d_words, const uint64_t *d_offsets, size_t n_seqs, size_t max_seq_len, void *d_work,
                        kbo_aln_run *d_runs, size_t capacity, uint32_t *d_n_runs, void *stream);
/* ------------------------------------------------------------------ Positions, segments, depth: a batch in SOURCE coordinates
 * Where on the sequences an index was built from a walked sequence lies, and how deep a batch piles up on every base of them - for
 * the single-index path, at any index size (the arithmetic: kbo_amd/csrc/index_locate.hpp, the kernels:
 * kbo_amd/csrc/locate_kernels.hip).  A handle without positions behaves byte for byte as it does without this section.
 *
 * THE POSITION TABLE.  The SOURCE coordinates are those of `seqs` concatenated in order with no separator: base j of sequence s is
 * src_off[s] + j.  An OCCURRENCE of a k-mer x is (p, FWD) when x equals source[p, p + k) and (p, REV) when the reverse complement of x
 * does (REV only with add_revcomp != 0), the window inside one sequence and inside a maximal run of A, C, G, T of at least k bases.
 * The entry of x's row is the reference sets' (above): of x's occurrences the one with FWD before REV and then the smallest p, bits
 * 0 .. 29 p, bit 30 REV, bit 31 (KBO_LOCUS_MULTI) set when x has more than one occurrence; a row that is no full k-mer holds
 * KBO_POS_NONE.
 * kbo_index_add_positions makes the table on `device` (-1: the current one) from the sequences the index was built from, on any
 * unsharded handle - built, loaded, or adopted through kbo_index_from_parts: it uploads them in slabs, reverses and complements each
 * slab on the device when add_revcomp is set (kbo_revcomp_batch_dev), walks them with kbo_ms_batch_dev's interval walk - at depth k an
 * interval is one row, the row of the window that ends there - and lets a lane per base keep the smallest and the largest occurrence of
 * its row (integer atomics: the same table whatever the arrival order).  It is a build step: it allocates, synchronises and reads two
 * counters back.  Every window of every indexed stretch must reach depth k, and the rows with an entry must number
 * kbo_index_n_kmers: otherwise the sequences are not the index's (or add_revcomp is not what it was built with) and the call fails
 * with KBO_E_BAD_ARG.  A second call replaces the table; a failed one leaves the handle without positions.  Before any HIP call:
 * KBO_E_BAD_ARG for null arguments or n_seqs == 0, KBO_E_UNSUPPORTED for a sharded handle and for sources of 2^30 bases or more (p has
 * 30 bits).  The handle keeps a host copy (kbo_index_positions: out may be NULL for *n_rows alone), the copy on `device`, and src_off
 * (kbo_index_source_offsets: n_seqs + 1 values, out may be NULL for *n alone; kbo_index_source_bases is the last);
 * kbo_index_positions_bytes is what the host copy and src_off take, 0 without positions.  kbo_index_positions_to_device is idempotent
 * and the one place a further device's copy is made.  The getters give KBO_E_BAD_ARG for a handle without positions.
 * kbo_index_save and kbo_index_load do NOT carry the table: a loaded handle has none until kbo_index_add_positions is called on it.
 * kbo_positions_from_ms_host restates the table's rule on the CPU (no HIP call; a test hook and a yardstick): d and lo are the MS bytes
 * and interval starts of one strand of the sources walked sequence by sequence (`offsets`; rev != 0: of every sequence's reverse
 * complement as kbo_revcomp_batch makes it), src_off where each begins in source coordinates; every base at depth k is merged into
 * entries_inout (n_sets words, KBO_POS_NONE before the first call), one strand a call.  *n_not_full (or NULL) counts the windows of
 * the sequences that did not reach depth k.
 *
 * SEGMENTS.  An ANCHOR of a walked sequence is a position q whose window [q, q + k) has depth k at its last base; its entry is the
 * table's word for that base's row.  Of a sequence's anchors by ascending q, two neighbours a < b are JOINED when b.q - a.q <= 1 +
 * bridge, both have the same REV bit and both lie on one diagonal (FWD: p - q equal; REV: p + q equal); MULTI does not matter.  A
 * SEGMENT is a maximal chain of joined neighbours: a collinear block of exact k-mer matches.  bridge = 0 joins only adjacent windows,
 * bridge = k carries a segment across a lone substitution, bridge > 255 is KBO_E_BAD_ARG.  An insertion or deletion changes the
 * diagonal and never joins.  A MULTI k-mer is placed at its stored occurrence only, so a read inside the second copy of an exact
 * repeat is reported at the first, and a read that leaves the repeat there changes its diagonal and starts a new segment; every
 * occurrence of a MULTI k-mer needs an occurrence list the handle does not keep and is out of scope, as for the reference sets.
 * kbo_segments_dev takes what kbo_ms_batch_dev wrote with intervals (d_ms, d_lo: total_bases values; d_offsets: n_seqs + 1) and is a
 * device-resident call like the others: everything is enqueued on `stream`, nothing is synchronised, read back or allocated, and no
 * byte of d_work (16-byte aligned) beyond kbo_segments_work_bytes() - exact: a byte per base, 8 bytes per 2048 bases, 8 per 2048 of
 * those, each rounded up to 16 - is touched.  Records are in (seq, q_first) order; record x is written iff x < capacity, *d_n_segs
 * (8-byte aligned) is the full count, and nothing at or behind element `capacity` is written (d_segs may be NULL when capacity == 0).
 * `strand` is copied into the records as given.  Sequences shorter than k, or empty, contribute nothing.  Errors, before anything is
 * enqueued and in this order: KBO_E_BAD_ARG for null or misaligned pointers and for bridge > 255; KBO_E_EMPTY_QUERY for n_seqs == 0;
 * KBO_E_UNSUPPORTED for total_bases + 16 > 2^32 or n_seqs >= 2^28 and for a sharded handle; KBO_E_BAD_ARG for a handle without
 * positions, a short work_bytes, and a handle without positions on the current device.
 * kbo_segments_from_ms_host is the same call restated on the CPU (host arrays; entries: n_rows words; delta, or NULL: source_bases + 1
 * words): byte-identical records, count and delta.
 *
 * DEPTH.  Base j of the sources is covered by a FWD segment when j lies in [pos_first, pos_last + k) and by a REV segment when it lies
 * in [pos_last, pos_first + k); DEPTH[j] is the number of segments that cover j, over every call that added to the same delta array -
 * a read counts once per base however many of its k-mers cover it, which is what tells it from kbo_cover_refset's D.  With d_delta !=
 * NULL (kbo_index_source_bases + 1 words, zeroed once by the caller, shared by any number of batches and strands) the anchor that
 * starts a segment and the anchor that ends it do one integer atomic add each: +1 where the covered range begins and -1 behind it.
 * kbo_depth_finish_dev writes the inclusive prefix sums of delta to d_depth (source_bases words): exact modulo 2^32 and independent
 * of the order of the batches.  d_work: kbo_depth_work_bytes(idx), 4 bytes per 2048 bases rounded up to 16; 0 for a handle without
 * positions.  KBO_E_BAD_ARG for null or misaligned pointers, a handle without positions and a short work_bytes.
 *
 * kbo_segments_batch is the host form: upload, the '-' strand made on the device (in the coordinates of the reverse-complemented
 * sequence, as everywhere), the interval walk, kbo_segments_dev's kernels per strand - once to count, once to write - the depth
 * finish, one download.  *segs is malloc'ed (kbo_free), in (seq, strand with KBO_STRAND_FWD first, q_first) order; depth_out (or
 * NULL) receives source_bases words, written, not added to.  Errors: KBO_E_BAD_ARG for strands outside 1 .. 3, null arguments and
 * bridge > 255, KBO_E_UNSUPPORTED for a sharded handle, KBO_E_BAD_ARG for a handle without positions, then the batch as
 * kbo_find_batch_strands checks it. */
typedef struct {
    uint32_t seq, strand;         /* index in the batch; the strand argument as given */
    uint32_t q_first, q_last;     /* first base of the first / last anchor's k-mer in the sequence */
    uint32_t pos_first, pos_last; /* their entries' p, source coordinates */
    uint32_t flags;               /* bit 0: REV; bit 2 / 3: the first / last anchor's entry is MULTI */
} kbo_seq_segment;                /* 28 bytes */
int kbo_index_add_positions(kbo_index_t *idx, const uint8_t *const *seqs, const size_t *lens, size_t n_seqs, int add_revcomp, int device);
int kbo_index_has_positions(const kbo_index_t *idx);        /* 1 or 0 */
uint64_t kbo_index_positions_bytes(const kbo_index_t *idx);
int kbo_index_positions(const kbo_index_t *idx, uint32_t *out, size_t *n_rows);
int kbo_index_source_offsets(const kbo_index_t *idx, uint64_t *out, size_t *n);
uint64_t kbo_index_source_bases(const kbo_index_t *idx);
int kbo_index_positions_to_device(kbo_index_t *idx, int device);
int kbo_positions_from_ms_host(uint32_t k, uint64_t n_sets, const uint8_t *d, const uint32_t *lo, const uint64_t *offsets, size_t n_seqs,
                               const uint64_t *src_off, int rev, uint32_t *entries_inout, uint64_t *n_not_full);
size_t kbo_segments_work_bytes(size_t n_seqs, uint64_t total_bases);
int kbo_segments_dev(kbo_index_t *idx, const uint8_t *d_ms, const uint32_t *d_lo, const uint64_t *d_offsets, size_t n_seqs, uint64_t total_bases,
                     uint32_t bridge, uint32_t strand, kbo_seq_segment *d_segs, size_t capacity, uint64_t *d_n_segs, uint32_t *d_delta,
                     void *d_work, size_t work_bytes, void *stream);
int kbo_segments_from_ms_host(const uint32_t *entries, uint64_t n_rows, uint32_t k, const uint8_t *d, const uint32_t *lo,
                              const uint64_t *offsets, size_t n_seqs, uint32_t bridge, uint32_t strand, kbo_seq_segment *segs, size_t capacity,
                              uint64_t *n_segs, uint32_t *delta, uint64_t source_bases);
size_t kbo_depth_work_bytes(const kbo_index_t *idx);
int kbo_depth_finish_dev(kbo_index_t *idx, const uint32_t *d_delta, uint32_t *d_depth, void *d_work, size_t work_bytes, void *stream);
int kbo_segments_batch(kbo_index_t *idx, const uint8_t *concat, const uint64_t *offsets, size_t n_seqs, uint32_t bridge, int strands,
                       kbo_seq_segment **segs, uint64_t *n_segs, uint32_t *depth_out);
/* ------------------------------------------------------------------ Placement: the segments of a sequence chained to ONE record
 * Where a sequence lies: on which source and strand, how much of it, and how clear that is (the arithmetic:
 * kbo_amd/csrc/index_place.hpp, the kernels: kbo_amd/csrc/place_kernels.hip).  A read with a substitution is two segments at bridge 0,
 * a read with an insertion or deletion two at any bridge, a 10 kbp read a few hundred; this step chains them on the device.
 *
 * DEFINITIONS.  Take the segments of one sequence from one kbo_segments_dev call (one strand argument), s_0 .. s_{n-1} in list order;
 * they are disjoint stretches of the anchor list, so q_last of s_j is below q_first of s_i for j < i.  For a segment: len = q_last -
 * q_first + k (the query bases it covers); rev = flag bit 0; diag = pos_first - q_first (FWD) or pos_first + q_first (REV) as a 64-bit
 * signed value, constant over the segment; src = the last source s with src_off[s] <= pos_first.
 * s_j MAY PRECEDE s_i iff all of: i - W <= j < i with W = KBO_PLACE_WINDOW = 64; the same rev and the same src; g = q_first_i -
 * q_last_j <= max_gap; and with shift = diag_i - diag_j (FWD) or diag_j - diag_i (REV) - the bases the source advances beyond the query:
 * > 0 a deletion in the sequence, < 0 an insertion - |shift| <= max_indel and g + shift >= 1 (the source advances).
 * gain(j, i) = min(len_i, q_last_i - q_last_j).
 * CHAINS.  f_i = max(len_i, max over the j that may precede i of f_j + gain(j, i)).  The predecessor taken is the one with the largest
 * value, ties to the larger j; there is none when len_i is at least that value.  Every segment carries along its chain the chain's
 * first segment (its ROOT), the number of segments, the sum of |shift| and the number of its segments with a MULTI flag at either end.
 * With at most W segments the recurrence is the exact maximum over all chains the rule allows; beyond, predecessors further back
 * than W are not looked at.
 * THE PLACEMENT of the sequence is the chain that ends at the i with the largest f, ties to the smaller i.  `second` is the largest f_i
 * over all i whose root differs from the best chain's root, 0 when there is none: chains of one root share a prefix with the best one
 * and are not a second placement.  A MULTI k-mer is placed at its stored occurrence only (SEGMENTS, above), so `second` does not see
 * the other copy of an exact repeat: n_multi is there to say that the chain rests on k-mers that occur elsewhere too.
 * MERGE.  Two records of one sequence merge to the one with the larger score, ties to the smaller strand value (then, for two calls
 * with one strand value, to the smaller of the remaining fields in their order); its `second` becomes the largest of both `second`s and
 * the loser's score.  A KBO_PLACE_NONE record loses to anything.  The merge is associative and commutative: the record is its own
 * reduction state, as kbo_ref_best is.
 *
 * kbo_place_dev takes d_segs, d_n_segs and capacity exactly as kbo_segments_dev leaves them and uses min(*d_n_segs, capacity) records,
 * read on the device.  It is a device-resident call like the others: at most four launches on `stream` - the ranges cleared; a lane per record
 * for its source (a bisection of the device copy of src_off that kbo_index_add_positions / kbo_index_positions_to_device make beside the
 * table) and the range of its sequence; a lane per sequence that chains a list of at most KBO_PLACE_LANE_MAX = 4 segments in registers;
 * a wave per sequence with a longer list, the up to 64 predecessors of a step one to a lane - nothing is synchronised, read back or
 * allocated, and the route is chosen per sequence on the device.  Both routes write the same bytes.  No byte of d_work (16-byte aligned)
 * beyond kbo_place_work_bytes(n_seqs, capacity) - exact: three times 4 bytes per sequence and 4 bytes per record of capacity, each
 * rounded up to 16, and 16 - or of d_place (16-byte aligned) beyond n_seqs records is touched.  merge != 0: every record is merged into
 * what d_place holds (the second strand's call); merge == 0: d_place is written, not read.  Whatever the records hold, no load or store
 * leaves the caller's buffers and the handle's table: a record whose seq is not its range's, or is at least n_seqs, is skipped, and the
 * result for a list that is not in (seq, q_first) order is unspecified but in bounds.  d_segs may be NULL when capacity == 0 (every
 * record is then KBO_PLACE_NONE).  Errors, before anything is enqueued and in this order: KBO_E_BAD_ARG for null or misaligned
 * pointers (d_segs 4-byte, d_n_segs 8-byte, d_place and d_work 16-byte); KBO_E_EMPTY_QUERY for n_seqs == 0; KBO_E_UNSUPPORTED for
 * n_seqs >= 2^28 or capacity >= 2^32 - 1 and for a sharded handle; KBO_E_BAD_ARG for a handle without positions, for one without
 * positions on the current device, and for a short work_bytes.  kbo_place_work_bytes is 0 for n_seqs == 0 and beyond those limits.
 * kbo_place_from_segments_host is the same call restated on the CPU (no HIP call; src_off: n_src + 1 values as
 * kbo_index_source_offsets gives them): byte-identical records, for any list.  KBO_E_BAD_ARG for null arguments (segs may be NULL when
 * n_segs == 0), k == 0, n_src == 0 and src_off that does not start at 0 or descends; KBO_E_EMPTY_QUERY for n_seqs == 0;
 * KBO_E_UNSUPPORTED beyond the limits above.
 * kbo_place_batch is the host form: upload, the '-' strand made on the device, the interval walk, kbo_segments_dev (once to count,
 * once to write) and kbo_place_dev per strand - the second with merge - and one download of n_seqs records to place_out.  Errors as
 * kbo_segments_batch. */
#define KBO_PLACE_NONE 0xFFFFFFFFu
#define KBO_PLACE_WINDOW 64
#define KBO_PLACE_LANE_MAX 4
#define KBO_PLACE_REV 1u
#define KBO_PLACE_SPILLS 2u
typedef struct {
    uint32_t source;             /* the root's src; KBO_PLACE_NONE when the sequence has no segment: every other field is then 0 */
    uint16_t strand;             /* the strand argument of the call that won (its low 16 bits), as the best chain's last record holds it */
    uint16_t flags;              /* bit 0 REV; bit 1 SPILLS: pos_end > src_off[source + 1], the chain runs across a junction of adjacent
                                    sources, which the segments' definition allows */
    uint32_t q_start, q_end;     /* the root's q_first; the end's q_last + k */
    uint32_t pos_start, pos_end; /* source coordinates, half open.  FWD: the root's pos_first, the end's pos_last + k; REV: the end's
                                    pos_last, the root's pos_first + k */
    uint32_t score;              /* f */
    uint32_t n_segs, indel, n_multi; /* as the chain carried them */
    uint32_t second;
    uint32_t reserved;           /* 0 */
} kbo_seq_place;                 /* 48 bytes */
size_t kbo_place_work_bytes(size_t n_seqs, size_t n_segs_capacity);
int kbo_place_dev(kbo_index_t *idx, const kbo_seq_segment *d_segs, const uint64_t *d_n_segs, size_t capacity, size_t n_seqs, uint32_t max_gap,
                  uint32_t max_indel, int merge, kbo_seq_place *d_place, void *d_work, size_t work_bytes, void *stream);
int kbo_place_from_segments_host(const kbo_seq_segment *segs, uint64_t n_segs, size_t n_seqs, const uint64_t *src_off, size_t n_src, uint32_t k,
                                 uint32_t max_gap, uint32_t max_indel, int merge, kbo_seq_place *place);
int kbo_place_batch(kbo_index_t *idx, const uint8_t *concat, const uint64_t *offsets, size_t n_seqs, uint32_t bridge, int strands,
                    uint32_t max_gap, uint32_t max_indel, kbo_seq_place *place_out);
/* ------------------------------------------------------------------ Pileup: what the reads SAY at every source base, candidate sites
 * DEPTH says that 31 reads cover source base j; this section says that 29 of them carry a T there where the source has a C (DESIGN.md
 * 4.15; the arithmetic: kbo_amd/csrc/index_pileup.hpp, the kernels: kbo_amd/csrc/pileup_kernels.hip).  A segment fixes a diagonal, so
 * every base inside its extent has one source coordinate, and the only bases that can differ from the source are the ones no exact
 * k-mer window of the segment covers: about 1 % of the bases at 1 % divergence.  A pileup is one integer atomic per such base.
 *
 * DEFINITIONS.  Take the records of one kbo_segments_dev call, the batch as it was walked (d_concat, d_offsets; for the '-' strand
 * the reverse-complemented batch, as everywhere) and the MS bytes that walk wrote (d_ms).
 * ANCHORS AND BRIDGED BASES.  For a record with sequence s and o = offsets[s], a window w in [q_first, q_last] is an ANCHOR iff
 * ms[o + w + k - 1] == k; every such anchor belongs to the segment, segments being maximal stretches of the anchor list.  A base x in
 * [q_first, q_last + k) is COVERED when some anchor a has a <= x < a + k, and BRIDGED otherwise.  Equivalently, for a record as
 * kbo_segments_dev writes it: for consecutive anchors a < b with b - a > k the bridged bases are a + k .. b - 1.
 * PROJECTION.  A bridged base x of a FWD record is counted at j = pos_first + (x - q_first) as the byte at x; of a REV record (flag bit
 * 0) at j = pos_first + k - 1 - (x - q_first) as the complement of the byte at x.  Base codes: A, C, G, T = 0 .. 3 as kbo_pack_reads
 * codes them; every other byte (N, lower case) is counted in no column.
 * THE PILE is uint32_t pile[source_bases][4] (16-byte aligned), zeroed once by the caller and shared by any number of batches and
 * strands, exactly like d_delta; it is added to by integer atomics, so the result is the same whatever the arrival order.
 * skip_multi != 0 leaves out a record whose flags hold either MULTI bit: a k-mer that also occurs elsewhere is placed at its stored
 * occurrence only, which is evidence a SNP caller does not want.
 * RECORDS THAT HOLD ANYTHING.  A record contributes nothing when seq >= n_seqs, when q_first > q_last, when o + q_last + k is past the
 * sequence's end, or when the sequence's offsets descend or end beyond total_bases; a single projected j outside [0, source_bases)
 * is skipped.  No load or store leaves the caller's buffers.  The host form applies the same rules: host and device agree byte for byte
 * on any list.
 * RELATION TO DEPTH.  When d_delta was accumulated by the same kbo_segments_dev calls, the sum over b of pile[j][b] is at most
 * DEPTH[j] for every j, and DEPTH[j] minus that sum is the number of reads that match the source exactly at j plus those whose
 * bridged byte there is no base.
 * SITES.  Base j is a SITE iff some b has pile[j][b] >= min_count and pile[j][b] * frac_den >= frac_num * DEPTH[j], the products in 64
 * bits; frac_den == 0 or min_count == 0 is KBO_E_BAD_ARG.  A column that equals the source base can qualify - a base between two
 * nearby substitutions is bridged too - and the device does not hold the source text: the caller drops that column
 * (kbo_amd.pileup_snps).  One kbo_pile_site is 32 bytes: pos in source coordinates, source by a bisection of the device copy of src_off
 * (the last source whose offset is <= pos), depth, count[4], reserved = 0.  Sites are in ascending pos; record x is written iff x <
 * capacity, *d_n_sites (8-byte aligned) is the full count, nothing at or behind element `capacity` is touched.
 *
 * kbo_pileup_dev uses min(*d_n_segs, capacity) records, read on the device, as kbo_place_dev does, and is a device-resident call like
 * the others: ONE launch on `stream` - waves stride over the records, a wave takes a record's windows 64 at a time, a lane loads one
 * MS byte, one ballot gives the anchors, the lane of an anchor counts the bridged bases in front of it - that allocates nothing,
 * synchronises nothing and reads nothing back.  It takes no scratch.  d_concat and d_ms: total_bases bytes; d_offsets: n_seqs + 1
 * values; d_pile is added to, never cleared.  d_segs may be NULL when capacity == 0.  Errors, before anything is enqueued and in this
 * order: KBO_E_BAD_ARG for null or misaligned pointers (d_segs 4-byte, d_offsets and d_n_segs 8-byte, d_pile 16-byte);
 * KBO_E_EMPTY_QUERY for n_seqs == 0; KBO_E_UNSUPPORTED for total_bases + 16 > 2^32, n_seqs >= 2^28 or capacity >= 2^32 - 1 and for a
 * sharded handle; KBO_E_BAD_ARG for a handle without positions and for one without positions on the current device.
 * kbo_pileup_sites_dev is flag, scan, emit - the plain three-pass scan of kbo_segments_dev and kbo_depth_finish_dev, three launches,
 * no workgroup waits for another - over d_pile and d_depth (source_bases words, as kbo_depth_finish_dev wrote them).  No byte of
 * d_work beyond kbo_pileup_sites_work_bytes(idx) - exact: 4 bytes per 2048 source bases rounded up to 16, at least 16; 0 for a handle
 * without positions - or of d_sites beyond `capacity` records is touched; d_sites may be NULL when capacity == 0.  Errors, in this
 * order: KBO_E_BAD_ARG for null or misaligned pointers (d_depth 4-byte, d_n_sites 8-byte, d_pile, d_sites and d_work 16-byte) and for
 * min_count == 0 or frac_den == 0; KBO_E_UNSUPPORTED for a sharded handle; KBO_E_BAD_ARG for a handle without positions, for one
 * without positions on the current device, and for a short work_bytes.
 * kbo_pileup_from_segments_host and kbo_pileup_sites_host are the two calls restated on the CPU (no HIP call; host arrays; src_off:
 * n_src + 1 values as kbo_index_source_offsets gives them): byte-identical pile, sites and count, for any list.  *n_bridged (or NULL)
 * receives the bridged bases of the records taken, counted in a column or not.  KBO_E_BAD_ARG for null arguments (segs may be NULL
 * when n_segs == 0, sites when capacity == 0), k == 0, n_src == 0, the two thresholds and src_off that does not start at 0 or
 * descends; KBO_E_EMPTY_QUERY for n_seqs == 0; KBO_E_UNSUPPORTED beyond the limits above and for sources of 2^30 bases or more.
 * kbo_pileup_batch is the host form: upload, the '-' strand made on the device, the interval walk, kbo_segments_dev (once to count,
 * once to write, with one delta for all strands) and kbo_pileup_dev per strand into one pile, the depth finish, the sites (once to
 * count, once to write), one download.  *sites is malloc'ed (kbo_free); depth_out (source_bases words) and pile_out (4 * source_bases
 * words) may be NULL and are written, not added to.  Errors as kbo_segments_batch, the two threshold checks behind bridge > 255. */
typedef struct {
    uint32_t pos;      /* source coordinates */
    uint32_t source;   /* the last source whose offset is <= pos */
    uint32_t depth;    /* DEPTH[pos] */
    uint32_t count[4]; /* pile[pos][A, C, G, T] */
    uint32_t reserved; /* 0 */
} kbo_pile_site;       /* 32 bytes */
int kbo_pileup_dev(kbo_index_t *idx, const uint8_t *d_concat, const uint8_t *d_ms, const uint64_t *d_offsets, size_t n_seqs, uint64_t total_bases,
                   const kbo_seq_segment *d_segs, const uint64_t *d_n_segs, size_t capacity, int skip_multi, uint32_t *d_pile, void *stream);
size_t kbo_pileup_sites_work_bytes(const kbo_index_t *idx);
int kbo_pileup_sites_dev(kbo_index_t *idx, const uint32_t *d_pile, const uint32_t *d_depth, uint32_t min_count, uint32_t frac_num, uint32_t frac_den,
                         kbo_pile_site *d_sites, size_t capacity, uint64_t *d_n_sites, void *d_work, size_t work_bytes, void *stream);
int kbo_pileup_from_segments_host(const kbo_seq_segment *segs, uint64_t n_segs, const uint8_t *concat, const uint8_t *ms, const uint64_t *offsets,
                                  size_t n_seqs, uint64_t total_bases, uint32_t k, int skip_multi, uint32_t *pile, uint64_t source_bases,
                                  uint64_t *n_bridged);
int kbo_pileup_sites_host(const uint32_t *pile, const uint32_t *depth, uint64_t source_bases, const uint64_t *src_off, size_t n_src, uint32_t min_count,
                          uint32_t frac_num, uint32_t frac_den, kbo_pile_site *sites, size_t capacity, uint64_t *n_sites);
int kbo_pileup_batch(kbo_index_t *idx, const uint8_t *concat, const uint64_t *offsets, size_t n_seqs, uint32_t bridge, int strands, int skip_multi,
                     uint32_t min_count, uint32_t frac_num, uint32_t frac_den, kbo_pile_site **sites, uint64_t *n_sites, uint32_t *depth_out,
                     uint32_t *pile_out);
/* ------------------------------------------------------------------ Indels: junction events in source coordinates, counted sites
 * The pileup sees substitutions; an insertion or deletion inside a read changes the diagonal, so it is TWO consecutive records of
 * kbo_segments_dev on one strand with nothing bridged between them (the arithmetic: kbo_amd/csrc/index_indel.hpp, the
 * kernels: kbo_amd/csrc/indel_kernels.hip).  This section turns every clean junction into one EVENT, collects the events of any number
 * of batches and strands in one list, and counts the list into SITES behind the depth finish.
 *
 * DEFINITIONS.  Take the records of ONE kbo_segments_dev call in list order and the batch as it was walked (d_concat, d_offsets; for
 * the '-' strand the reverse-complemented batch, as everywhere).
 * INTERVALS of a record s, rev = flag bit 0: the query interval Q(s) = [q_first, q_last + k); the source interval S(s) =
 * [pos_first, pos_last + k) FWD, [pos_last, pos_first + k) REV.
 * A PAIR is records x - 1 = A and x = B.  It counts when both hold something by the pileup's rules (RECORDS THAT HOLD ANYTHING above,
 * skip_multi included), both have the same seq and the same rev, and A.q_last < B.q_first.  FWD: lower = A, upper = B; REV: lower = B,
 * upper = A.  In signed 64 bits: gq = B.q_first - (A.q_last + k); gs = S(upper).lo - S(lower).hi; shift = gs - gq, which is
 * kbo_place_dev's shift.
 * EVENTS.  shift == 0, or |shift| > max_indel: nothing (a max_indel above 2^30 - 1 counts as 2^30 - 1: a len has 30 bits).
 * gq > 0 and gs > 0 together: a COMPLEX junction, an indel with a mismatch next to it - counted by the host form in *n_complex, never
 * written.  Otherwise shift > 0 (then gq <= 0: no unmatched read base lies between the segments) is a DELETION with len = shift and
 * pos = S(upper).lo - len, and shift < 0 (then gs <= 0) an INSERTION with len = -shift and pos = S(upper).lo, the source base in
 * front of which the bases go.  pos is the LEFT-ALIGNED placement: the upper segment extends down exactly as far as the read matches
 * its diagonal, so the event depends on `upper` and `shift` alone, and two reads that carry the same indel inside a homopolymer get
 * the same key.
 * THE INSERTED BASES in source orientation are, FWD, the bytes [B.q_first - len, B.q_first) of the sequence and, REV, the reverse
 * complement of the bytes [A.q_last + k, A.q_last + k + len).  For len <= KBO_INDEL_CODE_LEN = 16, `code` packs base i in ascending
 * source order at bits [2i, 2i + 2), coded as kbo_pack_reads codes them (A, C, G, T = 0 .. 3); for len > 16, code = 0 and the LONG
 * bit is set: such insertions are told apart by position and length only.  A deletion's code is 0.
 * NO EVENT is written when an inserted byte is not A, C, G or T; when those bytes would leave the sequence; when pos < 0; when
 * pos + (deletion ? len : 0) > source_bases; or when S(upper).lo and S(lower).hi - 1 lie in different sources (the last source whose
 * offset is <= the value, by bisection of the device copy of src_off).
 * kbo_indel_event, 16 bytes: pos; kind_len = len | LONG << 30 | INS << 31; code; flags, bit 0 MINUS - the read lies on the source's
 * '-' strand: rev XOR (the record's strand field == KBO_STRAND_REV) - the other bits 0.
 * THE LIST.  The events of a call are APPENDED behind the *d_n_events already in the list, in record order: event n of the list is
 * written iff n < event_capacity, and *d_n_events (8-byte aligned, zeroed once by the caller, shared by batches and strands like
 * d_delta) becomes the full count.  The order is deterministic, so the list is byte-comparable with the host form's.
 * SITES.  Of the first min(*d_n_events, event_capacity) events, those that hold an event - flags <= 1, len >= 1, pos <= source_bases,
 * a deletion with code == 0, no LONG bit and pos + len <= source_bases, an insertion with LONG set iff len > 16, code == 0 when LONG
 * and code < 4^len otherwise; every other word pattern is skipped - are grouped by (pos, kind_len, code).  A group is a SITE iff
 * count >= min_count and count * frac_den >= frac_num * depth, the products in 64 bits; min_count == 0 or frac_den == 0 is
 * KBO_E_BAD_ARG.  kbo_indel_site, 32 bytes: pos, source (the last source whose offset is <= pos), kind_len, code, count (the events
 * of the group), n_minus (those with MINUS), depth = DEPTH[pos - 1] for pos > 0, else DEPTH[0] - the base in front of the event,
 * which reads with and without the indel both cover - and reserved = 0.  Sites come in ascending (pos, kind_len, code) order as
 * unsigned words; site x is written iff x < site_capacity and *d_n_sites is the full count.  The sites do not depend on the order of
 * the events in the list.
 *
 * kbo_indels_dev uses min(*d_n_segs, capacity) records, read on the device, and is a device-resident call like its neighbours: flag,
 * scan, emit - the plain three-pass scan, THREE launches on `stream` sized by `capacity` alone (none at capacity == 0), a lane per
 * record x >= 1 that evaluates its pair and loads an insertion's bytes; nothing is allocated, synchronised or read back.  No byte of
 * d_work (16-byte aligned) beyond kbo_indels_work_bytes(capacity) - exact: 4 bytes per 2048 records of capacity rounded up to 16, and
 * 16 - or of d_events beyond event_capacity records is touched.  d_segs may be NULL at capacity == 0, d_events at event_capacity == 0.
 * Whatever the records hold, no load or store leaves the caller's buffers.  Errors, before anything is enqueued and in this order:
 * KBO_E_BAD_ARG for null or misaligned pointers (d_segs 4-byte; d_offsets, d_n_segs and d_n_events 8-byte; d_events and d_work
 * 16-byte) and max_indel == 0; KBO_E_EMPTY_QUERY for n_seqs == 0; KBO_E_UNSUPPORTED for total_bases + 16 > 2^32, n_seqs >= 2^28,
 * capacity or event_capacity >= 2^32 - 1 and for a sharded handle; KBO_E_BAD_ARG for a handle without positions, for one without
 * positions on the current device, and for a short work_bytes.
 * kbo_indel_sites_dev: the events become sort keys of two 64-bit words, the places [n, event_capacity) padded with keys of all ones
 * so that the sort's size is a host value; a stable LSD radix sort of 8-bit digits over the key bits a pos <= source_bases, kind_len
 * and code can set - P = ceil((64 + bits of source_bases) / 8) passes of four launches; the group heads flagged and scanned together
 * with the MINUS bits in one 64-bit word, count and n_minus taken as differences at the next head; the threshold, a second scan, the
 * records.  7 + 4 P launches on `stream` (4 at event_capacity == 0), sized by event_capacity alone.  No byte of d_work beyond
 * kbo_indel_sites_work_bytes(event_capacity) - exact, with n = event_capacity and every part rounded up to 16: 32 n for the keys and
 * the sort's other buffer, 1024 bytes per 4096 keys of n for the passes' histogram and 4 bytes per 1024 words of that, + 8, for its
 * sums, 8 (n + 1) for the groups, 8 bytes per 2048 of n + 1 and 4 bytes per 2048 of n for the two scans' sums, and 16 - or of d_sites
 * beyond site_capacity records is touched.  d_events may be NULL at event_capacity == 0, d_sites at site_capacity == 0.  Errors, in
 * this order: KBO_E_BAD_ARG for null or misaligned pointers (d_depth 4-byte; d_n_events and d_n_sites 8-byte; d_events, d_sites and
 * d_work 16-byte) and the two thresholds; KBO_E_UNSUPPORTED for event_capacity >= 2^32 - 1 and a sharded handle; KBO_E_BAD_ARG for a
 * handle without positions, for one without positions on the current device, and for a short work_bytes.  Both work-size functions
 * give 0 beyond their limit.
 * kbo_indels_from_segments_host and kbo_indel_sites_host are the two calls restated on the CPU (no HIP call; host arrays; src_off:
 * n_src + 1 values as kbo_index_source_offsets gives them, the last one being source_bases; depth: that many words): byte-identical
 * events, sites and counts, for any list.  *n_events is read and grows like *d_n_events; *n_complex (or NULL) grows by the COMPLEX
 * junctions.  KBO_E_BAD_ARG for null arguments (segs may be NULL when n_segs == 0, events at event_capacity == 0, sites at
 * site_capacity == 0), k == 0, n_src == 0, max_indel == 0, the two thresholds, and src_off that does not start at 0 or descends;
 * KBO_E_EMPTY_QUERY for n_seqs == 0; KBO_E_UNSUPPORTED beyond the limits above and for sources of 2^30 bases or more.
 * kbo_indels_batch is the host form, built from the stages of kbo_pileup_batch: upload, the '-' strand made on the device, the
 * interval walk, kbo_segments_dev (once to count, once to write, with one delta for all strands), the events of every strand into one
 * list, the depth finish, the sites (once to count, once to write), one download.  *sites is malloc'ed (kbo_free); depth_out
 * (source_bases words) may be NULL and is written, not added to.  Errors as kbo_pileup_batch, max_indel == 0 beside the thresholds. */
#define KBO_INDEL_INS (1u << 31)
#define KBO_INDEL_LONG (1u << 30)
#define KBO_INDEL_LEN_MASK ((1u << 30) - 1u)
#define KBO_INDEL_MINUS 1u
#define KBO_INDEL_CODE_LEN 16u
typedef struct {
    uint32_t pos;      /* source coordinates: the first deleted base; the base in front of which the inserted bases go */
    uint32_t kind_len; /* len | KBO_INDEL_LONG | KBO_INDEL_INS */
    uint32_t code;     /* an insertion's bases, 2 bits each, base 0 (the lowest in source order) lowest; 0 for LONG and for deletions */
    uint32_t flags;    /* bit 0: KBO_INDEL_MINUS */
} kbo_indel_event;     /* 16 bytes */
typedef struct {
    uint32_t pos;      /* as the events of the group */
    uint32_t source;   /* the last source whose offset is <= pos */
    uint32_t kind_len, code;
    uint32_t count;    /* events in the group */
    uint32_t n_minus;  /* ... with KBO_INDEL_MINUS */
    uint32_t depth;    /* DEPTH[pos - 1]; DEPTH[0] at pos 0 */
    uint32_t reserved; /* 0 */
} kbo_indel_site;      /* 32 bytes */
size_t kbo_indels_work_bytes(size_t n_segs_capacity);
int kbo_indels_dev(kbo_index_t *idx, const uint8_t *d_concat, const uint64_t *d_offsets, size_t n_seqs, uint64_t total_bases,
                   const kbo_seq_segment *d_segs, const uint64_t *d_n_segs, size_t capacity, int skip_multi, uint32_t max_indel,
                   kbo_indel_event *d_events, size_t event_capacity, uint64_t *d_n_events, void *d_work, size_t work_bytes, void *stream);
size_t kbo_indel_sites_work_bytes(size_t event_capacity);
int kbo_indel_sites_dev(kbo_index_t *idx, const kbo_indel_event *d_events, const uint64_t *d_n_events, size_t event_capacity, const uint32_t *d_depth,
                        uint32_t min_count, uint32_t frac_num, uint32_t frac_den, kbo_indel_site *d_sites, size_t site_capacity, uint64_t *d_n_sites,
                        void *d_work, size_t work_bytes, void *stream);
int kbo_indels_from_segments_host(const kbo_seq_segment *segs, uint64_t n_segs, const uint8_t *concat, const uint64_t *offsets, size_t n_seqs,
                                  uint64_t total_bases, uint32_t k, int skip_multi, uint32_t max_indel, const uint64_t *src_off, size_t n_src,
                                  kbo_indel_event *events, size_t event_capacity, uint64_t *n_events, uint64_t *n_complex);
int kbo_indel_sites_host(const kbo_indel_event *events, uint64_t n_events, size_t event_capacity, const uint32_t *depth, const uint64_t *src_off,
                         size_t n_src, uint32_t min_count, uint32_t frac_num, uint32_t frac_den, kbo_indel_site *sites, size_t site_capacity,
                         uint64_t *n_sites);
int kbo_indels_batch(kbo_index_t *idx, const uint8_t *concat, const uint64_t *offsets, size_t n_seqs, uint32_t bridge, int strands, int skip_multi,
                     uint32_t max_indel, uint32_t min_count, uint32_t frac_num, uint32_t frac_den, kbo_indel_site **sites, uint64_t *n_sites,
                     uint32_t *depth_out);

/* ---- alignment summaries (kbo_aln_summary, above) of device-resident batches; asynchronous, the library never synchronises.
 * kbo_summary_batch_dev: kbo::matches over the batch as kbo_map_batch_dev_tail runs it (format = 0: the same routes, streams and
 * second pass on `tail_stream`; the records are complete when BOTH streams have reached this point), with d_summary_out - n_seqs records,
 * 16-byte aligned, nothing beyond them is written - as the only output.  Reads (max_seq_len 1 .. 160) over an unsharded copy with a
 * depth table: map_reads_kernel counts the characters while they are in LDS and stores a record per read, its second pass the records of
 * the reads it leaves - no character and no MS value reaches memory (*fused = 1), d_ms is not touched, and the batch is planned whatever
 * the batches before it did to the copy's plan.  Every other batch - longer sequences, no depth table, a sharded index - runs as
 * kbo_map_batch_dev_tail does (*fused as there) with the characters in d_work, and a reducer (summary_kernels.hip) counts them there.
 * d_ms: total_bases + 16 bytes, 4-byte aligned (scratch of those routes).  d_work: kbo_summary_work_bytes() bytes, 16-byte aligned -
 * exact for the route the batch takes on the current device: what the walk needs for the one kernel, kbo_index_work_bytes() plus the
 * characters (total_bases + 16, rounded up to 64) otherwise.  What "exact" rests on: the route is decided from the index's copy on the
 * current device and the process-wide settings AT THE TIME OF THE QUERY - the query makes that copy (an upload, as kbo_index_to_device) if
 * there is none yet, so that the copy's depth table and path cover are there to be looked at - and kbo_summary_batch_dev decides again by
 * the same rule.  Both agree as long as kbo_set_plan, kbo_set_plan_stats - counted batches take the second route -, the handle's depth-table
 * option and the environment's KBO_MAP_FINISH are not changed in between; the copy's hold-off after a batch that gave its plan up does
 * NOT change the route.  When they disagree nothing is overrun: a d_work smaller than the batch's route needs is refused with
 * KBO_E_BAD_ARG, a larger one is accepted.  A caller that wants one size for any route takes the larger figure:
 * kbo_index_work_bytes() + total_bases + 16 rounded up to 64, + 64.  0 = bad arguments.  Errors as kbo_map_batch_dev_tail. */
size_t kbo_summary_work_bytes(kbo_index_t *idx, size_t n_seqs, uint64_t total_bases, size_t max_seq_len);
int kbo_summary_batch_dev(kbo_index_t *idx, const uint8_t *d_concat, const uint64_t *d_offsets, size_t n_seqs, uint64_t total_bases,
                          size_t max_seq_len, double max_error_prob, uint8_t *d_ms, kbo_aln_summary *d_summary_out, void *d_work,
                          size_t work_bytes, void *stream, void *tail_stream, int *fused);
/* The reducer alone, for characters the caller already has: one byte a character at d_chars + d_offsets[s] (kbo_matches_batch's
 * M - X R; any other byte counts as none of the three and does not end a run; d_chars of any alignment, no slack needed; d_offsets[0]
 * need not be 0 - only the aligned 16-byte blocks that hold a character of a sequence are read), or
 * (kbo_summary_words_dev) the 2-bit character words of kbo_matches_batch_packed / kbo_matches_packed_dev.  A sequence of fewer than 3
 * bases gets zeros whatever its characters are.  Sequences of any length: a wave takes 1 KiB of characters, a contig is reduced by as
 * many waves as it has KiB and a run that crosses from one to the next is counted once.  max_seq_len = the longest sequence if known
 * (it bounds the grid), 0 = unknown.  d_summary_out: n_seqs records, 16-byte aligned; d_offsets 8-byte aligned.  kbo_summary_words_dev's
 * d_work: kbo_summary_words_work_bytes(n_seqs) bytes, 16-byte aligned (0 from it: too many sequences). */
int kbo_summary_dev(const uint8_t *d_chars, const uint64_t *d_offsets, size_t n_seqs, size_t max_seq_len, kbo_aln_summary *d_summary_out,
                    void *stream);
size_t kbo_summary_words_work_bytes(size_t n_seqs);
int kbo_summary_words_dev(const uint32_t *d_words, const uint64_t *d_offsets, size_t n_seqs, size_t max_seq_len, kbo_aln_summary *d_summary_out,
                          void *d_work, void *stream);
/* kbo_map_stream_submit for a summary batch: the same pipelines, slots and tickets (kbo_map_stream_wait / _wait_on / _sync); a stream
 * takes character batches and summary batches in any order.  d_summary_out as for kbo_summary_batch_dev; the slots' buffers serve as
 * d_work and d_ms (a batch that does not take the one kernel keeps its characters in a buffer the slot gets when the first summary batch
 * that takes that route comes - a hipMalloc inside that one submit; streams of reads never make it). */
int kbo_map_stream_submit_summary(kbo_map_stream_t *ms, const uint8_t *d_concat, const uint64_t *d_offsets, size_t n_seqs, uint64_t total_bases,
                                  size_t max_seq_len, double max_error_prob, kbo_aln_summary *d_summary_out, void *ready_stream,
                                  uint64_t *ticket, int *fused);
/* Options of ONE index handle: what the process-wide setters below and in kbo_hip_tuning.h (kbo_set_devices, kbo_set_slab_bytes,
 * kbo_set_plan, kbo_set_depth_table, kbo_set_depth_table_anchors) decide for every index, decided for this one - two indexes of one
 * process (a small reference next to a large one; a service with one handle per tenant) no longer share them.  A field left at its
 * "inherit" value follows the process-wide setting at the time of use.  Set them before the handle's first batch / before
 * kbo_index_to_device: like the process-wide setters, depth_table* shape device copies made from then on (an existing copy keeps
 * its table; depth_table = -1 makes launches ignore it), plan = 0 stops planned launches at once, devices and slab_bytes apply to
 * the next host batch.  Not to be changed while a batch of this handle is in flight on another thread.  A sharded index hands its
 * options on to its shards. */
#define KBO_OPT_INHERIT (-2147483647 - 1)
#define KBO_OPT_MAX_DEVICES 16
typedef struct kbo_index_opts {
    uint32_t struct_size;        /* sizeof(kbo_index_opts_t), as filled in by kbo_index_opts_default: the struct may grow */
    int32_t plan;                /* KBO_OPT_INHERIT | 0 = plain walk only | 1 = path cover + tables on its device copies, planned launches */
    int32_t depth_table;         /* KBO_OPT_INHERIT | 0 = order by index size | -1 = none | 1 .. 17 = bases per entry */
    int32_t depth_table_anchors; /* KBO_OPT_INHERIT | -1 = by the table's margin over log4(rows) | 0 = no | 1 = yes */
    uint64_t slab_bytes;         /* 0 = inherit | query bytes per slab of its host batches (clamped to 64 KiB .. 3.75 GiB) */
    int32_t n_devices;           /* -1 = inherit | 0 = the current device | 1 .. 16 = devices[0 .. n) */
    int32_t devices[KBO_OPT_MAX_DEVICES];
} kbo_index_opts_t;
int kbo_index_opts_default(kbo_index_opts_t *opts); /* every field "inherit" */
int kbo_index_set_opts(kbo_index_t *idx, const kbo_index_opts_t *opts);
int kbo_index_get_opts(const kbo_index_t *idx, kbo_index_opts_t *opts);
/* Devices the host batch entry points (kbo_matches_batch / kbo_map_batch / kbo_find_batch) spread
 * their slabs over: index replicated per device, one submitting + one completing host thread and
 * three stage streams (upload, kernels, download) per device, disjoint output slices, no collective.
 * n = 0 restores the default (the current device). */
int kbo_set_devices(const int *devices, int n);
/* Host helper threads used by the host batch entry points for the staging copies between pageable
 * user buffers and pinned memory (two teams of this size; default min(8, cores)). */
int kbo_set_host_threads(int n);
/* host batches are processed in slabs of at most this many query bytes (default 16 MiB) */
int kbo_set_slab_bytes(size_t bytes);
/* Frees the per-device scratch (streams, device buffers, pinned staging) the host batch entry
 * points keep between calls, and the calling thread's own caches (kbo_call / kbo_call_batch keep a
 * device arena for their per-sequence indexes per host thread). */
int kbo_release_scratch(void);
/* The path cover the plan-guided walk uses (host computation, for inspection and tests): every row of the index sits at
 * exactly one text position; text[p] ('A','C','G','T') labels the edge node_at[p-1] -> node_at[p] of the index's de
 * Bruijn graph, 0 where a path starts.  All three arrays have n_sets entries. */
int kbo_index_path_cover(const kbo_index_t *idx, uint8_t *text, uint32_t *pos, uint32_t *node_at);
/* The recovery lines the guided walk reads large indexes through (host computation, for inspection and tests): line b
 * (128 bytes) covers rows [64 b, 64 b + 64): four 16-byte rank blocks { C[c] + rank_c(64 b), row bits 0..31, row bits
 * 32..63, 0 } for c = A, C, G, T, then the 64 LCS bytes of those rows (0 beyond the last row).  n_sets / 64 + 2 lines and
 * one all-zero line; *n_bytes receives the size, lines == NULL only asks for it. */
int kbo_index_recovery_lines(const kbo_index_t *idx, uint8_t *lines, size_t *n_bytes);
/* bytes of path cover + recovery lines + seed table + depth table (and its anchors) a device copy of this index carries (0 =
 * none).  The two tables are sized by log4(rows), not by the index: up to 2 GiB + 64 GiB (kbo_hip_tuning.h: kbo_set_depth_table,
 * INTEGRATION.md "Device memory: the depth table"). */
uint64_t kbo_index_device_plan_bytes(const kbo_index_t *idx);

/* Tuning knobs, experiment switches and test hooks (none of them changes a result) are declared in kbo_hip_tuning.h. */

#ifdef __cplusplus
}
#endif
#endif /* KBO_HIP_H */
