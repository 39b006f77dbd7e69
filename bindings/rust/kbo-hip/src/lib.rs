//! Bindings of the reference crate's matching-statistics path to `libkbo_hip.so` (MI355X, gfx950).
//!
//! SOURCE ONLY: no Rust toolchain exists in the image this repository is built in, so this file has never been
//! compiled; the C ABI it declares (`include/kbo_hip.h`) is what the test suite drives through Python/ctypes.
//! Function names and signatures follow the reference (`kbo` 0.5.1): `find`, `matches`, `map`, `call`,
//! `index::query_sbwt`; each wrapper cites the reference lines it replaces.  The reference panics on precondition
//! failures (`assert!` at index.rs:248, derandomize.rs:274-276, translate.rs:268-270, lib.rs:559-560, 729), so the
//! wrappers turn the library's error codes back into panics.
#![allow(unsafe_code)] // kbo has #![warn(unsafe_code)] (lib.rs:242); an FFI module has to opt out

use std::ops::Range;
use std::os::raw::{c_char, c_int, c_void};

pub mod ffi {
    use super::*;
    #[repr(C)] pub struct KboIndex { _private: [u8; 0] }
    #[repr(C)] pub struct KboMapStream { _private: [u8; 0] }
    #[repr(C)] pub struct KboRefset { _private: [u8; 0] }
    #[repr(C)] #[derive(Clone, Copy, Debug, PartialEq)]
    pub struct KboRle { pub start: u64, pub end: u64, pub matches: u64, pub mismatches: u64,
                        pub jumps: u64, pub gap_bases: u64, pub gap_opens: u64 }
    #[repr(C)] #[derive(Clone, Copy, Debug, PartialEq)]
    pub struct KboRle32 { pub start: u32, pub end: u32, pub matches: u32, pub mismatches: u32,
                          pub jumps: u32, pub gap_bases: u32, pub gap_opens: u32 }
    #[repr(C)] pub struct KboBuildOpts { pub k: u32, pub add_revcomp: i32, pub num_threads: u32, pub prefix_precalc: u32,
                                         pub build_select: i32, pub mem_gb: u32, pub dedup_batches: i32, pub temp_dir: *const c_char }
    #[repr(C)] pub struct KboFindOpts { pub max_error_prob: f64, pub max_gap_len: usize }
    #[repr(C)] pub struct KboMapOpts { pub max_error_prob: f64, pub fill_gaps: i32, pub call_variants: i32, pub format: i32,
                                       pub sbwt_build_opts: KboBuildOpts }
    #[repr(C)] pub struct KboCallOpts { pub max_error_prob: f64, pub sbwt_build_opts: KboBuildOpts }
    #[repr(C)] pub struct KboVariant { pub query_pos: u64, pub query_chars: *const u8, pub query_len: usize,
                                       pub ref_chars: *const u8, pub ref_len: usize }
    #[repr(C)] pub struct KboCallFlat { pub n_variants: u64, pub n_chars: u64, pub query_pos: *mut u32, pub query_len: *mut u16,
                                        pub ref_len: *mut u16, pub chars: *mut u8 }
    pub const KBO_OPT_INHERIT: i32 = i32::MIN;
    #[repr(C)] pub struct KboIndexOpts { pub struct_size: u32, pub plan: i32, pub depth_table: i32, pub depth_table_anchors: i32,
                                         pub slab_bytes: u64, pub n_devices: i32, pub devices: [i32; 16] }
    extern "C" {
        pub fn kbo_last_error() -> *const c_char;
        pub fn kbo_free(p: *mut c_void);
        // kbo::build (lib.rs:501-506) / an index the sbwt crate built, handed over by its parts
        pub fn kbo_index_build(seqs: *const *const u8, lens: *const usize, n_seqs: usize, opts: *const KboBuildOpts,
                               out: *mut *mut KboIndex) -> c_int;
        // ... by a HIP device (-1 = current); the same index, with that device's copy made there
        pub fn kbo_index_build_device(seqs: *const *const u8, lens: *const usize, n_seqs: usize, opts: *const KboBuildOpts,
                                      device: c_int, out: *mut *mut KboIndex) -> c_int;
        pub fn kbo_index_from_parts(k: u32, n_sets: u64, n_kmers: u64, rows: *const *const u64, c: *const u64, lcs: *const u8,
                                    out: *mut *mut KboIndex) -> c_int;
        pub fn kbo_index_free(idx: *mut KboIndex);
        pub fn kbo_index_shards(idx: *const KboIndex) -> c_int;
        pub fn kbo_index_save(idx: *const KboIndex, path: *const c_char) -> c_int;   // .kbohip: index + path cover
        pub fn kbo_index_load(path: *const c_char, out: *mut *mut KboIndex) -> c_int;
        // index::query_sbwt (index.rs:243-256), kbo::matches / map / find / call (lib.rs:612-628, 720-761, 808-821, 547-573)
        pub fn kbo_matching_statistics(idx: *mut KboIndex, query: *const u8, len: usize, d: *mut u64, lo: *mut u64, hi: *mut u64) -> c_int;
        pub fn kbo_matches(idx: *mut KboIndex, query: *const u8, len: usize, p: f64, chars_out: *mut u32) -> c_int;
        pub fn kbo_map(idx: *mut KboIndex, ref_seq: *const u8, len: usize, opts: *const KboMapOpts, out: *mut u8) -> c_int;
        pub fn kbo_find(idx: *mut KboIndex, query: *const u8, len: usize, opts: *const KboFindOpts, out: *mut *mut KboRle,
                        n_out: *mut usize) -> c_int;
        pub fn kbo_call(idx: *mut KboIndex, ref_seq: *const u8, len: usize, opts: *const KboCallOpts, out: *mut *mut KboVariant,
                        n_out: *mut usize) -> c_int;
        // batches: what kbo-cli's loop over the reads / contigs of a file calls once
        pub fn kbo_matches_batch(idx: *mut KboIndex, concat: *const u8, offsets: *const u64, n_seqs: usize, p: f64, chars_out: *mut u8) -> c_int;
        pub fn kbo_map_batch(idx: *mut KboIndex, concat: *const u8, offsets: *const u64, n_seqs: usize, p: f64, format: c_int, out: *mut u8) -> c_int;
        // kbo::map with any MapOpts over a batch; status[s] = 0 or the code kbo_map gives sequence s alone
        pub fn kbo_map_batch_opts(idx: *mut KboIndex, concat: *const u8, offsets: *const u64, n_seqs: usize, opts: *const KboMapOpts,
                                  out: *mut u8, status: *mut i32) -> c_int;
        pub fn kbo_fill_gaps_batch(idx: *mut KboIndex, concat: *const u8, offsets: *const u64, n_seqs: usize, threshold: usize,
                                   max_err_prob: f64, out: *mut u8, status: *mut i32) -> c_int;
        pub fn kbo_find_batch(idx: *mut KboIndex, concat: *const u8, offsets: *const u64, n_seqs: usize, opts: *const KboFindOpts,
                              rles: *mut *mut KboRle, rle_offsets: *mut u64) -> c_int;
        pub fn kbo_call_batch(idx: *mut KboIndex, concat: *const u8, offsets: *const u64, n_seqs: usize, opts: *const KboCallOpts,
                              out: *mut *mut KboVariant, var_offsets: *mut u64) -> c_int;
        pub fn kbo_call_batch_flat(idx: *mut KboIndex, concat: *const u8, offsets: *const u64, n_seqs: usize, opts: *const KboCallOpts,
                                   result: *mut KboCallFlat, var_offsets: *mut u64) -> c_int;
        pub fn kbo_call_flat_free(result: *mut KboCallFlat);
        pub fn kbo_stream_pair_create(tail_cus: c_int, stream: *mut *mut c_void, tail_stream: *mut *mut c_void) -> c_int;
        pub fn kbo_stream_pair_destroy(stream: *mut c_void, tail_stream: *mut c_void);
        // 2-bit packed batches: a quarter of the bytes over PCIe (kbo_hip.h "packed batches")
        pub fn kbo_packed_words(offsets: *const u64, n_seqs: usize) -> usize;
        pub fn kbo_pack_reads(concat: *const u8, offsets: *const u64, n_seqs: usize, words_out: *mut u32, exc_pos: *mut u64,
                              exc_byte: *mut u8, exc_cap: usize, n_exc: *mut usize) -> c_int;
        pub fn kbo_unpack_matches(words: *const u32, offsets: *const u64, n_seqs: usize, chars_out: *mut u8) -> c_int;
        pub fn kbo_matches_batch_packed(idx: *mut KboIndex, words: *const u32, offsets: *const u64, n_seqs: usize, exc_pos: *const u64,
                                        exc_byte: *const u8, n_exc: usize, p: f64, words_out: *mut u32) -> c_int;
        pub fn kbo_find_batch_packed(idx: *mut KboIndex, words: *const u32, offsets: *const u64, n_seqs: usize, exc_pos: *const u64,
                                     exc_byte: *const u8, n_exc: usize, opts: *const KboFindOpts, rles: *mut *mut KboRle32,
                                     rle_offsets: *mut u64) -> c_int;
        // both strands of every sequence in one call, the batch staged to the device once (kbo_hip.h "both strands")
        pub fn kbo_summary_batch(idx: *mut KboIndex, concat: *const u8, offsets: *const u64, n_seqs: usize, p: f64,
                                 summary_out: *mut super::AlnSummary) -> c_int;
        pub fn kbo_summary_batch_packed(idx: *mut KboIndex, words: *const u32, offsets: *const u64, n_seqs: usize, exc_pos: *const u64,
                                        exc_byte: *const u8, n_exc: usize, p: f64, summary_out: *mut super::AlnSummary) -> c_int;
        pub fn kbo_summary_work_bytes(idx: *mut KboIndex, n_seqs: usize, total_bases: u64, max_seq_len: usize) -> usize;
        pub fn kbo_summary_batch_dev(idx: *mut KboIndex, d_concat: *const u8, d_offsets: *const u64, n_seqs: usize, total_bases: u64,
                                     max_seq_len: usize, p: f64, d_ms: *mut u8, d_summary_out: *mut super::AlnSummary, d_work: *mut c_void,
                                     work_bytes: usize, stream: *mut c_void, tail_stream: *mut c_void, fused: *mut c_int) -> c_int;
        pub fn kbo_summary_dev(d_chars: *const u8, d_offsets: *const u64, n_seqs: usize, max_seq_len: usize,
                               d_summary_out: *mut super::AlnSummary, stream: *mut c_void) -> c_int;
        pub fn kbo_summary_words_work_bytes(n_seqs: usize) -> usize;
        pub fn kbo_summary_words_dev(d_words: *const u32, d_offsets: *const u64, n_seqs: usize, max_seq_len: usize,
                                     d_summary_out: *mut super::AlnSummary, d_work: *mut c_void, stream: *mut c_void) -> c_int;
        pub fn kbo_map_stream_submit_summary(ms: *mut KboMapStream, d_concat: *const u8, d_offsets: *const u64, n_seqs: usize, total_bases: u64,
                                             max_seq_len: usize, p: f64, d_summary_out: *mut super::AlnSummary, ready_stream: *mut c_void,
                                             ticket: *mut u64, fused: *mut c_int) -> c_int;
        pub fn kbo_revcomp_batch(concat: *const u8, offsets: *const u64, n_seqs: usize, out: *mut u8) -> c_int;
        pub fn kbo_matches_batch_strands(idx: *mut KboIndex, concat: *const u8, offsets: *const u64, n_seqs: usize, p: f64, format: c_int,
                                         strands: c_int, out_fwd: *mut u8, out_rev: *mut u8) -> c_int;
        pub fn kbo_find_batch_strands(idx: *mut KboIndex, concat: *const u8, offsets: *const u64, n_seqs: usize, opts: *const KboFindOpts,
                                      strands: c_int, rles: *mut *mut KboRle, rle_offsets: *mut u64) -> c_int;
        pub fn kbo_matches_batch_packed_strands(idx: *mut KboIndex, words: *const u32, offsets: *const u64, n_seqs: usize,
                                                exc_pos: *const u64, exc_byte: *const u8, n_exc: usize, p: f64, strands: c_int,
                                                words_fwd: *mut u32, words_rev: *mut u32) -> c_int;
        pub fn kbo_find_batch_packed_strands(idx: *mut KboIndex, words: *const u32, offsets: *const u64, n_seqs: usize,
                                             exc_pos: *const u64, exc_byte: *const u8, n_exc: usize, opts: *const KboFindOpts,
                                             strands: c_int, rles: *mut *mut KboRle32, rle_offsets: *mut u64) -> c_int;
        pub fn kbo_revcomp_batch_dev(d_concat: *const u8, d_offsets: *const u64, n_seqs: usize, total_bases: u64, max_seq_len: usize,
                                     d_out: *mut u8, stream: *mut c_void) -> c_int;
        pub fn kbo_revcomp_packed_scratch_bytes(n_seqs: usize) -> usize;
        pub fn kbo_revcomp_packed_dev(d_words: *const u32, d_offsets: *const u64, n_seqs: usize, total_words: u64, d_exc_pos: *const u64,
                                      d_exc_byte: *const u8, n_exc: usize, d_words_out: *mut u32, d_exc_pos_out: *mut u64,
                                      d_exc_byte_out: *mut u8, d_scratch: *mut c_void, stream: *mut c_void) -> c_int;
        // device-resident batches on a hipStream_t (kbo_hip.h): kbo::map / matches for reads as ONE kernel; `_tail`: its second
        // pass on a second stream, beside the next batch's kernel; packed: 2-bit words in and out
        pub fn kbo_work_bytes(n_seqs: usize, total_bases: u64, max_seq_len: usize, k: u32) -> usize;
        pub fn kbo_ms_work_bytes(n_seqs: usize, total_bases: u64, max_seq_len: usize, k: u32) -> usize;
        pub fn kbo_index_to_device(idx: *mut KboIndex, device: c_int) -> c_int;
        pub fn kbo_map_batch_dev(idx: *mut KboIndex, d_concat: *const u8, d_offsets: *const u64, n_seqs: usize, total_bases: u64,
                                 max_seq_len: usize, p: f64, format: c_int, want_ms: c_int, d_ms: *mut u8, d_chars_out: *mut u8,
                                 d_work: *mut c_void, work_bytes: usize, stream: *mut c_void, fused: *mut c_int) -> c_int;
        pub fn kbo_map_batch_dev_tail(idx: *mut KboIndex, d_concat: *const u8, d_offsets: *const u64, n_seqs: usize, total_bases: u64,
                                      max_seq_len: usize, p: f64, format: c_int, want_ms: c_int, d_ms: *mut u8, d_chars_out: *mut u8,
                                      d_work: *mut c_void, work_bytes: usize, stream: *mut c_void, tail_stream: *mut c_void,
                                      fused: *mut c_int) -> c_int;
        // several batches in flight through the library's own pipelines (kbo_hip.h kbo_map_stream_*): tickets instead of streams
        pub fn kbo_map_stream_create(idx: *mut KboIndex, pipelines: c_int, max_seqs: usize, max_bases: u64, max_seq_len: usize,
                                     out: *mut *mut KboMapStream) -> c_int;
        pub fn kbo_map_stream_submit(ms: *mut KboMapStream, d_concat: *const u8, d_offsets: *const u64, n_seqs: usize, total_bases: u64,
                                     max_seq_len: usize, p: f64, format: c_int, d_ms_out: *mut u8, d_chars_out: *mut u8,
                                     ready_stream: *mut c_void, ticket: *mut u64, fused: *mut c_int) -> c_int;
        pub fn kbo_map_stream_wait(ms: *mut KboMapStream, ticket: u64) -> c_int;
        pub fn kbo_map_stream_wait_on(ms: *mut KboMapStream, ticket: u64, stream: *mut c_void) -> c_int;
        pub fn kbo_map_stream_sync(ms: *mut KboMapStream) -> c_int;
        pub fn kbo_map_stream_free(ms: *mut KboMapStream);
        // kbo::find for a device-resident batch: the characters, then format::run_lengths_gapped of them (records of seven u32)
        pub fn kbo_run_lengths_work_bytes(n_seqs: usize) -> usize;
        pub fn kbo_find_batch_dev(idx: *mut KboIndex, d_concat: *const u8, d_offsets: *const u64, n_seqs: usize, total_bases: u64,
                                  max_seq_len: usize, p: f64, max_gap_len: usize, d_ms: *mut u8, d_chars_out: *mut u8, d_work: *mut c_void,
                                  work_bytes: usize, d_rle_work: *mut c_void, d_records: *mut u32, capacity: usize, stream: *mut c_void,
                                  tail_stream: *mut c_void, fused: *mut c_int) -> c_int;
        // derandomize_ms_vec + translate_ms_vec over device-resident MS bytes with a threshold per sequence, at any length
        pub fn kbo_derand_seq_work_bytes(n_seqs: usize, total_bases: u64, k: usize, min_threshold: usize) -> usize;
        pub fn kbo_derand_translate_seq_dev(d_ms: *const u8, d_offsets: *const u64, n_seqs: usize, total_bases: u64, k: usize,
                                            d_thresholds: *const u32, min_threshold: usize, d_ref: *const u8, d_chars_out: *mut u8,
                                            d_work: *mut c_void, work_bytes: usize, stream: *mut c_void) -> c_int;
        // ... and its summary form: one AlnExtent per sequence instead of a character per base
        pub fn kbo_derand_summary_seq_work_bytes(n_seqs: usize, total_bases: u64, k: usize, min_threshold: usize) -> usize;
        pub fn kbo_derand_summary_seq_dev(d_ms: *const u8, d_offsets: *const u64, n_seqs: usize, total_bases: u64, k: usize,
                                          d_thresholds: *const u32, min_threshold: usize, d_out: *mut super::AlnExtent,
                                          d_work: *mut c_void, work_bytes: usize, stream: *mut c_void) -> c_int;
        // the summary of every (reference, sequence, strand) pair of a reference set with a hit (the set: kbo_refset_build, kbo_hip.h)
        pub fn kbo_summary_refset(set: *mut KboRefset, concat: *const u8, offsets: *const u64, n_seqs: usize, p: f64, strands: c_int,
                                  records: *mut *mut super::RefSummary, n_records: *mut u64) -> c_int;
        // the best reference of every sequence, reduced on the device: one record per sequence; and its device-resident form, whose
        // d_out is the running table of n_seqs records
        pub fn kbo_best_refset(set: *mut KboRefset, concat: *const u8, offsets: *const u64, n_seqs: usize, p: f64, strands: c_int,
                               out: *mut *mut super::RefBest) -> c_int;
        pub fn kbo_best_refset_dev_work_bytes(set: *const KboRefset, n_seqs: usize, total_bases: u64, strands: c_int,
                                              refs_per_slab: usize) -> usize;
        pub fn kbo_best_refset_dev(set: *mut KboRefset, d_concat: *const u8, d_offsets: *const u64, n_seqs: usize, total_bases: u64,
                                   p: f64, strands: c_int, d_work: *mut c_void, work_bytes: usize, d_out: *mut super::RefBest,
                                   stream: *mut c_void) -> c_int;
        // a set whose references of up to max_wide_rows rows (16 384 ..= 2^20) keep their packed form and are walked from memory; the
        // route of reference r (-1 status, 0 LDS, 1 single-index, 2 wide); 1 when the device-resident calls take the set
        pub fn kbo_refset_build_wide(seqs: *const *const u8, lens: *const usize, n_refs: usize, opts: *const KboBuildOpts,
                                     max_wide_rows: usize, out: *mut *mut KboRefset) -> c_int;
        pub fn kbo_refset_route(set: *const KboRefset, r: usize) -> c_int;
        pub fn kbo_refset_packed_only(set: *const KboRefset) -> c_int;
        // a set with a prefilter (a seed table over the packed references): the host forms of find / summary / best then walk only the
        // (reference, sequence, strand) pairs that share a seed; kbo_refset_candidates is the screen alone - bit
        // (r * n_seqs + s) * 2 + strand - 1 of ceil(n_refs * n_seqs * 2 / 32) words
        pub fn kbo_refset_opts_default(o: *mut super::RefsetOpts);
        pub fn kbo_refset_build_opts(seqs: *const *const u8, lens: *const usize, n_refs: usize, opts: *const KboBuildOpts,
                                     refset_opts: *const super::RefsetOpts, out: *mut *mut KboRefset) -> c_int;
        pub fn kbo_refset_has_prefilter(set: *const KboRefset) -> c_int;
        pub fn kbo_refset_prefilter_bytes(set: *const KboRefset) -> u64;
        pub fn kbo_refset_candidates(set: *mut KboRefset, concat: *const u8, offsets: *const u64, n_seqs: usize, p: f64, strands: c_int,
                                     bits_out: *mut u32, n_candidates: *mut u64) -> c_int;
        // the screened device-resident forms: the screen for a batch on the device (d_bits: that bitmap, d_stats: the four figures), and
        // find / summary / best over ONE slab of the candidate list's longest prefix within max_pairs pairs and max_pair_bases bases;
        // d_runs: kbo_ref_run records of ten u32
        pub fn kbo_refset_candidates_dev_work_bytes(set: *const KboRefset, n_seqs: usize, total_bases: u64, strands: c_int) -> usize;
        pub fn kbo_refset_candidates_dev(set: *mut KboRefset, d_concat: *const u8, d_offsets: *const u64, n_seqs: usize, total_bases: u64,
                                         p: f64, strands: c_int, d_work: *mut c_void, work_bytes: usize, d_bits: *mut u32,
                                         d_stats: *mut super::RefsetScreenStats, stream: *mut c_void) -> c_int;
        pub fn kbo_find_refset_screened_dev_work_bytes(set: *const KboRefset, n_seqs: usize, total_bases: u64, strands: c_int,
                                                       capacity: usize, max_pairs: usize, max_pair_bases: u64) -> usize;
        pub fn kbo_find_refset_screened_dev(set: *mut KboRefset, d_concat: *const u8, d_offsets: *const u64, n_seqs: usize, total_bases: u64,
                                            opts: *const KboFindOpts, strands: c_int, d_work: *mut c_void, work_bytes: usize,
                                            d_runs: *mut c_void, capacity: usize, d_n_runs: *mut u64, max_pairs: usize, max_pair_bases: u64,
                                            d_stats: *mut super::RefsetScreenStats, stream: *mut c_void) -> c_int;
        pub fn kbo_summary_refset_screened_dev_work_bytes(set: *const KboRefset, n_seqs: usize, total_bases: u64, strands: c_int,
                                                          capacity: usize, max_pairs: usize, max_pair_bases: u64) -> usize;
        pub fn kbo_summary_refset_screened_dev(set: *mut KboRefset, d_concat: *const u8, d_offsets: *const u64, n_seqs: usize,
                                               total_bases: u64, p: f64, strands: c_int, d_work: *mut c_void, work_bytes: usize,
                                               d_records: *mut super::RefSummary, capacity: usize, d_n_records: *mut u64, max_pairs: usize,
                                               max_pair_bases: u64, d_stats: *mut super::RefsetScreenStats, stream: *mut c_void) -> c_int;
        pub fn kbo_best_refset_screened_dev_work_bytes(set: *const KboRefset, n_seqs: usize, total_bases: u64, strands: c_int,
                                                       max_pairs: usize, max_pair_bases: u64) -> usize;
        pub fn kbo_best_refset_screened_dev(set: *mut KboRefset, d_concat: *const u8, d_offsets: *const u64, n_seqs: usize, total_bases: u64,
                                            p: f64, strands: c_int, d_work: *mut c_void, work_bytes: usize, d_out: *mut super::RefBest,
                                            max_pairs: usize, max_pair_bases: u64, d_stats: *mut super::RefsetScreenStats,
                                            stream: *mut c_void) -> c_int;
        // the locus of a run: a set built with `RefsetOpts::positions` = 1 carries one entry per row; runs: kbo_ref_run records of ten
        // u32 ({ ref, seq, strand, start, end, ... }), loci: one RefLocus per run, same index
        pub fn kbo_refset_has_positions(set: *const KboRefset) -> c_int;
        pub fn kbo_refset_positions_bytes(set: *const KboRefset) -> u64;
        pub fn kbo_refset_positions(set: *const KboRefset, r: usize, out: *mut u32, n_rows: *mut usize) -> c_int;
        pub fn kbo_refset_ref_len(set: *const KboRefset, r: usize) -> u64;
        pub fn kbo_locate_refset(set: *mut KboRefset, concat: *const u8, offsets: *const u64, n_seqs: usize, runs: *const u32, n_runs: u64,
                                 loci_out: *mut super::RefLocus) -> c_int;
        pub fn kbo_locate_refset_dev(set: *mut KboRefset, d_concat: *const u8, d_offsets: *const u64, n_seqs: usize, total_bases: u64,
                                     d_runs: *const u32, d_n_runs: *const u64, capacity: usize, d_loci: *mut super::RefLocus,
                                     stream: *mut c_void) -> c_int;
        pub fn kbo_locate_refset_host(set: *const KboRefset, concat: *const u8, offsets: *const u64, n_seqs: usize, runs: *const u32,
                                      n_runs: u64, loci_out: *mut super::RefLocus) -> c_int;
        // the cover of a reference: depth and breadth of every reference over the runs; covers: one RefCover per reference, depth (or
        // null): the profile of kbo_refset_cover_bases u32, laid out by kbo_refset_cover_offsets
        pub fn kbo_refset_cover_bases(set: *const KboRefset) -> u64;
        pub fn kbo_refset_cover_offsets(set: *const KboRefset, out: *mut u64) -> c_int;
        pub fn kbo_cover_refset(set: *mut KboRefset, concat: *const u8, offsets: *const u64, n_seqs: usize, runs: *const u32, n_runs: u64,
                                covers_out: *mut super::RefCover, depth_out: *mut u32) -> c_int;
        pub fn kbo_cover_refset_host(set: *const KboRefset, concat: *const u8, offsets: *const u64, n_seqs: usize, runs: *const u32,
                                     n_runs: u64, covers_out: *mut super::RefCover, depth_out: *mut u32) -> c_int;
        pub fn kbo_cover_refset_dev_work_bytes(set: *const KboRefset) -> usize;
        pub fn kbo_cover_refset_dev(set: *mut KboRefset, d_concat: *const u8, d_offsets: *const u64, n_seqs: usize, total_bases: u64,
                                    d_runs: *const u32, d_n_runs: *const u64, capacity: usize, d_covers: *mut super::RefCover,
                                    d_depth: *mut u32, d_work: *mut c_void, work_bytes: usize, stream: *mut c_void) -> c_int;
        // the variants of a pair: kbo::call against every reference with a hit; out: records and their characters, released by
        // kbo_ref_calls_free.  opts.sbwt_build_opts.k is the set's k; useful calls need k of about twice the threshold or more
        pub fn kbo_call_refset(set: *mut KboRefset, concat: *const u8, offsets: *const u64, n_seqs: usize, opts: *const KboCallOpts,
                               strands: c_int, out: *mut super::RefCalls) -> c_int;
        pub fn kbo_call_refset_host(set: *const KboRefset, concat: *const u8, offsets: *const u64, n_seqs: usize, opts: *const KboCallOpts,
                                    strands: c_int, out: *mut super::RefCalls) -> c_int;
        pub fn kbo_ref_calls_free(calls: *mut super::RefCalls);
        // the device-resident forms: the same records and characters within max_variants / max_chars, the totals and what the lists
        // of max_sites could not hold in d_stats; nothing synchronised or read back
        pub fn kbo_call_refset_dev_work_bytes(set: *const KboRefset, n_seqs: usize, total_bases: u64, strands: c_int, max_sites: usize,
                                              refs_per_slab: usize) -> usize;
        pub fn kbo_call_refset_dev(set: *mut KboRefset, d_concat: *const u8, d_offsets: *const u64, n_seqs: usize, total_bases: u64,
                                   opts: *const KboCallOpts, strands: c_int, d_work: *mut c_void, work_bytes: usize,
                                   d_variants: *mut super::RefVariant, max_variants: usize, d_chars: *mut u8, max_chars: usize,
                                   max_sites: usize, d_stats: *mut super::RefCallsStats, stream: *mut c_void) -> c_int;
        pub fn kbo_call_refset_screened_dev_work_bytes(set: *const KboRefset, n_seqs: usize, total_bases: u64, strands: c_int,
                                                       max_sites: usize, max_pairs: usize, max_pair_bases: u64) -> usize;
        pub fn kbo_call_refset_screened_dev(set: *mut KboRefset, d_concat: *const u8, d_offsets: *const u64, n_seqs: usize, total_bases: u64,
                                            opts: *const KboCallOpts, strands: c_int, d_work: *mut c_void, work_bytes: usize,
                                            d_variants: *mut super::RefVariant, max_variants: usize, d_chars: *mut u8, max_chars: usize,
                                            max_sites: usize, d_stats: *mut super::RefCallsStats, max_pairs: usize, max_pair_bases: u64,
                                            d_screen_stats: *mut super::RefsetScreenStats, stream: *mut c_void) -> c_int;
        pub fn kbo_refset_last_call(out: *mut u64) -> c_int;
        pub fn kbo_refset_spell_row(set: *const KboRefset, r: usize, row: u32, out: *mut u8) -> c_int;
        // positions, segments, depth: the single-index path in SOURCE coordinates (kbo_hip.h).  add_positions makes the table on
        // `device` from the sequences the index was built from; segments_dev / depth_finish_dev compose behind kbo_ms_batch_dev with
        // intervals on one stream; segments_batch is the host form (segs released by kbo_free)
        pub fn kbo_index_add_positions(idx: *mut KboIndex, seqs: *const *const u8, lens: *const usize, n_seqs: usize, add_revcomp: c_int,
                                       device: c_int) -> c_int;
        pub fn kbo_index_has_positions(idx: *const KboIndex) -> c_int;
        pub fn kbo_index_positions_bytes(idx: *const KboIndex) -> u64;
        pub fn kbo_index_positions(idx: *const KboIndex, out: *mut u32, n_rows: *mut usize) -> c_int;
        pub fn kbo_index_source_offsets(idx: *const KboIndex, out: *mut u64, n: *mut usize) -> c_int;
        pub fn kbo_index_source_bases(idx: *const KboIndex) -> u64;
        pub fn kbo_index_positions_to_device(idx: *mut KboIndex, device: c_int) -> c_int;
        pub fn kbo_positions_from_ms_host(k: u32, n_sets: u64, d: *const u8, lo: *const u32, offsets: *const u64, n_seqs: usize,
                                          src_off: *const u64, rev: c_int, entries_inout: *mut u32, n_not_full: *mut u64) -> c_int;
        pub fn kbo_segments_work_bytes(n_seqs: usize, total_bases: u64) -> usize;
        pub fn kbo_segments_dev(idx: *mut KboIndex, d_ms: *const u8, d_lo: *const u32, d_offsets: *const u64, n_seqs: usize, total_bases: u64,
                                bridge: u32, strand: u32, d_segs: *mut super::SeqSegment, capacity: usize, d_n_segs: *mut u64,
                                d_delta: *mut u32, d_work: *mut c_void, work_bytes: usize, stream: *mut c_void) -> c_int;
        pub fn kbo_segments_from_ms_host(entries: *const u32, n_rows: u64, k: u32, d: *const u8, lo: *const u32, offsets: *const u64,
                                         n_seqs: usize, bridge: u32, strand: u32, segs: *mut super::SeqSegment, capacity: usize,
                                         n_segs: *mut u64, delta: *mut u32, source_bases: u64) -> c_int;
        pub fn kbo_depth_work_bytes(idx: *const KboIndex) -> usize;
        pub fn kbo_depth_finish_dev(idx: *mut KboIndex, d_delta: *const u32, d_depth: *mut u32, d_work: *mut c_void, work_bytes: usize,
                                    stream: *mut c_void) -> c_int;
        pub fn kbo_segments_batch(idx: *mut KboIndex, concat: *const u8, offsets: *const u64, n_seqs: usize, bridge: u32, strands: c_int,
                                  segs: *mut *mut super::SeqSegment, n_segs: *mut u64, depth_out: *mut u32) -> c_int;
        // placement: the segments of every sequence chained to one record, behind kbo_segments_dev on the same stream (merge != 0:
        // into what d_place holds - the second strand's call); place_from_segments_host is the CPU restatement, place_batch the host form
        pub fn kbo_place_work_bytes(n_seqs: usize, n_segs_capacity: usize) -> usize;
        pub fn kbo_place_dev(idx: *mut KboIndex, d_segs: *const super::SeqSegment, d_n_segs: *const u64, capacity: usize, n_seqs: usize,
                             max_gap: u32, max_indel: u32, merge: c_int, d_place: *mut super::SeqPlace, d_work: *mut c_void,
                             work_bytes: usize, stream: *mut c_void) -> c_int;
        pub fn kbo_place_from_segments_host(segs: *const super::SeqSegment, n_segs: u64, n_seqs: usize, src_off: *const u64, n_src: usize,
                                            k: u32, max_gap: u32, max_indel: u32, merge: c_int, place: *mut super::SeqPlace) -> c_int;
        pub fn kbo_place_batch(idx: *mut KboIndex, concat: *const u8, offsets: *const u64, n_seqs: usize, bridge: u32, strands: c_int,
                               max_gap: u32, max_indel: u32, place_out: *mut super::SeqPlace) -> c_int;
        // pileup: what the reads say at every source base - one integer atomic per base that no exact window of its segment covers,
        // into d_pile ([source_bases][4] u32, zeroed once, shared by batches and strands like d_delta) - behind kbo_segments_dev on
        // the same stream and without scratch; pileup_sites_dev turns pile and depth into candidate sites (flag, scan, emit);
        // the *_host calls restate both on the CPU, pileup_batch is the host form (sites released by kbo_free)
        pub fn kbo_pileup_dev(idx: *mut KboIndex, d_concat: *const u8, d_ms: *const u8, d_offsets: *const u64, n_seqs: usize, total_bases: u64,
                              d_segs: *const super::SeqSegment, d_n_segs: *const u64, capacity: usize, skip_multi: c_int, d_pile: *mut u32,
                              stream: *mut c_void) -> c_int;
        pub fn kbo_pileup_sites_work_bytes(idx: *const KboIndex) -> usize;
        pub fn kbo_pileup_sites_dev(idx: *mut KboIndex, d_pile: *const u32, d_depth: *const u32, min_count: u32, frac_num: u32, frac_den: u32,
                                    d_sites: *mut super::PileSite, capacity: usize, d_n_sites: *mut u64, d_work: *mut c_void,
                                    work_bytes: usize, stream: *mut c_void) -> c_int;
        pub fn kbo_pileup_from_segments_host(segs: *const super::SeqSegment, n_segs: u64, concat: *const u8, ms: *const u8, offsets: *const u64,
                                             n_seqs: usize, total_bases: u64, k: u32, skip_multi: c_int, pile: *mut u32, source_bases: u64,
                                             n_bridged: *mut u64) -> c_int;
        pub fn kbo_pileup_sites_host(pile: *const u32, depth: *const u32, source_bases: u64, src_off: *const u64, n_src: usize, min_count: u32,
                                     frac_num: u32, frac_den: u32, sites: *mut super::PileSite, capacity: usize, n_sites: *mut u64) -> c_int;
        pub fn kbo_pileup_batch(idx: *mut KboIndex, concat: *const u8, offsets: *const u64, n_seqs: usize, bridge: u32, strands: c_int,
                                skip_multi: c_int, min_count: u32, frac_num: u32, frac_den: u32, sites: *mut *mut super::PileSite,
                                n_sites: *mut u64, depth_out: *mut u32, pile_out: *mut u32) -> c_int;
        // indels: one event per clean junction of two consecutive records (a left-aligned deletion, or an insertion with its bases),
        // appended to one list behind *d_n_events (zeroed once, shared by batches and strands like d_delta); indel_sites_dev sorts
        // and counts the list into sites behind kbo_depth_finish_dev; the *_host calls restate both on the CPU, indels_batch is the
        // host form (sites released by kbo_free)
        pub fn kbo_indels_work_bytes(n_segs_capacity: usize) -> usize;
        pub fn kbo_indels_dev(idx: *mut KboIndex, d_concat: *const u8, d_offsets: *const u64, n_seqs: usize, total_bases: u64,
                              d_segs: *const super::SeqSegment, d_n_segs: *const u64, capacity: usize, skip_multi: c_int, max_indel: u32,
                              d_events: *mut super::IndelEvent, event_capacity: usize, d_n_events: *mut u64, d_work: *mut c_void,
                              work_bytes: usize, stream: *mut c_void) -> c_int;
        pub fn kbo_indel_sites_work_bytes(event_capacity: usize) -> usize;
        pub fn kbo_indel_sites_dev(idx: *mut KboIndex, d_events: *const super::IndelEvent, d_n_events: *const u64, event_capacity: usize,
                                   d_depth: *const u32, min_count: u32, frac_num: u32, frac_den: u32, d_sites: *mut super::IndelSite,
                                   site_capacity: usize, d_n_sites: *mut u64, d_work: *mut c_void, work_bytes: usize,
                                   stream: *mut c_void) -> c_int;
        pub fn kbo_indels_from_segments_host(segs: *const super::SeqSegment, n_segs: u64, concat: *const u8, offsets: *const u64, n_seqs: usize,
                                             total_bases: u64, k: u32, skip_multi: c_int, max_indel: u32, src_off: *const u64, n_src: usize,
                                             events: *mut super::IndelEvent, event_capacity: usize, n_events: *mut u64,
                                             n_complex: *mut u64) -> c_int;
        pub fn kbo_indel_sites_host(events: *const super::IndelEvent, n_events: u64, event_capacity: usize, depth: *const u32,
                                    src_off: *const u64, n_src: usize, min_count: u32, frac_num: u32, frac_den: u32,
                                    sites: *mut super::IndelSite, site_capacity: usize, n_sites: *mut u64) -> c_int;
        pub fn kbo_indels_batch(idx: *mut KboIndex, concat: *const u8, offsets: *const u64, n_seqs: usize, bridge: u32, strands: c_int,
                                skip_multi: c_int, max_indel: u32, min_count: u32, frac_num: u32, frac_den: u32,
                                sites: *mut *mut super::IndelSite, n_sites: *mut u64, depth_out: *mut u32) -> c_int;
        // format::run_lengths_gapped over device-resident characters at any sequence length: a chunk per lane (records of seven u32)
        pub fn kbo_run_lengths_seq_work_bytes(n_seqs: usize, total_bases: u64) -> usize;
        pub fn kbo_run_lengths_seq_dev(d_chars: *const u8, d_offsets: *const u64, n_seqs: usize, total_bases: u64, max_gap_len: usize,
                                       d_work: *mut c_void, work_bytes: usize, d_records: *mut u32, capacity: usize, d_first: *mut u32,
                                       stream: *mut c_void) -> c_int;
        pub fn kbo_matches_packed_dev_scratch_bytes(n_seqs: usize, total_bases: u64) -> usize;
        pub fn kbo_matches_packed_dev(idx: *mut KboIndex, d_words: *const u32, d_offsets: *const u64, n_seqs: usize, total_bases: u64,
                                      max_seq_len: usize, uniform_len: usize, d_exc_pos: *const u64, d_exc_byte: *const u8, n_exc: usize,
                                      p: f64, d_words_out: *mut u32, d_scratch: *mut c_void, d_work: *mut c_void, work_bytes: usize,
                                      stream: *mut c_void, tail_stream: *mut c_void) -> c_int;
        // options of one handle (what kbo_set_plan / kbo_set_depth_table* / kbo_set_devices / kbo_set_slab_bytes set process-wide)
        pub fn kbo_index_opts_default(opts: *mut KboIndexOpts) -> c_int;
        pub fn kbo_index_set_opts(idx: *mut KboIndex, opts: *const KboIndexOpts) -> c_int;
        pub fn kbo_index_get_opts(idx: *const KboIndex, opts: *mut KboIndexOpts) -> c_int;
    }
}

fn check(rc: c_int) {
    if rc != 0 {
        let msg = unsafe { std::ffi::CStr::from_ptr(ffi::kbo_last_error()) }.to_string_lossy().into_owned();
        panic!("kbo_hip error {}: {}", rc, msg);
    }
}

/// `translate_ms_vec(derandomize_ms_vec(ms_s, k, t_s), k, t_s)` (derandomize.rs:269-288, translate.rs:263-293) for every sequence of
/// a device-resident batch, `t_s = d_thresholds[s]`; with `d_ref` non-null `format::relative_to_ref` of it (format.rs:266-287).
/// Enqueues a constant number of launches on `stream` and returns; nothing is read back.  `d_work`: `derand_seq_work_bytes` bytes,
/// 16-byte aligned; the per-base buffers carry 16 bytes of slack; not in place.
///
/// # Safety
/// Every pointer is a device pointer of the size `include/kbo_hip.h` documents for `kbo_derand_translate_seq_dev`.
#[allow(clippy::too_many_arguments)]
pub unsafe fn derand_translate_seq_dev(d_ms: *const u8, d_offsets: *const u64, n_seqs: usize, total_bases: u64, k: usize,
                                       d_thresholds: *const u32, min_threshold: usize, d_ref: *const u8, d_chars_out: *mut u8,
                                       d_work: *mut c_void, work_bytes: usize, stream: *mut c_void) {
    check(ffi::kbo_derand_translate_seq_dev(d_ms, d_offsets, n_seqs, total_bases, k, d_thresholds, min_threshold, d_ref, d_chars_out,
                                            d_work, work_bytes, stream));
}
pub fn derand_seq_work_bytes(n_seqs: usize, total_bases: u64, k: usize, min_threshold: usize) -> usize {
    unsafe { ffi::kbo_derand_seq_work_bytes(n_seqs, total_bases, k, min_threshold) }
}

/// `kbo_aln_extent`: the counts of `AlnSummary` with the extent of the alignment - `start` the position of the first character other
/// than '-', `end` one past the last, both 0 when there is none.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct AlnExtent {
    pub n_match: u32,
    pub n_mismatch: u32,
    pub n_jump: u32,
    pub n_runs: u32,
    pub start: u32,
    pub end: u32,
}

/// `kbo_refset_screen_stats` (32 bytes, on the device): what the screened device-resident reference-set calls report - the candidate
/// pairs and their bases, and the pairs and bases of the one slab that was walked; `n_walked == n_candidates`: the call is complete.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct RefsetScreenStats {
    pub n_candidates: u64,
    pub candidate_bases: u64,
    pub n_walked: u64,
    pub walked_bases: u64,
}

/// `kbo_ref_summary` (36 bytes): what `kbo_summary_refset` returns per (reference, sequence, strand) pair with a hit.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct RefSummary {
    pub ref_: u32,
    pub seq: u32,
    pub strand: u32,
    pub aln: AlnExtent,
}

/// `kbo_ref_best` (48 bytes): what `kbo_best_refset` returns per query sequence - the first (reference, strand) pair by (larger
/// `aln.n_match`, smaller `ref_`, '+' first), the number of pairs with a hit, and the runner-up among the other references.
/// `ref_` / `second_ref` are `REF_NONE` where there is none.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct RefBest {
    pub seq: u32,
    pub ref_: u32,
    pub strand: u32,
    pub aln: AlnExtent,
    pub n_hits: u32,
    pub second_ref: u32,
    pub second_match: u32,
}
pub const REF_NONE: u32 = 0xFFFF_FFFF;

/// The summary form of `derand_translate_seq_dev`: the same inputs and contract, one `AlnExtent` per sequence at `d_out` (every one
/// written; sequences of fewer than 3 bases get zeros) and no character buffer.  `d_work`: `derand_summary_seq_work_bytes` bytes.
///
/// # Safety
/// Every pointer is a device pointer of the size `include/kbo_hip.h` documents for `kbo_derand_summary_seq_dev`.
#[allow(clippy::too_many_arguments)]
pub unsafe fn derand_summary_seq_dev(d_ms: *const u8, d_offsets: *const u64, n_seqs: usize, total_bases: u64, k: usize,
                                     d_thresholds: *const u32, min_threshold: usize, d_out: *mut AlnExtent, d_work: *mut c_void,
                                     work_bytes: usize, stream: *mut c_void) {
    check(ffi::kbo_derand_summary_seq_dev(d_ms, d_offsets, n_seqs, total_bases, k, d_thresholds, min_threshold, d_out, d_work, work_bytes,
                                          stream));
}
pub fn derand_summary_seq_work_bytes(n_seqs: usize, total_bases: u64, k: usize, min_threshold: usize) -> usize {
    unsafe { ffi::kbo_derand_summary_seq_work_bytes(n_seqs, total_bases, k, min_threshold) }
}

/// `kbo_summary_refset` over a set handle a caller built with `kbo_refset_build`: the records of the pairs with a hit, ordered by
/// (ref, seq, strand).
///
/// # Safety
/// `set` is a live `kbo_refset_t`.
pub unsafe fn summary_refset(set: *mut ffi::KboRefset, seqs: &[Vec<u8>], max_error_prob: f64, strands: c_int) -> Vec<RefSummary> {
    let mut offsets = vec![0u64; seqs.len() + 1];
    for (i, r) in seqs.iter().enumerate() { offsets[i + 1] = offsets[i] + r.len() as u64; }
    let concat: Vec<u8> = seqs.concat();
    let (mut p, mut n) = (std::ptr::null_mut::<RefSummary>(), 0u64);
    check(ffi::kbo_summary_refset(set, concat.as_ptr(), offsets.as_ptr(), seqs.len(), max_error_prob, strands, &mut p, &mut n));
    if n == 0 { return Vec::new(); }
    let out = std::slice::from_raw_parts(p, n as usize).to_vec();
    ffi::kbo_free(p as *mut c_void);
    out
}

/// `kbo_refset_opts`: `max_wide_rows` (16 384 ..= 2^20), `prefilter` and `positions` (0 or 1) of `kbo_refset_build_opts`.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct RefsetOpts {
    pub max_wide_rows: usize,
    pub prefilter: i32,
    pub positions: i32,
}

/// `KBO_LOCUS_NONE` / `KBO_POS_NONE`, and `KBO_LOCUS_MULTI` (bit 31 of a table entry; bit 30: a REV occurrence).
pub const LOCUS_NONE: u32 = 0xFFFF_FFFF;
pub const LOCUS_MULTI: u32 = 0x8000_0000;

/// `kbo_ref_locus` (24 bytes), one per `kbo_ref_run`: the run's first and last anchor as (position in the sequence on the run's
/// strand, position on the reference), `LOCUS_NONE` without one.  `flags`: bit 0 / 1 the first / last anchor is a REV occurrence,
/// bit 2 / 3 it is MULTI, bit 4 the record was not usable.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct RefLocus {
    pub q_first: u32,
    pub ref_first: u32,
    pub q_last: u32,
    pub ref_last: u32,
    pub flags: u32,
    pub n_tested: u32,
}

/// `kbo_seq_segment` (28 bytes): a collinear block of exact k-mer matches of sequence `seq` in source coordinates.  `q_first` /
/// `q_last`: the first base of the first / last anchor's k-mer in the sequence; `pos_first` / `pos_last`: their positions on the
/// sources.  `flags`: bit 0 REV, bit 2 / 3 the first / last anchor's k-mer occurs more than once.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct SeqSegment {
    pub seq: u32,
    pub strand: u32,
    pub q_first: u32,
    pub q_last: u32,
    pub pos_first: u32,
    pub pos_last: u32,
    pub flags: u32,
}

/// `KBO_PLACE_NONE`: `SeqPlace::source` of a sequence without a segment; `KBO_PLACE_REV` / `KBO_PLACE_SPILLS`: bits 0 and 1 of its flags.
pub const PLACE_NONE: u32 = 0xFFFF_FFFF;
pub const PLACE_REV: u16 = 1;
pub const PLACE_SPILLS: u16 = 2;

/// `kbo_seq_place` (48 bytes), one per sequence: the best chain of the sequence's segments.  `source`: the source sequence it lies on;
/// `q_start .. q_end` in the sequence and `pos_start .. pos_end` in source coordinates, half open; `score`: the query bases the chain's
/// segments cover; `n_segs`, `indel`, `n_multi`: segments, indel bases and segments with a repeated k-mer at an end along the chain;
/// `second`: the score of the best chain with another first segment, 0 without one.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct SeqPlace {
    pub source: u32,
    pub strand: u16,
    pub flags: u16,
    pub q_start: u32,
    pub q_end: u32,
    pub pos_start: u32,
    pub pos_end: u32,
    pub score: u32,
    pub n_segs: u32,
    pub indel: u32,
    pub n_multi: u32,
    pub second: u32,
    pub reserved: u32,
}

/// `kbo_pile_site` (32 bytes): a source base where a column of the pile holds at least `min_count` reads and at least
/// `frac_num / frac_den` of the depth.  `pos` in source coordinates, `source` the sequence that holds it, `count`: the reads whose
/// bridged base there is A, C, G, T - the column of the source's own base among them, which the caller drops against its text.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct PileSite {
    pub pos: u32,
    pub source: u32,
    pub depth: u32,
    pub count: [u32; 4],
    pub reserved: u32,
}

/// `KBO_INDEL_INS` / `KBO_INDEL_LONG` / `KBO_INDEL_LEN_MASK`: the fields of `kind_len`; `KBO_INDEL_MINUS`: bit 0 of `IndelEvent::flags`.
pub const INDEL_INS: u32 = 1 << 31;
pub const INDEL_LONG: u32 = 1 << 30;
pub const INDEL_LEN_MASK: u32 = (1 << 30) - 1;
pub const INDEL_MINUS: u32 = 1;

/// `kbo_indel_event` (16 bytes): one clean junction of two consecutive segments.  `pos` in source coordinates, left-aligned: the first
/// deleted base, or the base in front of which the inserted bases go; `code`: the inserted bases of an insertion of at most 16, two
/// bits each, the lowest in source order lowest.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct IndelEvent {
    pub pos: u32,
    pub kind_len: u32,
    pub code: u32,
    pub flags: u32,
}

/// `kbo_indel_site` (32 bytes): a group of equal events that holds at least `min_count` of them and at least `frac_num / frac_den` of
/// `depth`, the depth of the base in front of the event.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct IndelSite {
    pub pos: u32,
    pub source: u32,
    pub kind_len: u32,
    pub code: u32,
    pub count: u32,
    pub n_minus: u32,
    pub depth: u32,
    pub reserved: u32,
}

/// `KBO_COVER_NO_ENTRIES` / `KBO_COVER_OVERFLOW`: bits 0 and 1 of `RefCover::flags`.
pub const COVER_NO_ENTRIES: u32 = 1;
pub const COVER_OVERFLOW: u32 = 2;

/// `kbo_ref_cover` (48 bytes), one per reference of the set: how much of the reference the runs' anchors cover (`covered` bases in
/// `n_segments` pieces between `first` and `last`, `LOCUS_NONE` without one), how deep (`max_depth`), from how many runs and anchors.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct RefCover {
    pub ref_len: u32,
    pub covered: u32,
    pub n_segments: u32,
    pub first: u32,
    pub last: u32,
    pub max_depth: u32,
    pub n_runs: u32,
    pub flags: u32,
    pub n_anchors: u64,
    pub n_multi: u64,
}

/// `kbo_ref_variant` (24 bytes): a variant of `kbo::call` between reference `ref_` and sequence `seq` on `strand` - `Variant::query_pos`
/// on that strand, and where its characters lie in `RefCalls::chars`: `query_len` of the sequence, then `ref_len` of the reference.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct RefVariant {
    pub ref_: u32,
    pub seq: u32,
    pub strand: u32,
    pub pos: u32,
    pub chars: u32,
    pub query_len: u16,
    pub ref_len: u16,
}

/// `kbo_ref_calls`: what `kbo_call_refset` returns - `n_variants` records ordered by (ref, seq, strand, pos) and their `n_chars`
/// characters; both null without a variant.  `kbo_ref_calls_free` releases them.
#[repr(C)]
#[derive(Debug)]
pub struct RefCalls {
    pub n_variants: u64,
    pub n_chars: u64,
    pub variants: *mut RefVariant,
    pub chars: *mut u8,
}

/// `kbo_ref_calls_stats` (64 bytes, on the device): what `kbo_call_refset_dev` found - the totals, whether or not they fitted the
/// capacities - and what its lists of `max_sites` records could not hold: the call is complete iff `max_slab_candidates` and `n_sites`
/// are both at most `max_sites`.  `n_panics`: sites at which the reference would panic; nothing is emitted for them.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct RefCallsStats {
    pub n_variants: u64,
    pub n_chars: u64,
    pub n_sites: u64,
    pub max_slab_candidates: u64,
    pub n_panics: u64,
    pub reserved: [u64; 3],
}

/// `kbo_refset_candidates` over a set built with a prefilter: `out[(r * n_seqs + s) * 2 + strand - 1]` says whether sequence `s` on
/// that strand shares a seed with reference `r` - every pair with a record is among them.
///
/// # Safety
/// `set` is a live `kbo_refset_t`.
pub unsafe fn refset_candidates(set: *mut ffi::KboRefset, n_refs: usize, seqs: &[Vec<u8>], max_error_prob: f64, strands: c_int) -> Vec<bool> {
    let mut offsets = vec![0u64; seqs.len() + 1];
    for (i, r) in seqs.iter().enumerate() { offsets[i + 1] = offsets[i] + r.len() as u64; }
    let concat: Vec<u8> = seqs.concat();
    let n_bits = n_refs * seqs.len() * 2;
    let mut words = vec![0u32; (n_bits + 31) / 32];
    check(ffi::kbo_refset_candidates(set, concat.as_ptr(), offsets.as_ptr(), seqs.len(), max_error_prob, strands, words.as_mut_ptr(),
                                     std::ptr::null_mut()));
    (0..n_bits).map(|b| words[b / 32] >> (b % 32) & 1 == 1).collect()
}

/// `kbo_best_refset` over a set handle a caller built with `kbo_refset_build`: one record per sequence, in sequence order.
///
/// # Safety
/// `set` is a live `kbo_refset_t`.
pub unsafe fn best_refset(set: *mut ffi::KboRefset, seqs: &[Vec<u8>], max_error_prob: f64, strands: c_int) -> Vec<RefBest> {
    let mut offsets = vec![0u64; seqs.len() + 1];
    for (i, r) in seqs.iter().enumerate() { offsets[i + 1] = offsets[i] + r.len() as u64; }
    let concat: Vec<u8> = seqs.concat();
    let mut p = std::ptr::null_mut::<RefBest>();
    check(ffi::kbo_best_refset(set, concat.as_ptr(), offsets.as_ptr(), seqs.len(), max_error_prob, strands, &mut p));
    let out = std::slice::from_raw_parts(p, seqs.len()).to_vec();
    ffi::kbo_free(p as *mut c_void);
    out
}

/// `format::run_lengths_gapped(aln_s, max_gap_len)` (format.rs:143-193) for every sequence of a device-resident batch, at any length:
/// records of seven `u32` `{start, end, matches, mismatches, jumps, gap_bases, gap_opens}` ordered by (sequence, start), `d_first[s]` the
/// index of sequence `s`'s first record and `d_first[n_seqs]` their number (those beyond `capacity` are counted, not written).
/// Enqueues a constant number of launches on `stream` and returns; nothing is read back.  `d_work`: `run_lengths_seq_work_bytes`
/// bytes, 16-byte aligned; `d_chars` carries 16 bytes of slack.
///
/// # Safety
/// Every pointer is a device pointer of the size `include/kbo_hip.h` documents for `kbo_run_lengths_seq_dev`.
#[allow(clippy::too_many_arguments)]
pub unsafe fn run_lengths_seq_dev(d_chars: *const u8, d_offsets: *const u64, n_seqs: usize, total_bases: u64, max_gap_len: usize,
                                  d_work: *mut c_void, work_bytes: usize, d_records: *mut u32, capacity: usize, d_first: *mut u32,
                                  stream: *mut c_void) {
    check(ffi::kbo_run_lengths_seq_dev(d_chars, d_offsets, n_seqs, total_bases, max_gap_len, d_work, work_bytes, d_records, capacity,
                                       d_first, stream));
}
pub fn run_lengths_seq_work_bytes(n_seqs: usize, total_bases: u64) -> usize {
    unsafe { ffi::kbo_run_lengths_seq_work_bytes(n_seqs, total_bases) }
}

/// Stands in for `(&SbwtIndexVariant, &LcsArray)`: the index resident in HBM.  Immutable after construction.
pub struct GpuIndex(*mut ffi::KboIndex);
unsafe impl Send for GpuIndex {}
unsafe impl Sync for GpuIndex {}
impl Drop for GpuIndex { fn drop(&mut self) { unsafe { ffi::kbo_index_free(self.0) } } }

/// The abstract content of an `sbwt` index in the form `kbo_index_from_parts` takes: the four SubsetMatrix rows as
/// u64 words (bit `i & 63` of word `i >> 6` = row `i`), the C array, one LCS byte per row.
pub struct SbwtParts { pub k: usize, pub n_sets: usize, pub n_kmers: usize, pub rows: [Vec<u64>; 4], pub c: [u64; 4], pub lcs: Vec<u8> }

/// Reads an index built by the `sbwt` crate out through the calls the reference itself makes on it - `k()`,
/// `n_sets()`, `n_kmers()` (lib.rs:620), `access_kmer(colex)` (variant_calling.rs:276; needs `build_select = true`) -
/// and nothing else: the crate's source is not in the reference tree, so its bit-vector accessors could not be looked
/// up, let alone tested, where this was written.  O(n k log n) time and n k bytes: fine for bacterial genomes, too slow
/// for a human one - there a maintainer replaces the body by reads of the SubsetMatrix rows and the LCS int-vector
/// (one line each, once the accessor names are at hand).  Whatever fills it, `kbo_index_from_parts` validates the parts
/// (C against the edge bits, edge bits == n_sets - 1, LCS < k) and refuses anything inconsistent with KBO_E_BAD_ARG.
///
/// Definitions (verified against the reference's goldens): rows are in colex order;
/// `B_c[i] = 1` iff row i is the first row of its (k-1)-suffix group and `row[1..] + c` is a row;
/// `C[c] = 1 + sum_{c' < c} popcount(B_c')`; `LCS[i]` = longest common suffix of rows i-1 and i, `$` never matching.
pub fn export_sbwt_parts(sbwt: &sbwt::SbwtIndex<sbwt::SubsetMatrix>) -> SbwtParts {
    let (k, n) = (sbwt.k(), sbwt.n_sets());
    let kmers: Vec<Vec<u8>> = (0..n).map(|i| sbwt.access_kmer(i)).collect(); // '$'-padded on the left
    let colex = |a: &[u8], b: &[u8]| a.iter().rev().cmp(b.iter().rev()); // ('$' = 36 sorts below 'A')
    let words = (n + 63) / 64;
    let mut rows: [Vec<u64>; 4] = [vec![0; words], vec![0; words], vec![0; words], vec![0; words]];
    let mut lcs = vec![0u8; n];
    for i in 0..n {
        if i > 0 {
            let common = kmers[i - 1].iter().rev().zip(kmers[i].iter().rev()).take_while(|(a, b)| a == b && **a != b'$').count();
            lcs[i] = common as u8;
        }
        let first_of_group = i == 0 || kmers[i - 1][1..] != kmers[i][1..];
        if !first_of_group { continue; }
        for (ci, c) in b"ACGT".iter().enumerate() {
            let mut target = kmers[i][1..].to_vec();
            target.push(*c);
            if kmers.binary_search_by(|row| colex(row, &target)).is_ok() { rows[ci][i >> 6] |= 1u64 << (i & 63); }
        }
    }
    let mut c = [1u64; 4];
    for ci in 1..4 { c[ci] = c[ci - 1] + rows[ci - 1].iter().map(|w| w.count_ones() as u64).sum::<u64>(); }
    SbwtParts { k, n_sets: n, n_kmers: sbwt.n_kmers(), rows, c, lcs }
}

impl GpuIndex {
    /// `kbo::build` (lib.rs:501-506) with this library's own builder.
    pub fn build(seqs: &[Vec<u8>], opts: &kbo::BuildOpts) -> Self {
        let ptrs: Vec<*const u8> = seqs.iter().map(|s| s.as_ptr()).collect();
        let lens: Vec<usize> = seqs.iter().map(|s| s.len()).collect();
        let o = ffi::KboBuildOpts { k: opts.k as u32, add_revcomp: opts.add_revcomp as i32, num_threads: opts.num_threads as u32,
                                    prefix_precalc: opts.prefix_precalc as u32, build_select: opts.build_select as i32,
                                    mem_gb: opts.mem_gb as u32, dedup_batches: opts.dedup_batches as i32, temp_dir: std::ptr::null() };
        let mut h = std::ptr::null_mut();
        check(unsafe { ffi::kbo_index_build(ptrs.as_ptr(), lens.as_ptr(), seqs.len(), &o, &mut h) });
        GpuIndex(h)
    }
    /// 1 for an ordinary index; more when the input had 3.76e9 rows or more (a human genome with `add_revcomp`) and was built as
    /// shards: `matches` / `find` / `map` without refinement give the one index's results, `call` / gap filling / save are refused.
    pub fn shards(&self) -> usize { unsafe { ffi::kbo_index_shards(self.0) as usize } }
    /// An index the sbwt crate already built (what `kbo::build` returns, what kbo-cli loads from `.sbwt` / `.lcs`).
    pub fn from_sbwt(index: &sbwt::SbwtIndexVariant) -> Self {
        let sbwt::SbwtIndexVariant::SubsetMatrix(ref sbwt) = index;
        let p = export_sbwt_parts(sbwt);
        let ptrs: Vec<*const u64> = p.rows.iter().map(|r| r.as_ptr()).collect();
        let mut h = std::ptr::null_mut();
        check(unsafe { ffi::kbo_index_from_parts(p.k as u32, p.n_sets as u64, p.n_kmers as u64, ptrs.as_ptr(), p.c.as_ptr(),
                                                 p.lcs.as_ptr(), &mut h) });
        GpuIndex(h)
    }
}

/// `kbo::index::query_sbwt` (index.rs:243-256)
pub fn query_sbwt(query: &[u8], idx: &GpuIndex) -> Vec<(usize, Range<usize>)> {
    let n = query.len();
    let (mut d, mut lo, mut hi) = (vec![0u64; n], vec![0u64; n], vec![0u64; n]);
    check(unsafe { ffi::kbo_matching_statistics(idx.0, query.as_ptr(), n, d.as_mut_ptr(), lo.as_mut_ptr(), hi.as_mut_ptr()) });
    (0..n).map(|i| (d[i] as usize, lo[i] as usize..hi[i] as usize)).collect()
}

/// `kbo::matches` (lib.rs:612-628)
pub fn matches(query_seq: &[u8], idx: &GpuIndex, opts: kbo::MatchOpts) -> Vec<char> {
    let mut out = vec![0u32; query_seq.len()];
    check(unsafe { ffi::kbo_matches(idx.0, query_seq.as_ptr(), query_seq.len(), opts.max_error_prob, out.as_mut_ptr()) });
    out.into_iter().map(|c| char::from_u32(c).unwrap()).collect()
}

/// `kbo::find` (lib.rs:808-821)
pub fn find(query_seq: &[u8], idx: &GpuIndex, opts: kbo::FindOpts) -> Vec<kbo::format::RLE> {
    let (mut p, mut n) = (std::ptr::null_mut(), 0usize);
    let o = ffi::KboFindOpts { max_error_prob: opts.max_error_prob, max_gap_len: opts.max_gap_len };
    check(unsafe { ffi::kbo_find(idx.0, query_seq.as_ptr(), query_seq.len(), &o, &mut p, &mut n) });
    let v = unsafe { std::slice::from_raw_parts(p, n) }.iter().map(|r| kbo::format::RLE {
        start: r.start as usize, end: r.end as usize, matches: r.matches as usize, mismatches: r.mismatches as usize,
        jumps: r.jumps as usize, gap_bases: r.gap_bases as usize, gap_opens: r.gap_opens as usize }).collect();
    unsafe { ffi::kbo_free(p as *mut c_void) };
    v
}

/// `kbo::find` over all reads of a file at once, 2-bit packed over PCIe (`kbo_find_batch_packed`): reads[i] -> its runs.
pub fn find_batch(reads: &[Vec<u8>], idx: &GpuIndex, opts: kbo::FindOpts) -> Vec<Vec<kbo::format::RLE>> {
    let mut offsets = vec![0u64; reads.len() + 1];
    for (i, r) in reads.iter().enumerate() { offsets[i + 1] = offsets[i] + r.len() as u64; }
    let concat: Vec<u8> = reads.concat();
    let mut words = vec![0u32; unsafe { ffi::kbo_packed_words(offsets.as_ptr(), reads.len()) }];
    let cap = concat.iter().filter(|b| !matches!(**b, b'A' | b'C' | b'G' | b'T')).count();
    let (mut exc_pos, mut exc_byte, mut n_exc) = (vec![0u64; cap], vec![0u8; cap], 0usize);
    check(unsafe { ffi::kbo_pack_reads(concat.as_ptr(), offsets.as_ptr(), reads.len(), words.as_mut_ptr(), exc_pos.as_mut_ptr(),
                                       exc_byte.as_mut_ptr(), cap, &mut n_exc) });
    let o = ffi::KboFindOpts { max_error_prob: opts.max_error_prob, max_gap_len: opts.max_gap_len };
    let (mut p, mut ro) = (std::ptr::null_mut(), vec![0u64; reads.len() + 1]);
    check(unsafe { ffi::kbo_find_batch_packed(idx.0, words.as_ptr(), offsets.as_ptr(), reads.len(), exc_pos.as_ptr(), exc_byte.as_ptr(),
                                              n_exc, &o, &mut p, ro.as_mut_ptr()) });
    let all = unsafe { std::slice::from_raw_parts(p, ro[reads.len()] as usize) };
    let out = (0..reads.len()).map(|i| all[ro[i] as usize..ro[i + 1] as usize].iter().map(|r| kbo::format::RLE {
        start: r.start as usize, end: r.end as usize, matches: r.matches as usize, mismatches: r.mismatches as usize,
        jumps: r.jumps as usize, gap_bases: r.gap_bases as usize, gap_opens: r.gap_opens as usize }).collect()).collect();
    unsafe { ffi::kbo_free(p as *mut c_void) };
    out
}

/// `kbo_aln_summary`: what `kbo::matches` returns for one sequence, counted on the device - its numbers of 'M', 'X' and 'R' and of
/// maximal stretches without '-' (the runs `kbo::find` reports with `max_gap_len = 0`).  The '-' are `len - (n_match + n_mismatch + n_jump)`.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct AlnSummary {
    pub n_match: u32,
    pub n_mismatch: u32,
    pub n_jump: u32,
    pub n_runs: u32,
}

/// One `AlnSummary` per read, 2-bit packed on the way in and 16 bytes per read on the way back (`kbo_summary_batch_packed`):
/// screening, presence / absence, identity and coverage.  Reads of up to 160 bases over an index with a depth table are counted inside the
/// mapping kernel and no character is ever made; longer sequences keep a byte per base in device memory, counted there by a second kernel -
/// either way no character crosses PCIe.  Panics (through `check`, like the other wrappers) when the library refuses the batch: every
/// read must have 3 bases or more (`kbo::matches` asserts the same), and the batch must not be empty.
pub fn summary_batch(reads: &[Vec<u8>], idx: &GpuIndex, opts: kbo::MatchOpts) -> Vec<AlnSummary> {
    let mut offsets = vec![0u64; reads.len() + 1];
    for (i, r) in reads.iter().enumerate() { offsets[i + 1] = offsets[i] + r.len() as u64; }
    let concat: Vec<u8> = reads.concat();
    let mut words = vec![0u32; unsafe { ffi::kbo_packed_words(offsets.as_ptr(), reads.len()) }];
    let cap = concat.iter().filter(|b| !matches!(**b, b'A' | b'C' | b'G' | b'T')).count();
    let (mut exc_pos, mut exc_byte, mut n_exc) = (vec![0u64; cap], vec![0u8; cap], 0usize);
    check(unsafe { ffi::kbo_pack_reads(concat.as_ptr(), offsets.as_ptr(), reads.len(), words.as_mut_ptr(), exc_pos.as_mut_ptr(),
                                       exc_byte.as_mut_ptr(), cap, &mut n_exc) });
    let mut out = vec![AlnSummary::default(); reads.len()];
    check(unsafe { ffi::kbo_summary_batch_packed(idx.0, words.as_ptr(), offsets.as_ptr(), reads.len(), exc_pos.as_ptr(), exc_byte.as_ptr(),
                                                 n_exc, opts.max_error_prob, out.as_mut_ptr()) });
    out
}

pub const STRAND_FWD: c_int = 1;
pub const STRAND_REV: c_int = 2;

/// `kbo::find` of every read and of its reverse complement (what kbo-cli runs per strand), 2-bit packed over PCIe and staged once
/// (`kbo_find_batch_packed_strands`): reads[i] -> (its '+' runs, its '-' runs).  The '-' runs are in the coordinates of the
/// reverse-complemented read: position p there is base len - 1 - p of reads[i].
pub fn find_batch_strands(reads: &[Vec<u8>], idx: &GpuIndex, opts: kbo::FindOpts) -> Vec<(Vec<kbo::format::RLE>, Vec<kbo::format::RLE>)> {
    let n = reads.len();
    let mut offsets = vec![0u64; n + 1];
    for (i, r) in reads.iter().enumerate() { offsets[i + 1] = offsets[i] + r.len() as u64; }
    let concat: Vec<u8> = reads.concat();
    let mut words = vec![0u32; unsafe { ffi::kbo_packed_words(offsets.as_ptr(), n) }];
    let cap = concat.iter().filter(|b| !matches!(**b, b'A' | b'C' | b'G' | b'T')).count();
    let (mut exc_pos, mut exc_byte, mut n_exc) = (vec![0u64; cap], vec![0u8; cap], 0usize);
    check(unsafe { ffi::kbo_pack_reads(concat.as_ptr(), offsets.as_ptr(), n, words.as_mut_ptr(), exc_pos.as_mut_ptr(),
                                       exc_byte.as_mut_ptr(), cap, &mut n_exc) });
    let o = ffi::KboFindOpts { max_error_prob: opts.max_error_prob, max_gap_len: opts.max_gap_len };
    let (mut p, mut ro) = (std::ptr::null_mut(), vec![0u64; 2 * n + 1]);
    check(unsafe { ffi::kbo_find_batch_packed_strands(idx.0, words.as_ptr(), offsets.as_ptr(), n, exc_pos.as_ptr(), exc_byte.as_ptr(),
                                                      n_exc, &o, STRAND_FWD | STRAND_REV, &mut p, ro.as_mut_ptr()) });
    let all = unsafe { std::slice::from_raw_parts(p, ro[2 * n] as usize) };
    let runs = |j: usize| -> Vec<kbo::format::RLE> { all[ro[j] as usize..ro[j + 1] as usize].iter().map(|r| kbo::format::RLE {
        start: r.start as usize, end: r.end as usize, matches: r.matches as usize, mismatches: r.mismatches as usize,
        jumps: r.jumps as usize, gap_bases: r.gap_bases as usize, gap_opens: r.gap_opens as usize }).collect() };
    let out = (0..n).map(|i| (runs(2 * i), runs(2 * i + 1))).collect();
    unsafe { ffi::kbo_free(p as *mut c_void) };
    out
}

/// `kbo::call` (lib.rs:547-573) with every sequence of a batch as `ref_seq` (`kbo_call_batch`).
pub fn call_batch(idx: &GpuIndex, seqs: &[Vec<u8>], opts: &kbo::CallOpts) -> Vec<Vec<kbo::variant_calling::Variant>> {
    let mut offsets = vec![0u64; seqs.len() + 1];
    for (i, r) in seqs.iter().enumerate() { offsets[i + 1] = offsets[i] + r.len() as u64; }
    let concat: Vec<u8> = seqs.concat();
    let b = &opts.sbwt_build_opts;
    let o = ffi::KboCallOpts { max_error_prob: opts.max_error_prob, sbwt_build_opts: ffi::KboBuildOpts {
        k: b.k as u32, add_revcomp: b.add_revcomp as i32, num_threads: b.num_threads as u32, prefix_precalc: b.prefix_precalc as u32,
        build_select: b.build_select as i32, mem_gb: b.mem_gb as u32, dedup_batches: b.dedup_batches as i32, temp_dir: std::ptr::null() } };
    // the flat form (`kbo_call_batch_flat`): the device's own order and layout, one allocation, 10 bytes per variant - the two
    // `Vec<u8>` of every `Variant` are made from slices of `chars` here, where the reference's type asks for them
    let mut flat = ffi::KboCallFlat { n_variants: 0, n_chars: 0, query_pos: std::ptr::null_mut(), query_len: std::ptr::null_mut(),
                                      ref_len: std::ptr::null_mut(), chars: std::ptr::null_mut() };
    let mut vo = vec![0u64; seqs.len() + 1];
    check(unsafe { ffi::kbo_call_batch_flat(idx.0, concat.as_ptr(), offsets.as_ptr(), seqs.len(), &o, &mut flat, vo.as_mut_ptr()) });
    let nv = flat.n_variants as usize;
    let (pos, ql, rl, chars) = unsafe { (std::slice::from_raw_parts(flat.query_pos, nv), std::slice::from_raw_parts(flat.query_len, nv),
                                         std::slice::from_raw_parts(flat.ref_len, nv), std::slice::from_raw_parts(flat.chars, flat.n_chars as usize)) };
    let mut c = 0usize;
    let mut out = Vec::with_capacity(seqs.len());
    for s in 0..seqs.len() {
        let mut vs = Vec::with_capacity((vo[s + 1] - vo[s]) as usize);
        for v in vo[s] as usize..vo[s + 1] as usize {
            let (a, b) = (ql[v] as usize, rl[v] as usize);
            vs.push(kbo::variant_calling::Variant { query_pos: pos[v] as usize, query_chars: chars[c..c + a].to_vec(),
                                                    ref_chars: chars[c + a..c + a + b].to_vec() });
            c += a + b;
        }
        out.push(vs);
    }
    unsafe { ffi::kbo_call_flat_free(&mut flat) };
    out
}

/// The recipe that turns SURVEY.md section 8(f) 4 from "unpinned" into "pinned" on a machine that has the `sbwt` crate and an MI355X
/// (neither is in the image this was written in: never compiled, never run).  The reference's own test inputs (index.rs:262-275,
/// lib.rs:600-609, lib.rs:786-805): the index the crate builds, handed over by `export_sbwt_parts` -> `kbo_index_from_parts`, must
/// give what `sbwt::StreamingIndex::matching_statistics` gives - depths AND intervals - and `matches` / `find` must give the crate's.
// (never compiled - no Rust toolchain in the image this was written in - so behind a feature of its own: a plain `cargo test` must not
// break on a signature this module assumes wrongly.  `cargo test --features pin-tests` on a machine with the crate and a GPU.)
#[cfg(all(test, feature = "pin-tests"))]
mod pin_against_the_crate {
    use super::*;

    fn crate_ms(query: &[u8], index: &sbwt::SbwtIndexVariant, lcs: &sbwt::LcsArray) -> Vec<(usize, Range<usize>)> {
        kbo::index::query_sbwt(query, index, lcs) // index.rs:243-256: StreamingIndex::new + matching_statistics
    }

    #[test]
    fn query_sbwt_of_the_handed_over_index_equals_the_crates() {
        // index.rs:265-268
        let reference: Vec<Vec<u8>> = vec![b"AAAGAACCA-TCAGGGCG".to_vec()];
        let query = b"CAAGCCACTCATTGGGTC".to_vec();
        let mut opts = kbo::BuildOpts::default();
        opts.k = 3;
        let (sbwt, lcs) = kbo::index::build_sbwt_from_vecs(&reference, &Some(opts));
        let gpu = GpuIndex::from_sbwt(&sbwt);
        let want = crate_ms(&query, &sbwt, &lcs);
        assert_eq!(want.iter().map(|x| x.0).collect::<Vec<_>>(), vec![1, 2, 2, 3, 2, 2, 3, 2, 1, 2, 3, 1, 1, 1, 2, 3, 1, 2]); // index.rs:270
        assert_eq!(query_sbwt(&query, &gpu), want); // depths and intervals
    }

    #[test]
    fn random_genome_every_position() {
        // 50 kbp, k = 31, 1 % substitutions, a few N: depths and intervals of 200 reads of 150 bases and of one 20 kbp sequence
        let mut x = 0x6B626F0001u64;
        let mut next = || { x = x.wrapping_add(0x9E3779B97F4A7C15); let mut z = x; z = (z ^ (z >> 30)).wrapping_mul(0xBF58476D1CE4E5B9);
                            z = (z ^ (z >> 27)).wrapping_mul(0x94D049BB133111EB); z ^ (z >> 31) };
        let genome: Vec<u8> = (0..50_000).map(|_| b"ACGT"[(next() >> 62) as usize]).collect();
        let (sbwt, lcs) = kbo::index::build_sbwt_from_vecs(&[genome.clone()], &Some(kbo::BuildOpts::default()));
        let gpu = GpuIndex::from_sbwt(&sbwt);
        let mut reads: Vec<Vec<u8>> = (0..200).map(|_| { let s = (next() % (50_000 - 150)) as usize; genome[s..s + 150].to_vec() }).collect();
        reads.push(genome[10_000..30_000].to_vec());
        for r in reads.iter_mut() {
            for b in r.iter_mut() { let v = next(); if (v & 0xFFFF) < 655 { *b = b"ACGT"[(v >> 62) as usize]; } else if (v & 0xFFFFF) == 7 { *b = b'N'; } }
            assert_eq!(query_sbwt(r, &gpu), crate_ms(r, &sbwt, &lcs));
        }
    }

    #[test]
    fn matches_and_find_equal_the_crates() {
        // lib.rs:600-609
        let reference: Vec<Vec<u8>> = vec![b"AAAGAACCA-TCAGGGCG".to_vec()];
        let query = b"GTGACTATGAGGAT".to_vec();
        let mut opts = kbo::BuildOpts::default();
        opts.k = 3;
        let (sbwt, lcs) = kbo::build(&reference, opts);
        let gpu = GpuIndex::from_sbwt(&sbwt);
        assert_eq!(matches(&query, &gpu, kbo::MatchOpts::default()), kbo::matches(&query, &sbwt, &lcs, kbo::MatchOpts::default()));
        assert_eq!(matches(&query, &gpu, kbo::MatchOpts::default()).iter().collect::<String>(), "---------MMM--"); // lib.rs:607
        assert_eq!(find(&query, &gpu, kbo::FindOpts::default()), kbo::find(&query, &sbwt, &lcs, kbo::FindOpts::default()));
    }
}
