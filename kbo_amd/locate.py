"""Positions, segments, depth, placement (kbo_hip.h): where a batch lies on the sequences an index was built from.

add_positions() gives an index its position table; segments() turns a batch into collinear blocks of exact k-mer matches in source
coordinates and, when asked, the depth of every source base; segments_dev() / depth_finish_dev() are the same over device buffers.
place() chains the segments of every sequence to one record - source, strand, extent, score, runner-up; place_dev() is the same over
device buffers behind segments_dev(), place_from_segments_host() its restatement on the CPU.
pileup() counts what the reads say at every source base and gives the candidate sites; pileup_dev() / pileup_sites_dev() are the same
over device buffers behind segments_dev() and depth_finish_dev(), pileup_from_segments_host() / pileup_sites_host() their restatements
on the CPU, pileup_snps() the step from sites to substitutions against the source text.
indels() gives the insertion and deletion sites - one event per clean junction of two consecutive segments, the events of all batches
and strands sorted and counted; indels_dev() / indel_sites_dev() are the same over device buffers behind segments_dev() and
depth_finish_dev(), indels_from_segments_host() / indel_sites_host() their restatements on the CPU, indel_variants() the step from
sites to deleted and inserted bytes against the source text.
"""
import ctypes as C

import numpy as np

from ._capi import check, lib
from .index import SbwtIndexVariant, _u8

STRAND_FWD, STRAND_REV = 1, 2
POS_NONE, MULTI, REV, POS_MASK = 0xFFFFFFFF, 1 << 31, 1 << 30, (1 << 30) - 1
SEG_REV, SEG_FIRST_MULTI, SEG_LAST_MULTI = 1, 4, 8

# kbo_seq_segment
SEGMENT_DTYPE = np.dtype([(n, "<u4") for n in ("seq", "strand", "q_first", "q_last", "pos_first", "pos_last", "flags")])
# kbo_seq_place
PLACE_NONE, PLACE_REV, PLACE_SPILLS, PLACE_WINDOW, PLACE_LANE_MAX = 0xFFFFFFFF, 1, 2, 64, 4
PLACE_DTYPE = np.dtype([("source", "<u4"), ("strand", "<u2"), ("flags", "<u2")] + [(n, "<u4") for n in (
    "q_start", "q_end", "pos_start", "pos_end", "score", "n_segs", "indel", "n_multi", "second", "reserved")])
assert PLACE_DTYPE.itemsize == 48
# kbo_pile_site
SITE_DTYPE = np.dtype([("pos", "<u4"), ("source", "<u4"), ("depth", "<u4"), ("count", "<u4", (4,)), ("reserved", "<u4")])
assert SITE_DTYPE.itemsize == 32
SNP_DTYPE = np.dtype([("source", "<u4"), ("pos", "<u4"), ("ref", "u1"), ("alt", "u1"), ("count", "<u4"), ("depth", "<u4")])


def _batch(query_seqs):
    """(concat uint8, offsets uint64) of a list of sequences, or the pair itself"""
    if isinstance(query_seqs, tuple) and len(query_seqs) == 2 and isinstance(query_seqs[1], np.ndarray):
        return np.ascontiguousarray(query_seqs[0], dtype=np.uint8), np.ascontiguousarray(query_seqs[1], dtype=np.uint64)
    seqs = [_u8(s) for s in query_seqs]
    offsets = np.zeros(len(seqs) + 1, dtype=np.uint64)
    if seqs:
        offsets[1:] = np.cumsum([len(s) for s in seqs])
    concat = np.concatenate(seqs) if seqs else np.zeros(0, dtype=np.uint8)
    return np.ascontiguousarray(concat, dtype=np.uint8), offsets


def add_positions(sbwt, seqs, add_revcomp=False, device=-1):
    """kbo_index_add_positions: the position table of `sbwt`, made on `device` from the sequences it was built from"""
    seqs = [bytes(_u8(s)) for s in seqs]
    arr = (C.c_char_p * max(1, len(seqs)))(*seqs)
    lens = (C.c_size_t * max(1, len(seqs)))(*[len(s) for s in seqs])
    check(lib().kbo_index_add_positions(sbwt._h, arr, lens, len(seqs), int(bool(add_revcomp)), int(device)))
    return sbwt


def has_positions(sbwt):
    return bool(lib().kbo_index_has_positions(sbwt._h))


def positions(sbwt):
    """uint32[n_sets]: the entry of every row (kbo_index_positions)"""
    n = C.c_size_t(0)
    check(lib().kbo_index_positions(sbwt._h, None, C.byref(n)))
    out = np.zeros(n.value, dtype=np.uint32)
    check(lib().kbo_index_positions(sbwt._h, out.ctypes.data, C.byref(n)))
    return out


def source_offsets(sbwt):
    """uint64[n_seqs + 1]: where every source sequence begins in source coordinates (kbo_index_source_offsets)"""
    n = C.c_size_t(0)
    check(lib().kbo_index_source_offsets(sbwt._h, None, C.byref(n)))
    out = np.zeros(n.value, dtype=np.uint64)
    check(lib().kbo_index_source_offsets(sbwt._h, out.ctypes.data, C.byref(n)))
    return out


SbwtIndexVariant.positions = positions
SbwtIndexVariant.source_offsets = source_offsets
SbwtIndexVariant.has_positions = has_positions


def segments(query_seqs, sbwt, bridge=None, strands=STRAND_FWD, depth=False):
    """kbo_segments_batch -> records (SEGMENT_DTYPE) in (seq, strand, q_first) order, or (records, depth uint32[source bases]).
    query_seqs: a list of sequences or (concat, offsets); bridge: None = k"""
    concat, offsets = _batch(query_seqs)
    b = sbwt.k() if bridge is None else int(bridge)
    p, n = C.c_void_p(), C.c_uint64(0)
    d = np.zeros(int(lib().kbo_index_source_bases(sbwt._h)), dtype=np.uint32) if depth else None
    check(lib().kbo_segments_batch(sbwt._h, concat.ctypes.data if len(concat) else None, offsets.ctypes.data, len(offsets) - 1, min(b, 0xFFFFFFFF), int(strands),
                                   C.byref(p), C.byref(n), d.ctypes.data if depth else None))
    try:
        recs = np.frombuffer(C.string_at(p.value, n.value * SEGMENT_DTYPE.itemsize), dtype=SEGMENT_DTYPE).copy()
    finally:
        lib().kbo_free(p)
    return (recs, d) if depth else recs


def segments_work_bytes(n_seqs, total_bases):
    return int(lib().kbo_segments_work_bytes(n_seqs, total_bases))


def segments_dev(sbwt, ms, lo, offsets, n_seqs, total_bases, segs, capacity, n_segs, work, work_bytes=None, bridge=None, strand=STRAND_FWD,
                 delta=None, stream=None):
    """kbo_segments_dev over torch tensors (or raw device pointers) as kbo_ms_batch_dev left them; everything on `stream`"""
    def ptr(x):
        return None if x is None else x if isinstance(x, int) else x.data_ptr()
    b = sbwt.k() if bridge is None else int(bridge)
    wb = segments_work_bytes(n_seqs, total_bases) if work_bytes is None else int(work_bytes)
    s = stream.cuda_stream if hasattr(stream, "cuda_stream") else stream
    check(lib().kbo_segments_dev(sbwt._h, ptr(ms), ptr(lo), ptr(offsets), n_seqs, total_bases, b, int(strand), ptr(segs), int(capacity), ptr(n_segs),
                                 ptr(delta), ptr(work), wb, s))


def depth_work_bytes(sbwt):
    return int(lib().kbo_depth_work_bytes(sbwt._h))


def depth_finish_dev(sbwt, delta, depth, work, work_bytes=None, stream=None):
    """kbo_depth_finish_dev: depth = the inclusive prefix sums of delta"""
    def ptr(x):
        return None if x is None else x if isinstance(x, int) else x.data_ptr()
    wb = depth_work_bytes(sbwt) if work_bytes is None else int(work_bytes)
    s = stream.cuda_stream if hasattr(stream, "cuda_stream") else stream
    check(lib().kbo_depth_finish_dev(sbwt._h, ptr(delta), ptr(depth), ptr(work), wb, s))


def segment_source(segs, src_off):
    """(source sequence, offset of the segment's lowest base within it, orientation 0 = FWD / 1 = REV) of every record; src_off: the
    index's source_offsets()"""
    off = np.asarray(src_off, dtype=np.uint64)
    low = np.where(segs["flags"] & SEG_REV, segs["pos_last"], segs["pos_first"]).astype(np.uint64)
    src = np.searchsorted(off, low, side="right") - 1
    return src, low - off[src], (segs["flags"] & SEG_REV).astype(np.uint8)


def positions_from_ms_host(k, n_sets, d, lo, offsets, src_off, rev, entries):
    """kbo_positions_from_ms_host: one strand's walk of the sources merged into `entries` (uint32[n_sets], in place); returns n_not_full"""
    d = np.ascontiguousarray(d, dtype=np.uint8)
    lo = np.ascontiguousarray(lo, dtype=np.uint32)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    src_off = np.ascontiguousarray(src_off, dtype=np.uint64)
    assert entries.dtype == np.uint32 and entries.flags.c_contiguous and len(entries) == n_sets
    miss = C.c_uint64(0)
    check(lib().kbo_positions_from_ms_host(k, n_sets, d.ctypes.data, lo.ctypes.data, offsets.ctypes.data, len(offsets) - 1, src_off.ctypes.data, int(rev),
                                           entries.ctypes.data, C.byref(miss)))
    return int(miss.value)


def segments_from_ms_host(entries, k, d, lo, offsets, bridge, strand, capacity, source_bases, delta=None):
    """kbo_segments_from_ms_host -> (records written, count); delta (uint32[source_bases + 1]) is added to in place"""
    entries = np.ascontiguousarray(entries, dtype=np.uint32)
    d = np.ascontiguousarray(d, dtype=np.uint8)
    lo = np.ascontiguousarray(lo, dtype=np.uint32)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    segs = np.zeros(capacity, dtype=SEGMENT_DTYPE)
    n = C.c_uint64(0)
    if delta is not None:
        assert delta.dtype == np.uint32 and delta.flags.c_contiguous and len(delta) == source_bases + 1
    check(lib().kbo_segments_from_ms_host(entries.ctypes.data, len(entries), k, d.ctypes.data, lo.ctypes.data, offsets.ctypes.data, len(offsets) - 1,
                                          bridge, strand, segs.ctypes.data if capacity else None, capacity, C.byref(n),
                                          delta.ctypes.data if delta is not None else None, source_bases))
    return segs[:min(capacity, n.value)], int(n.value)


def place(query_seqs, sbwt, bridge=None, strands=STRAND_FWD, max_gap=1000, max_indel=100):
    """kbo_place_batch -> one record (PLACE_DTYPE) per sequence: the best chain of its segments over the strands asked for; source ==
    PLACE_NONE for a sequence without a segment.  query_seqs: a list of sequences or (concat, offsets); bridge: None = k.
    max_gap (query bases between two segments of a chain) and max_indel (bases the diagonal may move between them) default to 1000 and
    100: choices that suit reads up to a few 10 kbp with small indels, not derived figures"""
    concat, offsets = _batch(query_seqs)
    b = sbwt.k() if bridge is None else int(bridge)
    out = np.zeros(len(offsets) - 1, dtype=PLACE_DTYPE)
    check(lib().kbo_place_batch(sbwt._h, concat.ctypes.data if len(concat) else None, offsets.ctypes.data, len(offsets) - 1, min(b, 0xFFFFFFFF), int(strands),
                                int(max_gap), int(max_indel), out.ctypes.data if len(out) else None))
    return out


def place_work_bytes(n_seqs, capacity):
    return int(lib().kbo_place_work_bytes(n_seqs, capacity))


def place_dev(sbwt, segs, n_segs, capacity, n_seqs, place_out, work, work_bytes=None, max_gap=1000, max_indel=100, merge=False, stream=None):
    """kbo_place_dev over torch tensors (or raw device pointers): segs, n_segs and capacity as segments_dev() left them; everything on
    `stream`.  merge: into what place_out holds (the second strand's call)"""
    def ptr(x):
        return None if x is None else x if isinstance(x, int) else x.data_ptr()
    wb = place_work_bytes(n_seqs, capacity) if work_bytes is None else int(work_bytes)
    s = stream.cuda_stream if hasattr(stream, "cuda_stream") else stream
    check(lib().kbo_place_dev(sbwt._h, ptr(segs), ptr(n_segs), int(capacity), n_seqs, int(max_gap), int(max_indel), int(bool(merge)), ptr(place_out),
                              ptr(work), wb, s))


def place_from_segments_host(segs, n_seqs, src_off, k, max_gap=1000, max_indel=100, merge_into=None):
    """kbo_place_from_segments_host -> PLACE_DTYPE[n_seqs]; merge_into: records of an earlier call (another strand) to merge with"""
    segs = np.ascontiguousarray(segs, dtype=SEGMENT_DTYPE)
    src_off = np.ascontiguousarray(src_off, dtype=np.uint64)
    out = np.zeros(n_seqs, dtype=PLACE_DTYPE) if merge_into is None else np.ascontiguousarray(merge_into, dtype=PLACE_DTYPE).copy()
    assert len(out) == n_seqs
    check(lib().kbo_place_from_segments_host(segs.ctypes.data if len(segs) else None, len(segs), n_seqs, src_off.ctypes.data, len(src_off) - 1, k,
                                             int(max_gap), int(max_indel), int(merge_into is not None), out.ctypes.data if n_seqs else None))
    return out


def place_local(rec, src_off):
    """(source, start, end, orientation 0 = FWD / 1 = REV) of one record or an array of them, start and end in the source's own
    coordinates (end may lie beyond the source: PLACE_SPILLS); src_off: the index's source_offsets().  A PLACE_NONE record gives
    (PLACE_NONE, 0, 0, 0)"""
    off = np.asarray(src_off, dtype=np.uint64)
    src = np.asarray(rec["source"], dtype=np.int64)
    none = src == PLACE_NONE
    base = off[np.where(none, 0, src)].astype(np.int64)
    start = np.where(none, 0, np.asarray(rec["pos_start"], dtype=np.int64) - base)
    end = np.where(none, 0, np.asarray(rec["pos_end"], dtype=np.int64) - base)
    return src, start, end, np.where(none, 0, np.asarray(rec["flags"]) & PLACE_REV).astype(np.uint8)


def pileup(query_seqs, sbwt, bridge=None, strands=STRAND_FWD, skip_multi=True, min_count=3, frac_num=1, frac_den=2, depth=False, pile=False):
    """kbo_pileup_batch -> the candidate sites (SITE_DTYPE, ascending pos) of the batch piled up on the sources over the strands asked
    for, or (sites, depth uint32[source bases]) / (sites, pile uint32[source bases, 4]) / (sites, depth, pile).  A site has a column
    with at least min_count reads and count * frac_den >= frac_num * depth; min_count 3 and one half are choices that suit a haploid
    sample at tens of reads a base, not derived figures.  query_seqs: a list of sequences or (concat, offsets); bridge: None = k"""
    concat, offsets = _batch(query_seqs)
    b = sbwt.k() if bridge is None else int(bridge)
    bases = int(lib().kbo_index_source_bases(sbwt._h))
    d = np.zeros(bases, dtype=np.uint32) if depth else None
    pl = np.zeros((bases, 4), dtype=np.uint32) if pile else None
    p, n = C.c_void_p(), C.c_uint64(0)
    check(lib().kbo_pileup_batch(sbwt._h, concat.ctypes.data if len(concat) else None, offsets.ctypes.data, len(offsets) - 1, min(b, 0xFFFFFFFF), int(strands),
                                 int(bool(skip_multi)), int(min_count), int(frac_num), int(frac_den), C.byref(p), C.byref(n),
                                 d.ctypes.data if depth else None, pl.ctypes.data if pile else None))
    try:
        sites = np.frombuffer(C.string_at(p.value, n.value * SITE_DTYPE.itemsize), dtype=SITE_DTYPE).copy()
    finally:
        lib().kbo_free(p)
    extra = tuple(x for x in (d, pl) if x is not None)
    return (sites,) + extra if extra else sites


def pileup_dev(sbwt, concat, ms, offsets, n_seqs, total_bases, segs, n_segs, capacity, pile, skip_multi=True, stream=None):
    """kbo_pileup_dev over torch tensors (or raw device pointers): the batch as it was walked, the MS bytes of that walk, and segs, n_segs
    and capacity as segments_dev() left them; `pile` (uint32[source bases, 4]) is added to; everything on `stream`, no scratch"""
    def ptr(x):
        return None if x is None else x if isinstance(x, int) else x.data_ptr()
    s = stream.cuda_stream if hasattr(stream, "cuda_stream") else stream
    check(lib().kbo_pileup_dev(sbwt._h, ptr(concat), ptr(ms), ptr(offsets), n_seqs, total_bases, ptr(segs), ptr(n_segs), int(capacity), int(bool(skip_multi)),
                               ptr(pile), s))


def pileup_sites_work_bytes(sbwt):
    return int(lib().kbo_pileup_sites_work_bytes(sbwt._h))


def pileup_sites_dev(sbwt, pile, depth, sites, capacity, n_sites, work, work_bytes=None, min_count=3, frac_num=1, frac_den=2, stream=None):
    """kbo_pileup_sites_dev: the sites of `pile` against `depth` as depth_finish_dev() wrote it; record x is written iff x < capacity,
    n_sites (8 bytes) receives the full count"""
    def ptr(x):
        return None if x is None else x if isinstance(x, int) else x.data_ptr()
    wb = pileup_sites_work_bytes(sbwt) if work_bytes is None else int(work_bytes)
    s = stream.cuda_stream if hasattr(stream, "cuda_stream") else stream
    check(lib().kbo_pileup_sites_dev(sbwt._h, ptr(pile), ptr(depth), int(min_count), int(frac_num), int(frac_den), ptr(sites), int(capacity), ptr(n_sites),
                                     ptr(work), wb, s))


def pileup_from_segments_host(segs, concat, ms, offsets, k, source_bases, skip_multi=True, pile=None):
    """kbo_pileup_from_segments_host -> (pile uint32[source_bases, 4], bridged bases of the records taken); pile: an earlier call's
    (another batch or strand) to add to, in place"""
    segs = np.ascontiguousarray(segs, dtype=SEGMENT_DTYPE)
    concat = np.ascontiguousarray(concat, dtype=np.uint8)
    ms = np.ascontiguousarray(ms, dtype=np.uint8)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    if pile is None:
        pile = np.zeros((source_bases, 4), dtype=np.uint32)
    assert pile.dtype == np.uint32 and pile.flags.c_contiguous and pile.shape == (source_bases, 4) and len(ms) >= len(concat)
    n = C.c_uint64(0)
    check(lib().kbo_pileup_from_segments_host(segs.ctypes.data if len(segs) else None, len(segs), concat.ctypes.data if len(concat) else None,
                                              ms.ctypes.data if len(concat) else None, offsets.ctypes.data, len(offsets) - 1, len(concat), k,
                                              int(bool(skip_multi)), pile.ctypes.data if source_bases else None, source_bases, C.byref(n)))
    return pile, int(n.value)


def pileup_sites_host(pile, depth, src_off, capacity=None, min_count=3, frac_num=1, frac_den=2):
    """kbo_pileup_sites_host -> (records written (SITE_DTYPE), count); capacity: None = every site"""
    pile = np.ascontiguousarray(pile, dtype=np.uint32)
    depth = np.ascontiguousarray(depth, dtype=np.uint32)
    src_off = np.ascontiguousarray(src_off, dtype=np.uint64)
    bases = len(depth)
    assert pile.size == 4 * bases
    cap = bases if capacity is None else int(capacity)
    sites = np.zeros(cap, dtype=SITE_DTYPE)
    n = C.c_uint64(0)
    check(lib().kbo_pileup_sites_host(pile.ctypes.data if bases else None, depth.ctypes.data if bases else None, bases, src_off.ctypes.data,
                                      len(src_off) - 1, int(min_count), int(frac_num), int(frac_den), sites.ctypes.data if cap else None, cap, C.byref(n)))
    return sites[:min(cap, n.value)].copy(), int(n.value)


def pileup_snps(sites, sources, min_count=3, frac_num=1, frac_den=2):
    """the substitutions among `sites` against the source text (SNP_DTYPE): the column that equals the source base is dropped - the
    device does not hold the text, and a base between two nearby substitutions is bridged and counted too - and a site gives a row when
    exactly one of its remaining columns meets the thresholds the sites were made with: source, position within the source, ref and
    alt as bytes, the column's count, depth.  sources: the sequences the index was built from, in order"""
    srcs = [_u8(s) for s in sources]
    off = np.concatenate([[0], np.cumsum([len(s) for s in srcs])]).astype(np.int64)
    out = []
    for st in sites:
        src, at = int(st["source"]), int(st["pos"]) - int(off[int(st["source"])])
        ref = int(srcs[src][at])
        depth = int(st["depth"])
        alts = [(b, int(c)) for b, c in zip(b"ACGT", st["count"]) if b != ref and c >= min_count and int(c) * frac_den >= frac_num * depth]
        if len(alts) == 1:
            out.append((src, at, ref, alts[0][0], alts[0][1], depth))
    return np.array(out, dtype=SNP_DTYPE)


# kbo_indel_event, kbo_indel_site
INDEL_INS, INDEL_LONG, INDEL_LEN_MASK, INDEL_MINUS, INDEL_CODE_LEN = 1 << 31, 1 << 30, (1 << 30) - 1, 1, 16
INDEL_EVENT_DTYPE = np.dtype([(n, "<u4") for n in ("pos", "kind_len", "code", "flags")])
INDEL_SITE_DTYPE = np.dtype([(n, "<u4") for n in ("pos", "source", "kind_len", "code", "count", "n_minus", "depth", "reserved")])
assert INDEL_EVENT_DTYPE.itemsize == 16 and INDEL_SITE_DTYPE.itemsize == 32


def indels(query_seqs, sbwt, bridge=None, strands=STRAND_FWD, skip_multi=True, max_indel=16, min_count=3, frac_num=1, frac_den=2, depth=False):
    """kbo_indels_batch -> the insertion and deletion sites (INDEL_SITE_DTYPE, ascending (pos, kind_len, code)) of the batch over the
    strands asked for, or (sites, depth uint32[source bases]).  A site is a group of equal events - one per clean junction of two
    consecutive segments of a read - with at least min_count events and count * frac_den >= frac_num * the depth of the base in front;
    max_indel 16, min_count 3 and one half are choices that suit a haploid sample at tens of reads a base, not derived figures.
    query_seqs: a list of sequences or (concat, offsets); bridge: None = k"""
    concat, offsets = _batch(query_seqs)
    b = sbwt.k() if bridge is None else int(bridge)
    d = np.zeros(int(lib().kbo_index_source_bases(sbwt._h)), dtype=np.uint32) if depth else None
    p, n = C.c_void_p(), C.c_uint64(0)
    check(lib().kbo_indels_batch(sbwt._h, concat.ctypes.data if len(concat) else None, offsets.ctypes.data, len(offsets) - 1, min(b, 0xFFFFFFFF), int(strands),
                                 int(bool(skip_multi)), int(max_indel), int(min_count), int(frac_num), int(frac_den), C.byref(p), C.byref(n),
                                 d.ctypes.data if depth else None))
    try:
        sites = np.frombuffer(C.string_at(p.value, n.value * INDEL_SITE_DTYPE.itemsize), dtype=INDEL_SITE_DTYPE).copy()
    finally:
        lib().kbo_free(p)
    return (sites, d) if depth else sites


def indels_work_bytes(capacity):
    return int(lib().kbo_indels_work_bytes(int(capacity)))


def indels_dev(sbwt, concat, offsets, n_seqs, total_bases, segs, n_segs, capacity, events, event_capacity, n_events, work, work_bytes=None,
               skip_multi=True, max_indel=16, stream=None):
    """kbo_indels_dev over torch tensors (or raw device pointers): the batch as it was walked and segs, n_segs and capacity as
    segments_dev() left them; the events are appended to `events` behind n_events (8 bytes, zeroed once by the caller, shared by batches
    and strands), which becomes the full count; everything on `stream`"""
    def ptr(x):
        return None if x is None else x if isinstance(x, int) else x.data_ptr()
    wb = indels_work_bytes(capacity) if work_bytes is None else int(work_bytes)
    s = stream.cuda_stream if hasattr(stream, "cuda_stream") else stream
    check(lib().kbo_indels_dev(sbwt._h, ptr(concat), ptr(offsets), n_seqs, total_bases, ptr(segs), ptr(n_segs), int(capacity), int(bool(skip_multi)),
                               int(max_indel), ptr(events), int(event_capacity), ptr(n_events), ptr(work), wb, s))


def indel_sites_work_bytes(event_capacity):
    return int(lib().kbo_indel_sites_work_bytes(int(event_capacity)))


def indel_sites_dev(sbwt, events, n_events, event_capacity, depth, sites, site_capacity, n_sites, work, work_bytes=None, min_count=3, frac_num=1,
                    frac_den=2, stream=None):
    """kbo_indel_sites_dev: the first min(n_events, event_capacity) events sorted, grouped and counted against `depth` as
    depth_finish_dev() wrote it; site x is written iff x < site_capacity, n_sites (8 bytes) receives the full count"""
    def ptr(x):
        return None if x is None else x if isinstance(x, int) else x.data_ptr()
    wb = indel_sites_work_bytes(event_capacity) if work_bytes is None else int(work_bytes)
    s = stream.cuda_stream if hasattr(stream, "cuda_stream") else stream
    check(lib().kbo_indel_sites_dev(sbwt._h, ptr(events), ptr(n_events), int(event_capacity), ptr(depth), int(min_count), int(frac_num), int(frac_den),
                                    ptr(sites), int(site_capacity), ptr(n_sites), ptr(work), wb, s))


def indels_from_segments_host(segs, concat, offsets, k, src_off, skip_multi=True, max_indel=16, events=None, n_events=0, capacity=None):
    """kbo_indels_from_segments_host -> (the list (INDEL_EVENT_DTYPE[capacity]), its full count, the complex junctions of this call);
    events, n_events: the list of earlier calls (other batches or strands) to append to, in place; capacity: None = one event per record
    on top of what the list holds"""
    segs = np.ascontiguousarray(segs, dtype=SEGMENT_DTYPE)
    concat = np.ascontiguousarray(concat, dtype=np.uint8)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    src_off = np.ascontiguousarray(src_off, dtype=np.uint64)
    if events is None:
        events = np.zeros(int(n_events) + len(segs) if capacity is None else int(capacity), dtype=INDEL_EVENT_DTYPE)
    assert events.dtype == INDEL_EVENT_DTYPE and events.flags.c_contiguous
    n, cx = C.c_uint64(int(n_events)), C.c_uint64(0)
    check(lib().kbo_indels_from_segments_host(segs.ctypes.data if len(segs) else None, len(segs), concat.ctypes.data if len(concat) else None,
                                              offsets.ctypes.data, len(offsets) - 1, len(concat), k, int(bool(skip_multi)), int(max_indel),
                                              src_off.ctypes.data, len(src_off) - 1, events.ctypes.data if len(events) else None, len(events),
                                              C.byref(n), C.byref(cx)))
    return events, int(n.value), int(cx.value)


def indel_sites_host(events, n_events, depth, src_off, capacity=None, min_count=3, frac_num=1, frac_den=2):
    """kbo_indel_sites_host over the first min(n_events, len(events)) events -> (records written (INDEL_SITE_DTYPE), count);
    capacity: None = every site"""
    events = np.ascontiguousarray(events, dtype=INDEL_EVENT_DTYPE)
    depth = np.ascontiguousarray(depth, dtype=np.uint32)
    src_off = np.ascontiguousarray(src_off, dtype=np.uint64)
    assert len(depth) == int(src_off[-1])
    cap = min(int(n_events), len(events)) if capacity is None else int(capacity)
    sites = np.zeros(cap, dtype=INDEL_SITE_DTYPE)
    n = C.c_uint64(0)
    check(lib().kbo_indel_sites_host(events.ctypes.data if len(events) else None, int(n_events), len(events), depth.ctypes.data if len(depth) else None,
                                     src_off.ctypes.data, len(src_off) - 1, int(min_count), int(frac_num), int(frac_den),
                                     sites.ctypes.data if cap else None, cap, C.byref(n)))
    return sites[:min(cap, n.value)].copy(), int(n.value)


def indel_code_bases(code, length):
    """the bases a `code` packs, in source order (bytes); length <= INDEL_CODE_LEN"""
    return bytes(b"ACGT"[(int(code) >> (2 * i)) & 3] for i in range(length))


def indel_variants(sites, sources):
    """the sites against the source text, the counterpart of pileup_snps: a list of (source, position within the source, ref, alt,
    count, depth) - a deletion has the deleted source bytes as ref and alt b"", an insertion ref b"" and its bases as alt, in front of
    the position (b"" for a LONG one: told apart by position and length only).  sources: the sequences the index was built from"""
    srcs = [_u8(s) for s in sources]
    off = np.concatenate([[0], np.cumsum([len(s) for s in srcs])]).astype(np.int64)
    text = np.concatenate(srcs + [np.zeros(0, dtype=np.uint8)])
    out = []
    for st in sites:
        pos, kl = int(st["pos"]), int(st["kind_len"])
        length, src = kl & INDEL_LEN_MASK, int(st["source"])
        if kl & INDEL_INS:
            ref, alt = b"", b"" if kl & INDEL_LONG else indel_code_bases(st["code"], length)
        else:
            ref, alt = text[pos:pos + length].tobytes(), b""
        out.append((src, pos - int(off[src]), ref, alt, int(st["count"]), int(st["depth"])))
    return out
