"""kbo::find against a set of references: one index per reference, one call (kbo_hip.h "find against a set of references")."""
import ctypes as C

import numpy as np

from . import _capi
from ._capi import check, lib
from .index import _u8

STRAND_FWD, STRAND_REV, STRAND_BOTH = 1, 2, 3
# kbo_refset_route: the reference has a status / the LDS kernel / the single-index pipeline / the packed form walked from memory
ROUTE_NONE, ROUTE_LDS, ROUTE_INDEX, ROUTE_WIDE = -1, 0, 1, 2
MAX_ROWS, WIDE_MAX_ROWS = 16384, 1 << 20  # KBO_REFSET_MAX_ROWS, KBO_REFSET_WIDE_MAX_ROWS
SEED_MAX, SEED_MIN = 24, 11  # KBO_REFSET_SEED_MAX, KBO_REFSET_SEED_MIN: bases of a seed's code, bases that address a bucket

# kbo_ref_run (40 bytes): which (reference, sequence, strand) a run belongs to + the fields of format::RLE (format.rs:18-33)
REF_RUN = np.dtype([("ref", np.uint32), ("seq", np.uint32), ("strand", np.uint32), ("start", np.uint32), ("end", np.uint32),
                    ("matches", np.uint32), ("mismatches", np.uint32), ("jumps", np.uint32), ("gap_bases", np.uint32),
                    ("gap_opens", np.uint32)])

# kbo_ref_summary (36 bytes): the pair + kbo_aln_extent - the numbers of 'M', 'X' and 'R', the maximal stretches without '-', and
# where the first one starts and the last one ends
REF_SUMMARY = np.dtype([("ref", np.uint32), ("seq", np.uint32), ("strand", np.uint32), ("n_match", np.uint32), ("n_mismatch", np.uint32),
                        ("n_jump", np.uint32), ("n_runs", np.uint32), ("start", np.uint32), ("end", np.uint32)])

# kbo_ref_best (48 bytes): one per query sequence - the first (ref, strand) pair by (larger n_match, smaller ref, '+' first) with its
# kbo_aln_extent, the pairs with a hit, and ref / n_match of the runner-up among the OTHER references; REF_NONE where there is none
REF_NONE = 0xFFFFFFFF
REF_BEST = np.dtype([("seq", np.uint32), ("ref", np.uint32), ("strand", np.uint32), ("n_match", np.uint32), ("n_mismatch", np.uint32),
                     ("n_jump", np.uint32), ("n_runs", np.uint32), ("start", np.uint32), ("end", np.uint32), ("n_hits", np.uint32),
                     ("second_ref", np.uint32), ("second_match", np.uint32)])

# kbo_ref_locus (24 bytes), one per REF_RUN record: the run's first and last anchor - a k-mer window of the run that is a k-mer of
# the reference - as (position in the sequence on the run's strand, position on the reference); LOCUS_NONE where there is none
LOCUS_NONE = POS_NONE = 0xFFFFFFFF
LOCUS_MULTI = 0x80000000  # bit 31 of a table entry: the k-mer has more than one occurrence; bit 30: the entry is a REV occurrence
LOCUS_FIRST_REV, LOCUS_LAST_REV, LOCUS_FIRST_MULTI, LOCUS_LAST_MULTI, LOCUS_UNUSABLE = 1, 2, 4, 8, 16  # flags
REF_LOCUS = np.dtype([("q_first", np.uint32), ("ref_first", np.uint32), ("q_last", np.uint32), ("ref_last", np.uint32),
                      ("flags", np.uint32), ("n_tested", np.uint32)])

# kbo_ref_cover (48 bytes), one per reference of the set: the bases of the reference that the anchors of the runs given cover, in how
# many pieces, between which bases (LOCUS_NONE without one) and how deep, from how many runs and anchors
COVER_NO_ENTRIES, COVER_OVERFLOW = 1, 2  # flags
REF_COVER = np.dtype([("ref_len", np.uint32), ("covered", np.uint32), ("n_segments", np.uint32), ("first", np.uint32), ("last", np.uint32),
                      ("max_depth", np.uint32), ("n_runs", np.uint32), ("flags", np.uint32), ("n_anchors", np.uint64), ("n_multi", np.uint64)])

# kbo_ref_variant (24 bytes): a variant of kbo::call between reference `ref` and sequence `seq` on `strand` - Variant::query_pos on
# that strand of the sequence, and where its characters lie in the call's `chars`: query_len of the sequence, then ref_len of the
# reference (an insertion in the sequence has ref_len 0, a deletion query_len 0)
REF_VARIANT = np.dtype([("ref", np.uint32), ("seq", np.uint32), ("strand", np.uint32), ("pos", np.uint32), ("chars", np.uint32),
                        ("query_len", np.uint16), ("ref_len", np.uint16)])


class RefSet:
    """kbo_refset_t: index r is what kbo::build (lib.rs:501-506) makes of reference r alone"""

    def __init__(self, handle):
        self._h = handle

    @classmethod
    def build(cls, seqs, build_opts=None, wide_rows=None, prefilter=False, positions=False):
        """wide_rows: None - kbo_refset_build: a reference of more than MAX_ROWS rows takes the single-index route; a number in
        MAX_ROWS .. WIDE_MAX_ROWS - kbo_refset_build_wide: references of up to that many rows keep their packed form in the set and
        take the wide route, in the same slabs as the small ones, and a set without a larger one can go to find_refset_dev.
        prefilter: kbo_refset_build_opts with a seed table - find_refset, summary_refset and best_refset then screen the (reference,
        sequence, strand) pairs on the device and walk only those that share a seed; the records are the same.
        positions: kbo_refset_build_opts with a position table - one entry per row of every packed reference, what locate_refset
        needs to say where on its reference a run lies"""
        from . import BuildOpts
        o = build_opts if build_opts is not None else BuildOpts()
        raw = [bytes(_u8(s)) for s in seqs]
        arr = (C.c_char_p * max(1, len(raw)))(*raw)
        lens = (C.c_size_t * max(1, len(raw)))(*[len(s) for s in raw])
        co = o._to_c()
        h = C.c_void_p()
        if prefilter or positions:
            ro = _capi.RefsetOpts(MAX_ROWS if wide_rows is None else int(wide_rows), 1 if prefilter else 0, 1 if positions else 0)
            check(lib().kbo_refset_build_opts(arr, lens, len(raw), C.byref(co), C.byref(ro), C.byref(h)))
        elif wide_rows is None:
            check(lib().kbo_refset_build(arr, lens, len(raw), C.byref(co), C.byref(h)))
        else:
            check(lib().kbo_refset_build_wide(arr, lens, len(raw), C.byref(co), int(wide_rows), C.byref(h)))
        return cls(h)

    def __len__(self):
        return lib().kbo_refset_size(self._h)

    def k(self):
        return lib().kbo_refset_k(self._h)

    def n_kmers(self, r):
        return lib().kbo_refset_n_kmers(self._h, r)

    def status(self, r):
        """0, or the KBO_E_* code of querying reference r alone (it then contributes no runs)"""
        return lib().kbo_refset_status(self._h, r)

    def to_device(self, device=-1):
        check(lib().kbo_refset_to_device(self._h, device))
        return self

    def lds_only(self):
        """True when every reference that can be queried takes the LDS route"""
        return bool(lib().kbo_refset_lds_only(self._h))

    def packed_only(self):
        """True when no reference takes the single-index route: what find_refset_dev / summary_refset_dev ask of a set"""
        return bool(lib().kbo_refset_packed_only(self._h))

    def route(self, r):
        """ROUTE_LDS, ROUTE_INDEX or ROUTE_WIDE; ROUTE_NONE for a reference with a status"""
        v = lib().kbo_refset_route(self._h, r)
        if v < ROUTE_NONE:
            check(v)
        return v

    @property
    def has_prefilter(self):
        """True for a set built with prefilter=True"""
        return bool(lib().kbo_refset_has_prefilter(self._h))

    def prefilter_bytes(self):
        """bytes of the seed table (bucket offsets + 12 an entry); 0 without a prefilter"""
        return int(lib().kbo_refset_prefilter_bytes(self._h))

    def candidates(self, query_seqs, max_error_prob=1e-7, strands=STRAND_BOTH, host=False):
        """kbo_refset_candidates: the screen alone - a boolean array [n_refs, n_seqs, 2], True where sequence s on strand '+' (0) or
        '-' (1) shares a seed of the length this max_error_prob needs with reference r: every pair with a record is among them.
        host=True: the restatement on the CPU (kbo_refset_candidates_host, a test hook)"""
        concat, offsets, n = _batch(query_seqs)
        n_bits = len(self) * n * 2
        words = np.zeros((n_bits + 31) // 32, dtype=np.uint32)
        cnt = C.c_uint64()
        f = lib().kbo_refset_candidates_host if host else lib().kbo_refset_candidates
        check(f(self._h, concat.ctypes.data, offsets.ctypes.data, n, float(max_error_prob), int(strands), words.ctypes.data, C.byref(cnt)))
        bits = np.unpackbits(words.view(np.uint8), bitorder="little")[:n_bits].astype(bool)
        assert int(bits.sum()) == cnt.value
        return bits.reshape(len(self), n, 2)

    def candidates_dev(self, concat, offsets, max_error_prob=1e-7, strands=STRAND_BOTH, stream=None):
        """kbo_refset_candidates_dev over torch tensors on the device: the screen alone for a batch that is already there (the
        conventions are find_refset_dev's).  Returns (bits, stats): bits an int32 tensor of ceil(n_refs x n_seqs x 2 / 32) words,
        bit (r * n_seqs + s) * 2 + strand - 1 as candidates() has it; stats an int64 tensor of the four words of
        kbo_refset_screen_stats (n_candidates, candidate_bases, n_walked = 0, walked_bases = 0).  Nothing is synchronised."""
        import torch
        q, off, n_seqs, total, s = _dev_batch(concat, offsets, stream)
        L = lib()
        with torch.cuda.device(q.device), torch.cuda.stream(s):
            wb = int(L.kbo_refset_candidates_dev_work_bytes(self._h, n_seqs, total, int(strands)))
            work = torch.empty(wb // 8 + 2, dtype=torch.int64, device=q.device)
            bits = torch.empty((len(self) * n_seqs * 2 + 31) // 32, dtype=torch.int32, device=q.device)
            stats = torch.empty(4, dtype=torch.int64, device=q.device)
            check(L.kbo_refset_candidates_dev(self._h, q.data_ptr(), off.data_ptr(), n_seqs, total, float(max_error_prob), int(strands),
                                              work.data_ptr(), wb, bits.data_ptr(), stats.data_ptr(), s.cuda_stream))
        return bits, stats

    def has_positions(self):
        """True for a set built with positions=True"""
        return bool(lib().kbo_refset_has_positions(self._h))

    def positions_bytes(self):
        """bytes of the position table (4 a row + 8 a reference); 0 without one"""
        return int(lib().kbo_refset_positions_bytes(self._h))

    def positions(self, r):
        """test hook: the table's entries of reference r, one uint32 per row of its index (none for a reference without a packed
        form): bits 0 .. 29 p, bit 30 REV, bit 31 LOCUS_MULTI; POS_NONE for a row that is no full k-mer"""
        n = C.c_size_t()
        check(lib().kbo_refset_positions(self._h, r, None, C.byref(n)))
        out = np.zeros(n.value, dtype=np.uint32)
        check(lib().kbo_refset_positions(self._h, r, out.ctypes.data, C.byref(n)))
        return out

    def ref_len(self, r):
        """the length of reference r as it was given"""
        return int(lib().kbo_refset_ref_len(self._h, r))

    def cover_bases(self):
        """words of the depth profile: the bases of every reference with entries; 0 without positions"""
        return int(lib().kbo_refset_cover_bases(self._h))

    def cover_offsets(self):
        """where each reference's bases lie in the depth profile: len(self) + 1 uint64 offsets, a reference without entries owns none"""
        out = np.zeros(len(self) + 1, dtype=np.uint64)
        check(lib().kbo_refset_cover_offsets(self._h, out.ctypes.data))
        return out

    def cover_work_bytes(self):
        """kbo_cover_refset_dev_work_bytes: the d_work of cover_refset_dev; 0 without positions"""
        return int(lib().kbo_cover_refset_dev_work_bytes(self._h))

    def form(self, r):
        """test hook: the packed form of an LDS or wide reference, as bytes in a uint8 array"""
        n = C.c_size_t()
        check(lib().kbo_refset_form(self._h, r, None, C.byref(n)))
        out = np.zeros(n.value, dtype=np.uint8)
        check(lib().kbo_refset_form(self._h, r, out.ctypes.data, C.byref(n)))
        return out

    def ms_host(self, r, seq):
        """test hook: the matching statistics of seq against reference r, by the wide kernel's step on the CPU"""
        q = np.ascontiguousarray(_u8(seq))
        out = np.zeros(len(q), dtype=np.uint8)
        check(lib().kbo_refset_ms_host(self._h, r, q.ctypes.data, len(q), out.ctypes.data))
        return out

    def spell_row(self, r, row):
        """test hook: the k characters of row `row` of reference r's index, read off the packed form on the CPU ('$' in front of a
        row that is no full k-mer)"""
        out = np.zeros(self.k(), dtype=np.uint8)
        check(lib().kbo_refset_spell_row(self._h, r, int(row), out.ctypes.data))
        return out.tobytes()

    def __del__(self):
        if getattr(self, "_h", None):
            lib().kbo_refset_free(self._h)
            self._h = None


def _batch(query_seqs):
    raw = [_u8(s) for s in query_seqs]
    concat = np.ascontiguousarray(np.concatenate(raw) if raw else np.zeros(0, dtype=np.uint8))
    offsets = np.zeros(len(raw) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(s) for s in raw], dtype=np.uint64)
    return concat, offsets, len(raw)


def find_refset(query_seqs, refset, find_opts=None, strands=STRAND_BOTH, locate=False):
    """kbo::find (lib.rs:808-821) of every query sequence, on the strands asked for, against every reference of the set ->
    structured array of REF_RUN records ordered by (ref, seq, strand, start); '-' runs in the coordinates of the
    reverse-complemented sequence.  locate=True (a set built with positions=True): (runs, loci), loci as locate_refset's"""
    if locate:
        runs = find_refset(query_seqs, refset, find_opts, strands)
        return runs, locate_refset(query_seqs, refset, runs)
    from . import FindOpts
    o = find_opts if find_opts is not None else FindOpts()
    co = _capi.FindOpts(o.max_error_prob, o.max_gap_len)
    raw = [_u8(s) for s in query_seqs]
    concat = np.ascontiguousarray(np.concatenate(raw) if raw else np.zeros(0, dtype=np.uint8))
    offsets = np.zeros(len(raw) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(s) for s in raw], dtype=np.uint64)
    p, n = C.c_void_p(), C.c_uint64()
    check(lib().kbo_find_refset(refset._h, concat.ctypes.data, offsets.ctypes.data, len(raw), C.byref(co), int(strands), C.byref(p), C.byref(n)))
    try:
        if n.value == 0:
            return np.zeros(0, dtype=REF_RUN)
        buf = (C.c_uint8 * (n.value * REF_RUN.itemsize)).from_address(p.value)
        return np.frombuffer(buf, dtype=REF_RUN).copy()
    finally:
        lib().kbo_free(p)


def locate_refset(query_seqs, refset, runs, host=False):
    """kbo_locate_refset: where the runs of find_refset (REF_RUN records of the same query_seqs and set; the set built with
    positions=True) lie on their references -> a structured array of REF_LOCUS records, one per run, same index.
    host=True: the restatement on the CPU (kbo_locate_refset_host), byte-identical"""
    concat, offsets, n = _batch(query_seqs)
    runs = np.ascontiguousarray(runs, dtype=REF_RUN)
    loci = np.zeros(len(runs), dtype=REF_LOCUS)
    f = lib().kbo_locate_refset_host if host else lib().kbo_locate_refset
    check(f(refset._h, concat.ctypes.data, offsets.ctypes.data, n, runs.ctypes.data, len(runs), loci.ctypes.data))
    return loci


def locate_refset_dev(concat, offsets, refset, d_runs, d_n_runs, capacity, stream=None):
    """kbo_locate_refset_dev over torch tensors on the device: d_runs / d_n_runs as find_refset_dev returns them (records, count), the
    batch by find_refset_dev's conventions -> a (capacity, 6) int32 tensor that holds the u32 words of REF_LOCUS, the first
    min(count, capacity) rows written.  One launch on `stream` (default: the current one).  kbo_locate_refset_dev itself synchronises
    nothing; this wrapper, like find_refset_dev, reads offsets[-1] back once for the batch's bases, which waits for the device."""
    import torch
    q, off, n_seqs, total, s = _dev_batch(concat, offsets, stream)
    capacity = int(capacity)
    with torch.cuda.device(q.device), torch.cuda.stream(s):
        loci = torch.empty((capacity, 6), dtype=torch.int32, device=q.device)
        check(lib().kbo_locate_refset_dev(refset._h, q.data_ptr(), off.data_ptr(), n_seqs, total, d_runs.data_ptr() if capacity else None,
                                          d_n_runs.data_ptr(), capacity, loci.data_ptr() if capacity else None, s.cuda_stream))
    return loci


def cover_refset(query_seqs, refset, runs, depth=False, host=False):
    """kbo_cover_refset: depth and breadth of every reference of the set (built with positions=True) over the runs of find_refset
    (REF_RUN records of the same query_seqs and set) -> a structured array of REF_COVER records, one per reference.  depth=True:
    (covers, profile, offsets) - the depth of every base of every reference with entries as uint32, reference r's at
    profile[offsets[r]:offsets[r + 1]].  host=True: the restatement on the CPU (kbo_cover_refset_host), byte-identical"""
    concat, offsets, n = _batch(query_seqs)
    runs = np.ascontiguousarray(runs, dtype=REF_RUN)
    covers = np.zeros(len(refset), dtype=REF_COVER)
    profile = np.zeros(refset.cover_bases(), dtype=np.uint32) if depth else None
    f = lib().kbo_cover_refset_host if host else lib().kbo_cover_refset
    check(f(refset._h, concat.ctypes.data, offsets.ctypes.data, n, runs.ctypes.data if len(runs) else None, len(runs), covers.ctypes.data,
            profile.ctypes.data if depth else None))
    return (covers, profile, refset.cover_offsets()) if depth else covers


def cover_refset_dev(concat, offsets, refset, d_runs, d_n_runs, capacity, depth=False, stream=None):
    """kbo_cover_refset_dev over torch tensors on the device: d_runs / d_n_runs as find_refset_dev returns them (records, count), the
    batch by find_refset_dev's conventions -> (covers, profile): covers an (n_refs, 12) int32 tensor that holds the u32 words of
    REF_COVER, profile an int32 tensor of RefSet.cover_bases() words with depth=True, else None.  Everything on `stream` (default: the
    current one).  kbo_cover_refset_dev itself synchronises nothing; this wrapper, like find_refset_dev, reads offsets[-1] back once
    for the batch's bases, which waits for the device."""
    import torch
    q, off, n_seqs, total, s = _dev_batch(concat, offsets, stream)
    capacity = int(capacity)
    with torch.cuda.device(q.device), torch.cuda.stream(s):
        wb = refset.cover_work_bytes()
        work = torch.empty(wb // 8 + 2, dtype=torch.int64, device=q.device)
        covers = torch.empty((len(refset), 12), dtype=torch.int32, device=q.device)
        profile = torch.empty(refset.cover_bases(), dtype=torch.int32, device=q.device) if depth else None
        check(lib().kbo_cover_refset_dev(refset._h, q.data_ptr(), off.data_ptr(), n_seqs, total, d_runs.data_ptr() if capacity else None,
                                         d_n_runs.data_ptr(), capacity, covers.data_ptr(), profile.data_ptr() if depth else None,
                                         work.data_ptr(), wb, s.cuda_stream))
    return covers, profile  # (the scratch was allocated on `s`: the allocator reuses it in that stream's order)


def locus_interval(runs, loci, k, ref_lens):
    """Where each run lies on its reference, from its two anchors: (ref_lo, ref_hi, orientation), three int64 arrays.  The run's
    first base is projected along the diagonal of the first anchor and its last base along that of the last anchor - forward for a
    FWD anchor (query i <-> reference ref + (i - q)), antiparallel for a REV one (query i <-> reference ref + k - 1 - (i - q)) - and
    [ref_lo, ref_hi) is the range between the two images, both ends clipped to 0 .. ref_len (a projection that falls wholly
    outside the reference - possible only with indels - gives an empty range, ref_lo == ref_hi).  orientation: 1 when both anchors are FWD (the
    run's strand of the sequence reads along the reference), 2 when both are REV; 3 when they differ - an inverted repeat
    or a MULTI k-mer whose first occurrence lies on the other strand: neither forward nor reverse can be claimed, so neither is.  An ESTIMATE that is exact when
    the run holds no insertion or deletion: substitutions keep a diagonal, indels shift it.  A run without an anchor gets -1 in all
    three.  ref_lens: the references' lengths, indexed by runs["ref"] (RefSet.ref_len)."""
    runs = np.asarray(runs)
    loci = np.asarray(loci)
    ref_lens = np.asarray(ref_lens, dtype=np.int64)
    k = int(k)
    start, end = runs["start"].astype(np.int64), runs["end"].astype(np.int64)
    qf, rf = loci["q_first"].astype(np.int64), loci["ref_first"].astype(np.int64)
    ql, rl = loci["q_last"].astype(np.int64), loci["ref_last"].astype(np.int64)
    flags = loci["flags"].astype(np.int64)
    none = loci["q_first"] == LOCUS_NONE
    first_rev, last_rev = (flags & LOCUS_FIRST_REV) != 0, (flags & LOCUS_LAST_REV) != 0
    a = np.where(first_rev, rf + k - 1 + (qf - start), rf - (qf - start))            # the image of the run's first base
    b = np.where(last_rev, rl + k - 1 - (end - 1 - ql), rl + (end - 1 - ql))          # ... and of its last base
    n = ref_lens[np.where(none, 0, runs["ref"].astype(np.int64))] if len(runs) else np.zeros(0, dtype=np.int64)
    lo = np.clip(np.minimum(a, b), 0, n)
    hi = np.clip(np.maximum(a, b) + 1, 0, n)
    orient = np.where(first_rev & last_rev, 2, np.where(first_rev | last_rev, 3, 1))
    return np.where(none, -1, lo), np.where(none, -1, hi), np.where(none, -1, orient)


def call_refset(query_seqs, refset, opts=None, strands=STRAND_BOTH, host=False):
    """kbo::call (lib.rs:547-573) of every query sequence, on the strands asked for, against every reference of the set that
    summary_refset has a record for with it: (variants, chars) - a structured array of REF_VARIANT records ordered by (ref, seq,
    strand, pos) and the uint8 array their `chars` offsets point into (variant_chars slices it).  query characters are the
    sequence's, ref characters the reference's; '-' positions are those of the reverse-complemented sequence.  opts: CallOpts whose
    sbwt_build_opts.k is the set's k (None: the defaults with that k); its add_revcomp is the sequence's own index's, as in
    call_batch.  The set is packed_only().  Useful calls need k of about twice the threshold or more.
    host=True: the restatement on the CPU (kbo_call_refset_host), byte-identical; host="indexed": that with the second pass as the
    device-resident forms run it (kbo_call_refset_host_indexed), byte-identical too"""
    from . import BuildOpts, CallOpts
    o = opts if opts is not None else CallOpts(sbwt_build_opts=BuildOpts(k=refset.k(), build_select=True))
    co = _capi.CallOpts(o.max_error_prob, o.sbwt_build_opts._to_c())
    concat, offsets, n = _batch(query_seqs)
    res = _capi.RefCalls()
    f = lib().kbo_call_refset_host_indexed if host == "indexed" else lib().kbo_call_refset_host if host else lib().kbo_call_refset
    check(f(refset._h, concat.ctypes.data, offsets.ctypes.data, n, C.byref(co), int(strands), C.byref(res)))
    try:
        if res.n_variants == 0:
            assert not res.variants and not res.chars
            return np.zeros(0, dtype=REF_VARIANT), np.zeros(0, dtype=np.uint8)
        buf = (C.c_uint8 * (res.n_variants * REF_VARIANT.itemsize)).from_address(res.variants)
        variants = np.frombuffer(buf, dtype=REF_VARIANT).copy()
        chars = np.zeros(res.n_chars, dtype=np.uint8)
        if res.n_chars:
            chars[:] = np.frombuffer((C.c_uint8 * res.n_chars).from_address(res.chars), dtype=np.uint8)
        return variants, chars
    finally:
        lib().kbo_ref_calls_free(C.byref(res))


def variant_chars(variant, chars):
    """(query_chars, ref_chars) of one REF_VARIANT record as bytes"""
    at, ql, rl = int(variant["chars"]), int(variant["query_len"]), int(variant["ref_len"])
    return chars[at:at + ql].tobytes(), chars[at + ql:at + ql + rl].tobytes()


def call_refset_dev(concat, offsets, refset, opts=None, strands=STRAND_BOTH, max_variants=1 << 16, max_chars=1 << 20, max_sites=1 << 16,
                    refs_per_slab=None, stream=None, screened=False, max_pairs=None, max_pair_bases=None):
    """kbo_call_refset_dev over torch tensors on the device: call_refset's records, nothing synchronised.  Returns (variants, chars,
    stats): an (max_variants, 6) int32 tensor that holds the u32 words of REF_VARIANT, a uint8 tensor of max_chars characters and an
    int64 tensor of 8 words (n_variants, n_chars, n_sites, max_slab_candidates, n_panics, 0, 0, 0), complete when `stream` reaches
    the end of the call.  Record x is there iff x < max_variants, its characters iff chars + query_len + ref_len <= max_chars; the
    call is complete iff max_slab_candidates <= max_sites and n_sites <= max_sites.  The batch, refs_per_slab and stream as in
    summary_refset_dev.  screened=True: kbo_call_refset_screened_dev, the caps as find_refset_dev's; returns (variants, chars,
    stats, screen_stats)."""
    import torch
    from . import BuildOpts, CallOpts
    o = opts if opts is not None else CallOpts(sbwt_build_opts=BuildOpts(k=refset.k(), build_select=True))
    co = _capi.CallOpts(o.max_error_prob, o.sbwt_build_opts._to_c())
    q, off, n_seqs, total, s = _dev_batch(concat, offsets, stream)
    L = lib()
    max_variants, max_chars, max_sites = int(max_variants), int(max_chars), int(max_sites)
    if screened and (max_pairs is None or max_pair_bases is None):
        st = refset.candidates_dev(q, off, o.max_error_prob, strands, s)[1].cpu()  # (the one synchronisation of a call without caps)
        max_pairs = max(1, int(st[0])) if max_pairs is None else max_pairs
        max_pair_bases = int(st[1]) if max_pair_bases is None else max_pair_bases
    with torch.cuda.device(q.device), torch.cuda.stream(s):
        variants = torch.empty((max_variants, 6), dtype=torch.int32, device=q.device)
        chars = torch.empty(max_chars, dtype=torch.uint8, device=q.device)
        stats = torch.empty(8, dtype=torch.int64, device=q.device)
        vp = variants.data_ptr() if max_variants else None
        cp = chars.data_ptr() if max_chars else None
        if screened:
            max_pairs, max_pair_bases = int(max_pairs), int(max_pair_bases)
            wb = int(L.kbo_call_refset_screened_dev_work_bytes(refset._h, n_seqs, total, int(strands), max_sites, max_pairs, max_pair_bases))
            work = torch.empty(wb // 8 + 2, dtype=torch.int64, device=q.device)
            screen_stats = torch.empty(4, dtype=torch.int64, device=q.device)
            check(L.kbo_call_refset_screened_dev(refset._h, q.data_ptr(), off.data_ptr(), n_seqs, total, C.byref(co), int(strands),
                                                 work.data_ptr(), wb, vp, max_variants, cp, max_chars, max_sites, stats.data_ptr(),
                                                 max_pairs, max_pair_bases, screen_stats.data_ptr(), s.cuda_stream))
            return variants, chars, stats, screen_stats
        ns = 2 if int(strands) == STRAND_BOTH else 1  # (None: slabs of about 256 MiB, as summary_refset_dev)
        rps = max(1, (1 << 28) // max(1, ns * total)) if refs_per_slab is None else int(refs_per_slab)
        wb = int(L.kbo_call_refset_dev_work_bytes(refset._h, n_seqs, total, int(strands), max_sites, rps))
        work = torch.empty(wb // 8 + 2, dtype=torch.int64, device=q.device)
        check(L.kbo_call_refset_dev(refset._h, q.data_ptr(), off.data_ptr(), n_seqs, total, C.byref(co), int(strands), work.data_ptr(), wb,
                                    vp, max_variants, cp, max_chars, max_sites, stats.data_ptr(), s.cuda_stream))
    return variants, chars, stats


def last_call():
    """(pairs handed to the scan, candidate positions, sites with a match, variants) of the calling thread's last call_refset"""
    out = (C.c_uint64 * 4)()
    check(lib().kbo_refset_last_call(out))
    return tuple(int(v) for v in out)


def summary_refset(query_seqs, refset, max_error_prob=1e-7, strands=STRAND_BOTH):
    """The summary of kbo::matches of every query sequence, on the strands asked for, against every reference of the set: one
    REF_SUMMARY record per (ref, seq, strand) pair with a hit, ordered by (ref, seq, strand); a pair without a hit has none.  The
    pairs, thresholds and coordinates are find_refset's, and n_runs is its number of records for the pair with max_gap_len = 0."""
    raw = [_u8(s) for s in query_seqs]
    concat = np.ascontiguousarray(np.concatenate(raw) if raw else np.zeros(0, dtype=np.uint8))
    offsets = np.zeros(len(raw) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(s) for s in raw], dtype=np.uint64)
    p, n = C.c_void_p(), C.c_uint64()
    check(lib().kbo_summary_refset(refset._h, concat.ctypes.data, offsets.ctypes.data, len(raw), float(max_error_prob), int(strands),
                                   C.byref(p), C.byref(n)))
    try:
        if n.value == 0:
            return np.zeros(0, dtype=REF_SUMMARY)
        buf = (C.c_uint8 * (n.value * REF_SUMMARY.itemsize)).from_address(p.value)
        return np.frombuffer(buf, dtype=REF_SUMMARY).copy()
    finally:
        lib().kbo_free(p)


def best_refset(query_seqs, refset, max_error_prob=1e-7, strands=STRAND_BOTH):
    """The best reference of every query sequence, reduced on the device: a structured array of len(query_seqs) REF_BEST records in
    sequence order.  The pairs are summary_refset's; a sequence's record names the pair with the most matches (ties: the smaller
    ref, then '+'), how many pairs had a hit, and the runner-up among the other references.  A sequence without a hit has ref ==
    second_ref == REF_NONE and strand == 0."""
    raw = [_u8(s) for s in query_seqs]
    concat = np.ascontiguousarray(np.concatenate(raw) if raw else np.zeros(0, dtype=np.uint8))
    offsets = np.zeros(len(raw) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(s) for s in raw], dtype=np.uint64)
    p = C.c_void_p()
    check(lib().kbo_best_refset(refset._h, concat.ctypes.data, offsets.ctypes.data, len(raw), float(max_error_prob), int(strands), C.byref(p)))
    try:
        buf = (C.c_uint8 * (len(raw) * REF_BEST.itemsize)).from_address(p.value)
        return np.frombuffer(buf, dtype=REF_BEST).copy()
    finally:
        lib().kbo_free(p)


def _dev_batch(concat, offsets, stream):
    """the batch as the device-resident calls take it: (concat with 16 bytes of slack, 16-byte aligned; offsets; n_seqs; total; stream)"""
    import torch
    device = concat.device
    n_seqs = int(offsets.numel()) - 1
    assert concat.dtype == torch.uint8 and offsets.dtype in (torch.int64, getattr(torch, "uint64", torch.int64))
    total = int(offsets[-1].item()) if n_seqs > 0 else 0
    s = stream if stream is not None else torch.cuda.current_stream(device)
    with torch.cuda.device(device), torch.cuda.stream(s):
        q = concat.contiguous()
        if int(q.numel()) < total + 16 or q.data_ptr() % 16:  # the 16 bytes of slack behind a per-base buffer
            p = torch.zeros(total + 16, dtype=torch.uint8, device=device)
            p[:total].copy_(q[:total])
            q = p
        off = offsets.contiguous()
    return q, off, n_seqs, total, s


def _screened_dev(kind, concat, offsets, refset, arg, strands, capacity, max_pairs, max_pair_bases, stream):
    """kbo_find / summary / best_refset_screened_dev; max_pairs / max_pair_bases None: one read-back of candidates_dev's figures"""
    import torch
    q, off, n_seqs, total, s = _dev_batch(concat, offsets, stream)
    L = lib()
    if max_pairs is None or max_pair_bases is None:
        p = arg.max_error_prob if kind == "find" else arg
        st = refset.candidates_dev(q, off, p, strands, s)[1].cpu()  # (the one synchronisation of a call without caps)
        max_pairs = max(1, int(st[0])) if max_pairs is None else max_pairs
        max_pair_bases = int(st[1]) if max_pair_bases is None else max_pair_bases
    max_pairs, max_pair_bases = int(max_pairs), int(max_pair_bases)
    with torch.cuda.device(q.device), torch.cuda.stream(s):
        stats = torch.empty(4, dtype=torch.int64, device=q.device)
        if kind == "best":
            wb = int(L.kbo_best_refset_screened_dev_work_bytes(refset._h, n_seqs, total, int(strands), max_pairs, max_pair_bases))
            work = torch.empty(wb // 8 + 2, dtype=torch.int64, device=q.device)
            table = torch.empty((n_seqs, 12), dtype=torch.int32, device=q.device)
            check(L.kbo_best_refset_screened_dev(refset._h, q.data_ptr(), off.data_ptr(), n_seqs, total, float(arg), int(strands),
                                                 work.data_ptr(), wb, table.data_ptr(), max_pairs, max_pair_bases, stats.data_ptr(),
                                                 s.cuda_stream))
            return table, stats
        find = kind == "find"
        work_bytes = L.kbo_find_refset_screened_dev_work_bytes if find else L.kbo_summary_refset_screened_dev_work_bytes
        wb = int(work_bytes(refset._h, n_seqs, total, int(strands), capacity, max_pairs, max_pair_bases))
        work = torch.empty(wb // 8 + 2, dtype=torch.int64, device=q.device)
        records = torch.empty((capacity, 10 if find else 9), dtype=torch.int32, device=q.device)
        count = torch.empty(1, dtype=torch.int64, device=q.device)
        out = records.data_ptr() if capacity else None
        if find:
            check(L.kbo_find_refset_screened_dev(refset._h, q.data_ptr(), off.data_ptr(), n_seqs, total, C.byref(arg), int(strands),
                                                 work.data_ptr(), wb, out, capacity, count.data_ptr(), max_pairs, max_pair_bases,
                                                 stats.data_ptr(), s.cuda_stream))
        else:
            check(L.kbo_summary_refset_screened_dev(refset._h, q.data_ptr(), off.data_ptr(), n_seqs, total, float(arg), int(strands),
                                                    work.data_ptr(), wb, out, capacity, count.data_ptr(), max_pairs, max_pair_bases,
                                                    stats.data_ptr(), s.cuda_stream))
    return records, count, stats


def best_refset_dev(concat, offsets, refset, max_error_prob=1e-7, strands=STRAND_BOTH, refs_per_slab=None, stream=None, screened=False,
                    max_pairs=None, max_pair_bases=None):
    """kbo_best_refset_dev over torch tensors on the device: best_refset's records as an (n_seqs, 12) int32 tensor that holds the u32
    words of REF_BEST, complete when `stream` reaches the end of the call.  The conventions are summary_refset_dev's: the batch, the
    set (on that device, packed_only()), refs_per_slab, the stream, and nothing synchronised.  Sequences of fewer than 3 bases get
    the record without a hit.
    screened=True: kbo_best_refset_screened_dev over a set with a prefilter - the table over the pairs of ONE slab of candidates (see
    find_refset_dev); returns (table, stats)."""
    import torch
    if screened:
        return _screened_dev("best", concat, offsets, refset, max_error_prob, strands, 0, max_pairs, max_pair_bases, stream)
    device = concat.device
    n_seqs = int(offsets.numel()) - 1
    assert concat.dtype == torch.uint8 and offsets.dtype in (torch.int64, getattr(torch, "uint64", torch.int64))
    total = int(offsets[-1].item()) if n_seqs > 0 else 0
    L = lib()
    ns = 2 if int(strands) == STRAND_BOTH else 1
    if refs_per_slab is None:  # slabs of about 256 MiB; 0: as many references as a slab may hold
        refs_per_slab = max(1, (1 << 28) // max(1, ns * total))
    s = stream if stream is not None else torch.cuda.current_stream(device)
    with torch.cuda.device(device), torch.cuda.stream(s):
        q = concat.contiguous()
        if int(q.numel()) < total + 16 or q.data_ptr() % 16:  # the 16 bytes of slack behind a per-base buffer
            p = torch.zeros(total + 16, dtype=torch.uint8, device=device)
            p[:total].copy_(q[:total])
            q = p
        off = offsets.contiguous()
        wb = int(L.kbo_best_refset_dev_work_bytes(refset._h, n_seqs, total, int(strands), refs_per_slab))
        work = torch.empty(wb // 8 + 2, dtype=torch.int64, device=device)
        table = torch.empty((n_seqs, 12), dtype=torch.int32, device=device)
        check(L.kbo_best_refset_dev(refset._h, q.data_ptr(), off.data_ptr(), n_seqs, total, float(max_error_prob), int(strands),
                                    work.data_ptr(), wb, table.data_ptr(), s.cuda_stream))
    return table  # (the scratch was allocated on `s`: the allocator reuses it in that stream's order)


def _refset_dev(find, concat, offsets, refset, arg, strands, capacity, refs_per_slab, stream):
    import torch
    device = concat.device
    n_seqs = int(offsets.numel()) - 1
    assert concat.dtype == torch.uint8 and offsets.dtype in (torch.int64, getattr(torch, "uint64", torch.int64))
    total = int(offsets[-1].item()) if n_seqs > 0 else 0
    L = lib()
    words = 10 if find else 9
    work_bytes = L.kbo_find_refset_dev_work_bytes if find else L.kbo_summary_refset_dev_work_bytes
    ns = 2 if int(strands) == STRAND_BOTH else 1
    if refs_per_slab is None:  # slabs of about 256 MiB; 0: as many references as a slab may hold
        refs_per_slab = max(1, (1 << 28) // max(1, ns * total))
    s = stream if stream is not None else torch.cuda.current_stream(device)
    with torch.cuda.device(device), torch.cuda.stream(s):
        q = concat.contiguous()
        if int(q.numel()) < total + 16 or q.data_ptr() % 16:  # the 16 bytes of slack behind a per-base buffer
            p = torch.zeros(total + 16, dtype=torch.uint8, device=device)
            p[:total].copy_(q[:total])
            q = p
        off = offsets.contiguous()
        wb = int(work_bytes(refset._h, n_seqs, total, int(strands), capacity, refs_per_slab))
        work = torch.empty(wb // 8 + 2, dtype=torch.int64, device=device)
        records = torch.empty((capacity, words), dtype=torch.int32, device=device)
        count = torch.empty(1, dtype=torch.int64, device=device)
        out = records.data_ptr() if capacity else None
        if find:
            check(L.kbo_find_refset_dev(refset._h, q.data_ptr(), off.data_ptr(), n_seqs, total, C.byref(arg), int(strands), work.data_ptr(), wb,
                                        out, capacity, count.data_ptr(), s.cuda_stream))
        else:
            check(L.kbo_summary_refset_dev(refset._h, q.data_ptr(), off.data_ptr(), n_seqs, total, float(arg), int(strands), work.data_ptr(), wb,
                                           out, capacity, count.data_ptr(), s.cuda_stream))
    return records, count  # (the scratch was allocated on `s`: the allocator reuses it in that stream's order)


def find_refset_dev(concat, offsets, refset, find_opts=None, strands=STRAND_BOTH, capacity=1 << 16, refs_per_slab=None, stream=None,
                    screened=False, max_pairs=None, max_pair_bases=None):
    """kbo_find_refset_dev over torch tensors on the device: find_refset's records for a batch that is already there.  concat: uint8
    (the sequences back to back); offsets: int64 or uint64 (n_seqs + 1); the set has a copy on that device (RefSet.to_device) and is
    packed_only(): LDS and wide references (RefSet.build(wide_rows=...)), none of the single-index route.  Returns (records, count): records a (capacity, 10) int32 tensor that holds the u32 words of REF_RUN, the first
    min(count, capacity) rows written, and count an int64 tensor of one element, the number of records there are - beyond `capacity`
    they are counted only.  Sequences of fewer than 3 bases contribute nothing.  refs_per_slab: references of a slab (None: about
    256 MiB a slab, 0: as many as a slab may hold); it sizes the scratch.  Enqueued on `stream` (default: the current one); nothing is
    synchronised.
    screened=True: kbo_find_refset_screened_dev over a set built with prefilter=True - the screen runs on the device and ONE slab is
    walked, the longest prefix of the candidate pairs (in the records' order) with at most max_pairs pairs and max_pair_bases bases;
    refs_per_slab is not used.  Returns (records, count, stats): stats an int64 tensor (n_candidates, candidate_bases, n_walked,
    walked_bases), and n_walked == n_candidates says the records are complete.  A cap left None is taken from one read-back of
    RefSet.candidates_dev's figures (the only synchronisation; with both caps given there is none)."""
    from . import FindOpts
    o = find_opts if find_opts is not None else FindOpts()
    if screened:
        return _screened_dev("find", concat, offsets, refset, _capi.FindOpts(o.max_error_prob, o.max_gap_len), strands, int(capacity), max_pairs,
                             max_pair_bases, stream)
    return _refset_dev(True, concat, offsets, refset, _capi.FindOpts(o.max_error_prob, o.max_gap_len), strands, int(capacity), refs_per_slab, stream)


def summary_refset_dev(concat, offsets, refset, max_error_prob=1e-7, strands=STRAND_BOTH, capacity=1 << 16, refs_per_slab=None, stream=None,
                       screened=False, max_pairs=None, max_pair_bases=None):
    """kbo_summary_refset_dev over torch tensors on the device: summary_refset's records, as find_refset_dev returns find_refset's -
    (records, count) with records a (capacity, 9) int32 tensor that holds the u32 words of REF_SUMMARY.  The set is packed_only(), as
    there.  screened=True: kbo_summary_refset_screened_dev, as find_refset_dev's; returns (records, count, stats)."""
    if screened:
        return _screened_dev("summary", concat, offsets, refset, max_error_prob, strands, int(capacity), max_pairs, max_pair_bases, stream)
    return _refset_dev(False, concat, offsets, refset, max_error_prob, strands, int(capacity), refs_per_slab, stream)


def last_wide():
    """(references walked by the wide kernel, tasks it was launched with) of the calling thread's last find_refset or summary_refset"""
    out = (C.c_uint64 * 2)()
    check(lib().kbo_refset_last_wide(out))
    return tuple(int(v) for v in out)


def last_best():
    """(launches with a wave per sequence, launches with a workgroup per sequence) of refset_best_kernel in the calling thread's last
    best_refset or best_refset_dev"""
    out = (C.c_uint64 * 2)()
    check(lib().kbo_refset_last_best(out))
    return tuple(int(v) for v in out)


def last_prefilter():
    """(pairs of packed references, pairs with their bit set, pairs walked, 1 if the screen ran) of the calling thread's last
    find_refset, summary_refset or best_refset"""
    out = (C.c_uint64 * 4)()
    check(lib().kbo_refset_last_prefilter(out))
    return tuple(int(v) for v in out)


def set_prefilter_max_bits(bits):
    """test hook: the bitmap size (n_refs x n_seqs x 2 bits) above which a call on a set with a prefilter runs unscreened; 0: 2^31"""
    check(lib().kbo_set_refset_prefilter_max_bits(int(bits)))


def last_routes():
    """(references walked by the LDS kernel, references through the single-index pipeline, pairs walked, slabs) of the calling
    thread's last find_refset, summary_refset or best_refset"""
    out = (C.c_uint64 * 4)()
    check(lib().kbo_refset_last_routes(out))
    return tuple(int(v) for v in out)
