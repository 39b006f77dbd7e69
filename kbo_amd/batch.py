"""Batched and device-resident entry points (new surface; the reference API takes one
sequence per call, lib.rs:612-617, and leaves batching to kbo-cli)."""
import ctypes as C

import numpy as np

from . import _capi, derandomize
from ._capi import check, lib


def _prep(concat, offsets):
    concat = np.ascontiguousarray(concat, dtype=np.uint8)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    return concat, offsets, len(offsets) - 1


def ms_batch(sbwt, concat, offsets, want_intervals=False):
    """kbo_ms_batch -> (d uint8, lo uint32 | None, hi uint32 | None)"""
    concat, offsets, n = _prep(concat, offsets)
    total = int(offsets[-1]) if n > 0 else 0
    d = np.zeros(max(total, 1), dtype=np.uint8)
    lo = np.zeros(max(total, 1), dtype=np.uint32) if want_intervals else None
    hi = np.zeros(max(total, 1), dtype=np.uint32) if want_intervals else None
    check(lib().kbo_ms_batch(sbwt._h, concat.ctypes.data, offsets.ctypes.data, n, d.ctypes.data,
                             lo.ctypes.data if want_intervals else None,
                             hi.ctypes.data if want_intervals else None))
    return d[:total], (lo[:total] if want_intervals else None), (hi[:total] if want_intervals else None)


def matches_batch(sbwt, concat, offsets, max_error_prob=1e-7):
    """kbo::matches over every sequence of the batch -> uint8 chars"""
    concat, offsets, n = _prep(concat, offsets)
    total = int(offsets[-1]) if n > 0 else 0
    out = np.zeros(max(total, 1), dtype=np.uint8)
    check(lib().kbo_matches_batch(sbwt._h, concat.ctypes.data, offsets.ctypes.data, n, max_error_prob,
                                  out.ctypes.data))
    return out[:total]


def map_batch(sbwt, concat, offsets, max_error_prob=1e-7, format=True):  # noqa: A002
    """kbo::map with fill_gaps=false, call_variants=false over the batch -> uint8"""
    concat, offsets, n = _prep(concat, offsets)
    total = int(offsets[-1]) if n > 0 else 0
    out = np.zeros(max(total, 1), dtype=np.uint8)
    check(lib().kbo_map_batch(sbwt._h, concat.ctypes.data, offsets.ctypes.data, n, max_error_prob,
                              int(format), out.ctypes.data))
    return out[:total]


def map_batch_opts(sbwt, concat, offsets, map_opts=None):
    """kbo::map with any MapOpts (None = MapOpts(), the reference's defaults) over the batch ->
    (uint8 chars, int32 status per sequence: 0 or the code kbo_map returns for that sequence alone)"""
    from . import MapOpts
    o = map_opts if map_opts is not None else MapOpts()
    co = _capi.MapOpts(o.max_error_prob, int(o.fill_gaps), int(o.call_variants), int(o.format),
                       o.sbwt_build_opts._to_c())
    concat, offsets, n = _prep(concat, offsets)
    total = int(offsets[-1]) if n > 0 else 0
    out = np.zeros(max(total, 1), dtype=np.uint8)
    status = np.zeros(max(n, 1), dtype=np.int32)
    check(lib().kbo_map_batch_opts(sbwt._h, concat.ctypes.data, offsets.ctypes.data, n, C.byref(co), out.ctypes.data,
                                   status.ctypes.data))
    return out[:total], status[:n]


def fill_gaps_batch(sbwt, concat, offsets, threshold, max_err_prob):
    """gap_filling::fill_gaps over the batch, as kbo_fill_gaps per sequence -> (uint8 chars, int32 status)"""
    concat, offsets, n = _prep(concat, offsets)
    total = int(offsets[-1]) if n > 0 else 0
    out = np.zeros(max(total, 1), dtype=np.uint8)
    status = np.zeros(max(n, 1), dtype=np.int32)
    check(lib().kbo_fill_gaps_batch(sbwt._h, concat.ctypes.data, offsets.ctypes.data, n, threshold, max_err_prob,
                                    out.ctypes.data, status.ctypes.data))
    return out[:total], status[:n]


def fill_gaps_stats():
    """kbo_fill_gaps_stats: (gaps found, finished on the device, sequences redone on the host, device extension steps)
    of the calling thread's last fill_gaps_batch / map_batch_opts"""
    v = (C.c_uint64 * 4)()
    check(lib().kbo_fill_gaps_stats(v))
    return tuple(int(x) for x in v)


def find_batch(sbwt, concat, offsets, find_opts=None):
    """kbo::find over the batch -> (list of RLE tuples, rle_offsets uint64[n+1])"""
    from . import FindOpts
    o = find_opts if find_opts is not None else FindOpts()
    co = _capi.FindOpts(o.max_error_prob, o.max_gap_len)
    concat, offsets, n = _prep(concat, offsets)
    ro = np.zeros(n + 1, dtype=np.uint64)
    p = C.POINTER(_capi.RLE)()
    check(lib().kbo_find_batch(sbwt._h, concat.ctypes.data, offsets.ctypes.data, n, C.byref(co),
                               C.byref(p), ro.ctypes.data))
    total = int(ro[-1])
    if total > 100_000:  # big batches: hand back the records as an [n_runs, 7] uint64 array
        rles = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint64)), shape=(total, 7)).copy()
    else:
        rles = [p[i].as_tuple() for i in range(total)]
    lib().kbo_free(p)
    return rles, ro


def call_batch(sbwt, concat, offsets, call_opts=None):
    """kbo::call with every sequence of the batch as ref_seq -> list (per sequence) of lists of Variant"""
    from . import CallOpts, variant_calling
    o = call_opts if call_opts is not None else CallOpts()
    co = _capi.CallOpts(o.max_error_prob, o.sbwt_build_opts._to_c())
    concat, offsets, n = _prep(concat, offsets)
    vo = np.zeros(n + 1, dtype=np.uint64)
    p = C.POINTER(_capi.Variant)()
    check(lib().kbo_call_batch(sbwt._h, concat.ctypes.data, offsets.ctypes.data, n, C.byref(co), C.byref(p), vo.ctypes.data))
    allv = variant_calling._from_c(p, int(vo[-1]))  # (frees the allocation)
    return [allv[int(vo[s]):int(vo[s + 1])] for s in range(n)]


def pack_reads(concat, offsets):
    """bytes -> (u32 words, exception positions u64, exception bytes u8): the layout of kbo_hip.h's packed entry points"""
    concat, offsets, n = _prep(concat, offsets)
    words = np.zeros(int(lib().kbo_packed_words(offsets.ctypes.data, n)), dtype=np.uint32)
    cap = 1024
    while True:
        pos, byt, ne = np.zeros(cap, dtype=np.uint64), np.zeros(cap, dtype=np.uint8), C.c_size_t(0)
        rc = lib().kbo_pack_reads(concat.ctypes.data, offsets.ctypes.data, n, words.ctypes.data, pos.ctypes.data, byt.ctypes.data,
                                  cap, C.byref(ne))
        if rc == -5 and ne.value > cap:  # KBO_E_NOMEM: more non-ACGT bases than the list held
            cap = ne.value
            continue
        check(rc)
        return words, pos[:ne.value].copy(), byt[:ne.value].copy()


def unpack_matches(words, offsets):
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    out = np.zeros(int(offsets[-1]), dtype=np.uint8)
    check(lib().kbo_unpack_matches(words.ctypes.data, offsets.ctypes.data, len(offsets) - 1, out.ctypes.data))
    return out


def matches_batch_packed(sbwt, words, offsets, exc_pos, exc_byte, max_error_prob=1e-7):
    """kbo::matches over 2-bit packed reads -> 2-bit packed characters (M, -, X, R = 0 .. 3), same word layout"""
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    out = np.zeros(len(words), dtype=np.uint32)
    check(lib().kbo_matches_batch_packed(sbwt._h, words.ctypes.data, offsets.ctypes.data, len(offsets) - 1,
                                         exc_pos.ctypes.data if len(exc_pos) else None, exc_byte.ctypes.data if len(exc_byte) else None,
                                         len(exc_pos), max_error_prob, out.ctypes.data))
    return out


# kbo_hip.h kbo_aln_run as the C ABI lays it out, and as the Python side hands it out: length and code apart
_ALN_RUN = np.dtype([("seq", "<u4"), ("start", "<u4"), ("len_code", "<u4")])
SPARSE_DTYPE = np.dtype([("seq", "<u4"), ("start", "<u4"), ("len", "<u4"), ("code", "u1")])


def _sparse_from_raw(raw):
    out = np.empty(len(raw), dtype=SPARSE_DTYPE)
    out["seq"], out["start"] = raw["seq"], raw["start"]
    out["len"], out["code"] = raw["len_code"] >> 2, raw["len_code"] & 3
    return out


def _sparse_to_raw(runs):
    raw = np.empty(len(runs), dtype=_ALN_RUN)
    raw["seq"], raw["start"] = runs["seq"], runs["start"]
    raw["len_code"] = (runs["len"].astype(np.uint32) << np.uint32(2)) | runs["code"].astype(np.uint32)
    return raw


def matches_batch_sparse(sbwt, words, offsets, exc_pos, exc_byte, max_error_prob=1e-7):
    """kbo::matches over 2-bit packed reads, only the runs of characters other than 'M' -> structured array (SPARSE_DTYPE: seq,
    start, len, code with 1 = '-', 2 = 'X', 3 = 'R'), ordered by (seq, start)"""
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    p, n = C.c_void_p(), C.c_uint64(0)
    check(lib().kbo_matches_batch_sparse(sbwt._h, words.ctypes.data, offsets.ctypes.data, len(offsets) - 1,
                                         exc_pos.ctypes.data if len(exc_pos) else None, exc_byte.ctypes.data if len(exc_byte) else None,
                                         len(exc_pos), max_error_prob, C.byref(p), C.byref(n)))
    total = int(n.value)
    raw = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint32)), shape=(max(1, total) * 3,))[:total * 3].copy().view(_ALN_RUN)
    lib().kbo_free(p)
    return _sparse_from_raw(raw)


def expand_sparse(runs, offsets, ref=None):
    """sparse records -> one byte per base: kbo::matches' characters, or with the reads (ref) format::relative_to_ref of them"""
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    raw = _sparse_to_raw(runs)
    out = np.zeros(int(offsets[-1]), dtype=np.uint8)
    ref = np.ascontiguousarray(ref, dtype=np.uint8) if ref is not None else None
    check(lib().kbo_sparse_expand(raw.ctypes.data if len(raw) else None, len(raw), offsets.ctypes.data, len(offsets) - 1,
                                  ref.ctypes.data if ref is not None else None, out.ctypes.data))
    return out


def summary_of_chars(chars, offsets):
    """The per-sequence alignment summaries (kbo_hip.h kbo_aln_summary) of kbo::matches' characters, in plain numpy: an (n, 4) uint32
    array of [n_match ('M'), n_mismatch ('X'), n_jump ('R'), n_runs (maximal stretches without '-')]; all zero for a sequence
    of fewer than 3 bases (no alignment: derandomize.rs:274-276), whatever its characters are.  What the device entry points
    are tested against."""
    chars = np.frombuffer(chars, dtype=np.uint8) if isinstance(chars, (bytes, bytearray)) else np.asarray(chars, dtype=np.uint8)
    offsets = np.asarray(offsets, dtype=np.uint64).astype(np.int64)
    n = len(offsets) - 1
    out = np.zeros((max(n, 0), 4), dtype=np.uint32)
    if n <= 0:
        return out
    lens = np.diff(offsets)
    total = int(offsets[-1])
    c = chars[:total]
    csum = np.zeros((4, total + 1), dtype=np.int64)
    for j, ch in enumerate(b"MXR"):
        np.cumsum(c == ch, out=csum[j, 1:])
    nd = c != ord("-")
    starts = nd.copy()                      # a run starts at a character that is not '-' ...
    starts[1:] &= ~nd[:-1]                  # ... behind one that is ...
    heads = offsets[:-1][lens > 0]
    starts[heads] = nd[heads]               # ... or at the head of its sequence
    np.cumsum(starts, out=csum[3, 1:])
    for j in range(4):
        out[:, j] = csum[j, offsets[1:]] - csum[j, offsets[:-1]]
    out[lens < 3] = 0
    return out


def summary_batch(sbwt, seqs, max_error_prob=1e-7, packed=False):
    """kbo_summary_batch / kbo_summary_batch_packed: kbo::matches over every sequence, counted on the device -> (n, 4) uint32
    [n_match, n_mismatch, n_jump, n_runs] (summary_of_chars of matches_batch's characters; 16 bytes per sequence come back).
    seqs: (concat, offsets), or a list of bytes-like sequences.  packed: the reads cross to the device as 2-bit words."""
    if isinstance(seqs, tuple) and len(seqs) == 2:
        concat, offsets = seqs
    else:
        seqs = [np.frombuffer(bytes(q), dtype=np.uint8) for q in seqs]
        concat = np.concatenate(seqs) if seqs else np.zeros(0, dtype=np.uint8)
        offsets = np.concatenate([[0], np.cumsum([len(q) for q in seqs])]).astype(np.uint64)
    concat, offsets, n = _prep(concat, offsets)
    out = np.zeros((max(n, 1), 4), dtype=np.uint32)
    if packed:
        words, epos, ebyt = pack_reads(concat, offsets)
        check(lib().kbo_summary_batch_packed(sbwt._h, words.ctypes.data, offsets.ctypes.data, n, epos.ctypes.data if len(epos) else None,
                                             ebyt.ctypes.data if len(ebyt) else None, len(epos), max_error_prob, out.ctypes.data))
    else:
        check(lib().kbo_summary_batch(sbwt._h, concat.ctypes.data, offsets.ctypes.data, n, max_error_prob, out.ctypes.data))
    return out[:n]


def find_batch_packed(sbwt, words, offsets, exc_pos, exc_byte, find_opts=None):
    from . import FindOpts
    o = find_opts if find_opts is not None else FindOpts()
    co = _capi.FindOpts(o.max_error_prob, o.max_gap_len)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    n = len(offsets) - 1
    ro = np.zeros(n + 1, dtype=np.uint64)
    p = C.c_void_p()
    check(lib().kbo_find_batch_packed(sbwt._h, words.ctypes.data, offsets.ctypes.data, n, exc_pos.ctypes.data if len(exc_pos) else None,
                                      exc_byte.ctypes.data if len(exc_byte) else None, len(exc_pos), C.byref(co), C.byref(p), ro.ctypes.data))
    total = int(ro[-1])
    rles = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint32)), shape=(max(1, total), 7))[:total].astype(np.uint64)  # (kbo_rle32)
    lib().kbo_free(p)
    return rles, ro


# ---- both strands (kbo_hip.h "both strands"): the batch is staged to the device once, the '-' strand is made there
STRAND_FWD, STRAND_REV, STRAND_BOTH = 1, 2, 3


def revcomp_batch(concat, offsets):
    """kbo_revcomp_batch (host, threaded): the reverse complement of every sequence, in place of the sequence -> uint8"""
    concat, offsets, n = _prep(concat, offsets)
    out = np.zeros(max(len(concat), 1), dtype=np.uint8)
    check(lib().kbo_revcomp_batch(concat.ctypes.data, offsets.ctypes.data, n, out.ctypes.data))
    return out[:len(concat)]


def last_batch_staged_bytes():
    """host -> device bytes the calling thread's last host batch staged (kbo_hip_tuning.h)"""
    return int(lib().kbo_last_batch_staged_bytes())


def matches_batch_strands(sbwt, concat, offsets, max_error_prob=1e-7, format=False, strands=STRAND_BOTH):  # noqa: A002
    """kbo::matches (format=False) / kbo::map without refinement (format=True) of every sequence and of its reverse complement
    -> (chars '+' | None, chars '-' | None); '-' is in the coordinates of the reverse-complemented sequence"""
    concat, offsets, n = _prep(concat, offsets)
    total = int(offsets[-1]) if n > 0 else 0
    fwd = np.zeros(max(total, 1), dtype=np.uint8) if strands & 1 else None
    rev = np.zeros(max(total, 1), dtype=np.uint8) if strands & 2 else None
    check(lib().kbo_matches_batch_strands(sbwt._h, concat.ctypes.data, offsets.ctypes.data, n, max_error_prob, int(format), strands,
                                          fwd.ctypes.data if fwd is not None else None, rev.ctypes.data if rev is not None else None))
    return (fwd[:total] if fwd is not None else None), (rev[:total] if rev is not None else None)


def find_batch_strands(sbwt, concat, offsets, find_opts=None, strands=STRAND_BOTH):
    """kbo::find per strand -> ([n_runs, 7] uint64 records, rle_offsets uint64[2 n + 1]): the runs of sequence s are
    [ro[2 s], ro[2 s + 1]) for '+' and [ro[2 s + 1], ro[2 s + 2]) for '-'"""
    from . import FindOpts
    o = find_opts if find_opts is not None else FindOpts()
    co = _capi.FindOpts(o.max_error_prob, o.max_gap_len)
    concat, offsets, n = _prep(concat, offsets)
    ro = np.zeros(2 * n + 1, dtype=np.uint64)
    p = C.POINTER(_capi.RLE)()
    check(lib().kbo_find_batch_strands(sbwt._h, concat.ctypes.data, offsets.ctypes.data, n, C.byref(co), strands, C.byref(p), ro.ctypes.data))
    total = int(ro[-1])
    rles = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint64)), shape=(max(1, total), 7))[:total].copy()
    lib().kbo_free(p)
    return rles, ro


def matches_batch_packed_strands(sbwt, words, offsets, exc_pos, exc_byte, max_error_prob=1e-7, strands=STRAND_BOTH):
    """matches_batch_packed per strand -> (words '+' | None, words '-' | None)"""
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    fwd = np.zeros(max(len(words), 1), dtype=np.uint32) if strands & 1 else None
    rev = np.zeros(max(len(words), 1), dtype=np.uint32) if strands & 2 else None
    check(lib().kbo_matches_batch_packed_strands(sbwt._h, words.ctypes.data, offsets.ctypes.data, len(offsets) - 1,
                                                 exc_pos.ctypes.data if len(exc_pos) else None, exc_byte.ctypes.data if len(exc_byte) else None,
                                                 len(exc_pos), max_error_prob, strands, fwd.ctypes.data if fwd is not None else None,
                                                 rev.ctypes.data if rev is not None else None))
    return (fwd[:len(words)] if fwd is not None else None), (rev[:len(words)] if rev is not None else None)


def find_batch_packed_strands(sbwt, words, offsets, exc_pos, exc_byte, find_opts=None, strands=STRAND_BOTH):
    """find_batch_packed per strand -> ([n_runs, 7] uint64 records, rle_offsets uint64[2 n + 1]) as find_batch_strands"""
    from . import FindOpts
    o = find_opts if find_opts is not None else FindOpts()
    co = _capi.FindOpts(o.max_error_prob, o.max_gap_len)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    n = len(offsets) - 1
    ro = np.zeros(2 * n + 1, dtype=np.uint64)
    p = C.c_void_p()
    check(lib().kbo_find_batch_packed_strands(sbwt._h, words.ctypes.data, offsets.ctypes.data, n, exc_pos.ctypes.data if len(exc_pos) else None,
                                              exc_byte.ctypes.data if len(exc_byte) else None, len(exc_pos), C.byref(co), strands, C.byref(p),
                                              ro.ctypes.data))
    total = int(ro[-1])
    rles = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint32)), shape=(max(1, total), 7))[:total].astype(np.uint64)  # (kbo_rle32)
    lib().kbo_free(p)
    return rles, ro


class _FlatOwner:
    """keeps a kbo_call_flat alive for the numpy views into it (freed with the last of them)"""

    def __init__(self, flat):
        self.flat = flat

    def __del__(self):
        try:
            lib().kbo_call_flat_free(C.byref(self.flat))
        except Exception:  # noqa: BLE001  (interpreter shutdown)
            pass


def call_batch_arrays(sbwt, concat, offsets, call_opts=None):
    """kbo::call over a batch without a Python object per variant (kbo_hip.h kbo_call_batch_flat) -> dict of numpy arrays:
    var_offsets (n_seqs + 1), query_pos, query_len, ref_len (one entry per variant) and chars (per variant its query characters,
    then its reference characters, back to back in variant order) - views of the library's one allocation, nothing copied.
    variants_of(result, s) turns one sequence's slice into (query_pos, query_chars, ref_chars) tuples."""
    from . import CallOpts
    o = call_opts if call_opts is not None else CallOpts()
    co = _capi.CallOpts(o.max_error_prob, o.sbwt_build_opts._to_c())
    concat, offsets, n = _prep(concat, offsets)
    vo = np.zeros(n + 1, dtype=np.uint64)
    flat = _capi.CallFlat()
    check(lib().kbo_call_batch_flat(sbwt._h, concat.ctypes.data, offsets.ctypes.data, n, C.byref(co), C.byref(flat), vo.ctypes.data))
    owner = _FlatOwner(flat)
    nv, nc = int(flat.n_variants), int(flat.n_chars)

    def view(ptr, count, dtype):
        if count == 0:
            return np.zeros(0, dtype=dtype)
        return np.ctypeslib.as_array(ptr, shape=(count,))

    return {"var_offsets": vo, "query_pos": view(flat.query_pos, nv, np.uint32), "query_len": view(flat.query_len, nv, np.uint16),
            "ref_len": view(flat.ref_len, nv, np.uint16), "chars": view(flat.chars, nc, np.uint8), "_owner": owner}


def variants_of(res, s):
    """the variants of sequence s of a call_batch_arrays result as (query_pos, query_chars bytes, ref_chars bytes) tuples"""
    a, b = int(res["var_offsets"][s]), int(res["var_offsets"][s + 1])
    start = (np.concatenate([[0], np.cumsum(res["query_len"].astype(np.int64) + res["ref_len"].astype(np.int64))])
             if "_starts" not in res else res["_starts"])
    res["_starts"] = start
    out = []
    for v in range(a, b):
        q0, ql, rl = int(start[v]), int(res["query_len"][v]), int(res["ref_len"][v])
        out.append((int(res["query_pos"][v]), res["chars"][q0:q0 + ql].tobytes(), res["chars"][q0 + ql:q0 + ql + rl].tobytes()))
    return out


class PackedDeviceBatch:
    """A batch of reads resident in HBM as 2-bit words (kbo_hip.h kbo_matches_packed_dev): run() = kbo::matches through the one
    kernel's packed-native form, the characters as 2-bit words in self.words_out (unpack_matches() for bytes)."""

    def __init__(self, sbwt, concat, offsets, device, max_error_prob=1e-7):
        import torch
        self.torch, self.sbwt, self.device = torch, sbwt, device
        concat, offsets, n = _prep(concat, offsets)
        self.offsets = offsets
        self.n_seqs, self.total = n, int(offsets[-1])
        lens = np.diff(offsets.astype(np.int64))
        self.max_len = int(lens.max()) if n else 0
        self.uniform_len = self.max_len if n and int(lens.min()) == self.max_len else 0
        self.max_error_prob = max_error_prob
        words, pos, byt = pack_reads(concat, offsets)
        self.n_exc = len(pos)
        with torch.cuda.device(device):
            sbwt.to_device(-1)
            self.words = torch.from_numpy(words.view(np.int32)).to(device)
            self.words_out = torch.zeros(len(words) + 4, dtype=torch.int32, device=device)
            self.off = torch.from_numpy(offsets.view(np.int64)).to(device)
            self.exc_pos = torch.from_numpy(pos.view(np.int64)).to(device) if self.n_exc else None
            self.exc_byte = torch.from_numpy(byt).to(device) if self.n_exc else None
            self.scratch = torch.zeros(int(lib().kbo_matches_packed_dev_scratch_bytes(n, self.total)) // 8 + 2, dtype=torch.int64, device=device)
            self.work_bytes = int(lib().kbo_index_work_bytes(sbwt._h, n, self.total, self.max_len))
            self.work = torch.zeros(self.work_bytes // 8 + 2, dtype=torch.int64, device=device)

    def run(self, stream=None, tail_stream=None):
        s = stream if stream is not None else self.torch.cuda.current_stream(self.device)
        t = tail_stream if tail_stream is not None else s
        check(lib().kbo_matches_packed_dev(self.sbwt._h, self.words.data_ptr(), self.off.data_ptr(), self.n_seqs, self.total, self.max_len,
                                           self.uniform_len, self.exc_pos.data_ptr() if self.n_exc else None,
                                           self.exc_byte.data_ptr() if self.n_exc else None, self.n_exc, self.max_error_prob,
                                           self.words_out.data_ptr(), self.scratch.data_ptr(), self.work.data_ptr(), self.work_bytes,
                                           s.cuda_stream, t.cuda_stream))

    def chars(self):
        """the characters as bytes, on the host"""
        return unpack_matches(self.words_out[:len(self.words)].cpu().numpy().view(np.uint32), self.offsets)

    def sparse_runs(self, stream=None, capacity=None):
        """the runs other than 'M' of the characters run() left in words_out (kbo_hip.h kbo_sparse_runs_dev), on the host as
        matches_batch_sparse returns them; synchronises the stream (a second pass when they are more than `capacity`)"""
        torch = self.torch
        s = stream if stream is not None else torch.cuda.current_stream(self.device)
        if getattr(self, "sparse_work", None) is None:
            wb = int(lib().kbo_sparse_runs_work_bytes(self.n_seqs, len(self.words)))
            self.sparse_work = torch.zeros(wb // 8 + 2, dtype=torch.int64, device=self.device)
            self.sparse_count = torch.zeros(4, dtype=torch.int32, device=self.device)
        cap = capacity if capacity is not None else 2 * self.n_seqs + 16
        while True:
            recs = torch.zeros(max(1, cap) * 3, dtype=torch.int32, device=self.device)
            check(lib().kbo_sparse_runs_dev(self.words_out.data_ptr(), self.off.data_ptr(), self.n_seqs, self.max_len,
                                            self.sparse_work.data_ptr(), recs.data_ptr(), cap, self.sparse_count.data_ptr(), s.cuda_stream))
            s.synchronize()
            total = int(self.sparse_count[0].item())
            if total <= cap:
                return _sparse_from_raw(recs[:total * 3].cpu().numpy().view(np.uint32).view(_ALN_RUN))
            cap = total


class DeviceBatch:
    """A batch of reads resident in HBM (torch owns the memory, the C ABI gets raw
    pointers and the torch stream).  run() = A1 walk kernel, then fused A5+A6 kernel."""

    def __init__(self, sbwt, concat, offsets, device, max_error_prob=1e-7, want_intervals=False,
                 format=False, want_ms=True):  # noqa: A002
        import torch
        self.torch = torch
        self.sbwt = sbwt
        self.device = device
        concat, offsets, n = _prep(concat, offsets)
        self.n_seqs = n
        self.total = int(offsets[-1])
        self.max_len = int(np.max(np.diff(offsets.astype(np.int64)))) if n else 0
        self.k = sbwt.k()
        self.threshold = derandomize.random_match_threshold(self.k, sbwt.n_kmers(), 4, max_error_prob)
        pad = (self.total + 15) // 16 * 16 + 64
        with torch.cuda.device(device):
            sbwt.to_device(-1)
            self.q = torch.zeros(pad, dtype=torch.uint8, device=device)
            self.q[:self.total] = torch.from_numpy(concat if concat.flags.writeable else concat.copy()).to(device)
            self.off = torch.from_numpy(offsets.view(np.int64)).to(device)
            self.ms = torch.zeros(pad, dtype=torch.uint8, device=device)
            self.chars = torch.zeros(pad, dtype=torch.uint8, device=device)
            self.work_bytes = int(lib().kbo_index_work_bytes(sbwt._h, n, self.total, self.max_len))
            self.work = torch.zeros(self.work_bytes // 8 + 2, dtype=torch.int64, device=device)
            self.lo = torch.zeros(self.total, dtype=torch.int32, device=device) if want_intervals else None
            self.hi = torch.zeros(self.total, dtype=torch.int32, device=device) if want_intervals else None
        self.format = format
        self.want_ms = want_ms
        self.max_error_prob = max_error_prob
        self.fused = None  # set by run(): True when the last run() took the one-kernel route (map_kernels.hip)

    def walk(self, stream=None):
        s = stream if stream is not None else self.torch.cuda.current_stream(self.device)
        check(lib().kbo_ms_batch_dev(self.sbwt._h, self.q.data_ptr(), self.off.data_ptr(), self.n_seqs,
                                     self.total, self.max_len, self.ms.data_ptr(),
                                     self.lo.data_ptr() if self.lo is not None else None,
                                     self.hi.data_ptr() if self.hi is not None else None,
                                     self.work.data_ptr(), self.work_bytes, s.cuda_stream))

    def plan_stats(self, stream=None):
        """Work counters of the last walk() when it took the plan-guided stage (kbo_hip_tuning.h kbo_plan_stats_dev)."""
        s = stream if stream is not None else self.torch.cuda.current_stream(self.device)
        out = np.zeros(21, dtype=np.uint64)
        check(lib().kbo_plan_stats_dev(self.n_seqs, self.total, self.max_len, self.k, self.work.data_ptr(), out.ctypes.data,
                                       s.cuda_stream))
        names = ("units_walked", "accepted", "failed", "levels", "entry_levels", "seed_lookups", "seed_extensions",
                 "mismatches", "units", "redo_entries", "gave_up", "guard", "tab_lookups", "tab_written", "tab_flagged",
                 "tab_unresolved", "tab_anchored", "items_noplan", "subst_bits", "subst_clean", "subst_groups")
        return {n: int(v) for n, v in zip(names, out)}

    def plan_flags(self, stream=None):
        """uint8[n_seqs]: which reads the last planned launch left to the plain walk (kbo_hip_tuning.h kbo_plan_flags_dev)"""
        s = stream if stream is not None else self.torch.cuda.current_stream(self.device)
        out = np.zeros(self.n_seqs, dtype=np.uint8)
        check(lib().kbo_plan_flags_dev(self.n_seqs, self.total, self.max_len, self.k, self.work.data_ptr(), out.ctypes.data, s.cuda_stream))
        return out

    def long_stats(self, stream=None):
        """What the last run() / run_find() did when it took the kernel for sequences of any length (kbo_hip_tuning.h kbo_long_stats_dev)."""
        s = stream if stream is not None else self.torch.cuda.current_stream(self.device)
        out = np.zeros(25, dtype=np.uint64)
        check(lib().kbo_long_stats_dev(self.n_seqs, self.total, self.max_len, self.k, self.work.data_ptr(), out.ctypes.data, s.cuda_stream))
        names = ("pieces", "flagged", "sub_items", "seed_lookups", "filter_lookups", "table_lookups", "second_lookups", "_",
                 "cyc_staging", "cyc_stretches", "cyc_planes", "cyc_proof", "cyc_output", "band_tried", "band_taken", "_",
                 "why_other", "why_list", "why_ext", "why_back", "why_on", "why_band_list", "why_band_ext", "why_band_back", "why_band_on")
        return {n: int(v) for n, v in zip(names, out) if n != "_"}

    def derand_translate(self, stream=None):
        s = stream if stream is not None else self.torch.cuda.current_stream(self.device)
        if self.max_len == 0 or self.max_len > 480:  # long reads / contigs: scratch for the piece-wise kernel
            if getattr(self, "dt_work", None) is None:
                self.dt_work_bytes = int(lib().kbo_derand_work_bytes(self.n_seqs, self.total))
                self.dt_work = self.torch.zeros(self.dt_work_bytes // 8 + 2, dtype=self.torch.int64, device=self.device)
            work, work_bytes = self.dt_work.data_ptr(), self.dt_work_bytes
        else:
            work, work_bytes = None, 0
        check(lib().kbo_derand_translate_dev(self.ms.data_ptr(), self.off.data_ptr(), self.n_seqs, self.total, self.k,
                                             self.threshold, self.q.data_ptr() if self.format else None,
                                             self.chars.data_ptr(), self.max_len, work, work_bytes, s.cuda_stream))

    def run_lengths(self, max_gap_len=0, stream=None, runs_per_seq=2):
        """format::run_lengths_gapped of the (unformatted) characters, on the device: fills self.rle_records
        ([capacity, 7] int32) and self.rle_work (first-run indices; last word = number of runs)."""
        torch = self.torch
        s = stream if stream is not None else torch.cuda.current_stream(self.device)
        if getattr(self, "rle_work", None) is None:
            wb = int(lib().kbo_run_lengths_work_bytes(self.n_seqs))
            self.rle_work = torch.zeros(wb // 4 + 1, dtype=torch.int32, device=self.device)
            self.rle_capacity = runs_per_seq * self.n_seqs + 16
            self.rle_records = torch.zeros((self.rle_capacity, 7), dtype=torch.int32, device=self.device)
        check(lib().kbo_run_lengths_dev(self.chars.data_ptr(), self.off.data_ptr(), self.n_seqs, self.max_len, max_gap_len,
                                        self.rle_work.data_ptr(), self.rle_records.data_ptr(), self.rle_capacity,
                                        s.cuda_stream))

    def run_find(self, max_gap_len=0, stream=None, tail_stream=None, runs_per_seq=2):
        """kbo::find over the batch (kbo_hip.h kbo_find_batch_dev): the characters (unformatted) and their run lengths, as
        run() + run_lengths() leave them; with max_gap_len = 0 the one kernel counts the runs itself"""
        torch = self.torch
        s = stream if stream is not None else torch.cuda.current_stream(self.device)
        t = tail_stream if tail_stream is not None else s
        if getattr(self, "rle_work", None) is None:
            wb = int(lib().kbo_run_lengths_work_bytes(self.n_seqs))
            self.rle_work = torch.zeros(wb // 4 + 1, dtype=torch.int32, device=self.device)
            self.rle_capacity = runs_per_seq * self.n_seqs + 16
            self.rle_records = torch.zeros((self.rle_capacity, 7), dtype=torch.int32, device=self.device)
        fused = C.c_int(0)
        check(lib().kbo_find_batch_dev(self.sbwt._h, self.q.data_ptr(), self.off.data_ptr(), self.n_seqs, self.total, self.max_len,
                                       self.max_error_prob, max_gap_len, self.ms.data_ptr(), self.chars.data_ptr(), self.work.data_ptr(),
                                       self.work_bytes, self.rle_work.data_ptr(), self.rle_records.data_ptr(), self.rle_capacity,
                                       s.cuda_stream, t.cuda_stream, C.byref(fused)))
        self.fused = bool(fused.value)

    def run_lengths_host(self):
        """-> (records [n_runs, 7] uint32, first-run index per sequence uint32 [n_seqs + 1]) on the host"""
        w = self.rle_work.cpu().numpy().view(np.uint32)
        n = self.n_seqs
        words = n + 1 + (n + 1 + 1023) // 1024
        total = int(w[words])
        first = w[n + 1 + np.arange(n + 1) // 1024] + w[:n + 1]
        return self.rle_records[:total].cpu().numpy().view(np.uint32), first

    def run(self, stream=None, tail_stream=None):
        """kbo::map (format) / kbo::matches over the batch: kbo_map_batch_dev - one kernel for reads over an index copy with a
        depth table (self.ms then holds every MS value only when want_ms), one wave per piece for longer sequences when the MS
        values are not asked for (long_kernels.hip), else the walk + the derandomize / translate kernels."""
        if self.lo is not None:
            self.walk(stream)
            self.derand_translate(stream)
            self.fused = False
            return
        s = stream if stream is not None else self.torch.cuda.current_stream(self.device)
        fused = C.c_int(0)
        if tail_stream is not None:  # the second pass on another stream (kbo_hip.h kbo_map_batch_dev_tail): complete when both have drained
            check(lib().kbo_map_batch_dev_tail(self.sbwt._h, self.q.data_ptr(), self.off.data_ptr(), self.n_seqs, self.total, self.max_len,
                                               self.max_error_prob, int(self.format), int(self.want_ms), self.ms.data_ptr(),
                                               self.chars.data_ptr(), self.work.data_ptr(), self.work_bytes, s.cuda_stream,
                                               tail_stream.cuda_stream, C.byref(fused)))
        else:
            check(lib().kbo_map_batch_dev(self.sbwt._h, self.q.data_ptr(), self.off.data_ptr(), self.n_seqs, self.total, self.max_len,
                                          self.max_error_prob, int(self.format), int(self.want_ms), self.ms.data_ptr(), self.chars.data_ptr(),
                                          self.work.data_ptr(), self.work_bytes, s.cuda_stream, C.byref(fused)))
        self.fused = bool(fused.value)


    def _summary_buffers(self):
        torch = self.torch
        if getattr(self, "summary", None) is None:
            with torch.cuda.device(self.device):
                self.summary = torch.zeros((self.n_seqs, 4), dtype=torch.int32, device=self.device)
                self.summary_work_bytes = int(lib().kbo_summary_work_bytes(self.sbwt._h, self.n_seqs, self.total, self.max_len))
                self.summary_work = torch.zeros(self.summary_work_bytes // 8 + 2, dtype=torch.int64, device=self.device)

    def run_summary(self, stream=None, tail_stream=None):
        """kbo_summary_batch_dev: self.summary ([n_seqs, 4] int32: n_match, n_mismatch, n_jump, n_runs) of kbo::matches' characters,
        which are never stored when the one kernel takes the batch (self.fused)"""
        self._summary_buffers()
        s = stream if stream is not None else self.torch.cuda.current_stream(self.device)
        t = tail_stream if tail_stream is not None else s
        fused = C.c_int(0)
        check(lib().kbo_summary_batch_dev(self.sbwt._h, self.q.data_ptr(), self.off.data_ptr(), self.n_seqs, self.total, self.max_len,
                                          self.max_error_prob, self.ms.data_ptr(), self.summary.data_ptr(), self.summary_work.data_ptr(),
                                          self.summary_work_bytes, s.cuda_stream, t.cuda_stream, C.byref(fused)))
        self.fused = bool(fused.value)

    def summary_of_device_chars(self, stream=None):
        """kbo_summary_dev over self.chars (as run() left them) -> self.summary"""
        self._summary_buffers()
        s = stream if stream is not None else self.torch.cuda.current_stream(self.device)
        check(lib().kbo_summary_dev(self.chars.data_ptr(), self.off.data_ptr(), self.n_seqs, self.max_len, self.summary.data_ptr(), s.cuda_stream))

    def summary_host(self):
        return self.summary.cpu().numpy().view(np.uint32)


def derand_translate_seq(ms, offsets, k, thresholds, ref=None, stream=None, min_threshold=None):
    """kbo_derand_translate_seq_dev over torch tensors on the device: derandomize_ms_vec + translate_ms_vec (+ relative_to_ref when
    `ref` is given) with thresholds[s] for sequence s, at any length.  ms, ref: uint8; offsets: int64 or uint64 (n_seqs + 1);
    thresholds: int32 (n_seqs).  min_threshold: a lower bound of the thresholds when the caller knows one (it sizes the scratch);
    otherwise their minimum, from a host copy.  Returns the characters as a uint8 tensor of offsets[-1] elements; the bytes of
    sequences of fewer than 3 bases are unspecified.  Enqueued on `stream` (default: the current one), not synchronised."""
    import torch
    device = ms.device
    n_seqs = int(offsets.numel()) - 1
    assert ms.dtype == torch.uint8 and thresholds.dtype == torch.int32 and int(thresholds.numel()) == n_seqs
    assert offsets.dtype in (torch.int64, getattr(torch, "uint64", torch.int64))
    if min_threshold is None:
        min_threshold = int(thresholds.min().item()) if n_seqs > 0 else 2
    total = int(offsets[-1].item()) if n_seqs > 0 else 0

    def padded(t):  # the 16 bytes of slack behind a per-base buffer
        t = t.contiguous()
        if int(t.numel()) >= total + 16:
            return t
        p = torch.zeros(total + 16, dtype=torch.uint8, device=device)
        p[:total].copy_(t[:total])
        return p
    s = stream if stream is not None else torch.cuda.current_stream(device)
    with torch.cuda.stream(s):
        ms_p = padded(ms)
        ref_p = padded(ref) if ref is not None else None
        off, thr = offsets.contiguous(), thresholds.contiguous()
        out = torch.zeros(total + 16, dtype=torch.uint8, device=device)
        wb = int(lib().kbo_derand_seq_work_bytes(n_seqs, total, k, min_threshold))
        work = torch.empty(wb // 8 + 2, dtype=torch.int64, device=device)
        check(lib().kbo_derand_translate_seq_dev(ms_p.data_ptr(), off.data_ptr(), n_seqs, total, k, thr.data_ptr(), min_threshold,
                                                 ref_p.data_ptr() if ref_p is not None else None, out.data_ptr(), work.data_ptr(), wb,
                                                 s.cuda_stream))
    return out[:total]  # (the scratch and the padded copies were allocated on `s`: the allocator reuses them in that stream's order)


def derand_summary_seq(ms, offsets, k, thresholds, stream=None, min_threshold=None):
    """kbo_derand_summary_seq_dev over torch tensors on the device: the counts, runs and extent (kbo_hip.h kbo_aln_extent) of
    translate_ms_vec(derandomize_ms_vec(ms_s, k, thresholds[s]), k, thresholds[s]) for every sequence s, at any length - no characters
    are written anywhere.  Arguments as for derand_translate_seq.  Returns an (n_seqs, 6) int32 tensor that holds the u32 values
    {n_match, n_mismatch, n_jump, n_runs, start, end}; sequences of fewer than 3 bases have zeros.  Enqueued on `stream` (default:
    the current one), not synchronised."""
    import torch
    device = ms.device
    n_seqs = int(offsets.numel()) - 1
    assert ms.dtype == torch.uint8 and thresholds.dtype == torch.int32 and int(thresholds.numel()) == n_seqs
    assert offsets.dtype in (torch.int64, getattr(torch, "uint64", torch.int64))
    if min_threshold is None:
        min_threshold = int(thresholds.min().item()) if n_seqs > 0 else 2
    total = int(offsets[-1].item()) if n_seqs > 0 else 0
    s = stream if stream is not None else torch.cuda.current_stream(device)
    with torch.cuda.stream(s):
        ms_p = ms.contiguous()
        if int(ms_p.numel()) < total + 16:  # the 16 bytes of slack behind a per-base buffer
            ms_p = torch.zeros(total + 16, dtype=torch.uint8, device=device)
            ms_p[:total].copy_(ms[:total])
        off, thr = offsets.contiguous(), thresholds.contiguous()
        out = torch.empty((n_seqs, 6), dtype=torch.int32, device=device)
        wb = int(lib().kbo_derand_summary_seq_work_bytes(n_seqs, total, k, min_threshold))
        work = torch.empty(wb // 8 + 2, dtype=torch.int64, device=device)
        check(lib().kbo_derand_summary_seq_dev(ms_p.data_ptr(), off.data_ptr(), n_seqs, total, k, thr.data_ptr(), min_threshold,
                                               out.data_ptr(), work.data_ptr(), wb, s.cuda_stream))
    return out


def run_lengths_seq(chars, offsets, max_gap_len=0, stream=None):
    """kbo_run_lengths_seq_dev over torch tensors on the device: format::run_lengths_gapped of every sequence of a batch, at any length.
    chars: uint8; offsets: int64 or uint64 (n_seqs + 1).  Returns (records, first): records an (n, 7) int32 tensor that holds the u32
    values {start, end, matches, mismatches, jumps, gap_bases, gap_opens} of the batch's n runs, ordered by (sequence, start), and first
    an int32 tensor of n_seqs + 1 elements, first[s] the index of sequence s's first run and first[n_seqs] = n.  The number of runs is
    known on the device only: the call waits for `stream` (default: the current one) once to size the records, and runs the stage
    again when the room it guessed - a run per 64 characters - was too little."""
    import torch
    device = chars.device
    n_seqs = int(offsets.numel()) - 1
    assert chars.dtype == torch.uint8 and offsets.dtype in (torch.int64, getattr(torch, "uint64", torch.int64))
    total = int(offsets[-1].item()) if n_seqs > 0 else 0
    s = stream if stream is not None else torch.cuda.current_stream(device)
    with torch.cuda.stream(s):
        ch = chars.contiguous()
        if int(ch.numel()) < total + 16:  # the 16 bytes of slack behind a per-base buffer
            p = torch.zeros(total + 16, dtype=torch.uint8, device=device)
            p[:total].copy_(ch[:total])
            ch = p
        off = offsets.contiguous()
        wb = int(lib().kbo_run_lengths_seq_work_bytes(n_seqs, total))
        work = torch.empty(wb // 8 + 2, dtype=torch.int64, device=device)
        first = torch.zeros(n_seqs + 1, dtype=torch.int32, device=device)
        capacity = max(1024, 2 * n_seqs + total // 64)
        while True:
            records = torch.empty((capacity, 7), dtype=torch.int32, device=device)
            check(lib().kbo_run_lengths_seq_dev(ch.data_ptr(), off.data_ptr(), n_seqs, total, max_gap_len, work.data_ptr(), wb,
                                                records.data_ptr(), capacity, first.data_ptr(), s.cuda_stream))
            n = int(first[-1].item()) & 0xFFFFFFFF
            if n <= capacity:
                return records[:n], first
            capacity = n


def stream_pair(device, tail_cus=-1):
    """(stream, tail_stream) as torch streams, made by the library (kbo_hip.h kbo_stream_pair_create): the tail stream - a batch's second
    pass - on compute units of its own.  The pair lives as long as the process (the torch wrappers do not own the streams)."""
    import torch
    with torch.cuda.device(device):
        ks, ts = C.c_void_p(), C.c_void_p()
        check(lib().kbo_stream_pair_create(tail_cus, C.byref(ks), C.byref(ts)))
        return torch.cuda.ExternalStream(ks.value, device=device), torch.cuda.ExternalStream(ts.value, device=device)


class MapStream:
    """Several device-resident batches in flight through the library's own pipelines (kbo_hip.h kbo_map_stream_*): pairs of (kernel
    stream, second-pass stream) that take the batches in turn, two slots of work memory each."""

    def __init__(self, sbwt, max_seqs, max_bases, max_seq_len, pipelines=2):
        self.sbwt = sbwt
        h = C.c_void_p()
        check(lib().kbo_map_stream_create(sbwt._h, pipelines, max_seqs, max_bases, max_seq_len, C.byref(h)))
        self._h = h

    def submit(self, dev, ready_stream=None):
        """kbo::map (dev.format) / kbo::matches of a DeviceBatch's sequences into dev.chars (and the matching statistics into dev.ms
        when the batch was made with want_ms) -> ticket"""
        t = C.c_uint64(0)
        fused = C.c_int(0)
        check(lib().kbo_map_stream_submit(self._h, dev.q.data_ptr(), dev.off.data_ptr(), dev.n_seqs, dev.total, dev.max_len, dev.max_error_prob,
                                          int(dev.format), dev.ms.data_ptr() if dev.want_ms else None, dev.chars.data_ptr(),
                                          ready_stream.cuda_stream if ready_stream is not None else None, C.byref(t), C.byref(fused)))
        dev.fused = bool(fused.value)
        return int(t.value)

    def submit_summary(self, dev, ready_stream=None):
        """kbo_map_stream_submit_summary: the alignment summaries of a DeviceBatch's sequences into dev.summary -> ticket"""
        dev._summary_buffers()
        t = C.c_uint64(0)
        fused = C.c_int(0)
        check(lib().kbo_map_stream_submit_summary(self._h, dev.q.data_ptr(), dev.off.data_ptr(), dev.n_seqs, dev.total, dev.max_len,
                                                  dev.max_error_prob, dev.summary.data_ptr(),
                                                  ready_stream.cuda_stream if ready_stream is not None else None, C.byref(t), C.byref(fused)))
        dev.fused = bool(fused.value)
        return int(t.value)

    def wait(self, ticket):
        check(lib().kbo_map_stream_wait(self._h, ticket))

    def wait_on(self, ticket, stream):
        check(lib().kbo_map_stream_wait_on(self._h, ticket, stream.cuda_stream))

    def sync(self):
        check(lib().kbo_map_stream_sync(self._h))

    def close(self):
        if getattr(self, "_h", None):
            lib().kbo_map_stream_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
