"""kbo::find against a set of references: one index per reference, one call (kbo_hip.h "find against a set of references")."""
import ctypes as C

import numpy as np

from . import _capi
from ._capi import check, lib
from .index import _u8

STRAND_FWD, STRAND_REV, STRAND_BOTH = 1, 2, 3

# kbo_ref_run (40 bytes): which (reference, sequence, strand) a run belongs to + the fields of format::RLE (format.rs:18-33)
REF_RUN = np.dtype([("ref", np.uint32), ("seq", np.uint32), ("strand", np.uint32), ("start", np.uint32), ("end", np.uint32),
                    ("matches", np.uint32), ("mismatches", np.uint32), ("jumps", np.uint32), ("gap_bases", np.uint32),
                    ("gap_opens", np.uint32)])

# kbo_ref_summary (36 bytes): the pair + kbo_aln_extent - the numbers of 'M', 'X' and 'R', the maximal stretches without '-', and
# where the first one starts and the last one ends
REF_SUMMARY = np.dtype([("ref", np.uint32), ("seq", np.uint32), ("strand", np.uint32), ("n_match", np.uint32), ("n_mismatch", np.uint32),
                        ("n_jump", np.uint32), ("n_runs", np.uint32), ("start", np.uint32), ("end", np.uint32)])


class RefSet:
    """kbo_refset_t: index r is what kbo::build (lib.rs:501-506) makes of reference r alone"""

    def __init__(self, handle):
        self._h = handle

    @classmethod
    def build(cls, seqs, build_opts=None):
        from . import BuildOpts
        o = build_opts if build_opts is not None else BuildOpts()
        raw = [bytes(_u8(s)) for s in seqs]
        arr = (C.c_char_p * max(1, len(raw)))(*raw)
        lens = (C.c_size_t * max(1, len(raw)))(*[len(s) for s in raw])
        co = o._to_c()
        h = C.c_void_p()
        check(lib().kbo_refset_build(arr, lens, len(raw), C.byref(co), C.byref(h)))
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

    def __del__(self):
        if getattr(self, "_h", None):
            lib().kbo_refset_free(self._h)
            self._h = None


def find_refset(query_seqs, refset, find_opts=None, strands=STRAND_BOTH):
    """kbo::find (lib.rs:808-821) of every query sequence, on the strands asked for, against every reference of the set ->
    structured array of REF_RUN records ordered by (ref, seq, strand, start); '-' runs in the coordinates of the
    reverse-complemented sequence"""
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


def last_routes():
    """(references walked by the LDS kernel, references through the single-index pipeline, pairs walked, slabs) of the calling
    thread's last find_refset or summary_refset"""
    out = (C.c_uint64 * 4)()
    check(lib().kbo_refset_last_routes(out))
    return tuple(int(v) for v in out)
