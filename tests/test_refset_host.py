"""kbo_refset_t on the host (kbo_hip.h "find against a set of references"): every index of a set against one oracle index per
reference, and the argument errors of kbo_find_refset, which come back before any device is touched."""
import ctypes as C

import numpy as np
import pytest

import kbo_amd
from kbo_amd import _capi, refset
from oracle import binding as ora

E_LEN_LE_2, E_BAD_ARG = -2, -4


def _refs(k, seed):
    rng = np.random.default_rng(seed)

    def rnd(n):
        return np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)].tobytes()
    with_n = bytearray(rnd(200))
    with_n[100] = ord("N")
    twin = rnd(300)
    return [rnd(k - 1), rnd(k), rnd(40), rnd(300), rnd(1500), bytes(with_n), twin, twin, b"NNNN" * 20]


@pytest.mark.parametrize("k,rc", [(31, False), (96, False), (31, True), (96, True)])
def test_refset_build_matches_one_oracle_index_per_reference(k, rc):
    refs = _refs(k, 100 + k)
    rs = refset.RefSet.build(refs, kbo_amd.BuildOpts(k=k, add_revcomp=rc, num_threads=3))
    assert len(rs) == len(refs) and rs.k() == k
    for r, ref in enumerate(refs):
        oi = ora.Index.build([ref], k=k, add_revcomp=rc)
        assert rs.n_kmers(r) == oi.n_kmers, r
        assert rs.status(r) == (0 if oi.n_kmers > 0 else E_BAD_ARG), r
    assert rs.status(0) == E_BAD_ARG and rs.status(1) == 0 and rs.status(len(refs) - 1) == E_BAD_ARG
    assert rs.n_kmers(len(refs)) == 0 and rs.status(len(refs)) == E_BAD_ARG  # out of range
    assert rs.n_kmers(6) == rs.n_kmers(7)  # the twins


def test_refset_build_whole_call_errors():
    L = kbo_amd.lib()
    h = C.c_void_p()
    seq = (C.c_char_p * 1)(b"ACGT" * 20)
    lens = (C.c_size_t * 1)(80)
    assert L.kbo_refset_build(None, lens, 1, None, C.byref(h)) == E_BAD_ARG
    assert L.kbo_refset_build(seq, None, 1, None, C.byref(h)) == E_BAD_ARG
    assert L.kbo_refset_build(seq, lens, 0, None, C.byref(h)) == E_BAD_ARG
    assert L.kbo_refset_build(seq, lens, 1, None, None) == E_BAD_ARG
    for k in (0, 256):
        o = kbo_amd.BuildOpts(k=k)._to_c()
        assert L.kbo_refset_build(seq, lens, 1, C.byref(o), C.byref(h)) == E_BAD_ARG and not h.value
    assert L.kbo_refset_size(None) == 0 and L.kbo_refset_k(None) == 0
    L.kbo_refset_free(None)


def test_find_refset_argument_errors_need_no_device():
    L = kbo_amd.lib()
    rs = refset.RefSet.build(_refs(31, 5), kbo_amd.BuildOpts(k=31))
    q = np.frombuffer(b"ACGTACGTACGTAC", dtype=np.uint8).copy()
    off = np.array([0, 10, 14], dtype=np.uint64)
    p, n = C.c_void_p(), C.c_uint64()

    def call(h=rs._h, concat=q.ctypes.data, offsets=off, n_seqs=2, strands=3, runs=C.byref(p), n_runs=C.byref(n)):
        return L.kbo_find_refset(h, concat, offsets.ctypes.data if offsets is not None else None, n_seqs, None, strands, runs, n_runs)
    assert call(h=None) == E_BAD_ARG
    assert call(concat=None) == E_BAD_ARG
    assert call(offsets=None) == E_BAD_ARG
    assert call(runs=None) == E_BAD_ARG
    assert call(n_runs=None) == E_BAD_ARG
    for strands in (0, 4, -1):
        assert call(strands=strands) == E_BAD_ARG
    assert call(offsets=np.array([0, 12, 14], dtype=np.uint64)) == E_LEN_LE_2  # a 2-base sequence refuses the batch
    assert call(offsets=np.array([0, 12, 8], dtype=np.uint64)) == E_BAD_ARG    # offsets that do not ascend
    assert call(offsets=np.array([1, 10, 14], dtype=np.uint64)) == E_BAD_ARG   # ... or do not start at 0
    bad = _capi.FindOpts(0.0, 0)
    assert L.kbo_find_refset(rs._h, q.ctypes.data, off.ctypes.data, 2, C.byref(bad), 3, C.byref(p), C.byref(n)) == E_BAD_ARG
    assert not p.value and n.value == 0


def test_tuning_constants_are_the_headers():
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "kbo_hip_tuning.h")).read()
    assert int(re.search(r"#define KBO_REFSET_CHUNK (\d+)", hdr).group(1)) == 256
    assert int(re.search(r"#define KBO_REFSET_MAX_ROWS (\d+)", hdr).group(1)) == 16384
    assert kbo_amd.lib().kbo_set_refset_record_capacity(1 << 16) == 0
