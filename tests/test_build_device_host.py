"""kbo_index_build_device (include/kbo_hip.h): the argument checks and the refusal of sharded builds run before any HIP call,
so they hold on a machine without a GPU - with the codes kbo_index_build gives, and *out NULL on every error.  CPU only."""
import ctypes as C

import pytest

import kbo_amd
from kbo_amd import _capi

BAD_ARG, UNSUPPORTED = -4, -8
SEQS = [b"ACGTACGTTTGACCA" * 20, b"GGGTTTAACCNNACGTA" * 5]


def _args(seqs):
    arr = (C.c_char_p * len(seqs))(*seqs)
    lens = (C.c_size_t * len(seqs))(*[len(s) for s in seqs])
    return arr, lens


def _sentinel():
    return C.c_void_p(0x1234)  # *out must come back NULL


def _both(seqs_arg, lens_arg, n, opts, out_null=False):
    """(rc of kbo_index_build, rc of kbo_index_build_device) for the same arguments; out is checked to come back NULL"""
    L = kbo_amd.lib()
    rcs = []
    for dev in (None, 0):
        h = _sentinel()
        out = None if out_null else C.byref(h)
        if dev is None:
            rc = L.kbo_index_build(seqs_arg, lens_arg, n, opts, out)
        else:
            rc = L.kbo_index_build_device(seqs_arg, lens_arg, n, opts, dev, out)
        if not out_null:
            assert h.value is None, "out is not NULL after an error"
        rcs.append(rc)
    return rcs


def test_argument_errors_match_the_host_builder():
    arr, lens = _args(SEQS)
    o = kbo_amd.BuildOpts(k=31)._to_c()
    assert _both(arr, lens, len(SEQS), C.byref(o), out_null=True) == [BAD_ARG, BAD_ARG]          # null out
    assert _both(None, lens, len(SEQS), C.byref(o)) == [BAD_ARG, BAD_ARG]                        # null seqs
    assert _both(arr, None, len(SEQS), C.byref(o)) == [BAD_ARG, BAD_ARG]                         # null lens
    assert _both(arr, lens, 0, C.byref(o)) == [BAD_ARG, BAD_ARG]                                 # no sequence
    for k in (0, 256, 1000):
        ok = kbo_amd.BuildOpts(k=k)._to_c()
        assert _both(arr, lens, len(SEQS), C.byref(ok)) == [BAD_ARG, BAD_ARG], k
        assert b"k must be in 1..255" in kbo_amd.lib().kbo_last_error()


def test_sharded_builds_are_refused_before_any_hip_call():
    L = kbo_amd.lib()
    arr, lens = _args(SEQS)
    o = kbo_amd.BuildOpts(k=31)._to_c()
    try:
        L.kbo_set_index_shards(2)
        h = _sentinel()
        assert L.kbo_index_build_device(arr, lens, len(SEQS), C.byref(o), 0, C.byref(h)) == UNSUPPORTED
        assert h.value is None
        assert b"kbo_index_build" in L.kbo_last_error()
        # the host builder builds the same input as two shards
        h2 = C.c_void_p()
        assert L.kbo_index_build(arr, lens, len(SEQS), C.byref(o), C.byref(h2)) == 0
        assert L.kbo_index_shards(h2) == 2
        L.kbo_index_free(h2)
    finally:
        L.kbo_set_index_shards(0)


def test_python_device_argument_reaches_the_device_builder():
    L = kbo_amd.lib()
    try:
        L.kbo_set_index_shards(2)
        with pytest.raises(_capi.KboError) as e:
            kbo_amd.build(SEQS, kbo_amd.BuildOpts(k=31), device=0)
        assert e.value.code == UNSUPPORTED and "kbo_index_build_device" in e.value.message
        with pytest.raises(_capi.KboError) as e:
            kbo_amd.index.build_sbwt_from_vecs(SEQS, kbo_amd.BuildOpts(k=31), device=-1)
        assert e.value.code == UNSUPPORTED and "kbo_index_build_device" in e.value.message
        # device=None keeps the host build
        sbwt, _ = kbo_amd.build(SEQS, kbo_amd.BuildOpts(k=31))
        assert sbwt.shards() == 2
    finally:
        L.kbo_set_index_shards(0)
    with pytest.raises(_capi.KboError) as e:
        kbo_amd.build(SEQS, kbo_amd.BuildOpts(k=0), device=0)
    assert e.value.code == BAD_ARG and "k must be in 1..255" in e.value.message
