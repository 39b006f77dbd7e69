"""kbo_call_refset (kbo_hip.h "The VARIANTS of a pair") on the GPU.

Yardstick 1, the oracle's literal kbo::call per pair, is what tests/test_refset_call_host.py holds kbo_call_refset_host to, field by
field; here the GPU call must return the bytes of that host form - records and characters - on the same worlds: a dozen references of
300 to 2 000 bases, one of 20 kbp on the wide route, one without a k-mer, two alleles of each other, and eight contigs with the
planted cases of that file (at least 200 sites a world, i mod 64 taking every value).  Yardstick 2, for add_revcomp of the call's
options, which the oracle's call does not model: kbo_amd.call on one kbo_amd.build per reference, for the pairs with a summary
record.  All comparisons are exact."""
import numpy as np
import pytest

import kbo_amd
from kbo_amd import refset

from test_refset_call_host import ALLELE_B, WIDE, _rnd, as_tuples, call_opts, strand_seq, world

pytestmark = pytest.mark.gpu

DEFAULT_SLAB = 16 << 20


def _same(a, b):
    return a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


_host = {}


def _host_form(k, rc, strands, prob=1e-7, add_revcomp=False):
    """kbo_call_refset_host of a world, once (the prefilter changes no record)"""
    key = (k, rc, strands, prob, add_revcomp)
    if key not in _host:
        w = world(k, rc)
        _host[key] = refset.call_refset(w.seqs, w.rs, call_opts(k, prob, add_revcomp), strands, host=True)
    return _host[key]


@pytest.mark.parametrize("prefilter", [False, True])
@pytest.mark.parametrize("rc", [False, True])
@pytest.mark.parametrize("k", [31, 41, 63, 96])
def test_call_equals_the_host_form(k, rc, prefilter):
    w = world(k, rc, prefilter)
    assert w.rs.has_prefilter == prefilter and w.rs.packed_only()
    walked = {}
    for strands in (1, 2, 3):
        exp = _host_form(k, rc, strands)
        got = refset.call_refset(w.seqs, w.rs, call_opts(k), strands)
        assert _same(got, exp), (strands, len(got[0]), len(exp[0]))
        stats, pre = refset.last_call(), refset.last_prefilter()
        assert stats[3] == len(exp[0]) and stats[1] >= stats[2] >= stats[3] and stats[0] == pre[2] == refset.last_routes()[2]
        assert pre[3] == (1 if prefilter else 0)
        if strands & 1 or rc:
            assert stats[2] > 200  # the kernels were reached: sites
        else:
            assert stats[2] > 0  # '-' alone on a set without reverse complements: the copy that lies on '-' only has two variants
        if k >= 41 and (strands & 1 or rc):
            assert stats[3] > 100
        walked[strands] = stats[0]
    if prefilter:  # the screened call walked fewer pairs and returned the same bytes
        plain = world(k, rc, False)
        refset.call_refset(plain.seqs, plain.rs, call_opts(k), 3)
        assert 0 < walked[3] < refset.last_call()[0]
    assert refset.last_wide()[0] == 1 and (k < 41 or WIDE in set(exp[0]["ref"]))


@pytest.mark.parametrize("k,rc", [(41, False), (96, True)])
def test_the_other_max_error_prob(k, rc):
    w = world(k, rc, True)
    got = refset.call_refset(w.seqs, w.rs, call_opts(k, 1e-4), 3)
    assert _same(got, _host_form(k, rc, 3, 1e-4)) and len(got[0]) > 100


def test_several_slabs_and_lists_that_overflow():
    """64 KiB of pair bytes a slab; then room for ONE candidate at first, so that every slab is scanned again with room for its count"""
    k, rc = 41, True
    w = world(k, rc)
    exp = _host_form(k, rc, 3)
    L = kbo_amd.lib()
    got = refset.call_refset(w.seqs, w.rs, call_opts(k), 3)
    one, cands, sites = refset.last_routes()[3], refset.last_call()[1], refset.last_call()[2]
    L.kbo_set_slab_bytes(1 << 16)
    try:
        again = refset.call_refset(w.seqs, w.rs, call_opts(k), 3)
        many = refset.last_routes()[3]
        assert refset.last_call()[1:] == (cands, sites, len(exp[0])) and cands > sites > 200
    finally:
        L.kbo_set_slab_bytes(DEFAULT_SLAB)
    assert _same(got, exp) and _same(again, exp) and many > one and many >= 4
    L.kbo_set_refset_record_capacity(1)
    try:
        tight = refset.call_refset(w.seqs, w.rs, call_opts(k), 3)
    finally:
        L.kbo_set_refset_record_capacity(1 << 16)
    assert _same(tight, exp) and refset.last_call()[1:3] == (cands, sites)


@pytest.mark.parametrize("add_revcomp", [False, True])
def test_against_call_on_one_index_per_reference(add_revcomp):
    """yardstick 2: kbo_amd.call on kbo_amd.build of each reference alone, for the pairs kbo_summary_refset has a record for"""
    k, rc = 41, True
    w = world(k, rc)
    refs = (7, 11, ALLELE_B)
    opts = call_opts(k, add_revcomp=add_revcomp)
    variants, chars = refset.call_refset(w.seqs, w.rs, opts, 3)
    assert _same((variants, chars), _host_form(k, rc, 3, add_revcomp=add_revcomp))
    got = [v for v in as_tuples(variants, chars) if v[0] in refs]
    pairs = {(int(x["ref"]), int(x["seq"]), int(x["strand"])) for x in refset.summary_refset(w.seqs, w.rs, 1e-7, 3)}
    exp = []
    for r in refs:
        sbwt, lcs = kbo_amd.build([w.refs[r]], kbo_amd.BuildOpts(k=k, add_revcomp=rc, num_threads=2))
        for s, q in enumerate(w.seqs):
            for strand in (1, 2):
                if (r, s, strand) in pairs:
                    exp += [(r, s, strand, int(v.query_pos), bytes(v.query_chars), bytes(v.ref_chars))
                            for v in kbo_amd.call(sbwt, lcs, strand_seq(q, strand), opts)]
    assert got == exp and len(exp) > 8


def test_twice_and_behind_a_find():
    k, rc = 63, False
    w = world(k, rc, True)
    exp = _host_form(k, rc, 3)
    a = refset.call_refset(w.seqs, w.rs, call_opts(k), 3)
    b = refset.call_refset(w.seqs, w.rs, call_opts(k), 3)
    runs = refset.find_refset(w.seqs, w.rs, strands=3)
    c = refset.call_refset(w.seqs, w.rs, call_opts(k), 3)
    assert len(runs) > 10 and _same(a, exp)  # (a run at least for each of the dozen references with a copy)
    assert _same(b, exp) and _same(c, exp)


def test_unrelated_contigs_give_nothing():
    import ctypes as C
    from kbo_amd import _capi
    k = 41
    w = world(k, False)
    rng = np.random.default_rng(12)
    seqs = [_rnd(rng, 3000), _rnd(rng, 700)]
    variants, chars = refset.call_refset(seqs, w.rs, call_opts(k), 3)
    assert len(variants) == 0 == len(chars) and refset.last_call()[2:] == (0, 0) and refset.last_call()[0] > 0
    concat, off = np.concatenate(seqs), np.array([0, 3000, 3700], dtype=np.uint64)
    res = _capi.RefCalls(5, 5, 0x1000, 0x1000)
    o = _capi.CallOpts(1e-7, kbo_amd.BuildOpts(k=k, build_select=True)._to_c())
    assert kbo_amd.lib().kbo_call_refset(w.rs._h, concat.ctypes.data, off.ctypes.data, 2, C.byref(o), 3, C.byref(res)) == 0
    assert (res.n_variants, res.n_chars, res.variants, res.chars) == (0, 0, None, None)
