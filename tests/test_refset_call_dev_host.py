"""The device-resident variant calls (kbo_hip.h "The VARIANTS of a pair": kbo_call_refset_dev, kbo_call_refset_screened_dev) without a
device: their figures and argument checks, and the second pass they run behind the last slab (kbo_amd/csrc/refset_resolve.hpp)
restated on the CPU through the hooks of kbo_hip_tuning.h -

  - the depths of a k-mer against the runs of a sequence, from the definition: for every position the longest suffix that bytes.find
    finds in a run of at least k bases (in the runs' reverse complements);
  - kbo_call_refset_host_indexed byte for byte against kbo_call_refset_host, whose second pass is a suffix automaton per sequence,
    on the worlds of tests/test_refset_call_host.py with every planted case;
  - the resolve word for every (common suffix, query peak, reference peak) against resolve_variant_peaks;
  - the order of the variants by radix passes over the sites' keys;
  - tools/refset_resolve_check.cpp, the same arithmetic through accessors that check every index, plain and under ASan + UBSan.
No GPU: tests/test_gpu_refset_call_dev.py runs the kernels."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import kbo_amd
from kbo_amd import _capi, refset

import test_refset_screen_host as screen_host
from test_refset_call_host import COMP, KS, PROBS, WIDE, call_opts, world

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_EMPTY_QUERY, E_THRESHOLD_LE_1, E_BAD_ARG, E_K_MISMATCH, E_UNSUPPORTED = -1, -3, -4, -6, -8
Q, OFF, WORK, VARS, CHARS, STATS, SCREEN = 0x10000, 0x20000, 0x30000, 0x50000, 0x60000, 0x70000, 0x80000
MIXED_ROWS = 20000  # (tests/test_refset_screened_dev_host.py: one long reference wide, the other of the single-index route)
NEW_SYMBOLS = ["kbo_call_refset_dev_work_bytes", "kbo_call_refset_dev", "kbo_call_refset_screened_dev_work_bytes", "kbo_call_refset_screened_dev"]
NEW_HOOKS = ["kbo_call_refset_host_indexed", "kbo_refset_kmer_depths_host", "kbo_refset_resolve_word_host", "kbo_refset_resolve_words_check",
             "kbo_refset_order_sites_host"]
NO_PEAK, NO_VARIANT, PANIC = 0xFF, 0xFFFFFFFF, 0xFFFFFFFE


def test_symbols_are_exported_and_declared():
    L = kbo_amd.lib()
    hdr = open(os.path.join(ROOT, "include", "kbo_hip.h")).read()
    tuning = open(os.path.join(ROOT, "include", "kbo_hip_tuning.h")).read()
    rust = open(os.path.join(ROOT, "bindings", "rust", "kbo-hip", "src", "lib.rs")).read()
    for name in NEW_SYMBOLS:
        assert getattr(L, name) is not None and name in _capi.SYMBOLS
        assert re.search(r"\b%s\(" % name, hdr) and re.search(r"pub fn %s\(" % name, rust), name
    for name in NEW_HOOKS:
        assert getattr(L, name) is not None and name in _capi.TUNING_SYMBOLS and re.search(r"\b%s\(" % name, tuning), name
    assert re.search(r"uint64_t n_panics;[^}]*uint64_t reserved\[3\];\s*\} kbo_ref_calls_stats;", hdr) and "pub struct RefCallsStats" in rust
    assert callable(refset.call_refset_dev) and callable(kbo_amd.call_refset_dev)
    assert "Open: references of the single-index route" in hdr and "a device-resident form, and references" not in hdr


@pytest.fixture(scope="module")
def sw():
    return screen_host.world(31, False)


def _wb(L, screened, h, n_seqs, total, strands, max_sites, a, b=0):
    if screened:
        return int(L.kbo_call_refset_screened_dev_work_bytes(h, n_seqs, total, strands, max_sites, a, b))
    return int(L.kbo_call_refset_dev_work_bytes(h, n_seqs, total, strands, max_sites, a))


@pytest.mark.parametrize("screened", [False, True])
def test_work_bytes_are_monotonic_at_least_the_summarys_and_zero_for_what_is_refused(sw, screened):
    L = kbo_amd.lib()
    h = sw.rs._h
    for n_seqs, total in ((1, 3), (21, 70000), (300, 1500), (2, 0)):
        for strands in (1, 2, 3):
            rest = (50, 20000) if screened else (2,)
            by_sites = [_wb(L, screened, h, n_seqs, total, strands, ms, *rest) for ms in (1, 2, 100, 4096, 4097, 1 << 16, 1 << 23)]
            assert by_sites[0] > 0 and all(v % 16 == 0 for v in by_sites) and all(a < b for a, b in zip(by_sites, by_sites[1:]))
            if screened:
                by_pairs = [_wb(L, True, h, n_seqs, total, strands, 1000, mp, 50000) for mp in (1, 2, 17, 1024, 1025, 100000, (1 << 28) - 1)]
                by_bases = [_wb(L, True, h, n_seqs, total, strands, 1000, 100, mb) for mb in (0, 1, 300, 5000, 1 << 20, (1 << 32) - 17)]
                assert all(a <= b for a, b in zip(by_pairs, by_pairs[1:])) and by_pairs[0] < by_pairs[3] < by_pairs[-1]
                assert all(a <= b for a, b in zip(by_bases, by_bases[1:])) and by_bases[3] < by_bases[4] < by_bases[5]
                for ms, mp, mb in ((1, 1, 0), (1, 100000, 3), (50, 40, 70000), (1 << 20, 1, 1)):
                    for cap in (0, 1 << 16):
                        s = int(L.kbo_summary_refset_screened_dev_work_bytes(h, n_seqs, total, strands, cap, mp, mb))
                        assert 0 < s <= _wb(L, True, h, n_seqs, total, strands, ms, mp, mb), (n_seqs, total, strands, ms, mp, mb)
            else:
                by_refs = [_wb(L, False, h, n_seqs, total, strands, 1000, r) for r in (1, 2, 3, 7, 19)]
                assert all(a <= b for a, b in zip(by_refs, by_refs[1:])) and by_refs[0] < by_refs[-1]
                assert _wb(L, False, h, n_seqs, total, strands, 1000, 0) == _wb(L, False, h, n_seqs, total, strands, 1000, 1 << 20) >= by_refs[-1]
                for ms, r in ((1, 1), (1, 0), (77, 3), (1 << 20, 2)):
                    for cap in (0, 1 << 16):
                        s = int(L.kbo_summary_refset_dev_work_bytes(h, n_seqs, total, strands, cap, r))
                        assert 0 < s <= _wb(L, False, h, n_seqs, total, strands, ms, r), (n_seqs, total, strands, ms, r)
    ok = dict(h=h, n_seqs=21, total=70000, strands=3, max_sites=100, a=5, b=500)

    def wb(**kw):
        a = dict(ok, **kw)
        return _wb(L, screened, a["h"], a["n_seqs"], a["total"], a["strands"], a["max_sites"], a["a"], a["b"])
    assert wb() > 0
    assert wb(h=None) == 0 and wb(h=screen_host.world(31, False, MIXED_ROWS).rs._h) == 0
    assert wb(n_seqs=0, total=0) == 0 and wb(strands=0) == 0 and wb(strands=4) == 0
    assert wb(max_sites=0) == 0 and wb(max_sites=(1 << 23) + 1) == 0 and wb(max_sites=1 << 23) > 0
    assert wb(total=(1 << 32) - 16, strands=1) == 0 and wb(total=1 << 31, strands=3) == 0 and wb(n_seqs=1 << 28, total=1 << 28, strands=1) == 0
    if screened:
        assert wb(h=sw.plain._h) == 0 and wb(a=0) == 0 and wb(a=1 << 28) == 0 and wb(b=(1 << 32) - 16) == 0
        assert wb(total=1 << 31, strands=1) == 0 and wb(n_seqs=1 << 26, total=1 << 26, strands=1) == 0
    else:
        assert wb(h=sw.plain._h) > 0  # (the unscreened form ignores the prefilter)


def _caller(L, screened, h, k=31, n_seqs=21, total=70000, max_sites=100, max_pairs=50, max_bases=20000):
    """the entry point with dummy device pointers; its figure"""
    wb1 = _wb(L, screened, h, n_seqs, total, 3, max_sites, max_pairs if screened else 1, max_bases)

    def call(h=h, q=Q, off=OFF, n_seqs=n_seqs, total=total, prob=1e-7, kk=k, strands=3, work=WORK, work_bytes=wb1, var=VARS, max_variants=10, chars=CHARS,
             max_chars=100, max_sites=max_sites, stats=STATS, max_pairs=max_pairs, max_bases=max_bases, screen=SCREEN, opts=True):
        o = _capi.CallOpts(prob, kbo_amd.BuildOpts(k=kk, build_select=True)._to_c())
        head = (h, q, off, n_seqs, total, C.byref(o) if opts else None, strands, work, work_bytes, var, max_variants, chars, max_chars, max_sites, stats)
        if screened:
            return L.kbo_call_refset_screened_dev(*head, max_pairs, max_bases, screen, None)
        return L.kbo_call_refset_dev(*head, None)
    return call, wb1


@pytest.mark.parametrize("screened", [False, True])
def test_argument_errors_and_their_order_need_no_device(sw, screened):
    L = kbo_amd.lib()
    call, wb1 = _caller(L, screened, sw.rs._h)
    assert wb1 > 0
    # the device forms' checks
    for null in ("h", "q", "off", "work", "stats", "var", "chars") + (("screen",) if screened else ()):
        assert call(**{null: None}) == E_BAD_ARG, null
    assert call(var=None, max_variants=0, chars=None, max_chars=0, work_bytes=wb1 - 1) == E_BAD_ARG  # (allowed: it gets as far as work_bytes)
    for name, base, step in [("q", Q, 8), ("q", Q, 1), ("off", OFF, 4), ("work", WORK, 8), ("stats", STATS, 4), ("var", VARS, 2)] + \
            ([("screen", SCREEN, 4)] if screened else []):
        assert call(**{name: base + step}) == E_BAD_ARG, (name, step)
    for strands in (0, 4, -1):
        assert call(strands=strands) == E_BAD_ARG
    for prob in (0.0, 1.5, -1e-7):
        assert call(prob=prob) == E_BAD_ARG
    assert call(n_seqs=0) == E_EMPTY_QUERY and call(prob=1.0) == E_THRESHOLD_LE_1
    mixed, _ = _caller(L, screened, screen_host.world(31, False, MIXED_ROWS).rs._h)
    assert mixed(work_bytes=1 << 40) == E_UNSUPPORTED  # a reference of the single-index route
    if screened:
        plain, _ = _caller(L, True, sw.plain._h)
        assert plain(work_bytes=1 << 40) == E_BAD_ARG  # a set without a prefilter
        assert call(max_pairs=0, work_bytes=1 << 60) == E_BAD_ARG and call(max_pairs=1 << 28, work_bytes=1 << 60) == E_UNSUPPORTED
    # then the call's own: k of the options, max_sites; work_bytes last
    assert call(kk=41) == E_K_MISMATCH and call(kk=41, max_sites=0) == E_K_MISMATCH and call(kk=41, work_bytes=0) == E_K_MISMATCH
    assert call(opts=False, work_bytes=0) == E_BAD_ARG  # (NULL options are the defaults, k = 31: as far as work_bytes)
    assert call(max_sites=0) == E_BAD_ARG and call(max_sites=0, work_bytes=0) == E_BAD_ARG
    assert call(max_sites=(1 << 23) + 1, work_bytes=1 << 60) == E_UNSUPPORTED
    assert call(work_bytes=wb1 - 1) == E_BAD_ARG and call(work_bytes=0) == E_BAD_ARG and call(max_sites=101) == E_BAD_ARG
    # the order: the device forms' before k, k before max_sites
    assert call(kk=41, strands=0) == E_BAD_ARG and call(kk=41, n_seqs=0) == E_EMPTY_QUERY and call(kk=41, prob=1.0) == E_THRESHOLD_LE_1
    assert mixed(kk=41, work_bytes=1 << 40) == E_UNSUPPORTED and call(kk=41, stats=None) == E_BAD_ARG
    if screened:
        assert call(kk=41, max_pairs=0) == E_BAD_ARG


# ---- depths against brute force
def _runs(seq, k):
    return [m.group(0) for m in re.finditer(rb"[ACGT]+", seq) if len(m.group(0)) >= k]


def _brute_depths(seq, kmer, k, q, mode):
    fwd = _runs(seq, k)
    rev = [bytes(COMP[np.frombuffer(r, dtype=np.uint8)[::-1]]) for r in fwd]
    runs = (fwd if mode & 1 else []) + (rev if mode & 2 else [])
    out = []
    for t in range(k):
        best = 0
        for n in range(min(t + 1, k), 0, -1):
            s = kmer[t + 1 - n:t + 1]
            if re.fullmatch(rb"[ACGT]+", s) and any(r.find(s) >= 0 for r in runs):
                best = n
                break
        out.append(best if best >= q else 0)
    return out


def _depths(seq, kmer, k, q, mode):
    s, km = np.frombuffer(seq, dtype=np.uint8), np.frombuffer(kmer, dtype=np.uint8)
    out = np.full(k, 0xDEAD, dtype=np.uint32)
    kbo_amd.check(kbo_amd.lib().kbo_refset_kmer_depths_host(s.ctypes.data, len(s), k, q, mode, km.ctypes.data, out.ctypes.data))
    return [int(v) for v in out]


@pytest.mark.parametrize("q", [3, 5])
@pytest.mark.parametrize("k", [5, 9])
def test_depths_against_brute_force(k, q):
    rng = np.random.default_rng(100 * k + q)
    rnd = lambda n: bytes(np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)])
    first, last = rnd(k + 3), rnd(k + 4)
    seq = (first + b"N" + rnd(k - 1) + b"n" + rnd(k) + b"acg" + rnd(2 * k) + b"N" + b"A" * 30 + rnd(3) + b"N" + b"AC" * 20 + rnd(k) +
           b"$" + rnd(k - 1) + b"N" + last)
    assert len(seq) <= 300
    runs = _runs(seq, k)
    assert any(len(r) == k for r in runs) and len(re.findall(rb"[ACGT]+", seq)) > len(runs)  # runs of k and of k - 1 bases
    kmers = [seq[p:p + k] for p in range(0, len(seq) - k + 1)]                                # '$', 'N' and lower case among them
    kmers += [first[:k], last[-k:]]                                                           # at the first and at the last base
    kmers += [bytes(COMP[np.frombuffer(m, dtype=np.uint8)[::-1]]) for m in kmers[::4]]        # reverse complements
    across = runs[0][-(k // 2 + 1):] + runs[1][:k - k // 2 - 1]                                # across a run boundary: must not count
    kmers.append(across)
    dollars = b"$" * (k - 3) + first[:3]
    kmers.append(dollars)
    checked = 0
    for mode in (1, 2, 3):
        for km in kmers:
            assert _depths(seq, km, k, q, mode) == _brute_depths(seq, km, k, q, mode), (mode, km)
            checked += 1
        # the k-mer of two runs' ends occurs nowhere as a whole, though each half does
        d = _depths(seq, across, k, q, 1)
        assert d[k - 1] < k and (q > k // 2 + 1 or d[k // 2] == k // 2 + 1)
    assert checked > 400
    assert _depths(seq, dollars, k, 3, 1)[:k - 3] == [0] * (k - 3) and _depths(seq, dollars, k, 3, 1)[k - 1] == 3
    # a sequence without a run of k bases has no depth at all; the argument checks
    short = rnd(k - 1) + b"N" + rnd(k - 1)
    assert _depths(short, short[:k], k, q, 3) == [0] * k
    L, out = kbo_amd.lib(), np.zeros(k, dtype=np.uint32)
    s = np.frombuffer(seq, dtype=np.uint8)
    for bad in (dict(mode=0), dict(mode=4), dict(q=0), dict(q=13), dict(q=k + 1), dict(k=256)):
        a = dict(dict(k=k, q=q, mode=1), **bad)
        assert L.kbo_refset_kmer_depths_host(s.ctypes.data, len(s), a["k"], a["q"], a["mode"], s.ctypes.data, out.ctypes.data) == E_BAD_ARG, bad
    assert L.kbo_refset_kmer_depths_host(None, 0, k, q, 1, s.ctypes.data, out.ctypes.data) == E_BAD_ARG


@pytest.mark.parametrize("base", [b"T", b"A"])
def test_depths_at_twelve_bases_with_homopolymers(base):
    """q = 12, the q of every call whose thresholds reach it: the code of T x 12 is the largest there is, and the positions without a
    word - behind an 'N', in a short run, the last 11 of the sequence - must not lie among its occurrences.  A homopolymer of T probed
    forwards, one of A probed as reverse complements, each behind such positions and in two runs"""
    k, q = 31, 12
    rng = np.random.default_rng(base[0])
    rnd = lambda n: bytes(np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)])
    other = b"A" if base == b"T" else b"T"
    seq = rnd(7) + b"N" + rnd(40) + b"NN" + base * 20 + rnd(k) + b"N" + rnd(5) + b"N" + rnd(9) + base * 45 + rnd(k) + b"n" + other * 33 + rnd(k)
    kmers = [seq[p:p + k] for p in range(0, len(seq) - k + 1)] + [base * k, other * k, rnd(10) + base * 21, rnd(10) + other * 21]
    kmers += [bytes(COMP[np.frombuffer(m, dtype=np.uint8)[::-1]]) for m in kmers[::3]]
    deep = 0
    for mode in (1, 2, 3):
        for km in kmers:
            got = _depths(seq, km, k, q, mode)
            assert got == _brute_depths(seq, km, k, q, mode), (mode, km)
            deep += sum(v >= q for v in got)
    # the k-mer cut from the first homopolymer's run, verbatim: its depths are 12 .. 31 where they are at least q, none is 0 behind that
    at = seq.index(base * 20)
    d = _depths(seq, seq[at:at + k], k, q, 1)
    assert d[:q - 1] == [0] * (q - 1) and d[q - 1:] == list(range(q, k + 1)) and deep > 5000
    assert _depths(seq, bytes(COMP[np.frombuffer(base * k, dtype=np.uint8)]), k, q, 2)[q - 1:] == list(range(q, k + 1))


# ---- the whole call
def _call_indexed(w, opts, strands):
    """kbo_call_refset_host_indexed itself, not through kbo_amd.refset's dispatch"""
    concat = np.ascontiguousarray(np.concatenate(w.seqs))
    off = np.zeros(len(w.seqs) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(s) for s in w.seqs])
    co = _capi.CallOpts(opts.max_error_prob, opts.sbwt_build_opts._to_c())
    res = _capi.RefCalls()
    L = kbo_amd.lib()
    kbo_amd.check(L.kbo_call_refset_host_indexed(w.rs._h, concat.ctypes.data, off.ctypes.data, len(w.seqs), C.byref(co), strands, C.byref(res)))
    try:
        variants = bytes((C.c_uint8 * (res.n_variants * 24)).from_address(res.variants)) if res.n_variants else b""
        chars = bytes((C.c_uint8 * res.n_chars).from_address(res.chars)) if res.n_chars else b""
        return variants, chars
    finally:
        L.kbo_ref_calls_free(C.byref(res))


@pytest.mark.parametrize("rc", [False, True])
@pytest.mark.parametrize("k", KS)
def test_indexed_second_pass_equals_the_automaton_form(k, rc):
    """kbo_call_refset_host_indexed == kbo_call_refset_host byte for byte: both add_revcomp of the options, strands 1 - 3, both
    probabilities; the planted cases of the world are there (tests/test_refset_call_host.py asserts that they occur)"""
    w = world(k, rc)
    assert set(["N", "'$' in the row", "j < k - 1", "joint"]) <= set(w.at) and ("j = len - 1", 1e-7) in w.at and len(w.seqs[7]) > 9000
    total = 0
    for prob in PROBS:
        for arc in (False, True):
            for strands in (3, 1, 2):
                o = call_opts(k, prob, arc)
                a = refset.call_refset(w.seqs, w.rs, o, strands, host=True)
                counts = refset.last_call()
                b = _call_indexed(w, o, strands)
                assert (a[0].tobytes(), a[1].tobytes()) == b, (k, rc, prob, arc, strands)
                assert refset.last_call() == counts
                if strands == 3 and not arc:  # (and through the Python mirror)
                    c = refset.call_refset(w.seqs, w.rs, o, strands, host="indexed")
                    assert (c[0].tobytes(), c[1].tobytes()) == b
                total += len(a[0])
                if strands == 3 and prob == 1e-7 and k >= 41:
                    wide = a[0][(a[0]["ref"] == WIDE) & (a[0]["seq"] == 7)]
                    assert len(wide) >= 200 and counts[2] >= 243  # the contig with 243 sites
    assert total > 1000


def test_indexed_form_checks_its_arguments_like_the_host_form():
    L = kbo_amd.lib()
    w = world(41, False)
    concat = np.concatenate(w.seqs)
    off = np.zeros(len(w.seqs) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(s) for s in w.seqs])
    res = _capi.RefCalls(7, 7, 0x1000, 0x1000)

    def call(h=w.rs._h, kk=41, prob=1e-7, strands=3, n_seqs=len(w.seqs)):
        o = _capi.CallOpts(prob, kbo_amd.BuildOpts(k=kk, build_select=True)._to_c())
        return L.kbo_call_refset_host_indexed(h, concat.ctypes.data, off.ctypes.data, n_seqs, C.byref(o), strands, C.byref(res))
    assert call(strands=0) == E_BAD_ARG and (res.n_variants, res.variants) == (7, 0x1000)
    assert call(kk=31) == E_K_MISMATCH and (res.n_variants, res.variants) == (0, None)
    assert call(prob=2.0) == E_BAD_ARG and call(n_seqs=0) == E_EMPTY_QUERY and call(h=None) == E_BAD_ARG
    rng = np.random.default_rng(4)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    v, c = refset.call_refset([acgt[rng.integers(0, 4, 3000)]], w.rs, call_opts(41), host="indexed")
    assert len(v) == 0 == len(c) and refset.last_call()[2:] == (0, 0)


# ---- the resolve word
def _reference_resolve(k, csl, qpeak, rpeak):
    """resolve_variant (variant_calling.rs:139-201) on the three values: 'panic', None, or (q_from, q_to, r_from, r_to)"""
    if csl == 0:
        return "panic"
    if qpeak is None or rpeak is None:
        return None
    sms = k - csl
    query_gap, ref_gap = sms - qpeak - 1, sms - rpeak - 1
    if query_gap > 0 and ref_gap > 0:
        return (qpeak + 1, sms, rpeak + 1, sms)
    qo, ro = -query_gap, -ref_gap
    if qo == ro:
        return None
    vlen = abs(qo - ro)
    if qo > ro:
        return "panic" if rpeak + 1 + vlen > k else (0, 0, rpeak + 1, rpeak + 1 + vlen)
    return "panic" if qpeak + 1 + vlen > k else (qpeak + 1, qpeak + 1 + vlen, 0, 0)


@pytest.mark.parametrize("k", [5, 31, 64, 96, 255])
def test_the_resolve_word_exhaustively(k):
    L = kbo_amd.lib()
    counts = (C.c_uint64 * 4)()
    kbo_amd.check(L.kbo_refset_resolve_words_check(k, counts))
    cases, differ, panics, variants = (int(v) for v in counts)
    assert cases == (k + 1) * k * k and differ == 0 and variants > 0
    # the panics: a common suffix of 0 (k * k cases) and the slices beyond the k-mer, counted from the definition
    peaks = [None] + list(range(k - 1))
    if k <= 64:
        want = [_reference_resolve(k, csl, qp, rp) for csl in range(k + 1) for qp in peaks for rp in peaks]
        assert panics == sum(v == "panic" for v in want) and variants == sum(isinstance(v, tuple) for v in want)
    assert panics >= k * k
    # sampled cases through the single-case hook, against the definition written out here: the ranges, "no variant", the panics
    rng = np.random.default_rng(k)
    out = (C.c_uint32 * 6)()
    sample = [(0, 0, 0), (0, None, 1), (k, 0, 0), (1, k - 2, k - 2), (1, None, None), (k, k - 2, 0), (1, 0, k - 2), (2, k - 2, 0)]
    sample += [(int(rng.integers(0, k + 1)), peaks[int(rng.integers(0, k))], peaks[int(rng.integers(0, k))]) for _ in range(3000)]
    kinds = set()
    for csl, qp, rp in sample:
        kbo_amd.check(L.kbo_refset_resolve_word_host(k, csl, NO_PEAK if qp is None else qp, NO_PEAK if rp is None else rp, out))
        word, verdict = int(out[0]), int(out[1])
        want = _reference_resolve(k, csl, qp, rp)
        if want == "panic":
            assert word == PANIC and verdict == 2, (csl, qp, rp)
        elif want is None:
            assert word == NO_VARIANT and verdict == 0, (csl, qp, rp)
        else:
            qf, qt, rf, rt = want
            assert verdict == 1 and tuple(out[2:6]) == want and 0 <= qf <= qt <= k and 0 <= rf <= rt <= k, (csl, qp, rp)
            assert ((word >> 8) & 0xFF, word >> 24) == (qt - qf, rt - rf)
            assert (qt == qf or word & 0xFF == qf) and (rt == rf or (word >> 16) & 0xFF == rf)
        kinds.add(want if want in ("panic", None) else ("sub" if want[1] > want[0] and want[3] > want[2] else "ins" if want[1] > want[0] else "del"))
    assert kinds == {"panic", None, "sub", "ins", "del"}
    assert L.kbo_refset_resolve_word_host(k, k + 1, 0, 0, out) == E_BAD_ARG and L.kbo_refset_resolve_word_host(k, 1, k - 1, 0, out) == E_BAD_ARG
    assert L.kbo_refset_resolve_words_check(256, counts) == E_BAD_ARG and L.kbo_refset_resolve_words_check(k, None) == E_BAD_ARG


# ---- the order
def _order(refs, seqs, strands, pos, n_refs, n_seqs, total):
    a = [np.ascontiguousarray(v, dtype=np.uint32) for v in (refs, seqs, strands, pos)]
    out = np.full(len(a[0]), 0xFFFFFFFF, dtype=np.uint32)
    rc = kbo_amd.lib().kbo_refset_order_sites_host(len(out), *[v.ctypes.data for v in a], n_refs, n_seqs, total, out.ctypes.data)
    return rc, out


@pytest.mark.parametrize("shape", [(15, 8, 100_000), (2000, 1, 5_000_000), (1, 1, 70_000), (3, 300, (1 << 32) - 17), (255, 257, 65_536)])
def test_the_order_of_shuffled_sites(shape):
    """sites with equal (ref, seq) and different strands, with equal pairs, and one pair that holds 5 000 sites: sorted, a permutation"""
    n_refs, n_seqs, total = shape
    rng = np.random.default_rng(n_refs)
    n = 4000
    refs, seqs = rng.integers(0, n_refs, n), rng.integers(0, n_seqs, n)
    strands, pos = rng.integers(1, 3, n), rng.integers(0, min(total, 1 << 32), n)
    # pairs that share (ref, seq) on both strands, and 5 000 sites of one pair
    refs[:500], seqs[:500] = refs[500:1000], seqs[500:1000]
    strands[:500], strands[500:1000] = 1, 2
    big = 5000
    refs = np.concatenate([refs, np.full(big, n_refs - 1)])
    seqs = np.concatenate([seqs, np.full(big, n_seqs - 1)])
    strands = np.concatenate([strands, np.full(big, 2)])
    pos = np.concatenate([pos, rng.choice(min(total, 1 << 20), big, replace=False)])
    keys = np.stack([refs, seqs, strands, pos], axis=1).astype(np.int64)
    _, first = np.unique(keys, axis=0, return_index=True)  # (a pair has one site at a position)
    keep = rng.permutation(np.sort(first))
    refs, seqs, strands, pos, keys = refs[keep], seqs[keep], strands[keep], pos[keep], keys[keep]
    rc, order = _order(refs, seqs, strands, pos, n_refs, n_seqs, total)
    assert rc == 0 and np.array_equal(np.sort(order), np.arange(len(keep)))
    want = np.lexsort((keys[:, 3], keys[:, 2], keys[:, 1], keys[:, 0]))
    assert np.array_equal(order, want)
    assert int(((refs == n_refs - 1) & (seqs == n_seqs - 1) & (strands == 2)).sum()) >= big
    # what lies outside the shape is refused
    for bad in (dict(refs=[n_refs]), dict(seqs=[n_seqs]), dict(strands=[0]), dict(strands=[3]), dict(pos=[total])):
        a = dict(dict(refs=[0], seqs=[0], strands=[1], pos=[0]), **bad)
        assert _order(a["refs"], a["seqs"], a["strands"], a["pos"], n_refs, n_seqs, total)[0] == E_BAD_ARG, bad
    assert _order([], [], [], [], n_refs, n_seqs, total)[0] == 0


# ---- the check program
def _check_tool(tmp_path, sanitize):
    exe = str(tmp_path / ("refset_resolve_check" + ("_san" if sanitize else "")))
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else []
    subprocess.run(["c++", "-std=c++17", "-O1", "-g"] + flags + ["-I", os.path.join(ROOT, "kbo_amd", "csrc"),
                    os.path.join(ROOT, "tools", "refset_resolve_check.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    return run.stdout


@pytest.mark.parametrize("sanitize", [False, True])
def test_resolve_arithmetic_through_checked_accessors(tmp_path, sanitize):
    """tools/refset_resolve_check.cpp as a stand-alone program, plain and under AddressSanitizer and UBSan"""
    out = _check_tool(tmp_path, sanitize)
    assert "every index in range" in out and " 0 out of range or wrong" in out
    m = re.search(r"(\d+) depths agree with the definition", out)
    assert m and int(m.group(1)) > 100_000
    assert len(re.findall(r"resolve words agree with the reference", out)) == 5 and re.search(r"k 255: 16646400 resolve words", out)
    m = re.search(r"(\d+) sites ordered by their keys", out)
    assert m and int(m.group(1)) > 30_000
