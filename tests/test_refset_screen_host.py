"""The seed screen of a reference set (kbo_hip.h "A set with a PREFILTER") on the host: kbo_refset_build_opts, the seed table's
figures, kbo_refset_candidates_host - the CPU restatement of refset_screen_kernel over kbo_amd/csrc/refset_screen.hpp - and the
argument errors.  Every bit is checked in two ways:
  - against the contract, by brute force here: sets of m_r-mers of the reference's indexed stretches (numpy integers, nothing from
    the library but the thresholds' inputs k and n_kmers) against the m_r-mers of the sequence on that strand;
  - against the walk: the bit is 1 wherever max(kbo_refset_ms_host) >= w_r = min(t_r + 1, k), the least a record needs.
tools/refset_screen_check.cpp runs the seed and the bucket scan through an accessor that checks every index, as a stand-alone program
under AddressSanitizer and UBSan.  No GPU.  tests/test_gpu_refset_screen.py takes world() from here."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import kbo_amd
from kbo_amd import _capi, refset

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_LEN_LE_2, E_THRESHOLD_LE_1, E_BAD_ARG, E_UNSUPPORTED = -2, -3, -4, -8
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
COMP = np.arange(256, dtype=np.uint8)
for _a, _b in zip(b"ACGTacgt", b"TGCAtgca"):
    COMP[_a] = _b
CODE = np.full(256, 4, dtype=np.uint8)
for _i, _a in enumerate(b"ACGT"):
    CODE[_a] = _i
SEED_MAX, SEED_MIN = refset.SEED_MAX, refset.SEED_MIN
PROBS = (1e-7, 1e-4, 1e-12, 0.5)
N_UNRELATED, BIG = 3, 3  # the first contigs are unrelated to every reference; the contig with the planted seeds across boundaries
BIG_AT = 5000 + 12000 + 20000  # where BIG begins in the concatenated batch
PLANTED = (4, 5, 6, 7, 8, 9, 10, 11)  # references with 60 bases in BIG
SHORT_REF, N_REF, GAP_REF, TWIN_A, TWIN_B, WIDE_A, WIDE_B = 14, 15, 16, 17, 18, 12, 13


def _rnd(rng, n):
    return ACGT[rng.integers(0, 4, n)].copy()


def _mutate(rng, a, rate):
    a = a.copy()
    pos = np.flatnonzero(rng.random(len(a)) < rate)
    a[pos] = ACGT[(np.searchsorted(ACGT, a[pos]) + rng.integers(1, 4, len(pos))) % 4]
    return a


def _other(base):
    """a base that differs from `base`"""
    return ACGT[(int(np.searchsorted(ACGT, base)) + 1) % 4]


def threshold(k, n_kmers, prob):
    t = C.c_size_t()
    kbo_amd.check(kbo_amd.lib().kbo_random_match_threshold(k, n_kmers, 4, prob, C.byref(t)))
    return t.value


def seed_len(k, n_kmers, prob):
    """m_r"""
    return min(threshold(k, n_kmers, prob) + 1, k, SEED_MAX)


def make_refs(k, seed):
    rng = np.random.default_rng(seed)
    refs = [_rnd(rng, n) for n in (300, 333, 410, 500, 640, 700, 777, 850, 900, 1000, 1100, 1200)]
    refs += [_rnd(rng, 19970), _rnd(rng, 20050)]  # more than KBO_REFSET_MAX_ROWS rows: wide, or single-index
    refs.append(_rnd(rng, k - 1))                 # no k-mer: a status
    with_n = _rnd(rng, 700)
    with_n[300] = ord("N")
    with_n[350:370] |= 0x20                       # a lower-case stretch
    refs.append(with_n)
    gap = np.concatenate([_rnd(rng, 200), [ord("N")], _rnd(rng, k - 1), [ord("N")], _rnd(rng, 400)]).astype(np.uint8)
    refs.append(gap)                              # a run of k - 1 bases between two Ns: not indexed
    twin = _rnd(rng, 500)
    other = twin.copy()
    other[250] = _other(other[250])
    refs += [twin, other]                         # equal codes in one bucket, from two references
    return refs


def _exactly(rng, ref, at, n, left=200, right=200):
    """random bases around exactly n bases of ref from `at` on: the bases next to them differ from the reference's"""
    a, b = _rnd(rng, left), _rnd(rng, right)
    if left:
        a[-1] = _other(ref[at - 1])
    if right:
        b[0] = _other(ref[at + n])
    return np.concatenate([a, ref[at:at + n], b])


def make_seqs(k, refs, m, seed):
    """m: m_r of every reference at 1e-7"""
    rng = np.random.default_rng(seed)
    seqs = [_rnd(rng, n) for n in (5000, 12000, 20000)]
    big = _rnd(rng, 16000)
    run, group = lane_run(), lane_run() * lane_threads()
    wg_cut = (BIG_AT // group + 1) * group - BIG_AT         # the first workgroup boundary inside BIG, in its own coordinates
    lane_cut = ((BIG_AT + 3000) // run + 1) * run - BIG_AT  # a boundary between two lanes of one workgroup
    assert 0 < wg_cut < len(big) - 100 and (BIG_AT + lane_cut) % group and abs(lane_cut - wg_cut) > 200
    for r, cut in ((0, wg_cut), (1, lane_cut)):             # exactly m_r bases, half of them on either side of the boundary
        at = cut - m[r] // 2
        big[at - 1:at + m[r] + 1] = _exactly(rng, refs[r], 100, m[r], 1, 1)
    for i, r in enumerate(PLANTED):                         # more pairs of this long contig for the slabs of the calls
        big[5000 + 500 * i:5060 + 500 * i] = refs[r][150:210]
    seqs.append(big)
    seqs.append(np.concatenate([_rnd(rng, 300), _mutate(rng, refs[3], 0.02), _rnd(rng, 300)]))
    seqs.append(np.concatenate([_rnd(rng, 500), COMP[refs[5][::-1]], _rnd(rng, 100)]))
    seqs.append(np.concatenate([_exactly(rng, refs[6], 100, m[6] - 1), _exactly(rng, refs[7], 100, m[7])]))  # one base short / enough
    seqs.append(_exactly(rng, refs[8], 200, m[8], 400, 0))   # its only seed ends on its last base
    seqs.append(_exactly(rng, refs[9], 50, m[9], 0, 400))    # ... starts on its first base
    cut_n = np.concatenate([_rnd(rng, 100), refs[10][100:100 + m[10] - 1], [ord("N")], refs[10][100 + m[10]:110 + m[10]], _rnd(rng, 100)])
    seqs.append(cut_n.astype(np.uint8))                      # an N one base short of m_r
    seqs += [refs[11][:3].copy(), refs[11][:10].copy(), refs[11][:23].copy()]
    lower = np.concatenate([_rnd(rng, 100), refs[2], _rnd(rng, 100)])
    lower[150:250] |= 0x20
    seqs.append(lower)                                       # lower case in the query
    seqs.append(np.concatenate([_rnd(rng, 100), refs[GAP_REF][201:201 + k - 1], _rnd(rng, 100)]))  # the run that is not indexed
    seqs.append(np.concatenate([_rnd(rng, 50), refs[TWIN_A][200:300], _rnd(rng, 50)]))             # across the twins' one difference
    seqs.append(np.concatenate([_mutate(rng, refs[WIDE_A][5000:5600], 0.01), _rnd(rng, 40), refs[WIDE_B][100:500]]))  # the long ones
    return seqs


def _header_const(name):
    hpp = open(os.path.join(ROOT, "kbo_amd", "csrc", "kernels.hpp")).read()
    return int(re.search(r"constexpr uint32_t %s = (\d+);" % name, hpp).group(1))


def lane_run():
    return _header_const("kRefsetScreenRun")


def lane_threads():
    return _header_const("kRefsetScreenThreads")


# ---- the contract by brute force: m-mers as integers
def mers(a, m):
    """the codes of the m-mers of a that lie within it and are all bases"""
    c = CODE[a].astype(np.uint64)
    if len(c) < m:
        return np.zeros(0, dtype=np.uint64)
    n = len(c) - m + 1
    code = np.zeros(n, dtype=np.uint64)
    for j in range(m):
        code = code << np.uint64(2) | (c[j:j + n] & np.uint64(3))
    bad = np.concatenate([[0], np.cumsum(c > 3)])
    return code[bad[m:] == bad[:-m]]


def stretches(a, k):
    """the maximal runs of bases of at least k"""
    ok = np.concatenate([[False], CODE[a] < 4, [False]])
    edges = np.flatnonzero(ok[1:] != ok[:-1])
    return [a[i:j] for i, j in zip(edges[::2], edges[1::2]) if j - i >= k]


class World:
    pass


_cache = {}


def world(k, rc, wide_rows=refset.WIDE_MAX_ROWS):
    """references, sequences, the sets with and without the prefilter, per-pair brute force - once per (k, rc, wide_rows)"""
    key = (k, rc, wide_rows)
    if key in _cache:
        return _cache[key]
    w = World()
    w.k, w.rc = k, rc
    w.refs = make_refs(k, 4100 + k)
    opts = kbo_amd.BuildOpts(k=k, add_revcomp=rc, num_threads=4)
    w.rs = refset.RefSet.build(w.refs, opts, wide_rows=wide_rows, prefilter=True)
    w.plain = refset.RefSet.build(w.refs, opts, wide_rows=wide_rows)
    w.n_kmers = [w.rs.n_kmers(r) for r in range(len(w.refs))]
    w.packed = [r for r in range(len(w.refs)) if w.rs.status(r) == 0 and w.rs.route(r) != refset.ROUTE_INDEX]
    w.m = {p: [seed_len(k, n, p) if n else 0 for n in w.n_kmers] for p in PROBS}
    w.wr = {p: [min(threshold(k, n, p) + 1, k) if n else 0 for n in w.n_kmers] for p in PROBS}
    w.seqs = make_seqs(k, w.refs, w.m[1e-7], 4200 + k)
    w.stretches = {r: [x for st in stretches(w.refs[r], k) for x in ([st, COMP[st[::-1]]] if rc else [st])] for r in w.packed}
    w.strand = {(s, 1): q for s, q in enumerate(w.seqs)}
    w.strand.update({(s, 2): COMP[q[::-1]] for s, q in enumerate(w.seqs)})
    w._ref_mers, w._seq_mers = {}, {}
    _cache[key] = w
    return w


def expected(w, prob, strands=3):
    """the contract: [n_refs, n_seqs, 2]"""
    out = np.zeros((len(w.refs), len(w.seqs), 2), dtype=bool)
    for r in w.packed:
        m = w.m[prob][r]
        for s in range(len(w.seqs)):
            for strand in (1, 2):
                if not strands & strand:
                    continue
                if m < SEED_MIN:  # the reference cannot be screened at this max_error_prob: all its pairs
                    out[r, s, strand - 1] = True
                    continue
                if (r, m) not in w._ref_mers:
                    w._ref_mers[r, m] = np.unique(np.concatenate([mers(st, m) for st in w.stretches[r]]))
                if (s, strand, m) not in w._seq_mers:
                    w._seq_mers[s, strand, m] = np.unique(mers(w.strand[s, strand], m))
                out[r, s, strand - 1] = bool(np.isin(w._seq_mers[s, strand, m], w._ref_mers[r, m], assume_unique=True).any())
    return out


def max_ms(w):
    """[n_refs, n_seqs, 2]: the largest matching statistic of every pair of a packed reference, by the walk's step on the CPU"""
    if not hasattr(w, "_max_ms"):
        w._max_ms = np.zeros((len(w.refs), len(w.seqs), 2), dtype=np.int64)
        for r in w.packed:
            for (s, strand), q in w.strand.items():
                w._max_ms[r, s, strand - 1] = int(w.rs.ms_host(r, q).max())
    return w._max_ms


@pytest.fixture(scope="module", params=[False, True], ids=["fwd", "revcomp"])
def w31(request):
    return world(31, request.param)


def test_symbols_are_exported_and_declared():
    L = kbo_amd.lib()
    api = open(os.path.join(ROOT, "include", "kbo_hip.h")).read()
    tuning = open(os.path.join(ROOT, "include", "kbo_hip_tuning.h")).read()
    for name in ("kbo_refset_opts_default", "kbo_refset_build_opts", "kbo_refset_has_prefilter", "kbo_refset_prefilter_bytes",
                 "kbo_refset_candidates"):
        assert getattr(L, name) is not None and name in _capi.SYMBOLS and re.search(r"\b%s\(" % name, api), name
    for name in ("kbo_refset_candidates_host", "kbo_set_refset_prefilter_max_bits", "kbo_refset_last_prefilter"):
        assert getattr(L, name) is not None and name in _capi.TUNING_SYMBOLS and re.search(r"\b%s\(" % name, tuning), name
    hpp = open(os.path.join(ROOT, "kbo_amd", "csrc", "refset_screen.hpp")).read()
    assert int(re.search(r"#define KBO_REFSET_SEED_MAX (\d+)", api).group(1)) == SEED_MAX == 24
    assert int(re.search(r"#define KBO_REFSET_SEED_MIN (\d+)", api).group(1)) == SEED_MIN
    assert int(re.search(r"constexpr uint32_t kSeedMax = (\d+);", hpp).group(1)) == SEED_MAX
    assert int(re.search(r"constexpr uint32_t kSeedMin = (\d+);", hpp).group(1)) == SEED_MIN
    assert int(re.search(r"#define KBO_REFSET_SCREEN_RUN (\d+)", tuning).group(1)) == lane_run()
    assert int(re.search(r"#define KBO_REFSET_SCREEN_THREADS (\d+)", tuning).group(1)) == lane_threads()
    o = _capi.RefsetOpts(0, 7)
    L.kbo_refset_opts_default(C.byref(o))
    assert (o.max_wide_rows, o.prefilter) == (refset.MAX_ROWS, 0)
    assert L.kbo_refset_last_prefilter(None) == E_BAD_ARG


def test_the_world_is_what_it_says(w31):
    w = w31
    assert w.rs.has_prefilter and not w.plain.has_prefilter and w.plain.prefilter_bytes() == 0
    assert w.rs.status(SHORT_REF) != 0 and SHORT_REF not in w.packed and len(w.packed) == len(w.refs) - 1
    assert w.rs.route(WIDE_A) == w.rs.route(WIDE_B) == refset.ROUTE_WIDE and w.rs.route(0) == refset.ROUTE_LDS
    # the four max_error_prob values: m_r = w_r at 1e-7 and 1e-4, the cap applies at 1e-12, nothing can be screened at 0.5
    for r in w.packed:
        assert SEED_MIN <= w.m[1e-7][r] == w.wr[1e-7][r] < SEED_MAX and SEED_MIN <= w.m[1e-4][r] == w.wr[1e-4][r]
        assert w.m[1e-12][r] == SEED_MAX <= w.wr[1e-12][r] and w.m[0.5][r] < SEED_MIN
    assert any(w.wr[1e-12][r] > SEED_MAX for r in w.packed)
    exp = expected(w, 1e-7)
    # the claim the screen rests on - few candidates - of the brute force itself
    assert not exp[:, :N_UNRELATED].any(), np.argwhere(exp[:, :N_UNRELATED])
    assert exp[0, BIG, 0] and exp[1, BIG, 0]                                    # the seeds across the boundaries
    assert exp[3, BIG + 1, 0] and exp[5, BIG + 2, 1] and exp[5, BIG + 2, 0] == w.rc  # the mutated copy, the reverse complement
    assert not exp[6, BIG + 3, 0] and exp[7, BIG + 3, 0]                         # m_r - 1 bases, m_r bases
    assert exp[8, BIG + 4, 0] and exp[9, BIG + 5, 0] and not exp[10, BIG + 6].any()
    assert [len(q) for q in w.seqs[BIG + 7:BIG + 10]] == [3, 10, 23]
    assert not exp[11, BIG + 7].any() and not exp[11, BIG + 8].any() and exp[11, BIG + 9, 0]
    assert exp[2, BIG + 10, 0] and not exp[GAP_REF, BIG + 11].any()
    assert exp[TWIN_A, BIG + 12, 0] and exp[TWIN_B, BIG + 12, 0]
    assert exp[WIDE_A, BIG + 13, 0] and exp[WIDE_B, BIG + 13, 0] and len(w.seqs) == BIG + 14
    assert all(exp[r, BIG, 0] for r in PLANTED)
    # ... and nothing but what was planted: 21 pairs, on both strands when the references' reverse complements are indexed
    assert exp.sum() == (42 if w.rc else 21), np.argwhere(exp)


@pytest.mark.parametrize("prob", PROBS)
def test_every_bit_is_the_contract_and_covers_the_walk(w31, prob):
    w = w31
    exp = expected(w, prob)
    got = w.rs.candidates(w.seqs, prob, host=True)
    assert got.shape == exp.shape
    assert np.array_equal(got, exp), np.argwhere(got != exp)[:10]
    need = max_ms(w) >= np.array(w.wr[prob])[:, None, None]
    need[[r for r in range(len(w.refs)) if r not in w.packed]] = False
    assert not (need & ~got).any(), np.argwhere(need & ~got)[:10]
    assert need.any()
    for strands in (1, 2):
        one = w.rs.candidates(w.seqs, prob, strands=strands, host=True)
        assert np.array_equal(one[:, :, strands - 1], exp[:, :, strands - 1]) and not one[:, :, 2 - strands].any()


def test_the_tables_figures(w31):
    w = w31
    entries = sum(len(st) for r in w.packed for st in w.stretches[r])
    assert w.rs.prefilter_bytes() == 4 * (4 ** SEED_MIN + 1) + 12 * entries
    # a set whose 20 kbp references take the single-index route: no entries for them, and no bit
    own = world(w.k, w.rc, wide_rows=refset.MAX_ROWS)
    assert own.rs.route(WIDE_A) == own.rs.route(WIDE_B) == refset.ROUTE_INDEX and WIDE_A not in own.packed
    fewer = sum(len(st) for r in own.packed for st in own.stretches[r])
    assert fewer < entries - 39000 * (2 if w.rc else 1) and own.rs.prefilter_bytes() == 4 * (4 ** SEED_MIN + 1) + 12 * fewer
    for prob in (1e-7, 0.5):
        got = own.rs.candidates(own.seqs, prob, host=True)
        assert np.array_equal(got, expected(own, prob))
        assert not got[[WIDE_A, WIDE_B, SHORT_REF]].any()


def test_build_opts_without_prefilter_is_build_wide(w31):
    w = w31
    L = kbo_amd.lib()
    raw = [r.tobytes() for r in w.refs]
    arr = (C.c_char_p * len(raw))(*raw)
    lens = (C.c_size_t * len(raw))(*[len(r) for r in raw])
    co = kbo_amd.BuildOpts(k=w.k, add_revcomp=w.rc, num_threads=2)._to_c()
    h = C.c_void_p()
    ro = _capi.RefsetOpts(refset.WIDE_MAX_ROWS, 0)
    kbo_amd.check(L.kbo_refset_build_opts(arr, lens, len(raw), C.byref(co), C.byref(ro), C.byref(h)))
    rs = refset.RefSet(h)
    assert not rs.has_prefilter and rs.prefilter_bytes() == 0
    for r in range(len(w.refs)):
        assert rs.status(r) == w.plain.status(r) and rs.route(r) == w.plain.route(r) and rs.n_kmers(r) == w.plain.n_kmers(r)
        if r in w.packed:
            assert np.array_equal(rs.form(r), w.plain.form(r)) and np.array_equal(rs.form(r), w.rs.form(r))
    # NULL options: kbo_refset_build
    h2 = C.c_void_p()
    kbo_amd.check(L.kbo_refset_build_opts(arr, lens, len(raw), C.byref(co), None, C.byref(h2)))
    dflt = refset.RefSet(h2)
    assert not dflt.has_prefilter and dflt.route(WIDE_A) == refset.ROUTE_INDEX


def test_argument_errors_need_no_device(w31):
    w = w31
    L = kbo_amd.lib()
    raw = [w.refs[0].tobytes()]
    arr = (C.c_char_p * 1)(*raw)
    lens = (C.c_size_t * 1)(len(raw[0]))
    co = kbo_amd.BuildOpts(k=w.k)._to_c()
    h = C.c_void_p()
    for wide, pre in ((refset.MAX_ROWS, 2), (refset.MAX_ROWS, -1), (refset.MAX_ROWS - 1, 1), (refset.WIDE_MAX_ROWS + 1, 0)):
        ro = _capi.RefsetOpts(wide, pre)
        assert L.kbo_refset_build_opts(arr, lens, 1, C.byref(co), C.byref(ro), C.byref(h)) == E_BAD_ARG and not h.value
    ro = _capi.RefsetOpts(refset.MAX_ROWS, 1)
    assert L.kbo_refset_build_opts(arr, lens, 1, C.byref(co), C.byref(ro), None) == E_BAD_ARG
    assert L.kbo_refset_build_opts(None, lens, 1, C.byref(co), C.byref(ro), C.byref(h)) == E_BAD_ARG
    assert L.kbo_refset_has_prefilter(None) == 0 and L.kbo_refset_prefilter_bytes(None) == 0

    q = np.frombuffer(b"ACGTACGTACGTAC", dtype=np.uint8).copy()
    off = np.array([0, 10, 14], dtype=np.uint64)
    bits = np.zeros(len(w.refs), dtype=np.uint32)
    for f in (L.kbo_refset_candidates_host, L.kbo_refset_candidates):  # (both refuse before any work)
        def call(h=w.rs._h, concat=q.ctypes.data, offsets=off, n_seqs=2, prob=1e-7, strands=3, out=bits.ctypes.data):
            return f(h, concat, offsets.ctypes.data if offsets is not None else None, n_seqs, prob, strands, out, None)
        assert call(h=None) == E_BAD_ARG and call(h=w.plain._h) == E_BAD_ARG  # a set without a prefilter
        assert call(concat=None) == E_BAD_ARG and call(offsets=None) == E_BAD_ARG and call(out=None) == E_BAD_ARG
        for strands in (0, 4, -1):
            assert call(strands=strands) == E_BAD_ARG
        for prob in (0.0, 1.5, -1e-7):
            assert call(prob=prob) == E_BAD_ARG
        assert call(prob=1.0) == E_THRESHOLD_LE_1
        assert call(offsets=np.array([0, 12, 14], dtype=np.uint64)) == E_LEN_LE_2
        assert call(offsets=np.array([0, 12, 8], dtype=np.uint64)) == E_BAD_ARG
        assert call(offsets=np.array([0, 1 << 31], dtype=np.uint64), n_seqs=1) == E_UNSUPPORTED
    assert L.kbo_refset_candidates_host(w.rs._h, q.ctypes.data, off.ctypes.data, 2, 1e-7, 3, bits.ctypes.data, None) == 0
    assert L.kbo_set_refset_prefilter_max_bits(0) == 0


def test_the_screen_by_brute_force_under_sanitizers(tmp_path):
    """tools/refset_screen_check.cpp: the seed of every position and the bucket scan, through an accessor that checks every index,
    against sets of m-mers for every m of KBO_REFSET_SEED_MIN .. KBO_REFSET_SEED_MAX"""
    exe = str(tmp_path / "refset_screen_check")
    subprocess.run(["c++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I",
                    os.path.join(ROOT, "kbo_amd", "csrc"), os.path.join(ROOT, "tools", "refset_screen_check.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    m = re.search(r"(\d+) seeds, (\d+) cases agree, (\d+) marked", run.stdout)
    assert m and int(m.group(2)) == 12 * (SEED_MAX - SEED_MIN + 1) * 8 and 0 < int(m.group(3)) < int(m.group(2))
