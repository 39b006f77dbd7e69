"""kbo_map_batch_opts / kbo_fill_gaps_batch on the device (gap_kernels.hip + map_batch_opts.cpp): every sequence of a batch
bit-equal to what kbo_map / kbo_fill_gaps give for it alone and to the oracle's literal reference restatement, its status
equal to kbo_map's return code; the host fallback routes (no path cover, frequent path starts) equal as well."""
import numpy as np
import pytest

import kbo_amd
from kbo_amd import batch, derandomize, gap_filling, synth

from gpu_helpers import threads

pytestmark = pytest.mark.gpu

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def _batch(seqs):
    seqs = [bytes(s) for s in seqs]
    off = np.zeros(len(seqs) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    return np.frombuffer(b"".join(seqs) or b"\0", dtype=np.uint8)[:int(off[-1])].copy(), off


def _seqs(concat, off):
    return [concat[int(off[i]):int(off[i + 1])].tobytes() for i in range(len(off) - 1)]


def _fill_one(sbwt, seq, t, p):
    try:
        return 0, "".join(gap_filling.fill_gaps_from_sequences(seq, sbwt, t, p)).encode("latin-1")
    except kbo_amd.KboError as e:
        return e.code, None


def _map_one(sbwt, seq, mo):
    try:
        return 0, kbo_amd.map(seq, sbwt, None, mo)
    except kbo_amd.KboError as e:
        return e.code, None


def _repeat_genome(n, seed):
    """a genome with tandem repeats and copied stretches: intervals of more than one row occur"""
    rng = np.random.default_rng(seed)
    g = synth.genome(n, seed=seed)
    for _ in range(60):
        a = int(rng.integers(0, n - 2000))
        unit = g[a:a + int(rng.integers(2, 40))].copy()
        L = int(rng.integers(100, 1200))
        b = int(rng.integers(0, n - L))
        g[b:b + L] = np.resize(unit, L)
    for _ in range(40):
        a, b, L = int(rng.integers(0, n - 3000)), int(rng.integers(0, n - 3000)), int(rng.integers(200, 3000))
        g[b:b + L] = g[a:a + L]
    return g


def _check_fill_batch(sbwt, concat, off, t, p, ora=None, n_oracle=0):
    out, st = batch.fill_gaps_batch(sbwt, concat, off, t, p)
    stats = batch.fill_gaps_stats()
    for i, s in enumerate(_seqs(concat, off)):
        code, exp = _fill_one(sbwt, s, t, p)
        assert st[i] == code, (i, len(s), st[i], code)
        if code == 0:
            got = out[int(off[i]):int(off[i + 1])].tobytes()
            assert got == exp, (i, len(s), [j for j in range(len(s)) if got[j] != exp[j]][:10])
            if ora is not None and i < n_oracle:
                d, _, _ = ora.matching_statistics(s)
                k = sbwt.k()
                tr = ora_mod.translate_ms_vec(ora_mod.derandomize_ms_vec(d, k, t), k, t)
                assert ora.fill_gaps(tr, s, t, p) == got, i
    return stats


ora_mod = None


@pytest.fixture(autouse=True)
def _oracle_module(oracle):
    global ora_mod
    ora_mod = oracle


def test_fill_gaps_goldens_as_batches(golden):  # gap_filling.rs:419-441, 641-922
    for g in golden["fill_gaps"]:
        sbwt, _ = kbo_amd.build([g["query"]], kbo_amd.BuildOpts(k=g["k"], build_select=True))
        t = g["threshold"]
        if t is None:
            t = derandomize.random_match_threshold(sbwt.k(), sbwt.n_kmers(), 4, g["max_err_prob"])
        concat, off = _batch([g["reference"].encode()])
        out, st = batch.fill_gaps_batch(sbwt, concat, off, t, g["max_err_prob"])
        assert st[0] == 0 and out.tobytes().decode() == g["expected"], g["src"]


def test_map_goldens_with_refinement(golden):  # lib.rs:647-717
    n = 0
    for g in golden["map"]:
        if not (g["fill_gaps"] or g["call_variants"]):
            continue
        opts = kbo_amd.BuildOpts(k=g["k"], build_select=True)
        sbwt, _ = kbo_amd.build(g["query_seqs"], opts)
        mo = kbo_amd.MapOpts(max_error_prob=g["max_error_prob"], fill_gaps=g["fill_gaps"], call_variants=g["call_variants"],
                             format=g["format"], sbwt_build_opts=opts)
        concat, off = _batch([g["ref_seq"].encode()])
        out, st = batch.map_batch_opts(sbwt, concat, off, mo)
        assert st[0] == 0 and out.tobytes().decode() == g["expected"], g["src"]
        n += 1
    assert n > 0


@pytest.mark.parametrize("k", [15, 31, 63])
def test_random_fill_gaps_parity(oracle, k):
    g = _repeat_genome(1_000_000, 900 + k)
    sbwt, _ = kbo_amd.build([g], kbo_amd.BuildOpts(k=k, num_threads=threads()))
    ora = oracle.Index.build([g.tobytes()], k=k)
    concat, off = synth.variant_contigs(g, 2000, 200, 20_000, sub_rate=0.01, indel_every=1500, insert_frac=0.1,
                                        n_rate=0.0005, seed=77 + k)
    t = derandomize.random_match_threshold(k, sbwt.n_kmers(), 4, 1e-7)
    stats = _check_fill_batch(sbwt, concat, off, t, 1e-7, ora=ora, n_oracle=150)
    print("k", k, "stats", stats)
    assert stats[0] > 5000
    assert stats[1] >= 0.95 * stats[0], stats


def test_fallback_routes(oracle):
    # (a) no path cover for this handle: every sequence with a gap whose candidate row has to be spelled is redone on the host
    # (a gap without any single-row context to its right needs no spelling and is still finished on the device)
    g = _repeat_genome(300_000, 5)
    sbwt, _ = kbo_amd.build([g], kbo_amd.BuildOpts(k=31, num_threads=threads()))
    concat, off = synth.variant_contigs(g, 300, 200, 5000, insert_frac=0.2, seed=3)
    t = derandomize.random_match_threshold(31, sbwt.n_kmers(), 4, 1e-7)
    on = _check_fill_batch(sbwt, concat, off, t, 1e-7)
    sbwt.set_opts(plan=0)
    off_stats = _check_fill_batch(sbwt, concat, off, t, 1e-7)
    assert off_stats[0] == on[0] > 0 and off_stats[1] < 0.05 * on[1] and off_stats[2] > on[2]
    # (b) 3 000 short contigs: path starts are frequent
    rng = np.random.default_rng(8)
    contigs = [ACGT[rng.integers(0, 4, int(rng.integers(40, 200)))].tobytes() for _ in range(3000)]
    sbwt2, _ = kbo_amd.build(contigs, kbo_amd.BuildOpts(k=31, num_threads=threads()))
    qs = []
    for i in range(400):
        a, b = contigs[i], contigs[i + 1]
        q = bytearray(a + ACGT[rng.integers(0, 4, int(rng.integers(1, 30)))].tobytes() + b)
        for p in rng.integers(0, len(q), 2):
            q[p] = b"ACGT"[(b"ACGT".index(q[p]) + 1) % 4]
        qs.append(bytes(q))
    c2, o2 = _batch(qs)
    t2 = derandomize.random_match_threshold(31, sbwt2.n_kmers(), 4, 1e-7)
    st2 = _check_fill_batch(sbwt2, c2, o2, t2, 1e-7)
    print("short contigs stats", st2, "no cover stats", off_stats)


@pytest.mark.parametrize("p", [1e-3, 1e-7])
def test_map_batch_opts_all_combinations(oracle, p):
    g = _repeat_genome(400_000, 21)
    opts = kbo_amd.BuildOpts(k=31, build_select=True, num_threads=threads())
    sbwt, _ = kbo_amd.build([g], opts)
    ora = oracle.Index.build([g.tobytes()], k=31)
    concat, off = synth.variant_contigs(g, 500, 100, 3000, insert_frac=0.1, seed=int(1 / p) % 1000)
    seqs = _seqs(concat, off)
    for fill in (False, True):
        for call in (False, True):
            for fmt in (False, True):
                mo = kbo_amd.MapOpts(max_error_prob=p, fill_gaps=fill, call_variants=call, format=fmt, sbwt_build_opts=opts)
                out, st = batch.map_batch_opts(sbwt, concat, off, mo)
                for i, s in enumerate(seqs):
                    code, exp = _map_one(sbwt, s, mo)
                    assert st[i] == code, (fill, call, fmt, i)
                    got = out[int(off[i]):int(off[i + 1])].tobytes()
                    assert code != 0 or got == exp, (fill, call, fmt, i)
                    if code == 0 and i < 40:
                        assert ora.map(s, 31, p, fill, call, fmt) == got, (fill, call, fmt, i)
                if not fill and not call:
                    assert np.array_equal(out, batch.map_batch(sbwt, concat, off, p, fmt))


def test_status_per_sequence():
    g = _repeat_genome(200_000, 31)
    opts = kbo_amd.BuildOpts(k=31, build_select=True, num_threads=threads())
    sbwt, _ = kbo_amd.build([g], opts)
    good_c, good_o = synth.variant_contigs(g, 60, 300, 3000, seed=4)
    good = _seqs(good_c, good_o)
    rng = np.random.default_rng(2)
    foreign = [ACGT[rng.integers(0, 4, 500)].tobytes(), ACGT[rng.integers(0, 4, 80)].tobytes()]
    bad = [b"", b"A", b"AC", g[1000:1010].tobytes(), b"ACG"] + foreign
    mixed = []
    for i, s in enumerate(good):
        mixed.append(s)
        if i < len(bad):
            mixed.append(bad[i])
    for mo in (kbo_amd.MapOpts(sbwt_build_opts=opts), kbo_amd.MapOpts(call_variants=False, sbwt_build_opts=opts),
               kbo_amd.MapOpts(fill_gaps=False, call_variants=False, sbwt_build_opts=opts)):
        c, o = _batch(mixed)
        out, st = batch.map_batch_opts(sbwt, c, o, mo)
        gc, go = _batch(good)
        gout, gst = batch.map_batch_opts(sbwt, gc, go, mo)
        assert (gst == 0).all()
        for i, s in enumerate(mixed):
            code, exp = _map_one(sbwt, s, mo)
            assert st[i] == code, (i, len(s), st[i], code)
            if code == 0:
                assert out[int(o[i]):int(o[i + 1])].tobytes() == exp
        # the good ones are unaffected by the bad ones between them
        pos = [i for i in range(len(mixed)) if any(mixed[i] is x for x in good)]
        assert len(pos) == len(good)
        for gi, i in enumerate(pos):
            assert out[int(o[i]):int(o[i + 1])].tobytes() == gout[int(go[gi]):int(go[gi + 1])].tobytes()
    # fill_gaps_batch: the same rule against kbo_fill_gaps
    t = derandomize.random_match_threshold(31, sbwt.n_kmers(), 4, 1e-7)
    c, o = _batch(mixed)
    _check_fill_batch(sbwt, c, o, t, 1e-7)


def test_edges_and_slabs():
    L = kbo_amd.lib()
    g = _repeat_genome(300_000, 41)
    k = 31
    sbwt, _ = kbo_amd.build([g], kbo_amd.BuildOpts(k=k, num_threads=threads()))
    t = derandomize.random_match_threshold(k, sbwt.n_kmers(), 4, 1e-7)
    rng = np.random.default_rng(5)
    seqs = []
    base = g[10_000:12_000].copy()
    for s0 in (t, 2000 - t - 1, 2000 - t - 2, t + 1):
        s = base.copy()
        s[s0] = ACGT[(np.searchsorted(ACGT, s[s0]) + 1) % 4]
        seqs.append(s.tobytes())
    seqs.append(base[:1500].tobytes() + ACGT[rng.integers(0, 4, 500)].tobytes())  # a gap running to the end
    seqs.append(ACGT[rng.integers(0, 4, 300)].tobytes() + base[:1500].tobytes())   # ... and from the start
    seqs.append(base[:800].tobytes() + ACGT[rng.integers(0, 4, 100)].tobytes())    # adjacent gaps across a boundary
    seqs.append(ACGT[rng.integers(0, 4, 100)].tobytes() + base[800:1600].tobytes())
    c, o = _batch(seqs)
    _check_fill_batch(sbwt, c, o, t, 1e-7)
    # sequences longer than a slab: each its own slab
    lc, lo = synth.variant_contigs(g, 4, 90_000, 120_000, insert_frac=1.0, seed=9)
    lc = np.concatenate([lc, c])
    lo = np.concatenate([lo, lo[-1] + o[1:]])
    whole = batch.fill_gaps_batch(sbwt, lc, lo, t, 1e-7)
    L.kbo_set_slab_bytes(1 << 16)
    sl = batch.fill_gaps_batch(sbwt, lc, lo, t, 1e-7)
    assert np.array_equal(whole[0], sl[0]) and np.array_equal(whole[1], sl[1])
    _check_fill_batch(sbwt, lc, lo, t, 1e-7)


def test_c1_shape_batched(oracle):
    """test_c1_map_full_defaults_10kbp_vs_1mbp's construction, 200 times with other seeds, in one call"""
    g = synth.genome(1_000_000, seed=1234)
    opts = kbo_amd.BuildOpts(k=31, build_select=True, num_threads=threads())
    sbwt, _ = kbo_amd.build([g], opts)
    ora = oracle.Index.build([g.tobytes()], k=31)
    refs = []
    for seed in range(200):
        rng = np.random.default_rng(1000 + seed)
        a = int(rng.integers(0, 990_000))
        ref = bytearray(g[a:a + 10_000].tobytes())
        for p in sorted(rng.integers(100, 9900, 25)):
            ref[p] = b"ACGT"[(b"ACGT".index(ref[p]) + 1 + int(rng.integers(0, 3))) % 4]
        del ref[5000:5007]
        ref[7000:7000] = b"GATTACAGATTACA"
        refs.append(bytes(ref))
    c, o = _batch(refs)
    mo = kbo_amd.MapOpts(sbwt_build_opts=opts)
    out, st = batch.map_batch_opts(sbwt, c, o, mo)
    assert (st == 0).all()
    for i, ref in enumerate(refs):
        got = out[int(o[i]):int(o[i + 1])].tobytes()
        if i < 40:
            assert got == ora.map(ref, 31, 1e-7, True, True, True), i
        assert got == kbo_amd.map(ref, sbwt, None, mo), i
