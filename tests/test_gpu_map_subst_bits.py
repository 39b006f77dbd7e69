"""map_reads_kernel's stage 3 with the bit per text position that settles a lone substitution (kbo_amd/csrc/map_subst.hpp):
an eligible mismatch - no junction, a read on one diagonal, no other list entry within order - 1 bases - asks one word of the copy's
bitmap; a set bit answers all of its windows "absent", a clear one sends them to the depth table.  Only a wrongly set bit, a wrong key
(diagonal + base) or a wrongly eligible mismatch could change a character, so every case compares every byte with the oracle.

The genome (45 kbp, k = 31) holds six stretches of 1 - 2 kbp with a copy each that differs by a substitution every 25 - 60 bases: around
those differences the text's one-base neighbours ARE in the index - dirty positions, computed here on the host with numpy from the
definition.  The cases: substitutions at dirty and at clean positions placed at the read's edges for six read lengths; two substitutions
order - 2 .. order + 1 apart in the three combinations of dirty and clean; one insertion or deletion of 1 - 3 bases with a substitution
order - 1, order and order + 2 bases to either side, also inside runs of equal bases, where the cut merges with a mismatch (a wrong
diagonal would key the wrong bit); an index of 12 short contigs and a long one with substitutions next to contig starts and ends and
reads across two contigs; a call at another threshold, which must run without the bitmap; a copy made under KBO_SUBST_BITS=0 beside one
made without it; a table of 16 bases (the kernel's 64-bit keys).  Each goes through the character form with and without
relative_to_ref and kbo::find's run counts at documented buffer sizes between guard bands (test_gpu_map_default_line._run), the
summary form, and the packed forms (words in / bytes out, words in / words out)."""
import os

import numpy as np
import pytest

import kbo_amd
from kbo_amd import batch, derandomize, synth
from gpu_helpers import threads
from test_gpu_map_default_line import Expected, _dev, _first_difference, _run

pytestmark = pytest.mark.gpu

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
K = 31
LENGTHS = ("3", "thr", "thr+1", "31", "150", "160")
CASES = ["edges_clean", "edges_dirty", "two_substitutions", "indel_and_substitution"]


def _other(base, step):
    return ACGT[(int(np.searchsorted(ACGT, base)) + step) % 4]


def _genome():
    rng = np.random.default_rng(9_2026)
    g = synth.genome(45_000, seed=77).copy()
    for i in range(6):
        src, n = 2_000 + 7_000 * i, int(rng.integers(1_000, 2_001))
        dst = src + 3_000
        g[dst:dst + n] = g[src:src + n]
        p = dst + int(rng.integers(25, 61))
        while p < dst + n:
            g[p] = _other(g[p], int(rng.integers(1, 4)))
            p += int(rng.integers(25, 61))
    return g


def _offsets(order, thr, anch):
    """map_subst.hpp: window_step, window_used, window_offset"""
    cov = thr - order if anch else thr - order + 2
    return sorted({min(i * cov, order - 1) for i in range(4) if i == 0 or (i - 1) * cov < order - 1})


def _dirty(contigs, order, thr, anch):
    """per contig: True where a one-base neighbour of one of the proof's windows around the position is in the index (every string
    of `order` bases of any contig counts as in it), or where the position is within order - 1 bases of the contig's ends"""
    codes = [np.searchsorted(ACGT, c).astype(np.int64) for c in contigs]

    def keys(c):  # key[e] of the window ending at e >= order - 1
        k = np.zeros(len(c), dtype=np.int64)
        for j in range(order):
            k[order - 1:] += c[order - 1 - j:len(c) - j] << (2 * j)
        return k
    all_keys = np.unique(np.concatenate([keys(c)[order - 1:] for c in codes]))
    out = []
    for c in codes:
        k, n = keys(c), len(c)
        d = np.ones(n, dtype=bool)
        inner = np.arange(order - 1, n - (order - 1))
        bad = np.zeros(len(inner), dtype=bool)
        for o in _offsets(order, thr, anch):
            for step in (1, 2, 3):
                bad |= np.isin(k[inner + o] ^ ((c[inner] ^ ((c[inner] + step) % 4)) << (2 * o)), all_keys)
        d[inner] = bad
        out.append(d)
    return out


def _placements(length, order):
    at = (0, 1, 2, order - 2, order - 1, order, length // 2, length - order - 1, length - order, length - order + 1, length - 2, length - 1)
    return sorted({m for m in at if 0 <= m < length})


def _edge_reads(g, positions, order, thr):
    reads = []
    for p in positions:
        for name in LENGTHS:
            length = {"thr": thr, "thr+1": thr + 1}.get(name) or int(name)
            for m in _placements(length, order):
                for step in (1, 2, 3):
                    r = g[p - m:p - m + length].copy()
                    r[m] = _other(r[m], step)
                    reads.append(r)
    return reads


def _pairs(dirty, a_dirty, b_dirty, d, rng, n):
    lo, hi = 400, len(dirty) - 400
    ok = np.flatnonzero((dirty[lo:hi - d] == a_dirty) & (dirty[lo + d:hi] == b_dirty)) + lo
    assert len(ok), "no pair of positions %d apart that is %s / %s" % (d, a_dirty, b_dirty)
    return rng.choice(ok, min(n, len(ok)), replace=False)


def _cases(g, dirty, order, thr):
    rng = np.random.default_rng(20_28)
    inner = np.arange(400, len(g) - 400)
    c = {}
    c["edges_clean"] = _edge_reads(g, rng.choice(inner[~dirty[inner]], 3, replace=False), order, thr)
    c["edges_dirty"] = _edge_reads(g, rng.choice(inner[dirty[inner]], 3, replace=False), order, thr)
    two = []
    for d in (order - 2, order - 1, order, order + 1):
        for a_dirty, b_dirty in ((True, False), (False, True), (False, False), (True, True)):
            for p in _pairs(dirty, a_dirty, b_dirty, d, rng, 4):
                for step in (1, 2, 3):
                    for m in (60, 3, 149 - d - 3):
                        r = g[p - m:p - m + 150].copy()
                        r[m], r[m + d] = _other(r[m], step), _other(r[m + d], 1 + step % 3)
                        two.append(r)
    c["two_substitutions"] = two
    # one insertion / deletion (tools/exp_indel3.py's generator, one read at a time) and a substitution beside it; the text positions
    # of the break: random ones, dirty ones and ones inside a run of three equal bases (the cut then merges with a mismatch or moves)
    runs = np.flatnonzero((g[:-2] == g[1:-1]) & (g[1:-1] == g[2:]))
    runs = runs[(runs > 400) & (runs < len(g) - 400)]
    near_dirty = inner[dirty[inner]]
    indel = []
    for kind, where in (("any", rng.choice(inner, 4)), ("run", rng.choice(runs, 6)), ("dirty", rng.choice(near_dirty, 4))):
        for t in where:
            for pos in (25, 75, 125):
                for size in (1, 2, 3):
                    for ins in (False, True):
                        start = int(t) - pos
                        i = np.arange(150)
                        shift = np.where(i >= pos, -np.minimum(size, i - pos) if ins else size, 0)
                        base = g[start + i + shift]
                        if ins:
                            base[pos:pos + size] = g[t] if kind == "run" else ACGT[rng.integers(0, 4, size)]
                        for off in (order - 1, order, order + 2):
                            for m in (pos - off, pos + size - 1 + off):
                                r = base.copy()
                                r[m] = _other(r[m], 1 + (m + size) % 3)
                                indel.append(r)
    sel = rng.permutation(len(indel))[:1_900]
    c["indel_and_substitution"] = [indel[i] for i in sorted(sel)]
    for name, reads in c.items():
        assert 0 < len(reads) <= 2_000, (name, len(reads))
    return c


def _thresholds(sbwt):
    order = int(sbwt.depth_table_order())
    thr = int(derandomize.random_match_threshold(K, sbwt.n_kmers(), 4, 1e-7))
    anch = sbwt.device_layout()["anchor_bytes"] > 0 and thr > order
    return order, thr, anch


def _make(oracle, contigs, order=0, anchors=-1, bits=True):
    L = kbo_amd.lib()
    L.kbo_set_depth_table(order)
    L.kbo_set_depth_table_anchors(anchors)
    if not bits:
        os.environ["KBO_SUBST_BITS"] = "0"
    try:
        sbwt, _ = kbo_amd.build([c.tobytes() for c in contigs], kbo_amd.BuildOpts(k=K, num_threads=threads()))
        sbwt.to_device(-1)
        # (a copy makes its plan structures with the first batch that pays for them: make it now, under this environment)
        r = np.concatenate([contigs[-1][100:250]] * 64)
        batch.matches_batch(sbwt, r, np.arange(65, dtype=np.uint64) * 150)
    finally:
        os.environ.pop("KBO_SUBST_BITS", None)
        L.kbo_set_depth_table(0)
        L.kbo_set_depth_table_anchors(-1)
    assert sbwt.depth_table_order() > 0 and (not order or sbwt.depth_table_order() == order)
    return sbwt


@pytest.fixture(scope="module")
def world(oracle):
    g = _genome()
    sbwt = _make(oracle, [g])
    ora = oracle.Index.build([g.tobytes()], k=K)
    order, thr, anch = _thresholds(sbwt)
    dirty = _dirty([g], order, thr, anch)[0]
    return {"sbwt": sbwt, "ora": ora, "oracle": oracle, "g": g, "dirty": dirty, "order": order, "thr": thr, "anch": anch,
            "cases": {n: (r, False) for n, r in _cases(g, dirty, order, thr).items()}, "expected": {}}


def _expected(world, name):
    if name not in world["expected"]:
        world["expected"][name] = Expected(world["oracle"], world["ora"], world["cases"][name][0], False)
    return world["expected"][name]


def _stats(sbwt, concat, offsets, prob=1e-7):
    """the batch through kbo_map_batch_dev with the kernel's counting instantiation -> (characters, plan stats)"""
    import torch
    L = kbo_amd.lib()
    L.kbo_set_plan(1, 0, 0)
    L.kbo_set_plan_stats(1)
    try:
        dev = batch.DeviceBatch(sbwt, concat, offsets, device=_dev(), max_error_prob=prob, format=False, want_ms=False)
        dev.run()
        torch.cuda.synchronize()
        assert dev.fused
        return dev.chars.cpu().numpy()[:int(offsets[-1])], dev.plan_stats()
    finally:
        L.kbo_set_plan_stats(0)


def _other_forms(sbwt, e, what):
    """the summary form (reads as bytes and as words) and the packed forms, against the oracle's characters"""
    want = batch.summary_of_chars(e.chars, e.offsets)
    for packed in (False, True):
        got = batch.summary_batch(sbwt, (e.concat, e.offsets), packed=packed)
        bad = np.flatnonzero((got != want).any(axis=1))
        assert len(bad) == 0, "%s, summary (packed = %s): read %d: %s, expected %s" % (what, packed, bad[0], got[bad[0]], want[bad[0]])
    words, pos, byt = batch.pack_reads(e.concat, e.offsets)
    kbo_amd.lib().kbo_set_plan(1, 0, 0)
    _first_difference(batch.unpack_matches(batch.matches_batch_packed(sbwt, words, e.offsets, pos, byt), e.offsets), e.chars, e.keep, e.offsets,
                      what + ", words in / words out")
    runs = batch.matches_batch_sparse(sbwt, words, e.offsets, pos, byt)
    _first_difference(batch.expand_sparse(runs, e.offsets), e.chars, e.keep, e.offsets, what + ", words in / bytes out")


def test_the_fixture_has_dirty_and_clean_positions_and_the_kernel_meets_both(world):
    """conditions on the fixture: dirty positions exist (the planted near-copies), and a batch of substitutions at dirty and at clean
    positions has at least one mismatch the bitmap settled and at least one it sent to the table"""
    dirty, g = world["dirty"], world["g"]
    inner = np.arange(400, len(g) - 400)
    assert 0 < int(dirty[inner].sum()) < len(inner)
    e = _expected(world, "edges_clean")
    d = _expected(world, "edges_dirty")
    concat = np.concatenate([e.concat, d.concat])
    offsets = np.concatenate([e.offsets, d.offsets[1:] + e.offsets[-1]])
    chars, st = _stats(world["sbwt"], concat, offsets)
    print(st)
    _first_difference(chars, np.concatenate([e.chars, d.chars]), np.concatenate([e.keep, d.keep]), offsets, "edges, counting form")
    assert st["subst_clean"] >= 1 and st["subst_bits"] - st["subst_clean"] >= 1, st


@pytest.mark.parametrize("fmt", [False, True], ids=["matches", "relative_to_ref"])
@pytest.mark.parametrize("name", CASES)
def test_every_byte_against_the_oracle(world, name, fmt):
    _run(world, name, fmt, find=False)


@pytest.mark.parametrize("name", CASES)
def test_find_characters_and_runs(world, name):
    _run(world, name, False, find=True)


@pytest.mark.parametrize("name", CASES)
def test_summary_and_packed_forms(world, name):
    _other_forms(world["sbwt"], _expected(world, name), name)


def test_another_threshold_runs_without_the_bitmap(world):
    """an error probability that moves the threshold: the bitmap speaks for the default's windows only, the launch gets none"""
    prob = 1e-9
    assert derandomize.random_match_threshold(K, world["sbwt"].n_kmers(), 4, prob) != world["thr"]
    for name in ("edges_dirty", "two_substitutions"):
        e = _expected(world, name)
        want = world["ora"].matches_batch(e.concat, e.offsets, prob, n_threads=threads())
        chars, st = _stats(world["sbwt"], e.concat, e.offsets, prob)
        _first_difference(chars, want, e.keep, e.offsets, name + ", another threshold")
        assert st["subst_bits"] == 0 and st["subst_clean"] == 0 and st["tab_lookups"] > 0, st


def test_a_copy_without_the_bitmap_beside_one_with_it(world, oracle):
    """KBO_SUBST_BITS=0 is read when a copy's plan structures are made: both kinds in one process, the same characters, fewer table
    look-ups with the bitmap"""
    plain = _make(oracle, [world["g"]], bits=False)
    assert plain.device_layout()["cover_bytes"] < world["sbwt"].device_layout()["cover_bytes"]
    for name in CASES:
        e = _expected(world, name)
        with_bits, st_with = _stats(world["sbwt"], e.concat, e.offsets)
        without, st_without = _stats(plain, e.concat, e.offsets)
        _first_difference(with_bits, e.chars, e.keep, e.offsets, name + ", with the bitmap")
        _first_difference(without, e.chars, e.keep, e.offsets, name + ", without the bitmap")
        assert st_without["subst_bits"] == 0, st_without
        # (a read with an insertion or a deletion lies on two diagonals: none of its mismatches is eligible)
        assert st_with["subst_bits"] > 0 or name == "indel_and_substitution", st_with
        if name == "edges_clean":
            assert st_with["tab_lookups"] < st_without["tab_lookups"], (st_with, st_without)


def test_a_table_of_16_bases(world, oracle):
    """the kernel's instantiation with 64-bit keys (NP = 18; test_gpu_map_reads.py's order 16, no anchors: the direct form at this
    threshold): dirty positions by that order's windows"""
    g = world["g"]
    sbwt = _make(oracle, [g], order=16, anchors=0)
    order, thr, anch = _thresholds(sbwt)
    assert order == 16 and not anch
    dirty = _dirty([g], order, thr, anch)[0]
    rng = np.random.default_rng(5)
    inner = np.arange(400, len(g) - 400)
    reads = _edge_reads(g, list(rng.choice(inner[~dirty[inner]], 1)) + list(rng.choice(inner[dirty[inner]], 1)), order, thr)
    reads += world["cases"]["two_substitutions"][0][:300] + world["cases"]["indel_and_substitution"][0][:600]
    w = {"sbwt": sbwt, "ora": world["ora"], "oracle": oracle, "cases": {"order_16": (reads, False)}, "expected": {}}
    for fmt in (False, True):
        _run(w, "order_16", fmt, find=False)
    _run(w, "order_16", False, find=True)
    e = w["expected"]["order_16"]
    _other_forms(sbwt, e, "order 16")
    chars, st = _stats(sbwt, e.concat, e.offsets)
    _first_difference(chars, e.chars, e.keep, e.offsets, "order 16, counting form")
    assert st["subst_clean"] >= 1 and st["subst_bits"] - st["subst_clean"] >= 1, st


def test_twelve_short_contigs(oracle):
    """12 contigs of 300 - 500 bases and one of 45 kbp (path starts inside the text): substitutions within order - 1 bases of a contig's
    start and end - the windows there reach a mark: not clean -, deeper inside, and in reads across two contigs"""
    rng = np.random.default_rng(8_2027)
    short = [synth.genome(int(n), seed=700 + i) for i, n in enumerate(rng.integers(300, 501, 12))]
    contigs = short + [_genome()]
    sbwt = _make(oracle, contigs)
    ora = oracle.Index.build([c.tobytes() for c in contigs], k=K)
    order, thr, anch = _thresholds(sbwt)
    reads = []
    for c in short:
        for length in (thr + 1, 100, 150):
            for m in sorted({0, 1, order - 2, order - 1, order, order + 1, length // 2}):
                for step in (1, 2, 3):
                    head, tail = c[:length].copy(), c[len(c) - length:].copy()
                    head[m] = _other(head[m], step)
                    tail[length - 1 - m] = _other(tail[length - 1 - m], step)
                    reads += [head, tail]
    for ia in range(12):
        ib = (ia + 5) % 12
        for s in (15, 75, 134):
            for m in (s - order, s - 1, s, s + order - 1, s + order):
                r = np.concatenate([short[ia][len(short[ia]) - s:], short[ib][:150 - s]])
                r[m] = _other(r[m], 1 + m % 3)
                reads.append(r)
    sel = rng.permutation(len(reads))[:2_000]
    w = {"sbwt": sbwt, "ora": ora, "oracle": oracle, "cases": {"contigs": ([reads[i] for i in sorted(sel)], False)}, "expected": {}}
    for fmt in (False, True):
        _run(w, "contigs", fmt, find=False)
    _run(w, "contigs", False, find=True)
    e = w["expected"]["contigs"]
    _other_forms(sbwt, e, "contigs")
    chars, st = _stats(sbwt, e.concat, e.offsets)
    _first_difference(chars, e.chars, e.keep, e.offsets, "contigs, counting form")
    assert st["subst_bits"] >= 1, st
