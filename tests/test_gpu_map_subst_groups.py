"""map_reads_kernel with the clean groups next to the bit per text position (sub_group; kbo_amd/csrc/map_subst.hpp):
stage 2 loads the 8 bytes that hold the groups of the diagonal's window beside the text, the read's own lane settles every eligible
lone substitution whose group is clean, and stage 3 deals only what is left.  A mismatch settled early is one stage 3 would have
settled by the same rule, so every case compares every byte with the oracle - characters with and without relative_to_ref, kbo::find's
runs, summaries, both packed forms - and the counters say which way each mismatch went: subst_bits = eligible mismatches asked,
subst_clean = of those, settled, subst_groups = of those, settled in the owner lane.

What the counters must be is worked out here from what the copy itself holds, read back through kbo_index_plan_part: the text with its
marks (pc_tm), the seed positions (seed_pos), the bit per position (sub_clean) and the groups (sub_group).  _model() restates stage 1
(the first window of seed_d bases whose string ends one row only; else the first ambiguous one), stage 2's compare on that diagonal and
the rule of eligibility; a read that would enter stage 2b (no seed, a list too long, six mismatches in its first or last 16 bases) is
not modelled and is left out of the batches whose counters are compared exactly.  The genome is test_gpu_map_subst_bits.py's: 45 kbp with
six planted near-copies, around whose differences the dirty positions lie."""
import os

import numpy as np
import pytest

from kbo_amd import synth
from gpu_helpers import threads
from test_gpu_map_default_line import Expected, _first_difference, _run
from test_gpu_map_subst_bits import ACGT, K, _genome, _make, _other, _other_forms, _stats, _thresholds

pytestmark = pytest.mark.gpu

PAD = 192    # positions in front of text position 0 (map_subst.hpp kPad)
GROUP = 4    # positions a group (map_subst.hpp kGroup)
CAP = 64     # bases of a read in which stage 1 looks for its seed (plan_kernels.hip g_plan_cap)
LIST = 13    # entries of a read's list
LENGTHS = (3, 22, 23, 97, 128, 129, 150, 160)


class Copy:
    """what the device copy holds, by position q of the padded text (q = text position + PAD)"""

    def __init__(self, sbwt):
        tm, _ = sbwt.plan_part("pc_tm")
        sh = 2 * (15 - np.arange(16, dtype=np.uint32))
        self.base = ((tm[:, 0:1] >> sh) & 3).astype(np.uint8).reshape(-1)
        self.mark = ((tm[:, 1:2] >> sh) & 1).astype(bool).reshape(-1)
        self.units = len(tm)
        sp, info = sbwt.plan_part("seed_pos")
        self.seed_d, self.seed_pos = info[0], sp[:4 ** info[0]]
        cl, self.clean_info = sbwt.plan_part("sub_clean")
        self.clean_words = cl
        self.clean = np.unpackbits(cl.view(np.uint8), bitorder="little").astype(bool)
        gr, self.group_info = sbwt.plan_part("sub_group")
        self.group_bytes = gr.view(np.uint8)
        self.group = np.unpackbits(self.group_bytes, bitorder="little").astype(bool)
        self.text = ACGT[self.base].tobytes()  # (marked positions read as 'A': a match there is checked against the marks)

    def own(self, q):
        return bool(self.clean[q]) if q < len(self.clean) else False

    def grp(self, q):
        return bool(self.group[q // GROUP]) if q // GROUP < len(self.group) else False


def _first_seed(cp, read):
    """stage 1: q0 of the diagonal by the first window of seed_d bases whose string ends one row only, else by the first ambiguous one"""
    n, D = len(read), cp.seed_d
    code = np.searchsorted(ACGT, read).astype(np.int64)
    amb = None
    for e in range(D - 1, min(n, CAP), D):
        key = 0
        for c in code[e + 1 - D:e + 1]:
            key = (key << 2) | int(c)
        tp = int(cp.seed_pos[key])
        if tp == 0xFFFFFFFF:
            continue
        if not tp & 0x80000000:
            return tp - e + PAD
        if amb is None:
            amb = (tp & 0x7FFFFFFF) - e + PAD
    return amb


def _model(cp, read, order, thr):
    """-> None for a read that stage 2b would look at, else (q0 or None, [(m, eligible)]) of its list on the seed's diagonal"""
    n, D = len(read), cp.seed_d
    code = np.searchsorted(ACGT, read).astype(np.int64)
    q0 = _first_seed(cp, read)
    if q0 is None:
        return None if n >= 2 * D else (None, [])
    if q0 < 0 or q0 + n > len(cp.base):
        return None
    mm = np.flatnonzero((cp.base[q0:q0 + n] != code) | cp.mark[q0:q0 + n])
    dense = n >= 32 and (int((mm < 16).sum()) >= 6 or int((mm >= n - 16).sum()) >= 6)
    if n >= 2 * D and (len(mm) > LIST or dense):
        return None
    if len(mm) > LIST or n <= thr:
        return q0, []
    out = []
    for i, m in enumerate(mm):
        lone = (i == 0 or m - mm[i - 1] > order - 1) and (i + 1 == len(mm) or mm[i + 1] - m > order - 1)
        out.append((int(m), bool(lone)))
    return q0, out


def _predict(cp, reads, order, thr):
    """the reads the model speaks for, and the three counters of a batch of them"""
    kept, bits, clean, groups = [], 0, 0, 0
    for r in reads:
        got = _model(cp, r, order, thr)
        if got is None:
            continue
        kept.append(r)
        q0, entries = got
        for m, lone in entries:
            if lone:
                bits += 1
                clean += cp.own(q0 + m)
                groups += cp.grp(q0 + m)
    return kept, {"subst_bits": bits, "subst_clean": clean, "subst_groups": groups}


def _sub(r, at, step=1):
    r = r.copy()
    for i, m in enumerate(np.atleast_1d(at)):
        r[m] = _other(r[m], 1 + (step + i) % 3)
    return r


@pytest.fixture(scope="module")
def world(oracle):
    g = _genome()
    sbwt = _make(oracle, [g])
    ora = oracle.Index.build([g.tobytes()], k=K)
    order, thr, anch = _thresholds(sbwt)
    cp = Copy(sbwt)
    # where the genome lies in the text: a read's window is found by its bases (a stretch that crosses a path start is not found)
    return {"sbwt": sbwt, "ora": ora, "oracle": oracle, "g": g, "order": order, "thr": thr, "anch": anch, "cp": cp, "cases": {}, "expected": {}}


def _q_of(world, p):
    """position q of the padded text at which genome position p lies (by the 40 bases from p - 20 on), or None"""
    g, cp = world["g"], world["cp"]
    at = cp.text.find(g[p - 20:p + 20].tobytes())
    return None if at < 0 or cp.mark[at:at + 40].any() else at + 20


def _check(world, name, reads, exact=True, forms=True):
    """the batch against the oracle in every form; -> its counters (exact: the model's reads only, and its counters)"""
    cp, order, thr = world["cp"], world["order"], world["thr"]
    want = None
    if exact:
        n_all = len(reads)
        reads, want = _predict(cp, reads, order, thr)
        assert len(reads) * 10 >= n_all * 8, "%s: the model speaks for %d of %d reads only" % (name, len(reads), n_all)
    assert 0 < len(reads) <= 2_000, (name, len(reads))
    world["cases"][name] = (reads, False)
    for fmt in (False, True):
        _run(world, name, fmt, find=False)
    e = world["expected"][name]
    if forms:
        _run(world, name, False, find=True)
        _other_forms(world["sbwt"], e, name)
    chars, st = _stats(world["sbwt"], e.concat, e.offsets)
    print(name, {k: st[k] for k in ("mismatches", "subst_bits", "subst_clean", "subst_groups", "seed_extensions", "tab_lookups")}, want)
    _first_difference(chars, e.chars, e.keep, e.offsets, name + ", counting form")
    assert st["subst_groups"] <= st["subst_clean"] <= st["subst_bits"] <= st["mismatches"], st
    if want is not None:
        assert {k: st[k] for k in want} == want, (name, st, want)
    return st


def _positions(world, rng, kind, n):
    """genome positions whose text position is (kind) 'group': in a clean group, 'own': clean in a group that is not, 'dirty': not clean"""
    cp, g = world["cp"], world["g"]
    out = []
    for p in rng.permutation(np.arange(400, len(g) - 400)):
        q = _q_of(world, int(p))
        if q is None:
            continue
        k = "group" if cp.grp(q) else "own" if cp.own(q) else "dirty"
        if k == kind:
            out.append(int(p))
            if len(out) == n:
                break
    assert len(out) == n, "%d positions of kind %s, %d wanted" % (len(out), kind, n)
    return out


def test_the_part_read_back_is_the_and_of_the_bits_with_zeroed_slack(world):
    cp = world["cp"]
    assert cp.group_info == cp.clean_info and cp.group_info[0] == cp.units and cp.group_info[2] == world["thr"]
    n_words = (cp.units + 7) // 8
    assert len(cp.group_bytes) == 4 * n_words + 64 and not cp.group_bytes[4 * n_words:].any()
    bits = np.zeros(32 * 4 * n_words, dtype=bool)
    bits[:len(cp.clean)] = cp.clean
    assert np.array_equal(cp.group[:32 * n_words], bits.reshape(-1, GROUP).all(axis=1))
    assert 0 < int(cp.group.sum()) < int(cp.clean.sum())


@pytest.mark.parametrize("kind", ["group", "own", "dirty"])
def test_a_lone_substitution_by_the_kind_of_its_position(world, kind):
    """in a clean group: settled in the owner lane; clean in a group that is not: dealt, settled by its word of sub_clean; dirty: dealt,
    sent to the table.  Only reads that the model puts on their own diagonal with that one entry (not on a near-copy's)"""
    rng = np.random.default_rng(31)
    g, cp = world["g"], world["cp"]
    reads = []
    for p in _positions(world, rng, kind, 60):
        for m in (40, 75, 110):
            r = _sub(g[p - m:p - m + 150], m, p)
            if _model(cp, r, world["order"], world["thr"]) == (_q_of(world, p) - m, [(m, True)]):
                reads.append(r)
    n = len(reads)
    assert n >= 40, n
    st = _check(world, "kind_" + kind, reads)
    assert len(world["cases"]["kind_" + kind][0]) == n and st["mismatches"] == n == st["subst_bits"], st
    if kind == "group":
        assert st["subst_groups"] == n == st["subst_clean"] and st["tab_lookups"] == 0, st
    elif kind == "own":
        assert st["subst_groups"] == 0 and st["subst_clean"] == n and st["tab_lookups"] == 0, st
    else:
        assert st["subst_groups"] == 0 == st["subst_clean"] and st["tab_lookups"] > 0, st


def test_every_alignment_of_the_diagonal_and_the_bases_at_the_edges(world):
    """32 consecutive diagonals (every q0 mod 32), eight lengths, the substitution at 0, 1, order - 1, order, len - order, len - 1"""
    g, order = world["g"], world["order"]
    reads = []
    for length in LENGTHS:
        for a in range(20_500, 20_532):
            for m in sorted({m for m in (0, 1, order - 1, order, length - order, length - 1) if 0 <= m < length}):
                reads.append(_sub(g[a:a + length], m, a + m))
    assert len(reads) == 32 * sum(len({m for m in (0, 1, order - 1, order, n - order, n - 1) if 0 <= m < n}) for n in LENGTHS)
    st = _check(world, "alignments", reads)
    assert st["subst_groups"] > 0 and st["subst_bits"] > st["subst_groups"]


def test_the_text_s_ends_and_short_contigs(oracle):
    """reads at the first and the last positions of the text and across short contigs: marks clear the bits within order - 1 bases, and
    with them the groups they touch"""
    rng = np.random.default_rng(8_2027)
    short = [synth.genome(int(n), seed=700 + i) for i, n in enumerate(rng.integers(300, 501, 12))]
    contigs = short + [_genome()]
    sbwt = _make(oracle, contigs)
    order, thr, anch = _thresholds(sbwt)
    w = {"sbwt": sbwt, "ora": oracle.Index.build([c.tobytes() for c in contigs], k=K), "oracle": oracle, "order": order, "thr": thr, "cp": Copy(sbwt),
         "cases": {}, "expected": {}}
    reads = []
    for c in short + [contigs[-1]]:
        for length in (thr + 1, 100, 150):
            for m in sorted({0, 1, order - 2, order - 1, order, order + 1, order + 2, order + 3, order + 4, length // 2}):
                head, tail = c[:length].copy(), c[len(c) - length:].copy()
                reads += [_sub(head, m, m), _sub(tail, length - 1 - m, m)]
    for ia in range(12):
        for s in (15, 75, 134):
            for m in (s - order, s - 1, s, s + order - 1, s + order):
                reads.append(_sub(np.concatenate([short[ia][len(short[ia]) - s:], short[(ia + 5) % 12][:150 - s]]), m, m))
    st = _check(w, "ends", reads[:2_000], exact=False)
    assert st["subst_bits"] >= 1
    _, want = _predict(w["cp"], [r for r in reads if _model(w["cp"], r, order, thr) is not None], order, thr)
    assert want["subst_groups"] < want["subst_clean"], want  # (the fixture has positions beside a mark whose bit is set and whose group is not)


def test_two_substitutions_where_eligibility_flips(world):
    g, order = world["g"], world["order"]
    rng = np.random.default_rng(5)
    reads = []
    for d in (order - 2, order - 1, order, order + 1):
        for p in _positions(world, rng, "group", 12):
            for m in (3, 60, 149 - d - 3):
                reads.append(_sub(g[p - m:p - m + 150], (m, m + d), p))
    st = _check(world, "two_apart", reads)
    assert 0 < st["subst_bits"] < st["mismatches"]


def test_a_full_list_all_settled_and_a_wave_that_deals_nothing(world):
    """thirteen lone substitutions in one read, each in a clean group; and a wave of 64 reads whose every mismatch is settled in its
    owner lane: stage 3's loop runs zero times - no filter word, no table byte -, the characters are written, nothing is flagged"""
    g, order, thr, cp = world["g"], world["order"], world["thr"], world["cp"]
    D = cp.seed_d
    at = [D + order * i for i in range(LIST)]
    assert at[-1] < 160
    full = []
    for a in range(1_000, 44_000, 7):
        r = _sub(g[a:a + 160], at, a)
        got = _model(cp, r, order, thr)
        if got is not None and got[0] is not None and len(got[1]) == LIST and all(lone and cp.grp(got[0] + m) for m, lone in got[1]):
            full.append(r)
            if len(full) == 8:
                break
    assert len(full) == 8, "no window with thirteen clean groups %d bases apart" % order
    st = _check(world, "list_full", full)
    assert st["subst_groups"] == 8 * LIST == st["mismatches"] and st["tab_lookups"] == 0 and st["seed_extensions"] == 0, st
    rng = np.random.default_rng(64)
    wave = []
    for p in _positions(world, rng, "group", 200):
        r = _sub(g[p - 75:p + 75], 75, p)
        if len(wave) < 64 and _model(cp, r, order, thr) == (_q_of(world, p) - 75, [(75, True)]):
            wave.append(r)
    st = _check(world, "wave_settled", wave)
    assert len(world["cases"]["wave_settled"][0]) == 64
    assert st["subst_groups"] == 64 == st["mismatches"] and st["tab_lookups"] == 0 and st["seed_extensions"] == 0 and st["tab_flagged"] == 0, st


def test_a_wave_that_still_deals_more_than_64_items(world):
    """5 % substitutions: what the owner lanes leave is more than a round of the wave's lanes - the loop runs twice"""
    g = world["g"]
    rng = np.random.default_rng(50)
    reads = []
    for a in rng.integers(400, len(g) - 600, 128):
        r = g[a:a + 150].copy()
        hit = np.flatnonzero(rng.random(150) < 0.05)
        reads.append(_sub(r, hit, int(a)) if len(hit) else r)
    st = _check(world, "five_percent", reads, exact=False)
    assert st["mismatches"] - st["subst_groups"] > 2 * 64 and st["subst_groups"] > 0, st


def _indel(g, start, pos, size, ins, rng):
    i = np.arange(150)
    shift = np.where(i >= pos, -np.minimum(size, i - pos) if ins else size, 0)
    r = g[start + i + shift].copy()
    if ins:
        r[pos:pos + size] = ACGT[rng.integers(0, 4, size)]
    return r


def test_reads_that_leave_their_first_diagonal_use_no_loaded_word(world):
    """an insertion or deletion near the head (the seed's diagonal becomes the second one), a read whose first windows give no seed (its
    diagonal comes from its end), a cut read with a substitution far from the cut, reads of another genome (a chance seed or none:
    judged like reads without a diagonal): the owner lane settles nothing for any of them, and the bytes are the oracle's.
    What these cases can and cannot tell: a cut read is refused by eligible() and a read that lost its seed by the walk's own condition,
    whether or not the word was zeroed, and a read seeded from its end never loaded one; after a front swap the read is cut or takes
    one diagonal whole, both of which zero the word again.  The one zeroing that alone keeps a stale word from being used - a whole
    diagonal from the second seed - has the test below."""
    g, order, cp = world["g"], world["order"], world["cp"]
    D = cp.seed_d
    rng = np.random.default_rng(77)
    clean = _positions(world, rng, "group", 60)
    head, tail_seeded, cut = [], [], []
    for p in clean:
        start = p - 110  # the substitution at base 110 of the read, in a clean group
        for size in (1, 2, 3):
            for ins in (False, True):
                r = _indel(g, start - (0 if ins else 0), D - 2, size, ins, rng)  # the break inside the first window
                # (the bases in front of the break against the tail's diagonal: six or more mismatch - stage 2b looks beside it)
                shifted = g[start + size * (-1 if ins else 1) + np.arange(D - 2)] if not ins else g[start - size + np.arange(D - 2)]
                r = _sub(r, 110, p)
                # (... the model, which knows the diagonal the seed gives, agrees that stage 2b looks at the read, and the text HAS the
                # head's diagonal beside the tail's: a path of the cover that starts or changes copies there leaves the read where it is)
                q_tail = cp.text.find(r[40:100].tobytes()) - 40
                q_head = q_tail + (size if ins else -size)
                beside = q_tail >= 40 and cp.text[q_head:q_head + D - 2] == r[:D - 2].tobytes() and not cp.mark[q_head - 3:q_head + 16].any()
                if int((r[:D - 2] != shifted).sum()) >= 6 and beside and _model(cp, r, order, world["thr"]) is None:
                    head.append(r)
                cut.append(_sub(_indel(g, start, 75, size, ins, rng), 20, p))
        r = g[start:start + 150].copy()
        tail_seeded.append(_sub(r, [D // 2 + D * i for i in range(CAP // D + 1)] + [110], p))  # a substitution in every window stage 1 tries
    other = synth.genome(20_000, seed=4242)
    unrelated = [other[a:a + 150].copy() for a in rng.integers(0, len(other) - 150, 384)]
    # (some of them DO get a seed, by chance, on which more than a third of their bases mismatch: the reset)
    n_reset = 0
    for r in unrelated:
        q0 = _first_seed(cp, r)
        if q0 is not None and 0 <= q0 and q0 + 150 <= len(cp.base):
            n_mm = int(((cp.base[q0:q0 + 150] != np.searchsorted(ACGT, r)) | cp.mark[q0:q0 + 150]).sum())
            n_reset += n_mm > LIST and 3 * n_mm > 150
    assert n_reset >= 1, "no read of the other genome finds a seed by chance"
    settled = {}
    for name, reads in (("indel_at_head", head), ("seeded_from_the_end", tail_seeded), ("cut_far_from_substitution", cut), ("chance_seed", unrelated)):
        assert len(reads) >= 20, (name, len(reads))
        st = _check(world, name, reads[:400], exact=False)
        settled[name] = st["subst_groups"]
        if name == "seeded_from_the_end":
            assert st["subst_bits"] >= 1, st  # (their lone substitution is eligible - on a diagonal found in 2b: dealt, asked of sub_clean)
    assert not any(settled.values()), settled


def test_a_whole_diagonal_from_the_second_seed_drops_the_first_one_s_word(oracle):
    """a genome with stretches of 30 bases (fewer than k: the paths of the cover stay apart) that stand in it twice.  A read that starts
    with such a stretch and has a substitution in each of the next three windows stage 1 tries finds only ambiguous seeds and takes
    the stretch's first copy; where that is the wrong one, everything behind the stretch mismatches, stage 2b seeds the read from its
    end and the second diagonal alone is as good as any cut - the read moves to it whole, and the word loaded for the first diagonal
    must not be asked: the read's lone substitution at base 110 is eligible and is dealt, the owner lane settles nothing"""
    g = synth.genome(30_000, seed=505).copy()
    pairs = []
    for i in range(10):
        s, d = 1_000 + 2_800 * i, 2_400 + 2_800 * i
        g[d:d + 30] = g[s:s + 30]
        pairs += [s, d]
    sbwt = _make(oracle, [g])
    order, thr, _ = _thresholds(sbwt)
    w = {"sbwt": sbwt, "ora": oracle.Index.build([g.tobytes()], k=K), "oracle": oracle, "g": g, "order": order, "thr": thr, "cp": Copy(sbwt),
         "cases": {}, "expected": {}}
    cp = w["cp"]
    moved, stayed = [], []
    for a in pairs:
        D = cp.seed_d
        r = _sub(g[a:a + 150], [30 + D * i for i in range(3) if 30 + D * i < CAP] + [110], a)
        q_true = cp.text.find(g[a + 75:a + 145].tobytes()) - 75
        q_seed = _first_seed(cp, r)
        if q_true < 0 or q_seed is None or cp.mark[q_true:q_true + 150].any() or not cp.grp(q_true + 110):
            continue
        (stayed if q_seed == q_true else moved).append(r)
    assert len(moved) >= 3 and len(stayed) >= 3, (len(moved), len(stayed))
    st = _check(w, "moved_whole", moved, exact=False)
    assert st["subst_groups"] == 0 and st["subst_bits"] >= len(moved) and st["mismatches"] == 4 * len(moved), st
    st = _check(w, "stayed", stayed)
    assert st["subst_groups"] == len(stayed), st


def test_another_threshold_gets_no_groups(world):
    from kbo_amd import derandomize
    prob = 1e-9
    assert derandomize.random_match_threshold(K, world["sbwt"].n_kmers(), 4, prob) != world["thr"]
    e = world["expected"].get("kind_group") or Expected(world["oracle"], world["ora"], [_sub(world["g"][a:a + 150], 75, a) for a in range(5_000, 5_640, 10)], False)
    want = world["ora"].matches_batch(e.concat, e.offsets, prob, n_threads=threads())
    chars, st = _stats(world["sbwt"], e.concat, e.offsets, prob)
    _first_difference(chars, want, e.keep, e.offsets, "another threshold")
    assert st["subst_groups"] == 0 and st["subst_bits"] == 0 and st["tab_lookups"] > 0, st


def test_a_copy_without_the_groups_beside_one_with_them(world, oracle):
    """KBO_SUBST_GROUPS=0 is read when a copy's plan structures are made: the same bytes, the same subst_bits and subst_clean, and
    nothing settled in the owner lane"""
    os.environ["KBO_SUBST_GROUPS"] = "0"
    try:
        plain = _make(oracle, [world["g"]])
    finally:
        os.environ.pop("KBO_SUBST_GROUPS", None)
    assert len(plain.plan_part("sub_group")[0]) == 0 and np.array_equal(plain.plan_part("sub_clean")[0], world["cp"].clean_words)
    assert plain.device_layout()["cover_bytes"] + 4 * ((world["cp"].units + 7) // 8) == world["sbwt"].device_layout()["cover_bytes"]
    g = world["g"]
    rng = np.random.default_rng(9)
    reads = [_sub(g[a:a + 150], rng.choice(150, int(rng.integers(1, 4)), replace=False), int(a)) for a in rng.integers(400, len(g) - 600, 640)]
    e = Expected(oracle, world["ora"], reads, False)
    with_g, st_with = _stats(world["sbwt"], e.concat, e.offsets)
    without, st_without = _stats(plain, e.concat, e.offsets)
    _first_difference(with_g, e.chars, e.keep, e.offsets, "with the groups")
    _first_difference(without, e.chars, e.keep, e.offsets, "without the groups")
    assert np.array_equal(with_g, without)
    print({k: (st_with[k], st_without[k]) for k in ("mismatches", "subst_bits", "subst_clean", "subst_groups", "seed_extensions", "tab_lookups", "tab_flagged")})
    assert (st_with["subst_bits"], st_with["subst_clean"]) == (st_without["subst_bits"], st_without["subst_clean"]), (st_with, st_without)
    assert st_without["subst_groups"] == 0 < st_with["subst_groups"], (st_with, st_without)
