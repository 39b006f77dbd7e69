"""The second randomized oracle soak on the host: the generator of tests/refset_random_configs.py is deterministic and well formed, the
coverage conditions that the generator and the oracle alone decide hold over its SEEDS, and for every seed the CPU restatements of the
reference-set kernels - kbo_refset_ms_host, kbo_refset_candidates_host, kbo_locate_refset_host, kbo_cover_refset_host and
kbo_call_refset_host - agree with the yardsticks tests/test_gpu_refset_random_configs.py compares the device code with.  No GPU.

World(cfg, oracle) is the oracle side of one configuration, and the GPU module's: ONE oracle index per reference
(oracle.Index.build([ref], k, add_revcomp)), the reverse complements made in numpy, and the brute-force contracts of
tests/test_refset_screen_host.py (expected), tests/test_refset_locate_host.py (occurrences, expected_locus, expected_tested) and
tests/test_refset_cover_host.py (brute_cover) over them.  Nothing expected comes from the library under test, except the argument of
the screen's contract that kbo_hip.h gives it: k and n_kmers, which the oracle's index states too and which are compared.

A set is REFUSED as a whole when some reference's threshold at the call's max_error_prob is 1 or less (kbo_hip.h, kbo_find_refset:
KBO_E_THRESHOLD_LE_1, as kbo_find on that reference's own handle; k = 1 always is)."""
import re

import numpy as np
import pytest

import kbo_amd
from kbo_amd import refset

import refset_random_configs as rrc
from test_gpu_refset_dev import fold
from test_refset_cover_host import brute_cover
from test_refset_locate_host import expected_locus, expected_tested, occurrences
from test_refset_screen_host import expected as screen_expected, stretches as base_stretches

E_THRESHOLD_LE_1, E_UNSUPPORTED, E_REF_PANIC = -3, -8, -11
NONE = 0xFFFFFFFF
L_, I_, W_, NONE_ = refset.ROUTE_LDS, refset.ROUTE_INDEX, refset.ROUTE_WIDE, refset.ROUTE_NONE


class World:
    """the oracle side of one configuration; every expected value is made once and kept"""

    def __init__(self, cfg, oracle):
        self.cfg, self.ora, self.k, self.rc = cfg, oracle, cfg.k, cfg.add_revcomp
        self.refs, self.seqs, self.planted = rrc.make_inputs(cfg)
        self.n_refs, self.n_seqs = len(self.refs), len(self.seqs)
        self.lens = np.asarray([len(s) for s in self.seqs], dtype=np.int64)
        self.index = [oracle.Index.build([ref.tobytes()], k=self.k, add_revcomp=self.rc) for ref in self.refs]
        self.n_kmers = [ix.n_kmers for ix in self.index]
        self.rows = [ix.n_sets for ix in self.index]
        self.queryable = [r for r in range(self.n_refs) if self.n_kmers[r] > 0]
        self.route = [NONE_ if self.n_kmers[r] == 0 else L_ if self.rows[r] <= rrc.MAX_ROWS else W_ if self.rows[r] <= cfg.wide_rows else I_
                      for r in range(self.n_refs)]
        self.packed = [r for r in self.queryable if self.route[r] != I_]  # the references with entries
        self.packed_only = len(self.packed) == len(self.queryable)
        self.strand = {(s, 1): q for s, q in enumerate(self.seqs)}
        self.strand.update({(s, 2): rrc.revcomp(q) for s, q in enumerate(self.seqs)})
        self._thr, self._aln, self._find, self._calls, self._dicts = {}, {}, {}, {}, None
        self.m, self._ref_mers, self._seq_mers = {}, {}, {}  # what test_refset_screen_host.expected reads
        self.stretches = {r: [x for st in base_stretches(self.refs[r], self.k) for x in ([st, rrc.revcomp(st)] if self.rc else [st])]
                          for r in self.packed}

    def thr(self, prob):
        if prob not in self._thr:
            self._thr[prob] = [self.ora.random_match_threshold(self.k, n, 4, prob) if n else 0 for n in self.n_kmers]
            self.m[prob] = [min(t + 1, self.k, rrc.SEED_MAX) if n else 0 for t, n in zip(self._thr[prob], self.n_kmers)]
        return self._thr[prob]

    def refused(self, prob):
        """the code every call on the set returns at this max_error_prob, or 0"""
        return E_THRESHOLD_LE_1 if any(self.thr(prob)[r] <= 1 for r in self.queryable) else 0

    def aln(self, prob):
        """(r, s, strand) -> the oracle's characters, for every reference that can be queried"""
        if prob not in self._aln:
            out = {}
            for r in self.queryable:
                seen = {}
                for (s, strand), q in self.strand.items():
                    text = q.tobytes()
                    if text not in seen:
                        seen[text] = self.index[r].matches(text, prob)
                    out[r, s, strand] = seen[text]
            self._aln[prob] = out
        return self._aln[prob]

    def _pairs(self, strands, refs=None):
        for r in (self.queryable if refs is None else refs):
            for s in range(self.n_seqs):
                for strand in (1, 2):
                    if strands & strand:
                        yield r, s, strand

    def find(self, prob, gap, strands):
        """kbo_find_refset's records: tuples (ref, seq, strand, the seven fields of a run), in its order"""
        key = (prob, gap)
        if key not in self._find:
            aln = self.aln(prob)
            self._find[key] = {p: self.ora.run_lengths_gapped(aln[p], gap) for p in self._pairs(3)}
        return [p + tuple(t) for p in self._pairs(strands) for t in self._find[key][p]]

    def summary(self, prob, strands):
        """kbo_summary_refset's records: (ref, seq, strand) + the fold of the characters, the pairs that are all '-' dropped"""
        aln = self.aln(prob)
        out = [p + fold(aln[p]) for p in self._pairs(strands)]
        return [t for t in out if t[6] > 0]

    def hits(self, prob, strands):
        return {t[:3] for t in self.summary(prob, strands)}

    @staticmethod
    def best(n_seqs, records):
        """kbo_ref_best of every sequence, by sorting the summary records by (larger n_match, smaller ref, '+' first)"""
        out = []
        for s in range(n_seqs):
            mine = sorted((t for t in records if t[1] == s), key=lambda t: (-t[3], t[0], t[2]))
            if not mine:
                out.append((s, NONE, 0, 0, 0, 0, 0, 0, 0, 0, NONE, 0))
                continue
            first = mine[0]
            others = [t for t in mine if t[0] != first[0]]
            out.append((s, first[0], first[2]) + tuple(first[3:9]) + (len(mine), others[0][0] if others else NONE, others[0][3] if others else 0))
        return out

    def screen(self, prob, strands):
        """the brute-force contract of the screen: [n_refs, n_seqs, 2]"""
        self.thr(prob)
        return screen_expected(self, prob, strands)

    def runs(self, strands):
        """the runs legs e and f are given: find's at max_error_prob and max_gap_len, of the references with entries"""
        rec = [t for t in self.find(self.cfg.max_error_prob, self.cfg.max_gap_len, strands) if self.route[t[0]] in (L_, W_)]
        return np.array(rec, dtype=refset.REF_RUN)

    def dicts(self):
        if self._dicts is None:
            self._dicts = [occurrences(ref, self.k, self.rc) if r in self.packed else {} for r, ref in enumerate(self.refs)]
        return self._dicts

    def loci(self, runs):
        d = self.dicts()
        out = np.zeros(len(runs), dtype=refset.REF_LOCUS)
        for x, w in enumerate(runs):
            loc = expected_locus(d[w["ref"]], self.k, self.seqs[w["seq"]], int(w["strand"]), int(w["start"]), int(w["end"]))
            out[x] = loc + (expected_tested(self.k, int(w["start"]), int(w["end"]), loc),)
        return out

    def cover(self, runs):
        """(covers, profile, offsets) by the definitions"""
        entries = [r in self.packed for r in range(self.n_refs)]
        return brute_cover(self.refs, self.dicts(), entries, self.k, self.seqs, runs)[:3]

    def calls(self, strands):
        """kbo_call_refset's records by the oracle's literal call of every pair with a hit: tuples (ref, seq, strand, pos, query_chars,
        ref_chars) in its order; or the oracle's error code when the reference panics at a site"""
        prob = self.cfg.max_error_prob
        out = []
        for p in sorted(self.hits(prob, strands)):
            if p not in self._calls:
                try:
                    self._calls[p] = [(pos, qc.encode(), rf.encode()) for pos, qc, rf in self.index[p[0]].call(self.strand[p[1], p[2]], self.k, prob)[0]]
                except self.ora.OracleError as e:
                    self._calls[p] = e.code
            if isinstance(self._calls[p], int):
                return self._calls[p]
            out += [p + v for v in self._calls[p]]
        return out

    def slab_groups(self):
        """the slabs of the unscreened device forms: consecutive queryable references, refs_per_slab of them"""
        q, n = self.queryable, self.cfg.refs_per_slab or max(1, len(self.queryable))
        return [q[i:i + n] for i in range(0, len(q), n)]

    def mixed_slab(self):
        return any({L_, W_} <= {self.route[r] for r in g} for g in self.slab_groups())

    def stats(self):
        """what the coverage conditions count, from the generator and the oracle alone"""
        cfg = self.cfg
        st = dict(refused=bool(self.refused(cfg.max_error_prob) or self.refused(cfg.find_prob)), routes=set(self.route),
                  mixed_slab=self.packed_only and self.mixed_slab(), wide_rows_above_64k=any(self.route[r] == W_ and self.rows[r] > 65536
                                                                                               for r in range(self.n_refs)))
        if st["refused"]:
            return st
        st["hits"] = len(self.hits(cfg.find_prob, cfg.strands))
        if self.packed_only:
            calls = self.calls(cfg.strands)
            st["variants"] = -1 if isinstance(calls, int) else len(calls)
        if cfg.prefilter:
            bits = self.screen(cfg.find_prob, cfg.strands)
            st["candidates"] = int(bits.sum())
            st["unscreenable"] = any(self.m[cfg.find_prob][r] < rrc.SEED_MIN for r in self.packed)
        return st


def build_set(cfg, refs):
    return refset.RefSet.build(refs, kbo_amd.BuildOpts(k=cfg.k, add_revcomp=cfg.add_revcomp, num_threads=4), wide_rows=cfg.wide_rows,
                               prefilter=cfg.prefilter, positions=cfg.positions)


def call_opts(cfg, add_revcomp=None):
    arc = cfg.call_add_revcomp if add_revcomp is None else add_revcomp
    return kbo_amd.CallOpts(max_error_prob=cfg.max_error_prob, sbwt_build_opts=kbo_amd.BuildOpts(k=cfg.k, add_revcomp=arc, build_select=True))


def check_set(w, rs):
    """the set is what the oracle says of every reference alone: k-mers, status, route"""
    for r in range(w.n_refs):
        assert rs.n_kmers(r) == w.n_kmers[r] and (rs.status(r) != 0) == (w.n_kmers[r] == 0) and rs.route(r) == w.route[r], \
            (r, rs.n_kmers(r), w.n_kmers[r], rs.status(r), rs.route(r), w.route[r], w.rows[r])
    assert rs.packed_only() == w.packed_only and len(rs) == w.n_refs and rs.k() == w.k


def as_tuples(variants, chars):
    return [(int(v["ref"]), int(v["seq"]), int(v["strand"]), int(v["pos"])) + refset.variant_chars(v, chars) for v in variants]


def _words(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32).reshape(len(a), a.dtype.itemsize // 4)


STATS = {}  # seed -> (Config, World.stats()): what the coverage test counts


def check_host(cfg, oracle):
    """the host restatements against the yardsticks, on this configuration's inputs -> World.stats()"""
    w = World(cfg, oracle)
    rs = build_set(cfg, w.refs)
    check_set(w, rs)
    tag = cfg.describe()
    for prob in {cfg.max_error_prob, cfg.find_prob}:
        code = w.refused(prob)
        if code and cfg.prefilter:
            with pytest.raises(kbo_amd.KboError) as ei:
                rs.candidates(w.seqs, prob, cfg.strands, host=True)
            assert ei.value.code == code, tag
    if w.refused(cfg.max_error_prob):
        if w.packed_only:
            with pytest.raises(kbo_amd.KboError) as ei:
                refset.call_refset(w.seqs, rs, call_opts(cfg), cfg.strands, host=True)
            assert ei.value.code == w.refused(cfg.max_error_prob), tag
        return w.stats()
    # kbo_refset_ms_host: the wide kernel's step against the oracle's matching statistics, every pair of a packed reference
    for r in w.packed:
        seen = {}
        for (s, strand), q in w.strand.items():
            text = q.tobytes()
            if text not in seen:
                seen[text] = True
                d = w.index[r].matching_statistics(q)[0]
                assert np.array_equal(rs.ms_host(r, q), d.astype(np.uint8)), "ms_host: reference %d sequence %d strand %d | %s" % (r, s, strand, tag)
    # kbo_refset_candidates_host against the contract, and every pair with a hit has its bit
    if cfg.prefilter:
        for prob in sorted({cfg.max_error_prob, cfg.find_prob}):
            if w.refused(prob):
                continue
            bits = rs.candidates(w.seqs, prob, cfg.strands, host=True)
            exp = w.screen(prob, cfg.strands)
            assert np.array_equal(bits, exp), "candidates_host at %g: %s | %s" % (prob, np.argwhere(bits != exp)[:5].tolist(), tag)
            for r, s, strand in w.hits(prob, cfg.strands):
                assert w.route[r] == I_ or bits[r, s, strand - 1], "a pair with a hit without its bit: %s | %s" % ((r, s, strand), tag)
    # kbo_locate_refset_host and kbo_cover_refset_host against brute force over the oracle's runs
    if cfg.positions:
        runs = w.runs(cfg.strands)
        loci = refset.locate_refset(w.seqs, rs, runs, host=True)
        exp = w.loci(runs)
        assert np.array_equal(_words(loci), _words(exp)), "locate_host: record %s | %s" % (np.flatnonzero((_words(loci) != _words(exp)).any(axis=1))[:5], tag)
        covers, profile, offsets = refset.cover_refset(w.seqs, rs, runs, depth=True, host=True)
        ec, ep, eo = w.cover(runs)
        assert np.array_equal(offsets, eo) and covers.tobytes() == ec.tobytes() and np.array_equal(profile, ep), "cover_host | " + tag
    # kbo_call_refset_host against the oracle's call of every pair with a hit
    if w.packed_only:
        exp = w.calls(cfg.strands)
        if isinstance(exp, int):  # the reference panics at a site
            with pytest.raises(kbo_amd.KboError) as ei:
                refset.call_refset(w.seqs, rs, call_opts(cfg, False), cfg.strands, host=True)
            assert ei.value.code == E_REF_PANIC, tag
        else:
            variants, chars = refset.call_refset(w.seqs, rs, call_opts(cfg, False), cfg.strands, host=True)
            assert as_tuples(variants, chars) == exp, "call_host (%d vs %d records) | %s" % (len(variants), len(exp), tag)
            if cfg.call_add_revcomp:  # no contig holds a stretch and its reverse complement: the flag changes no byte, so the oracle,
                v2, c2 = refset.call_refset(w.seqs, rs, call_opts(cfg, True), cfg.strands, host=True)  # which does not model it, judges both
                assert v2.tobytes() == variants.tobytes() and c2.tobytes() == chars.tobytes(), "call_host with add_revcomp | " + tag
    else:
        with pytest.raises(kbo_amd.KboError) as ei:
            refset.call_refset(w.seqs, rs, call_opts(cfg), cfg.strands, host=True)
        assert ei.value.code == E_UNSUPPORTED, tag
    return w.stats()


# ---- the generator
def test_the_generator_is_deterministic():
    for seed in rrc.SEEDS[:12] + (rrc.STRESS_FIRST_SEED,):
        a, b = rrc.config(seed), rrc.config(seed)
        assert a == b and a.describe() == b.describe()
        (r1, s1, p1), (r2, s2, p2) = rrc.make_inputs(a), rrc.make_inputs(b)
        assert p1 == p2 and all(x.tobytes() == y.tobytes() for x, y in zip(r1 + s1, r2 + s2)) and len(r1) == len(r2) and len(s1) == len(s2)
    assert rrc.config(1) != rrc.config(2)
    assert rrc.K_CLASSES is __import__("random_configs").K_CLASSES


@pytest.mark.parametrize("seed", rrc.SEEDS)
def test_every_configuration_is_well_formed(seed):
    cfg = rrc.config(seed)
    refs, seqs, planted = rrc.make_inputs(cfg)
    k = cfg.k
    assert 3 <= len(refs) <= 24 and [len(r) for r in refs] == list(cfg.ref_lens) and len(cfg.kinds) == len(refs)
    assert 1 <= len(seqs) == cfg.n_seqs <= 300 and all(len(s) >= 3 and s.dtype == np.uint8 for s in seqs)
    assert 1 <= k <= 255 and rrc.MAX_ROWS <= cfg.wide_rows <= rrc.WIDE_MAX_ROWS and cfg.strands in (1, 2, 3)
    assert cfg.max_error_prob in (1e-7, 1e-4) and cfg.find_prob in (cfg.max_error_prob, 0.5) and cfg.max_gap_len in (0, 5, 40)
    for kind, ref in zip(cfg.kinds, refs):
        n = {"short": k - 1, "k": k, "k1": k + 1, "2k": 2 * k}.get(kind)
        assert n is None or len(ref) == n
        if kind == "long":
            assert 17_000 <= len(ref) <= 70_000 and k >= rrc.LONG_MIN_K
        if kind == "n_lower":
            assert (ref == ord("N")).sum() == 1 and re.search(b"[acgt]{5,}", ref.tobytes())
        if kind == "two_letter":
            assert set(ref.tobytes()) <= set(b"AT")
    twins = [r for r, kind in enumerate(cfg.kinds) if kind == "twin"]
    assert len(twins) in (0, 2) and (not twins or refs[twins[0]].tobytes() == refs[twins[1]].tobytes())
    lens = sorted(len(s) for s in seqs)
    if cfg.n_seqs > 1:
        assert {max(3, n) for n in (3, k - 1, k, k + 1, 2 * k + 1)} <= set(lens) and any((s == ord("N")).sum() >= 3 for s in seqs)
    chunk = rrc.chunk_of(k)
    assert cfg.more_than_256_chunks == (lens[-1] > rrc.TASK_ITEMS * chunk) and cfg.above_65536 == (lens[-1] > 65536)
    assert cfg.above_65536 or sum(lens) < 60_000
    assert len(planted) >= 9
    ops = set()
    for p in planted:
        q, ref, at, a, w = seqs[p["seq"]], refs[p["ref"]], p["at"], p["a"], p["w"]
        piece = ref[a:a + w]
        assert len(piece) == w > 0
        ops.add(p["op"])
        if p["op"] == "exact":
            assert q[at:at + w].tobytes() == piece.tobytes()
        elif p["op"] == "rc":
            assert q[at:at + w].tobytes() == rrc.revcomp(piece).tobytes()
        elif p["op"] in ("sub1", "sub3"):
            assert (q[at:at + w] != piece).mean() <= (0.04 if p["op"] == "sub1" else 0.08) + 2.0 / w
        elif p["op"] == "ins2":
            x = p["x"]
            assert q[at:at + x].tobytes() == piece[:x].tobytes() and q[at + x + 2:at + w + 2].tobytes() == piece[x:].tobytes()
        else:
            x = p["x"]
            assert p["op"] == "del3" and q[at:at + x].tobytes() == piece[:x].tobytes() and q[at + x:at + w - 3].tobytes() == piece[x + 3:].tobytes()
    first = [p for p in planted if p["seq"] == planted[0]["seq"]][:3]
    for i, p in enumerate(first):  # across the first three multiples of the chunk
        assert p["at"] < (i + 1) * chunk < p["at"] + p["w"] or p["w"] <= 75
    if cfg.n_seqs > 1:
        assert any(p["at"] == 0 for p in planted) and any(p["at"] + p["w"] == len(seqs[p["seq"]]) for p in planted)
    dev, index = rrc.with_shorts(cfg, seqs)
    assert len(dev) == len(seqs) + len(cfg.short_seqs) and all(dev[i] is seqs[s] for s, i in enumerate(index))
    assert sorted(len(dev[i]) for i in set(range(len(dev))) - set(index.tolist())) == sorted(n for _, n in cfg.short_seqs)
    if cfg.call_add_revcomp:
        assert k >= 32


# ---- the host restatements, every seed
@pytest.mark.parametrize("seed", rrc.SEEDS)
def test_host_restatements_equal_the_yardsticks(oracle, seed):
    cfg = rrc.config(seed)
    try:
        STATS[seed] = (cfg, check_host(cfg, oracle))
    except BaseException:
        print("FAILED seed %d: %s" % (seed, cfg.describe()))
        raise


def _count(pred):
    return sum(1 for cfg, st in STATS.values() if pred(cfg, st))


def _ran(c, st):
    return not st["refused"]


def _k_in(lo, hi):
    return lambda c: lo <= c.k <= hi


_K_RANGES = (("k <= 64", 8, _k_in(1, 64)), ("64 < k < 128", 8, _k_in(65, 127)), ("128 <= k < 192", 5, _k_in(128, 191)), ("k >= 192", 5, _k_in(192, 255)),
             ("k a multiple of 16", 3, lambda c: c.k % 16 == 0))
# (what, at least, predicate over (Config, World.stats())): conditions on the seed list that the generator and the oracle alone decide
HOST_CONDITIONS = [("k class %d %s" % (i, (cls[0], cls[-1])), 8, (lambda i: lambda c, st: rrc.k_class(c.k) == i)(i)) for i, cls in enumerate(rrc.K_CLASSES)] + [
    ("k = %d" % k, 3, (lambda k: lambda c, st: c.k == k)(k)) for k in (64, 65, 128, 129)] + [
    ("k = 255", 4, lambda c, st: c.k == 255),
    ("k < 11 with a prefilter", 8, lambda c, st: c.k < 11 and c.prefilter),
    ("11 <= k < 24 with a prefilter", 5, lambda c, st: 11 <= c.k < 24 and c.prefilter),
    ("a chunk that is no multiple of 16", 15, lambda c, st: rrc.chunk_of(c.k) % 16 != 0),
    ("a chunk that is no multiple of 16, with a device leg", 5, lambda c, st: rrc.chunk_of(c.k) % 16 != 0 and c.device_leg and _ran(c, st)),
    ("a chunk of 4k with k a multiple of 4", 5, lambda c, st: rrc.chunk_of(c.k) == 4 * c.k and c.k % 4 == 0),
    ("LDS and wide references in one slab", 25, lambda c, st: st["mixed_slab"] and _ran(c, st)),
    ("a reference on the single-index route", 8, lambda c, st: I_ in st["routes"]),
    ("a reference with a status", 30, lambda c, st: NONE_ in st["routes"]),
    ("wide rows above 65 536", 3, lambda c, st: st["wide_rows_above_64k"] and _ran(c, st)),
    ("more than 256 chunks in one sequence", 5, lambda c, st: c.more_than_256_chunks and _ran(c, st)),
    ("a contig above 65 536 bases", 3, lambda c, st: c.above_65536 and _ran(c, st)),
    ("64 sequences or more", 10, lambda c, st: c.n_seqs >= 64),
    ("one sequence", 3, lambda c, st: c.n_seqs == 1),
] + [("sequences of %d bases in a device leg" % n, 5, (lambda n: lambda c, st: c.device_leg and _ran(c, st) and I_ not in st["routes"] and any(x[1] == n for x in c.short_seqs))(n)) for n in (0, 1, 2)] + [
    ("strands = %d" % v, 20, (lambda v: lambda c, st: c.strands == v)(v)) for v in (1, 2, 3)] + [
    ("slab budget %d" % v, 10, (lambda v: lambda c, st: c.slab_bytes == v)(v)) for v in (1 << 16, 1 << 18, 16 << 20)] + [
    ("refs_per_slab = %d" % v, 8, (lambda v: lambda c, st: c.refs_per_slab == v)(v)) for v in (1, 3)] + [
    ("record capacity 1", 10, lambda c, st: c.record_capacity == 1),
    ("pairs with a hit", 100, lambda c, st: st.get("hits", 0) > 0),
    ("an unscreenable reference under a screened form", 10, lambda c, st: st.get("unscreenable", False) and c.legs["h"] and I_ not in st["routes"]),
    ("max_pairs below the candidates", 8, lambda c, st: c.caps == "pairs" and st.get("candidates", 0) > 1 and (c.legs["h"] or c.legs["i"]) and I_ not in st["routes"]),
] + [
    ("the oracle calls a variant under leg %s, %s" % (leg, name), least, (lambda leg, f: lambda c, st: st.get("variants", 0) > 0 and c.legs[leg] and f(c))(leg, f))
    for leg in "gi" for name, least, f in _K_RANGES] + [
    ("add_revcomp of the call's own options where the oracle calls a variant, leg %s" % leg, 5,
     (lambda leg: lambda c, st: c.call_add_revcomp and c.legs[leg] and st.get("variants", 0) > 0)(leg)) for leg in "gi"] + [
    ("leg %s runs" % leg, 20, (lambda leg: lambda c, st: c.legs[leg] and _ran(c, st) and (
        c.prefilter if leg == "d" else c.positions if leg in "ef" else I_ not in st["routes"]))(leg)) for leg in rrc.LEGS]


def test_the_seed_list_covers_what_it_claims():
    """conditions on the seed list, not measurements: the classes, the routes the oracle's rows give, pairs with a hit, variants the
    oracle calls and candidates of the brute-force screen - and at most 10 % of the seeds refused as a whole"""
    missing = [s for s in rrc.SEEDS if s not in STATS]
    assert not missing, "seeds that did not run (or failed): %s" % missing[:20]
    counts = [(what, least, _count(pred)) for what, least, pred in HOST_CONDITIONS]
    for what, least, n in counts:
        print("%-70s %4d (>= %d)" % (what, n, least))
    refused = _count(lambda c, st: st["refused"])
    print("refused: %d of %d" % (refused, len(STATS)))
    assert refused * 10 <= len(STATS), "%d of %d configurations refused" % (refused, len(STATS))
    short = [(what, n, least) for what, least, n in counts if n < least]
    assert not short, "conditions not met (what, seen, at least): %s" % short
