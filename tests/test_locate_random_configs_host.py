"""The third randomized oracle soak on the host: the generator of tests/locate_random_configs.py is deterministic and well formed, the
coverage conditions that the generator and the brute force alone decide hold over its SEEDS, and for every seed the CPU restatements
of the kernels - kbo_positions_from_ms_host, kbo_segments_from_ms_host, kbo_place_from_segments_host, kbo_pileup_from_segments_host,
kbo_pileup_sites_host, kbo_indels_from_segments_host and kbo_indel_sites_host - agree word for word with the yardsticks
tests/test_gpu_locate_random_configs.py compares the device code with.  No GPU.

World(cfg) is the reference side of one configuration, and the GPU module's: the oracle's index over the sources and its walk of the
batch, the occurrence dict and the expected table of tests/test_index_locate_host.py, and over them that module's brute_segments,
brute_delta and brute_depth, py_place of tests/test_index_place_host.py, brute_pile and brute_sites of
tests/test_index_pileup_host.py and brute_events and brute_sites of tests/test_index_indel_host.py - imported, not copied.  Nothing
expected comes from the library under test.  The calls run strand by strand in the configuration's order; a d_segs capacity below the
count leaves placement, pileup and the indel events the records that fit, while delta counts every segment (kbo_hip.h); the events of
every strand go into one list, whose capacity cuts it to a prefix."""
import numpy as np
import pytest

from kbo_amd import locate

import locate_random_configs as lrc
from test_index_indel_host import INS, LONG, brute_events, event_tuples
from test_index_indel_host import brute_sites as brute_indel_sites
from test_index_locate_host import (NONE, brute_delta, brute_depth, brute_segments, covered, expected_table, occurrences, revcomp,
                                    src_offsets, stretches, walk)
from test_index_pileup_host import brute_pile, brute_sites, site_tuples
from test_index_place_host import py_place, same
from oracle import binding as ora


class World:
    """the reference side of one configuration; every expected value is made once and kept"""

    def __init__(self, cfg):
        self.cfg, self.k, self.rc = cfg, cfg.k, cfg.add_revcomp
        k = cfg.k
        self.srcs, self.seqs = lrc.make_inputs(cfg)
        self.soff = src_offsets(self.srcs)
        self.n_bases, self.n_seqs = int(self.soff[-1]), len(self.seqs)
        self.oi = ora.Index.build([s.tobytes() for s in self.srcs], k=k, add_revcomp=self.rc)
        self.occ = occurrences(self.srcs, k, self.rc)
        self.table = expected_table(self.oi, self.occ)
        self.strand_seqs = {st: [revcomp(s) for s in self.seqs] if st == 2 else self.seqs for st in cfg.strands}
        self.walks, self.segs, self.kept, self.kept_tuples, self.caps, self.places, self.bridged = {}, {}, {}, {}, {}, {}, {}
        delta = np.zeros(self.n_bases + 1, dtype=np.int64)
        self.depth = np.zeros(self.n_bases, dtype=np.uint32)
        self.pile = np.zeros((self.n_bases, 4), dtype=np.int64)
        place = None
        for st in cfg.strands:
            ss = self.strand_seqs[st]
            self.walks[st] = walk(self.oi, ss)
            recs = brute_segments(ss, self.occ, k, cfg.bridge, st)
            self.segs[st] = recs
            self.caps[st] = lrc.capacity(cfg.seg_cap, len(recs))
            kept = recs[:self.caps[st]]
            self.kept_tuples[st] = kept
            self.kept[st] = np.array(kept, dtype=locate.SEGMENT_DTYPE)
            delta += brute_delta(recs, k, self.n_bases).astype(np.int64)
            self.depth += brute_depth(recs, k, self.n_bases)
            place = py_place(self.kept[st], self.n_seqs, k, self.soff, cfg.max_gap, cfg.max_indel, merge_into=place if cfg.merge else None)
            self.places[st] = place
            d, _, off = self.walks[st]
            _, self.bridged[st] = brute_pile(kept, ss, d, off, k, self.n_bases, cfg.skip_multi, self.pile)
        self.delta = (delta & 0xFFFFFFFF).astype(np.uint32)
        self.place = place
        self.sites = brute_sites(self.pile, self.depth, self.soff, cfg.min_count, cfg.frac_num, cfg.frac_den, rows=np.flatnonzero(self.pile.any(axis=1)).tolist())
        self.site_cap = lrc.capacity(cfg.site_cap, len(self.sites))
        # the indel events of the kept records, strand behind strand in one list, and their sites against the depth above
        self.all_events, self.ev_made, self.ev_complex = self.events_of(self.kept_tuples)
        self.event_cap = lrc.capacity(cfg.event_cap, len(self.all_events))
        self.events = self.all_events[:self.event_cap]
        self.ev_sites = brute_indel_sites(self.events, self.depth, self.soff, cfg.ev_min_count, cfg.ev_frac_num, cfg.ev_frac_den)
        self.ev_site_cap = lrc.capacity(cfg.ev_site_cap, len(self.ev_sites))

    def events_of(self, recs):
        """brute_events over {strand: records} in the configuration's order into one list -> (the list, events per strand, complex
        junctions per strand)"""
        cfg, out, made, cx = self.cfg, [], {}, {}
        for st in cfg.strands:
            made[st], cx[st] = brute_events(recs[st], self.strand_seqs[st], self.walks[st][2], self.k, self.soff, cfg.skip_multi, cfg.ev_max_indel, out, 1 << 62)
        return out, made, cx

    def host_batch(self):
        """what the host-batch forms (kbo_segments_batch, kbo_place_batch, kbo_pileup_batch) give: every record of every strand asked
        for, the strands' placements merged -> (records in (seq, strand, q_first) order, place, pile, sites)"""
        cfg, k = self.cfg, self.k
        recs = sorted((r for st in cfg.strands for r in self.segs[st]), key=lambda r: (r[0], r[1], r[2]))
        whole = all(self.caps[st] >= len(self.segs[st]) for st in cfg.strands)
        if whole and (cfg.merge or len(cfg.strands) == 1):
            return recs, self.place, self.pile, self.sites
        place, pile = None, np.zeros((self.n_bases, 4), dtype=np.int64)
        for st in cfg.strands:
            place = py_place(np.array(self.segs[st], dtype=locate.SEGMENT_DTYPE), self.n_seqs, k, self.soff, cfg.max_gap, cfg.max_indel, merge_into=place)
            if whole:
                pile = self.pile
            else:
                brute_pile(self.segs[st], self.strand_seqs[st], self.walks[st][0], self.walks[st][2], k, self.n_bases, cfg.skip_multi, pile)
        sites = brute_sites(pile, self.depth, self.soff, cfg.min_count, cfg.frac_num, cfg.frac_den, rows=np.flatnonzero(pile.any(axis=1)).tolist())
        return recs, place, pile, sites

    def host_indels(self):
        """what kbo_indels_batch gives: the sites of the events of every record of every strand asked for, no list cut short"""
        cfg = self.cfg
        if all(self.caps[st] >= len(self.segs[st]) for st in cfg.strands) and self.event_cap >= len(self.all_events):
            return self.ev_sites
        return brute_indel_sites(self.events_of(self.segs)[0], self.depth, self.soff, cfg.ev_min_count, cfg.ev_frac_num, cfg.ev_frac_den)

    def stats(self):
        """what the coverage conditions count, from the generator and the brute force alone"""
        cfg, k = self.cfg, self.k
        st = dict(refused=False, lane_max=False, window=False, multi=False, rev_fwd=False, tile=False, long_gap=False, two_sources=False)
        off = src_offsets(self.seqs).astype(np.int64)
        tiles = range((int(off[-1]) + lrc.TILE - 1) // lrc.TILE)
        st["starts"] = any(((off[:-1] > max(0, t * lrc.TILE - lrc.HALO)) & (off[:-1] < min(off[-1], (t + 1) * lrc.TILE + lrc.HALO))).sum() > lrc.STARTS_TURN
                           for t in tiles)
        for s in cfg.strands:
            recs, kept = self.segs[s], self.segs[s][:self.caps[s]]
            per_seq = np.bincount([r[0] for r in kept], minlength=self.n_seqs) if kept else np.zeros(1, dtype=np.int64)
            st["lane_max"] |= bool(per_seq.max() > lrc.LANE_MAX)
            st["window"] |= bool(per_seq.max() > lrc.WINDOW)
            st["multi"] |= any(r[6] & 12 for r in recs)
            st["rev_fwd"] |= s == 1 and any(r[6] & 1 for r in recs)
            st["tile"] |= any((int(off[r[0]]) + r[2] + k - 1) // lrc.TILE != (int(off[r[0]]) + r[3] + k - 1) // lrc.TILE for r in recs)
            ends = self.soff[1:-1].astype(np.int64)
            st["two_sources"] |= any(((ends > covered(r, k)[0]) & (ends < covered(r, k)[1])).any() for r in recs)
            d = self.walks[s][0]
            for r in kept:
                if r[3] - r[2] > 64 and not (cfg.skip_multi and r[6] & 12):
                    a = np.flatnonzero(d[int(off[r[0]]) + r[2] + k - 1:int(off[r[0]]) + r[3] + k] == k)
                    st["long_gap"] |= bool(len(a) > 1 and np.diff(a).max() > 65)
        st["indel"] = bool((self.place["indel"] > 0).any())
        st["second"] = bool((self.place["second"] > 0).any())
        st["segs_below"] = any(self.caps[s] < len(self.segs[s]) for s in cfg.strands)
        st["sites_below"] = self.site_cap < len(self.sites)
        # the indel calls, on the brute force's full list: an event's records were REV when MINUS differs from "the '-' strand's call"
        ev, at = self.all_events, 0
        st["ev_rev"] = False
        for i, s in enumerate(cfg.strands):
            st["ev_rev"] |= any((e[3] == 1) != (s == 2) for e in ev[at:at + self.ev_made[s]])
            at += self.ev_made[s]
        st["ev_any"] = len(ev) > 0
        st["ev_ins_del"] = any(e[1] & INS for e in ev) and any(not e[1] & INS for e in ev)
        st["ev_long"] = any(e[1] & LONG for e in ev)
        st["ev_complex"] = sum(self.ev_complex.values()) > 0
        st["ev_second"] = len(cfg.strands) == 2 and self.ev_made[cfg.strands[0]] > 0 and self.ev_made[cfg.strands[1]] > 0
        st["ev_below"] = self.event_cap < len(ev)
        st["ev_site2"] = any(s[4] >= 2 for s in self.ev_sites)
        st["ev_sites_below"] = self.ev_site_cap < len(self.ev_sites)
        return st


STATS = {}  # seed -> (Config, World.stats()): what the coverage test counts


def check_host(cfg):
    """the host restatements against the yardsticks, on this configuration's inputs -> World"""
    w = World(cfg)
    k, tag = cfg.k, cfg.describe()
    # kbo_positions_from_ms_host over the oracle's walk of the sources
    assert len(w.occ) == w.oi.n_kmers, tag
    got = np.full(w.oi.n_sets, NONE, dtype=np.uint32)
    for rev in ([0, 1] if w.rc else [0]):
        d, lo, off = walk(w.oi, [revcomp(s) for s in w.srcs] if rev else w.srcs)
        locate.positions_from_ms_host(k, w.oi.n_sets, d, lo, off, w.soff, rev, got)
    assert np.array_equal(got, w.table), "positions_from_ms_host: rows %s | %s" % (np.flatnonzero(got != w.table)[:5], tag)
    delta = np.zeros(w.n_bases + 1, dtype=np.uint32)
    pile = np.zeros((w.n_bases, 4), dtype=np.uint32)
    place = None
    for st in cfg.strands:
        d, lo, off = w.walks[st]
        segs, n = locate.segments_from_ms_host(w.table, k, d, lo, off, cfg.bridge, st, w.caps[st], w.n_bases, delta)
        assert n == len(w.segs[st]) and np.array_equal(segs, w.kept[st]), "segments_from_ms_host strand %d (%d vs %d) | %s" % (st, n, len(w.segs[st]), tag)
        place = locate.place_from_segments_host(segs, w.n_seqs, w.soff, k, cfg.max_gap, cfg.max_indel, merge_into=place if cfg.merge else None)
        same(place, w.places[st])
        cat = np.concatenate(w.strand_seqs[st] + [np.zeros(0, dtype=np.uint8)])
        _, bridged = locate.pileup_from_segments_host(segs, cat, d, off, k, w.n_bases, skip_multi=cfg.skip_multi, pile=pile)
        assert bridged == w.bridged[st], "pileup_from_segments_host strand %d | %s" % (st, tag)
    assert np.array_equal(delta, w.delta) and np.array_equal(np.cumsum(delta[:-1], dtype=np.uint32), w.depth), "delta / depth | " + tag
    assert np.array_equal(pile, w.pile), "pile: %s | %s" % (np.argwhere(pile != w.pile)[:5].tolist(), tag)
    sites, n = locate.pileup_sites_host(pile, w.depth, w.soff, capacity=w.site_cap, min_count=cfg.min_count, frac_num=cfg.frac_num, frac_den=cfg.frac_den)
    assert n == len(w.sites) and site_tuples(sites) == w.sites[:w.site_cap], "pileup_sites_host (%d vs %d) | %s" % (n, len(w.sites), tag)
    # kbo_indels_from_segments_host, strand behind strand into one list of exactly the capacity, and kbo_indel_sites_host over it
    events, n_events = np.zeros(w.event_cap, dtype=locate.INDEL_EVENT_DTYPE), 0
    for st in cfg.strands:
        cat = np.concatenate(w.strand_seqs[st] + [np.zeros(0, dtype=np.uint8)])
        _, after, cx = locate.indels_from_segments_host(w.kept[st], cat, w.walks[st][2], k, w.soff, skip_multi=cfg.skip_multi, max_indel=cfg.ev_max_indel,
                                                        events=events, n_events=n_events)
        assert after - n_events == w.ev_made[st] and cx == w.ev_complex[st], "indels_from_segments_host strand %d (%d vs %d events, %d vs %d complex) | %s" % (
            st, after - n_events, w.ev_made[st], cx, w.ev_complex[st], tag)
        n_events = after
    assert n_events == len(w.all_events) and event_tuples(events[:n_events]) == w.events, "indels_from_segments_host: the list | " + tag
    assert not events[n_events:].view(np.uint32).any(), "nothing behind the count is written | " + tag
    sites, n = locate.indel_sites_host(events, n_events, w.depth, w.soff, capacity=w.ev_site_cap, min_count=cfg.ev_min_count, frac_num=cfg.ev_frac_num,
                                       frac_den=cfg.ev_frac_den)
    assert n == len(w.ev_sites) and event_tuples(sites) == w.ev_sites[:w.ev_site_cap], "indel_sites_host (%d vs %d) | %s" % (n, len(w.ev_sites), tag)
    return w


# ---- the generator
def test_the_generator_is_deterministic():
    for seed in lrc.SEEDS[:12] + (lrc.STRESS_FIRST_SEED,):
        a, b = lrc.config(seed), lrc.config(seed)
        assert a == b and a.describe() == b.describe()
        (s1, q1), (s2, q2) = lrc.make_inputs(a), lrc.make_inputs(b)
        assert len(s1) == len(s2) and len(q1) == len(q2) and all(x.tobytes() == y.tobytes() for x, y in zip(s1 + q1, s2 + q2))
    assert lrc.config(1) != lrc.config(2)


@pytest.mark.parametrize("seed", lrc.SEEDS)
def test_every_configuration_is_well_formed(seed):
    cfg = lrc.config(seed)
    srcs, seqs = lrc.make_inputs(cfg)
    k = cfg.k
    assert 3 <= k <= 255 and any(k in c for c in lrc.K_CLASSES) and 0 <= cfg.bridge <= 255
    assert 1 <= len(srcs) <= 40 and [len(s) for s in srcs] == list(cfg.src_lens) and 1500 <= sum(cfg.src_lens) <= 36000
    assert cfg.strands in ((1,), (2,), (1, 2), (2, 1)) and cfg.how in lrc.HOWS and cfg.shape in lrc.SHAPES
    assert cfg.slab == 0 or 1 <= cfg.slab < 2000 and cfg.min_count >= 1 and cfg.frac_den >= 1
    m = srcs[lrc.main_source(cfg)]
    assert (m == ord("N")).sum() == 1 and sum(1 for b in m.tobytes() if b in b"acgt") == 1
    step = (len(m) - (k + 40)) // 7
    assert m[2 * step:2 * step + k + 20].tobytes() == m[:k + 20].tobytes(), "the exact repeat"
    assert m[3 * step:3 * step + k + 10].tobytes() == revcomp(m[step:step + k + 10]).tobytes(), "the inverted repeat"
    assert m[4 * step:4 * step + k + 23].tobytes() == m[4 * step + 7:4 * step + k + 30].tobytes(), "the tandem repeat"
    assert stretches(m, k) and all(s.dtype == np.uint8 for s in seqs) and len(seqs) >= 5
    lens = np.array([len(s) for s in seqs])
    assert lens.sum() <= 80000
    if cfg.shape == "tiny":
        assert len(seqs) > 400 and lens[0] == 0 and lens[-1] == 0 and (lens == 0).sum() > 20 and lens.max() <= max(2 * k + 100, 360)  # (the reads that share a substitution: up to 2k + 80 bases, an insertion of up to 20)
    if cfg.shape == "long":
        assert sum(n in (lrc.TILE - 1, lrc.TILE + 1, 2 * lrc.TILE - 1, 2 * lrc.TILE + 1, lrc.TILE + lrc.HALO - 1, lrc.TILE + lrc.HALO + 1) for n in lens) >= 3
    if cfg.shape == "reads" and k <= 100:
        assert ((lens >= 80) & (lens <= 180)).sum() >= 60
    if cfg.shape == "junction" and (np.array(cfg.src_lens) > 0).sum() > 1:
        cat = np.concatenate(srcs).tobytes()
        assert cfg.sub_rate or any(q.tobytes() in cat for q in seqs[:40])


# ---- the host restatements, every seed
@pytest.mark.parametrize("seed", lrc.SEEDS)
def test_host_restatements_equal_the_yardsticks(seed):
    cfg = lrc.config(seed)
    try:
        STATS[seed] = (cfg, check_host(cfg).stats())
    except BaseException:
        print("FAILED seed %d: %s" % (seed, cfg.describe()))
        raise


# (what, at least, predicate over (Config, World.stats())): conditions on the seed list, evaluated on the reference's output alone
CONDITIONS = [("k class %d %s" % (i, (cls[0], cls[-1])), 5, (lambda i: lambda c, st: lrc.k_class(c.k) == i)(i)) for i, cls in enumerate(lrc.K_CLASSES)] + [
    ("place wave route: a list longer than kLaneMax", 10, lambda c, st: st["lane_max"]),
    ("a list longer than kWindow", 3, lambda c, st: st["window"]),
    ("MULTI segments", 10, lambda c, st: st["multi"]),
    ("REV segments from a forward walk", 10, lambda c, st: st["rev_fwd"]),
    ("a segment that crosses a tile boundary", 10, lambda c, st: st["tile"]),
    ("a pileup gap longer than 64 windows", 5, lambda c, st: st["long_gap"]),
    ("more than 256 sequence starts in a tile", 5, lambda c, st: st["starts"]),
    ("a segment that spans two sources", 3, lambda c, st: st["two_sources"]),
    ("a place record with indel > 0", 10, lambda c, st: st["indel"]),
    ("a place record with second > 0", 10, lambda c, st: st["second"]),
    ("d_segs capacity below the count", 10, lambda c, st: st["segs_below"]),
    ("d_sites capacity below the count", 10, lambda c, st: st["sites_below"]),
    ("an indel event", 10, lambda c, st: st["ev_any"]),
    ("an insertion and a deletion in one list", 5, lambda c, st: st["ev_ins_del"]),
    ("a LONG insertion", 3, lambda c, st: st["ev_long"]),
    ("an event from REV records", 5, lambda c, st: st["ev_rev"]),
    ("a complex junction", 5, lambda c, st: st["ev_complex"]),
    ("events appended by a second strand", 5, lambda c, st: st["ev_second"]),
    ("d_events capacity below the count", 5, lambda c, st: st["ev_below"]),
    ("an indel site with count >= 2", 5, lambda c, st: st["ev_site2"]),
    ("indel site capacity below the count", 3, lambda c, st: st["ev_sites_below"]),
]


def coverage(stats):
    """[(what, at least, seen)] over {seed: (Config, stats)}, and the seeds refused as a whole"""
    counts = [(what, least, sum(1 for c, st in stats.values() if not st["refused"] and pred(c, st))) for what, least, pred in CONDITIONS]
    return counts, sum(1 for c, st in stats.values() if st["refused"])


def test_the_seed_list_covers_what_it_claims():
    """conditions on the seed list, not measurements, and at most 10 % of the seeds refused as a whole"""
    missing = [s for s in lrc.SEEDS if s not in STATS]
    assert not missing, "seeds that did not run (or failed): %s" % missing[:20]
    counts, refused = coverage(STATS)
    for what, least, n in counts:
        print("%-60s %4d (>= %d)" % (what, n, least))
    print("refused: %d of %d" % (refused, len(STATS)))
    assert refused * 10 <= len(STATS), "%d of %d configurations refused" % (refused, len(STATS))
    short = [(what, n, least) for what, least, n in counts if n < least]
    assert not short, "conditions not met (what, seen, at least): %s" % short
