"""Pileup (kbo_hip.h) on the GPU: kbo_pileup_dev and kbo_pileup_sites_dev byte for byte against the host form and the brute force of
tests/test_index_pileup_host.py - behind kbo_ms_batch_dev, kbo_segments_dev and kbo_depth_finish_dev on one stream for that file's
planted batch (both strands into one pile, in both orders, twice) and for 300 reads, a 5 000-base sequence with a substitution every
97 and sequences of tile + halo bases; over uploaded arrays with every buffer at exactly its figure behind guard bands, *d_n_segs
above capacity, records that hold anything, site capacities below the count and 0; kbo_amd.pileup equal to both and the end-to-end
substitution set exact; and what is refused."""
import numpy as np
import pytest

import kbo_amd
from kbo_amd import locate

from gpu_helpers import Guarded
from test_gpu_index_locate import _Batch, _dev, _located, _reads
from test_index_locate_host import as_tuples, revcomp, src_offsets, walk, world
from test_index_pileup_host import LENS, brute_pile, brute_sites, host_piles, sample_and_reads, site_tuples, snp_set, wild_records

pytestmark = pytest.mark.gpu

E_BAD_ARG = -4
LONG = (9000, 2500, 64, 4)
SEG, SITE = locate.SEGMENT_DTYPE.itemsize, locate.SITE_DTYPE.itemsize
THRESHOLDS = ((3, 1, 2), (1, 0, 1), (2, 1, 1))


class _Piles:
    """d_pile, d_delta, d_depth, d_sites, d_n_sites and the d_work of kbo_depth_finish_dev and kbo_pileup_sites_dev for a handle, each at
    exactly its figure"""

    def __init__(self, sbwt, site_cap, seed=1):
        self.sbwt, self.dev = sbwt, _dev()
        self.n_bases = n = int(kbo_amd.lib().kbo_index_source_bases(sbwt._h))
        self.pile = Guarded("d_pile", 16 * n, 1 << 16, self.dev, seed=seed, data=np.zeros(16 * n, dtype=np.uint8))
        self.delta = Guarded("d_delta", 4 * (n + 1), 1 << 16, self.dev, seed=seed + 1, data=np.zeros(4 * (n + 1), dtype=np.uint8))
        self.depth = Guarded("d_depth", 4 * n, 1 << 16, self.dev, seed=seed + 2)
        self.dwb, self.twb = locate.depth_work_bytes(sbwt), locate.pileup_sites_work_bytes(sbwt)
        assert self.twb == max(16, (4 * ((n + 2047) // 2048) + 15) // 16 * 16), "4 bytes per 2048 source bases rounded up to 16"
        self.dwork = Guarded("d_work", self.dwb, 1 << 16, self.dev, seed=seed + 3)
        self.twork = Guarded("d_work", self.twb, 1 << 16, self.dev, seed=seed + 4)
        self.site_cap = site_cap
        self.sites = Guarded("d_sites", SITE * site_cap, 1 << 16, self.dev, seed=seed + 5)
        self.cnt = Guarded("d_n_sites", 8, 4096, self.dev, seed=seed + 6)

    def clear(self, seed):
        self.pile.fill(seed)
        self.delta.fill(seed + 1)

    def finish(self, t, stream, depth=True):
        if depth:
            locate.depth_finish_dev(self.sbwt, self.delta.ptr, self.depth.ptr, self.dwork.ptr, self.dwb, stream=stream)
        locate.pileup_sites_dev(self.sbwt, self.pile.ptr, self.depth.ptr, self.sites.ptr if self.site_cap else None, self.site_cap, self.cnt.ptr, self.twork.ptr,
                                self.twb, min_count=t[0], frac_num=t[1], frac_den=t[2], stream=stream)

    def results(self, what=""):
        """after a synchronise: (pile, depth, sites written, count), every guard band checked"""
        for g in (self.pile, self.delta, self.depth, self.dwork, self.twork, self.sites, self.cnt):
            g.assert_intact(what)
        n = int(self.cnt.host().view(np.uint64)[0])
        return (self.pile.host().view(np.uint32).reshape(-1, 4).copy(), self.depth.host().view(np.uint32).copy(),
                self.sites.host().view(locate.SITE_DTYPE)[:min(n, self.site_cap)].copy(), n)


def _walked_pipeline(sbwt, b, p, bridge, order, skip_multi, t, seg_cap, stream):
    """kbo_ms_batch_dev -> kbo_segments_dev (with delta) -> kbo_pileup_dev per strand of `order`, kbo_depth_finish_dev and
    kbo_pileup_sites_dev behind them, all on ONE stream with one wait at the end; -> ({strand: records}, pile, depth, sites, count)"""
    import torch
    segs = {st: Guarded("d_segs", SEG * seg_cap, 1 << 16, b.dev, seed=10 + st) for st in order}
    cnts = {st: Guarded("d_n_segs", 8, 4096, b.dev, seed=20 + st) for st in order}
    sworks = {st: Guarded("d_work", b.sb, 1 << 16, b.dev, seed=30 + st) for st in order}
    q0, off0 = b.q.clone(), b.d_off.clone()
    torch.cuda.synchronize()
    for st in order:
        b.walk(st, stream)
        locate.segments_dev(sbwt, b.ms, b.lo, b.d_off, b.n, b.total, segs[st].ptr, seg_cap, cnts[st].ptr, sworks[st].ptr, b.sb, bridge=bridge, strand=st,
                            delta=p.delta.ptr, stream=stream)
        locate.pileup_dev(sbwt, b.qr if st == 2 else b.q, b.ms, b.d_off, b.n, b.total, segs[st].ptr, cnts[st].ptr, seg_cap, p.pile.ptr,
                          skip_multi=skip_multi, stream=stream)
    p.finish(t, stream)
    torch.cuda.synchronize()
    for g in list(segs.values()) + list(cnts.values()) + list(sworks.values()):
        g.assert_intact()
    assert torch.equal(b.q, q0) and torch.equal(b.d_off, off0), "the inputs are read only"
    lists = {}
    for st in order:
        n = int(cnts[st].host().view(np.uint64)[0])
        assert n <= seg_cap
        lists[st] = segs[st].host().view(locate.SEGMENT_DTYPE)[:n].copy()
    return (lists,) + p.results()


@pytest.mark.parametrize("k,rc", [(31, False), (31, True), (96, False)])
def test_planted_batch_behind_the_walk_on_one_stream(k, rc):
    import torch
    sbwt = _located(k, rc, LENS)
    stream = torch.cuda.Stream()
    for bridge, skip_multi in ((k, True), (255, False), (k + 5, False), (0, True)):
        h = host_piles(k, rc, bridge, skip_multi)  # (checked against brute force word for word where it is made)
        t = THRESHOLDS[0]
        want = brute_sites(h["pile"], h["depth"], h["soff"], *t)
        b = _Batch(sbwt, h["seqs"], h["n_bases"] + 1, seed=k)
        p = _Piles(sbwt, len(want) + 3)
        seen = []
        for run, order in enumerate(((1, 2), (2, 1), (2, 1))):  # both orders, and once more over what the run before left in every d_work
            p.clear(run)
            lists, pile, depth, sites, n = _walked_pipeline(sbwt, b, p, bridge, order, skip_multi, t, len(h["segs"][0]) + len(h["segs"][1]) + 5, stream)
            for st in (1, 2):
                assert np.array_equal(lists[st], h["segs"][st - 1])
            assert np.array_equal(pile, h["pile"]), (bridge, order, np.argwhere(pile != h["pile"])[:5])
            assert np.array_equal(depth, h["depth"])
            assert n == len(want) and site_tuples(sites) == want
            seen.append((pile.tobytes(), sites.tobytes()))
        assert seen[0] == seen[1] == seen[2]
        assert np.array_equal(b.ms.cpu().numpy()[:b.total], h["ms"][0]), "the MS bytes are the last walk's ('+'), unchanged"
        if bridge:
            assert pile.any() and len(want) >= 1


@pytest.mark.parametrize("k,rc", [(31, True), (96, False)])
def test_reads_a_long_sequence_and_tile_sized_sequences(k, rc):
    import torch
    srcs, oi, occ, table = world(k, rc, LONG)
    sbwt = _located(k, rc, LONG)
    soff = src_offsets(srcs)
    n_bases = int(soff[-1])
    seqs = _reads(srcs, k, np.random.default_rng(200 + k))
    stream = torch.cuda.Stream()
    walks = {st: walk(oi, [revcomp(s) for s in seqs] if st == 2 else seqs) for st in (1, 2)}
    cats = {1: np.concatenate(seqs), 2: np.concatenate([revcomp(s) for s in seqs])}
    t = THRESHOLDS[1]
    for bridge in (k, 255):
        # the host form, and brute force over its records
        delta = np.zeros(n_bases + 1, dtype=np.uint32)
        hp = np.zeros((n_bases, 4), dtype=np.uint32)
        bp = np.zeros((n_bases, 4), dtype=np.int64)
        host_segs = {}
        for st in (1, 2):
            ss = [revcomp(s) for s in seqs] if st == 2 else seqs
            d, lo, off = walks[st]
            host_segs[st], n = locate.segments_from_ms_host(table, k, d, lo, off, bridge, st, 8000, n_bases, delta)
            assert n == len(host_segs[st])
            _, nb = locate.pileup_from_segments_host(host_segs[st], cats[st], d, off, k, n_bases, skip_multi=False, pile=hp)
            assert nb == brute_pile(host_segs[st], ss, d, off, k, n_bases, False, bp)[1]
        assert np.array_equal(hp, bp)
        hd = np.cumsum(delta[:-1], dtype=np.uint32)
        want = brute_sites(hp, hd, soff, *t)
        long_seq = [r for r in as_tuples(host_segs[1]) if r[0] == 300]
        assert len(long_seq) == 1 and long_seq[0][3] - long_seq[0][2] > 4000, "a substitution every 97 bases: one segment"
        # (52 substitutions from base 50 to base 4 997: all but the last - and at k = 96 the first - have a window on either side)
        assert (hp[1000:6000].sum(axis=1) > 0).sum() >= 50
        b = _Batch(sbwt, seqs, n_bases + 1, seed=k)
        p = _Piles(sbwt, len(want))
        lists, pile, depth, sites, n = _walked_pipeline(sbwt, b, p, bridge, (1, 2), False, t, 8000, stream)
        for st in (1, 2):
            assert np.array_equal(lists[st], host_segs[st])
        assert np.array_equal(pile, hp) and np.array_equal(depth, hd)
        assert n == len(want) >= 50 and site_tuples(sites) == want
        # kbo_amd.pileup is the same composition
        s2, d2, p2 = kbo_amd.pileup(seqs, sbwt, bridge=bridge, strands=3, skip_multi=False, min_count=t[0], frac_num=t[1], frac_den=t[2], depth=True, pile=True)
        assert np.array_equal(s2, sites) and np.array_equal(d2, hd) and np.array_equal(p2, hp)
    # one strand, and the default thresholds
    d, lo, off = walks[1]
    segs, _ = locate.segments_from_ms_host(table, k, d, lo, off, k, 1, 8000, n_bases)
    hp, _ = locate.pileup_from_segments_host(segs, cats[1], d, off, k, n_bases, skip_multi=True)
    one, d1 = kbo_amd.pileup(seqs, sbwt, strands=1, min_count=1, frac_num=0, frac_den=1, depth=True)
    assert one["pos"].tolist() == np.flatnonzero(hp.sum(axis=1)).tolist() and np.array_equal(one["count"], hp[one["pos"]])
    assert site_tuples(kbo_amd.pileup(seqs, sbwt, strands=1)) == brute_sites(hp, d1, soff, 3, 1, 2)


class _Uploaded:
    """host arrays - a walked batch, its MS bytes, a record list and a count - on the device, every one behind guard bands"""

    def __init__(self, sbwt, h, segs, capacity=None, count=None, seed=1):
        import torch
        self.sbwt, self.dev = sbwt, _dev()
        ss = h["strand_seqs"][0]
        cat = np.concatenate(ss)
        self.n, self.total = len(ss), len(cat)
        self.capacity = len(segs) if capacity is None else capacity
        self.cat = Guarded("d_concat", self.total, 1 << 16, self.dev, seed=seed, data=cat)
        self.ms = Guarded("d_ms", self.total, 1 << 16, self.dev, seed=seed + 1, data=h["ms"][0][:self.total])
        self.off = Guarded("d_offsets", 8 * (self.n + 1), 4096, self.dev, seed=seed + 2, data=h["off"].view(np.uint8))
        self.segs = Guarded("d_segs", SEG * self.capacity, 1 << 16, self.dev, seed=seed + 3, data=segs[:self.capacity].view(np.uint8))
        cnt = np.array([len(segs) if count is None else count], dtype=np.uint64)
        self.cnt = Guarded("d_n_segs", 8, 4096, self.dev, seed=seed + 4, data=cnt.view(np.uint8))
        torch.cuda.synchronize()

    def run(self, p, skip_multi, t=None, stream=None):
        import torch
        locate.pileup_dev(self.sbwt, self.cat.ptr, self.ms.ptr, self.off.ptr, self.n, self.total, self.segs.ptr if self.capacity else None, self.cnt.ptr,
                          self.capacity, p.pile.ptr, skip_multi=skip_multi, stream=stream)
        if t is not None:
            p.finish(t, stream, depth=False)
        torch.cuda.synchronize()
        for g in (self.cat, self.ms, self.off, self.segs, self.cnt):
            g.assert_intact()
            assert not g.changed(), "the inputs are read only"


def test_counts_above_capacity_and_site_capacities_below_the_count():
    import torch
    k = 31
    sbwt = _located(k, False, LENS)
    h = host_piles(k, False, 255, False)
    segs = h["segs"][0]
    ss, ms, off = h["strand_seqs"][0], h["ms"][0], h["off"]
    depth = h["depth"]
    for cap in (len(segs), len(segs) - 1, len(segs) // 2, 1, 0):
        want, _ = locate.pileup_from_segments_host(segs[:cap], np.concatenate(ss), ms, off, k, h["n_bases"], skip_multi=False)
        assert np.array_equal(want, brute_pile(segs[:cap], ss, ms, off, k, h["n_bases"], False)[0])
        for t in THRESHOLDS[:2]:
            sites_want = brute_sites(want, depth, h["soff"], *t)
            assert cap < len(segs) or len(sites_want) > (5 if t[1] == 0 else 0)
            for site_cap in (len(sites_want), len(sites_want) // 2, 0):
                p = _Piles(sbwt, site_cap, seed=cap)
                p.depth.data = depth.view(np.uint8)
                p.depth.fill(cap)
                torch.cuda.synchronize()
                _Uploaded(sbwt, h, segs, capacity=cap, count=len(segs) + 1000, seed=cap).run(p, False, t, stream=torch.cuda.Stream())
                pile, _, sites, n = p.results("capacity %d, sites %d" % (cap, site_cap))
                assert np.array_equal(pile, want)
                assert n == len(sites_want) and site_tuples(sites) == sites_want[:site_cap]
                assert not p.depth.changed(), "d_depth is read only"


def test_records_that_hold_anything_leave_the_guard_bands_intact():
    k = 31
    sbwt = _located(k, False, LENS)
    h = host_piles(k, False, 255, False)
    ss, ms, off = h["strand_seqs"][0], h["ms"][0], h["off"]
    for trial in range(4):
        wild, _ = wild_records(h, k, 40 + trial)
        if trial == 3:
            wild = wild[np.random.default_rng(trial).permutation(len(wild))]  # (no order at all)
        skip_multi = bool(trial & 1)
        p = _Piles(sbwt, 0, seed=trial)
        _Uploaded(sbwt, h, wild, seed=trial).run(p, skip_multi)  # (run() checks the inputs' guard bands)
        p.pile.assert_intact("trial %d" % trial)
        pile = p.pile.host().view(np.uint32).reshape(-1, 4)
        want, _ = locate.pileup_from_segments_host(wild, np.concatenate(ss), ms, off, k, h["n_bases"], skip_multi=skip_multi)
        assert np.array_equal(pile, want), "integer atomics: one result whatever the order"


@pytest.mark.parametrize("rc", [False, True])
def test_tiled_reads_give_exactly_the_planted_substitutions(rc):
    k = 31
    srcs = world(k, rc, LENS)[0]
    sbwt = _located(k, rc, LENS)
    reads, want = sample_and_reads(srcs, k)
    sites = kbo_amd.pileup(reads, sbwt, strands=3, min_count=3, frac_num=1, frac_den=2)
    snps = kbo_amd.pileup_snps(sites, srcs, min_count=3, frac_num=1, frac_den=2)
    assert snp_set(snps) == want and len(snps) == len(want)


def test_what_is_refused_on_the_device():
    import torch
    k = 31
    sbwt = _located(k, False, LENS)
    h = host_piles(k, False, k, True)
    p = _Piles(sbwt, 4)
    u = _Uploaded(sbwt, h, h["segs"][0])
    with pytest.raises(kbo_amd.KboError) as e:
        locate.pileup_sites_dev(sbwt, p.pile.ptr, p.depth.ptr, p.sites.ptr, 4, p.cnt.ptr, p.twork.ptr, p.twb - 1)
    assert e.value.code == E_BAD_ARG and "work_bytes" in e.value.message
    for kw in (dict(min_count=0), dict(frac_den=0)):
        with pytest.raises(kbo_amd.KboError) as e:
            locate.pileup_sites_dev(sbwt, p.pile.ptr, p.depth.ptr, p.sites.ptr, 4, p.cnt.ptr, p.twork.ptr, p.twb, **kw)
        assert e.value.code == E_BAD_ARG
    plain = kbo_amd.build([np.frombuffer(b"ACGTTGCATGCATGCAAGTCGATCGATTTGACCATG" * 3, dtype=np.uint8)], kbo_amd.BuildOpts(k=7))[0]
    with pytest.raises(kbo_amd.KboError) as e:
        locate.pileup_dev(plain, u.cat.ptr, u.ms.ptr, u.off.ptr, u.n, u.total, u.segs.ptr, u.cnt.ptr, u.capacity, p.pile.ptr)
    assert e.value.code == E_BAD_ARG and "no positions" in e.value.message
    with pytest.raises(kbo_amd.KboError) as e:
        locate.pileup_sites_dev(plain, p.pile.ptr, p.depth.ptr, p.sites.ptr, 4, p.cnt.ptr, p.twork.ptr, p.twb)
    assert e.value.code == E_BAD_ARG and "no positions" in e.value.message
    for f in (lambda: kbo_amd.pileup([b"ACGTTGCATGCATGCAAGTCGATCG"], plain), lambda: kbo_amd.pileup(h["seqs"], sbwt, min_count=0),
              lambda: kbo_amd.pileup(h["seqs"], sbwt, bridge=256)):
        with pytest.raises(kbo_amd.KboError) as e:
            f()
        assert e.value.code == E_BAD_ARG
    torch.cuda.synchronize()
    for g in (p.pile, p.depth, p.sites, p.cnt, p.twork, u.cat, u.ms, u.off, u.segs, u.cnt):
        assert not g.changed(), "a refused call enqueues nothing"
