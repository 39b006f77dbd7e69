"""Indels (kbo_hip.h) on the GPU: kbo_indels_dev and kbo_indel_sites_dev byte for byte against the host forms and the brute force of
tests/test_index_indel_host.py - behind kbo_ms_batch_dev, kbo_segments_dev and kbo_depth_finish_dev on one stream for that file's
planted batch (strand 1 then 2 into one list, twice); over uploaded arrays with every buffer at exactly its figure behind guard bands:
junction pairs across the chunks of the record scan, more events than a radix tile, a group across a chunk of the head scan, groups of
1, 63, 64 and 65, capacities below, at and above the counts, padding far beyond the count, records and events that hold anything;
kbo_indels_batch and kbo_amd.indels against the composed calls, the end-to-end indel set exact; and what is refused."""
import numpy as np
import pytest

import kbo_amd
from kbo_amd import locate

from gpu_helpers import Guarded
from test_gpu_index_locate import _Batch, _build, _dev
from test_index_indel_host import (INS, brute_events, brute_sites, event_tuples, host_lists, indel_world, sample_and_reads, site_tuples,
                                   variant_set, wild_events, wild_records)

pytestmark = pytest.mark.gpu

E_BAD_ARG = -4
SEG, EV, SITE = locate.SEGMENT_DTYPE.itemsize, locate.INDEL_EVENT_DTYPE.itemsize, locate.INDEL_SITE_DTYPE.itemsize
CHUNK, TILE = 2048, 4096  # kScanChunk, kBuildTile
T_ALL, T_HALF = (1, 0, 1), (3, 1, 2)

_handles = {}


def _located(k, rc):
    """a handle over indel_world's sources with its position table, once per world"""
    if (k, rc) not in _handles:
        srcs = indel_world(k, rc)[0]
        _handles[(k, rc)] = kbo_amd.add_positions(_build(srcs, k, rc, "host"), srcs, add_revcomp=rc)
    return _handles[(k, rc)]


class _Lists:
    """d_events, d_n_events, d_delta, d_depth, d_sites, d_n_sites and the d_work of kbo_indels_dev, kbo_depth_finish_dev and
    kbo_indel_sites_dev, each at exactly its figure behind guard bands"""

    def __init__(self, sbwt, seg_cap, event_cap, site_cap, seed=1, events=None, n_events=0, depth=None):
        self.sbwt, self.dev = sbwt, _dev()
        self.n_bases = n = int(kbo_amd.lib().kbo_index_source_bases(sbwt._h))
        self.seg_cap, self.event_cap, self.site_cap = seg_cap, event_cap, site_cap
        self.events = Guarded("d_events", EV * event_cap, 1 << 16, self.dev, seed=seed, data=None if events is None else events[:event_cap].view(np.uint8))
        self.ecnt = Guarded("d_n_events", 8, 4096, self.dev, seed=seed + 1, data=np.array([n_events], dtype=np.uint64).view(np.uint8))
        self.delta = Guarded("d_delta", 4 * (n + 1), 1 << 16, self.dev, seed=seed + 2, data=np.zeros(4 * (n + 1), dtype=np.uint8))
        self.depth = Guarded("d_depth", 4 * n, 1 << 16, self.dev, seed=seed + 3, data=None if depth is None else depth.view(np.uint8))
        self.ewb, self.dwb, self.twb = locate.indels_work_bytes(seg_cap), locate.depth_work_bytes(sbwt), locate.indel_sites_work_bytes(event_cap)
        self.ework = Guarded("d_work", self.ewb, 1 << 16, self.dev, seed=seed + 4)
        self.dwork = Guarded("d_work", self.dwb, 1 << 16, self.dev, seed=seed + 5)
        self.twork = Guarded("d_work", self.twb, 1 << 16, self.dev, seed=seed + 6)
        self.sites = Guarded("d_sites", SITE * site_cap, 1 << 16, self.dev, seed=seed + 7)
        self.cnt = Guarded("d_n_sites", 8, 4096, self.dev, seed=seed + 8)

    def clear(self, seed):
        for i, g in enumerate((self.events, self.ecnt, self.delta, self.ework, self.twork, self.sites, self.cnt)):
            g.fill(seed + i)

    def finish(self, t, stream, depth=True):
        if depth:
            locate.depth_finish_dev(self.sbwt, self.delta.ptr, self.depth.ptr, self.dwork.ptr, self.dwb, stream=stream)
        locate.indel_sites_dev(self.sbwt, self.events.ptr if self.event_cap else None, self.ecnt.ptr, self.event_cap, self.depth.ptr,
                               self.sites.ptr if self.site_cap else None, self.site_cap, self.cnt.ptr, self.twork.ptr, self.twb, min_count=t[0], frac_num=t[1],
                               frac_den=t[2], stream=stream)

    def results(self, what=""):
        """after a synchronise: (events written, their full count, sites written, their full count), every guard band checked"""
        for g in (self.events, self.ecnt, self.delta, self.depth, self.ework, self.dwork, self.twork, self.sites, self.cnt):
            g.assert_intact(what)
        ne, ns = int(self.ecnt.host().view(np.uint64)[0]), int(self.cnt.host().view(np.uint64)[0])
        return (self.events.host().view(locate.INDEL_EVENT_DTYPE)[:min(ne, self.event_cap)].copy(), ne,
                self.sites.host().view(locate.INDEL_SITE_DTYPE)[:min(ns, self.site_cap)].copy(), ns)


@pytest.mark.parametrize("k,rc", [(31, False), (31, True), (96, False)])
def test_planted_batch_behind_the_walk_on_one_stream(k, rc):
    import torch
    sbwt = _located(k, rc)
    stream = torch.cuda.Stream()
    for bridge, skip_multi, max_indel in ((k, True, 16), (255, False, 100), (0, False, 17)):
        h = host_lists(k, rc, bridge, skip_multi, max_indel)  # (checked against brute force field for field where it is made)
        wanted = {}
        for t in (T_ALL, T_HALF):
            want_sites = brute_sites(event_tuples(h["events"]), h["depth"], h["soff"], *t)
            host_sites, hn = locate.indel_sites_host(h["events"], h["n_events"], h["depth"], h["soff"], min_count=t[0], frac_num=t[1], frac_den=t[2])
            assert site_tuples(host_sites) == want_sites and hn == len(want_sites) >= (5 if t == T_ALL else 1)
            wanted[t] = (want_sites, host_sites)
        b = _Batch(sbwt, h["seqs"], h["n_bases"] + 1, seed=k)
        seg_cap = max(len(s) for s in h["segs"]) + 5
        p = _Lists(sbwt, seg_cap, h["n_events"] + 3, len(wanted[T_ALL][0]) + 3)
        segs = {st: Guarded("d_segs", SEG * seg_cap, 1 << 16, b.dev, seed=10 + st) for st in (1, 2)}
        cnts = {st: Guarded("d_n_segs", 8, 4096, b.dev, seed=20 + st) for st in (1, 2)}
        sworks = {st: Guarded("d_work", b.sb, 1 << 16, b.dev, seed=30 + st) for st in (1, 2)}
        seen = []
        for run, t in enumerate((T_ALL, T_ALL, T_HALF)):  # once more over what the run before left in every d_work, then other thresholds
            want_sites, host_sites = wanted[t]
            p.clear(run)
            torch.cuda.synchronize()
            for st in (1, 2):
                b.walk(st, stream)
                locate.segments_dev(sbwt, b.ms, b.lo, b.d_off, b.n, b.total, segs[st].ptr, seg_cap, cnts[st].ptr, sworks[st].ptr, b.sb, bridge=bridge, strand=st,
                                    delta=p.delta.ptr, stream=stream)
                locate.indels_dev(sbwt, b.qr if st == 2 else b.q, b.d_off, b.n, b.total, segs[st].ptr, cnts[st].ptr, seg_cap, p.events.ptr, p.event_cap,
                                  p.ecnt.ptr, p.ework.ptr, p.ewb, skip_multi=skip_multi, max_indel=max_indel, stream=stream)
            p.finish(t, stream)
            torch.cuda.synchronize()
            for g in list(segs.values()) + list(cnts.values()) + list(sworks.values()):
                g.assert_intact()
            for st in (1, 2):
                n = int(cnts[st].host().view(np.uint64)[0])
                assert np.array_equal(segs[st].host().view(locate.SEGMENT_DTYPE)[:n], h["segs"][st - 1])
            ev, ne, sites, ns = p.results("bridge %d run %d" % (bridge, run))
            assert ne == h["n_events"] and len(ev) == ne
            bad = [(i, a, w) for i, (a, w) in enumerate(zip(event_tuples(ev), event_tuples(h["events"]))) if a != w]
            assert not bad, (bridge, run, bad[:5])
            assert np.array_equal(p.depth.host().view(np.uint32), h["depth"])
            assert ns == len(want_sites) and sites.tobytes() == host_sites.tobytes() and site_tuples(sites) == want_sites
            seen.append((ev.tobytes(), sites.tobytes()))
        assert seen[0] == seen[1]


class _Uploaded:
    """host arrays - a walked batch, a record list and a count - on the device, every one behind guard bands"""

    def __init__(self, sbwt, seqs, off, segs, capacity=None, count=None, seed=1):
        import torch
        self.sbwt, self.dev = sbwt, _dev()
        cat = np.concatenate(list(seqs) + [np.zeros(0, dtype=np.uint8)])
        self.n, self.total = len(off) - 1, len(cat)
        self.capacity = len(segs) if capacity is None else capacity
        self.cat = Guarded("d_concat", self.total, 1 << 16, self.dev, seed=seed, data=cat)
        self.off = Guarded("d_offsets", 8 * (self.n + 1), 4096, self.dev, seed=seed + 2, data=np.ascontiguousarray(off, dtype=np.uint64).view(np.uint8))
        self.segs = Guarded("d_segs", SEG * self.capacity, 1 << 16, self.dev, seed=seed + 3, data=np.ascontiguousarray(segs[:self.capacity]).view(np.uint8))
        cnt = np.array([len(segs) if count is None else count], dtype=np.uint64)
        self.cnt = Guarded("d_n_segs", 8, 4096, self.dev, seed=seed + 4, data=cnt.view(np.uint8))
        torch.cuda.synchronize()

    def run(self, p, skip_multi, max_indel, t=None, stream=None):
        import torch
        locate.indels_dev(self.sbwt, self.cat.ptr, self.off.ptr, self.n, self.total, self.segs.ptr if self.capacity else None, self.cnt.ptr, self.capacity,
                          p.events.ptr if p.event_cap else None, p.event_cap, p.ecnt.ptr, p.ework.ptr, p.ewb, skip_multi=skip_multi, max_indel=max_indel,
                          stream=stream)
        if t is not None:
            p.finish(t, stream, depth=False)
        torch.cuda.synchronize()
        for g in (self.cat, self.off, self.segs, self.cnt):
            g.assert_intact()
            assert not g.changed(), "the inputs are read only"


def _two_segment_reads(h, front, n_reads, strand=1):
    """`front` single-segment reads, then n_reads reads of two segments each - the planted reads that give an event, a complex
    junction, an N and none in turn, as `strand`'s walk saw them - as (sequences, offsets, records): the records of a read are its
    records in h, renumbered"""
    names = ["insertion", "deletion", "hp_del", "hp_ins", "ins16", "ins17", "ins_n", "complex", "same_ins0", "across"]
    segs0 = h["segs"][strand - 1]
    seqs, recs = [], []
    for r in range(front + n_reads):
        if r < front:  # a stretch of the first source: one record
            seqs.append(h["srcs"][0][1000:1100].copy())
            one = np.zeros(1, dtype=locate.SEGMENT_DTYPE)
            one[0] = (r, 1, 0, 100 - h["k"], 1000, 1000 + 100 - h["k"], 0)
            recs.append(one)
            continue
        name = names[(r - front) % len(names)]
        i = h["names"].index(name)
        mine = segs0[segs0["seq"] == i].copy()
        assert len(mine) == 2, name
        mine["seq"] = r
        seqs.append(h["strand_seqs"][strand - 1][i])
        recs.append(mine)
    off = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.uint64)
    return seqs, off, np.concatenate(recs)


def test_reverse_records_at_every_place_of_a_lane():
    """a lane takes 8 consecutive records: the '-' walk's REV records of an index with add_revcomp, their pairs at each of the 8 places"""
    import torch
    k = 31
    sbwt = _located(k, True)
    h = dict(host_lists(k, True, k, False, 100), k=k)
    stream = torch.cuda.Stream()
    for front in range(8):
        seqs, off, recs = _two_segment_reads(h, front, 40, strand=2)
        assert (recs["flags"][front:] & 1).all()
        want, n, cx = locate.indels_from_segments_host(recs, np.concatenate(seqs), off, k, h["soff"], skip_multi=False, max_indel=100)
        check = []
        assert brute_events(recs, seqs, off, k, h["soff"], False, 100, check, n)[0] == n == 28 and event_tuples(want[:n]) == check and cx == 4
        p = _Lists(sbwt, len(recs), n, 0, seed=front)
        _Uploaded(sbwt, seqs, off, recs, seed=front).run(p, False, 100, stream=stream)
        ev, ne, _, _ = p.results("front %d" % front)
        bad = [(i, a, w) for i, (a, w) in enumerate(zip(event_tuples(ev), check)) if a != w]
        assert ne == n and not bad, (front, bad[:4])


def test_junction_pairs_across_the_chunks_of_the_record_scan():
    import torch
    k = 31
    sbwt = _located(k, False)
    h = dict(host_lists(k, False, k, False, 100), k=k)
    stream = torch.cuda.Stream()
    for front in (1, 2, 0):
        seqs, off, recs = _two_segment_reads(h, front, 2100)
        if front == 1:
            assert recs["seq"][CHUNK - 1] == recs["seq"][CHUNK], "a junction pair lies on either side of the chunk boundary"
        else:
            assert recs["seq"][CHUNK - 1] != recs["seq"][CHUNK]
        want, n, cx = locate.indels_from_segments_host(recs, np.concatenate(seqs), off, k, h["soff"], skip_multi=False, max_indel=100)
        assert n == 210 * 7 and cx == 210, "seven of ten reads give an event, one a complex junction"
        if front == 1:
            check = []
            assert brute_events(recs[:600], seqs, off, k, h["soff"], False, 100, check, 600)[0] == len(check) and event_tuples(want[:len(check)]) == check
        for ecap in (n + 4, n, n - 1, 5, 0):  # above, at and below the count
            p = _Lists(sbwt, len(recs), ecap, 0, seed=front)
            _Uploaded(sbwt, seqs, off, recs, seed=front).run(p, False, 100, stream=stream)
            ev, ne, _, _ = p.results("front %d, capacity %d" % (front, ecap))
            assert ne == n and ev.tobytes() == want[:min(n, ecap)].tobytes()
        # *d_n_segs above the capacity, the capacity inside a read; appended behind 3 events already there
        cap = CHUNK + 1
        want, n, _ = locate.indels_from_segments_host(recs[:cap], np.concatenate(seqs), off, k, h["soff"], skip_multi=False, max_indel=100, n_events=3,
                                                      capacity=n + 8)
        p = _Lists(sbwt, cap, n + 8, 0, seed=7, n_events=3)
        before = p.events.host().view(locate.INDEL_EVENT_DTYPE)[:3].copy()
        _Uploaded(sbwt, seqs, off, recs, capacity=cap, count=len(recs) + 1000, seed=front).run(p, False, 100, stream=stream)
        ev, ne, _, _ = p.results()
        assert ne == n and ev[3:].tobytes() == want[3:n].tobytes() and ev[:3].tobytes() == before.tobytes()


def _grouped_events(h, n_random, seed):
    """a shuffled list: groups of 1, 63, 64, 65 and CHUNK + 70 identical events - MINUS set in some of each - and n_random events drawn
    from the planted list at random positions"""
    rng = np.random.default_rng(seed)
    rows = []
    for i, size in enumerate((1, 63, 64, 65, CHUNK + 70)):
        key = (100 + 7 * i, (2 + i) | (INS if i % 2 else 0), 0x1B1B1B1B & ((1 << (2 * (2 + i))) - 1) if i % 2 else 0)
        rows += [key + (int(rng.integers(0, 2)),) for _ in range(size)]
    ev = np.zeros(len(rows) + n_random, dtype=locate.INDEL_EVENT_DTYPE)
    for i, r in enumerate(rows):
        ev[i] = r
    own = h["events"][rng.integers(0, len(h["events"]), n_random)]
    own["pos"] = rng.integers(200, h["n_bases"] - 200, n_random)
    own["flags"] = rng.integers(0, 2, n_random)
    ev[len(rows):] = own
    return ev[rng.permutation(len(ev))]


def test_more_events_than_a_radix_tile_and_groups_across_the_head_scan():
    import torch
    k = 31
    sbwt = _located(k, False)
    h = host_lists(k, False, k, False, 100)
    ev = _grouped_events(h, TILE + 9 - (1 + 63 + 64 + 65 + CHUNK + 70), 3)
    assert len(ev) == TILE + 9
    depth = np.random.default_rng(5).integers(0, 200, h["n_bases"]).astype(np.uint32)
    stream = torch.cuda.Stream()
    for t in (T_ALL, (60, 1, 2)):
        want, n = locate.indel_sites_host(ev, len(ev), depth, h["soff"], min_count=t[0], frac_num=t[1], frac_den=t[2])
        assert site_tuples(want) == brute_sites(event_tuples(ev), depth, h["soff"], *t)
        counts = want["count"].tolist()
        assert CHUNK + 70 in counts and (t != T_ALL or {1, 63, 64, 65} <= set(counts)) and 0 < n < len(ev)
        # event capacities at the count, above it by a few and by far (padding sorted and ignored), below it; site capacities
        for ecap, scap in ((len(ev), n), (len(ev) + 5, n + 2), (3 * TILE + 1, n), (len(ev), n // 2), (len(ev), 0), (len(ev) - CHUNK, n), (CHUNK, n)):
            p = _Lists(sbwt, 0, ecap, scap, seed=ecap % 97, events=ev, n_events=len(ev), depth=depth)
            torch.cuda.synchronize()
            p.finish(t, stream, depth=False)
            torch.cuda.synchronize()
            _, ne, sites, ns = p.results("event capacity %d, site capacity %d" % (ecap, scap))
            assert not p.events.changed() and not p.depth.changed() and not p.ecnt.changed(), "the list, its count and d_depth are read only"
            w, wn = (want, n) if ecap >= len(ev) else locate.indel_sites_host(ev[:ecap], len(ev), depth, h["soff"], min_count=t[0], frac_num=t[1], frac_den=t[2])
            assert ns == wn and sites.tobytes() == w[:scap].tobytes(), (ecap, scap)
    # a shuffled list: the same bytes
    again = ev[np.random.default_rng(8).permutation(len(ev))]
    p = _Lists(sbwt, 0, len(ev), n, events=again, n_events=len(ev), depth=depth)
    torch.cuda.synchronize()
    p.finish((60, 1, 2), stream, depth=False)
    torch.cuda.synchronize()
    assert p.results()[2].tobytes() == want.tobytes()
    # an empty list, and a capacity of 0
    for ecap, count in ((16, 0), (0, 0), (0, 9)):
        p = _Lists(sbwt, 0, ecap, 4, events=ev, n_events=count, depth=depth)
        torch.cuda.synchronize()
        p.finish(T_ALL, stream, depth=False)
        torch.cuda.synchronize()
        assert p.results()[3] == 0


def test_records_and_events_that_hold_anything_leave_the_guard_bands_intact():
    import torch
    k = 31
    sbwt = _located(k, False)
    h = host_lists(k, False, 255, False, 100)
    ss, off, soff = h["strand_seqs"][0], h["off"], h["soff"]
    stream = torch.cuda.Stream()
    for trial in range(4):
        wild, _ = wild_records(h, k, 40 + trial)
        if trial == 3:
            wild = wild[np.random.default_rng(trial).permutation(len(wild))]  # (no order at all)
        skip_multi, max_indel = bool(trial & 1), (16, 100, 0xFFFFFFFF, 1000)[trial]
        want, n, _ = locate.indels_from_segments_host(wild, np.concatenate(ss), off, k, soff, skip_multi=skip_multi, max_indel=max_indel)
        p = _Lists(sbwt, len(wild), len(wild), 0, seed=trial)
        _Uploaded(sbwt, ss, off, wild, seed=trial).run(p, skip_multi, max_indel, stream=stream)  # (run() checks the inputs' guard bands)
        ev, ne, _, _ = p.results("trial %d" % trial)
        assert ne == n and ev.tobytes() == want[:n].tobytes()
        we = wild_events(h, 60 + trial)
        for t in (T_ALL, (2, 1, 2)):
            wsites, wn = locate.indel_sites_host(we, len(we), h["depth"], soff, min_count=t[0], frac_num=t[1], frac_den=t[2])
            p = _Lists(sbwt, 0, len(we), wn + 1, seed=trial, events=we, n_events=len(we) + 1000, depth=h["depth"])
            torch.cuda.synchronize()
            p.finish(t, stream, depth=False)
            torch.cuda.synchronize()
            _, _, sites, ns = p.results("wild events %d" % trial)
            assert ns == wn and sites.tobytes() == wsites.tobytes()


@pytest.mark.parametrize("rc", [False, True])
def test_the_host_form_is_the_composition_and_tiled_reads_give_exactly_the_planted_indels(rc):
    k = 31
    srcs = indel_world(k, rc)[0]
    sbwt = _located(k, rc)
    for bridge, skip_multi, max_indel, strands in ((k, True, 16, 3), (255, False, 100, 3), (k, False, 100, 1)):
        h = host_lists(k, rc, bridge, skip_multi, max_indel)
        ev = h["events"] if strands == 3 else h["events"][:h["per_strand"][0]]
        seqs = [s for s in h["seqs"] if len(s)]  # (the host batch refuses an empty sequence, as kbo_find_batch_strands does: it has no record)
        for t in (T_HALF, T_ALL):
            want = brute_sites(event_tuples(ev), h["depth"], h["soff"], *t) if strands == 3 else None
            got, depth = kbo_amd.indels(seqs, sbwt, bridge=bridge, strands=strands, skip_multi=skip_multi, max_indel=max_indel, min_count=t[0], frac_num=t[1],
                                        frac_den=t[2], depth=True)
            if strands == 3:
                assert site_tuples(got) == want and np.array_equal(depth, h["depth"])
            else:
                one, _ = locate.indel_sites_host(ev, len(ev), depth, h["soff"], min_count=t[0], frac_num=t[1], frac_den=t[2])
                assert got.tobytes() == one.tobytes() and len(got)
    reads, want = sample_and_reads(srcs, k)
    sites = kbo_amd.indels(reads, sbwt, strands=3, max_indel=16, min_count=3, frac_num=1, frac_den=2)
    got = kbo_amd.indel_variants(sites, srcs)
    assert variant_set(got) == want and len(got) == len(want)
    assert (sites["n_minus"] * 2 == sites["count"]).all()
    assert len(kbo_amd.indels([srcs[0][:200]], sbwt, strands=3)) == 0


def test_what_is_refused_on_the_device():
    import torch
    k = 31
    sbwt = _located(k, False)
    h = host_lists(k, False, k, True, 16)
    p = _Lists(sbwt, len(h["segs"][0]), 16, 4)
    u = _Uploaded(sbwt, h["strand_seqs"][0], h["off"], h["segs"][0])

    def events(idx=sbwt, wb=p.ewb, **kw):
        locate.indels_dev(idx, u.cat.ptr, u.off.ptr, u.n, u.total, u.segs.ptr, u.cnt.ptr, u.capacity, p.events.ptr, 16, p.ecnt.ptr, p.ework.ptr, wb, **kw)

    def sites(idx=sbwt, wb=p.twb, **kw):
        locate.indel_sites_dev(idx, p.events.ptr, p.ecnt.ptr, 16, p.depth.ptr, p.sites.ptr, 4, p.cnt.ptr, p.twork.ptr, wb, **kw)
    plain = kbo_amd.build([np.frombuffer(b"ACGTTGCATGCATGCAAGTCGATCGATTTGACCATG" * 3, dtype=np.uint8)], kbo_amd.BuildOpts(k=7))[0]
    for f, word in ((lambda: events(wb=p.ewb - 1), "work_bytes"), (lambda: sites(wb=p.twb - 1), "work_bytes"), (lambda: events(max_indel=0), "max_indel"),
                    (lambda: sites(min_count=0), "min_count"), (lambda: sites(frac_den=0), "frac_den"), (lambda: events(idx=plain), "no positions"),
                    (lambda: sites(idx=plain), "no positions"), (lambda: kbo_amd.indels([b"ACGTTGCATGCATGCAAGTCGATCG"], plain), "no positions"),
                    (lambda: kbo_amd.indels(h["seqs"], sbwt, max_indel=0), "max_indel"), (lambda: kbo_amd.indels(h["seqs"], sbwt, bridge=256), "bridge")):
        with pytest.raises(kbo_amd.KboError) as e:
            f()
        assert e.value.code == E_BAD_ARG and word in e.value.message
    torch.cuda.synchronize()
    for g in (p.events, p.ecnt, p.depth, p.sites, p.cnt, p.ework, p.twork, u.cat, u.off, u.segs, u.cnt):
        assert not g.changed(), "a refused call enqueues nothing"
