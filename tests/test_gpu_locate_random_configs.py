"""The third randomized oracle soak, inside the suite: a fixed list of seeded configurations (tests/locate_random_configs.py: k by class
over 3 .. 255, sources of every kind behind an index made on the host, on the device or from parts, batch shapes at the tiles'
boundaries, every call parameter and capacity) through positions, segments, depth, placement, pileup and indels - the device composition
kbo_ms_batch_dev -> kbo_segments_dev (with delta) -> kbo_place_dev -> kbo_pileup_dev -> kbo_indels_dev per strand, kbo_depth_finish_dev,
kbo_pileup_sites_dev and kbo_indel_sites_dev behind them, all on ONE stream, and the host-batch forms kbo_amd.segments, kbo_amd.place,
kbo_amd.pileup and kbo_amd.indels - every
output word compared with brute force over the oracle's index, never with the product itself.  The expected values are World's
(tests/test_locate_random_configs_host.py), which that module has already compared with the CPU restatements of the kernels on every
seed: a failure here points at the device code.

Every device buffer is at exactly its documented figure between guard bands, and the inputs are checked to be unchanged.  The last
test asserts, over all seeds, the coverage conditions of the host module - evaluated on the reference's output, for the seeds that ran
here.

A failure names its seed and prints the configuration: `SOAK=locate SEED=<n> SECONDS=1 python tools/stress.py` replays exactly that
case.  A seed that ends in a GPU fault, an abort or a hang is a finding to be read, not a run to be repeated."""
import numpy as np
import pytest

import kbo_amd
from kbo_amd import locate

import locate_random_configs as lrc
from gpu_helpers import Guarded
from test_gpu_index_locate import _Batch, _build, _geometry
from test_gpu_index_pileup import _Piles
from test_index_indel_host import event_tuples
from test_index_pileup_host import site_tuples
from test_index_place_host import same
from test_locate_random_configs_host import World, coverage

pytestmark = pytest.mark.gpu

SEEN = {}  # seed -> (Config, World.stats()): what the last test of the module counts
SEG, REC = locate.SEGMENT_DTYPE.itemsize, locate.PLACE_DTYPE.itemsize
EV, EV_SITE = locate.INDEL_EVENT_DTYPE.itemsize, locate.INDEL_SITE_DTYPE.itemsize
E_HIP, E_EMPTY_QUERY = -7, -1


def check_config(cfg):
    """one configuration through the device composition and the host-batch forms -> World.stats()"""
    import torch
    w = World(cfg)
    k, tag = cfg.k, cfg.describe()
    assert _geometry() == (lrc.TILE, lrc.HALO)
    # the handle and its table
    sbwt = _build(w.srcs, k, w.rc, cfg.how)
    L = kbo_amd.lib()
    L.kbo_set_positions_slab_bases(cfg.slab)
    try:
        kbo_amd.add_positions(sbwt, w.srcs, add_revcomp=w.rc)
    finally:
        L.kbo_set_positions_slab_bases(0)
    assert sbwt.n_sets() == w.oi.n_sets and np.array_equal(sbwt.source_offsets(), w.soff), tag
    table = sbwt.positions()
    assert np.array_equal(table, w.table), "table: rows %s | %s" % (np.flatnonzero(table != w.table)[:5], tag)
    # the device composition, one stream, one wait
    b = _Batch(sbwt, w.seqs, w.n_bases + 1, seed=cfg.seed)
    p = _Piles(sbwt, w.site_cap, seed=cfg.seed)
    p.delta = b.delta  # (one d_delta: _Batch's, zeroed)
    segs = {st: Guarded("d_segs", SEG * w.caps[st], 1 << 16, b.dev, seed=10 + st) for st in cfg.strands}
    cnts = {st: Guarded("d_n_segs", 8, 4096, b.dev, seed=20 + st) for st in cfg.strands}
    sworks = {st: Guarded("d_work", b.sb, 1 << 16, b.dev, seed=30 + st) for st in cfg.strands}
    pwb = {st: locate.place_work_bytes(b.n, w.caps[st]) for st in cfg.strands}
    pworks = {st: Guarded("d_work", pwb[st], 1 << 16, b.dev, seed=40 + st) for st in cfg.strands}
    place = Guarded("d_place", REC * b.n, 1 << 16, b.dev, seed=50)
    # the indel calls: one list for every strand, its count zeroed once; d_work of kbo_indels_dev by each strand's d_segs capacity
    ecap, icap = w.event_cap, w.ev_site_cap
    events = Guarded("d_events", EV * ecap, 1 << 16, b.dev, seed=60)
    ecnt = Guarded("d_n_events", 8, 4096, b.dev, seed=61, data=np.zeros(8, dtype=np.uint8))
    ewb = {st: locate.indels_work_bytes(w.caps[st]) for st in cfg.strands}
    eworks = {st: Guarded("d_work", ewb[st], 1 << 16, b.dev, seed=62 + st) for st in cfg.strands}
    twb = locate.indel_sites_work_bytes(ecap)
    twork = Guarded("d_work", twb, 1 << 16, b.dev, seed=65)
    isites = Guarded("d_sites", EV_SITE * icap, 1 << 16, b.dev, seed=66)
    icnt = Guarded("d_n_sites", 8, 4096, b.dev, seed=67)
    q0, off0 = b.q.clone(), b.d_off.clone()
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    for i, st in enumerate(cfg.strands):
        cap = w.caps[st]
        b.walk(st, stream)
        locate.segments_dev(sbwt, b.ms, b.lo, b.d_off, b.n, b.total, segs[st].ptr if cap else None, cap, cnts[st].ptr, sworks[st].ptr, b.sb, bridge=cfg.bridge,
                            strand=st, delta=b.delta.ptr, stream=stream)
        locate.place_dev(sbwt, segs[st].ptr if cap else None, cnts[st].ptr, cap, b.n, place.ptr, pworks[st].ptr, pwb[st], max_gap=cfg.max_gap,
                         max_indel=cfg.max_indel, merge=cfg.merge and i > 0, stream=stream)
        locate.pileup_dev(sbwt, b.qr if st == 2 else b.q, b.ms, b.d_off, b.n, b.total, segs[st].ptr if cap else None, cnts[st].ptr, cap, p.pile.ptr,
                          skip_multi=cfg.skip_multi, stream=stream)
        locate.indels_dev(sbwt, b.qr if st == 2 else b.q, b.d_off, b.n, b.total, segs[st].ptr if cap else None, cnts[st].ptr, cap, events.ptr if ecap else None, ecap,
                          ecnt.ptr, eworks[st].ptr, ewb[st], skip_multi=cfg.skip_multi, max_indel=cfg.ev_max_indel, stream=stream)
    p.finish((cfg.min_count, cfg.frac_num, cfg.frac_den), stream)
    locate.indel_sites_dev(sbwt, events.ptr if ecap else None, ecnt.ptr, ecap, p.depth.ptr, isites.ptr if icap else None, icap, icnt.ptr, twork.ptr, twb,
                           min_count=cfg.ev_min_count, frac_num=cfg.ev_frac_num, frac_den=cfg.ev_frac_den, stream=stream)
    torch.cuda.synchronize()
    for g in list(segs.values()) + list(cnts.values()) + list(sworks.values()) + list(pworks.values()) + [place, b.swork, b.cnt] + list(eworks.values()) + [
            events, ecnt, twork, isites, icnt]:
        g.assert_intact(tag)
    assert torch.equal(b.q, q0) and torch.equal(b.d_off, off0), "the inputs are read only | " + tag
    pile, depth, sites, n_sites = p.results(tag)
    for st in cfg.strands:
        n = int(cnts[st].host().view(np.uint64)[0])
        got = segs[st].host().view(locate.SEGMENT_DTYPE)[:min(n, w.caps[st])]
        assert n == len(w.segs[st]) and np.array_equal(got, w.kept[st]), "segments strand %d (%d vs %d): records %s | %s" % (
            st, n, len(w.segs[st]), np.flatnonzero(got != w.kept[st])[:5] if len(got) == len(w.kept[st]) else "-", tag)
    assert np.array_equal(b.delta.host().view(np.uint32), w.delta), "delta | " + tag
    assert np.array_equal(depth, w.depth), "depth: bases %s | %s" % (np.flatnonzero(depth != w.depth)[:5], tag)
    same(place.host().view(locate.PLACE_DTYPE), w.place)
    assert np.array_equal(pile, w.pile), "pile: %s | %s" % (np.argwhere(pile != w.pile)[:5].tolist(), tag)
    assert n_sites == len(w.sites) and site_tuples(sites) == w.sites[:w.site_cap], "sites (%d vs %d) | %s" % (n_sites, len(w.sites), tag)
    n_events, n_isites = int(ecnt.host().view(np.uint64)[0]), int(icnt.host().view(np.uint64)[0])
    got_ev = events.host().view(locate.INDEL_EVENT_DTYPE)[:min(n_events, ecap)]
    want_ev = np.array(w.events, dtype=locate.INDEL_EVENT_DTYPE)
    assert n_events == len(w.all_events) and got_ev.tobytes() == want_ev.tobytes(), "indel events (%d vs %d): %s | %s" % (
        n_events, len(w.all_events), [(i, a, x) for i, (a, x) in enumerate(zip(event_tuples(got_ev), w.events)) if a != x][:4], tag)
    got_is = isites.host().view(locate.INDEL_SITE_DTYPE)[:min(n_isites, icap)]
    want_is = np.array(w.ev_sites[:icap], dtype=locate.INDEL_SITE_DTYPE)
    assert n_isites == len(w.ev_sites) and got_is.tobytes() == want_is.tobytes(), "indel sites (%d vs %d): %s | %s" % (
        n_isites, len(w.ev_sites), [(i, a, x) for i, (a, x) in enumerate(zip(event_tuples(got_is), w.ev_sites)) if a != x][:4], tag)
    # the host-batch forms: a batch with an empty sequence is refused as kbo_find_batch_strands refuses it (kbo_hip.h), so they get
    # the sequences that are not empty, and the records' seq is counted among those
    recs, h_place, h_pile, h_sites = w.host_batch()
    mask = sum(set(cfg.strands))
    keep = np.flatnonzero(np.array([len(s) for s in w.seqs]) > 0)
    seqs = [w.seqs[i] for i in keep]
    if len(keep) < w.n_seqs:
        for call in (lambda: kbo_amd.segments(w.seqs, sbwt, strands=mask), lambda: kbo_amd.place(w.seqs, sbwt, strands=mask),
                     lambda: kbo_amd.pileup(w.seqs, sbwt, strands=mask), lambda: kbo_amd.indels(w.seqs, sbwt, strands=mask)):
            with pytest.raises(kbo_amd.KboError) as ei:
                call()
            assert ei.value.code == E_EMPTY_QUERY, tag
        index = np.cumsum(np.array([len(s) for s in w.seqs]) > 0) - 1
        recs = [(int(index[r[0]]),) + r[1:] for r in recs]
    got, d2 = kbo_amd.segments(seqs, sbwt, bridge=cfg.bridge, strands=mask, depth=True)
    assert [tuple(int(v) for v in r) for r in got.tolist()] == recs and np.array_equal(d2, w.depth), "kbo_amd.segments | " + tag
    same(kbo_amd.place(seqs, sbwt, bridge=cfg.bridge, strands=mask, max_gap=cfg.max_gap, max_indel=cfg.max_indel), h_place[keep])
    s3, d3, p3 = kbo_amd.pileup(seqs, sbwt, bridge=cfg.bridge, strands=mask, skip_multi=cfg.skip_multi, min_count=cfg.min_count, frac_num=cfg.frac_num,
                                frac_den=cfg.frac_den, depth=True, pile=True)
    assert np.array_equal(p3, h_pile) and np.array_equal(d3, w.depth) and site_tuples(s3) == h_sites, "kbo_amd.pileup | " + tag
    s4, d4 = kbo_amd.indels(seqs, sbwt, bridge=cfg.bridge, strands=mask, skip_multi=cfg.skip_multi, max_indel=cfg.ev_max_indel, min_count=cfg.ev_min_count,
                            frac_num=cfg.ev_frac_num, frac_den=cfg.ev_frac_den, depth=True)
    assert np.array_equal(d4, w.depth) and event_tuples(s4) == w.host_indels(), "kbo_amd.indels | " + tag
    return w.stats()


def _gpu_fault(e):
    """a HIP error from the library (KBO_E_HIP) or from torch - not a mismatch, a refusal or a guard band"""
    return (isinstance(e, kbo_amd.KboError) and e.code == E_HIP) or (isinstance(e, RuntimeError) and "hip" in str(e).lower())


def run_seed(seed, oracle=None):
    """what the test of `seed` runs (tools/stress.py calls this too) -> (Config, routes); the oracle is World's own"""
    cfg = lrc.config(seed)
    try:
        st = check_config(cfg)
    except BaseException as e:
        print("FAILED seed %d: %s\n  replay: SOAK=locate SEED=%d SECONDS=1 python tools/stress.py" % (seed, cfg.describe(), seed))
        if _gpu_fault(e):  # nothing more is started on a GPU that has faulted: the session ends here, and the seed is read, not re-run
            pytest.exit("seed %d ended in a GPU fault (%s); no further configuration runs" % (seed, e), returncode=3)
        raise
    SEEN[seed] = (cfg, st)
    return cfg, {"refused"} if st["refused"] else {n for n, v in st.items() if v is True} | {cfg.how, cfg.shape, "k class %d" % lrc.k_class(cfg.k)}


@pytest.mark.parametrize("seed", lrc.SEEDS)
def test_config_equals_the_brute_force(seed):
    run_seed(seed)


def route_tally():
    counts, refused = coverage(SEEN)
    return {what: n for what, _, n in counts}


def test_routes_covered():
    """over all seeds: the coverage conditions of the host module, on the reference's output, for the seeds that ran here"""
    missing = [s for s in lrc.SEEDS if s not in SEEN]
    assert not missing, "seeds that did not run (or failed): %s" % missing[:20]
    print("route tally over %d seeds: %s" % (len(SEEN), route_tally()))
    counts, refused = coverage({s: SEEN[s] for s in lrc.SEEDS})
    for what, least, n in counts:
        print("%-60s %4d (>= %d)" % (what, n, least))
    print("refused: %d of %d" % (refused, len(lrc.SEEDS)))
    assert refused * 10 <= len(lrc.SEEDS), "%d of %d configurations refused" % (refused, len(lrc.SEEDS))
    short = [(what, n, least) for what, least, n in counts if n < least]
    assert not short, "conditions not met (what, seen, at least): %s" % short
