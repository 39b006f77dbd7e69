"""The randomized oracle soak, inside the suite: a fixed list of seeded configurations (tests/random_configs.py: random k by class,
index content, every process-wide knob, batch shapes at the kernels' boundaries) through every batch entry point, each result
compared with the CPU oracle - never with the product itself.  check_config() returns the routes it saw the product take; the last
test of the module asserts, over all seeds, that the kernels the module claims to cover were reached (ROUTE_CONDITIONS).

A failure names its seed and prints the configuration: `SEED=<n> SECONDS=1 python tools/stress.py` replays exactly that case."""
import ctypes

import numpy as np
import pytest

import random_configs as rc
from gpu_helpers import expected_runs

pytestmark = pytest.mark.gpu

SEEN = {}  # seed -> (Config, set of route names): what the last test of the module counts


def apply_knobs(L, cfg):
    kn = cfg.knobs
    L.kbo_set_pair_steps(*kn["pair_steps"])
    L.kbo_set_slab_bytes(kn["slab_bytes"])
    L.kbo_set_force_big_layout(int(kn["big_layout"]))
    L.kbo_set_plan(*kn["plan"])
    L.kbo_set_plan_tuning(*kn["plan_tuning"])
    L.kbo_set_plan_unit_cap_divisor(kn["unit_cap_divisor"])
    L.kbo_set_guided_walk(*kn["guided_walk"])
    L.kbo_set_depth_table(kn["depth_table"])
    L.kbo_set_depth_table_anchors(kn["depth_table_anchors"])
    devs = (ctypes.c_int * 2)(0, 0)  # the batch spread over a device list (both entries GPU 0)
    L.kbo_set_devices(devs if kn["two_workers"] else None, 2 if kn["two_workers"] else 0)


def _seqs(concat, off):
    return [concat[int(off[i]):int(off[i + 1])].tobytes() for i in range(len(off) - 1)]


def _first_bad(got, want, offsets):
    bad = np.flatnonzero(np.asarray(got) != np.asarray(want))
    s = min(int(np.searchsorted(offsets, bad[0], side="right")) - 1, len(offsets) - 2)
    return "sequence %d (len %d), base %d, %d bases differ" % (s, int(offsets[s + 1] - offsets[s]), int(bad[0] - offsets[s]), len(bad))


def _eq(got, want, offsets, what, tag):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, "%s: %s vs %s | %s" % (what, got.shape, want.shape, tag)
    assert np.array_equal(got, want), "%s: %s | %s" % (what, _first_bad(got, want, offsets), tag)


# oracle error code -> the product's (kbo_hip.h): the same reference assertion
_CODE = {-1: -1, -2: -2, -3: -3, -6: -11}


def check_config(cfg, oracle):  # noqa: C901 (one leg after the other)
    """one configuration through every leg it draws, each against the oracle -> the set of routes the product reported"""
    import torch

    import kbo_amd
    from kbo_amd import batch

    L = kbo_amd.lib()
    dev0 = torch.device("cuda:0")
    tag = cfg.describe()
    routes = set()
    apply_knobs(L, cfg)
    contigs, concat, offsets = rc.make_inputs(cfg)
    k, p_err = cfg.k, cfg.max_error_prob
    bopts = kbo_amd.BuildOpts(k=k, num_threads=4, add_revcomp=cfg.add_revcomp)
    sbwt, _ = kbo_amd.build(contigs, bopts)
    oi = oracle.Index.build(contigs, k=k, add_revcomp=cfg.add_revcomp)
    assert (sbwt.k(), sbwt.n_sets(), sbwt.n_kmers()) == (oi.k, oi.n_sets, oi.n_kmers), "index " + tag
    try:
        exp_chars, exp_d = oi.matches_batch(concat, offsets, p_err, n_threads=8, want_d=True)
    except oracle.OracleError as e:  # threshold <= 1: both sides must refuse, for the same reason
        with pytest.raises(kbo_amd.KboError) as ei:
            batch.matches_batch(sbwt, concat, offsets, p_err)
        assert ei.value.code == _CODE.get(e.code, e.code), "refusal code %d vs the oracle's %d | %s" % (ei.value.code, e.code, tag)
        return {"refused"}
    thr = oracle.random_match_threshold(k, oi.n_kmers, 4, p_err)
    exp_map = np.frombuffer(oracle.relative_to_ref(concat, exp_chars), dtype=np.uint8)
    lens = np.diff(offsets.astype(np.int64))
    max_len = int(lens.max())

    if cfg.refuse_len >= 0:  # a sequence of 0 / 1 / 2 bases: the host entry points refuse the batch as the reference panics
        c2, o2 = rc.with_refused(cfg, concat, offsets)
        with pytest.raises(oracle.OracleError) as oe:
            oi.matches_batch(c2, o2, p_err, n_threads=2)
        with pytest.raises(kbo_amd.KboError) as ei:
            batch.matches_batch(sbwt, c2, o2, p_err)
        assert ei.value.code == _CODE.get(oe.value.code, oe.value.code), "refusal code %d vs the oracle's %d | %s" % (ei.value.code, oe.value.code, tag)
        routes.add("refused_len_%d" % cfg.refuse_len)

    # the batch of the device legs: sequences of 0 / 1 / 2 bases among the others (kbo_hip.h: they have no alignment, their bytes are
    # unspecified; every other sequence as without them) - compared over the bases of the sequences of 3 bases or more
    sc, so, keep = rc.with_shorts(cfg, concat, offsets)
    if cfg.short_seqs:
        routes.update("short_%d_in_device_legs" % n for _, n in cfg.short_seqs)

    def leg_a(h, name):
        d, _, _ = batch.ms_batch(h, concat, offsets)
        _eq(d, exp_d, offsets, name + " ms_batch", tag)
        if any(n > 0 for _, n in cfg.short_seqs):  # kbo_ms_batch refuses empty sequences only: 1 and 2 bases have matching statistics
            c1, o1, keep1 = rc.with_shorts(cfg, concat, offsets, lengths=(1, 2))
            want1 = np.zeros(len(c1), dtype=np.uint8)
            want1[keep1] = exp_d
            for i in np.flatnonzero(np.diff(o1.astype(np.int64)) < 3):
                a, b = int(o1[i]), int(o1[i + 1])
                want1[a:b] = oi.matching_statistics(c1[a:b].tobytes())[0]
            d1, _, _ = batch.ms_batch(h, c1, o1)
            _eq(d1, want1, o1, name + " ms_batch with sequences of 1 / 2 bases", tag)
            routes.add("ms_batch_short")
        _eq(batch.matches_batch(h, concat, offsets, p_err), exp_chars, offsets, name + " matches_batch", tag)
        _eq(batch.map_batch(h, concat, offsets, p_err, cfg.dev_format), exp_map if cfg.dev_format else exp_chars, offsets,
            name + " map_batch", tag)

    def leg_i(h, name):
        exp_runs = expected_runs(exp_chars, offsets)
        words, epos, ebyt = batch.pack_reads(concat, offsets)
        runs = batch.matches_batch_sparse(h, words, offsets, epos, ebyt, p_err)
        assert len(runs) == len(exp_runs) and np.array_equal(runs, exp_runs), "%s sparse runs (%d vs %d) | %s" % (name, len(runs), len(exp_runs), tag)
        _eq(batch.expand_sparse(runs, offsets), exp_chars, offsets, name + " sparse expansion", tag)
        _eq(batch.expand_sparse(runs, offsets, ref=concat), exp_map, offsets, name + " sparse expansion, formatted", tag)
        return exp_runs

    def leg_d(h, name):
        """the device-resident entry points over handle h -> the batch that took the one-kernel / two-kernel route"""
        dev = batch.DeviceBatch(h, sc, so, device=dev0, max_error_prob=p_err, format=cfg.dev_format)
        if cfg.dev_zero_sizing:
            dev.max_len = 0
            dev.work_bytes = int(L.kbo_work_bytes(dev.n_seqs, dev.total, 0, k))
            dev.work = torch.zeros(dev.work_bytes // 8 + 2, dtype=torch.int64, device=dev0)
        dev.ms.fill_(0xEE)
        dev.chars.fill_(0xEE)
        dev.run()
        torch.cuda.synchronize()
        want = exp_map if cfg.dev_format else exp_chars
        _eq(dev.ms.cpu().numpy()[:len(sc)][keep], exp_d, offsets, name + " device MS", tag)
        _eq(dev.chars.cpu().numpy()[:len(sc)][keep], want, offsets, name + " device chars (fused %s)" % dev.fused, tag)
        del dev
        # without the MS values: map_reads_kernel's direct form (<= 160 bases) / map_long_kernel (longer), second pass on a tail stream
        tail = torch.cuda.Stream(dev0) if cfg.tail_stream else None
        d2 = batch.DeviceBatch(h, sc, so, device=dev0, max_error_prob=p_err, format=cfg.dev_format, want_ms=False)
        d2.chars.fill_(0xEE)
        d2.run(tail_stream=tail)
        torch.cuda.synchronize()
        _eq(d2.chars.cpu().numpy()[:len(sc)][keep], want, offsets, name + " device chars without MS (fused %s)" % d2.fused, tag)
        return d2

    # ---- a: the host entry points
    leg_a(sbwt, "host")
    routes.add("a")
    lay = sbwt.device_layout()
    routes.add("dtab_order_%d" % lay["dtab_order"])
    if lay["entries_64bit"]:
        routes.add("entries_64bit")

    # ---- b: the packed entry points
    if cfg.legs["packed"]:
        words, epos, ebyt = batch.pack_reads(concat, offsets)
        pout = batch.matches_batch_packed(sbwt, words, offsets, epos, ebyt, p_err)
        _eq(batch.unpack_matches(pout, offsets), exp_chars, offsets, "packed chars", tag)
        prl, pro = batch.find_batch_packed(sbwt, words, offsets, epos, ebyt, kbo_amd.FindOpts(max_error_prob=p_err, max_gap_len=cfg.packed_gap_len))
        er, eo = oracle.run_lengths_batch(exp_chars, offsets, cfg.packed_gap_len)
        assert np.array_equal(pro, eo) and np.array_equal(prl.reshape(-1, 7), er), "packed run lengths | " + tag
        routes.add("b")

    # ---- c: kbo::find with a gap length, every sequence
    if cfg.legs["find"]:
        rles, ro = batch.find_batch(sbwt, concat, offsets, kbo_amd.FindOpts(max_error_prob=p_err, max_gap_len=cfg.gap_len))
        er, eo = oracle.run_lengths_batch(exp_chars, offsets, cfg.gap_len)
        assert np.array_equal(ro, eo), "find: runs per sequence | " + tag
        got = np.asarray(rles, dtype=np.uint64).reshape(-1, 7)
        assert np.array_equal(got, er), "find: run-length records | " + tag
        for s in (0, len(lens) - 1):  # (the batch form of the oracle against its one-sequence form)
            exp = oracle.run_lengths_gapped(exp_chars[int(offsets[s]):int(offsets[s + 1])].tobytes(), cfg.gap_len)
            assert [tuple(int(v) for v in r) for r in got[int(ro[s]):int(ro[s + 1])]] == exp, "find: sequence %d | %s" % (s, tag)
        routes.add("c")

    # ---- d: the device-resident entry points
    if cfg.legs["device"]:
        d2 = leg_d(sbwt, "host-built")
        routes.add("d")
        if not d2.fused:
            routes.add("two_kernel")
        elif max_len <= 160:
            routes.add("map_reads")
            if np.count_nonzero(d2.plan_flags()):
                routes.add("map_reads_second_pass")
        else:
            st = d2.long_stats()
            if st["pieces"] > 0:
                routes.add("map_long")
            if st["flagged"] > 0:
                routes.add("map_long_flagged")
        del d2

    # ---- e: kbo::call over a few sequences as a batch vs the oracle one by one, agreeing on whether the call fails
    if cfg.legs["call"]:
        L.kbo_set_call_device_emit(cfg.call_emit)
        try:
            pick = sorted(set(cfg.call_pick))
            seqs = [concat[int(offsets[x]):int(offsets[x + 1])] for x in pick]
            cc = np.concatenate(seqs)
            co = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.uint64)
            opts = kbo_amd.CallOpts(max_error_prob=p_err, sbwt_build_opts=kbo_amd.BuildOpts(k=k, build_select=True))
            exp_all, ora_err = [], None
            try:
                for s in seqs:
                    exp_all.append(oi.call(s.tobytes(), k, p_err)[0])
            except oracle.OracleError as e:
                ora_err = e
            try:
                got_calls = batch.call_batch(sbwt, cc, co, opts)
            except kbo_amd.KboError as e:
                assert ora_err is not None, "call: the product refused (%s) what the oracle accepted | %s" % (e, tag)
                got_calls = None
            if got_calls is not None:
                assert ora_err is None, "call: the oracle refused (%s) what the product accepted | %s" % (ora_err, tag)
                n_var = 0
                for x, exp_calls, vs in zip(pick, exp_all, got_calls):
                    got = [(v.query_pos, bytes(v.query_chars).decode(), bytes(v.ref_chars).decode()) for v in vs]
                    assert got == exp_calls, "call: sequence %d | %s" % (x, tag)
                    n_var += len(got)
                if n_var:
                    routes.add("call_variants")
            else:
                routes.add("call_refused")
        finally:
            L.kbo_set_call_device_emit(1)
        routes.add("e")

    # ---- f: the same index built by the device; legs a / d through that handle
    if cfg.legs["devbuild"]:
        dsbwt, _ = kbo_amd.build(contigs, bopts, device=0)
        rows, Carr, lcs = dsbwt.export_parts()
        assert (dsbwt.k(), dsbwt.n_sets(), dsbwt.n_kmers()) == (oi.k, oi.n_sets, oi.n_kmers), "device build: sizes | " + tag
        assert list(Carr) == list(oi.C), "device build: C | " + tag
        for c in range(4):
            assert np.array_equal(rows[c], oi.bits(c)), "device build: row %d | %s" % (c, tag)
        assert np.array_equal(lcs, oi.lcs()), "device build: lcs | " + tag
        leg_a(dsbwt, "device-built")
        leg_d(dsbwt, "device-built")
        del dsbwt
        routes.add("f")

    # ---- g, h: kbo::map with any MapOpts / gap filling over a batch with gaps to fill and the lengths that are refused one by one
    if cfg.legs["map_opts"] or cfg.legs["fill_gaps"]:
        oc, oo = rc.make_opts_inputs(cfg, thr)
        oseqs = _seqs(oc, oo)
    if cfg.legs["map_opts"]:
        fill, call, fmt = cfg.map_opts
        mo = kbo_amd.MapOpts(max_error_prob=p_err, fill_gaps=fill, call_variants=call, format=fmt,
                             sbwt_build_opts=kbo_amd.BuildOpts(k=k, build_select=True))
        out, st = batch.map_batch_opts(sbwt, oc, oo, mo)
        gst = batch.fill_gaps_stats() if fill else None
        for i, s in enumerate(oseqs):
            try:
                exp, code = oi.map(s, k, p_err, fill, call, fmt), 0
            except oracle.OracleError as e:
                exp, code = None, _CODE.get(e.code, e.code)
            assert int(st[i]) == code, "map_batch_opts %s: status %d vs the oracle's %d, sequence %d (len %d) | %s" % (cfg.map_opts, st[i], code, i, len(s), tag)
            if code == 0:
                assert out[int(oo[i]):int(oo[i + 1])].tobytes() == exp, "map_batch_opts %s: sequence %d (len %d) | %s" % (cfg.map_opts, i, len(s), tag)
        routes.add("g")
        if gst is not None:
            routes.update(_gap_routes(gst))
    if cfg.legs["fill_gaps"]:
        out, st = batch.fill_gaps_batch(sbwt, oc, oo, thr, p_err)
        gst = batch.fill_gaps_stats()
        for i, s in enumerate(oseqs):
            try:
                if len(s) == 0:
                    raise oracle.OracleError(-1)  # index.rs:248
                d, _, _ = oi.matching_statistics(s)
                tr = oracle.translate_ms_vec(oracle.derandomize_ms_vec(d, k, thr), k, thr)
                exp, code = oi.fill_gaps(tr, s, thr, p_err), 0
            except oracle.OracleError as e:
                exp, code = None, _CODE.get(e.code, e.code)
            assert int(st[i]) == code, "fill_gaps_batch: status %d vs the oracle's %d, sequence %d (len %d) | %s" % (st[i], code, i, len(s), tag)
            if code == 0:
                assert out[int(oo[i]):int(oo[i + 1])].tobytes() == exp, "fill_gaps_batch: sequence %d (len %d) | %s" % (i, len(s), tag)
        routes.add("h")
        routes.update(_gap_routes(gst))

    # ---- i: the sparse form through the slab pipeline, and over device-resident words (reads: the packed-native kernel's output)
    if cfg.legs["sparse"]:
        leg_i(sbwt, "host-built")
        routes.add("i")
    if max_len <= 160 and (cfg.legs["sparse"] or cfg.legs["device"]):
        try:
            pb = batch.PackedDeviceBatch(sbwt, sc, so, device=dev0, max_error_prob=p_err)
            pb.run(tail_stream=torch.cuda.Stream(dev0) if cfg.tail_stream else None)
            torch.cuda.synchronize()
        except kbo_amd.KboError as e:
            assert e.code == -8, "packed-native: %s | %s" % (e, tag)  # KBO_E_UNSUPPORTED: this copy cannot take that kernel
            pb = None
        if pb is not None:
            _eq(pb.chars()[keep], exp_chars, offsets, "packed-native chars", tag)
            routes.add("packed_native")
            if cfg.legs["sparse"]:  # full capacity and a capacity below the count; a sequence of fewer than 3 bases has no run
                full = np.full(len(sc), ord("M"), dtype=np.uint8)
                full[keep] = exp_chars
                exp_runs = expected_runs(full, so, min_len=3)
                for cap in (None, max(1, len(exp_runs) // 3)):
                    runs = pb.sparse_runs(capacity=cap)
                    assert len(runs) == len(exp_runs) and np.array_equal(runs, exp_runs), "sparse_runs capacity %s (%d vs %d runs) | %s" % (cap, len(runs), len(exp_runs), tag)
                routes.add("sparse_dev")
            del pb

    # ---- j: the batch cut into sub-batches through a MapStream, two rounds (slots reused), each against the ORACLE's characters
    if cfg.legs["stream"]:
        slens = np.diff(so.astype(np.int64))
        n = len(slens)
        parts = min(cfg.stream_parts, n)
        cuts = [n * i // parts for i in range(parts + 1)]
        wfull = np.zeros(len(sc), dtype=np.uint8)
        wfull[keep] = exp_map if cfg.dev_format else exp_chars
        subs = []
        for a, b in zip(cuts[:-1], cuts[1:]):
            lo, hi = int(so[a]), int(so[b])
            subs.append((lo, hi, batch.DeviceBatch(sbwt, sc[lo:hi], so[a:b + 1] - so[a], device=dev0, max_error_prob=p_err,
                                                   format=cfg.dev_format, want_ms=False)))
        ms = batch.MapStream(sbwt, max(d.n_seqs for _, _, d in subs), max(d.total for _, _, d in subs), max_len if max_len <= 160 else 0,
                             pipelines=cfg.stream_pipelines)
        try:
            for rnd in range(2):
                for _, _, d in subs:
                    d.chars.fill_(0xEE)
                torch.cuda.synchronize()
                tickets = [ms.submit(d) for _, _, d in subs]
                for i, ((lo, hi, d), t) in enumerate(zip(subs, tickets)):
                    ms.wait(t)
                    kp = keep[lo:hi]
                    _eq(d.chars[:d.total].cpu().numpy()[kp], wfull[lo:hi][kp], so[cuts[i]:cuts[i + 1] + 1] - so[cuts[i]],
                        "map stream (%d pipelines) round %d sub-batch %d (fused %s)" % (cfg.stream_pipelines, rnd, i, d.fused), tag)
            routes.add("stream_fused_reads" if subs[0][2].fused and max_len <= 160 else
                       "stream_fused_long" if subs[0][2].fused else "stream_two_kernel")
        finally:
            ms.close()
        del subs
        routes.add("j")

    # ---- k: a sharded index for the legs that accept one
    if cfg.legs["shards"]:
        try:
            L.kbo_set_index_shards(cfg.shards)
            ssbwt, _ = kbo_amd.build(contigs, bopts)
        finally:
            L.kbo_set_index_shards(0)
        leg_a(ssbwt, "sharded x%d" % ssbwt.shards())
        leg_i(ssbwt, "sharded x%d" % ssbwt.shards())
        if ssbwt.shards() > 1:  # (an index of fewer k-mers than shards stays whole: it does not count as leg k)
            routes.add("k")
        del ssbwt
    return routes


def _gap_routes(stats):
    """kbo_fill_gaps_stats: (gaps found, finished on the device, sequences redone on the host, extension steps)"""
    out = set()
    if stats[1] > 0:
        out.add("gaps_on_device")
    if stats[2] > 0:
        out.add("gaps_redone_on_host")
    return out


def run_seed(seed, oracle):
    """what the test of `seed` runs (tools/stress.py calls this too) -> (Config, routes)"""
    cfg = rc.config(seed)
    try:
        routes = check_config(cfg, oracle)
    except BaseException:
        print("FAILED seed %d: %r\n  replay: SEED=%d SECONDS=1 python tools/stress.py" % (seed, cfg, seed))
        raise
    return cfg, routes


@pytest.mark.parametrize("seed", rc.SEEDS)
def test_config_equals_the_oracle(oracle, seed):
    cfg, routes = run_seed(seed, oracle)
    SEEN[seed] = (cfg, routes)


def _count(pred):
    return sum(1 for cfg, r in SEEN.values() if pred(cfg, r))


def route_tally():
    names = sorted({n for _, r in SEEN.values() for n in r})
    return {n: (_count(lambda c, r: n in r), _count(lambda c, r: n in r and c.k >= 64)) for n in names}


# (what, at least, predicate over (Config, routes)): conditions on the seed list, not measurements
ROUTE_CONDITIONS = [
    ("map_reads_kernel, k >= 64", 10, lambda c, r: "map_reads" in r and c.k >= 64),
    ("map_reads_kernel, k < 64", 10, lambda c, r: "map_reads" in r and c.k < 64),
    ("map_reads_kernel with reads left to its second pass, k >= 64", 5, lambda c, r: "map_reads_second_pass" in r and c.k >= 64),
    ("map_reads_kernel with reads left to its second pass, k < 64", 5, lambda c, r: "map_reads_second_pass" in r and c.k < 64),
    ("map_long_kernel, k >= 64", 10, lambda c, r: "map_long" in r and c.k >= 64),
    ("map_long_kernel, k >= 128", 3, lambda c, r: "map_long" in r and c.k >= 128),
    ("map_long_kernel with flagged pieces, k >= 64", 5, lambda c, r: "map_long_flagged" in r and c.k >= 64),
    ("the two-kernel route", 10, lambda c, r: "two_kernel" in r),
    ("gaps finished on the device", 10, lambda c, r: "gaps_on_device" in r),
    ("gaps finished on the device, k >= 64", 5, lambda c, r: "gaps_on_device" in r and c.k >= 64),
    ("sequences redone on the host by gap filling", 1, lambda c, r: "gaps_redone_on_host" in r),
    ("call_batch with variants, k > 64 (call_depths_kernel)", 5, lambda c, r: "call_variants" in r and c.k > 64),
    ("call_batch with variants, k <= 64", 5, lambda c, r: "call_variants" in r and c.k <= 64),
    ("big layout (64-bit entries)", 3, lambda c, r: "entries_64bit" in r),
    ("two workers", 3, lambda c, r: c.knobs["two_workers"] and "a" in r),
    ("depth table of order 1", 3, lambda c, r: "dtab_order_1" in r),
    ("depth table of order 16", 3, lambda c, r: "dtab_order_16" in r),
    ("plan off", 3, lambda c, r: c.knobs["plan"][0] == 0 and "a" in r),
    # the device forms of legs i and j, which a copy without a depth table refuses or sends down the two-kernel route: as often as the
    # kernels themselves above
    ("the packed-native kernel (kbo_matches_packed_dev)", 10, lambda c, r: "packed_native" in r),
    ("kbo_sparse_runs_dev over its words", 10, lambda c, r: "sparse_dev" in r),
    ("map stream over reads through map_reads_kernel", 10, lambda c, r: "stream_fused_reads" in r),
    ("map stream over reads through map_reads_kernel, k >= 64", 3, lambda c, r: "stream_fused_reads" in r and c.k >= 64),
    ("map stream over long sequences through map_long_kernel", 10, lambda c, r: "stream_fused_long" in r),
    ("map stream over long sequences through map_long_kernel, k >= 64", 3, lambda c, r: "stream_fused_long" in r and c.k >= 64),
    # sequences of 0 / 1 / 2 bases inside the batch of the device legs (d, j, sparse_runs) and of kbo_ms_batch (1 / 2)
    ("a sequence of 0 bases in map_reads_kernel's batch", 3, lambda c, r: "short_0_in_device_legs" in r and "map_reads" in r),
    ("a sequence of 1 base in map_reads_kernel's batch", 3, lambda c, r: "short_1_in_device_legs" in r and "map_reads" in r),
    ("a sequence of 2 bases in map_reads_kernel's batch", 3, lambda c, r: "short_2_in_device_legs" in r and "map_reads" in r),
    ("sequences of 0 - 2 bases in map_reads_kernel's batch, k >= 64", 3, lambda c, r: c.short_seqs and "map_reads" in r and c.k >= 64),
    ("sequences of 0 - 2 bases in map_long_kernel's batch, k >= 64", 3, lambda c, r: c.short_seqs and "map_long" in r and c.k >= 64),
    ("sequences of 0 - 2 bases in a map stream's batches", 5, lambda c, r: c.short_seqs and "j" in r),
    ("sequences of 0 - 2 bases under kbo_sparse_runs_dev", 3, lambda c, r: c.short_seqs and "sparse_dev" in r),
    ("sequences of 1 / 2 bases through kbo_ms_batch", 10, lambda c, r: "ms_batch_short" in r),
] + [("leg %s" % leg, 15, (lambda leg: lambda c, r: leg in r)(leg)) for leg in "fghijk"] + [
    ("device build, %s, revcomp %s" % (name, rcomp), 1, (lambda lo, hi, rcomp: lambda c, r: "f" in r and lo < c.k <= hi and c.add_revcomp == rcomp)(lo, hi, rcomp))
    for name, lo, hi in (("k <= 32", 0, 32), ("k <= 64", 32, 64), ("k <= 128", 64, 128), ("k <= 255", 128, 255)) for rcomp in (False, True)]


def test_routes_covered():
    """over the union of all seeds: every kernel the module claims to cover was reached, and at most 10 % of the seeds were refused"""
    missing = [s for s in rc.SEEDS if s not in SEEN]
    assert not missing, "seeds that did not run (or failed): %s" % missing[:20]
    tally = route_tally()
    print("route tally over %d seeds (configurations, of them k >= 64): %s" % (len(SEEN), tally))
    refused = _count(lambda c, r: r == {"refused"})
    counts = [(what, least, _count(pred)) for what, least, pred in ROUTE_CONDITIONS]
    for what, least, n in counts:
        print("%-70s %4d (>= %d)" % (what, n, least))
    print("refused: %d of %d" % (refused, len(SEEN)))
    assert refused * 10 <= len(SEEN), "%d of %d configurations refused" % (refused, len(SEEN))
    short = [(what, n, least) for what, least, n in counts if n < least]
    assert not short, "routes not reached often enough (what, seen, at least): %s" % short
