"""The randomized oracle soak, inside the suite: a fixed list of seeded configurations (tests/random_configs.py: random k by class,
index content, every process-wide knob, batch shapes at the kernels' boundaries) through every batch entry point, each result
compared with the CPU oracle - never with the product itself.  check_config() returns the routes it saw the product take; the last
test of the module asserts, over all seeds, that the kernels the module claims to cover were reached (ROUTE_CONDITIONS).

Legs a - k: the host entry points, the packed ones, find, the device-resident map, call, the device builder, map_batch_opts, fill_gaps,
the sparse form, map streams, a sharded index.  Legs l - q (random_configs.LEGS2, drawn into Config.extra): the per-sequence summaries
(host, packed, device, map stream, the reducer alone), both strands, kbo_find_batch_dev, a threshold per sequence over the oracle's MS
bytes, run lengths of the oracle's characters on the device, the reverse complement of a device-resident batch.

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

# ---- legs l - q: what the oracle's characters say, in numpy written here - nothing of kbo_amd makes an expected value
SENTINEL = 0x5A5A5A5A  # behind a record buffer's capacity


def _np_summary(oracle, chars, offsets):
    """kbo_aln_summary of every sequence: the numbers of 'M', 'X' and 'R', and the runs the oracle's run_lengths_gapped counts with
    max_gap_len = 0; all zero for a sequence of fewer than 3 bases -> (n, 4) uint32"""
    off = np.asarray(offsets).astype(np.int64)
    out = np.zeros((len(off) - 1, 4), dtype=np.uint32)
    for j, ch in enumerate(b"MXR"):
        cs = np.concatenate([[0], np.cumsum(chars == ch)])
        out[:, j] = cs[off[1:]] - cs[off[:-1]]
    out[:, 3] = np.diff(oracle.run_lengths_batch(chars, offsets, 0)[1].astype(np.int64))
    out[np.diff(off) < 3] = 0
    return out


def _eq_records(got, want, offsets, what, tag):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, "%s: %s vs %s | %s" % (what, got.shape, want.shape, tag)
    if not np.array_equal(got, want):
        bad = np.flatnonzero((got != want).any(axis=1))
        s = int(bad[0])
        raise AssertionError("%s: %d of %d records differ; first: sequence %d (len %d) got %s want %s | %s" % (
            what, len(bad), len(want), s, int(offsets[s + 1] - offsets[s]), got[s].tolist(), want[s].tolist(), tag))


def _eq_runs(got_recs, got_first, want_recs, want_first, what, tag):
    assert np.array_equal(np.asarray(got_first, dtype=np.uint64), np.asarray(want_first, dtype=np.uint64)), "%s: first-run indices | %s" % (what, tag)
    got = np.asarray(got_recs, dtype=np.uint64).reshape(-1, 7)
    assert got.shape == want_recs.shape and np.array_equal(got, want_recs), "%s: run-length records (%d vs %d) | %s" % (what, len(got), len(want_recs), tag)


def _interleave_strands(per, n, strands):
    """kbo_find_batch_strands' layout from the oracle's run lengths per strand: per sequence the '+' runs, then the '-' runs; a strand
    not asked for has none -> (records, rle_offsets uint64[2 n + 1])"""
    counts = np.zeros(2 * n, dtype=np.int64)
    for st in (1, 2):
        if strands & st:
            counts[st - 1::2] = np.diff(per[st][1].astype(np.int64))
    ro = np.concatenate([[0], np.cumsum(counts)])
    recs = np.zeros((int(ro[-1]), 7), dtype=np.uint64)
    for st in (1, 2):
        if strands & st:
            r, o = per[st]
            o = o.astype(np.int64)
            seq = np.repeat(np.arange(n), np.diff(o))
            recs[ro[2 * seq + st - 1] + np.arange(len(r)) - o[seq]] = r
    return recs, ro.astype(np.uint64)


def _n_slabs(offsets, max_bytes):
    """how many slabs the host pipeline cuts a batch into: whole sequences, as many as fit max_bytes and one at least;
    of three slabs or more the last - if it holds 64 sequences or more - in a half and two quarters"""
    off = np.asarray(offsets).astype(np.int64)
    n, s0, slabs = len(off) - 1, 0, []
    while s0 < n:
        s1 = max(int(np.searchsorted(off, off[s0] + max_bytes, side="right")) - 1, s0 + 1)
        slabs.append(s1 - s0)
        s0 = s1
    return len(slabs) + (2 if len(slabs) >= 3 and slabs[-1] >= 64 else 0)


def _slab_routes(L):
    a, b = ctypes.c_uint64(0), ctypes.c_uint64(0)
    assert L.kbo_summary_slab_routes(ctypes.byref(a), ctypes.byref(b)) == 0
    return int(a.value), int(b.value)


def _rle_buffers(torch, dev, capacity):
    """a DeviceBatch's run-length buffers with room for `capacity` records and eight rows of SENTINEL behind them"""
    import kbo_amd
    L = kbo_amd.lib()
    dev.rle_work = torch.zeros(int(L.kbo_run_lengths_work_bytes(dev.n_seqs)) // 4 + 1, dtype=torch.int32, device=dev.device)
    dev.rle_capacity = int(capacity)
    dev.rle_records = torch.full((int(capacity) + 8, 7), SENTINEL, dtype=torch.int32, device=dev.device)


def _rle_total(dev):
    """the number of runs the last run_lengths() / run_find() counted: the last word of its work buffer"""
    n = dev.n_seqs
    return int(dev.rle_work.cpu().numpy().view(np.uint32)[n + 1 + (n + 1 + 1023) // 1024])


def _check_capped(records, capacity, total, want_recs, what, tag):
    """a record buffer of fewer slots than runs: the runs that fit are there, nothing is written behind `capacity`"""
    got = records.cpu().numpy().view(np.uint32)
    assert total == len(want_recs), "%s: %d runs counted, the oracle has %d | %s" % (what, total, len(want_recs), tag)
    m = min(capacity, total)
    assert np.array_equal(got[:m].astype(np.uint64), want_recs[:m]), "%s: the %d records that fit | %s" % (what, m, tag)
    assert (got[capacity:] == SENTINEL).all(), "%s: a record written behind capacity %d | %s" % (what, capacity, tag)


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
    slens = np.diff(so.astype(np.int64))
    ex, legs2 = cfg.extra, cfg.extra["legs"]
    # the oracle's characters in the layout of the device legs' batch, 'M' at the sequences of fewer than 3 bases
    full_chars = np.full(len(sc), ord("M"), dtype=np.uint8)
    full_chars[keep] = exp_chars
    strand_exp = {}

    def strand_expect():
        """leg m's batch - the main batch with the sequences of `minus` reverse-complemented - and what the oracle says of it: its
        matches_batch of that batch ('+') and of the batch's numpy reverse complement ('-').  One oracle call more: a sequence not
        of `minus` is the main batch's (exp_chars) on '+', and the reverse complement of a reverse complement is the sequence itself"""
        if not strand_exp:
            pm = np.repeat(np.asarray(ex["minus"], dtype=bool), lens)
            sin = rc.make_strand_inputs(cfg, concat, offsets)
            srev = rc.revcomp(sin, offsets)
            other = oi.matches_batch(rc.revcomp(concat, offsets), offsets, p_err, n_threads=8)
            assert np.array_equal(srev, np.where(pm, concat, rc.revcomp(concat, offsets)))
            strand_exp["in"] = sin
            strand_exp[1] = np.where(pm, other, exp_chars)
            strand_exp[2] = np.where(pm, exp_chars, other)
            strand_exp["fmt", 1] = np.frombuffer(oracle.relative_to_ref(sin, strand_exp[1]), dtype=np.uint8)
            strand_exp["fmt", 2] = np.frombuffer(oracle.relative_to_ref(srev, strand_exp[2]), dtype=np.uint8)
            per = {st: oracle.run_lengths_batch(strand_exp[st], offsets, ex["strand_gap"]) for st in (1, 2)}
            strand_exp["runs"] = _interleave_strands(per, len(lens), ex["strands"])
            strand_exp["words"] = batch.pack_reads(sin, offsets)
        return strand_exp

    def leg_m(h, name):
        """both strands through handle h, every strand asked for against the oracle"""
        E = strand_expect()
        st, fmt, n = ex["strands"], ex["strand_format"], len(lens)
        fwd, rev = batch.matches_batch_strands(h, E["in"], offsets, p_err, format=fmt, strands=st)
        staged = batch.last_batch_staged_bytes()
        assert (fwd is not None) == bool(st & 1) and (rev is not None) == bool(st & 2), name + " strands | " + tag
        for bit, got in ((1, fwd), (2, rev)):
            if st & bit:
                _eq(got, E["fmt", bit] if fmt else E[bit], offsets, "%s matches_batch_strands %d, format %s, strand %d" % (name, st, fmt, bit), tag)
        if st == 3:  # the batch is staged once: both strands stage what one strand stages - the bases and, per slab, one offset more
            # than it has sequences.  Both strands cut slabs of half the configured size (of 32 KiB at least); kbo_set_slab_bytes takes
            # 64 KiB at least.  Where one strand can be cut the same way the figures are equal; else they differ by the slabs' offsets
            half = max(cfg.knobs["slab_bytes"] // 2, 1 << 15)
            same_cut = half >= 1 << 16
            L.kbo_set_slab_bytes(half if same_cut else cfg.knobs["slab_bytes"])
            try:
                batch.matches_batch_strands(h, E["in"], offsets, p_err, format=fmt, strands=1)
            finally:
                L.kbo_set_slab_bytes(cfg.knobs["slab_bytes"])
            more = 0 if same_cut else 8 * (_n_slabs(offsets, half) - _n_slabs(offsets, cfg.knobs["slab_bytes"]))
            one = batch.last_batch_staged_bytes()
            what = "%s: staged %d bytes for one strand (+ %d of offsets), %d for both | %s" % (name, one, more, staged, tag)
            if same_cut or max_len <= 160:
                assert one + more == staged, what
            else:  # (longer sequences are cut into work items by the slab's size, and those are uploaded: another cut, other items -
                # a few bytes each; a batch staged twice would be all of its bases more)
                assert 2 * abs(staged - one - more) < len(concat), what
        words, epos, ebyt = E["words"]
        wf, wr = batch.matches_batch_packed_strands(h, words, offsets, epos, ebyt, p_err, strands=st)
        for bit, got in ((1, wf), (2, wr)):
            assert (got is not None) == bool(st & bit), name + " packed strands | " + tag
            if st & bit:
                _eq(batch.unpack_matches(got, offsets), E[bit], offsets, "%s matches_batch_packed_strands %d, strand %d" % (name, st, bit), tag)
        exp_recs, exp_ro = E["runs"]
        fo = kbo_amd.FindOpts(max_error_prob=p_err, max_gap_len=ex["strand_gap"])
        for what, (recs, ro) in (("find_batch_strands", batch.find_batch_strands(h, E["in"], offsets, fo, strands=st)),
                                 ("find_batch_packed_strands", batch.find_batch_packed_strands(h, words, offsets, epos, ebyt, fo, strands=st))):
            assert len(ro) == 2 * n + 1, "%s %s: 2 n + 1 offsets | %s" % (name, what, tag)
            _eq_runs(recs, ro, exp_recs, exp_ro, "%s %s %d, gap %d" % (name, what, st, ex["strand_gap"]), tag)

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
    def stream_subs(fmt):
        """the device legs' batch cut into cfg.stream_parts sub-batches -> (cuts, [(first base, last base, DeviceBatch)])"""
        n = len(slens)
        parts = min(cfg.stream_parts, n)
        cuts = [n * i // parts for i in range(parts + 1)]
        subs = []
        for a, b in zip(cuts[:-1], cuts[1:]):
            lo, hi = int(so[a]), int(so[b])
            subs.append((lo, hi, batch.DeviceBatch(sbwt, sc[lo:hi], so[a:b + 1] - so[a], device=dev0, max_error_prob=p_err,
                                                   format=fmt, want_ms=False)))
        return cuts, subs

    if cfg.legs["stream"]:
        cuts, subs = stream_subs(cfg.dev_format)
        wfull = np.zeros(len(sc), dtype=np.uint8)
        wfull[keep] = exp_map if cfg.dev_format else exp_chars
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
        if legs2["strands"]:
            leg_m(ssbwt, "sharded x%d" % ssbwt.shards())
        if ssbwt.shards() > 1:  # (an index of fewer k-mers than shards stays whole: it does not count as leg k)
            routes.add("k")
            if legs2["strands"]:
                routes.add("strands_sharded")
        del ssbwt

    off_t = torch.from_numpy(so.view(np.int64)).to(dev0)
    n_s, total_s, max_s = len(slens), len(sc), int(slens.max())
    cur = torch.cuda.current_stream(dev0)

    # ---- l: per-sequence summaries - map_reads_kernel's and finish_reads_kernel's summary forms, the reducer - against the oracle's
    # characters counted by numpy; the host forms over the main batch (they refuse short sequences), the device forms over the batch
    # with sequences of 0 / 1 / 2 bases, whose records are all zero
    if legs2["summary"]:
        forms = ex["summary_forms"]
        want_d = _np_summary(oracle, full_chars, so)
        assert (want_d[slens < 3] == 0).all()
        if forms["host"] or forms["packed"]:
            want_h = _np_summary(oracle, exp_chars, offsets)
        for packed in (False, True):
            if forms["packed" if packed else "host"]:
                k0, r0 = _slab_routes(L)
                got = batch.summary_batch(sbwt, (concat, offsets), p_err, packed=packed)
                k1, r1 = _slab_routes(L)
                _eq_records(got, want_h, offsets, "summary_batch, packed %s" % packed, tag)
                assert (k1 - k0) + (r1 - r0) > 0, "summary_batch: no slab counted | " + tag
                if k1 > k0:
                    routes.add("summary_host_packed_kernel" if packed else "summary_host_kernel")
                if r1 > r0:
                    routes.add("summary_host_reducer")
        if forms["device"]:
            dev = batch.DeviceBatch(sbwt, sc, so, device=dev0, max_error_prob=p_err, format=False, want_ms=False)
            dev._summary_buffers()
            dev.summary.view(torch.uint8).fill_(0xEE)
            dev.ms.fill_(0xEE)
            dev.run_summary(tail_stream=torch.cuda.Stream(dev0) if cfg.tail_stream else None)
            torch.cuda.synchronize()
            _eq_records(dev.summary_host(), want_d, so, "kbo_summary_batch_dev (fused %s)" % dev.fused, tag)
            if dev.fused and max_s <= 160:  # the one kernel's summary form: no MS value and no character reaches memory
                assert bool((dev.ms == 0xEE).all()), "kbo_summary_batch_dev: the one-kernel route touched d_ms | " + tag
                flags = np.zeros(n_s, dtype=np.uint8)  # (off the summary batch's own work memory)
                kbo_amd.check(L.kbo_plan_flags_dev(n_s, total_s, dev.max_len, k, dev.summary_work.data_ptr(), flags.ctypes.data, cur.cuda_stream))
                routes.add("summary_dev_fused")
                if np.count_nonzero(flags):
                    routes.add("summary_dev_second_pass")
                if lay["dtab_order"] >= 16:
                    routes.add("summary_fused_np18")
                if cfg.short_seqs:
                    routes.add("summary_fused_shorts")
            else:
                routes.add("summary_dev_reducer")
            del dev
        if forms["stream"] and cfg.legs["stream"]:  # summaries and characters in turn through one MapStream, over leg j's sub-batches
            cuts, subs = stream_subs(False)
            ms = batch.MapStream(sbwt, max(d.n_seqs for _, _, d in subs), max(d.total for _, _, d in subs), max_len if max_len <= 160 else 0,
                                 pipelines=cfg.stream_pipelines)
            try:
                tickets = []
                for i, (_, _, d) in enumerate(subs):
                    d.chars.fill_(0xEE)
                    if i % 2 == 0:
                        d._summary_buffers()
                        d.summary.view(torch.uint8).fill_(0xEE)
                torch.cuda.synchronize()
                for i, (_, _, d) in enumerate(subs):
                    tickets.append(ms.submit_summary(d) if i % 2 == 0 else ms.submit(d))
                for i, ((lo, hi, d), t) in enumerate(zip(subs, tickets)):
                    ms.wait(t)
                    sub_off = so[cuts[i]:cuts[i + 1] + 1] - so[cuts[i]]
                    if i % 2 == 0:
                        _eq_records(d.summary_host(), want_d[cuts[i]:cuts[i + 1]], sub_off, "map stream summary, sub-batch %d (fused %s)" % (i, d.fused), tag)
                    else:
                        kp = keep[lo:hi]
                        _eq(d.chars[:d.total].cpu().numpy()[kp], full_chars[lo:hi][kp], sub_off, "map stream characters between summaries, sub-batch %d" % i, tag)
                routes.add("summary_stream")
            finally:
                ms.close()
            del subs
        # the reducer alone over the ORACLE's characters, as bytes and as 2-bit words (M - X R = 0 .. 3)
        code = np.zeros(256, dtype=np.uint8)
        code[ord("-")], code[ord("X")], code[ord("R")] = 1, 2, 3
        d_chars = torch.from_numpy(full_chars).to(dev0)
        d_words = torch.from_numpy(rc.pack_words(code[full_chars], so).view(np.int32)).to(dev0)
        d_wwork = torch.zeros(int(L.kbo_summary_words_work_bytes(n_s)) // 8 + 2, dtype=torch.int64, device=dev0)
        known = max_s if ex["summary_max_len_known"] else 0
        for what in ("kbo_summary_dev", "kbo_summary_words_dev"):
            out = torch.full((n_s, 4), -0x11111112, dtype=torch.int32, device=dev0)  # (0xEE bytes)
            if what == "kbo_summary_dev":
                kbo_amd.check(L.kbo_summary_dev(d_chars.data_ptr(), off_t.data_ptr(), n_s, known, out.data_ptr(), cur.cuda_stream))
            else:
                kbo_amd.check(L.kbo_summary_words_dev(d_words.data_ptr(), off_t.data_ptr(), n_s, known, out.data_ptr(), d_wwork.data_ptr(), cur.cuda_stream))
            torch.cuda.synchronize()
            _eq_records(out.cpu().numpy().view(np.uint32), want_d, so, "%s, max_seq_len %d" % (what, known), tag)
        routes.add("l")

    # ---- m: both strands of the main batch, half of its sequences reverse-complemented, under the configuration's knobs
    if legs2["strands"]:
        leg_m(sbwt, "host-built")
        routes.add("m")
        routes.add("strands_%d" % ex["strands"])

    # ---- n: kbo::find on the device (with max_gap_len = 0 the one kernel counts the runs while the characters are in LDS)
    if legs2["find_dev"]:
        gap = ex["find_dev_gap"]
        er, eo = oracle.run_lengths_batch(exp_chars, offsets, gap)
        cnt = np.zeros(n_s, dtype=np.int64)  # (no run for a sequence of fewer than 3 bases)
        cnt[slens >= 3] = np.diff(eo.astype(np.int64))
        efirst = np.concatenate([[0], np.cumsum(cnt)])
        dev = batch.DeviceBatch(sbwt, sc, so, device=dev0, max_error_prob=p_err, format=False, want_ms=False)
        tail = torch.cuda.Stream(dev0) if cfg.tail_stream else None
        _rle_buffers(torch, dev, len(er))
        dev.chars.fill_(0xEE)
        dev.run_find(gap, tail_stream=tail)
        torch.cuda.synchronize()
        _eq(dev.chars.cpu().numpy()[:len(sc)][keep], exp_chars, offsets, "kbo_find_batch_dev chars (fused %s)" % dev.fused, tag)
        assert _rle_total(dev) == len(er), "kbo_find_batch_dev gap %d: %d runs, the oracle has %d | %s" % (gap, _rle_total(dev), len(er), tag)
        recs, first = dev.run_lengths_host()
        _eq_runs(recs, first, er, efirst, "kbo_find_batch_dev gap %d (fused %s)" % (gap, dev.fused), tag)
        _check_capped(dev.rle_records, len(er), len(er), er, "kbo_find_batch_dev gap %d" % gap, tag)
        if len(er):  # a capacity below the count: every run is counted, only those that fit are written
            cap = int(len(er) * ex["find_dev_cap"])
            _rle_buffers(torch, dev, cap)
            dev.run_find(gap, tail_stream=tail)
            torch.cuda.synchronize()
            _check_capped(dev.rle_records, cap, _rle_total(dev), er, "kbo_find_batch_dev gap %d, capacity %d" % (gap, cap), tag)
        routes.add(("find_dev_fused_reads" if dev.fused and max_s <= 160 else "find_dev_fused_long" if dev.fused else "find_dev_two_kernel")
                   + ("_gap0" if gap == 0 else "_gapped"))
        routes.add("n")
        del dev

    # ---- o: a threshold per sequence over the ORACLE's MS bytes of a real walk (anything - here 0 - at the sequences of fewer than 3 bases)
    if legs2["seq_thresholds"] and k >= 3:
        thr_s = rc.thresholds_of(cfg, thr, n_s)
        ms_full = np.zeros(len(sc), dtype=np.uint8)
        ms_full[keep] = exp_d
        want_c = np.full(len(sc), ord("-"), dtype=np.uint8)
        want_x = np.zeros((n_s, 6), dtype=np.uint32)
        for s in np.flatnonzero(slens >= 3):
            a, b, t = int(so[s]), int(so[s + 1]), int(thr_s[s])
            c = np.frombuffer(oracle.translate_ms_vec(oracle.derandomize_ms_vec(ms_full[a:b], k, t), k, t).encode(), dtype=np.uint8)
            want_c[a:b] = c
            nd = np.flatnonzero(c != ord("-"))
            if len(nd):
                want_x[s, 4:] = (nd[0], nd[-1] + 1)
        want_x[:, :4] = _np_summary(oracle, want_c, so)
        want_f = np.frombuffer(oracle.relative_to_ref(sc, want_c), dtype=np.uint8)
        ms_t, ref_t = torch.from_numpy(ms_full).to(dev0), torch.from_numpy(sc.copy()).to(dev0)
        thr_t = torch.from_numpy(thr_s).to(dev0)
        for min_t in sorted({int(thr_s.min()), 2}, reverse=True):  # the true minimum, and the loosest bound there is
            what = "k %d, thresholds %s, min_threshold %d" % (k, sorted(set(thr_s.tolist())), min_t)
            got = batch.derand_translate_seq(ms_t, off_t, k, thr_t, min_threshold=min_t)
            gotf = batch.derand_translate_seq(ms_t, off_t, k, thr_t, ref=ref_t, min_threshold=min_t)
            gots = batch.derand_summary_seq(ms_t, off_t, k, thr_t, min_threshold=min_t)
            torch.cuda.synchronize()
            _eq(got.cpu().numpy()[keep], want_c[keep], offsets, "derand_translate_seq, " + what, tag)
            _eq(gotf.cpu().numpy()[keep], want_f[keep], offsets, "derand_translate_seq with ref, " + what, tag)
            _eq_records(gots.cpu().numpy().view(np.uint32), want_x, so, "derand_summary_seq, " + what, tag)
        if len(set(thr_s[slens >= 3].tolist())) > 1:
            routes.add("seq_thresholds_differ")
        routes.add("o")

    # ---- p: run lengths of device-resident characters - the ORACLE's, in the layout of the device legs' batch ('M' at the sequences
    # of 1 and 2 bases).  kbo_run_lengths_seq_dev promises every sequence, any byte values, "sequences of length 0 are legal": all of
    # it is compared.  kbo_run_lengths_dev says "device-resident characters" and nothing of empty sequences: its records are compared
    # over the sequences of 1 base or more, and the total it counts (an empty sequence has no character to make a run of)
    if legs2["rle_dev"]:
        gap, mode = ex["rle_gap"], ex["rle_capacity_mode"]
        er, eo = oracle.run_lengths_batch(full_chars, so, gap)
        cap = {"full": len(er), "third": len(er) // 3, "zero": 0}[mode]
        d_chars = torch.zeros(len(sc) + 16, dtype=torch.uint8, device=dev0)
        d_chars[:len(sc)] = torch.from_numpy(full_chars).to(dev0)
        recs, first = batch.run_lengths_seq(d_chars, off_t, gap)
        torch.cuda.synchronize()
        _eq_runs(recs.cpu().numpy().view(np.uint32), first.cpu().numpy().view(np.uint32), er, eo, "run_lengths_seq gap %d" % gap, tag)
        if mode != "full":
            wb = int(L.kbo_run_lengths_seq_work_bytes(n_s, total_s))
            work = torch.zeros(wb // 8 + 2, dtype=torch.int64, device=dev0)
            recs = torch.full((cap + 8, 7), SENTINEL, dtype=torch.int32, device=dev0)
            first = torch.zeros(n_s + 1, dtype=torch.int32, device=dev0)
            kbo_amd.check(L.kbo_run_lengths_seq_dev(d_chars.data_ptr(), off_t.data_ptr(), n_s, total_s, gap, work.data_ptr(), wb, recs.data_ptr(), cap,
                                                    first.data_ptr(), cur.cuda_stream))
            torch.cuda.synchronize()
            fh = first.cpu().numpy().view(np.uint32)
            assert np.array_equal(fh.astype(np.uint64), eo), "kbo_run_lengths_seq_dev capacity %d: first-run indices | %s" % (cap, tag)
            _check_capped(recs, cap, int(fh[-1]), er, "kbo_run_lengths_seq_dev gap %d, capacity %d" % (gap, cap), tag)
        dev = batch.DeviceBatch(sbwt, sc, so, device=dev0, max_error_prob=p_err, format=False, want_ms=False)
        dev.chars[:len(sc)] = d_chars[:len(sc)]
        _rle_buffers(torch, dev, cap)
        dev.run_lengths(max_gap_len=gap)
        torch.cuda.synchronize()
        _check_capped(dev.rle_records, cap, _rle_total(dev), er, "kbo_run_lengths_dev gap %d, capacity %d" % (gap, cap), tag)
        if mode == "full":
            _, first = dev.run_lengths_host()
            some = slens >= 1
            assert np.array_equal(np.asarray(first, dtype=np.uint64)[:-1][some], eo[:-1][some]), "kbo_run_lengths_dev gap %d: first-run indices | %s" % (gap, tag)
        del dev
        routes.add("p")
        routes.add("rle_capacity_" + mode)

    # ---- q: the reverse complement of a device-resident batch, bytes and 2-bit words, empty and 1-base sequences included, against
    # numpy; plain buffers at the documented sizes (behind guard bands: test_gpu_strands.py)
    if legs2["revcomp_dev"]:
        want = rc.revcomp(sc, so)
        d_in = torch.zeros(total_s + 16, dtype=torch.uint8, device=dev0)
        d_in[:total_s] = torch.from_numpy(sc.copy()).to(dev0)
        d_out = torch.full((total_s,), 0xEE, dtype=torch.uint8, device=dev0)
        kbo_amd.check(L.kbo_revcomp_batch_dev(d_in.data_ptr(), off_t.data_ptr(), n_s, total_s, max_s if ex["summary_max_len_known"] else 0,
                                              d_out.data_ptr(), cur.cuda_stream))
        torch.cuda.synchronize()
        _eq(d_out.cpu().numpy(), want, so, "kbo_revcomp_batch_dev", tag)
        words, epos, ebyt, _ = rc.pack_reads(sc, so)
        want_w, want_pos, want_byt, mask = rc.pack_reads(want, so)
        nw, ne = len(words), len(epos)
        d_w = torch.from_numpy(words.view(np.int32)).to(dev0)
        d_wo = torch.full((nw,), -0x11111112, dtype=torch.int32, device=dev0)
        d_scr = torch.zeros(int(L.kbo_revcomp_packed_scratch_bytes(n_s)) // 8 + 2, dtype=torch.int64, device=dev0)
        d_ep = torch.from_numpy(epos.view(np.int64)).to(dev0) if ne else None
        d_eb = torch.from_numpy(ebyt).to(dev0) if ne else None
        d_epo = torch.full((ne,), -1, dtype=torch.int64, device=dev0) if ne else None
        d_ebo = torch.full((ne,), 0xEE, dtype=torch.uint8, device=dev0) if ne else None
        ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        kbo_amd.check(L.kbo_revcomp_packed_dev(d_w.data_ptr(), off_t.data_ptr(), n_s, nw, ptr(d_ep), ptr(d_eb), ne, d_wo.data_ptr(), ptr(d_epo), ptr(d_ebo),
                                               d_scr.data_ptr(), cur.cuda_stream))
        torch.cuda.synchronize()
        got_w = d_wo.cpu().numpy().view(np.uint32)
        bad = np.flatnonzero((got_w & mask) != (want_w & mask))
        assert len(bad) == 0, "kbo_revcomp_packed_dev: %d of %d words differ, first %d: %08x against %08x | %s" % (
            len(bad), nw, int(bad[0]), got_w[bad[0]], want_w[bad[0]], tag)
        if ne:
            assert np.array_equal(d_epo.cpu().numpy().view(np.uint64), want_pos), "kbo_revcomp_packed_dev: mirrored exception positions | " + tag
            assert np.array_equal(d_ebo.cpu().numpy(), want_byt), "kbo_revcomp_packed_dev: complemented exception bytes | " + tag
            routes.add("revcomp_packed_exceptions")
        routes.add("q")
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
    # legs l - q: the summary and run-count forms of map_reads_kernel / finish_reads_kernel, the reducer, both strands, a threshold per sequence
    ("kbo_summary_batch_dev through map_reads_kernel's summary form, k >= 64", 5, lambda c, r: "summary_dev_fused" in r and c.k >= 64),
    ("kbo_summary_batch_dev through map_reads_kernel's summary form, k < 64", 5, lambda c, r: "summary_dev_fused" in r and c.k < 64),
    ("... with reads left to finish_reads_kernel's summary form, k >= 64", 3, lambda c, r: "summary_dev_second_pass" in r and c.k >= 64),
    ("... over a depth table of order 16 or more (the NP = 18 summary forms)", 3, lambda c, r: "summary_fused_np18" in r),
    ("... with sequences of 0 - 2 bases in the batch", 3, lambda c, r: "summary_fused_shorts" in r),
    ("kbo_summary_batch_dev through the reducer, k >= 64", 3, lambda c, r: "summary_dev_reducer" in r and c.k >= 64),
    ("kbo_summary_batch: slabs through the kernel's summary form (bytes in)", 3, lambda c, r: "summary_host_kernel" in r),
    ("kbo_summary_batch_packed: slabs through the kernel's summary form (words in)", 3, lambda c, r: "summary_host_packed_kernel" in r),
    ("kbo_summary_batch[_packed]: slabs through the reducer", 3, lambda c, r: "summary_host_reducer" in r),
    ("summaries and characters in turn through a map stream", 3, lambda c, r: "summary_stream" in r),
    ("kbo_find_batch_dev through map_reads_kernel, gap 0 (runs counted in LDS), k >= 64", 3, lambda c, r: "find_dev_fused_reads_gap0" in r and c.k >= 64),
    ("kbo_find_batch_dev through map_reads_kernel, gap > 0", 3, lambda c, r: "find_dev_fused_reads_gapped" in r),
    ("kbo_find_batch_dev through map_long_kernel, k >= 64", 3,
     lambda c, r: ("find_dev_fused_long_gap0" in r or "find_dev_fused_long_gapped" in r) and c.k >= 64),
    ("kbo_find_batch_dev through the two-kernel route", 3, lambda c, r: "find_dev_two_kernel_gap0" in r or "find_dev_two_kernel_gapped" in r),
    ("both strands at once (strands = 3)", 15, lambda c, r: "strands_3" in r),
    ("both strands at once, k >= 64", 5, lambda c, r: "strands_3" in r and c.k >= 64),
    ("one strand alone, '+' / '-'", 3, lambda c, r: "strands_1" in r or "strands_2" in r),
    ("both strands through a sharded index", 3, lambda c, r: "strands_sharded" in r and c.extra["strands"] == 3),
    ("a threshold per sequence, two or more different ones in the batch", 15, lambda c, r: "seq_thresholds_differ" in r),
    ("run lengths of device characters with room for a third of the records", 3, lambda c, r: "rle_capacity_third" in r),
    ("run lengths of device characters with room for none", 3, lambda c, r: "rle_capacity_zero" in r),
    ("kbo_revcomp_packed_dev with an exception list", 3, lambda c, r: "revcomp_packed_exceptions" in r),
] + [("leg %s" % leg, 15, (lambda leg: lambda c, r: leg in r)(leg)) for leg in "fghijklmnopq"] + [
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
