"""The second randomized oracle soak, inside the suite: a fixed list of seeded configurations (tests/refset_random_configs.py: k by
class over 1 .. 255, reference sets of every kind and route, batch shapes at the kernels' boundaries, every knob and capacity)
through every reference-set entry point - the host-batch calls and the device-resident and screened forms - each result compared
with the CPU oracle, never with the product itself.  The expected values are World's (tests/test_refset_random_configs_host.py: one
oracle index per reference, the brute-force contracts of the screen, the locus and the cover), which that module has already
compared with the CPU restatements of the kernels on every seed: a failure here points at the device code.

check_config() returns the routes it saw the product take - from RefSet.route, last_routes(), last_wide(), last_best(),
last_prefilter(), last_call() and the screen and stats words - and the last test of the module asserts, over all seeds, that what the
module claims to cover was reached (ROUTE_CONDITIONS).  Every device-resident call runs with d_work at exactly its *_work_bytes figure
and its outputs at exactly their capacities, each between guard bands.

A failure names its seed and prints the configuration: `SOAK=refset SEED=<n> SECONDS=1 python tools/stress.py` replays exactly that
case.  A seed that ends in a GPU fault, an abort or a hang is a finding to be read, not a run to be repeated."""
import ctypes as C

import numpy as np
import pytest

import kbo_amd
from kbo_amd import _capi, refset

import refset_random_configs as rrc
from gpu_helpers import Guarded
from test_gpu_refset_call_dev import DevBatch
from test_refset_random_configs_host import (E_REF_PANIC, E_THRESHOLD_LE_1, E_UNSUPPORTED, HOST_CONDITIONS, I_, L_, NONE_, W_, _K_RANGES, World, as_tuples,
                                             build_set, call_opts, check_set)

pytestmark = pytest.mark.gpu

SEEN = {}  # seed -> (Config, set of route names): what the last test of the module counts
WORDS = {"find": 10, "summary": 9, "best": 12}
DTYPE = {"find": refset.REF_RUN, "summary": refset.REF_SUMMARY, "best": refset.REF_BEST}
BACK = 1 << 16
E_HIP = -7


def _tuples(rec):
    return [tuple(int(v) for v in row) for row in rec.tolist()]


def _words(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32).reshape(len(a), a.dtype.itemsize // 4)


def _capacity(mode, n):
    return {"ample": n + 9, "exact": n, "below": max(0, n - 1 - n // 3)}[mode]


def _refuses(code, fn, *args, **kw):
    with pytest.raises(kbo_amd.KboError) as ei:
        fn(*args, **kw)
    assert ei.value.code == code, (ei.value.code, code)


def dev_records(rs, b, form, arg, strands, capacity, refs_per_slab=0, caps=None, seed=1):
    """one device-resident find / summary / best call, plain (refs_per_slab) or screened (caps = (max_pairs, max_pair_bases)): d_work at
    exactly its figure and the output at exactly `capacity` records (n_seqs for best), behind guards -> (count, records[, screen stats])"""
    import torch
    L = kbo_amd.lib()
    h, s = rs._h, torch.cuda.current_stream(b.device)
    name = "kbo_%s_refset%s_dev" % (form, "" if caps is None else "_screened")
    tail = (refs_per_slab,) if caps is None else tuple(caps)
    if form == "best":
        wb = int(getattr(L, name + "_work_bytes")(h, b.n_seqs, b.total, strands, *tail))
        capacity = b.n_seqs
    else:
        wb = int(getattr(L, name + "_work_bytes")(h, b.n_seqs, b.total, strands, capacity, *tail))
    assert wb > 0, name
    work = Guarded("d_work", wb, 1 << 20, b.device, seed=seed)
    out = Guarded("records", capacity * WORDS[form] * 4, BACK, b.device, seed=seed + 1)
    count = torch.full((1,), 12345, dtype=torch.int64, device=b.device)
    stats = torch.full((4,), -1, dtype=torch.int64, device=b.device)
    o = _capi.FindOpts(*arg) if form == "find" else None
    head = (h, b.d_q.data_ptr(), b.d_off.data_ptr(), b.n_seqs, b.total, C.byref(o) if form == "find" else float(arg), strands, work.ptr, wb)
    mid = (out.ptr,) if form == "best" else (out.ptr if capacity else None, capacity, count.data_ptr())
    end = () if caps is None else tuple(caps) + (stats.data_ptr(),)
    kbo_amd.check(getattr(L, name)(*head, *mid, *end, s.cuda_stream))
    torch.cuda.synchronize()
    work.assert_intact(name)
    out.assert_intact(name)
    n = b.n_seqs if form == "best" else int(count.item())
    rec = np.frombuffer(out.host().tobytes(), dtype=DTYPE[form])[:min(n, capacity)]
    return (n, rec) if caps is None else (n, rec, tuple(int(v) for v in stats.cpu().numpy()))


def dev_call(rs, b, opts, strands, max_variants, max_chars, max_sites, refs_per_slab=0, caps=None, seed=1):
    """kbo_call_refset_dev / _screened_dev behind guard bands -> dict(stats, variants, chars, raw[, screen])"""
    import torch
    L = kbo_amd.lib()
    co = _capi.CallOpts(opts.max_error_prob, opts.sbwt_build_opts._to_c())
    s = torch.cuda.current_stream(b.device)
    if caps is None:
        wb = int(L.kbo_call_refset_dev_work_bytes(rs._h, b.n_seqs, b.total, strands, max_sites, refs_per_slab))
    else:
        wb = int(L.kbo_call_refset_screened_dev_work_bytes(rs._h, b.n_seqs, b.total, strands, max_sites, caps[0], caps[1]))
    assert wb > 0
    work = Guarded("d_work", wb, 1 << 20, b.device, seed=seed)
    var = Guarded("d_variants", max_variants * 24, BACK, b.device, seed=seed + 1)
    chars = Guarded("d_chars", max_chars, BACK, b.device, seed=seed + 2)
    stats = Guarded("d_stats", 64, 4096, b.device, seed=seed + 3)
    head = (rs._h, b.d_q.data_ptr(), b.d_off.data_ptr(), b.n_seqs, b.total, C.byref(co), strands, work.ptr, wb,
            var.ptr if max_variants else None, max_variants, chars.ptr if max_chars else None, max_chars, max_sites, stats.ptr)
    screen = None
    if caps is None:
        kbo_amd.check(L.kbo_call_refset_dev(*head, s.cuda_stream))
    else:
        screen = torch.full((4,), -1, dtype=torch.int64, device=b.device)
        kbo_amd.check(L.kbo_call_refset_screened_dev(*head, caps[0], caps[1], screen.data_ptr(), s.cuda_stream))
    torch.cuda.synchronize()
    for g in (work, var, chars, stats):
        g.assert_intact("call")
    out = dict(stats=tuple(int(v) for v in stats.host().view(np.uint64)), raw=(var, chars))
    n = min(out["stats"][0], max_variants)
    out["variants"] = var.host()[:n * 24].view(refset.REF_VARIANT).copy()
    out["chars"] = chars.host().copy()
    if screen is not None:
        out["screen"] = tuple(int(v) for v in screen.cpu().numpy())
    return out


def variant_arrays(calls):
    """the records and characters of kbo_call_refset from tuples (ref, seq, strand, pos, query_chars, ref_chars) in its order: the
    characters lie back to back in the records' order"""
    rec = np.zeros(len(calls), dtype=refset.REF_VARIANT)
    at, text = 0, []
    for x, (r, s, strand, pos, qc, rf) in enumerate(calls):
        rec[x] = (r, s, strand, pos, at, len(qc), len(rf))
        text += [qc, rf]
        at += len(qc) + len(rf)
    return rec, np.frombuffer(b"".join(text), dtype=np.uint8)


def check_config(cfg, oracle):  # noqa: C901 (one leg after the other)
    """one configuration through every leg it draws, each against the oracle -> the set of routes the product reported"""
    L = kbo_amd.lib()
    L.kbo_set_slab_bytes(cfg.slab_bytes)
    L.kbo_set_refset_record_capacity(cfg.record_capacity)
    try:
        return _check(cfg, oracle)
    finally:  # (the suite's autouse fixture resets neither of these two)
        L.kbo_set_refset_record_capacity(1 << 16)
        refset.set_prefilter_max_bits(0)
        L.kbo_set_slab_bytes(16 << 20)


def _check(cfg, oracle):  # noqa: C901
    import torch
    L = kbo_amd.lib()
    tag = cfg.describe()
    routes = set()
    w = World(cfg, oracle)
    rs = build_set(cfg, w.refs)
    check_set(w, rs)
    strands, p_a, p, gap = cfg.strands, cfg.find_prob, cfg.max_error_prob, cfg.max_gap_len
    routes.update({NONE_: "ref_status", L_: "ref_lds", W_: "ref_wide", I_: "ref_index"}[rs.route(r)] for r in range(w.n_refs))
    if any(rs.route(r) == W_ and w.rows[r] > 65536 for r in range(w.n_refs)):
        routes.add("wide_rows_above_64k")
    fopts = kbo_amd.FindOpts(max_error_prob=p_a, max_gap_len=gap)
    dev_seqs, index = rrc.with_shorts(cfg, w.seqs)
    b = DevBatch(dev_seqs)
    rs.to_device()

    # ---- a set that some call refuses: a threshold of 1 or less (kbo_hip.h: KBO_E_THRESHOLD_LE_1, host and device forms alike)
    if w.refused(p_a) or w.refused(p):
        if w.refused(p_a):
            _refuses(E_THRESHOLD_LE_1, refset.find_refset, w.seqs, rs, fopts, strands)
            _refuses(E_THRESHOLD_LE_1, refset.summary_refset, w.seqs, rs, p_a, strands)
            _refuses(E_THRESHOLD_LE_1, refset.best_refset, w.seqs, rs, p_a, strands)
            if w.packed_only:
                _refuses(E_THRESHOLD_LE_1, refset.find_refset_dev, b.d_q, b.d_off, rs, fopts, strands, 16, cfg.refs_per_slab)
                _refuses(E_THRESHOLD_LE_1, refset.best_refset_dev, b.d_q, b.d_off, rs, p_a, strands, cfg.refs_per_slab)
        if w.refused(p) and w.packed_only:
            _refuses(E_THRESHOLD_LE_1, refset.call_refset, w.seqs, rs, call_opts(cfg), strands)
            _refuses(E_THRESHOLD_LE_1, refset.call_refset_dev, b.d_q, b.d_off, rs, call_opts(cfg), strands, 16, 64, 16, cfg.refs_per_slab)
        return {"refused"}

    # ---- a: find
    exp_find = w.find(p_a, gap, strands)
    got = refset.find_refset(w.seqs, rs, fopts, strands)
    assert _tuples(got) == exp_find, "find_refset: %d vs %d records | %s" % (len(got), len(exp_find), tag)
    lr, lw, lp = refset.last_routes(), refset.last_wide(), refset.last_prefilter()
    assert lr[1] == sum(1 for r in w.queryable if w.route[r] == I_), (lr, tag)
    routes.update(n for n, on in (("lds", lr[0]), ("index", lr[1]), ("wide", lw[0]), ("host_slabs_2", lr[3] > 1), ("screen_ran", lp[3]),
                                  ("screen_skipped_pairs", lp[3] and lp[2] < lp[0]), ("records", len(got))) if on)
    if lr[0] and lw[0] and lr[3] == 1:
        routes.add("mixed_slab")
    routes.add("a")

    # ---- b, c: summary and best
    exp_sum = w.summary(p_a, strands)
    got = refset.summary_refset(w.seqs, rs, p_a, strands)
    assert _tuples(got) == exp_sum, "summary_refset: %d vs %d records | %s" % (len(got), len(exp_sum), tag)
    got = refset.best_refset(w.seqs, rs, p_a, strands)
    assert _tuples(got) == World.best(w.n_seqs, exp_sum), "best_refset | " + tag
    lb = refset.last_best()
    routes.update(n for n, on in (("best_wave", lb[0]), ("best_workgroup", lb[1])) if on)

    def to_dev(records, seq_at=1):
        """records of the host batch in the device legs' batch: `seq` mapped"""
        return [t[:seq_at] + (int(index[t[seq_at]]),) + t[seq_at + 1:] for t in records]

    dev_ok = w.packed_only
    if cfg.short_seqs and dev_ok and cfg.device_leg:
        routes.update("short_%d_in_device_legs" % n for _, n in cfg.short_seqs)

    # ---- a set with a reference of the single-index route: the device forms refuse it, and so does the call
    if not dev_ok:
        assert not rs.packed_only()
        _refuses(E_UNSUPPORTED, refset.find_refset_dev, b.d_q, b.d_off, rs, fopts, strands, 16, cfg.refs_per_slab)
        _refuses(E_UNSUPPORTED, refset.summary_refset_dev, b.d_q, b.d_off, rs, p_a, strands, 16, cfg.refs_per_slab)
        _refuses(E_UNSUPPORTED, refset.best_refset_dev, b.d_q, b.d_off, rs, p_a, strands, cfg.refs_per_slab)
        _refuses(E_UNSUPPORTED, refset.call_refset_dev, b.d_q, b.d_off, rs, call_opts(cfg), strands, 16, 64, 16, cfg.refs_per_slab)
        _refuses(E_UNSUPPORTED, refset.call_refset, w.seqs, rs, call_opts(cfg), strands)
        for fn in (L.kbo_find_refset_dev_work_bytes, L.kbo_summary_refset_dev_work_bytes):
            assert fn(rs._h, b.n_seqs, b.total, strands, 16, 1) == 0
        if cfg.prefilter:
            _refuses(E_UNSUPPORTED, refset.find_refset_dev, b.d_q, b.d_off, rs, fopts, strands, 16, None, None, True, 4, 1 << 20)
        routes.add("dev_refused")

    # the screen's contract in the device legs' batch
    bits_dev = _bits_at(w, cfg, b, index, p_a) if cfg.prefilter else None
    if cfg.prefilter and any(w.m[p_a][r] < rrc.SEED_MIN for r in w.packed):
        routes.add("unscreenable_ref")

    # ---- d: the screen alone
    if cfg.legs["d"] and cfg.prefilter:
        exp_bits = w.screen(p_a, strands)
        got = rs.candidates(w.seqs, p_a, strands)
        assert np.array_equal(got, exp_bits), "candidates: %s | %s" % (np.argwhere(got != exp_bits)[:5].tolist(), tag)
        for r, s, strand in w.hits(p_a, strands):
            assert w.route[r] == I_ or got[r, s, strand - 1], "a pair with a hit without its bit: %s | %s" % ((r, s, strand), tag)
        if dev_ok:
            wb = int(L.kbo_refset_candidates_dev_work_bytes(rs._h, b.n_seqs, b.total, strands))
            n_bits = w.n_refs * b.n_seqs * 2
            work = Guarded("d_work", wb, 1 << 20, b.device, seed=3)
            bits = Guarded("d_bits", (n_bits + 31) // 32 * 4, BACK, b.device, seed=4)
            stats = torch.zeros(4, dtype=torch.int64, device=b.device)
            kbo_amd.check(L.kbo_refset_candidates_dev(rs._h, b.d_q.data_ptr(), b.d_off.data_ptr(), b.n_seqs, b.total, p_a, strands, work.ptr, wb,
                                                      bits.ptr, stats.data_ptr(), torch.cuda.current_stream(b.device).cuda_stream))
            torch.cuda.synchronize()
            work.assert_intact("candidates_dev")
            bits.assert_intact("candidates_dev")
            got = np.unpackbits(bits.host(), bitorder="little")[:n_bits].astype(bool).reshape(bits_dev.shape)
            assert np.array_equal(got, bits_dev), "candidates_dev: %s | %s" % (np.argwhere(got != bits_dev)[:5].tolist(), tag)
            order = np.flatnonzero(bits_dev.ravel())
            assert tuple(int(v) for v in stats.cpu().numpy()) == (len(order), int(b.lens[(order >> 1) % b.n_seqs].sum()), 0, 0), tag
            routes.add("d_dev")
        routes.add("d")

    # ---- e, f: locate and cover over the oracle's runs of find at max_error_prob (the references with entries)
    if cfg.positions and (cfg.legs["e"] or cfg.legs["f"]):
        runs = w.runs(strands)
        n = len(runs)
        cap = _capacity(cfg.capacity, n)
        if dev_ok:
            druns = np.zeros(max(n, cap, 1), dtype=refset.REF_RUN)  # (d_runs holds `capacity` records, n of them given)
            druns[:n] = runs
            druns["seq"][:n] = index[runs["seq"]]
            d_runs = torch.from_numpy(_words(druns).view(np.int32).copy()).to(b.device)
            d_n = torch.tensor([n], dtype=torch.int64, device=b.device)
            s = torch.cuda.current_stream(b.device).cuda_stream
            runs_ptr = d_runs.data_ptr() if cap else None
        if n:
            routes.add("runs_for_e_f")
    if cfg.positions and cfg.legs["e"]:
        exp = w.loci(runs)
        got = refset.locate_refset(w.seqs, rs, runs)
        assert np.array_equal(_words(got), _words(exp)), "locate_refset: record %s | %s" % (np.flatnonzero((_words(got) != _words(exp)).any(axis=1))[:5], tag)
        if dev_ok:
            loci = Guarded("d_loci", cap * 24, BACK, b.device, seed=5)
            kbo_amd.check(L.kbo_locate_refset_dev(rs._h, b.d_q.data_ptr(), b.d_off.data_ptr(), b.n_seqs, b.total, runs_ptr, d_n.data_ptr(), cap,
                                                  loci.ptr if cap else None, s))
            torch.cuda.synchronize()
            loci.assert_intact("locate_dev")
            m = min(n, cap)
            assert np.array_equal(loci.host().view(np.uint32).reshape(cap, 6)[:m], _words(exp)[:m]), "locate_refset_dev | " + tag
            assert bool((loci.buf[m * 24:] == loci.image[loci.front + m * 24:loci.front + loci.n]).all()), "locate_refset_dev wrote behind the count | " + tag
            if cap < n:
                routes.add("locate_dev_truncated")
            routes.add("e_dev")
        routes.add("e")
    if cfg.positions and cfg.legs["f"]:
        exp = w.cover(runs)
        for depth in (True, False):
            got = refset.cover_refset(w.seqs, rs, runs, depth=depth)
            assert (got[0] if depth else got).tobytes() == exp[0].tobytes(), "cover_refset (depth %s) | %s" % (depth, tag)
            if depth:
                assert np.array_equal(got[2], exp[2]) and np.array_equal(got[1], exp[1]), "cover_refset: the profile | " + tag
        if dev_ok:
            expd = exp if cap >= n else w.cover(runs[:cap])
            wb, bases = rs.cover_work_bytes(), rs.cover_bases()
            assert bases == int(exp[2][-1])
            for depth in (True, False):
                covers = Guarded("d_covers", w.n_refs * 48, BACK, b.device, seed=6)
                prof = Guarded("d_depth", bases * 4, BACK, b.device, seed=7) if depth else None
                work = Guarded("d_work", wb, BACK, b.device, seed=8)
                kbo_amd.check(L.kbo_cover_refset_dev(rs._h, b.d_q.data_ptr(), b.d_off.data_ptr(), b.n_seqs, b.total, runs_ptr, d_n.data_ptr(), cap,
                                                     covers.ptr, prof.ptr if depth else None, work.ptr, wb, s))
                torch.cuda.synchronize()
                for g in (covers, prof, work):
                    if g is not None:
                        g.assert_intact("cover_dev")
                assert covers.host().tobytes() == expd[0].tobytes(), "cover_refset_dev (depth %s) | %s" % (depth, tag)
                if depth:
                    assert np.array_equal(prof.host().view(np.uint32), expd[1]), "cover_refset_dev: the profile | " + tag
            if cap < n:
                routes.add("cover_dev_truncated")
            routes.add("f_dev")
        routes.add("f")

    # ---- g: call
    exp_calls = w.calls(strands) if dev_ok else None
    arc = cfg.call_add_revcomp
    if arc and dev_ok and cfg.seed not in rrc.SEEDS and not isinstance(exp_calls, int):
        # a seed beyond the list, where the host module has not shown that the flag changes no byte: the oracle, which does not model
        # the flag, judges it only if the CPU restatement says the same of this seed
        a, c = (refset.call_refset(w.seqs, rs, call_opts(cfg, x), strands, host=True) for x in (False, True))
        if a[0].tobytes() != c[0].tobytes() or a[1].tobytes() != c[1].tobytes():
            arc = False
            routes.add("add_revcomp_dropped")
    if cfg.legs["g"] and dev_ok:
        if isinstance(exp_calls, int):
            _refuses(E_REF_PANIC, refset.call_refset, w.seqs, rs, call_opts(cfg), strands)
            routes.add("call_panic")
        else:
            variants, chars = refset.call_refset(w.seqs, rs, call_opts(cfg, arc), strands)
            assert as_tuples(variants, chars) == exp_calls, "call_refset: %d vs %d records | %s" % (len(variants), len(exp_calls), tag)
            lc = refset.last_call()
            assert lc[3] == len(exp_calls)
            routes.update(n for n, on in (("g_variants", len(exp_calls)), ("g_sites", lc[2])) if on)
            if arc and exp_calls:
                routes.add("g_add_revcomp")
        routes.add("g")

    # the caps of the screened forms, from the contract's bitmap
    def caps_of(prob_bits):
        order = np.flatnonzero(prob_bits.ravel())
        lens = b.lens[(order >> 1) % b.n_seqs]
        n_cand, bases = len(order), int(lens.sum())
        if cfg.caps == "pairs" and n_cand > 1:
            caps = (n_cand // 2, bases + 100)
        elif cfg.caps == "bases" and n_cand > 1:
            caps = (n_cand + 3, max(1, bases // 2))
        else:
            caps = (n_cand + 3, bases + 100)
        within = np.cumsum(lens)[:caps[0]] <= caps[1]
        n_walked = int(within.sum()) if within.all() else int(np.argmin(within))
        return caps, order, (n_cand, bases, n_walked, int(lens[:n_walked].sum()))

    def walked_only(records, order, n_walked):
        keep = set(order[:n_walked].tolist())
        return [t for t in records if (t[0] * b.n_seqs + t[1]) * 2 + t[2] - 1 in keep]

    # ---- h: the device-resident forms of find / summary / best, plain and screened
    if cfg.legs["h"] and dev_ok:
        exp = {"find": to_dev(exp_find), "summary": to_dev(exp_sum)}
        for form, arg in (("find", (p_a, gap)), ("summary", p_a)):
            n_exp = len(exp[form])
            cap = _capacity(cfg.capacity, n_exp)
            n, rec = dev_records(rs, b, form, arg, strands, cap, cfg.refs_per_slab, seed=11)
            assert n == n_exp and _tuples(rec) == exp[form][:cap], "%s_refset_dev: %d vs %d records | %s" % (form, n, n_exp, tag)
            if cap < n_exp:
                routes.add(form + "_dev_truncated")
        n, rec = dev_records(rs, b, "best", p_a, strands, 0, cfg.refs_per_slab, seed=12)
        assert _tuples(rec) == World.best(b.n_seqs, exp["summary"]), "best_refset_dev | " + tag
        lb = refset.last_best()
        routes.update(n for n, on in (("best_dev_wave", lb[0]), ("best_dev_workgroup", lb[1])) if on)
        routes.add("h")
        if any({L_, W_} <= {w.route[r] for r in g} for g in w.slab_groups()):
            routes.add("mixed_slab")
        if cfg.prefilter:
            caps, order, st = caps_of(bits_dev)
            for form, arg in (("find", (p_a, gap)), ("summary", p_a)):
                want = walked_only(exp[form], order, st[2])
                cap = _capacity(cfg.capacity, len(want))
                n, rec, got_st = dev_records(rs, b, form, arg, strands, cap, caps=caps, seed=13)
                assert got_st == st, "%s_refset_screened_dev: stats %s vs %s | %s" % (form, got_st, st, tag)
                assert n == len(want) and _tuples(rec) == want[:cap], "%s_refset_screened_dev: %d vs %d records | %s" % (form, n, len(want), tag)
                if cap < len(want):
                    routes.add(form + "_screened_truncated")
            n, rec, got_st = dev_records(rs, b, "best", p_a, strands, 0, caps=caps, seed=14)
            assert got_st == st and _tuples(rec) == World.best(b.n_seqs, walked_only(exp["summary"], order, st[2])), "best_refset_screened_dev | " + tag
            routes.add("h_screened")
            if st[2] < st[0]:
                routes.add("tight_pairs" if cfg.caps == "pairs" else "tight_bases")
            if "unscreenable_ref" in routes:
                routes.add("unscreenable_ref_screened")

    # ---- i: the device-resident forms of call, plain and screened
    if cfg.legs["i"] and dev_ok:
        opts = call_opts(cfg, arc)
        forms = [dict(refs_per_slab=cfg.refs_per_slab)]
        if cfg.prefilter:
            caps, order, st = caps_of(bits_dev if p_a == p else _bits_at(w, cfg, b, index, p))
            forms.append(dict(caps=caps))
        if isinstance(exp_calls, int):
            got = dev_call(rs, b, opts, strands, 64, 1 << 12, 1 << 12, **forms[0])
            assert got["stats"][4] > 0 and got["stats"][5:] == (0, 0, 0), "call_refset_dev: no panic counted | " + tag
            routes.add("call_panic")
        else:
            calls = to_dev(exp_calls)
            for f in forms:
                want = calls if "caps" not in f else walked_only(calls, order, st[2])
                var, chars = variant_arrays(want)
                nv, nc = len(var), len(chars)
                mv, mc = _capacity(cfg.capacity, nv), _capacity(cfg.capacity, nc)
                name = "call_refset%s_dev" % ("_screened" if "caps" in f else "")
                max_sites = 1 << 12
                got = dev_call(rs, b, opts, strands, mv, mc, max_sites, seed=15, **f)
                for _ in range(2):  # more candidates or sites than the lists held: again, with the lists at exactly the counts.  (The
                    # sites of candidates that a slab could not store are not counted: the second call's n_sites is the first exact one.)
                    if max(got["stats"][2:4]) > max_sites:
                        max_sites = max(got["stats"][2:4])
                        got = dev_call(rs, b, opts, strands, mv, mc, max_sites, seed=15, **f)
                        routes.add("max_sites_exact")
                assert got["stats"][:2] == (nv, nc) and got["stats"][4:] == (0, 0, 0, 0), "%s: stats %s, %d variants %d chars expected | %s" % (name, got["stats"], nv, nc, tag)
                assert got["variants"].tobytes() == var[:mv].tobytes(), "%s: the records | %s" % (name, tag)
                ends = var["chars"].astype(np.int64) + var["query_len"] + var["ref_len"]
                fits = ends <= mc  # (characters go with their record: all of them or none)
                for x in np.flatnonzero(fits):
                    assert got["chars"][int(var["chars"][x]):int(ends[x])].tobytes() == chars[int(var["chars"][x]):int(ends[x])].tobytes(), "%s: the characters of record %d | %s" % (name, x, tag)
                written = int(ends[fits].max()) if fits.any() else 0
                g_var, g_ch = got["raw"]
                assert bool((g_ch.t[g_ch.front + written:g_ch.front + mc] == g_ch.image[g_ch.front + written:g_ch.front + mc]).all()), name + ": characters behind the last record | " + tag
                assert bool((g_var.t[g_var.front + min(nv, mv) * 24:g_var.front + mv * 24] == g_var.image[g_var.front + min(nv, mv) * 24:g_var.front + mv * 24]).all()), name + ": records behind the count | " + tag
                if "caps" in f:
                    assert got["screen"] == st, "%s: screen stats %s vs %s | %s" % (name, got["screen"], st, tag)
                    routes.add("i_screened")
                    if st[2] < st[0]:
                        routes.add("tight_pairs" if cfg.caps == "pairs" else "tight_bases")
                if mv < nv or mc < nc:
                    routes.add("call_dev_truncated")
                if nv:
                    routes.add("i_variants")
                # max_sites below the sites: the call says it is incomplete, and what it returns are records of the expected ones
                n_sites, slab_cands = got["stats"][2:4]
                if cfg.max_sites == "below" and min(n_sites, slab_cands) > 1 and "caps" not in f:
                    tight = min(n_sites, slab_cands) // 2
                    less = dev_call(rs, b, opts, strands, nv, nc, tight, seed=16, **f)
                    ls = less["stats"]
                    assert (ls[3] > tight or ls[2] > tight) and ls[4:] == (0, 0, 0, 0) and ls[0] <= nv, "%s with max_sites %d: stats %s | %s" % (name, tight, ls, tag)
                    mine = as_tuples(less["variants"], less["chars"])
                    assert len(set(mine)) == len(mine) and mine == sorted(mine, key=lambda v: v[:4]) and set(mine) <= set(want), \
                        "%s with max_sites %d: records that are not the expected ones', in order, once | %s" % (name, tight, tag)
                    routes.add("max_sites_below")
            if arc and calls:
                routes.add("i_add_revcomp")
        routes.add("i")
    return routes


def _bits_at(w, cfg, b, index, prob):
    """the screen's contract at `prob` in the device legs' batch: a sequence of fewer than 3 bases shares no seed, and has every bit of
    a reference that cannot be screened (kbo_hip.h: all its pairs on the strands asked for)"""
    exp = w.screen(prob, cfg.strands)
    out = np.zeros((w.n_refs, b.n_seqs, 2), dtype=bool)
    out[:, index, :] = exp
    for r in w.packed:
        if w.m[prob][r] < rrc.SEED_MIN:
            for strand in (1, 2):
                if cfg.strands & strand:
                    out[r, :, strand - 1] = True
    return out


def _gpu_fault(e):
    """a HIP error from the library (KBO_E_HIP) or from torch - not a mismatch, a refusal or a guard band"""
    return (isinstance(e, kbo_amd.KboError) and e.code == E_HIP) or (isinstance(e, RuntimeError) and "hip" in str(e).lower())


def run_seed(seed, oracle):
    """what the test of `seed` runs (tools/stress.py calls this too) -> (Config, routes)"""
    cfg = rrc.config(seed)
    try:
        routes = check_config(cfg, oracle)
    except BaseException as e:
        print("FAILED seed %d: %s\n  replay: SOAK=refset SEED=%d SECONDS=1 python tools/stress.py" % (seed, cfg.describe(), seed))
        if _gpu_fault(e):  # nothing more is started on a GPU that has faulted: the session ends here, and the seed is read, not re-run
            pytest.exit("seed %d ended in a GPU fault (%s); no further configuration runs" % (seed, e), returncode=3)
        raise
    return cfg, routes


@pytest.mark.parametrize("seed", rrc.SEEDS)
def test_config_equals_the_oracle(oracle, seed):
    cfg, routes = run_seed(seed, oracle)
    SEEN[seed] = (cfg, routes)


def _count(pred):
    return sum(1 for cfg, r in SEEN.values() if pred(cfg, r))


def route_tally():
    names = sorted({n for _, r in SEEN.values() for n in r})
    return {n: (_count(lambda c, r: n in r), _count(lambda c, r: n in r and c.k >= 64)) for n in names}


_GENERATOR_ONLY = ("k class", "k = ", "k < 11", "11 <= k", "a chunk that is no multiple of 16", "a chunk of 4k", "strands = ", "slab budget",
                   "refs_per_slab", "record capacity", "64 sequences", "one sequence")
# (what, at least, predicate over (Config, routes)): conditions on the seed list, not measurements.  First the ones the generator alone
# decides, as the host module states them (a seed counts only when the product ran it), then what the product reported
ROUTE_CONDITIONS = [(what, least, (lambda pred: lambda c, r: r != {"refused"} and pred(c, {"refused": False}))(pred))
                    for what, least, pred in HOST_CONDITIONS if what.startswith(_GENERATOR_ONLY) and "device leg" not in what] + [
    ("a chunk that is no multiple of 16, with a device leg", 5, lambda c, r: rrc.chunk_of(c.k) % 16 != 0 and r & {"d_dev", "e_dev", "f_dev", "h", "i"}),
    ("LDS and wide references in one slab", 25, lambda c, r: "mixed_slab" in r),
    ("a reference on the single-index route", 8, lambda c, r: "ref_index" in r),
    ("the single-index route walked by find", 5, lambda c, r: "index" in r),
    ("a set the device forms refuse", 5, lambda c, r: "dev_refused" in r),
    ("a reference with a status", 30, lambda c, r: "ref_status" in r),
    ("wide rows above 65 536", 3, lambda c, r: "wide_rows_above_64k" in r and "wide" in r),
    ("more than 256 chunks in one sequence", 5, lambda c, r: c.more_than_256_chunks and "a" in r),
    ("a contig above 65 536 bases", 3, lambda c, r: c.above_65536 and "a" in r),
    ("refset_best_kernel with a wave per sequence", 10, lambda c, r: r & {"best_wave", "best_dev_wave"}),
    ("refset_best_kernel with a workgroup per sequence", 10, lambda c, r: r & {"best_workgroup", "best_dev_workgroup"}),
    ("max_pairs below the candidates", 8, lambda c, r: "tight_pairs" in r),
    ("an unscreenable reference under a screened form", 10, lambda c, r: "unscreenable_ref_screened" in r),
    ("max_sites below the sites", 5, lambda c, r: "max_sites_below" in r),
] + [("sequences of %d bases in a device leg" % n, 5, (lambda n: lambda c, r: "short_%d_in_device_legs" % n in r)(n)) for n in (0, 1, 2)] + [
    ("%s truncated" % n, 5, (lambda n: lambda c, r: n + "_truncated" in r)(n)) for n in ("find_dev", "summary_dev", "find_screened", "summary_screened",
                                                                                        "locate_dev", "cover_dev", "call_dev")] + [
    ("leg %s with variants, %s" % (leg, name), least, (lambda leg, f: lambda c, r: leg + "_variants" in r and f(c))(leg, f))
    for leg in "gi" for name, least, f in _K_RANGES] + [
    ("add_revcomp of the call's own options with variants, leg %s" % leg, 5, (lambda leg: lambda c, r: leg + "_add_revcomp" in r)(leg)) for leg in "gi"] + [
    ("leg %s" % leg, 20, (lambda leg: lambda c, r: leg in r)(leg)) for leg in rrc.LEGS]


def test_routes_covered():
    """over the union of all seeds: everything the module claims to cover was reached, and at most 10 % of the seeds were refused"""
    missing = [s for s in rrc.SEEDS if s not in SEEN]
    assert not missing, "seeds that did not run (or failed): %s" % missing[:20]
    print("route tally over %d seeds (configurations, of them k >= 64): %s" % (len(SEEN), route_tally()))
    refused = _count(lambda c, r: r == {"refused"})
    counts = [(what, least, _count(pred)) for what, least, pred in ROUTE_CONDITIONS]
    for what, least, n in counts:
        print("%-70s %4d (>= %d)" % (what, n, least))
    print("refused: %d of %d" % (refused, len(SEEN)))
    assert refused * 10 <= len(SEEN), "%d of %d configurations refused" % (refused, len(SEEN))
    short = [(what, n, least) for what, least, n in counts if n < least]
    assert not short, "routes not reached often enough (what, seen, at least): %s" % short
