"""The generator of the randomized oracle soak (tests/random_configs.py) without a GPU: it is deterministic, and the fixed seed list
the GPU module runs (random_configs.SEEDS) holds what the reference side decides - every k class, every boundary length, every leg
and knob corner often enough, few refusals, gaps that the oracle's gap filling really fills."""
import collections

import numpy as np
import pytest

import random_configs as rc


@pytest.fixture(scope="module")
def configs():
    return {s: rc.config(s) for s in rc.SEEDS}


def test_deterministic_and_order_independent():
    seeds = list(rc.SEEDS[:12]) + [rc.STRESS_FIRST_SEED + 5]
    first = {}
    for s in seeds:
        cfg = rc.config(s)
        first[s] = (repr(cfg), rc.make_inputs(cfg), rc.make_opts_inputs(cfg, 17))
    for s in reversed(seeds):  # asked again, in another order
        cfg = rc.config(s)
        assert repr(cfg) == first[s][0]
        contigs, concat, off = rc.make_inputs(cfg)
        assert contigs == first[s][1][0] and concat.tobytes() == first[s][1][1].tobytes() and np.array_equal(off, first[s][1][2])
        oc, oo = rc.make_opts_inputs(cfg, 17)
        assert oc.tobytes() == first[s][2][0].tobytes() and np.array_equal(oo, first[s][2][1])
        assert np.array_equal(np.diff(off.astype(np.int64)), np.minimum(cfg.lens, len(b"".join(contigs)) - 1)) or cfg.repeats or cfg.n_contigs > 1
    assert len({first[s][1][1].tobytes() for s in seeds}) == len(seeds)


def test_seed_list_holds_every_class_length_leg_and_knob(configs):
    n = len(configs)
    ks = collections.Counter(rc.k_class(c.k) for c in configs.values())
    assert all(ks[i] >= 3 for i in range(len(rc.K_CLASSES))), ks
    assert {1, 2, 255} <= {c.k for c in configs.values()}
    assert 3 * sum(1 for c in configs.values() if c.k >= 64) >= n
    assert sum(1 for c in configs.values() if c.k >= 128) >= 30
    # read lengths at map_reads_kernel's boundaries; reads shorter than k and shorter than the smallest threshold; refused lengths
    lens = collections.Counter(x for c in configs.values() for x in set(c.lens))
    assert all(lens[x] >= 5 for x in rc.BOUNDARY_READ_LENS), [x for x in rc.BOUNDARY_READ_LENS if lens[x] < 5]
    assert all(any(x % m == 0 for x in lens) for m in (16, 32))
    assert sum(1 for c in configs.values() if min(c.lens) < c.k) >= 30 and sum(1 for c in configs.values() if min(c.lens) < 5) >= 30
    assert all(sum(1 for c in configs.values() if c.refuse_len == x) >= 3 for x in (0, 1, 2))
    # sequences of 0, 1 and 2 bases inside the batches of the legs whose entry points take them: the device-resident ones (d), the map
    # streams (j), kbo_sparse_runs_dev (reads, leg i) and - 1 and 2 bases - kbo_ms_batch (always run); at reads and at long sequences,
    # below and from k = 64
    for x in (0, 1, 2):
        has = [c for c in configs.values() if any(n == x for _, n in c.short_seqs)]
        assert sum(1 for c in has if c.legs["device"] and max(c.lens) <= 160) >= 5, x
        assert sum(1 for c in has if c.legs["device"] and max(c.lens) <= 160 and c.k >= 64) >= 3, x
        assert sum(1 for c in has if c.legs["device"] and max(c.lens) > 160 and c.k >= 64) >= 3, x
        assert sum(1 for c in has if c.legs["stream"]) >= 5, x
        assert sum(1 for c in has if c.legs["sparse"] and max(c.lens) <= 160) >= 3, x
    for c in list(configs.values())[:40]:
        _, concat, off = rc.make_inputs(c)
        c2, o2, keep = rc.with_shorts(c, concat, off)
        l2 = np.diff(o2.astype(np.int64))
        assert np.array_equal(c2[keep], concat) and int(o2[-1]) == len(c2) and sorted(l2[l2 < 3]) == sorted(n for _, n in c.short_seqs)
        assert [int(np.sum(l2[:i] >= 3)) for i in np.flatnonzero(l2 < 3)] == [w for w, _ in c.short_seqs]
    # sequences around map_long_kernel's piece size, and around k for large k
    for c in configs.values():
        if c.shape == "long_boundary":
            want = [min(x, c.G - 1) for x in rc.long_boundary_lens(c.k)]
            assert set(want) <= set(c.lens), (c.seed, c.k)
    lb = [c for c in configs.values() if c.shape == "long_boundary"]
    assert sum(1 for c in lb if c.k >= 64) >= 10 and sum(1 for c in lb if c.k >= 128) >= 5
    for k in (64, 128, 255):
        own = rc.long_own(k)
        assert own % 16 == 0 and own + 2 * k + 1 <= rc.LONG_REGION < own + 2 * k + 1 + 16
    # legs and knob corners
    for leg in rc.LEGS:
        assert sum(1 for c in configs.values() if c.legs[leg]) >= 15, leg
    assert all(c.n_contigs > 1 for c in configs.values() if c.legs["shards"])  # leg k: a sharded index over several contigs
    for name, pred in (("big layout", lambda kn: kn["big_layout"]), ("two workers", lambda kn: kn["two_workers"]),
                       ("depth table order 1", lambda kn: kn["depth_table"] == 1), ("depth table order 16", lambda kn: kn["depth_table"] == 16),
                       ("no depth table", lambda kn: kn["depth_table"] == -1), ("plan off", lambda kn: kn["plan"][0] == 0),
                       ("anchors forced on", lambda kn: kn["depth_table_anchors"] == 1), ("anchors forced off", lambda kn: kn["depth_table_anchors"] == 0),
                       ("small slabs", lambda kn: kn["slab_bytes"] == 1 << 16), ("pair steps off", lambda kn: kn["pair_steps"][0] != 0)):
        assert sum(1 for c in configs.values() if pred(c.knobs)) >= 3, name
    assert sum(1 for c in configs.values() if c.n_contigs > 1) >= 15 and sum(1 for c in configs.values() if c.add_revcomp) >= 15
    for emit in (0, 1, 2):
        assert sum(1 for c in configs.values() if c.legs["call"] and c.call_emit == emit) >= 3, emit
    for lo, hi in ((0, 32), (32, 64), (64, 128), (128, 255)):
        for rcomp in (False, True):
            assert any(c.legs["devbuild"] and lo < c.k <= hi and c.add_revcomp == rcomp for c in configs.values()), (lo, hi, rcomp)


def test_no_draw_of_the_first_legs_moved_and_the_new_ones_are_deterministic(configs):
    """Config.extra comes from a stream of its own: without it a configuration is what it was before legs l - q (the digest over the
    list, LABNOTES); helpers of the new legs against their definitions"""
    for s in list(rc.SEEDS[:6]):
        c = configs[s]
        assert repr(rc.config(s).extra) == repr(c.extra) and set(c.extra["legs"]) == set(rc.LEGS2)
        _, concat, off = rc.make_inputs(c)
        lens = np.diff(off.astype(np.int64))
        r = rc.revcomp(concat, off)
        for i in (0, len(lens) // 2, len(lens) - 1):  # the definition, sequence by sequence
            a, b = int(off[i]), int(off[i + 1])
            assert np.array_equal(r[a:b], rc.COMP[concat[a:b][::-1]])
        assert np.array_equal(rc.revcomp(r, off), concat)
        assert rc.COMP[ord("N")] == ord("N") and bytes(rc.COMP[list(b"ACGTacgt")]) == b"TGCAtgca"
        sin = rc.make_strand_inputs(c, concat, off)
        pm = np.repeat(np.asarray(c.extra["minus"]), lens)
        assert np.array_equal(sin[pm], r[pm]) and np.array_equal(sin[~pm], concat[~pm])
        words, pos, byt, mask = rc.pack_reads(concat, off)
        assert len(words) == int(((lens + 15) // 16).sum()) and np.array_equal(concat[pos.astype(np.int64)], byt)
        a, b = int(off[1]), int(off[2])  # sequence 1 starts a word; 16 bases a word from the low bits up
        w0 = int(((lens[0] + 15) // 16))
        for i in range(min(b - a, 40)):
            if rc.PACK_CODE[concat[a + i]] < 4:
                assert (int(words[w0 + i // 16]) >> (2 * (i % 16))) & 3 == rc.PACK_CODE[concat[a + i]]
                assert (int(mask[w0 + i // 16]) >> (2 * (i % 16))) & 3 == 3


def test_seed_list_holds_the_second_set_of_legs(configs):
    """what the reference side alone decides about legs l - q (the product's routes: test_routes_covered of the GPU module)"""
    cs = list(configs.values())
    for leg in rc.LEGS2:
        has = [c for c in cs if c.extra["legs"][leg]]
        assert len(has) >= 15 and sum(1 for c in has if c.k >= 64) >= 5 and sum(1 for c in has if c.k >= 128) >= 3, leg
    # what the list holds for them to run over: reads, reads at k >= 64, reads over a depth table of order 16
    reads = [c for c in cs if max(c.lens) <= 160]
    assert len(reads) >= 100 and sum(1 for c in reads if c.k >= 64) >= 50 and sum(1 for c in reads if c.knobs["depth_table"] == 16) >= 15
    for c in reads:  # the NP = 18 summary forms: every configuration that can reach them runs the device summaries
        if c.knobs["depth_table"] == 16 and c.k >= 16:
            assert c.extra["legs"]["summary"] and c.extra["summary_forms"]["device"], c.seed
    summ = [c for c in cs if c.extra["legs"]["summary"]]
    for form in rc.SUMMARY_FORMS:
        assert sum(1 for c in summ if c.extra["summary_forms"][form]) >= 15, form
    assert sum(1 for c in summ if c.extra["summary_forms"]["stream"] and c.legs["stream"]) >= 5
    assert sum(1 for c in summ if c.extra["summary_forms"]["device"] and c.short_seqs and max(c.lens) <= 160 and c.k >= 64) >= 3
    # both strands: under small slabs, two workers, a sharded index, an index with its reverse complement, large k
    both = [c for c in cs if c.extra["legs"]["strands"] and c.extra["strands"] == 3]
    assert sum(1 for c in both if c.knobs["slab_bytes"] == 1 << 16) >= 3
    assert sum(1 for c in both if c.knobs["two_workers"]) >= 3
    assert sum(1 for c in both if c.legs["shards"]) >= 3
    assert sum(1 for c in both if c.add_revcomp) >= 3
    assert sum(1 for c in both if c.k >= 64) >= 5
    assert {c.extra["strands"] for c in cs if c.extra["legs"]["strands"]} == {1, 2, 3}
    n_minus = sum(sum(c.extra["minus"]) for c in cs)
    n_all = sum(len(c.lens) for c in cs)
    assert n_all <= 4 * n_minus <= 3 * n_all
    for c in cs:
        assert len(c.extra["minus"]) == len(c.lens)
        if len(c.lens) >= 2:
            assert len(c.lens) <= 4 * sum(c.extra["minus"]) <= 3 * len(c.lens), c.seed
        # a threshold per sequence of the device legs' batch; two different ones in every batch, whatever the oracle's threshold is
        n_s = len(c.lens) + len(c.short_seqs)
        for t in (2, 3, min(c.k, 12), c.k):
            if c.k >= 3 and t <= c.k:
                thr = rc.thresholds_of(c, t, n_s)
                assert thr.dtype == np.int32 and thr.min() >= 2 and thr.max() <= c.k
                assert n_s < 2 or len(set(thr[:2].tolist())) == 2, (c.seed, t)
    for key, values in (("strand_gap", {0, 3, 50}), ("find_dev_gap", {0, 5, 2**32 - 1}), ("rle_gap", {0, 3, 50, 2**32 - 1}),
                        ("rle_capacity_mode", {"full", "third", "zero"}), ("strand_format", {False, True})):
        leg = {"strand_gap": "strands", "strand_format": "strands", "find_dev_gap": "find_dev"}.get(key, "rle_dev")
        for v in values:
            assert sum(1 for c in cs if c.extra["legs"][leg] and c.extra[key] == v) >= 3, (key, v)


def test_the_oracle_alone_over_the_seed_list(oracle, configs):
    """index build + matches over every configuration: few refusals; legs g / h run to an answer or a refusal and have gaps to fill"""
    refused, filled = [], 0
    for s, cfg in configs.items():
        contigs, concat, off = rc.make_inputs(cfg)
        oi = oracle.Index.build(contigs, k=cfg.k, add_revcomp=cfg.add_revcomp)
        if len(off) > 301:  # (a part of the batch: whether the oracle refuses depends on the index and on the shortest sequence)
            concat, off = concat[:int(off[300])], off[:301]
        try:
            chars = oi.matches_batch(concat, off, cfg.max_error_prob, n_threads=4)
        except oracle.OracleError as e:
            refused.append((s, cfg.k, cfg.G, e.code))
            continue
        assert len(chars) == len(concat)
        if cfg.refuse_len >= 0:
            c2, o2 = rc.with_refused(cfg, *rc.make_inputs(cfg)[1:])
            with pytest.raises(oracle.OracleError) as ei:
                oi.matches_batch(c2, o2, cfg.max_error_prob, n_threads=2)
            assert ei.value.code == (-1 if cfg.refuse_len == 0 else -2), (s, ei.value.code)
        if not (cfg.legs["map_opts"] or cfg.legs["fill_gaps"]):
            continue
        thr = oracle.random_match_threshold(cfg.k, oi.n_kmers, 4, cfg.max_error_prob)
        oc, oo = rc.make_opts_inputs(cfg, thr)
        n_ok = n_changed = 0
        codes = set()
        for i in range(len(oo) - 1):
            seq = oc[int(oo[i]):int(oo[i + 1])].tobytes()
            if cfg.legs["map_opts"]:
                try:
                    assert len(oi.map(seq, cfg.k, cfg.max_error_prob, *cfg.map_opts)) == len(seq)
                except oracle.OracleError as e:
                    codes.add(e.code)
            if cfg.legs["fill_gaps"] and len(seq):
                try:
                    d, _, _ = oi.matching_statistics(seq)
                    tr = oracle.translate_ms_vec(oracle.derandomize_ms_vec(d, cfg.k, thr), cfg.k, thr)
                    out = oi.fill_gaps(tr, seq, thr, cfg.max_error_prob)
                    n_ok += 1
                    n_changed += out != tr.encode()
                except oracle.OracleError as e:
                    codes.add(e.code)
        assert codes <= {-1, -2, -3, -6}, (s, codes)
        if cfg.legs["fill_gaps"]:
            assert n_ok > 0, s
            filled += n_changed > 0
    print("refused:", refused, "configurations whose gaps the oracle fills:", filled)
    assert len(refused) * 10 <= len(configs), refused
    assert filled >= 10, filled
