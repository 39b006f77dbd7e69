"""kbo_call_refset_dev and kbo_call_refset_screened_dev (kbo_hip.h "The VARIANTS of a pair"; kbo_amd/csrc/refset_resolve_kernels.hip):
the device-resident variant calls, byte for byte against kbo_call_refset on the same set, batch, options and strands.

Every call runs with d_work at exactly its *_work_bytes figure, d_variants at exactly max_variants records, d_chars at exactly
max_chars bytes and d_stats at its 64 bytes, each between guard bands that are checked behind the call.  The worlds are those of
tests/test_refset_call_host.py (an LDS and a wide route in one set, every planted case, the contig with 243 sites); the other batches
are made here: positions beyond 20 bits, long repeats, more than 4 096 sites in one pair, bytes that are no bases and a sequence of two
bases."""
import ctypes as C

import numpy as np
import pytest

import kbo_amd
from kbo_amd import _capi, refset

from gpu_helpers import Guarded
from test_refset_call_host import _rnd, _sub, call_opts, revcomp, world

pytestmark = pytest.mark.gpu


class DevBatch:
    def __init__(self, seqs):
        import torch
        self.seqs, self.n_seqs = seqs, len(seqs)
        self.lens = np.asarray([len(s) for s in seqs], dtype=np.int64)
        self.offsets = np.zeros(self.n_seqs + 1, dtype=np.int64)
        self.offsets[1:] = np.cumsum(self.lens)
        self.total = int(self.offsets[-1])
        self.device = torch.device("cuda", torch.cuda.current_device())
        q = np.zeros(self.total + 16, dtype=np.uint8)
        q[:self.total] = np.concatenate(seqs)
        self.d_q = torch.from_numpy(q).to(self.device)
        self.d_off = torch.from_numpy(self.offsets).to(self.device)


def run_dev(rs, b, opts, strands, max_variants, max_chars, max_sites, refs_per_slab=0, caps=None, seed=1):
    """one call behind guard bands -> dict(variants, chars, stats[, screen]); variants: the records written, chars: the whole buffer"""
    import torch
    L = kbo_amd.lib()
    rs.to_device()
    co = _capi.CallOpts(opts.max_error_prob, opts.sbwt_build_opts._to_c())
    s = torch.cuda.current_stream(b.device)
    if caps is None:
        wb = int(L.kbo_call_refset_dev_work_bytes(rs._h, b.n_seqs, b.total, strands, max_sites, refs_per_slab))
    else:
        wb = int(L.kbo_call_refset_screened_dev_work_bytes(rs._h, b.n_seqs, b.total, strands, max_sites, caps[0], caps[1]))
    assert wb > 0
    work = Guarded("d_work", wb, 1 << 20, b.device, seed=seed)
    var = Guarded("d_variants", max_variants * 24, 1 << 16, b.device, seed=seed + 1)
    chars = Guarded("d_chars", max_chars, 1 << 16, b.device, seed=seed + 2)
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
    st = stats.host().view(np.uint64)
    out = dict(stats=tuple(int(v) for v in st), raw=(var, chars))
    assert out["stats"][5:] == (0, 0, 0)
    n = min(out["stats"][0], max_variants)
    out["variants"] = var.host()[:n * 24].view(refset.REF_VARIANT).copy()
    out["chars"] = chars.host().copy()
    if screen is not None:
        out["screen"] = tuple(int(v) for v in screen.cpu().numpy())
    return out


def host_calls(rs, seqs, opts, strands):
    variants, chars = refset.call_refset(seqs, rs, opts, strands)
    return variants, chars, refset.last_call()


def assert_same(got, variants, chars, what):
    """a complete call with room for everything: the host's bytes"""
    assert got["stats"][:2] == (len(variants), len(chars)) and got["stats"][4] == 0, (what, got["stats"], len(variants), len(chars))
    assert got["variants"].tobytes() == variants.tobytes(), what
    assert got["chars"][:len(chars)].tobytes() == chars.tobytes(), what


_batches = {}


def world_batch(k, rc):
    if (k, rc) not in _batches:
        w = world(k, rc, prefilter=True)
        _batches[k, rc] = (w, DevBatch(w.seqs))
    return _batches[k, rc]


@pytest.mark.parametrize("rc", [False, True])
@pytest.mark.parametrize("k", [41, 96])
def test_the_worlds_byte_for_byte(k, rc):
    """options with and without add_revcomp, strands 1 - 3, 1e-7 and 1e-4; unscreened with 1, 3 and all references a slab, screened with
    ample caps"""
    w, b = world_batch(k, rc)
    caps = (len(w.refs) * b.n_seqs * 2, len(w.refs) * b.total * 2)
    n_calls = 0
    for prob in (1e-7, 1e-4):
        for arc in (False, True):
            for strands in (3, 1, 2):
                o = call_opts(k, prob, arc)
                variants, chars, counts = host_calls(w.rs, w.seqs, o, strands)
                assert strands == 2 and not rc or len(variants) > 100
                forms = [dict(refs_per_slab=0), dict(caps=caps)] + ([dict(refs_per_slab=1), dict(refs_per_slab=3)] if strands == 3 or arc else [])
                for f in forms:
                    got = run_dev(w.rs, b, o, strands, len(variants), len(chars), 1 << 12, **f)
                    assert_same(got, variants, chars, (k, rc, prob, arc, strands, f))
                    assert got["stats"][2] == counts[2] and got["stats"][3] <= counts[1] and got["stats"][2] <= 1 << 12
                    if "caps" in f:
                        assert got["screen"][0] == got["screen"][2] > 0
                    elif f["refs_per_slab"] == 0:
                        assert got["stats"][3] == counts[1]  # (one slab: its candidates are the call's)
                    n_calls += 1
    assert n_calls >= 36


def test_tight_screened_caps():
    """max_pairs below the candidates: the records of the host form restricted to the walked pairs"""
    k = 41
    w, b = world_batch(k, False)
    o = call_opts(k)
    variants, chars, _ = host_calls(w.rs, w.seqs, o, 3)
    order = np.flatnonzero(w.rs.candidates(w.seqs, 1e-7, 3, host=True).ravel())
    bit = (variants["ref"].astype(np.int64) * b.n_seqs + variants["seq"]) * 2 + variants["strand"] - 1
    seen = set()
    for max_pairs in (len(order) // 2, 3):
        keep = np.isin(bit, order[:max_pairs])
        exp = variants[keep]
        seen.add(len(exp))
        got = run_dev(w.rs, b, o, 3, len(variants), len(chars), 1 << 12, caps=(max_pairs, len(w.refs) * b.total * 2))
        assert got["screen"][2] == max_pairs < got["screen"][0] == len(order)
        assert got["stats"][0] == len(exp) and got["stats"][1] == int(exp["query_len"].sum() + exp["ref_len"].sum())
        for name in ("ref", "seq", "strand", "pos", "query_len", "ref_len"):
            assert np.array_equal(got["variants"][name], exp[name]), name
        for a, e in zip(got["variants"], exp):
            assert refset.variant_chars(a, got["chars"]) == refset.variant_chars(e, chars)
    assert len(seen) == 2 and 0 < max(seen) < len(variants)


def test_variant_and_character_capacities():
    """max_variants = n, n - 1 and 0, max_chars = n_chars, one less and 0: the totals stay, nothing behind a capacity is written"""
    k = 41
    w, b = world_batch(k, False)
    o = call_opts(k)
    variants, chars, _ = host_calls(w.rs, w.seqs, o, 3)
    n, nc = len(variants), len(chars)
    last = int(variants["query_len"][-1]) + int(variants["ref_len"][-1])
    assert n > 100 and last > 0
    for mv, mc in ((n, nc), (n - 1, nc), (0, nc), (n, nc - 1), (n, 0), (0, 0), (n + 5, nc + 9)):
        got = run_dev(w.rs, b, o, 3, mv, mc, 1 << 12, seed=7)
        assert got["stats"][:2] == (n, nc), (mv, mc, got["stats"])
        assert got["variants"].tobytes() == variants[:mv].tobytes(), (mv, mc)
        written = nc if mc >= nc else (nc - last if mc == nc - 1 else 0)  # (characters go with their record: all of them or none)
        assert got["chars"][:min(written, mc)].tobytes() == chars[:min(written, mc)].tobytes(), (mv, mc)
        var, ch = got["raw"]
        untouched = ch.t[ch.front + written:ch.front + mc] == ch.image[ch.front + written:ch.front + mc]
        assert bool(untouched.all()), (mv, mc)
        if mv > n:
            assert bool((var.t[var.front + n * 24:] == var.image[var.front + n * 24:]).all())


def test_max_sites_below_the_sites():
    """the lists hold fewer candidates than the contig with 243 sites has: the call says so, counts what it could not store, and writes
    nothing out of place"""
    k = 41
    w, b = world_batch(k, False)
    o = call_opts(k)
    variants, chars, counts = host_calls(w.rs, w.seqs, o, 1)
    full = run_dev(w.rs, b, o, 1, len(variants), len(chars), 1 << 12)
    assert_same(full, variants, chars, "room for every site")
    assert counts[1] > 243 and full["stats"][2:5] == (counts[2], counts[1], 0) and full["stats"][0] == counts[3]
    got = run_dev(w.rs, b, o, 1, len(variants), len(chars), 100)
    n_var, n_chars, n_sites, slab_cands, panics = got["stats"][:5]
    assert slab_cands == counts[1] > 100 and n_sites <= 100 and panics == 0  # incomplete: max_slab_candidates > max_sites
    assert 0 < n_var <= n_sites and n_var < len(variants)
    exp = {(int(v["ref"]), int(v["seq"]), int(v["strand"]), int(v["pos"])) + refset.variant_chars(v, chars) for v in variants}
    mine = [(int(v["ref"]), int(v["seq"]), int(v["strand"]), int(v["pos"])) + refset.variant_chars(v, got["chars"]) for v in got["variants"]]
    assert set(mine) <= exp and mine == sorted(mine, key=lambda v: v[:4]) and len(set(mine)) == len(mine)  # (the stored sites' records are exact)
    # every slab within the lists, the call's list not: counted, not stored
    per_ref = run_dev(w.rs, b, o, 1, len(variants), len(chars), 1 << 12, refs_per_slab=1)
    top = per_ref["stats"][3]
    assert per_ref["stats"][2] == counts[2] and top <= counts[1]
    got = run_dev(w.rs, b, o, 1, len(variants), len(chars), top, refs_per_slab=1)
    assert got["stats"][2:4] == (counts[2], top)
    if counts[2] > top:
        assert got["stats"][0] < len(variants)
    else:
        assert_same(got, variants, chars, "the lists just hold the sites")


def _planted(rng, ref):
    """a copy of ref with a substitution, an insertion and a deletion"""
    c = _sub(ref, [250])
    return np.concatenate([c[:500], _rnd(rng, 2), c[500:750], c[753:]])


def test_positions_beyond_20_bits():
    """one contig of 1.2 Mbp with a copy of a reference at 1.1 Mbp"""
    k = 41
    rng = np.random.default_rng(20)
    refs = [_rnd(rng, 1000) for _ in range(3)]
    rs = refset.RefSet.build(refs, kbo_amd.BuildOpts(k=k, num_threads=4), prefilter=True)
    contig = np.concatenate([_rnd(rng, 1_100_000), _planted(rng, refs[1]), _rnd(rng, 100_000 - 999)])
    b = DevBatch([contig])
    o = call_opts(k)
    variants, chars, _ = host_calls(rs, b.seqs, o, 1)
    assert len(variants) == 3 and int(variants["pos"].min()) > 1 << 20
    assert sorted((int(v["query_len"]), int(v["ref_len"])) for v in variants) == [(0, 3), (1, 1), (2, 0)]
    assert_same(run_dev(rs, b, o, 1, 16, 256, 256), variants, chars, "unscreened")
    got = run_dev(rs, b, o, 1, 16, 256, 256, caps=(6, 6 * b.total))
    assert_same(got, variants, chars, "screened")
    assert got["screen"][0] == got["screen"][2] >= 1


def test_long_repeats_in_the_contig():
    """a homopolymer of 20 000 bases and 10 000 x AC in the contig, a homopolymer of 14 bases in the reference 20 bases in front of a
    substitution: the row's k-mer probes the long chains.  The same with T, whose 12-mer has the largest code there is: a reference
    with 14 T right in front of a substitution and one with 14 A there (probed as T on the '-' strand), their copies in a second contig
    behind a sequence with 'N's, a short run and 20 000 T - positions without a word must not lie among the occurrences of T x 12"""
    k = 41
    rng = np.random.default_rng(21)
    ref = _rnd(rng, 1200)
    ref[566:580] = ord("A")
    ref[565], ref[580] = ord("C"), ord("G")
    refs = [_rnd(rng, 900), ref, np.concatenate([_rnd(rng, 300), np.tile(np.frombuffer(b"AC", dtype=np.uint8), 40), _rnd(rng, 300)])]
    for base in b"TA":
        r = _rnd(rng, 1100)
        r[586:600] = base
        r[585] = ord("C")
        r[600] = ord("G")
        refs.append(r)
    rs = refset.RefSet.build(refs, kbo_amd.BuildOpts(k=k, num_threads=4))
    contig = np.concatenate([_rnd(rng, 500), np.full(20000, ord("A"), dtype=np.uint8), _rnd(rng, 300), np.tile(np.frombuffer(b"AC", dtype=np.uint8), 10000),
                             _rnd(rng, 400), _sub(ref, [600]), _rnd(rng, 300), _sub(refs[2], [395]), _rnd(rng, 200)])
    holes = np.concatenate([_rnd(rng, 60), [ord("N")], _rnd(rng, 30), [ord("N")] * 3, np.full(20000, ord("T"), dtype=np.uint8), _rnd(rng, 100), [ord("N")],
                            _rnd(rng, 11)]).astype(np.uint8)
    second = np.concatenate([_rnd(rng, 200), _sub(refs[3], [600]), [ord("N")], _rnd(rng, 250), _sub(refs[4], [600]), _rnd(rng, 300),
                             np.full(300, ord("T"), dtype=np.uint8), _rnd(rng, 100), revcomp(_sub(refs[4], [600])), _rnd(rng, 150)]).astype(np.uint8)
    b = DevBatch([contig, holes, second])
    for arc in (False, True):
        o = call_opts(k, add_revcomp=arc)
        for strands in (1, 3):
            variants, chars, _ = host_calls(rs, b.seqs, o, strands)
            assert len(variants) >= 4 and {1, 3, 4} <= set(variants["ref"]) and {0, 2} <= set(variants["seq"])
            assert strands == 1 or 2 in set(variants["strand"])  # (the copy on '-': its row's 14 A are probed as T)
            assert_same(run_dev(rs, b, o, strands, 64, 1024, 1 << 10), variants, chars, (arc, strands))


def test_more_than_4096_sites_in_one_pair():
    """a wide reference of 165 kbp whose copy carries substitutions 37 apart"""
    k = 41
    rng = np.random.default_rng(22)
    refs = [_rnd(rng, 165_000), _rnd(rng, 800)]
    rs = refset.RefSet.build(refs, kbo_amd.BuildOpts(k=k, num_threads=4), wide_rows=1 << 18)
    assert rs.route(0) == refset.ROUTE_WIDE
    contig = np.concatenate([_rnd(rng, 300), _sub(refs[0], range(40, 164_950, 37)), _rnd(rng, 300)])
    b = DevBatch([contig, refs[1].copy()])
    o = call_opts(k)
    variants, chars, counts = host_calls(rs, b.seqs, o, 1)
    assert counts[2] > 4096 and len(variants) > 4096
    got = run_dev(rs, b, o, 1, len(variants), len(chars), 1 << 13)
    assert_same(got, variants, chars, "4 458 sites of one pair")
    assert got["stats"][2] == counts[2]


def test_bytes_that_are_no_bases_and_a_sequence_of_two_bases():
    """the device forms take a batch the host form refuses: the sequence of two bases contributes nothing, the others what they give
    without it"""
    k = 41
    w, _ = world_batch(k, False)
    lower = w.seqs[0].copy()
    lower[700:703] = np.frombuffer(b"acg", dtype=np.uint8)
    seqs = [w.seqs[4], np.frombuffer(b"AC", dtype=np.uint8).copy(), lower, np.frombuffer(b"NN$", dtype=np.uint8).copy(), w.seqs[6]]
    assert ord("N") in w.seqs[4]
    b = DevBatch(seqs)
    for arc in (False, True):
        o = call_opts(k, add_revcomp=arc)
        variants, chars, _ = host_calls(w.rs, [seqs[0], seqs[2], seqs[3], seqs[4]], o, 3)
        variants = variants.copy()
        variants["seq"] += variants["seq"] >= 1
        assert len(variants) > 10 and {0, 2, 4} <= set(variants["seq"])
        assert_same(run_dev(w.rs, b, o, 3, 256, 4096, 1 << 10), variants, chars, "unscreened")
        assert_same(run_dev(w.rs, b, o, 3, 256, 4096, 1 << 10, caps=(len(w.refs) * 10, len(w.refs) * 2 * b.total)), variants, chars, "screened")


def test_two_runs_give_the_same_bytes():
    k = 96
    w, b = world_batch(k, True)
    o = call_opts(k, 1e-4, True)
    runs = [run_dev(w.rs, b, o, 3, 1 << 10, 1 << 14, 1 << 12, refs_per_slab=3, seed=5) for _ in range(2)]
    n, nc = runs[0]["stats"][:2]
    assert n > 400 and runs[0]["stats"] == runs[1]["stats"]
    assert runs[0]["variants"].tobytes() == runs[1]["variants"].tobytes() and runs[0]["chars"][:nc].tobytes() == runs[1]["chars"][:nc].tobytes()


def test_find_and_call_on_one_stream():
    """find_refset_dev(screened=True) and the call on one stream, both outputs read once at the end (the Python mirror)"""
    import torch
    k = 41
    w, b = world_batch(k, False)
    o = call_opts(k)
    stream = torch.cuda.Stream()
    caps = dict(max_pairs=len(w.refs) * b.n_seqs * 2, max_pair_bases=len(w.refs) * b.total * 2)
    runs, n_runs, screen = refset.find_refset_dev(b.d_q, b.d_off, w.rs, kbo_amd.FindOpts(max_error_prob=1e-7), 3, 1 << 12, stream=stream, screened=True, **caps)
    dv, dc, stats, screen2 = refset.call_refset_dev(b.d_q, b.d_off, w.rs, o, 3, 1 << 10, 1 << 13, 1 << 12, stream=stream, screened=True, **caps)
    dv2, dc2, stats2 = kbo_amd.call_refset_dev(b.d_q, b.d_off, w.rs, o, 3, 1 << 10, 1 << 13, 1 << 12, stream=stream)
    stream.synchronize()
    variants, chars, _ = host_calls(w.rs, w.seqs, o, 3)
    exp_runs = refset.find_refset(w.seqs, w.rs, kbo_amd.FindOpts(max_error_prob=1e-7), 3)
    assert int(n_runs[0]) == len(exp_runs) and runs.cpu().numpy()[:len(exp_runs)].tobytes() == exp_runs.tobytes()
    assert tuple(screen.cpu().numpy()) == tuple(screen2.cpu().numpy())
    for v, c, st in ((dv, dc, stats), (dv2, dc2, stats2)):
        assert v.shape == (1 << 10, 6) and v.dtype == torch.int32 and c.dtype == torch.uint8 and st.shape == (8,) and st.dtype == torch.int64
        assert tuple(int(x) for x in st.cpu().numpy()[:2]) == (len(variants), len(chars))
        assert v.cpu().numpy()[:len(variants)].tobytes() == variants.tobytes() and c.cpu().numpy()[:len(chars)].tobytes() == chars.tobytes()
