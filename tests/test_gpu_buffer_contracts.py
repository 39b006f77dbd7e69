"""The device-resident entry points held to the buffer sizes include/kbo_hip.h documents (INTEGRATION.md "Device-resident buffers:
slack"): every buffer is declared at exactly its documented minimum and sits between guard bands of a seeded pattern
(gpu_helpers.Guarded).  Each case compares every specified output byte with the oracle and asserts that no guard changed; then it
refills d_work, the scratch buffers and the outputs with another pattern and runs again: the results must be the same (no reliance on
zeroed or left-over scratch).  The guards and the slack of d_concat and of the packed words continue the genome, so a kernel that
reads past its slack or in front of the first sequence changes its results.  Declaring a checked size one byte short must be refused
without touching any buffer; so must kbo_work_bytes() for map / find over a sharded index, which need kbo_index_work_bytes()."""
import ctypes as C

import numpy as np
import pytest

import kbo_amd
from kbo_amd import batch, derandomize, synth
from gpu_helpers import PER_BASE_GUARD, Guarded, round16, scratch_guard_bytes, threads

pytestmark = pytest.mark.gpu

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
COMP = np.zeros(256, dtype=np.uint8)
for _a, _b in zip(b"ACGTacgtN", b"TGCAtgcaN"):
    COMP[_a] = _b
BAD_ARG = -4
LISTS = 256  # KBO_CALL_LISTS
HEAD, TAIL = 20_000, 40_000  # the first sequence of a batch starts at contig 0's HEAD, the last one ends at TAIL: the guards continue them


def _dev():
    import torch
    return torch.device("cuda:0")


def _stream():
    import torch
    return torch.cuda.current_stream(_dev()).cuda_stream


def _sync():
    import torch
    torch.cuda.synchronize()


def _contigs():
    """≈ 300 kbp in three contigs that share a 2 kbp stretch"""
    g = [synth.genome(n, seed=s) for n, s in ((150_000, 911), (100_000, 912), (50_000, 913))]
    g[1][30_000:32_000] = g[0][60_000:62_000]
    g[2][10_000:12_000] = g[0][60_000:62_000]
    return g


def _mutate(rng, src, sub, spice):
    """1 % substitutions; with `spice` now and then an N or a stretch of lower case; either strand"""
    q = src.copy()
    hit = rng.random(len(q)) < sub
    q[hit] = ACGT[(np.searchsorted(ACGT, q[hit]) + rng.integers(1, 4, int(hit.sum()))) % 4]
    if spice and len(q) > 10:
        r = rng.random()
        if r < 0.06:
            q[int(rng.integers(0, len(q)))] = ord("N")
        elif r < 0.12:
            p = int(rng.integers(0, len(q) - 5))
            q[p:p + int(rng.integers(1, 40))] |= 0x20
    if rng.random() < 0.5:
        q = COMP[q[::-1]].copy()
    return q


class Batch:
    """Sequences on the host with everything the oracle says about them."""

    def __init__(self, name, contigs, seqs, k, ora, oracle):
        self.name, self.k, self.g0, self.ora = name, k, contigs[0], ora
        self.concat = np.concatenate(seqs)
        self.offsets = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.uint64)
        self.n, self.total = len(seqs), int(self.offsets[-1])
        self.lens = np.diff(self.offsets.astype(np.int64))
        self.max_len = int(self.lens.max())
        # sequences of 1 and 2 bases: their bytes are unspecified (kbo_hip.h), and the oracle, like the reference, refuses them
        self.big = np.flatnonzero(self.lens >= 3)
        self.keep = np.repeat(self.lens >= 3, self.lens)
        self.big_off = np.concatenate([[0], np.cumsum(self.lens[self.big])]).astype(np.uint64)
        self.chars, self.d = np.zeros(self.total, dtype=np.uint8), np.zeros(self.total, dtype=np.uint8)
        self.chars[self.keep], self.d[self.keep] = ora.matches_batch(self.concat[self.keep], self.big_off, 1e-7, n_threads=threads(),
                                                                     want_d=True)
        self.map = np.frombuffer(oracle.relative_to_ref(self.concat, self.chars), dtype=np.uint8)
        self._runs = {}

    def runs(self, oracle, gap):
        """(records [n_runs, 7], first-run index per sequence [n + 1]) as kbo_find_batch_dev gives them: none for the sequences of
        fewer than 3 bases"""
        if gap not in self._runs:
            recs, first_big = oracle.run_lengths_batch(self.chars[self.keep], self.big_off, gap)
            before = np.concatenate([[0], np.cumsum(self.lens >= 3)])  # sequences of 3 bases or more in front of sequence s
            self._runs[gap] = (recs, np.asarray(first_big, dtype=np.uint64)[before])
        return self._runs[gap]

    def sites(self, thr):
        """the first pass of call_variants (variant_calling.rs:266-273) for every sequence of 3 bases or more: {(sequence, i, j, row)}"""
        recs = self.ora.call_sites_batch(self.concat[self.keep], self.big_off, thr, n_threads=threads())
        return {(int(self.big[s]), int(i), int(j), int(r)) for s, i, j, r in recs}


def _reads(rng, contigs, n_reads, total_mod16, lengths=(20, 160), spice=True, tiny=True, uniform=0):
    """reads of mixed lengths (or all `uniform` bases long), 1- and 2-base sequences between them, a clean first read at contig 0's
    HEAD and a clean last one ending at TAIL (9 bases, or `uniform`); the first read's length sets total_bases mod 16"""
    g0 = contigs[0]
    body = []
    for r in range(n_reads):
        c = contigs[int(rng.integers(0, len(contigs)))]
        n = uniform or int(rng.integers(lengths[0], lengths[1] + 1))
        a = int(rng.integers(0, len(c) - n))
        body.append(_mutate(rng, c[a:a + n], 0.01, spice))
        if tiny and r % 53 == 7:
            body.append(ACGT[rng.integers(0, 4, 1 + r % 2)])
    if uniform:
        return [g0[HEAD:HEAD + uniform].copy()] + body + [g0[TAIL - uniform:TAIL].copy()]
    rest = sum(len(s) for s in body) + 9
    n0 = 100 + (total_mod16 - rest - 100) % 16
    seqs = [g0[HEAD:HEAD + n0].copy()] + body + [g0[TAIL - 9:TAIL].copy()]
    assert sum(len(s) for s in seqs) % 16 == total_mod16
    return seqs


def _longs(rng, contigs):
    """sequences of 500 - 20 000 bases (1 % substitutions, an N, lower case, either strand), reads and 1- / 2-base sequences between
    them; the last sequence 11 bases"""
    g0 = contigs[0]
    seqs = [g0[HEAD:HEAD + 613].copy()]
    for i, n in enumerate((500, 3000, 20_000, 1200, 7000, 900)):
        c = contigs[i % len(contigs)]
        a = int(rng.integers(0, len(c) - n))
        q = _mutate(rng, c[a:a + n], 0.01, False)
        q[int(rng.integers(0, n))] = ord("N")
        q[100:130] |= 0x20
        seqs.append(q)
        seqs.append(ACGT[rng.integers(0, 4, 1 + i % 2)])
        a = int(rng.integers(0, len(c) - 150))
        seqs.append(_mutate(rng, c[a:a + 150], 0.01, True))
    seqs.append(g0[TAIL - 11:TAIL].copy())
    return seqs


@pytest.fixture(scope="module")
def world(oracle):
    """the contigs, the indexes (k = 31 plain and with two shards, k = 63) and the batches, shared by the module"""
    import torch
    L = kbo_amd.lib()
    contigs = _contigs()
    w = {"L": L}
    for k in (31, 63):
        w["sbwt%d" % k], _ = kbo_amd.build(contigs, kbo_amd.BuildOpts(k=k, num_threads=threads()))
        w["ora%d" % k] = oracle.Index.build([c.tobytes() for c in contigs], k=k)
    try:
        L.kbo_set_index_shards(2)
        w["sharded"], _ = kbo_amd.build(contigs, kbo_amd.BuildOpts(k=31, num_threads=threads()))
    finally:
        L.kbo_set_index_shards(0)
    assert w["sharded"].shards() == 2 and w["sharded"].n_kmers() == w["sbwt31"].n_kmers()
    with torch.cuda.device(_dev()):
        for key in ("sbwt31", "sbwt63", "sharded"):
            w[key].to_device(-1)
    rng = np.random.default_rng(2024)
    ora = w["ora31"]
    w["reads0"] = Batch("reads0", contigs, _reads(rng, contigs, 1500, 0), 31, ora, oracle)
    w["reads7"] = Batch("reads7", contigs, _reads(rng, contigs, 1500, 7), 31, ora, oracle)
    w["longs"] = Batch("longs", contigs, _longs(rng, contigs), 31, ora, oracle)
    w["uniform"] = Batch("uniform", contigs, _reads(rng, contigs, 800, 0, spice=False, tiny=False, uniform=150), 31, ora, oracle)
    w["uniform_n"] = Batch("uniform_n", contigs, _reads(rng, contigs, 800, 0, tiny=False, uniform=150), 31, ora, oracle)
    w["mixed_clean"] = Batch("mixed_clean", contigs, _reads(rng, contigs, 900, 5, spice=False), 31, ora, oracle)
    w["reads63"] = Batch("reads63", contigs, _reads(rng, contigs, 1200, 3, lengths=(70, 160)), 63, w["ora63"], oracle)
    return w


# ---------------------------------------------------------------------------------------------------------------- buffers and steps

def _concat_buf(b):
    """d_concat: total_bases + 16 bytes; the front guard ends with the genome in front of the first read, the slack and the back guard
    continue the genome behind the last one"""
    back = np.resize(b.g0[TAIL:], 16 + PER_BASE_GUARD)
    return Guarded("d_concat", b.total + 16, PER_BASE_GUARD, _dev(), data=b.concat, front_bytes=b.g0[HEAD - 4096:HEAD], back_bytes=back)


def _offsets_buf(b):
    return Guarded("d_offsets", 8 * (b.n + 1), PER_BASE_GUARD, _dev(), data=b.offsets.view(np.uint8))


def _out(name, n, seed=1):
    return Guarded(name, n, PER_BASE_GUARD, _dev(), seed=seed)


def _scratch(name, n, b, seed=2):
    return Guarded(name, n, scratch_guard_bytes(b.n, b.total, b.k), _dev(), seed=seed)


def _eq(got, want, keep, what):
    got, want = np.asarray(got)[:len(want)], np.asarray(want)
    if keep is not None:
        got, want = got[keep], want[keep]
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        raise AssertionError("%s: %d values differ from the oracle, the first at %d (got %r, want %r)" % (
            what, len(bad), bad[0], got[bad[0]], want[bad[0]]))


def _twice(run, check, mutable, guarded, what):
    """run, check the results and every guard; refill the mutable buffers (d_work, scratch, outputs) with another pattern and run
    again: the same results, every guard intact again"""
    run()
    _sync()
    first = check()
    for x in guarded:
        x.assert_intact(what + " (first run)")
    for x in mutable:
        x.fill(77)
    run()
    _sync()
    second = check()
    for x in guarded:
        x.assert_intact(what + " (second run, other scratch pattern)")
    for a, b in zip(first, second):
        assert np.array_equal(a, b), what + ": the results differ between scratch patterns"


def _refused(calls, bufs):
    """each call of [(what, call[, buffers of its own])] returns KBO_E_BAD_ARG and leaves every buffer - inside and outside - as it was"""
    bad = []
    for what, call, *own in calls:
        _sync()
        bufs_ = bufs + (own[0] if own else [])
        for x in bufs_:
            x.fill(5)
        rc = call()
        _sync()
        changed = ["%s (%s)" % (x.name, "%s guard at %d, %d bytes" % x.check() if x.check() else "inside") for x in bufs_ if x.changed()]
        if rc != BAD_ARG or changed:
            bad.append("%s: rc %d (expected KBO_E_BAD_ARG); changed: %s" % (what, rc, ", ".join(changed) or "nothing"))
    assert not bad, "\n".join(bad)


# ---------------------------------------------------------------------------------------------------------------- kbo_ms_batch_dev

MS_CASES = [  # (id, batch, index, max_seq_len (None: the longest), knob)
    ("one_kernel", "reads7", "sbwt31", None, None),
    ("one_kernel_mod16", "reads0", "sbwt31", None, None),
    ("guided_walk", "reads7", "sbwt31", None, "ms_one_kernel_off"),
    ("plain_walk", "reads0", "sbwt31", None, "plan_off"),
    ("intervals", "reads7", "sbwt31", None, "intervals"),
    ("long_len0", "longs", "sbwt31", 0, None),
    ("long_exact", "longs", "sbwt31", None, None),
    ("k63", "reads63", "sbwt63", None, None),
    ("sharded_reads", "reads7", "sharded", None, None),
    ("sharded_reads_len0", "reads0", "sharded", 0, None),
    ("sharded_long_len0", "longs", "sharded", 0, None),
]


@pytest.mark.parametrize("case", MS_CASES, ids=[c[0] for c in MS_CASES])
def test_ms_batch_dev_exact_buffers(world, case):
    name, bkey, ikey, max_len, knob = case
    L, b, sbwt = world["L"], world[bkey], world[ikey]
    ml = b.max_len if max_len is None else max_len
    if knob == "ms_one_kernel_off":
        L.kbo_set_ms_one_kernel(0)
    elif knob == "plan_off":
        L.kbo_set_plan(0, 0, 0)
    intervals = knob == "intervals"
    # kbo_ms_work_bytes, + one shard's MS values for a sharded index (kbo_hip.h, kbo_index_work_bytes)
    wb = int(L.kbo_ms_work_bytes(b.n, b.total, ml, b.k)) + (round16(b.total) + 16 if sbwt.shards() > 1 else 0)
    q, off = _concat_buf(b), _offsets_buf(b)
    ms = _out("d_ms_out", b.total + 16)
    lo = _out("d_lo_out", 4 * b.total, 3) if intervals else None
    hi = _out("d_hi_out", 4 * b.total, 4) if intervals else None
    work = _scratch("d_work", wb, b)
    outs = [x for x in (ms, lo, hi) if x is not None]
    if intervals:
        want_lo, want_hi = np.zeros(b.total, dtype=np.uint32), np.zeros(b.total, dtype=np.uint32)
        for s in range(b.n):
            a, e = int(b.offsets[s]), int(b.offsets[s + 1])
            _, want_lo[a:e], want_hi[a:e] = b.ora.matching_statistics(b.concat[a:e])

    def call(work_bytes):
        return L.kbo_ms_batch_dev(sbwt._h, q.ptr, off.ptr, b.n, b.total, ml, ms.ptr, lo.ptr if intervals else None,
                                  hi.ptr if intervals else None, work.ptr, work_bytes, _stream())

    def check():
        got = ms.host()
        _eq(got, b.d, b.keep, name + ": MS values")
        res = [got[:b.total][b.keep]]
        if intervals:
            gl, gh = lo.host().view(np.uint32), hi.host().view(np.uint32)
            _eq(gl, want_lo, b.keep, name + ": lo")
            _eq(gh, want_hi, b.keep, name + ": hi")
            res += [gl[:b.total][b.keep], gh[:b.total][b.keep]]
        return res

    _twice(lambda: kbo_amd.check(call(wb)), check, [work] + outs, [q, off, work] + outs, name)
    _refused([(name + ": d_work one byte short", lambda: call(wb - 1))], [q, off, work] + outs)


# ---------------------------------------------------------------------------------------------------------------- kbo_derand_translate_dev

@pytest.mark.parametrize("bkey,with_work,with_ref", [("reads7", False, False), ("reads0", False, True), ("longs", True, False),
                                                     ("longs", True, True)])
def test_derand_translate_dev_exact_buffers(world, bkey, with_work, with_ref):
    L, b = world["L"], world[bkey]
    name = "derand_translate %s d_work %s d_ref %s" % (bkey, with_work, with_ref)
    thr = derandomize.random_match_threshold(b.k, world["sbwt31"].n_kmers(), 4, 1e-7)
    msin = Guarded("d_ms", b.total + 16, PER_BASE_GUARD, _dev(), seed=8, data=b.d)
    q, off = _concat_buf(b), _offsets_buf(b)
    chars = _out("d_chars_out", b.total + 16)
    ml = 0 if with_work else b.max_len
    wb = int(L.kbo_derand_work_bytes(b.n, b.total))
    work = _scratch("d_work", wb, b) if with_work else None
    want = b.map if with_ref else b.chars
    mutable = [chars] + ([work] if with_work else [])

    def call(work_bytes):
        return L.kbo_derand_translate_dev(msin.ptr, off.ptr, b.n, b.total, b.k, thr, q.ptr if with_ref else None, chars.ptr, ml,
                                          work.ptr if with_work else None, work_bytes if with_work else 0, _stream())

    def check():
        got = chars.host()
        _eq(got, want, b.keep, name)
        return [got[:b.total][b.keep]]

    _twice(lambda: kbo_amd.check(call(wb)), check, mutable, [msin, q, off] + mutable, name)
    if with_work:  # (a smaller d_work is not refused: the call takes the lane-per-sequence kernel instead - the same results)
        _twice(lambda: kbo_amd.check(call(wb - 1)), check, mutable, [msin, q, off] + mutable, name + ", d_work one byte short")


# ---------------------------------------------------------------------------------------------------------------- kbo_map_batch_dev[_tail]

MAP_CASES = [  # (id, batch, index, max_seq_len (None: the longest; > 0: that much above it), format, want_ms, tail stream, fused)
    ("reads_chars", "reads7", "sbwt31", None, 0, 0, False, True),
    ("reads_map", "reads0", "sbwt31", None, 1, 0, False, True),
    ("reads_chars_ms", "reads0", "sbwt31", None, 0, 1, False, True),
    ("reads_map_ms_tail", "reads7", "sbwt31", None, 1, 1, True, True),
    ("reads_len0", "reads7", "sbwt31", 0, 0, 0, False, True),
    ("long_kernel_len0", "longs", "sbwt31", 0, 1, 0, False, True),
    ("long_kernel_exact_tail", "longs", "sbwt31", None, 0, 0, True, True),
    ("long_kernel_larger", "longs", "sbwt31", 1000, 1, 0, False, True),
    ("two_kernels_long_ms", "longs", "sbwt31", 0, 1, 1, False, False),
    ("no_depth_table", "reads7", "sbwt31", None, 1, 1, False, False),
    ("k63_reads", "reads63", "sbwt63", None, 1, 1, False, None),
    ("sharded_reads", "reads7", "sharded", None, 1, 1, False, False),
    ("sharded_reads_tail", "reads0", "sharded", None, 0, 0, True, False),
    ("sharded_long_len0", "longs", "sharded", 0, 1, 1, False, False),
    ("sharded_reads_len0", "reads0", "sharded", 0, 0, 0, True, False),
]


@pytest.mark.parametrize("case", MAP_CASES, ids=[c[0] for c in MAP_CASES])
def test_map_batch_dev_exact_buffers(world, case):
    import torch
    name, bkey, ikey, max_len, fmt, want_ms, tail, want_fused = case
    L, b, sbwt = world["L"], world[bkey], world[ikey]
    ml = b.max_len if max_len is None else (b.max_len + max_len if max_len else 0)
    if name == "no_depth_table":
        L.kbo_set_depth_table(-1)  # (launches ignore the copy's table: the two-kernel route)
    wb = int(L.kbo_index_work_bytes(sbwt._h, b.n, b.total, ml))
    plain = int(L.kbo_work_bytes(b.n, b.total, ml, b.k))
    q, off = _concat_buf(b), _offsets_buf(b)
    ms, chars = _out("d_ms", b.total + 16), _out("d_chars_out", b.total + 16, 3)
    work = _scratch("d_work", wb, b)
    ts = torch.cuda.Stream(_dev()) if tail else None
    fused = C.c_int(-1)
    want = b.map if fmt else b.chars

    def call(work_bytes, work_=work):
        if tail:
            return L.kbo_map_batch_dev_tail(sbwt._h, q.ptr, off.ptr, b.n, b.total, ml, 1e-7, fmt, want_ms, ms.ptr, chars.ptr, work_.ptr,
                                            work_bytes, _stream(), ts.cuda_stream, C.byref(fused))
        return L.kbo_map_batch_dev(sbwt._h, q.ptr, off.ptr, b.n, b.total, ml, 1e-7, fmt, want_ms, ms.ptr, chars.ptr, work_.ptr,
                                   work_bytes, _stream(), C.byref(fused))

    def check():
        got = chars.host()
        _eq(got, want, b.keep, name + ": characters")
        res = [got[:b.total][b.keep]]
        if want_ms or not fused.value:  # (the two-kernel route leaves every MS value in d_ms)
            gm = ms.host()
            _eq(gm, b.d, b.keep, name + ": MS values")
            res.append(gm[:b.total][b.keep])
        return res

    bufs = [q, off, ms, chars, work]
    _twice(lambda: kbo_amd.check(call(wb)), check, [ms, chars, work], bufs, name)
    if want_fused is not None:
        assert bool(fused.value) == want_fused, "%s: fused = %d" % (name, fused.value)
    short = [(name + ": d_work one byte short", lambda: call(wb - 1))]
    if sbwt.shards() > 1:  # + what a caller that reads the unsharded contract would pass, declared and allocated
        assert wb == plain + round16(b.total) + 16
        short.append((name + ": d_work of kbo_work_bytes() over a sharded index", lambda: call(plain)))
        work_plain = _scratch("d_work of kbo_work_bytes()", plain, b)
        short.append((name + ": d_work allocated at kbo_work_bytes()", lambda: call(plain, work_plain), [work_plain]))
    else:
        assert wb == plain
    _refused(short, bufs)


# ---------------------------------------------------------------------------------------------------------------- kbo_find_batch_dev

FIND_CASES = [  # (id, batch, index, max_seq_len (None: the longest), max_gap_len)
    ("reads_gap0", "reads7", "sbwt31", None, 0),
    ("reads_gap2", "reads0", "sbwt31", None, 2),
    ("long_len0_gap0", "longs", "sbwt31", 0, 0),
    ("long_gap2", "longs", "sbwt31", None, 2),
    ("sharded_reads_gap0", "reads7", "sharded", None, 0),
    ("sharded_long_len0_gap2", "longs", "sharded", 0, 2),
]


def _runs_host(rle_work, n):
    """(number of runs, first-run index per sequence) out of a run-length work buffer (kbo_hip.h kbo_run_lengths_dev)"""
    w = rle_work.host().view(np.uint32)
    words = n + 1 + (n + 1 + 1023) // 1024
    return int(w[words]), w[n + 1 + np.arange(n + 1) // 1024].astype(np.uint64) + w[:n + 1]


@pytest.mark.parametrize("short", [0, 5], ids=["capacity_exact", "capacity_short5"])
@pytest.mark.parametrize("case", FIND_CASES, ids=[c[0] for c in FIND_CASES])
def test_find_batch_dev_exact_buffers(world, oracle, case, short):
    import torch
    name, bkey, ikey, max_len, gap = case
    name = "%s, capacity runs - %d" % (name, short)
    L, b, sbwt = world["L"], world[bkey], world[ikey]
    ml = b.max_len if max_len is None else max_len
    want_recs, want_first = b.runs(oracle, gap)
    n_runs = len(want_recs)
    cap = n_runs - short
    wb = int(L.kbo_index_work_bytes(sbwt._h, b.n, b.total, ml))
    plain = int(L.kbo_work_bytes(b.n, b.total, ml, b.k))
    q, off = _concat_buf(b), _offsets_buf(b)
    ms, chars = _out("d_ms", b.total + 16), _out("d_chars_out", b.total + 16, 3)
    work = _scratch("d_work", wb, b)
    rle = _scratch("d_rle_work", int(L.kbo_run_lengths_work_bytes(b.n)), b)
    recs = _out("d_records", 28 * cap, 6)
    ts = torch.cuda.Stream(_dev())
    fused = C.c_int(-1)

    def call(work_bytes, work_=work):
        return L.kbo_find_batch_dev(sbwt._h, q.ptr, off.ptr, b.n, b.total, ml, 1e-7, gap, ms.ptr, chars.ptr, work_.ptr, work_bytes,
                                    rle.ptr, recs.ptr, cap, _stream(), ts.cuda_stream, C.byref(fused))

    def check():
        got = chars.host()
        _eq(got, b.chars, b.keep, name + ": characters")
        total, first = _runs_host(rle, b.n)
        assert total == n_runs, "%s: %d runs counted, %d expected" % (name, total, n_runs)
        assert np.array_equal(first, want_first), name + ": first-run indices"
        r = recs.host().view(np.uint32).reshape(-1, 7)
        assert np.array_equal(r.astype(np.uint64), want_recs[:cap]), name + ": records"
        return [got[:b.total][b.keep], first, r]

    bufs = [q, off, ms, chars, work, rle, recs]
    _twice(lambda: kbo_amd.check(call(wb)), check, [ms, chars, work, rle, recs], bufs, name)
    assert bool(fused.value) == (sbwt.shards() == 1), "%s: fused = %d" % (name, fused.value)
    short = [(name + ": d_work one byte short", lambda: call(wb - 1))]
    if sbwt.shards() > 1:
        short.append((name + ": d_work of kbo_work_bytes() over a sharded index", lambda: call(plain)))
        work_plain = _scratch("d_work of kbo_work_bytes()", plain, b)
        short.append((name + ": d_work allocated at kbo_work_bytes()", lambda: call(plain, work_plain), [work_plain]))
    _refused(short, bufs)


# ---------------------------------------------------------------------------------------------------------------- kbo_run_lengths_dev

@pytest.mark.parametrize("short", [0, 5], ids=["capacity_exact", "capacity_short5"])
@pytest.mark.parametrize("bkey,len0,gap", [("reads7", False, 0), ("reads0", False, 2), ("longs", True, 0), ("longs", False, 2)])
def test_run_lengths_dev_exact_buffers(world, oracle, bkey, len0, gap, short):
    L, b = world["L"], world[bkey]
    name = "run_lengths %s max_seq_len %s gap %d, capacity runs - %d" % (bkey, 0 if len0 else b.max_len, gap, short)
    want_recs, want_first = b.runs(oracle, gap)
    cap = len(want_recs) - short
    data = b.chars.copy()
    data[~b.keep] = ord("-")  # (the sequences of 1 and 2 bases: no alignment, no run)
    chars = Guarded("d_chars", b.total + 16, PER_BASE_GUARD, _dev(), seed=9, data=data)
    off = _offsets_buf(b)
    rle = _scratch("d_work", int(L.kbo_run_lengths_work_bytes(b.n)), b)
    recs = _out("d_records", 28 * cap, 6)

    def run():
        kbo_amd.check(L.kbo_run_lengths_dev(chars.ptr, off.ptr, b.n, 0 if len0 else b.max_len, gap, rle.ptr, recs.ptr, cap, _stream()))

    def check():
        total, first = _runs_host(rle, b.n)
        assert total == len(want_recs), "%s: %d runs counted, %d expected" % (name, total, len(want_recs))
        assert np.array_equal(first, want_first), name + ": first-run indices"
        r = recs.host().view(np.uint32).reshape(-1, 7)
        assert np.array_equal(r.astype(np.uint64), want_recs[:cap]), name + ": records"
        return [first, r]

    _twice(run, check, [rle, recs], [chars, off, rle, recs], name)


# ---------------------------------------------------------------------------------------------------------------- kbo_matches_packed_dev

def _pack(seq):
    """ACGT bytes -> 2-bit words (a multiple of 16 bases)"""
    s = np.ascontiguousarray(seq, dtype=np.uint8)[:len(seq) // 16 * 16]
    w, _, _ = batch.pack_reads(s, np.array([0, len(s)], dtype=np.uint64))
    return w


@pytest.mark.parametrize("bkey", ["uniform", "uniform_n", "mixed_clean", "reads7"])
def test_matches_packed_dev_exact_buffers(world, bkey):
    L, b, sbwt = world["L"], world[bkey], world["sbwt31"]
    name = "matches_packed " + bkey
    uniform = b.max_len if int(b.lens.min()) == b.max_len else 0
    assert (uniform != 0) == bkey.startswith("uniform")
    words, pos, byt = batch.pack_reads(b.concat, b.offsets)
    nw = int(L.kbo_packed_words(b.offsets.ctypes.data, b.n))
    assert nw == len(words)
    n_exc = len(pos)
    assert (n_exc > 0) == (bkey in ("uniform_n", "reads7"))
    # the guards: words that continue the genome in front of the first read and behind the last read's last word
    behind = TAIL + (-int(b.lens[-1])) % 16
    d_words = Guarded("d_words", 4 * nw, PER_BASE_GUARD, _dev(), data=words.view(np.uint8),
                      front_bytes=_pack(b.g0[HEAD - 16 * 1024:HEAD]).view(np.uint8),
                      back_bytes=_pack(np.resize(b.g0[behind:], 4 * PER_BASE_GUARD)).view(np.uint8))
    off = _offsets_buf(b)
    epos = Guarded("d_exc_pos", 8 * n_exc, PER_BASE_GUARD, _dev(), seed=10, data=pos.view(np.uint8)) if n_exc else None
    ebyt = Guarded("d_exc_byte", n_exc, PER_BASE_GUARD, _dev(), seed=11, data=byt) if n_exc else None
    out = _out("d_words_out", 4 * nw)  # (kbo_packed_words() words: the header names no slack here)
    scratch = _scratch("d_scratch", int(L.kbo_matches_packed_dev_scratch_bytes(b.n, b.total)), b)
    wb = int(L.kbo_work_bytes(b.n, b.total, b.max_len, b.k))
    work = _scratch("d_work", wb, b, seed=12)
    wkeep = np.repeat(b.lens >= 3, (b.lens + 15) // 16)  # (the words of the reads of 1 and 2 bases are unspecified)

    def call(work_bytes):
        return L.kbo_matches_packed_dev(sbwt._h, d_words.ptr, off.ptr, b.n, b.total, b.max_len, uniform, epos.ptr if n_exc else None,
                                        ebyt.ptr if n_exc else None, n_exc, 1e-7, out.ptr, scratch.ptr, work.ptr, work_bytes, _stream(),
                                        _stream())

    def check():
        got = out.host().view(np.uint32).copy()
        got[~wkeep] = 0
        _eq(batch.unpack_matches(got, b.offsets), b.chars, b.keep, name)
        return [got]

    bufs = [d_words, off] + ([epos, ebyt] if n_exc else []) + [out, scratch, work]
    _twice(lambda: kbo_amd.check(call(wb)), check, [out, scratch, work], bufs, name)
    _refused([(name + ": d_work one byte short", lambda: call(wb - 1))], bufs)


# ---------------------------------------------------------------------------------------------------------------- kbo_call_walk_dev, kbo_call_sites_dev

def _sites_cap(total):
    return (total // 4 + 8192) // LISTS * LISTS  # (as gpu_helpers.call_walk_sites sizes it)


def _sites(sites, count, cap, n_counters):
    c = count.host().view(np.uint32)
    seg = cap // LISTS
    assert (c[:LISTS * 16:16] <= seg).all(), "a site list overflowed"
    assert n_counters == LISTS or int(c[LISTS * 16]) == 0, "a read had more than four breakpoints waiting"
    h = sites.host().view(np.uint32).reshape(-1, 4)
    raw = np.concatenate([h[g * seg:g * seg + int(c[g * 16])] for g in range(LISTS)])
    return raw[raw[:, 0] != 0xFFFFFFFF]


@pytest.mark.parametrize("bkey", ["reads7", "reads0"])
def test_call_walk_dev_exact_buffers(world, bkey):
    L, b, sbwt = world["L"], world[bkey], world["sbwt31"]
    name = "call_walk " + bkey
    thr = derandomize.random_match_threshold(b.k, sbwt.n_kmers(), 4, 1e-7)
    want = {(int(b.offsets[s]) + i, int(b.offsets[s]) + j, r) for s, i, j, r in b.sites(thr)}  # (as gpu_helpers.oracle_sites gives them)
    assert len(want) > 100
    cap = _sites_cap(b.total)
    wb = int(L.kbo_ms_work_bytes(b.n, b.total, b.max_len, b.k))
    q, off = _concat_buf(b), _offsets_buf(b)
    ms = _out("d_ms_out", b.total + 16)
    sites = _out("d_sites", 16 * cap, 3)
    count = _out("d_count", LISTS * 64 + 64, 4)
    work = _scratch("d_work", wb, b)

    def call(work_bytes):
        return L.kbo_call_walk_dev(sbwt._h, q.ptr, off.ptr, b.n, b.total, b.max_len, thr, ms.ptr, sites.ptr, cap, count.ptr, work.ptr,
                                   work_bytes, _stream())

    def check():
        gm = ms.host()
        _eq(gm, b.d, b.keep, name + ": MS values")
        got = {(int(i), int(j), int(r)) for i, j, r, _ in _sites(sites, count, cap, LISTS + 1)}
        assert got == want, "%s: %d sites missing, %d extra" % (name, len(want - got), len(got - want))
        return [gm[:b.total][b.keep], np.array(sorted(got))]

    bufs = [q, off, ms, sites, count, work]
    _twice(lambda: kbo_amd.check(call(wb)), check, [ms, sites, count, work], bufs, name)
    _refused([(name + ": d_work one byte short", lambda: call(wb - 1))], bufs)


def test_call_sites_dev_exact_buffers(world):
    L, b, sbwt = world["L"], world["reads7"], world["sbwt31"]
    thr = derandomize.random_match_threshold(b.k, sbwt.n_kmers(), 4, 1e-7)
    want = b.sites(thr)
    assert len(want) > 100
    d = np.zeros(b.total, dtype=np.uint8)
    lo, hi = np.zeros(b.total, dtype=np.uint32), np.zeros(b.total, dtype=np.uint32)
    for s in range(b.n):
        a, e = int(b.offsets[s]), int(b.offsets[s + 1])
        d[a:e], lo[a:e], hi[a:e] = b.ora.matching_statistics(b.concat[a:e])
    dms = Guarded("d_ms", b.total + 16, PER_BASE_GUARD, _dev(), seed=13, data=d)
    dlo = Guarded("d_lo", 4 * b.total, PER_BASE_GUARD, _dev(), seed=14, data=lo.view(np.uint8))
    dhi = Guarded("d_hi", 4 * b.total, PER_BASE_GUARD, _dev(), seed=15, data=hi.view(np.uint8))
    off = _offsets_buf(b)
    cap = _sites_cap(b.total)
    sites = _out("d_sites", 16 * cap, 3)
    count = _out("d_count", LISTS * 64, 4)  # (KBO_CALL_LISTS counters 64 bytes apart: 16 KiB)

    def run():
        kbo_amd.check(L.kbo_call_sites_dev(dms.ptr, dlo.ptr, dhi.ptr, off.ptr, b.n, b.total, b.k, thr, sites.ptr, cap, count.ptr, _stream()))

    def check():
        got = {tuple(int(v) for v in r) for r in _sites(sites, count, cap, LISTS)}
        assert got == want, "call_sites: %d sites missing, %d extra" % (len(want - got), len(got - want))
        return [np.array(sorted(got))]

    _twice(run, check, [sites, count], [dms, dlo, dhi, off, sites, count], "call_sites")


# ---------------------------------------------------------------------------------------------------------------- kbo_map_stream_*

def test_map_stream_exact_buffers(world):
    """two pipelines, seven batches (every slot taken again), the last of them exactly max_seqs / max_bases of create"""
    L, big, sbwt = world["L"], world["reads7"], world["sbwt31"]
    h = C.c_void_p()
    kbo_amd.check(L.kbo_map_stream_create(sbwt._h, 2, big.n, big.total, 160, C.byref(h)))
    try:
        cuts = [0, 211, 650, 651, 1100, 1400, big.n]
        parts = [(cuts[i], cuts[i + 1]) for i in range(len(cuts) - 1)] + [(0, big.n)]
        jobs = []
        for i, (s0, s1) in enumerate(parts):
            a, e = int(big.offsets[s0]), int(big.offsets[s1])
            o = (big.offsets[s0:s1 + 1] - big.offsets[s0]).astype(np.uint64)
            n, total = s1 - s0, e - a
            q = Guarded("d_concat", total + 16, PER_BASE_GUARD, _dev(), seed=20 + i, data=big.concat[a:e],
                        back_bytes=np.resize(big.g0[TAIL:], 16 + PER_BASE_GUARD) if s1 == big.n else None)
            off = Guarded("d_offsets", 8 * (n + 1), PER_BASE_GUARD, _dev(), seed=30 + i, data=o.view(np.uint8))
            chars = _out("d_chars_out", total + 16, 40 + i)
            ms = _out("d_ms_out", total + 16, 50 + i) if i % 2 else None
            jobs.append((a, e, n, total, int(np.diff(o.astype(np.int64)).max()), i % 3 == 0, q, off, chars, ms))
        tickets = []
        for a, e, n, total, ml, fmt, q, off, chars, ms in jobs:
            t = C.c_uint64(0)
            kbo_amd.check(L.kbo_map_stream_submit(h, q.ptr, off.ptr, n, total, ml, 1e-7, int(fmt), ms.ptr if ms else None, chars.ptr,
                                                  None, C.byref(t), None))
            tickets.append(t.value)
        for t in tickets:
            kbo_amd.check(L.kbo_map_stream_wait(h, t))
        kbo_amd.check(L.kbo_map_stream_sync(h))
        _sync()
        assert jobs[-1][2] == big.n and jobs[-1][3] == big.total
        for i, (a, e, n, total, ml, fmt, q, off, chars, ms) in enumerate(jobs):
            what = "map_stream batch %d (%d sequences)" % (i, n)
            keep = big.keep[a:e]
            _eq(chars.host(), (big.map if fmt else big.chars)[a:e], keep, what + ": characters")
            if ms:
                _eq(ms.host(), big.d[a:e], keep, what + ": MS values")
            for x in [q, off, chars] + ([ms] if ms else []):
                x.assert_intact(what)
    finally:
        L.kbo_map_stream_free(h)
