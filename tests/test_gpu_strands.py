"""Both strands in one batch (kbo_hip.h "both strands").

Kernels: kbo_revcomp_batch_dev / kbo_revcomp_packed_dev at exactly their documented buffer sizes behind guard bands
(gpu_helpers.Guarded), against a numpy restatement of the definition.

Pipelines: kbo_matches_batch_strands (format 0 and 1), kbo_find_batch_strands (max_gap_len 0 and 5) and the packed pair with
strands = 1, 2 and 3 over forward-only indexes at k = 31 and k = 63.  Every expected value is the oracle's for the reads as given
('+') and for the reads reverse-complemented by numpy here ('-'); nothing comes from the library under test.  Each batch runs once
more cut into 64 KiB slabs.  The batch is staged once: kbo_last_batch_staged_bytes() is the same for both strands as for one."""
import numpy as np
import pytest

import kbo_amd
from kbo_amd import batch, synth
from gpu_helpers import Guarded, threads
from oracle import binding as ora

pytestmark = pytest.mark.gpu

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
COMP = np.arange(256, dtype=np.uint8)
for _a, _b in zip(b"ACGTacgt", b"TGCAtgca"):
    COMP[_a] = _b
CODE = np.full(256, 4, dtype=np.uint8)
for _i, _c in enumerate(b"ACGT"):
    CODE[_c] = _i
GUARD = 64 << 10
DEFAULT_SLAB = 16 << 20


def _dev():
    import torch
    return torch.device("cuda:0")


def _stream():
    import torch
    return torch.cuda.current_stream(_dev()).cuda_stream


def _sync():
    import torch
    torch.cuda.synchronize()


def np_revcomp(concat, offsets):
    out = np.empty_like(concat)
    for s in range(len(offsets) - 1):
        a, b = int(offsets[s]), int(offsets[s + 1])
        out[a:b] = COMP[concat[a:b][::-1]]
    return out


def np_pack(concat, offsets):
    """the packed layout of kbo_hip.h restated: (words, exception positions, exception bytes, mask of the bits that are specified)"""
    words, masks = [], []
    for s in range(len(offsets) - 1):
        q = concat[int(offsets[s]):int(offsets[s + 1])]
        nw = (len(q) + 15) // 16
        c = np.zeros(nw * 16, dtype=np.uint64)
        m = np.zeros(nw * 16, dtype=np.uint64)
        c[:len(q)] = CODE[q] & 3
        m[:len(q)] = np.where(CODE[q] < 4, 3, 0)  # (the 2 bits at a listed position are unspecified)
        m[len(q):] = 3                            # (padding: specified, zero)
        sh = (2 * np.arange(16, dtype=np.uint64))[None, :]
        words.append((c.reshape(nw, 16) << sh).sum(axis=1).astype(np.uint32))
        masks.append((m.reshape(nw, 16) << sh).sum(axis=1).astype(np.uint32))
    pos = np.flatnonzero(CODE[concat] == 4).astype(np.uint64)
    cat = (lambda v: np.concatenate(v) if v else np.zeros(0, dtype=np.uint32))
    return cat(words), pos, concat[pos.astype(np.int64)].copy(), cat(masks)


def offsets_of(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)


def spiced(rng, total, rate=0.05):
    q = ACGT[rng.integers(0, 4, total)].copy()
    r = rng.random(total)
    q[r < rate * 0.3] = ord("N")
    low = (r >= rate * 0.3) & (r < rate * 0.8)
    q[low] |= 0x20
    high = (r >= rate * 0.8) & (r < rate)
    q[high] = rng.integers(0x80, 0x100, int(high.sum()), dtype=np.uint8)
    return q


def assert_only_buffer_changed(g, lo, hi, what):
    """nothing of the tensor outside buffer bytes [lo, hi) differs from what fill() wrote"""
    diff = (g.t != g.image)
    diff[g.front + lo:g.front + hi] = False
    bad = diff.nonzero()
    assert len(bad) == 0, "%s: %s: %d bytes outside the output changed, first at tensor offset %d (buffer starts at %d)" % (
        what, g.name, len(bad), int(bad[0]), g.front)


# ------------------------------------------------------------------------------------------------------------------ kernels

BYTE_CASES = {
    "len_0_to_40": lambda rng: rng.permutation(np.repeat(np.arange(0, 41), 7)),
    "reads_150": lambda rng: np.full(3000, 150),
    "mixed_1_to_400": lambda rng: rng.integers(1, 401, 2500),
    "long": lambda rng: np.array([10_000, 3, 10_001, 0, 1_000_000, 17, 9_999, 1]),
}


@pytest.mark.parametrize("shift", [0, 4, 12])
@pytest.mark.parametrize("case", sorted(BYTE_CASES))
def test_revcomp_bytes_kernel_behind_guards(case, shift):
    """d_concat: total + 16 bytes; d_out: exactly total bytes, 4-byte aligned (shift: where it begins within a 16-byte block)"""
    import zlib
    rng = np.random.default_rng(zlib.crc32(case.encode()) + shift)
    lens = BYTE_CASES[case](rng)
    offsets = offsets_of(lens)
    total = int(offsets[-1])
    concat = spiced(rng, total)
    exp = np_revcomp(concat, offsets)
    L = kbo_amd.lib()
    dev = _dev()
    tail = spiced(rng, 16)  # (the slack holds letters too: a kernel that mirrors them in changes its result)
    d_in = Guarded("d_concat", total + 16, GUARD, dev, seed=1, data=np.concatenate([concat, tail]), front_bytes=spiced(rng, 4096))
    d_off = Guarded("d_offsets", 8 * len(offsets), GUARD, dev, seed=2, data=offsets.view(np.uint8))
    d_out = Guarded("d_out", total + shift, GUARD, dev, seed=3)
    for rnd in range(2):
        if rnd:
            d_out.fill(40 + rnd)  # (another pattern: nothing relies on what the output held)
        kbo_amd.check(L.kbo_revcomp_batch_dev(d_in.ptr, d_off.ptr, len(lens), total, int(lens.max()) if rnd else 0, d_out.ptr + shift, _stream()))
        _sync()
        got = d_out.host()[shift:]
        bad = np.flatnonzero(got != exp)
        assert len(bad) == 0, "%s: %d bases differ, first at %d" % (case, len(bad), int(bad[0]))
        assert_only_buffer_changed(d_out, shift, shift + total, case)
        d_in.assert_intact(case)
        d_off.assert_intact(case)
        assert not d_in.changed() and not d_off.changed(), "inputs are read-only"


PACKED_CASES = {
    "every_len_mod_16": lambda rng: rng.permutation(np.concatenate([np.arange(1, 101), np.arange(1, 40)])),
    "reads_150": lambda rng: np.full(2000, 150),
    "with_long": lambda rng: np.array([10_000, 16, 10_001, 1, 32, 300_007, 15, 17, 33]),
}


@pytest.mark.parametrize("case", sorted(PACKED_CASES))
def test_revcomp_packed_kernel_behind_guards(case):
    import zlib
    rng = np.random.default_rng(zlib.crc32(case.encode()))
    lens = PACKED_CASES[case](rng)
    offsets = offsets_of(lens)
    total = int(offsets[-1])
    concat = ACGT[rng.integers(0, 4, total)].copy()
    # exceptions: at the first and at the last base of some sequences, a few inside; most sequences have none
    for s in rng.choice(len(lens), max(3, len(lens) // 6), replace=False):
        a, b = int(offsets[s]), int(offsets[s + 1])
        which = rng.integers(0, 4)
        if which in (0, 2):
            concat[a] = ord("N")
        if which in (1, 2):
            concat[b - 1] = ord("n")
        if which == 3:
            concat[a + int(rng.integers(0, b - a))] = 0x80 + int(rng.integers(0, 100))
    words, epos, ebyt, _ = np_pack(concat, offsets)
    assert len(epos) >= 3
    exp_words, exp_pos, exp_byt, mask = np_pack(np_revcomp(concat, offsets), offsets)
    L = kbo_amd.lib()
    dev = _dev()
    nw, ne = len(words), len(epos)
    assert nw == L.kbo_packed_words(offsets.ctypes.data, len(lens))
    scr_bytes = int(L.kbo_revcomp_packed_scratch_bytes(len(lens)))
    assert scr_bytes > 0
    d_w = Guarded("d_words", 4 * nw, GUARD, dev, seed=1, data=words.view(np.uint8))
    d_off = Guarded("d_offsets", 8 * len(offsets), GUARD, dev, seed=2, data=offsets.view(np.uint8))
    d_ep = Guarded("d_exc_pos", 8 * ne, GUARD, dev, seed=3, data=epos.view(np.uint8))
    d_eb = Guarded("d_exc_byte", ne, GUARD, dev, seed=4, data=ebyt)
    d_wo = Guarded("d_words_out", 4 * nw, GUARD, dev, seed=5)
    d_epo = Guarded("d_exc_pos_out", 8 * ne, GUARD, dev, seed=6)
    d_ebo = Guarded("d_exc_byte_out", ne, GUARD, dev, seed=7)
    d_scr = Guarded("d_scratch", scr_bytes, GUARD, dev, seed=8)
    for rnd in range(2):
        if rnd:
            for g in (d_wo, d_epo, d_ebo, d_scr):
                g.fill(50 + rnd)
        kbo_amd.check(L.kbo_revcomp_packed_dev(d_w.ptr, d_off.ptr, len(lens), nw, d_ep.ptr, d_eb.ptr, ne, d_wo.ptr, d_epo.ptr, d_ebo.ptr,
                                               d_scr.ptr, _stream()))
        _sync()
        got_w = d_wo.host().view(np.uint32)
        bad = np.flatnonzero((got_w & mask) != (exp_words & mask))
        assert len(bad) == 0, "%s: %d words differ, first %d: %08x against %08x" % (case, len(bad), int(bad[0]), got_w[bad[0]], exp_words[bad[0]])
        got_pos = d_epo.host().view(np.uint64)
        assert np.array_equal(got_pos, exp_pos), "mirrored exception positions (ascending again)"
        assert np.array_equal(d_ebo.host(), exp_byt), "complemented exception bytes"
        for g in (d_w, d_off, d_ep, d_eb, d_wo, d_epo, d_ebo, d_scr):
            g.assert_intact(case)
        assert not any(g.changed() for g in (d_w, d_off, d_ep, d_eb)), "inputs are read-only"


# ---------------------------------------------------------------------------------------------------------------- pipelines

def draw(rng, g, length, edit=True):
    """a read of `length` bases from either strand of g: 1 % substitutions, now and then an indel or an N -> (read, strand, edited)"""
    p = int(rng.integers(0, len(g) - length - 2))
    q = g[p:p + length].copy()
    edited = False
    if edit:
        hit = rng.random(length) < 0.01
        if hit.any():
            q[hit] = ACGT[(CODE[q[hit]] + rng.integers(1, 4, int(hit.sum()))) % 4]
            edited = True
        r = rng.random()
        if r < 0.04 and length > 20:    # deletion (the read stays `length` long: one more base of the genome at its end)
            i = int(rng.integers(5, length - 5))
            q = np.concatenate([q[:i], q[i + 1:], g[p + length:p + length + 1]])
            edited = True
        elif r < 0.08 and length > 20:  # insertion
            i = int(rng.integers(5, length - 5))
            q = np.concatenate([q[:i], ACGT[rng.integers(0, 4, 1)], q[i:-1]])
            edited = True
        elif r < 0.12:
            q[int(rng.integers(0, length))] = ord("N")
            edited = True
    minus = rng.random() < 0.5
    if minus:
        q = COMP[q[::-1]].copy()
    return q, minus, edited


class Setup:
    def __init__(self, k, genome_len, kind, seed):
        rng = np.random.default_rng(seed)
        self.k = k
        self.g = synth.genome(genome_len, seed=seed)
        self.sbwt, _ = kbo_amd.build([self.g], kbo_amd.BuildOpts(k=k, num_threads=threads()))
        self.oi = ora.Index.build([self.g.tobytes()], k=k)
        if kind == "reads":  # <= 160 bases
            lens = np.full(4000, 150) if k == 31 else rng.integers(70, 161, 4000)
        else:                # mixed, with 10 kbp sequences
            lens = rng.permutation(np.concatenate([np.full(6, 10_000), rng.integers(3, 400, 1500), rng.integers(400, 3000, 60), np.full(300, 150)]))
        seqs, self.minus, self.edited = [], [], []
        for n in lens:
            q, minus, edited = draw(rng, self.g, int(n), edit=rng.random() < 0.8)
            seqs.append(q)
            self.minus.append(minus)
            self.edited.append(edited)
        self.concat = np.concatenate(seqs)
        self.offsets = offsets_of(lens)
        self.n = len(lens)
        self.rc = np_revcomp(self.concat, self.offsets)
        nt = threads()
        # what the single-strand entry points return for the reads ('+') and for their reverse complements ('-'), by the oracle
        self.exp = {1: self.oi.matches_batch(self.concat, self.offsets, 1e-7, n_threads=nt),
                    2: self.oi.matches_batch(self.rc, self.offsets, 1e-7, n_threads=nt)}
        self.exp_fmt = {1: np.frombuffer(ora.relative_to_ref(self.concat, self.exp[1]), dtype=np.uint8),
                        2: np.frombuffer(ora.relative_to_ref(self.rc, self.exp[2]), dtype=np.uint8)}

    def exp_runs(self, strands, gap):
        """the 2 n + 1 layout: per sequence the '+' runs, then the '-' runs; a strand not asked for has none"""
        per = {st: ora.run_lengths_batch(self.exp[st], self.offsets, gap) for st in (1, 2) if strands & st}
        recs, ro = [], [0]
        for s in range(self.n):
            for st in (1, 2):
                if strands & st:
                    r, o = per[st]
                    recs.append(r[int(o[s]):int(o[s + 1])])
                ro.append(ro[-1] + (len(recs[-1]) if strands & st else 0))
        return np.concatenate(recs), np.array(ro, dtype=np.uint64)


_SETUPS = {}


def setup_for(k, kind):
    key = (k, kind)
    if key not in _SETUPS:
        _SETUPS.clear()  # (one at a time: an index and its oracle are not small)
        _SETUPS[key] = Setup(k, 400_000 if k == 31 else 250_000, kind, seed=1000 + k + (7 if kind == "reads" else 0))
    return _SETUPS[key]


def same_per_read(got, exp, offsets, what):
    bad = np.flatnonzero(got != exp)
    if len(bad):
        s = int(np.searchsorted(offsets, bad[0], side="right")) - 1
        raise AssertionError("%s: %d characters differ, first in read %d at %d" % (what, len(bad), s, int(bad[0]) - int(offsets[s])))


def check_all(S, slab_note=""):
    L = kbo_amd.lib()
    words, epos, ebyt = batch.pack_reads(S.concat, S.offsets)
    staged = {}
    for strands in (1, 2, 3):
        tag = "k=%d strands=%d%s" % (S.k, strands, slab_note)
        for fmt in (False, True):
            fwd, rev = batch.matches_batch_strands(S.sbwt, S.concat, S.offsets, 1e-7, format=fmt, strands=strands)
            if not fmt:
                staged["bytes", strands] = batch.last_batch_staged_bytes()
            exp = S.exp_fmt if fmt else S.exp
            assert (fwd is not None) == bool(strands & 1) and (rev is not None) == bool(strands & 2)
            if strands & 1:
                same_per_read(fwd, exp[1], S.offsets, tag + " format=%d '+'" % fmt)
            if strands & 2:
                same_per_read(rev, exp[2], S.offsets, tag + " format=%d '-'" % fmt)
        wf, wr = batch.matches_batch_packed_strands(S.sbwt, words, S.offsets, epos, ebyt, 1e-7, strands=strands)
        staged["packed", strands] = batch.last_batch_staged_bytes()
        if strands & 1:
            same_per_read(batch.unpack_matches(wf, S.offsets), S.exp[1], S.offsets, tag + " packed '+'")
        if strands & 2:
            same_per_read(batch.unpack_matches(wr, S.offsets), S.exp[2], S.offsets, tag + " packed '-'")
        for gap in (0, 5):
            exp_recs, exp_ro = S.exp_runs(strands, gap)
            for name, (recs, ro) in (("find", batch.find_batch_strands(S.sbwt, S.concat, S.offsets, kbo_amd.FindOpts(max_gap_len=gap), strands=strands)),
                                     ("find packed", batch.find_batch_packed_strands(S.sbwt, words, S.offsets, epos, ebyt,
                                                                                     kbo_amd.FindOpts(max_gap_len=gap), strands=strands))):
                assert len(ro) == 2 * S.n + 1 and ro[0] == 0 and np.all(np.diff(ro.astype(np.int64)) >= 0), tag + " " + name + ": rle_offsets monotone, 2 n + 1"
                assert np.array_equal(ro, exp_ro), tag + " %s gap=%d: rle_offsets" % (name, gap)
                assert np.array_equal(np.asarray(recs, dtype=np.uint64).reshape(-1, 7), exp_recs), tag + " %s gap=%d: records" % (name, gap)
    return staged


@pytest.mark.parametrize("kind", ["reads", "mixed"])
@pytest.mark.parametrize("k", [31, 63])
def test_strand_pipelines_against_the_oracle(k, kind):
    S = setup_for(k, kind)
    # not vacuous: the strands differ for many reads, and an unedited read of the '-' strand is all 'M' on '-'
    differ = sum(not np.array_equal(S.exp[1][int(S.offsets[s]):int(S.offsets[s + 1])], S.exp[2][int(S.offsets[s]):int(S.offsets[s + 1])])
                 for s in range(S.n))
    assert differ >= 0.4 * S.n, "only %d of %d reads have different '+' and '-' outputs" % (differ, S.n)
    clean_minus = [s for s in range(S.n) if S.minus[s] and not S.edited[s] and S.offsets[s + 1] - S.offsets[s] >= 100]
    assert len(clean_minus) >= 20
    for s in clean_minus:
        assert np.all(S.exp[2][int(S.offsets[s]):int(S.offsets[s + 1])] == ord("M"))
    staged = check_all(S)
    # the upload claim: both strands stage what one strand stages
    for form in ("bytes", "packed"):
        assert staged[form, 3] == staged[form, 1] == staged[form, 2], "%s: staged %r" % (form, {st: staged[form, st] for st in (1, 2, 3)})
    assert staged["bytes", 1] >= len(S.concat) and staged["packed", 1] >= len(S.concat) // 4
    assert staged["packed", 1] < staged["bytes", 1]


@pytest.mark.parametrize("kind", ["reads", "mixed"])
def test_strand_pipelines_over_many_slabs(kind):
    S = setup_for(31, kind)
    L = kbo_amd.lib()
    kbo_amd.check(L.kbo_set_slab_bytes(64 << 10))
    try:
        check_all(S, " slabs of 64 KiB")
    finally:
        kbo_amd.check(L.kbo_set_slab_bytes(DEFAULT_SLAB))
