"""kbo_index_build_device (build_kernels.hip + build_device.cpp): the index the device builds is the host builder's bit for bit -
k, n_kmers, n_sets, C, rows and LCS - over every key width, add_revcomp, N runs, lower case, short and repetitive input; small
inputs against the oracle's independent builder as well.  The device copy it leaves equals the one kbo_index_to_device makes from
a host-built handle, and queries through either handle give the same answers."""
import ctypes as C
import os

import numpy as np
import pytest

import kbo_amd
from kbo_amd import batch, synth

pytestmark = pytest.mark.gpu

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
KS = [1, 2, 3, 5, 11, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255]


def _pair(seqs, k, rc=False):
    o = kbo_amd.BuildOpts(k=k, add_revcomp=rc, num_threads=8)
    host, _ = kbo_amd.build(seqs, o)
    dev, _ = kbo_amd.build(seqs, o, device=0)
    return host, dev


def _same(a, b, what=""):
    assert (a.k(), a.n_sets(), a.n_kmers()) == (b.k(), b.n_sets(), b.n_kmers()), what
    ra, Ca, la = a.export_parts()
    rb, Cb, lb = b.export_parts()
    assert list(Ca) == list(Cb), what
    for c in range(4):
        assert np.array_equal(ra[c], rb[c]), (what, "row", c)
    assert np.array_equal(la, lb), (what, "lcs")


def _same_as_oracle(oracle, prod, seqs, k, rc):
    ora = oracle.Index.build(seqs, k=k, add_revcomp=rc)
    rows, Carr, lcs = prod.export_parts()
    assert (prod.k(), prod.n_sets(), prod.n_kmers()) == (ora.k, ora.n_sets, ora.n_kmers)
    assert list(Carr) == list(ora.C)
    for c in range(4):
        assert np.array_equal(rows[c], ora.bits(c))
    assert np.array_equal(lcs, ora.lcs())


def _rand(rng, n, lo, hi):
    return [ACGT[rng.integers(0, 4, int(rng.integers(lo, hi)))].tobytes() for _ in range(n)]


@pytest.mark.parametrize("rc", [False, True])
@pytest.mark.parametrize("k", KS)
def test_every_key_width(oracle, k, rc):
    rng = np.random.default_rng(40 + k)
    seqs = _rand(rng, 4, max(k, 5), 3 * k + 300)
    s = bytearray(seqs[1])
    s[len(s) // 3: len(s) // 3 + 4] = b"NNNN"  # an N run splits the ACGT runs
    seqs[1] = bytes(s)
    seqs.append(seqs[0][: len(seqs[0]) // 2])  # equal k-mers
    seqs.append(b"ACG")                        # shorter than k for most k
    host, dev = _pair(seqs, k, rc)
    _same(host, dev, (k, rc))
    _same_as_oracle(oracle, dev, seqs, k, rc)
    # lower case splits a run, as on the host
    low = [seqs[0][:40].lower() + seqs[0][40:], seqs[2][:-7] + seqs[2][-7:].lower()]
    _same(*_pair(low, k, rc), (k, rc, "lower case"))


def test_short_homopolymer_and_empty(oracle):
    short = [b"ACGTA", b"", b"GGT", b"acgtacgtacgt"]
    for k in (11, 31, 64):
        host, dev = _pair(short, k)
        assert dev.n_sets() == 1 and dev.n_kmers() == 0  # no k-mer at all: the root only
        _same(host, dev, k)
    for k, rc in ((1, False), (31, False), (31, True), (100, True)):
        seqs = [b"A" * 5000]
        host, dev = _pair(seqs, k, rc)
        _same(host, dev, ("homopolymer", k, rc))
        _same_as_oracle(oracle, dev, seqs, k, rc)


def test_many_short_contigs():
    rng = np.random.default_rng(3)
    lens = rng.integers(50, 301, 100_000)
    pool = ACGT[rng.integers(0, 4, int(lens.sum()))].tobytes()
    seqs, at = [], 0
    for n in lens:
        seqs.append(pool[at:at + int(n)])
        at += int(n)
    for rc in (False, True):
        _same(*_pair(seqs, 31, rc), ("contigs", rc))


def test_repeat_rich_genome():
    rng = np.random.default_rng(11)
    unit = ACGT[rng.integers(0, 4, 2000)]
    copies = []
    for _ in range(300):
        u = unit.copy()
        pos = rng.integers(0, len(u), 6)
        u[pos] = ACGT[rng.integers(0, 4, len(pos))]
        copies.append(u)
    g = np.concatenate(copies).tobytes()
    for k in (31, 63):
        _same(*_pair([g], k, True), ("repeats", k))


def test_20mbp_genome_and_the_copy_it_leaves(tmp_path):
    L = kbo_amd.lib()
    g = synth.genome(20_000_000)
    host, dev = _pair([g], 31)
    _same(host, dev, "20 Mbp")
    # the device-built handle's copy is there already; the host-built one gets it from kbo_index_to_device
    host.to_device(0)
    for h in (dev, host):
        d1, d2 = C.c_uint64(1), C.c_uint64(1)
        kbo_amd.check(L.kbo_index_layout_check(h._h, 0, C.byref(d1)))
        kbo_amd.check(L.kbo_index_cover_check(h._h, C.byref(d2)))
        assert d1.value == 0 and d2.value == 0
    la, lb = dev.device_layout(0), host.device_layout(0)
    for f in la:
        if f.endswith("_bytes") or f in ("entries_64bit", "seed_depth", "dtab_order", "dtab_grouped"):
            assert la[f] == lb[f], f
    pa, pb = str(tmp_path / "dev.kbo"), str(tmp_path / "host.kbo")
    kbo_amd.index.save_flat(pa, dev)
    kbo_amd.index.save_flat(pb, host)
    assert open(pa, "rb").read() == open(pb, "rb").read()
    # queries through either handle
    concat, offsets = synth.reads(g, 2000, 150, 0.01, seed=9)
    assert np.array_equal(batch.matches_batch(dev, concat, offsets), batch.matches_batch(host, concat, offsets))
    assert np.array_equal(batch.map_batch(dev, concat, offsets), batch.map_batch(host, concat, offsets))
    assert repr(batch.find_batch(dev, concat, offsets)) == repr(batch.find_batch(host, concat, offsets))
    ref = g[5_000_000:5_050_000].tobytes()
    assert kbo_amd.map(ref, dev) == kbo_amd.map(ref, host)
    lc, lo = synth.reads(g, 8, 3000, 0.01, seed=5)
    co = kbo_amd.CallOpts(sbwt_build_opts=kbo_amd.BuildOpts(k=31, build_select=True))
    got_d = batch.call_batch(dev, lc, lo, co)
    got_h = batch.call_batch(host, lc, lo, co)
    key = lambda vs: [[(v.query_pos, bytes(v.query_chars), bytes(v.ref_chars)) for v in s] for s in vs]  # noqa: E731
    assert key(got_d) == key(got_h)


def test_current_device_is_unchanged():
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    hip = C.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
    assert hip.hipSetDevice(1) == 0
    try:
        g = synth.genome(200_000)
        host, dev = _pair([g], 31)
        cur = C.c_int(-1)
        assert hip.hipGetDevice(C.byref(cur)) == 0 and cur.value == 1
        _same(host, dev)
        d = C.c_uint64(1)
        kbo_amd.check(kbo_amd.lib().kbo_index_layout_check(dev._h, 0, C.byref(d)))
        assert d.value == 0
    finally:
        hip.hipSetDevice(0)
