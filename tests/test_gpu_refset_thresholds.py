"""kbo_find_refset over references whose thresholds differ: one slab holds them all (the derandomize / translate stage behind the
walk takes a threshold per pair, kbo_hip.h kbo_derand_translate_seq_dev), and contigs above 65 536 bases need nothing of their own.

Expected records: oracle.run_lengths_gapped(oracle.Index.build([ref_r], k).matches(seq_s or its reverse complement), max_gap_len),
one oracle index per reference; compared as one ordered list."""
import numpy as np
import pytest

import kbo_amd
from kbo_amd import derandomize, refset
from oracle import binding as ora

pytestmark = pytest.mark.gpu

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
COMP = np.arange(256, dtype=np.uint8)
for _a, _b in zip(b"ACGT", b"TGCA"):
    COMP[_a] = _b
DEFAULT_SLAB = 16 << 20


def _rnd(rng, n):
    return ACGT[rng.integers(0, 4, n)].copy()


def _revcomp(a):
    return COMP[a[::-1]]


_cache = {}


def _world(name):
    """references, query sequences, the set under test, its thresholds and the oracle's alignment of every (reference, sequence,
    strand) - made once"""
    if name not in _cache:
        if name == "k31":
            k, rng = 31, np.random.default_rng(3100)
            refs = [_rnd(rng, n) for n in (100, 300, 1000, 10000)]
            big = _rnd(rng, 70000)
            big[500:600] = refs[0]
            big[2000:2300] = refs[1]
            big[5000:6000] = refs[2]
            big[20000:30000] = refs[3]
            big[65536 - 150:65536 + 150] = refs[1]          # across position 65 536
            big[40000:41000] = _revcomp(refs[2])            # a reverse-complemented copy
            seqs = [big, _rnd(rng, 200), _rnd(rng, 3)]
        else:
            k, rng = 96, np.random.default_rng(9600)
            refs = [_rnd(rng, n) for n in (200, 12000, 300)]
            big = _rnd(rng, 66000)
            big[1000:1200] = refs[0]
            big[30000:42000] = refs[1]
            big[65536 - 100:65536 + 200] = refs[2]
            big[50000:50200] = _revcomp(refs[0])
            seqs = [big, _rnd(rng, 150)]
        rs = refset.RefSet.build(refs, kbo_amd.BuildOpts(k=k, num_threads=4))
        thr = [derandomize.random_match_threshold(k, rs.n_kmers(r), 4, 1e-7) for r in range(len(refs))]
        aln = {}
        for r, ref in enumerate(refs):
            oi = ora.Index.build([ref.tobytes()], k=k)
            assert rs.status(r) == 0 and rs.n_kmers(r) == oi.n_kmers
            for s, q in enumerate(seqs):
                aln[r, s, 1] = oi.matches(q.tobytes(), 1e-7)
                aln[r, s, 2] = oi.matches(_revcomp(q).tobytes(), 1e-7)
        _cache[name] = (k, refs, seqs, rs, thr, aln)
    return _cache[name]


def _expected(name, gap, strands=3):
    k, refs, seqs, rs, thr, aln = _world(name)
    out = []
    for r in range(len(refs)):
        for s in range(len(seqs)):
            for strand in (1, 2):
                if strands & strand:
                    out += [(r, s, strand) + t for t in ora.run_lengths_gapped(aln[r, s, strand], gap)]
    return out


def _find(name, gap, strands=3):
    k, refs, seqs, rs, thr, aln = _world(name)
    rec = refset.find_refset(seqs, rs, kbo_amd.FindOpts(max_gap_len=gap), strands=strands)
    return [tuple(int(v) for v in row) for row in rec.tolist()]


@pytest.mark.parametrize("gap", [0, 5])
def test_one_slab_mixes_thresholds(gap):
    k, refs, seqs, rs, thr, aln = _world("k31")
    assert len(set(thr)) >= 3 and thr == [14, 15, 16, 18]
    got, exp = _find("k31", gap), _expected("k31", gap)
    assert len(exp) >= 6 and {t[0] for t in exp} == {0, 1, 2, 3} and {t[2] for t in exp} == {1, 2}
    assert got == exp
    lds, own, pairs, slabs = refset.last_routes()
    assert (lds, own, pairs) == (4, 0, 4 * len(seqs) * 2)
    assert slabs == 1  # 0.56 MB of pairs, far inside one 16 MiB slab: no cut where the threshold changes


def test_the_same_set_in_slabs_of_64_kib():
    base = _find("k31", 5)
    L = kbo_amd.lib()
    L.kbo_set_slab_bytes(1 << 16)
    try:
        again = _find("k31", 5)
        many = refset.last_routes()[3]
    finally:
        L.kbo_set_slab_bytes(DEFAULT_SLAB)
    assert again == base == _expected("k31", 5) and many >= 8


@pytest.mark.parametrize("gap", [0, 5])
def test_k96_two_thresholds_and_a_contig_above_65536(gap):
    k, refs, seqs, rs, thr, aln = _world("k96")
    assert len(set(thr)) >= 2
    got, exp = _find("k96", gap), _expected("k96", gap)
    assert len(exp) >= 4 and {t[0] for t in exp} == {0, 1, 2}
    assert got == exp
    assert refset.last_routes() == (3, 0, 3 * len(seqs) * 2, 1)
