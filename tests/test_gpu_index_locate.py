"""Positions, segments, depth (kbo_hip.h) on the GPU against brute force.

The yardstick is tests/test_index_locate_host.py's: a dict from every k-mer of every indexed stretch of the sources to its occurrences,
the expected entry of every row from it, and a chain builder over the dict - nothing from the library's walk.  All comparisons are
exact and cover every row, record, delta and depth word.  The small world is that file's (which its own tests check on the CPU first);
the batches here need longer sources, made by the same function: the same planted repeat, inverted repeat, N and lower-case base."""
import ctypes as C

import numpy as np
import pytest

import kbo_amd
from kbo_amd import locate

from gpu_helpers import Guarded
from test_index_locate_host import (_other, as_tuples, brute_delta, brute_depth, brute_segments, queries, revcomp, src_offsets,
                                    walk, world)

pytestmark = pytest.mark.gpu

E_BAD_ARG, E_UNSUPPORTED = -4, -8
CASES = [(31, False), (31, True), (96, False), (96, True)]
LONG = (9000, 2500, 64, 4)
REC = locate.SEGMENT_DTYPE.itemsize


def _dev():
    import torch
    return torch.device("cuda", torch.cuda.current_device())


def _geometry():
    tile, halo, chunk = C.c_uint32(), C.c_uint32(), C.c_uint32()
    kbo_amd.check(kbo_amd.lib().kbo_segments_geometry(C.byref(tile), C.byref(halo), C.byref(chunk)))
    return tile.value, halo.value


def _build(srcs, k, rc, how):
    opts = kbo_amd.BuildOpts(k=k, add_revcomp=rc, num_threads=4)
    if how == "host":
        return kbo_amd.build(srcs, opts)[0]
    if how == "device":
        return kbo_amd.build(srcs, opts, device=-1)[0]
    built = kbo_amd.build(srcs, opts)[0]
    rows, Carr, lcs = built.export_parts()
    return kbo_amd.SbwtIndexVariant.from_parts(k, built.n_sets(), built.n_kmers(), rows, Carr, lcs)


_handles = {}


def _located(k, rc, lens):
    """a handle over the world's sources with its position table, once per world"""
    key = (k, rc, lens)
    if key not in _handles:
        srcs = world(k, rc, lens)[0]
        _handles[key] = kbo_amd.add_positions(_build(srcs, k, rc, "host"), srcs, add_revcomp=rc)
    return _handles[key]


# ---- the table
@pytest.mark.parametrize("how", ["host", "device", "parts"])
@pytest.mark.parametrize("k,rc", CASES)
def test_add_positions_gives_the_brute_force_table(k, rc, how):
    srcs, oi, occ, want = world(k, rc)
    sbwt = _build(srcs, k, rc, how)
    assert sbwt.n_sets() == oi.n_sets and not sbwt.has_positions()
    L = kbo_amd.lib()
    for slab in (0, 97, 256):  # (one slab; slabs shorter than a source, than k + 1, and than the repeat)
        L.kbo_set_positions_slab_bases(slab)
        try:
            kbo_amd.add_positions(sbwt, srcs, add_revcomp=rc)
        finally:
            L.kbo_set_positions_slab_bases(0)
        got = sbwt.positions()
        assert np.array_equal(got, want), (slab, np.flatnonzero(got != want)[:10])
    assert sbwt.has_positions() and np.array_equal(sbwt.source_offsets(), src_offsets(srcs))
    assert L.kbo_index_source_bases(sbwt._h) == sum(len(s) for s in srcs)
    assert L.kbo_index_positions_bytes(sbwt._h) == 4 * oi.n_sets + 8 * (len(srcs) + 1)
    kbo_amd.check(L.kbo_index_positions_to_device(sbwt._h, -1))
    kbo_amd.check(L.kbo_index_positions_to_device(sbwt._h, -1))


@pytest.mark.parametrize("k,rc", [(31, False), (31, True)])
def test_wrong_sequences_are_refused_and_leave_no_table(k, rc):
    srcs, _, _, want = world(k, rc)
    sbwt = kbo_amd.add_positions(_build(srcs, k, rc, "host"), srcs, add_revcomp=rc)
    assert sbwt.has_positions()
    other = [s.copy() for s in srcs]
    other[0][333] = _other(other[0][333])
    for seqs, flag in ((other, rc), (srcs, not rc), (srcs[:1], rc)):
        kbo_amd.add_positions(sbwt, srcs, add_revcomp=rc)
        with pytest.raises(kbo_amd.KboError) as e:
            kbo_amd.add_positions(sbwt, seqs, add_revcomp=flag)
        assert e.value.code == E_BAD_ARG and not sbwt.has_positions()
    kbo_amd.add_positions(sbwt, srcs, add_revcomp=rc)
    assert np.array_equal(sbwt.positions(), want)


# ---- segments
def _reads(srcs, k, rng):
    """what the issue lists: 300 reads with 1 % substitutions (every other one from the reverse strand), 5 000 bases with a substitution
    every 97, and sequences of tile + halo bases and one more and one fewer; and a sequence of k - 1 bases"""
    s0 = srcs[0]
    tile, halo = _geometry()
    out = []
    for r in range(300):
        n = int(rng.integers(100, 151))
        at = int(rng.integers(0, len(s0) - n))
        q = s0[at:at + n].copy()
        for i in np.flatnonzero(rng.random(n) < 0.01):
            q[i] = _other(q[i])
        out.append(revcomp(q) if r % 2 else q)
    long = s0[1000:6000].copy()
    for i in range(50, 5000, 97):
        long[i] = _other(long[i])
    out.append(long)
    out.append(s0[300:300 + k - 1].copy())
    for n in (tile + halo, tile + halo + 1, tile + halo - 1):
        out.append(s0[500:500 + n].copy())
    return out


class _Batch:
    """a batch on the device, walked with intervals, and the Guarded buffers of kbo_segments_dev at exactly their figures"""

    def __init__(self, sbwt, seqs, n_delta, seed):
        import torch
        self.sbwt, self.seqs, self.dev = sbwt, seqs, _dev()
        self.off = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.uint64)
        self.n, self.total = len(seqs), int(self.off[-1])
        q = np.zeros(self.total + 16, dtype=np.uint8)
        q[:self.total] = np.concatenate(seqs)
        self.q = torch.from_numpy(q).to(self.dev)
        self.qr = torch.zeros_like(self.q)
        self.d_off = torch.from_numpy(self.off.astype(np.int64)).to(self.dev)
        self.ms = torch.zeros(self.total + 16, dtype=torch.uint8, device=self.dev)
        self.lo = torch.zeros(self.total, dtype=torch.int32, device=self.dev)
        self.hi = torch.zeros(self.total, dtype=torch.int32, device=self.dev)
        L = kbo_amd.lib()
        self.wb = int(L.kbo_ms_work_bytes(self.n, self.total, 0, sbwt.k()))
        self.work = torch.zeros(self.wb // 8 + 2, dtype=torch.int64, device=self.dev)
        self.sb = locate.segments_work_bytes(self.n, self.total)
        self.swork = Guarded("d_work", self.sb, 1 << 16, self.dev, seed=seed)
        self.cnt = Guarded("d_n_segs", 8, 4096, self.dev, seed=seed + 1)
        self.delta = Guarded("d_delta", 4 * n_delta, 1 << 16, self.dev, seed=seed + 2, data=np.zeros(4 * n_delta, dtype=np.uint8))

    def walk(self, strand, stream):
        L = kbo_amd.lib()
        src = self.q
        if strand == 2:
            kbo_amd.check(L.kbo_revcomp_batch_dev(self.q.data_ptr(), self.d_off.data_ptr(), self.n, self.total, 0, self.qr.data_ptr(), stream.cuda_stream))
            src = self.qr
        kbo_amd.check(L.kbo_ms_batch_dev(self.sbwt._h, src.data_ptr(), self.d_off.data_ptr(), self.n, self.total, 0, self.ms.data_ptr(), self.lo.data_ptr(),
                                         self.hi.data_ptr(), self.work.data_ptr(), self.wb, stream.cuda_stream))

    def segments(self, strand, bridge, capacity, stream, delta=True, seed=5):
        """walk + kbo_segments_dev on one stream; -> (records written, count)"""
        import torch
        segs = Guarded("d_segs", REC * capacity, 1 << 16, self.dev, seed=seed)
        self.swork.fill(seed + 1)
        self.cnt.fill(seed + 2)
        torch.cuda.synchronize()  # (the fills ran on the default stream)
        self.walk(strand, stream)
        locate.segments_dev(self.sbwt, self.ms, self.lo, self.d_off, self.n, self.total, segs.ptr if capacity else None, capacity, self.cnt.ptr,
                            self.swork.ptr, self.sb, bridge=bridge, strand=strand, delta=self.delta.ptr if delta else None, stream=stream)
        torch.cuda.synchronize()
        for g in (segs, self.swork, self.cnt, self.delta):
            g.assert_intact("strand %d bridge %d capacity %d" % (strand, bridge, capacity))
        n = int(self.cnt.host().view(np.uint64)[0])
        return segs.host().view(locate.SEGMENT_DTYPE)[:min(n, capacity)].copy(), n

    def strand_seqs(self, strand):
        return [revcomp(s) for s in self.seqs] if strand == 2 else self.seqs

    def host_form(self, oi, table, strand, bridge, capacity, n_bases, delta):
        d, lo, off = walk(oi, self.strand_seqs(strand))
        return locate.segments_from_ms_host(table, self.sbwt.k(), d, lo, off, bridge, strand, capacity, n_bases, delta)


@pytest.mark.parametrize("k,rc", CASES)
def test_segments_behind_the_walk_equal_the_host_form_and_brute_force(k, rc):
    import torch
    srcs, oi, occ, table = world(k, rc, LONG)
    sbwt = _located(k, rc, LONG)
    assert np.array_equal(sbwt.positions(), table)
    n_bases = int(src_offsets(srcs)[-1])
    seqs = _reads(srcs, k, np.random.default_rng(100 + k))
    b = _Batch(sbwt, seqs, n_bases + 1, seed=k)
    stream = torch.cuda.Stream()
    want_delta = np.zeros(n_bases + 1, dtype=np.uint32)
    for strand, bridge in ((1, k), (2, k), (1, 0), (1, 255), (2, 1)):
        want = brute_segments(b.strand_seqs(strand), occ, k, bridge, strand)
        assert len(want) > 50
        host_delta = want_delta.copy()
        host, hn = b.host_form(oi, table, strand, bridge, len(want) + 7, n_bases, host_delta)
        assert hn == len(want) and as_tuples(host) == want
        want_delta += brute_delta(want, k, n_bases)
        assert np.array_equal(host_delta, want_delta)
        got, n = b.segments(strand, bridge, len(want) + 7, stream)
        assert n == len(want) and np.array_equal(got, host), (strand, bridge, np.flatnonzero(got != host)[:5])
        assert np.array_equal(b.delta.host().view(np.uint32), want_delta)
        # the same bytes twice, without delta; then a capacity below the count, and none at all
        again, n2 = b.segments(strand, bridge, len(want) + 7, stream, delta=False, seed=9)
        assert n2 == n and np.array_equal(again, got)
        few, n3 = b.segments(strand, bridge, len(want) // 2, stream, delta=False, seed=11)
        assert n3 == n and np.array_equal(few, got[:len(want) // 2])
        none, n4 = b.segments(strand, bridge, 0, stream, delta=False, seed=13)
        assert n4 == n and len(none) == 0
        assert np.array_equal(b.delta.host().view(np.uint32), want_delta)
    # the long sequence: a boundary every 97 bases at bridge 0, one segment at bridge k
    long_seq = 300
    assert sum(r[0] == long_seq for r in brute_segments(seqs, occ, k, 0, 1)) >= 5000 // 97 - 2
    # a short d_work, and a handle whose table is not on this device
    with pytest.raises(kbo_amd.KboError) as e:
        locate.segments_dev(sbwt, b.ms, b.lo, b.d_off, b.n, b.total, None, 0, b.cnt.ptr, b.swork.ptr, b.sb - 1, stream=stream)
    assert e.value.code == E_BAD_ARG


def test_segments_of_arrays_with_empty_sequences():
    """kbo_segments_dev over the host test's queries - an empty sequence and one of k - 1 bases among them - with the oracle's walk
    uploaded: the kernels' own handling of the offsets, whatever kbo_ms_batch_dev does with such a batch"""
    import torch
    k, rc = 31, True
    srcs, oi, occ, table = world(k, rc)
    sbwt = _located(k, rc, tuple(len(s) for s in srcs))
    n_bases = int(src_offsets(srcs)[-1])
    seqs = list(queries(srcs, k).values())
    seqs = [seqs[-2]] + seqs + [seqs[-2]]  # (the empty one first and last as well)
    d, lo, off = walk(oi, seqs)
    dev, total = _dev(), int(off[-1])
    t_d = torch.from_numpy(np.concatenate([d, np.zeros(16, dtype=np.uint8)])).to(dev)
    t_lo = torch.from_numpy(lo.astype(np.int32)).to(dev)
    t_off = torch.from_numpy(off.astype(np.int64)).to(dev)
    sb = locate.segments_work_bytes(len(seqs), total)
    for bridge in (0, k, 255):
        want = brute_segments(seqs, occ, k, bridge, 1)
        work, cnt = Guarded("d_work", sb, 1 << 16, dev, seed=bridge), Guarded("d_n_segs", 8, 4096, dev, seed=1)
        segs = Guarded("d_segs", REC * len(want), 1 << 16, dev, seed=2)
        delta = Guarded("d_delta", 4 * (n_bases + 1), 1 << 16, dev, seed=3, data=np.zeros(4 * (n_bases + 1), dtype=np.uint8))
        torch.cuda.synchronize()
        locate.segments_dev(sbwt, t_d, t_lo, t_off, len(seqs), total, segs.ptr, len(want), cnt.ptr, work.ptr, sb, bridge=bridge, delta=delta.ptr)
        torch.cuda.synchronize()
        for g in (work, cnt, segs, delta):
            g.assert_intact("bridge %d" % bridge)
        assert int(cnt.host().view(np.uint64)[0]) == len(want)
        assert as_tuples(segs.host().view(locate.SEGMENT_DTYPE)) == want
        assert np.array_equal(delta.host().view(np.uint32), brute_delta(want, k, n_bases))


# ---- depth
@pytest.mark.parametrize("k,rc", [(31, True), (96, False)])
def test_depth_of_two_batches_and_a_reverse_strand(k, rc):
    import torch
    srcs, oi, occ, table = world(k, rc, LONG)
    sbwt = _located(k, rc, LONG)
    n_bases = int(src_offsets(srcs)[-1])
    rng = np.random.default_rng(7 + k)
    first, second = _reads(srcs, k, rng), _reads(srcs, k, rng)[:120]
    stream = torch.cuda.Stream()
    dev = _dev()
    delta = Guarded("d_delta", 4 * (n_bases + 1), 1 << 16, dev, seed=1, data=np.zeros(4 * (n_bases + 1), dtype=np.uint8))
    depth = Guarded("d_depth", 4 * n_bases, 1 << 16, dev, seed=2)
    wb = locate.depth_work_bytes(sbwt)
    assert wb == (4 * ((n_bases + 2047) // 2048) + 15) // 16 * 16
    dwork = Guarded("d_work", wb, 1 << 16, dev, seed=3)
    want = np.zeros(n_bases, dtype=np.uint32)
    for seqs, strand in ((first, 1), (second, 1), (second, 2)):
        b = _Batch(sbwt, seqs, n_bases + 1, seed=strand)
        b.delta = delta
        recs = brute_segments(b.strand_seqs(strand), occ, k, k, strand)
        want += brute_depth(recs, k, n_bases)
        _, n = b.segments(strand, k, 0, stream)
        assert n == len(recs)
    torch.cuda.synchronize()
    locate.depth_finish_dev(sbwt, delta.ptr, depth.ptr, dwork.ptr, wb, stream=stream)
    torch.cuda.synchronize()
    for g in (delta, depth, dwork):
        g.assert_intact()
    assert want.max() > 3 and np.array_equal(depth.host().view(np.uint32), want)
    with pytest.raises(kbo_amd.KboError) as e:
        locate.depth_finish_dev(sbwt, delta.ptr, depth.ptr, dwork.ptr, wb - 1, stream=stream)
    assert e.value.code == E_BAD_ARG


# ---- the host form
@pytest.mark.parametrize("k,rc", [(31, True), (96, True)])
def test_host_form_equals_the_device_composition_and_brute_force(k, rc):
    srcs, oi, occ, table = world(k, rc, LONG)
    sbwt = _located(k, rc, LONG)
    n_bases = int(src_offsets(srcs)[-1])
    seqs = _reads(srcs, k, np.random.default_rng(3 + k))
    fwd = brute_segments(seqs, occ, k, k, 1)
    rev = brute_segments([revcomp(s) for s in seqs], occ, k, k, 2)
    want = sorted(fwd + rev, key=lambda r: (r[0], r[1], r[2]))
    recs, depth = kbo_amd.segments(seqs, sbwt, strands=3, depth=True)
    assert as_tuples(recs) == want
    assert np.array_equal(depth, brute_depth(fwd + rev, k, n_bases))
    assert as_tuples(kbo_amd.segments(seqs, sbwt, bridge=0, strands=2)) == brute_segments([revcomp(s) for s in seqs], occ, k, 0, 2)
    src, at, orient = kbo_amd.segment_source(recs, sbwt.source_offsets())
    # (a reverse-strand read over the inverted repeat lies FORWARD on the second source: FWD before REV)
    assert set(src.tolist()) <= {0, 1} and (src == 0).sum() > 0.9 * len(src) and orient.any() and not orient.all()
    assert (at < np.array([len(s) for s in srcs])[src]).all()
    # a handle without positions, a sharded handle, bridge 256
    plain = _build(srcs, k, rc, "host")
    for f in (lambda: kbo_amd.segments(seqs, plain), lambda: kbo_amd.segments(seqs, sbwt, bridge=256)):
        with pytest.raises(kbo_amd.KboError) as e:
            f()
        assert e.value.code == E_BAD_ARG
    L = kbo_amd.lib()
    L.kbo_set_index_shards(2)
    try:
        sharded = _build(srcs, k, rc, "host")
    finally:
        L.kbo_set_index_shards(0)
    assert sharded.shards() >= 2
    with pytest.raises(kbo_amd.KboError) as e:
        kbo_amd.segments(seqs, sharded)
    assert e.value.code == E_UNSUPPORTED
    with pytest.raises(kbo_amd.KboError) as e:
        kbo_amd.add_positions(sharded, srcs, add_revcomp=rc)
    assert e.value.code == E_UNSUPPORTED
