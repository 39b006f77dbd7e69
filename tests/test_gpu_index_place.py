"""Placement (kbo_hip.h) on the GPU: kbo_place_dev byte for byte against the host form and the Python chain builder of
tests/test_index_place_host.py - on that file's hand-made lists (both routes are forced by list length) with d_place and d_work at
exactly their figures behind guard bands, with *d_n_segs above capacity, twice, and with records that hold anything; behind
kbo_ms_batch_dev and kbo_segments_dev on one stream for 300 reads and a 5 000-base sequence on both strands with merge, over an
index with add_revcomp and one without; kbo_amd.place equal to both; and what is refused."""
import numpy as np
import pytest

import kbo_amd
from kbo_amd import locate

from gpu_helpers import Guarded
from test_gpu_index_locate import _Batch, _dev, _located, _reads
from test_index_locate_host import src_offsets, world
from test_index_place_host import (K, LANE_MAX, MAX_GAP, MAX_INDEL, NONE, SRC_OFF, hand_batch, hand_made, py_place, same, strand_lists)

pytestmark = pytest.mark.gpu

E_BAD_ARG = -4
LONG = (9000, 2500, 64, 4)
SEG, REC = locate.SEGMENT_DTYPE.itemsize, locate.PLACE_DTYPE.itemsize

_hand_index = {}


def _hand_handle():
    """a handle whose sources have SRC_OFF's lengths (the second one empty): place only needs its source offsets and k"""
    if not _hand_index:
        rng = np.random.default_rng(77)
        lens = np.diff(SRC_OFF.astype(np.int64))
        srcs = [np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, int(n))] for n in lens]
        sbwt = kbo_amd.build(srcs, kbo_amd.BuildOpts(k=K, num_threads=4))[0]
        _hand_index["x"] = kbo_amd.add_positions(sbwt, srcs)
        assert np.array_equal(sbwt.source_offsets(), SRC_OFF)
    return _hand_index["x"]


class _Dev:
    """a segment list on the device with its count, and d_place / d_work of kbo_place_dev at exactly their figures"""

    def __init__(self, segs, n_seqs, capacity=None, count=None, seed=1, place_data=None):
        import torch
        self.dev = _dev()
        self.n_seqs = n_seqs
        self.capacity = len(segs) if capacity is None else capacity
        self.segs = Guarded("d_segs", SEG * self.capacity, 1 << 16, self.dev, seed=seed, data=segs[:self.capacity].view(np.uint8))
        cnt = np.array([len(segs) if count is None else count], dtype=np.uint64)
        self.cnt = Guarded("d_n_segs", 8, 4096, self.dev, seed=seed + 1, data=cnt.view(np.uint8))
        self.wb = locate.place_work_bytes(n_seqs, self.capacity)
        self.work = Guarded("d_work", self.wb, 1 << 16, self.dev, seed=seed + 2)
        self.place = Guarded("d_place", REC * n_seqs, 1 << 16, self.dev, seed=seed + 3, data=None if place_data is None else place_data.view(np.uint8))
        torch.cuda.synchronize()

    def run(self, sbwt, merge=False, stream=None, max_gap=MAX_GAP, max_indel=MAX_INDEL):
        import torch
        locate.place_dev(sbwt, self.segs.ptr if self.capacity else None, self.cnt.ptr, self.capacity, self.n_seqs, self.place.ptr, self.work.ptr, self.wb,
                         max_gap=max_gap, max_indel=max_indel, merge=merge, stream=stream)
        torch.cuda.synchronize()
        for g in (self.segs, self.cnt, self.work, self.place):
            g.assert_intact()
        assert not self.segs.changed() and not self.cnt.changed(), "the inputs are read only"
        return self.place.host().view(locate.PLACE_DTYPE).copy()


def test_hand_made_lists_equal_the_host_form_and_the_builder():
    import torch
    sbwt = _hand_handle()
    segs, names, want = hand_batch()
    counts = [len(v) for v in hand_made().values()]
    assert LANE_MAX in counts and LANE_MAX + 1 in counts and 0 in counts and 1 in counts and max(counts) > 64, "both routes, and neither"
    host = locate.place_from_segments_host(segs, len(names), SRC_OFF, K, MAX_GAP, MAX_INDEL)
    same(host, want)
    d = _Dev(segs, len(names))
    got = d.run(sbwt, stream=torch.cuda.Stream())
    same(got, want)
    # the same bytes twice, over what the first run left in d_work and d_place
    same(d.run(sbwt), want)
    # other limits: chains that break elsewhere
    for max_gap, max_indel in ((69, 100), (1000, 0), (0, 0)):
        same(_Dev(segs, len(names), seed=3).run(sbwt, max_gap=max_gap, max_indel=max_indel), py_place(segs, len(names), K, SRC_OFF, max_gap, max_indel))
    # more sequences than the list knows of, and no record at all
    same(_Dev(segs, len(names) + 300, seed=5).run(sbwt)[len(names):], py_place(segs[:0], 300, K, SRC_OFF))
    same(_Dev(segs[:0], 7, seed=7).run(sbwt), py_place(segs[:0], 7, K, SRC_OFF))


def test_a_count_above_capacity_uses_capacity_records():
    sbwt = _hand_handle()
    segs, names, _ = hand_batch()
    for cap in (len(segs) - 1, len(segs) // 2, 5, 1, 0):
        got = _Dev(segs, len(names), capacity=cap, count=len(segs) + 1000, seed=cap).run(sbwt)
        host = locate.place_from_segments_host(segs[:cap], len(names), SRC_OFF, K)
        same(got, host)
        same(got, py_place(segs[:cap], len(names), K, SRC_OFF))
    cut = segs[:len(segs) // 2]
    assert 0 < (np.flatnonzero(segs["seq"] == cut["seq"][-1]) >= len(cut)).sum(), "a list cut inside a sequence"


def test_merge_on_the_device_in_both_orders():
    sbwt = _hand_handle()
    a, b, names = strand_lists()
    n = len(names)
    want = py_place(b, n, K, SRC_OFF, merge_into=py_place(a, n, K, SRC_OFF))
    pa, pb = _Dev(a, n, seed=1).run(sbwt), _Dev(b, n, seed=2).run(sbwt)
    same(_Dev(b, n, seed=3, place_data=pa).run(sbwt, merge=True), want)
    same(_Dev(a, n, seed=4, place_data=pb).run(sbwt, merge=True), want)
    same(locate.place_from_segments_host(b, n, SRC_OFF, K, merge_into=pa), want)
    assert want["strand"].tolist()[:4] == [2, 1, 1, 1] and want["source"][4] == NONE
    # merge == 0 writes over what is there
    same(_Dev(a, n, seed=5, place_data=pb).run(sbwt, merge=False), pa)


def test_records_that_hold_anything_leave_the_guard_bands_intact():
    sbwt = _hand_handle()
    segs, names, want = hand_batch()
    rng = np.random.default_rng(31)
    for trial in range(4):
        wild = segs.copy()
        hit = rng.choice(len(wild), 90, replace=False)
        wild["seq"][hit[:30]] = [0xFFFFFFFF, len(names), len(names) + 1] * 10
        wild["seq"][hit[30:60]] = rng.integers(0, len(names), 30)
        for f in ("q_first", "q_last", "pos_first", "pos_last", "flags"):
            wild[f][hit[60:]] = rng.integers(0, 1 << 32, 30, dtype=np.uint64).astype(np.uint32)
        if trial == 3:
            wild = wild[rng.permutation(len(wild))]  # (no order at all)
        got = _Dev(wild, len(names), seed=trial).run(sbwt, merge=bool(trial & 1))  # (run() checks every guard band)
        if not trial & 1:
            same(got, locate.place_from_segments_host(wild, len(names), SRC_OFF, K))  # the ranges are minima and maxima: one result


def _pipeline(sbwt, seqs, k, bridge, n_bases, cap):
    """kbo_ms_batch_dev -> kbo_segments_dev -> kbo_place_dev for '+' then '-' with merge, all on ONE stream, one wait at the end;
    -> (records, [segments of '+', segments of '-'])"""
    import torch
    b = _Batch(sbwt, seqs, n_bases + 1, seed=k)
    dev = b.dev
    segs = [Guarded("d_segs", SEG * cap, 1 << 16, dev, seed=10 + st) for st in range(2)]
    cnts = [Guarded("d_n_segs", 8, 4096, dev, seed=20 + st) for st in range(2)]
    sworks = [Guarded("d_work", b.sb, 1 << 16, dev, seed=30 + st) for st in range(2)]
    wb = locate.place_work_bytes(b.n, cap)
    pwork = Guarded("d_work", wb, 1 << 16, dev, seed=40)
    place = Guarded("d_place", REC * b.n, 1 << 16, dev, seed=41)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    for st in range(2):
        b.walk(st + 1, stream)
        locate.segments_dev(sbwt, b.ms, b.lo, b.d_off, b.n, b.total, segs[st].ptr, cap, cnts[st].ptr, sworks[st].ptr, b.sb, bridge=bridge, strand=st + 1,
                            stream=stream)
        locate.place_dev(sbwt, segs[st].ptr, cnts[st].ptr, cap, b.n, place.ptr, pwork.ptr, wb, merge=st == 1, stream=stream)
    torch.cuda.synchronize()
    for g in segs + cnts + sworks + [pwork, place]:
        g.assert_intact()
    lists = []
    for st in range(2):
        n = int(cnts[st].host().view(np.uint64)[0])
        assert n <= cap
        lists.append(segs[st].host().view(locate.SEGMENT_DTYPE)[:n].copy())
    return place.host().view(locate.PLACE_DTYPE).copy(), lists


@pytest.mark.parametrize("k,rc", [(31, False), (31, True), (96, False)])
def test_walk_segments_and_place_on_one_stream_for_both_strands(k, rc):
    srcs = world(k, rc, LONG)[0]
    sbwt = _located(k, rc, LONG)
    soff = src_offsets(srcs)
    seqs = _reads(srcs, k, np.random.default_rng(100 + k))
    n = len(seqs)
    for bridge in (0, k):
        got, (fwd, rev) = _pipeline(sbwt, seqs, k, bridge, int(soff[-1]), 6000)
        host = locate.place_from_segments_host(rev, n, soff, k, merge_into=locate.place_from_segments_host(fwd, n, soff, k))
        same(got, host)
        same(got, py_place(rev, n, k, soff, merge_into=py_place(fwd, n, k, soff)))
        same(kbo_amd.place(seqs, sbwt, bridge=bridge, strands=3), got)
        same(kbo_amd.place(seqs, sbwt, bridge=bridge, strands=1), py_place(fwd, n, k, soff))
        same(kbo_amd.place(seqs, sbwt, bridge=bridge, strands=2), py_place(rev, n, k, soff))
        # what the batch is there for
        reads, long_seq = got[:300], got[300]
        if k == 31 and rc:  # both strands of the sources are indexed: either walk finds every read, and the other strand's chain is the runner-up
            assert (reads["source"] == 0).all() and (reads["q_end"] - reads["q_start"] >= k).all() and (reads["second"] > 0).all()
            assert (reads["flags"][1::2] & 1).all() and not (reads["flags"][0::2] & 1).any()
        elif k == 31:
            assert (reads["source"] == 0).all() and (reads["q_end"] - reads["q_start"] >= k).all()
            assert (reads["strand"][0::2] == 1).all() and (reads["strand"][1::2] == 2).all() and not (reads["flags"] & 1).any()
        else:  # (a read of 100 .. 150 bases with a substitution near its middle has no window of 96 bases: no segment)
            assert (reads["source"] == NONE).any() and (reads["source"] == 0).any()
        if bridge == 0:
            per_seq = np.bincount(fwd["seq"], minlength=n)
            assert per_seq[300] > LANE_MAX and (per_seq[:300] <= LANE_MAX).all(), "the long sequence takes the wave route, the reads the lane route"
            assert k != 31 or (per_seq[:300] >= 2).sum() > 50, "reads with a substitution: lists of two and more for the lane route"
            assert long_seq["n_segs"] == per_seq[300] and long_seq["indel"] == 0
        assert long_seq["source"] == 0 and long_seq["strand"] == 1 and 1000 <= long_seq["pos_start"] < 1100 and 5900 < long_seq["pos_end"] <= 6000
        assert got[301]["source"] == NONE, "a sequence of k - 1 bases has no segment"


def test_what_is_refused_on_the_device():
    import torch
    sbwt = _hand_handle()
    segs, names, _ = hand_batch()
    d = _Dev(segs, len(names))
    with pytest.raises(kbo_amd.KboError) as e:
        locate.place_dev(sbwt, d.segs.ptr, d.cnt.ptr, d.capacity, d.n_seqs, d.place.ptr, d.work.ptr, d.wb - 1)
    assert e.value.code == E_BAD_ARG and "work_bytes" in e.value.message
    plain = kbo_amd.build([np.frombuffer(b"ACGTTGCATGCATGCAAGTCGATCGATTTGACCATG" * 3, dtype=np.uint8)], kbo_amd.BuildOpts(k=7))[0]
    with pytest.raises(kbo_amd.KboError) as e:
        locate.place_dev(plain, d.segs.ptr, d.cnt.ptr, d.capacity, d.n_seqs, d.place.ptr, d.work.ptr, d.wb)
    assert e.value.code == E_BAD_ARG and "no positions" in e.value.message
    with pytest.raises(kbo_amd.KboError) as e:
        kbo_amd.place([b"ACGTTGCATGCATGCAAGTCGATCG"], plain)
    assert e.value.code == E_BAD_ARG
    torch.cuda.synchronize()
    for g in (d.segs, d.cnt, d.work, d.place):
        assert not g.changed(), "a refused call enqueues nothing"
