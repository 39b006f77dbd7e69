"""The sparse form of kbo::matches (kbo_hip.h kbo_aln_run): kbo_matches_batch_sparse through the slab pipeline and
kbo_sparse_runs_dev over device-resident character words, record for record against runs built in numpy from the oracle's
characters; the expansion against the oracle's characters and its relative_to_ref; the device entry point's buffers behind
guard bands."""
import ctypes

import numpy as np
import pytest

import kbo_amd
from kbo_amd import batch, synth

from gpu_helpers import RUN_CODE as CODE, Guarded, expected_runs

pytestmark = pytest.mark.gpu


def reads_with_junk(rng, g, lens, sub_rate=0.02):
    pieces = []
    for n in lens:
        a = int(rng.integers(0, len(g) - n))
        p = g[a:a + n].copy()
        hit = rng.random(n) < sub_rate
        p[hit] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, int(hit.sum()))]
        if rng.random() < 0.2:
            p[rng.integers(0, n, 2)] = rng.choice(list(b"Nnx$"))
        pieces.append(p)
    return np.concatenate(pieces), np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)


def check_host_sparse(oracle, sbwt, ora, name, concat, offsets, settings=((32 << 20, None), (1 << 16, None), (1 << 16, (0, 0)))):
    exp_chars = ora.matches_batch(concat, offsets, 1e-7, n_threads=4)
    exp_runs = expected_runs(exp_chars, offsets)
    exp_map = np.frombuffer(oracle.relative_to_ref(concat, exp_chars), dtype=np.uint8)
    words, pos, byt = batch.pack_reads(concat, offsets)
    L = kbo_amd.lib()
    for slab, devs in settings:
        try:
            L.kbo_set_slab_bytes(slab)
            if devs:
                kbo_amd.check(L.kbo_set_devices((ctypes.c_int * len(devs))(*devs), len(devs)))
            runs = batch.matches_batch_sparse(sbwt, words, offsets, pos, byt)
        finally:
            L.kbo_set_devices(None, 0)
            L.kbo_set_slab_bytes(16 << 20)
        assert len(runs) == len(exp_runs) and np.array_equal(runs, exp_runs), (name, slab, devs, len(runs), len(exp_runs))
        assert np.array_equal(batch.expand_sparse(runs, offsets), exp_chars), (name, slab, devs)
        assert np.array_equal(batch.expand_sparse(runs, offsets, ref=concat), exp_map), (name, slab, devs)
    return exp_runs


def test_sparse_matches_equal_the_oracle(oracle):
    """kbo_matches_batch_sparse against runs made from the oracle's characters: uniform 150 bp at 1 %, uniform 128 bp at 2 %, ragged
    3 - 700 bp with non-ACGT bytes in the side list, error-free reads (no record), reads of an unrelated genome (mostly one '-' run
    each), sequences of thousands of bases (the kernel for sequences of any length); whole slabs, slabs of 64 KiB (records of
    many slabs: seq is the batch's), and the device list (0, 0) (slabs completing out of order)"""
    g = synth.genome(300_000, seed=61)
    sbwt, _ = kbo_amd.build([g], kbo_amd.BuildOpts(k=31, num_threads=4))
    ora = oracle.Index.build([g.tobytes()], k=31)
    rng = np.random.default_rng(62)
    c, o = synth.reads(g, 30_000, 150, 0.01, seed=63)
    r = check_host_sparse(oracle, sbwt, ora, "uniform 150", c, o)
    assert len(r) > 10_000 and len(np.unique(r["seq"])) > 10_000
    c, o = synth.reads(g, 8_000, 128, 0.02, seed=64)
    check_host_sparse(oracle, sbwt, ora, "uniform 128", c, o)
    c, o = reads_with_junk(rng, g, rng.integers(3, 700, 6_000))
    r = check_host_sparse(oracle, sbwt, ora, "ragged with non-ACGT", c, o)
    assert {1, 2} <= set(int(x) for x in np.unique(r["code"])) <= {1, 2, 3}
    c, o = synth.reads(g, 4_000, 150, 0.0, seed=65)
    assert len(check_host_sparse(oracle, sbwt, ora, "error-free", c, o)) == 0
    c, o = synth.reads(synth.genome(300_000, seed=977), 3_000, 150, 0.0, seed=66)
    r = check_host_sparse(oracle, sbwt, ora, "unrelated genome", c, o)
    assert (r["code"] == 1).mean() > 0.9 and len(r) < 2 * 3_000
    c, o = reads_with_junk(rng, g, rng.integers(161, 6_000, 60), sub_rate=0.01)
    check_host_sparse(oracle, sbwt, ora, "longer than 160", c, o)


def test_sparse_matches_over_a_sharded_index(oracle):
    """a sharded index (kbo_set_index_shards) serves the sparse form: matches needs depths only"""
    g = synth.genome(240_000, seed=91)
    contigs = [g[i * 20_000:(i + 1) * 20_000].copy() for i in range(12)]
    seqs = [x.tobytes() for x in contigs]
    ora = oracle.Index.build(seqs, k=31)
    L = kbo_amd.lib()
    try:
        L.kbo_set_index_shards(3)
        sbwt, _ = kbo_amd.build(seqs, kbo_amd.BuildOpts(k=31, num_threads=4))
    finally:
        L.kbo_set_index_shards(0)
    assert sbwt.shards() >= 3
    rng = np.random.default_rng(92)
    c, o = reads_with_junk(rng, g, rng.choice([40, 150, 151, 300], 5_000), sub_rate=0.01)
    check_host_sparse(oracle, sbwt, ora, "sharded", c, o, settings=((32 << 20, None), (1 << 16, None)))


def test_sparse_runs_dev_after_the_packed_kernel(oracle):
    """kbo_matches_packed_dev, then kbo_sparse_runs_dev over its words (PackedDeviceBatch.sparse_runs): the records of the host
    entry point, for equally long and for ragged reads; and with too small a capacity the count is still the batch's"""
    import torch
    g = synth.genome(300_000, seed=71)
    sbwt, _ = kbo_amd.build([g], kbo_amd.BuildOpts(k=31, num_threads=4))
    ora = oracle.Index.build([g.tobytes()], k=31)
    rng = np.random.default_rng(72)
    cu, ou = synth.reads(g, 20_000, 150, 0.01, seed=73)
    cr, orr = reads_with_junk(rng, g, rng.integers(3, 161, 8_000))
    for name, concat, offsets in (("uniform 150", cu, ou), ("ragged", cr, orr)):
        exp = expected_runs(ora.matches_batch(concat, offsets, 1e-7, n_threads=4), offsets)
        dev = batch.PackedDeviceBatch(sbwt, concat, offsets, device=torch.device("cuda:0"))
        dev.run()
        assert np.array_equal(dev.sparse_runs(), exp), name
        assert np.array_equal(dev.sparse_runs(capacity=len(exp) // 3), exp), name  # (a second pass with the count it got)
        words, pos, byt = batch.pack_reads(concat, offsets)
        assert np.array_equal(batch.matches_batch_sparse(sbwt, words, offsets, pos, byt), exp), name


def pack_chars(chars, offsets, rng):
    """M - X R characters -> the packed layout, the padding of every sequence's last word random"""
    codes = CODE[np.asarray(chars, dtype=np.uint8)].astype(np.uint32)
    words = []
    for s in range(len(offsets) - 1):
        a, b = int(offsets[s]), int(offsets[s + 1])
        nw = (b - a + 15) // 16
        c = np.zeros(nw * 16, dtype=np.uint32)
        c[:b - a] = codes[a:b]
        c[b - a:] = rng.integers(0, 4, nw * 16 - (b - a))
        words.append((c.reshape(nw, 16) << (2 * np.arange(16, dtype=np.uint32))).sum(axis=1, dtype=np.uint64).astype(np.uint32))
    return np.concatenate(words)


def sparse_dev_guarded(words, offsets, max_len, capacity, seed):
    """kbo_sparse_runs_dev with every buffer at exactly its documented size behind guard bands -> (records, count)"""
    import torch
    dev = torch.device("cuda:0")
    L = kbo_amd.lib()
    n = len(offsets) - 1
    wb = int(L.kbo_sparse_runs_work_bytes(n, len(words)))
    assert wb > 0
    gw = Guarded("d_words", len(words) * 4, 4096, dev, seed=seed, data=words.view(np.uint8))
    go = Guarded("d_offsets", (n + 1) * 8, 4096, dev, seed=seed + 1, data=np.asarray(offsets, dtype=np.uint64).view(np.uint8))
    gk = Guarded("d_work", wb, 4096, dev, seed=seed + 2)
    gr = Guarded("d_runs", capacity * 12, 4096, dev, seed=seed + 3)
    gn = Guarded("d_n_runs", 4, 4096, dev, seed=seed + 4)
    s = torch.cuda.current_stream(dev)
    kbo_amd.check(L.kbo_sparse_runs_dev(gw.ptr, go.ptr, n, max_len, gk.ptr, gr.ptr if capacity else None, capacity, gn.ptr, s.cuda_stream))
    torch.cuda.synchronize()
    for g_ in (gw, go, gk, gr, gn):
        g_.assert_intact()
    assert np.array_equal(gw.host(), words.view(np.uint8)) and np.array_equal(go.host(), np.asarray(offsets, dtype=np.uint64).view(np.uint8))
    count = int(gn.host().view(np.uint32)[0])
    recs = gr.host().view(np.uint32).view(batch._ALN_RUN) if capacity else np.zeros(0, dtype=batch._ALN_RUN)
    return batch._sparse_from_raw(recs[:min(count, capacity)]), count


def test_sparse_runs_dev_buffer_contracts():
    """kbo_sparse_runs_dev over made-up characters - runs at a sequence's first and last base, runs across words and across the
    256-word chunks of a workgroup, sequences of 1 and 2 bases (no records), sequences that are one run - with random bits in
    the padding of every sequence's last word: buffers of exactly the documented size, guards intact; with max_seq_len
    unknown; and with too small a capacity the total is right and nothing past `capacity` records is written"""
    rng = np.random.default_rng(81)
    lens = np.concatenate([[1, 2, 3, 16, 17, 32, 5000, 4096], rng.integers(1, 400, 3000), [1, 2]])
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    chars = np.full(int(offsets[-1]), ord("M"), dtype=np.uint8)
    for _ in range(6000):
        p = int(rng.integers(0, len(chars)))
        chars[p:p + int(rng.choice([1, 2, 5, 15, 16, 17, 40]))] = rng.choice(list(b"-XR"))
    chars[int(offsets[6]):int(offsets[7])] = ord("-")            # a sequence that is one run of 5000
    chars[int(offsets[7]):int(offsets[7]) + 2000] = ord("X")      # two runs of 2000 / 2096 back to back
    chars[int(offsets[7]) + 2000:int(offsets[8])] = ord("-")
    for s in range(len(lens)):                                    # runs at first and last bases
        if s % 3 == 0:
            chars[int(offsets[s])] = ord("R")
        if s % 5 == 0:
            chars[int(offsets[s + 1]) - 1] = ord("X")
    exp = expected_runs(chars, offsets, min_len=3)
    words = pack_chars(chars, offsets, rng)
    assert len(words) > 4 * 256
    got, count = sparse_dev_guarded(words, offsets, int(lens.max()), len(exp), seed=1)
    assert count == len(exp) and np.array_equal(got, exp)
    got, count = sparse_dev_guarded(words, offsets, 0, len(exp) + 7, seed=2)
    assert count == len(exp) and np.array_equal(got, exp)
    got, count = sparse_dev_guarded(words, offsets, int(lens.max()), len(exp) // 2, seed=3)
    assert count == len(exp) and np.array_equal(got, exp[:len(exp) // 2])
    got, count = sparse_dev_guarded(words, offsets, int(lens.max()), 0, seed=4)
    assert count == len(exp)


def test_sparse_runs_dev_unknown_length_fills_the_device():
    """max_seq_len = 0 (unknown) must not cost more than a known length: the same workgroups as the largest batch (a length
    that overflowed the bound once ran the whole batch in ONE workgroup), the same records, and about the same time"""
    import torch
    L = kbo_amd.lib()
    dev = torch.device("cuda:0")
    n, wps = 1_000_000, 10  # 160-base sequences: 10 M words, no padding
    assert L.kbo_sparse_runs_blocks(n, 0) == L.kbo_sparse_runs_blocks(n, 160) == 2048
    rng = np.random.default_rng(83)
    words = np.where(rng.random(n * wps) < 0.02, rng.integers(1, 1 << 32, n * wps, dtype=np.uint64), 0).astype(np.uint32)
    offsets = np.arange(n + 1, dtype=np.uint64) * np.uint64(160)
    d_words = torch.from_numpy(words.view(np.int32)).to(dev)
    d_off = torch.from_numpy(offsets.view(np.int64)).to(dev)
    work = torch.zeros(int(L.kbo_sparse_runs_work_bytes(n, len(words))) // 8 + 2, dtype=torch.int64, device=dev)
    cap = 8 * n
    s = torch.cuda.current_stream(dev)
    out = {}
    for max_len in (160, 0):
        recs = torch.zeros(cap * 3, dtype=torch.int32, device=dev)
        cnt = torch.zeros(4, dtype=torch.int32, device=dev)
        best = 1e9
        for _ in range(4):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(s)
            kbo_amd.check(L.kbo_sparse_runs_dev(d_words.data_ptr(), d_off.data_ptr(), n, max_len, work.data_ptr(), recs.data_ptr(), cap,
                                                cnt.data_ptr(), s.cuda_stream))
            b.record(s)
            b.synchronize()
            best = min(best, a.elapsed_time(b))
        total = int(cnt[0].item())
        assert 0 < total <= cap
        out[max_len] = (best, total, recs[:total * 3].cpu().numpy())
    assert out[0][1] == out[160][1] and np.array_equal(out[0][2], out[160][2])
    assert out[0][0] < 3 * out[160][0] + 0.5, (out[0][0], out[160][0])
