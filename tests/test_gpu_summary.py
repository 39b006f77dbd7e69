"""Per-sequence alignment summaries on the device (kbo_hip.h kbo_aln_summary): every sequence's record against batch.summary_of_chars of
(a) the oracle's characters and (b) kbo_matches_batch's / kbo_map_batch_dev's characters for the same batch - through map_reads_kernel's
summary form (both threshold cases) and finish_reads_kernel's (its three list shapes, workgroups of one and of four waves), through the
reducer (summary_kernels.hip) for everything else, at exactly the documented buffer sizes, through the pipelines and through the host
slab pipeline."""
import ctypes as C

import numpy as np
import pytest

import kbo_amd
from kbo_amd import batch, derandomize, synth
from gpu_helpers import Guarded, threads, scratch_guard_bytes, round16

pytestmark = pytest.mark.gpu

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
GENOME = 30_000


def _batch_of(reads):
    concat = np.concatenate(reads)
    offsets = np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.uint64)
    return concat, offsets


_INDEX = {}


def _index(oracle, k):
    """a random genome of 30 kbp (its depth table: about 11 bases), the product's index and the oracle's - made once per k"""
    if k not in _INDEX:
        g = synth.genome(GENOME, seed=4000 + k)
        sbwt, _ = kbo_amd.build([g], kbo_amd.BuildOpts(k=k, num_threads=threads()))
        sbwt.to_device(-1)
        _INDEX[k] = (g, sbwt, oracle.Index.build([g.tobytes()], k=k))
    return _INDEX[k]


def _oracle_summary(ora, concat, offsets, p):
    """summary_of_chars of the oracle's characters; the oracle (like the reference) takes only sequences of 3 bases or more"""
    lens = np.diff(offsets.astype(np.int64))
    keep = np.flatnonzero(lens >= 3)
    sub = [concat[int(offsets[s]):int(offsets[s + 1])] for s in keep]
    out = np.zeros((len(lens), 4), dtype=np.uint32)
    if len(sub):
        c2, o2 = _batch_of(sub)
        out[keep] = batch.summary_of_chars(ora.matches_batch(c2, o2, p, n_threads=threads()), o2)
    return out


def _device_chars_summary(sbwt, concat, offsets, p):
    """summary_of_chars of the characters kbo_map_batch_dev (format 0) leaves for the same batch"""
    import torch
    dev = batch.DeviceBatch(sbwt, concat, offsets, device=torch.device("cuda:0"), max_error_prob=p, format=False, want_ms=False)
    kbo_amd.lib().kbo_set_plan(1, 0, 0)
    dev.run()
    torch.cuda.synchronize()
    return batch.summary_of_chars(dev.chars[:dev.total].cpu().numpy(), offsets)


def _assert_records(got, want, offsets, what):
    if not np.array_equal(got, want):
        bad = np.flatnonzero((got != want).any(axis=1))
        s = int(bad[0])
        raise AssertionError("%s: %d of %d records differ; first: sequence %d (len %d) got %s want %s" % (
            what, len(bad), len(want), s, int(offsets[s + 1] - offsets[s]), got[s].tolist(), want[s].tolist()))


def _flags(dev):
    """which reads the one kernel left to the second pass, off the summary batch's own work memory"""
    import torch
    out = np.zeros(dev.n_seqs, dtype=np.uint8)
    s = torch.cuda.current_stream(dev.device)
    kbo_amd.check(kbo_amd.lib().kbo_plan_flags_dev(dev.n_seqs, dev.total, dev.max_len, dev.k, dev.summary_work.data_ptr(), out.ctypes.data, s.cuda_stream))
    return out


def _ragged_reads(rng, g):
    """about 200 reads, lengths 1 .. 160: error-free to 8 % substitutions, indels, chimeras, the other strand, unrelated, N and lower case,
    more than 13 mismatches"""
    comp = np.zeros(256, dtype=np.uint8)
    comp[list(b"ACGT")] = list(b"TGCA")
    other = synth.genome(5_000, seed=77)
    reads = []
    for length in range(1, 161):
        a = int(rng.integers(0, len(g) - 200))
        r = g[a:a + length].copy()
        rate = (length % 9) / 100.0  # 0 % .. 8 %
        hit = rng.random(length) < rate
        r[hit] = ACGT[rng.integers(0, 4, int(hit.sum()))]
        reads.append(r)

    def take(length):
        a = int(rng.integers(0, len(g) - 200))
        return g[a:a + length].copy()
    for _ in range(6):  # one and two indels
        r = take(150)
        p_ = int(rng.integers(20, 130))
        reads.append(np.concatenate([r[:p_], r[p_ + 2:]]))
        reads.append(np.concatenate([r[:p_], ACGT[rng.integers(0, 4, 2)], r[p_:]]))
        q = int(rng.integers(20, 60))
        reads.append(np.concatenate([r[:q], r[q + 1:100], ACGT[rng.integers(0, 4, 1)], r[100:]]))
    for _ in range(5):
        c = int(rng.integers(30, 120))
        reads.append(np.concatenate([take(150)[:c], take(150)[c:]]))          # chimeras
        reads.append(comp[take(150)][::-1].copy())                            # the other strand
        reads.append(other[(b := int(rng.integers(0, len(other) - 150))):b + 150].copy())  # unrelated
    for i in range(8):  # N and lower case: always the second pass's
        r = take(100 + 7 * i)
        r[int(rng.integers(0, len(r)))] = ord("N") if i % 2 == 0 else (r[5] | 0x20)
        reads.append(r)
    for _ in range(4):  # more than 13 mismatches
        r = take(160)
        pos = rng.choice(160, 20, replace=False)
        r[pos] = comp[r[pos]]
        reads.append(r)
    return reads


def _thresholds(sbwt):
    """(p with the threshold at or above the depth table's order, p with it below)"""
    order = sbwt.depth_table_order()
    thr = lambda p: derandomize.random_match_threshold(sbwt.k(), sbwt.n_kmers(), 4, p)  # noqa: E731
    cands = [1e-7, 1e-5, 1e-3, 1e-2, 0.05, 0.1, 0.2, 0.3, 0.5, 0.7, 0.9]
    above = [p for p in cands if thr(p) >= order]
    below = [p for p in cands if 1 < thr(p) < order]
    assert above and below, (order, [thr(p) for p in cands])
    return above[0], below[0]


@pytest.mark.parametrize("k", [11, 31, 63])
def test_one_kernel_ragged_reads_both_threshold_cases(oracle, k):
    import torch
    g, sbwt, ora = _index(oracle, k)
    assert sbwt.depth_table_order() > 0
    reads = _ragged_reads(np.random.default_rng(10 + k), g)
    assert 190 <= len(reads) <= 256 and len(reads) % 64 != 0  # three or four waves, the last partly filled
    concat, offsets = _batch_of(reads)
    for p in _thresholds(sbwt):
        dev = batch.DeviceBatch(sbwt, concat, offsets, device=torch.device("cuda:0"), max_error_prob=p, format=False, want_ms=False)
        dev._summary_buffers()
        dev.summary.fill_(-1)
        dev.ms.fill_(0xEE)
        dev.run_summary()
        torch.cuda.synchronize()
        assert dev.fused
        assert bool((dev.ms == 0xEE).all()), "the one-kernel route stores no MS value"
        fl = _flags(dev) != 0
        assert fl.any() and not fl.all(), "the first kernel finished a read and the second pass received one"
        got = dev.summary_host()
        _assert_records(got, _oracle_summary(ora, concat, offsets, p), offsets, "k %d p %g vs the oracle" % (k, p))
        _assert_records(got, _device_chars_summary(sbwt, concat, offsets, p), offsets, "k %d p %g vs kbo_map_batch_dev's characters" % (k, p))
        assert (got[np.diff(offsets.astype(np.int64)) < 3] == 0).all()


@pytest.mark.parametrize("n_flagged", [700, 3000, 5000])
def test_second_pass_list_shapes(oracle, n_flagged):
    """finish_reads_kernel's summary form: one, four and sixteen reads a wave (up to 1 024 / up to 4 096 / more flagged reads), in
    workgroups of four waves (kbo_summary_batch_dev) and of one (the pipelines' urgent second pass)"""
    import torch
    g, sbwt, ora = _index(oracle, 31)
    rng = np.random.default_rng(n_flagged)
    reads = []
    for i in range(n_flagged):  # short reads that each hold an N
        length = int(rng.integers(20, 41))
        a = int(rng.integers(0, len(g) - 50))
        r = g[a:a + length].copy()
        r[int(rng.integers(0, length))] = ord("N")
        reads.append(r)
    for i in range(100):
        a = int(rng.integers(0, len(g) - 50))
        reads.append(g[a:a + 40].copy())
    order = rng.permutation(len(reads))
    concat, offsets = _batch_of([reads[i] for i in order])
    want = _oracle_summary(ora, concat, offsets, 1e-7)
    _assert_records(want, _device_chars_summary(sbwt, concat, offsets, 1e-7), offsets, "kbo_map_batch_dev's characters vs the oracle")
    dev = batch.DeviceBatch(sbwt, concat, offsets, device=torch.device("cuda:0"), format=False, want_ms=False)
    dev._summary_buffers()
    dev.summary.fill_(-1)
    dev.run_summary()
    torch.cuda.synchronize()
    assert dev.fused
    n_fl = int((_flags(dev) != 0).sum())
    assert n_flagged <= n_fl < n_flagged + 100
    _assert_records(dev.summary_host(), want, offsets, "kbo_summary_batch_dev")
    ms = batch.MapStream(sbwt, dev.n_seqs, dev.total, dev.max_len, pipelines=2)
    try:
        dev.summary.fill_(-1)
        ms.wait(ms.submit_summary(dev))
        assert dev.fused
        _assert_records(dev.summary_host(), want, offsets, "kbo_map_stream_submit_summary")
    finally:
        ms.close()


def _long_batch(rng, g):
    """161 b, 1 kb and 50 kb: an N run, and a run of '-' across the reducer's 1 024-character tile boundary (unrelated bases there)"""
    seqs = []
    for length in (161, 1000, 50_000):
        reps = (length + len(g) - 1) // len(g)
        s = np.tile(g, reps)[:length].copy() if length > len(g) else g[100:100 + length].copy()
        hit = rng.random(length) < 0.01
        s[hit] = ACGT[rng.integers(0, 4, int(hit.sum()))]
        seqs.append(s)
    seqs[1][400:420] = ord("N")
    seqs[2][3000:3050] = ord("N")
    junk = ACGT[rng.integers(0, 4, 300)]
    b0 = 8 * 1024 - (161 + 1000)  # position of the 50 kb sequence that lies on a tile boundary of the batch's characters
    seqs[2][b0 - 150:b0 + 150] = junk
    return seqs


def test_generic_route_long_sequences_and_settings(oracle):
    import torch
    L = kbo_amd.lib()
    g, sbwt, ora = _index(oracle, 31)
    rng = np.random.default_rng(3)
    seqs = _long_batch(rng, g)
    concat, offsets = _batch_of(seqs)
    want = _oracle_summary(ora, concat, offsets, 1e-7)
    chars = ora.matches_batch(concat, offsets, 1e-7, n_threads=threads())
    c50 = chars[161 + 1000:]
    b0 = 8 * 1024 - (161 + 1000)
    assert c50[b0 - 1] == ord("-") and c50[b0] == ord("-"), "a run of '-' crosses the reducer's tile boundary"
    mixed = [g[a:a + 150].copy() for a in rng.integers(0, len(g) - 150, 70)] + seqs[:2] + [g[a:a + 2].copy() for a in (5, 9)] + [seqs[2][:5000]]
    mc, mo = _batch_of([mixed[i] for i in rng.permutation(len(mixed))])
    for long_mode in (1, 0, 2):
        L.kbo_set_map_long(long_mode)
        for cc, oo, ww in ((concat, offsets, want), (mc, mo, _oracle_summary(ora, mc, mo, 1e-7))):
            dev = batch.DeviceBatch(sbwt, cc, oo, device=torch.device("cuda:0"), format=False, want_ms=False)
            dev._summary_buffers()
            dev.summary.fill_(-1)
            dev.run_summary()
            torch.cuda.synchronize()
            _assert_records(dev.summary_host(), ww, oo, "kbo_set_map_long(%d)" % long_mode)
            _assert_records(dev.summary_host(), _device_chars_summary(sbwt, cc, oo, 1e-7), oo, "kbo_set_map_long(%d) vs the device's characters" % long_mode)
    L.kbo_set_map_long(1)


def test_generic_route_no_depth_table_and_shards(oracle):
    import torch
    L = kbo_amd.lib()
    g, _, ora = _index(oracle, 31)
    rng = np.random.default_rng(4)
    reads = _ragged_reads(rng, g)
    concat, offsets = _batch_of(reads)
    want = _oracle_summary(ora, concat, offsets, 1e-7)
    # a handle whose options switch the depth table off
    sb2, _ = kbo_amd.build([g], kbo_amd.BuildOpts(k=31, num_threads=threads()))
    sb2.set_opts(depth_table=-1)
    dev = batch.DeviceBatch(sb2, concat, offsets, device=torch.device("cuda:0"), format=False, want_ms=False)
    dev.run_summary()
    torch.cuda.synchronize()
    assert not dev.fused
    _assert_records(dev.summary_host(), want, offsets, "no depth table")
    # a sharded handle
    contigs = [g[:GENOME // 2], g[GENOME // 2:]]  # (an index is sharded by its input sequences)
    L.kbo_set_index_shards(2)
    sb3, _ = kbo_amd.build(contigs, kbo_amd.BuildOpts(k=31, num_threads=threads()))
    L.kbo_set_index_shards(0)
    assert L.kbo_index_shards(sb3._h) == 2
    want = _oracle_summary(oracle.Index.build([c.tobytes() for c in contigs], k=31), concat, offsets, 1e-7)
    dev = batch.DeviceBatch(sb3, concat, offsets, device=torch.device("cuda:0"), format=False, want_ms=False)
    dev.run_summary()
    torch.cuda.synchronize()
    assert not dev.fused
    _assert_records(dev.summary_host(), want, offsets, "sharded")
    keep = np.diff(offsets.astype(np.int64)) >= 3
    c2, o2 = _batch_of([r for r, kp in zip(reads, keep) if kp])
    _assert_records(batch.summary_batch(sb3, (c2, o2)), want[keep], o2, "kbo_summary_batch, sharded")


def test_reducer_alone_on_bytes_and_words(oracle):
    import torch
    L = kbo_amd.lib()
    g, sbwt, ora = _index(oracle, 31)
    rng = np.random.default_rng(6)
    seqs = _ragged_reads(rng, g) + _long_batch(rng, g)
    concat, offsets = _batch_of([seqs[i] for i in rng.permutation(len(seqs))])
    lens = np.diff(offsets.astype(np.int64))
    chars = np.full(len(concat), ord("M"), dtype=np.uint8)  # the bytes of the sequences of fewer than 3 bases: pre-filled with 'M'
    keep = np.flatnonzero(lens >= 3)
    c2, o2 = _batch_of([concat[int(offsets[s]):int(offsets[s + 1])] for s in keep])
    oc = ora.matches_batch(c2, o2, 1e-7, n_threads=threads())
    for j, s in enumerate(keep):
        chars[int(offsets[s]):int(offsets[s + 1])] = oc[int(o2[j]):int(o2[j + 1])]
    want = batch.summary_of_chars(chars, offsets)
    assert (want[lens < 3] == 0).all() and (lens < 3).any()
    dv = torch.device("cuda:0")
    n = len(lens)
    off_d = torch.from_numpy(offsets.view(np.int64)).to(dv)
    s = torch.cuda.current_stream(dv)
    for shift in (0, 5):  # any alignment of the characters
        d_chars = Guarded("chars", len(chars), 4096, dv, data=chars, front=4096)
        if shift:
            d_chars = Guarded("chars", len(chars) + shift, 4096, dv, data=np.concatenate([np.full(shift, ord("X"), dtype=np.uint8), chars]))
        out = Guarded("summary", 16 * n, 4096, dv)
        for max_len in (int(lens.max()), 0):
            kbo_amd.check(L.kbo_summary_dev(d_chars.ptr + shift, off_d.data_ptr(), n, max_len, out.ptr, s.cuda_stream))
            torch.cuda.synchronize()
            out.assert_intact("kbo_summary_dev")
            _assert_records(out.host().view(np.uint32).reshape(n, 4), want, offsets, "kbo_summary_dev (bytes, shift %d, max_len %d)" % (shift, max_len))
    # the words: kbo_matches_batch_packed's alphabet; the padding bits of a sequence's last word and the words of the short sequences hold anything
    code = np.zeros(256, dtype=np.uint32)
    code[ord("-")], code[ord("X")], code[ord("R")] = 1, 2, 3
    nw = (lens + 15) // 16
    wo = np.concatenate([[0], np.cumsum(nw)])
    words = rng.integers(0, 1 << 32, int(wo[-1]), dtype=np.uint64).astype(np.uint32)
    for sq in range(n):
        a, b = int(offsets[sq]), int(offsets[sq + 1])
        if b - a < 3:
            continue
        cs = code[chars[a:b]]
        for w in range(int(nw[sq])):
            part = cs[16 * w:16 * w + 16]
            keep_bits = np.uint32(0xFFFFFFFF) if len(part) == 16 else np.uint32((1 << (2 * len(part))) - 1)
            v = np.uint32(sum(int(c) << (2 * i) for i, c in enumerate(part)))
            words[int(wo[sq]) + w] = (words[int(wo[sq]) + w] & ~keep_bits) | v
    d_words = Guarded("words", 4 * len(words), 4096, dv, data=words.view(np.uint8))
    wb = int(L.kbo_summary_words_work_bytes(n))
    assert wb > 0
    work = Guarded("work", wb, 4096, dv)
    out = Guarded("summary", 16 * n, 4096, dv)
    kbo_amd.check(L.kbo_summary_words_dev(d_words.ptr, off_d.data_ptr(), n, 0, out.ptr, work.ptr, s.cuda_stream))
    torch.cuda.synchronize()
    for b_ in (out, work, d_words):
        b_.assert_intact("kbo_summary_words_dev")
    _assert_records(out.host().view(np.uint32).reshape(n, 4), want, offsets, "kbo_summary_words_dev")


@pytest.mark.parametrize("shape", ["reads", "long"])
def test_exact_buffer_sizes_behind_guard_bands(oracle, shape):
    """d_summary_out of exactly 16 n_seqs bytes and d_work of exactly kbo_summary_work_bytes(), the bands around them intact"""
    import torch
    L = kbo_amd.lib()
    g, sbwt, ora = _index(oracle, 31)
    rng = np.random.default_rng(8)
    seqs = _ragged_reads(rng, g) if shape == "reads" else _long_batch(rng, g)[:2] + [g[a:a + 150].copy() for a in (10, 500)]
    concat, offsets = _batch_of(seqs)
    n, total = len(seqs), len(concat)
    max_len = int(np.diff(offsets.astype(np.int64)).max())
    dv = torch.device("cuda:0")
    wb = int(L.kbo_summary_work_bytes(sbwt._h, n, total, max_len))
    assert wb > 0
    if shape == "reads":
        assert wb == int(L.kbo_work_bytes(n, total, max_len, 31)), "the one-kernel route reserves no room for characters"
    else:
        assert wb >= int(L.kbo_index_work_bytes(sbwt._h, n, total, max_len)) + total
    q = Guarded("concat", round16(total) + 16, 4096, dv, data=concat)
    off_d = torch.from_numpy(offsets.view(np.int64)).to(dv)
    msb = Guarded("ms", round16(total) + 16, 65536, dv)
    work = Guarded("work", wb, scratch_guard_bytes(n, total, 31) + round16(total) + 4096, dv)
    out = Guarded("summary", 16 * n, 65536, dv)
    s = torch.cuda.current_stream(dv)
    fused = C.c_int(-1)
    kbo_amd.check(L.kbo_summary_batch_dev(sbwt._h, q.ptr, off_d.data_ptr(), n, total, max_len, 1e-7, msb.ptr, out.ptr, work.ptr, wb,
                                          s.cuda_stream, s.cuda_stream, C.byref(fused)))
    torch.cuda.synchronize()
    for b_ in (q, msb, work, out):
        b_.assert_intact(shape)
    assert fused.value == 1 or shape != "reads"
    _assert_records(out.host().view(np.uint32).reshape(n, 4), _oracle_summary(ora, concat, offsets, 1e-7), offsets, shape)
    # a byte less of d_work is refused, as kbo_map_batch_dev refuses it
    assert L.kbo_summary_batch_dev(sbwt._h, q.ptr, off_d.data_ptr(), n, total, max_len, 1e-7, msb.ptr, out.ptr, work.ptr, wb - 1,
                                   s.cuda_stream, s.cuda_stream, None) == -4


def test_pipelines_alternate_characters_and_summaries(oracle):
    import torch
    g, sbwt, ora = _index(oracle, 31)
    rng = np.random.default_rng(12)
    dv = torch.device("cuda:0")
    batches = []
    for b in range(10):  # more batches than the two pipelines have slots
        reads = [g[a:a + int(l)].copy() for a, l in zip(rng.integers(0, len(g) - 200, 150), rng.integers(3, 161, 150))]
        for r in reads[::7]:
            r[len(r) // 2] = ord("N")
        concat, offsets = _batch_of(reads)
        dev = batch.DeviceBatch(sbwt, concat, offsets, device=dv, format=False, want_ms=False)
        dev.chars.fill_(0xEE)
        exp = ora.matches_batch(concat, offsets, 1e-7, n_threads=threads())
        batches.append((dev, offsets, exp))
    ms = batch.MapStream(sbwt, 150, 150 * 160, 160, pipelines=2)
    try:
        tickets = []
        for b, (dev, _, _) in enumerate(batches):
            tickets.append(ms.submit_summary(dev) if b % 2 == 0 else ms.submit(dev))
            assert dev.fused
        for b in rng.permutation(len(batches)):  # out of order
            ms.wait(tickets[b])
            dev, offsets, exp = batches[b]
            if b % 2 == 0:
                _assert_records(dev.summary_host(), batch.summary_of_chars(exp, offsets), offsets, "batch %d" % b)
                assert bool((dev.chars == 0xEE).all())
            else:
                assert np.array_equal(dev.chars[:dev.total].cpu().numpy(), exp)
    finally:
        ms.close()


def test_host_entry_points_slabs_and_errors(oracle):
    L = kbo_amd.lib()
    g, sbwt, ora = _index(oracle, 31)
    rng = np.random.default_rng(14)
    # sequences of 4 096 bases: with slabs of 64 KiB a sequence boundary falls on every slab boundary; reads in between, N and lower case
    seqs = []
    for i in range(80):
        a = int(rng.integers(0, len(g) - 4096))
        s = g[a:a + 4096].copy()
        hit = rng.random(4096) < 0.01
        s[hit] = ACGT[rng.integers(0, 4, int(hit.sum()))]
        if i % 5 == 0:
            s[100:103] = ord("N")
        if i % 7 == 0:
            s[50] |= 0x20
        seqs.append(s)
    concat, offsets = _batch_of(seqs)
    L.kbo_set_slab_bytes(64 << 10)
    assert len(concat) >= 4 * (64 << 10) and (64 << 10) % 4096 == 0
    want = _oracle_summary(ora, concat, offsets, 1e-7)
    _assert_records(want, batch.summary_of_chars(batch.matches_batch(sbwt, concat, offsets), offsets), offsets, "kbo_matches_batch vs the oracle")
    _assert_records(batch.summary_batch(sbwt, (concat, offsets)), want, offsets, "kbo_summary_batch")
    words, epos, ebyt = batch.pack_reads(concat, offsets)
    assert len(epos) > 0
    _assert_records(batch.summary_batch(sbwt, (concat, offsets), packed=True), want, offsets, "kbo_summary_batch_packed")
    # ragged reads (3 .. 160), packed and bytes
    reads = [r for r in _ragged_reads(rng, g) if len(r) >= 3] * 20
    rc, ro = _batch_of(reads)
    want = _oracle_summary(ora, rc, ro, 1e-7)
    _assert_records(batch.summary_batch(sbwt, (rc, ro)), want, ro, "kbo_summary_batch, reads")
    _assert_records(batch.summary_batch(sbwt, (rc, ro), packed=True), want, ro, "kbo_summary_batch_packed, reads")
    _assert_records(batch.summary_batch(sbwt, [bytes(r) for r in reads[:50]]), want[:50], ro[:51], "a list of sequences")
    # error codes: those of kbo_matches_batch[_packed]
    out = np.zeros((len(ro) - 1, 4), dtype=np.uint32)
    chars = np.zeros(len(rc), dtype=np.uint8)
    n = len(ro) - 1
    for args_m, args_s in (
        ((None, rc.ctypes.data, ro.ctypes.data, n, 1e-7, chars.ctypes.data), (None, rc.ctypes.data, ro.ctypes.data, n, 1e-7, out.ctypes.data)),
        ((sbwt._h, None, ro.ctypes.data, n, 1e-7, chars.ctypes.data), (sbwt._h, None, ro.ctypes.data, n, 1e-7, out.ctypes.data)),
        ((sbwt._h, rc.ctypes.data, None, n, 1e-7, chars.ctypes.data), (sbwt._h, rc.ctypes.data, None, n, 1e-7, out.ctypes.data)),
        ((sbwt._h, rc.ctypes.data, ro.ctypes.data, n, 1e-7, None), (sbwt._h, rc.ctypes.data, ro.ctypes.data, n, 1e-7, None)),
        ((sbwt._h, rc.ctypes.data, ro.ctypes.data, n, 1.0, chars.ctypes.data), (sbwt._h, rc.ctypes.data, ro.ctypes.data, n, 1.0, out.ctypes.data)),
        ((sbwt._h, rc.ctypes.data, ro.ctypes.data, n, -1.0, chars.ctypes.data), (sbwt._h, rc.ctypes.data, ro.ctypes.data, n, -1.0, out.ctypes.data)),
    ):
        rm, rs = L.kbo_matches_batch(*args_m), L.kbo_summary_batch(*args_s)
        assert rm == rs and (rm != 0 or args_m[4] != 1e-7), (rm, rs)
    w2, e2, b2 = batch.pack_reads(rc, ro)
    wout = np.zeros(len(w2), dtype=np.uint32)
    for sub in ((0, None), (1, None), (2, None), (8, None), (7, 1.0)):
        am = [sbwt._h, w2.ctypes.data, ro.ctypes.data, n, e2.ctypes.data if len(e2) else None, b2.ctypes.data if len(b2) else None, len(e2), 1e-7, wout.ctypes.data]
        as_ = list(am)
        as_[8] = out.ctypes.data
        am[sub[0]] = sub[1]
        as_[sub[0]] = sub[1]
        rm, rs = L.kbo_matches_batch_packed(*am), L.kbo_summary_batch_packed(*as_)
        assert rm == rs and (rm != 0 or sub[0] == 7), (sub, rm, rs)


def _routes():
    a, b = C.c_uint64(0), C.c_uint64(0)
    kbo_amd.check(kbo_amd.lib().kbo_summary_slab_routes(C.byref(a), C.byref(b)))
    return int(a.value), int(b.value)


@pytest.mark.parametrize("packed", [False, True])
def test_host_slabs_of_reads_take_the_kernels_summary_forms(oracle, packed):
    """kbo_summary_batch (reads as bytes: IO = 0) and kbo_summary_batch_packed (reads as 2-bit words: the IO = 1 form, its listed reads
    unpacked for finish_reads_kernel): slabs of reads store records and no characters (kbo_summary_slab_routes says which route a slab
    took).  Clean reads are the first kernel's; reads with an N or a lower-case base - in the packed form: a non-ACGT list - are always
    the second pass's; equal-length reads take the uniform form of the packed layout, ragged ones the scanned one."""
    L = kbo_amd.lib()
    g, sbwt, ora = _index(oracle, 31)
    rng = np.random.default_rng(21)
    big = 5 if packed else 1  # (a packed slab holds four times the bases)
    ragged = [r for r in _ragged_reads(rng, g) if len(r) >= 3] * (8 * big)
    uniform = []
    for i in range(1500 * big):
        a = int(rng.integers(0, len(g) - 200))
        r = g[a:a + 150].copy()
        hit = rng.random(150) < 0.02
        r[hit] = ACGT[rng.integers(0, 4, int(hit.sum()))]
        if i % 11 == 0:
            r[int(rng.integers(0, 150))] = ord("N")
        uniform.append(r)
    L.kbo_set_slab_bytes(64 << 10)
    for reads, what in ((ragged, "ragged"), (uniform, "uniform")):
        concat, offsets = _batch_of(reads)
        assert len(concat) > 2 * (64 << 10)  # several slabs
        has_n = np.array([bool(((r == ord("N")) | (r >= 0x60)).any()) for r in reads])
        assert has_n.any() and not has_n.all()
        for p in _thresholds(sbwt) if not packed else (1e-7,):
            want = _oracle_summary(ora, concat, offsets, p)
            k0, r0 = _routes()
            got = batch.summary_batch(sbwt, (concat, offsets), p, packed=packed)
            k1, r1 = _routes()
            assert k1 > k0 + 1 and r1 == r0, "every slab took the kernel's summary form (%d kernel, %d reducer slabs)" % (k1 - k0, r1 - r0)
            _assert_records(got, want, offsets, "%s reads, packed %s, p %g" % (what, packed, p))
    # sequences of more than 160 bases: characters on the device and the reducer
    seqs = [g[a:a + 1000].copy() for a in rng.integers(0, len(g) - 1000, 200 * big)]
    concat, offsets = _batch_of(seqs)
    k0, r0 = _routes()
    got = batch.summary_batch(sbwt, (concat, offsets), packed=packed)
    k1, r1 = _routes()
    assert k1 == k0 and r1 > r0
    _assert_records(got, _oracle_summary(ora, concat, offsets, 1e-7), offsets, "1 kb sequences, packed %s" % packed)


def test_reducer_with_offsets_that_do_not_start_at_zero(oracle):
    """kbo_summary_dev where d_offsets[0] != 0: the characters in front of the first sequence belong to nobody"""
    import torch
    L = kbo_amd.lib()
    rng = np.random.default_rng(23)
    alphabet = np.frombuffer(b"MMMMMM--XR", dtype=np.uint8)
    lens = np.concatenate([rng.integers(0, 200, 60), [3000, 1, 2, 5000]])
    offsets = (5003 + np.concatenate([[0], np.cumsum(lens)])).astype(np.uint64)
    chars = alphabet[rng.integers(0, len(alphabet), int(offsets[-1]))]
    rel = (offsets - offsets[0]).astype(np.uint64)
    want = batch.summary_of_chars(chars[int(offsets[0]):], rel)
    dv = torch.device("cuda:0")
    n = len(lens)
    d_chars = Guarded("chars", len(chars), 4096, dv, data=chars)
    off_d = torch.from_numpy(offsets.view(np.int64)).to(dv)
    out = Guarded("summary", 16 * n, 4096, dv)
    kbo_amd.check(L.kbo_summary_dev(d_chars.ptr, off_d.data_ptr(), n, 0, out.ptr, torch.cuda.current_stream(dv).cuda_stream))
    torch.cuda.synchronize()
    out.assert_intact("kbo_summary_dev")
    _assert_records(out.host().view(np.uint32).reshape(n, 4), want, rel, "offsets from 5003")
