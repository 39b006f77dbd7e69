"""kbo_map_stream_* over batches of reads: the pipelines whose kernels' stream runs on every compute unit and whose second passes
(finish_reads_kernel in workgroups of one wave) go to a stream of the highest priority.  Every batch's output must equal what
kbo_map_batch_dev computes for it on one stream - for reads that leave few, many or nearly all of themselves to the second pass."""
import numpy as np
import pytest
import torch

import kbo_amd
from kbo_amd import batch, synth

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


@pytest.fixture(scope="module")
def index():
    g = synth.genome(300_000)
    sbwt, _ = kbo_amd.build([g], kbo_amd.BuildOpts(k=31, num_threads=8))
    return g, sbwt


def _revcomp(concat, offsets):
    comp = np.zeros(256, dtype=np.uint8)
    for a, b in zip(b"ACGT", b"TGCA"):
        comp[a] = b
    out = concat.copy()
    for i in range(len(offsets) - 1):
        s, e = int(offsets[i]), int(offsets[i + 1])
        out[s:e] = comp[concat[s:e][::-1]]
    return out


def _batches(g):
    """(name, concat, offsets): 1 % and 5 % substitutions, reads of the other strand, reads of an unrelated genome"""
    out = []
    c, o = synth.reads(g, 20_000, 150, 0.01, seed=11)
    out.append(("c2", c, o))
    c, o = synth.reads(g, 20_000, 150, 0.05, seed=12)
    out.append(("sub5", c, o))
    c, o = synth.reads(g, 8_000, 150, 0.01, seed=13)
    out.append(("other_strand", _revcomp(c, o), o))
    c, o = synth.reads(synth.genome(300_000, seed=99), 8_000, 150, 0.01, seed=14)
    out.append(("unrelated", c, o))
    return out


def _expected(sbwt, concat, offsets, fmt):
    d = batch.DeviceBatch(sbwt, concat, offsets, device=DEV, format=fmt, want_ms=False)
    s = torch.cuda.Stream(DEV)
    d.run(s)
    torch.cuda.synchronize(DEV)
    assert d.fused, "reads over an index copy with a depth table take map_reads_kernel"
    return d.chars[:d.total].cpu().numpy().copy()


@pytest.mark.parametrize("pipelines", [1, 2])
@pytest.mark.parametrize("fmt", [True, False])
def test_every_batch_equals_one_stream(index, pipelines, fmt):
    g, sbwt = index
    sets = [(name, batch.DeviceBatch(sbwt, c, o, device=DEV, format=fmt, want_ms=False), _expected(sbwt, c, o, fmt))
            for name, c, o in _batches(g)]
    ms = batch.MapStream(sbwt, max(d.n_seqs for _, d, _ in sets), max(d.total for _, d, _ in sets), 150, pipelines=pipelines)
    try:
        for rnd in range(3):  # (the slots and the resident output buffers taken again on later submits)
            for _, d, _ in sets:
                d.chars.fill_(0xEE)
            torch.cuda.synchronize(DEV)
            tickets = [ms.submit(d) for _, d, _ in sets]
            for (name, d, want), t in zip(sets, tickets):
                ms.wait(t)
                assert d.fused
                got = d.chars[:d.total].cpu().numpy()
                assert np.array_equal(got, want), "pipelines=%d fmt=%s round %d: batch %s differs from kbo_map_batch_dev" % (
                    pipelines, fmt, rnd, name)
    finally:
        ms.close()


@pytest.mark.parametrize("n_submits", [1, 2, 3])
def test_sync_after_submits(index, n_submits):
    g, sbwt = index
    sets = [(batch.DeviceBatch(sbwt, c, o, device=DEV, format=True, want_ms=False), _expected(sbwt, c, o, True)) for _, c, o in _batches(g)[:3]]
    ms = batch.MapStream(sbwt, max(d.n_seqs for d, _ in sets), max(d.total for d, _ in sets), 150, pipelines=2)
    try:
        for d, _ in sets:
            d.chars.fill_(0xEE)
        torch.cuda.synchronize(DEV)
        for d, _ in sets[:n_submits]:
            ms.submit(d)
        ms.sync()
        for d, want in sets[:n_submits]:
            assert np.array_equal(d.chars[:d.total].cpu().numpy(), want)
    finally:
        ms.close()
