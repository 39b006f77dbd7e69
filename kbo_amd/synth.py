"""Deterministic synthetic genomes/reads for tests and bench.py."""
import ctypes as C

import numpy as np

from ._capi import lib

GENOME_SEED = 0x6B626F0001
READS_SEED = 0x6B626F0002


def genome(length, seed=GENOME_SEED):
    out = np.empty(length, dtype=np.uint8)
    f = lib().kbo_synth_genome
    f.argtypes = [C.c_uint64, C.c_void_p, C.c_uint64]
    f.restype = None
    f(seed, out.ctypes.data, length)
    return out


def reads(genome_arr, n_reads, read_len=150, sub_rate=0.01, seed=READS_SEED, first_read=0):
    """-> (concat uint8 [n_reads*read_len], offsets uint64 [n_reads+1])"""
    g = np.ascontiguousarray(genome_arr, dtype=np.uint8)
    out = np.empty(n_reads * read_len, dtype=np.uint8)
    f = lib().kbo_synth_reads
    f.argtypes = [C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32,
                  C.c_void_p]
    f.restype = None
    f(seed, g.ctypes.data, len(g), first_read, n_reads, read_len, int(round(sub_rate * 65536)),
      out.ctypes.data)
    offsets = np.arange(n_reads + 1, dtype=np.uint64) * np.uint64(read_len)
    return out, offsets


def variant_contigs(genome_arr, n_seqs, min_len, max_len=None, sub_rate=0.01, indel_every=2000, max_indel=20,
                    insert_frac=0.05, insert_len=300, n_rate=0.0, seed=READS_SEED):
    """Stretches of `genome_arr` as another strain would have them, for kbo::map with gap filling and variants
    (tools/bench_map_opts.py, tests/test_gpu_map_batch_opts.py): sub_rate substitutions, one 1..max_indel base insertion or
    deletion every ~indel_every bases, a foreign insert of insert_len random bases in insert_frac of the sequences and
    n_rate 'N's.  Lengths uniform in [min_len, max_len].  -> (concat uint8, offsets uint64 [n_seqs + 1])"""
    rng = np.random.default_rng(seed)
    g = np.ascontiguousarray(genome_arr, dtype=np.uint8)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    max_len = max_len or min_len
    seqs = []
    for _ in range(n_seqs):
        L = int(rng.integers(min_len, max_len + 1))
        a = int(rng.integers(0, max(1, len(g) - L)))
        s = g[a:a + L].copy()
        hit = rng.random(len(s)) < sub_rate
        s[hit] = acgt[(np.searchsorted(acgt, s[hit]) + rng.integers(1, 4, int(hit.sum()))) % 4]
        parts, prev = [], 0
        for p in sorted(rng.integers(0, len(s), int(rng.poisson(len(s) / indel_every)))):
            if p < prev:
                continue
            n = int(rng.integers(1, max_indel + 1))
            parts.append(s[prev:p])
            if rng.random() < 0.5:
                parts.append(acgt[rng.integers(0, 4, n)])
                prev = p
            else:
                prev = min(len(s), p + n)
        parts.append(s[prev:])
        s = np.concatenate(parts)
        if rng.random() < insert_frac and len(s) > 2:
            p = int(rng.integers(1, len(s)))
            s = np.concatenate([s[:p], acgt[rng.integers(0, 4, insert_len)], s[p:]])
        if n_rate > 0:
            s[rng.random(len(s)) < n_rate] = ord("N")
        seqs.append(s[:max(len(s), 1)])
    offsets = np.zeros(n_seqs + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(s) for s in seqs])
    return np.concatenate(seqs).astype(np.uint8), offsets
