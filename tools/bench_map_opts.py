#!/usr/bin/env python3
"""kbo map with MapOpts over a batch: a loop of kbo_map (one sequence per call) against one kbo_map_batch_opts call, with the
reference's defaults and with fill_gaps only, and kbo_map_batch (no refinement) as the ceiling.  Prints one JSON line: Mbp/s of
each, the batch's phase split (kbo_map_batch_opts_phases), kbo_fill_gaps_stats and whether every sequence equals the loop.
Workload (kbo_amd.synth): a G bp genome at k = 31, N sequences of L bp taken from it with 1 % substitutions, a 1-20 base indel
every ~2 kbp and a 300 bp foreign insert in 5 % of them.  Usage: tools/bench_map_opts.py [G=5000000] [N=2000] [L=10000] [LOOP=N]
(environment; LOOP = how many sequences the kbo_map loop takes, its rate is per base)."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import kbo_amd  # noqa: E402
from kbo_amd import batch, synth  # noqa: E402

G, N, L = (int(os.environ.get(n, d)) for n, d in (("G", 5_000_000), ("N", 2000), ("L", 10_000)))
LOOP = int(os.environ.get("LOOP", N))
g = synth.genome(G)
opts = kbo_amd.BuildOpts(k=31, build_select=True, num_threads=16)
sbwt, _ = kbo_amd.build([g], opts)
sbwt.to_device()
concat, offsets = synth.variant_contigs(g, N, L, L, sub_rate=0.01, indel_every=2000, max_indel=20, insert_frac=0.05,
                                        insert_len=300, seed=11)
total = int(offsets[-1])
seqs = [concat[int(offsets[i]):int(offsets[i + 1])].tobytes() for i in range(N)]
Lb = kbo_amd.lib()


def phases():
    v = (C.c_double * 6)()
    kbo_amd.check(Lb.kbo_map_batch_opts_phases(v))
    return dict(zip(("walk", "translate", "gap_kernels", "host_fallback", "call", "apply_format"), (round(x * 1e3, 2) for x in v)))


res = {"workload": {"genome_bp": G, "n_seqs": N, "seq_bp": L, "bases": total}}
equal = True
for name, mo in (("defaults", kbo_amd.MapOpts(sbwt_build_opts=opts)),
                 ("fill_gaps_only", kbo_amd.MapOpts(call_variants=False, sbwt_build_opts=opts))):
    batch.map_batch_opts(sbwt, concat[:int(offsets[1])], offsets[:2], mo)  # (warm: the device copy and its cover)
    t0 = time.perf_counter()
    out, st = batch.map_batch_opts(sbwt, concat, offsets, mo)
    tb = time.perf_counter() - t0
    ph, stats = phases(), batch.fill_gaps_stats()
    t0 = time.perf_counter()
    loop = [kbo_amd.map(seqs[i], sbwt, None, mo) for i in range(LOOP)]
    tl = time.perf_counter() - t0
    loop_bases = sum(len(seqs[i]) for i in range(LOOP))
    eq = bool((st == 0).all()) and all(out[int(offsets[i]):int(offsets[i + 1])].tobytes() == loop[i] for i in range(LOOP))
    equal = equal and eq
    res[name] = {"batch_mbps": round(total / tb / 1e6, 3), "loop_mbps": round(loop_bases / tl / 1e6, 3),
                 "speedup": round((total / tb) / (loop_bases / tl), 2), "batch_ms": round(tb * 1e3, 1), "phases_ms": ph,
                 "gap_stats": {"gaps": stats[0], "device": stats[1], "host_seqs": stats[2], "ext_steps": stats[3],
                               "device_share": round(stats[1] / max(1, stats[0]), 4)}, "equal_to_loop": eq}
batch.map_batch(sbwt, concat, offsets, 1e-7, True)
t0 = time.perf_counter()
batch.map_batch(sbwt, concat, offsets, 1e-7, True)
res["map_batch_ceiling_mbps"] = round(total / (time.perf_counter() - t0) / 1e6, 3)
res["equal_to_loop"] = equal
print(json.dumps(res), flush=True)
