#!/usr/bin/env python3
"""kbo::build on the host against kbo::build on the device.  For each size: kbo_index_build (16 threads) followed by kbo_index_to_device,
against kbo_index_build_device (whose handle carries its device copy on return): both timings go from host bytes in to a handle with
a device copy out.  The two handles are compared with kbo_index_export_parts (k, n_kmers, n_sets, C, rows, LCS).  Prints one JSON
line per size, with the device build's split by pass (kbo_index_build_device_phases: HIP events, the copy by the host clock).
Workload: kbo_amd.synth.genome of 5 Mbp (k = 31), 100 Mbp (k = 31) and 3 Gbp (k = 63, C5's index).
Usage: tools/bench_build.py [SIZES=5e6:31,1e8:31,3e9:63] (environment)."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import kbo_amd  # noqa: E402
from kbo_amd import synth  # noqa: E402
from kbo_amd.index import SbwtIndexVariant  # noqa: E402

SIZES = [(int(float(g)), int(k)) for g, k in (s.split(":") for s in os.environ.get("SIZES", "5e6:31,1e8:31,3e9:63").split(","))]
PHASES = ("upload", "extract", "sort", "dedup", "dummies", "merge", "edges_lcs", "download", "device_copy")
L = kbo_amd.lib()


def same(a, b):
    if (a.k(), a.n_sets(), a.n_kmers()) != (b.k(), b.n_sets(), b.n_kmers()):
        return False
    ra, Ca, la = a.export_parts()
    rb, Cb, lb = b.export_parts()
    return list(Ca) == list(Cb) and all(np.array_equal(ra[c], rb[c]) for c in range(4)) and np.array_equal(la, lb)


for G, k in SIZES:
    g = synth.genome(G)
    arr = (C.c_char_p * 1)(C.cast(g.ctypes.data, C.c_char_p))
    lens = (C.c_size_t * 1)(G)
    o = kbo_amd.BuildOpts(k=k, num_threads=16)._to_c()
    res = {"genome_bp": G, "k": k}
    # device first (warm: a tiny build creates the context and loads the kernels)
    hw = C.c_void_p()
    kbo_amd.check(L.kbo_index_build_device(arr, (C.c_size_t * 1)(min(G, 10_000)), 1, C.byref(o), 0, C.byref(hw)))
    L.kbo_index_free(hw)
    hd = C.c_void_p()
    t0 = time.perf_counter()
    kbo_amd.check(L.kbo_index_build_device(arr, lens, 1, C.byref(o), 0, C.byref(hd)))
    res["device_s"] = round(time.perf_counter() - t0, 3)
    ph = (C.c_double * 9)()
    kbo_amd.check(L.kbo_index_build_device_phases(ph))
    res["device_phases_s"] = dict(zip(PHASES, (round(x, 3) for x in ph)))
    hh = C.c_void_p()
    t0 = time.perf_counter()
    kbo_amd.check(L.kbo_index_build(arr, lens, 1, C.byref(o), C.byref(hh)))
    res["host_build_s"] = round(time.perf_counter() - t0, 3)
    t1 = time.perf_counter()
    kbo_amd.check(L.kbo_index_to_device(hh, 0))
    res["host_to_device_s"] = round(time.perf_counter() - t1, 3)
    res["host_s"] = round(res["host_build_s"] + res["host_to_device_s"], 3)
    res["speedup"] = round(res["host_s"] / res["device_s"], 2)
    a, b = SbwtIndexVariant(hd), SbwtIndexVariant(hh)
    res["n_sets"] = a.n_sets()
    res["equal"] = same(a, b)
    del a, b
    print(json.dumps(res), flush=True)
