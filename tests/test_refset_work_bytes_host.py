"""Every *_work_bytes figure of the device-resident reference-set calls (kbo_hip.h) against a recorded table: the figures are contract -
the guard-band tests run the calls at exactly their figure - so a change to the d_work layouts (kbo_amd/csrc/refset_dev.cpp) that moves
one of them shows here, without a device.  tests/golden/refset_work_bytes.json holds the sets (seeded reference sequences; LDS only,
with a wide reference, with one of the single-index route, with a prefilter, with positions; k = 5 and 31) and a few hundred rows thinned
from the full grid of arguments, refused ones (a figure of 0) among them."""
import json
import os

import numpy as np

import kbo_amd
from kbo_amd import refset

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "refset_work_bytes.json")
FUNCTIONS = {
    "find": "kbo_find_refset_dev_work_bytes", "summary": "kbo_summary_refset_dev_work_bytes", "best": "kbo_best_refset_dev_work_bytes",
    "cand": "kbo_refset_candidates_dev_work_bytes", "find_screened": "kbo_find_refset_screened_dev_work_bytes",
    "summary_screened": "kbo_summary_refset_screened_dev_work_bytes", "best_screened": "kbo_best_refset_screened_dev_work_bytes",
    "cover": "kbo_cover_refset_dev_work_bytes",
}


def _build(spec, k):
    rng = np.random.RandomState(spec["seed"])
    seqs = [np.frombuffer(b"ACGT", dtype=np.uint8)[rng.randint(0, 4, n)] for n in spec["lens"]]
    return refset.RefSet.build(seqs, kbo_amd.BuildOpts(k=k, num_threads=1), wide_rows=spec.get("wide_rows"),
                               prefilter=bool(spec.get("prefilter")), positions=bool(spec.get("positions")))


def test_work_bytes_equal_the_recorded_figures():
    table = json.load(open(GOLDEN))
    specs = {s["name"]: s for s in table["sets"]}
    L = kbo_amd.lib()
    sets, seen, nonzero = {}, set(), 0
    assert len(table["rows"]) >= 200
    for name, k, fn, args, want in table["rows"]:
        if (name, k) not in sets:
            sets[(name, k)] = _build(specs[name], k)
        got = int(getattr(L, FUNCTIONS[fn])(sets[(name, k)]._h, *args))
        assert got == want, "%s(%s, k = %d, %r): %d, recorded %d" % (FUNCTIONS[fn], name, k, args, got, want)
        seen.add(fn)
        nonzero += want != 0
    assert seen == set(FUNCTIONS) and len(sets) == 2 * len(specs) and nonzero >= 100
