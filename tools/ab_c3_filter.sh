#!/bin/bash
# Runs on the GPU box: bench.py --config C3 with a filter of F bases in front of the depth table (KBO_DEPTH_FILTER; 0 = none), index from one cache file
OUT=${OUT:-bench_out/c3f}
mkdir -p $OUT
python bench.py --config C3 --steps 1 --warmup 0 --no-extras --no-cpu-baseline --index-cache /tmp/C3.kbohip > /dev/null 2>&1
for f in "$@"; do
  KBO_DEPTH_FILTER=$f python bench.py --full --config C3 --steps 5 --warmup 2 --no-extras --no-cpu-baseline --index-cache /tmp/C3.kbohip > $OUT/f$f.json 2> $OUT/f$f.err
  python - $OUT/f$f.json $f <<'PY'
import json, sys
b = json.load(open(sys.argv[1])); ro = b["roofline"]
print("filter", sys.argv[2], b["value"], b["ms_per_step"], "kernel", ro.get("kernel_ms"), "redo", ro.get("redo_pass_ms"), "alone", (ro.get("alone") or {}).get("kernel_ms"), "one", (b.get("one_batch_at_a_time") or {}).get("value"))
PY
done
