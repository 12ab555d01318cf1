#!/bin/bash
# quick headline bench on the GPU box: tools/qbench.sh <tag> [extra bench flags]  -> $OUT_DIR/<tag>.json (default bench_out/) + per-kernel table
tag=$1; shift
res=${OUT_DIR:-bench_out}/$tag; mkdir -p $(dirname $res)
timeout -k 10 300 python3 bench.py --full --steps 100 --warmup 10 --no-cpu-baseline --no-gather --no-extra-precisions --no-other-configs "$@" > $res.json 2> $res.err || { tail -5 $res.err; exit 1; }
python3 - $res.json <<'PY'
import json, sys
d = json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
print("seq/s", d["value"], "ms/step", d["ms_per_step"], "launches", d["config"]["launches_per_step"])
for k, v in d["kernels"].items():
    print("  %-28s %7.1f us/step  %d launches" % (k, v["us_per_step"], v["launches"]))
PY
