#!/bin/bash
# A/B of two builds of the library on one box: the default and CASTREC_LIB=<variant>, alternating, N rounds (the step differs by ~0.5 %
# between runs of one binary: a single pair does not separate a 1 % effect)
#   gpurun -- tools/probes/run_ab.sh <variant .so> [rounds]
var=$1; n=${2:-3}; out=${OUT_DIR:-bench_out}/ab; mkdir -p $out
for r in $(seq 1 $n); do
  for w in base var; do
    if [ $w = var ]; then export CASTREC_LIB=$PWD/$var; else unset CASTREC_LIB; fi
    timeout -k 10 200 python bench.py --full --no-cpu-baseline --no-gather --no-other-configs --no-extra-precisions > $out/$w$r.json 2> $out/$w$r.err || { echo fail; tail -3 $out/$w$r.err; exit 1; }
    python - <<P
import json
d = json.loads(open("$out/$w$r.json").read().strip().split("\n")[-1])
print("$w round $r:", d["value"], d["ms_per_step"], {k: v["us_per_step"] for k, v in d["kernels"].items()})
P
  done
done
