#!/bin/bash
# A/B of one library under two environments on one box, alternating, N rounds:  gpurun -- tools/probes/run_ab_env.sh "VAR=1" [rounds] [bench args]
# (the step differs by ~0.5 % between runs of one binary and by 1-2 % between boxes: compare only inside one call)
envs=$1; n=${2:-3}; shift 2; out=${OUT_DIR:-bench_out}/abe; mkdir -p $out
for r in $(seq 1 $n); do
  for w in base var; do
    if [ $w = var ]; then pre="env $envs"; else pre=""; fi
    $pre timeout -k 10 200 python bench.py --full --no-cpu-baseline --no-gather --no-other-configs --no-extra-precisions "$@" > $out/$w$r.json 2> $out/$w$r.err || { echo fail; tail -3 $out/$w$r.err; exit 1; }
    python - <<P
import json
d = json.loads(open("$out/$w$r.json").read().strip().split("\n")[-1])
print("$w round $r:", d["value"], d["ms_per_step"], {k: v["us_per_step"] for k, v in d["kernels"].items()})
P
  done
done
