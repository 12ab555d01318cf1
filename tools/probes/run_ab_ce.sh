#!/bin/bash
# A/B of two builds of the library over the candidate-sweep losses (csrc/cr_ce.hip) on one box in one job: CASTREC_LIB=<base .so>
# against the default, alternating base / branch, N rounds of the four loss benchmarks (kernel times only).  Every step runs under
# its own limit and the first failure ends the job.
#   tools/probes/run_ab_ce.sh <base .so> [rounds] [out.json]
# out.json: per (tool, shape, N, precision) both sides' per-run medians, the median of each, the ratio branch / base and the base's
# own spread (max - min) / median -- the margin the ratio is read against.
base="$1"; n="${2:-3}"; json="${3:-${OUT_DIR:-bench_out}/ab_ce/ab.json}"; out="$(dirname "$json")/runs"; mkdir -p "$out"
for r in $(seq 1 "$n"); do
  for w in base branch; do
    if [ "$w" = base ]; then export CASTREC_LIB="$PWD/$base"; else unset CASTREC_LIB; fi
    timeout -k 10 120 python tools/ce_bench.py --no-torch --no-step --shapes a,b > "$out/$w$r.ce.jsonl" 2> "$out/$w$r.ce.err" &&
    timeout -k 10 240 python tools/sce_bench.py --no-torch --no-ce --no-step > "$out/$w$r.sce.jsonl" 2> "$out/$w$r.sce.err" &&
    timeout -k 10 240 python tools/sce_bench.py --no-torch --no-ce --no-step --proposal popularity > "$out/$w$r.sce_pop.jsonl" 2> "$out/$w$r.sce_pop.err" &&
    timeout -k 10 240 python tools/gbce_bench.py --no-torch --no-step > "$out/$w$r.gbce.jsonl" 2> "$out/$w$r.gbce.err" ||
      { echo "failed: $w round $r"; tail -n 3 "$out/$w$r".*.err; exit 1; }
    echo "$w round $r done"
  done
done
unset CASTREC_LIB
python - "$out" "$n" "$json" <<'P'
import json, os, statistics, sys
out, n, path = sys.argv[1], int(sys.argv[2]), sys.argv[3]
rows = {}
for side in ("base", "branch"):
    for r in range(1, n + 1):
        for tool in ("ce", "sce", "sce_pop", "gbce"):
            for line in open(os.path.join(out, "%s%d.%s.jsonl" % (side, r, tool))):
                if line.startswith("{"):
                    d = json.loads(line)
                    key = (tool, d["shape"], d.get("N", 0), d["precision"])
                    rows.setdefault(key, dict(base=[], branch=[]))[side].append(d["time_s"])
res = []
for (tool, shape, N, prec), t in sorted(rows.items()):
    b, v = statistics.median(t["base"]), statistics.median(t["branch"])
    res.append(dict(tool=tool, shape=shape, N=N, precision=prec, base_s=t["base"], branch_s=t["branch"], base_median_s=b,
                    branch_median_s=v, ratio=v / b, base_spread=(max(t["base"]) - min(t["base"])) / b))
    res[-1]["slower_than_spread"] = res[-1]["ratio"] - 1.0 > res[-1]["base_spread"]
    print("%-8s %s N=%-5d %-7s base %.4e branch %.4e ratio %.4f spread %.4f%s" % (tool, shape, N, prec, b, v, v / b, res[-1]["base_spread"],
                                                                                 "  <-- slower" if res[-1]["slower_than_spread"] else ""))
with open(path, "w") as f:
    json.dump(dict(rounds=n, rows=res), f, indent=1)
P
