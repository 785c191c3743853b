#!/bin/bash
# the full bench line twice on one box (run-to-run spread of the step and of config 5's heuristic leg); usage: gpu_bench_twice.sh OUTDIR
OUT=${1:?usage: tools/gpu_bench_twice.sh OUTDIR}
mkdir -p "$OUT"
for k in 1 2; do
  timeout 900 python bench.py --full > "$OUT/bench_$k.json" 2> "$OUT/bench_$k.err"
  python3 - <<PY
import json
d = json.loads(open("$OUT/bench_$k.json").read().strip().splitlines()[-1])
print("run $k", round(d["ms_per_step"], 1), "%.3e" % d["value"], "revcomp", (d.get("revcomp") or {}).get("value"), {k: (v.get("value"), v.get("wall_s"), v.get("wall_s_runs"), v.get("slow_run_trace")) for k, v in d["configs"].items()})
PY
done
