#!/bin/bash
# wall time of `bench.py --full` (the headline line with every leg beside it)
#   usage: tools/gpu_bench_time.sh <output dir>
out=$(realpath -m "${1:?usage: tools/gpu_bench_time.sh <output dir>}"); mkdir -p $out
cd "$(dirname "$0")/.."
s=$(date +%s.%N)
python bench.py --full > $out/bench_full.json 2> $out/bench_full.err; rc=$?
e=$(date +%s.%N)
echo "bench.py --full: $(echo "$e - $s" | bc) s, rc=$rc"
python - $out/bench_full.json <<'PY'
import json, sys
d = json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
print(d["value"], d["ms_per_step"], d["roofline"]["frac"], d["roofline"]["frac_algorithmic"], d["cpu_baseline"]["all_cores"]["note"][:70], [s["value"] for s in d["secondary"]])
PY
