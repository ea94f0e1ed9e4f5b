#!/bin/bash
# GPU-box script: bench.py A/B over environment settings with extra bench arguments.
# Usage: ab_env_args.sh TAG ROUNDS "BENCH ARGS" "ENV1" "ENV2" ...   (each ENV: VAR=VALUE[,VAR=VALUE])
R=${GRAFT_REPO_ROOT:-$(cd "$(dirname "$0")/../.." && pwd)}
O=$R/gpurun_out/$1; ROUNDS=$2; ARGS=$3; shift 3
mkdir -p "$O"
for r in $(seq 1 "$ROUNDS"); do
  for E in "$@"; do
    env $(echo "$E" | tr ',' ' ') timeout -k 10 600 python "$R/bench.py" --full $ARGS --no-cpu-baseline > "$O/tmp.json" 2> "$O/tmp.err" || { cat "$O/tmp.err"; exit 1; }
    python3 -c "import json,sys; r=json.load(open('$O/tmp.json')); print('$ARGS', '$E', round(r['ms_per_step'],3), round(r['roofline']['kernel_ms'],4), round(r['value']/1e9,2))" | tee -a "$O/ab.txt"
  done
done
