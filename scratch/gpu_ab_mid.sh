#!/bin/bash
# scratch: A/B environment settings on a mid-size scene (3000 / 5000 poses)
OUT=$(mktemp -d)
P=$1; L=$2; shift 2
for e in "$@"; do
  env $e python bench.py --full --config 1 --poses $P --landmarks $L --steps 5 --warmup 1 --no-cpu-baseline > $OUT/abm.json 2> $OUT/abm.err || exit 1
  python - "$e" <<PY
import json, sys
d = json.loads(open("$OUT/abm.json").read().strip().splitlines()[-1])
print("%-32s n=%d  %.2f ms  solve %.2f  bulk %.1f TF" % (sys.argv[1], d["config"]["reduced_system_n"], d["ms_per_step"], d["phase_ms_last_step"]["solve"], d["roofline"]["achieved"]), flush=True)
PY
done
