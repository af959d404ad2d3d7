#!/bin/bash
# scratch: A/B a list of environment settings on the default bench (same box, back to back)
OUT=$(mktemp -d)
for e in "$@"; do
  env $e python bench.py --full --steps 3 --warmup 1 > $OUT/ab.json 2> $OUT/ab.err || exit 1
  python - "$e" <<PY
import json, sys
d = json.loads(open("$OUT/ab.json").read().strip().splitlines()[-1])
print("%-28s %.2f ms  solve %.1f  bulk %.1f TF  err %.10g" % (sys.argv[1], d["ms_per_step"], d["phase_ms_last_step"]["solve"], d["roofline"]["achieved"], d["final_error"]), flush=True)
PY
done
