#!/bin/bash
# same-box A/B of environment switches on the default bench: tools/ab_env.sh "VAR=a" "VAR=b" ...   ("-" = no variable)
for v in "$@"; do
  if [ "$v" = "-" ]; then pre=""; else pre="$v"; fi
  env $pre timeout 400 python bench.py --full --no-cpu-baseline --no-literal --no-strict --no-parity --steps 5 2>/dev/null | python -c '
import json, sys
d = json.loads(sys.stdin.read().strip().splitlines()[-1])
r = d["roofline"]
print(sys.argv[1], "value", round(d["value"]), "ms", round(d["ms_per_step"], 2), "edge launch us", round(r["avg_launch_us"], 1), "frac", round(r["frac"], 4))' "$v"
done
