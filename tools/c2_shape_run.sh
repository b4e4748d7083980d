#!/bin/bash
# GPU box: the bench line at BASELINE C2's shape (32 agents, 512 map tokens, R = 80) for 1024 and 2048 scenes per GPU
for s in 1024 2048; do
  timeout 600 python bench.py --full --agents 32 --map-tokens 512 --scenes $s --steps 5 --warmup 2 --no-cpu-baseline --no-literal | python -c "
import json, sys
d = json.loads(sys.stdin.read().strip().splitlines()[-1])
r = d['roofline']
print($s, d['value'], d['ms_per_step'], r['frac'], r['avg_launch_us'], r.get('traffic'), d.get('parity', {}).get('ok'))"
done
