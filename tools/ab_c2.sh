#!/bin/bash
# usage: tools/ab_c2.sh libA.so libB.so ...   -- C2 (the headline workload) with each library, alternating, three rounds:
# points/s, roofline fraction, layer-kernel milliseconds.  Same box, same process environment: 0.05 % run-to-run spread.
for round in 1 2 3; do
  for lib in "$@"; do
    MOM_LIBRARY=$PWD/$lib python bench.py --full --steps 10 --warmup 2 --no-cpu-baseline --no-voigt --no-extras 2>/dev/null | python -c "
import sys, json
d = json.loads(sys.stdin.read()); s = d['stages_ms']
print('$lib', round(d['value'], 1), round(d['roofline']['frac'], 4), 'full', round(s['full_layers_ms'], 2), 'red', round(s['reduced_layers_ms'], 2), 'step', round(d['ms_per_step'], 2))"
  done
done
