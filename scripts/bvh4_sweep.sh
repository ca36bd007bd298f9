#!/bin/bash
# Same-call comparison of the leaf parameters of the SAH-optimal BVH4 collapse (development build: KZ_BVH4_PRIM_COST / KZ_BVH4_MAX_LEAF) on the C4 stage
# times and executed counters: scripts/bvh4_sweep.sh "0.4 0.6 0.9" "4 8"
run() { echo "$1 $(env $1 python scripts/probe.py stages 2>&1 | tail -1 | python -c "import sys,json; d=json.loads(sys.stdin.read()); print(d['Msamples_per_s'], d['stages_one_pass_alone'])")"; }
for pc in ${1:-0.6}; do for ml in ${2:-4}; do run "KZ_BVH4_PRIM_COST=$pc KZ_BVH4_MAX_LEAF=$ml"; done; done
