#!/bin/sh
# Same-call A/B of two builds of the library on the bench workload (box-to-box variance is 3-6 %, so only numbers from ONE gpurun call compare):
#   scripts/ab_bench.sh <variant-name> [rounds] [control-variant]   -> alternates variants/<name>/libkazen_mi355x.so and the in-tree build
# control-variant: a second build of <variant-name>'s sources (scripts/build_rev.sh again under another name), run in the same alternation - how far two builds
# of the SAME sources lie apart is the spread a difference between the variant and the tree has to exceed.
# Output: the file $OUT below, with one "<tag> Msamples/s ms_per_step C1-job-Msamples/s" line per run (the last: ext_scenes.C1, the host-bound job, which bench.py
# runs under --full only: AB_BENCH_ARGS="--full --no-cpu-baseline --no-asset-scene --no-cold-job --no-parity" adds it to every run).
NAME=$1; ROUNDS=${2:-2}; CONTROL=$3
OUT=gpurun_out/ab_$NAME.txt
mkdir -p gpurun_out; : > $OUT
one() {   # tag, lib path ('' = in-tree)
    KZ_LIB_PATH=$2 timeout -k 10 300 python bench.py --steps 3 --warmup 1 $AB_BENCH_ARGS 2>${OUT%.txt}.err | python -c "import sys,json; d=json.loads(sys.stdin.read()); print('$1', d['value'], d['ms_per_step'], d.get('ext_scenes', {}).get('C1', {}).get('value'))" >> $OUT || exit 1
}
i=0
while [ $i -lt $ROUNDS ]; do
    one "$NAME" nano-kazen_amd/csrc/variants/$NAME/libkazen_mi355x.so || exit 1
    one tree "" || exit 1
    [ -z "$CONTROL" ] || one "$CONTROL" nano-kazen_amd/csrc/variants/$CONTROL/libkazen_mi355x.so || exit 1
    i=$((i + 1))
done
cat $OUT
