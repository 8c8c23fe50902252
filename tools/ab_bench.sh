#!/bin/bash
# tools/ab_bench.sh <tag> v1 v2 ...: the headline bench (short) with each variants/<v>.so, interleaved, same box; one line per run
# (ms_per_step) into the log.  REPS (default 3): rounds; BENCH_ARGS (default: the short --full run): bench.py's arguments, e.g.
# REPS=9 BENCH_ARGS="--steps 20 --warmup 5" or BENCH_ARGS="--steps 20 --warmup 5 --workload wt".
# A run that fails or exceeds its time limit ends the script: nothing more is started on the GPU.
TAG=$1; shift
OUT=gpurun_out/${TAG}.log; rm -f $OUT
REPS=${REPS:-3}
BENCH_ARGS=${BENCH_ARGS:---full --steps 10 --warmup 2 --no-cpu-baseline}
for rep in $(seq 1 $REPS); do
  for v in "$@"; do
    r=$(PIME_ALLOW_LIB_OVERRIDE=1 PIME_LIB_PATH=$PWD/variants/$v.so timeout -k 10 200 python bench.py $BENCH_ARGS 2>/dev/null | tail -1 | python -c "import json,sys; d=json.load(sys.stdin); print('ms_per_step', round(d['ms_per_step'],4), ' ', round(d['value']/1e6,3), 'M env-steps/s')") || exit 1
    echo "$v round $rep: $r" >> $OUT
  done
done
sort -s -k1,1 $OUT
