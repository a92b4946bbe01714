#!/bin/bash
# Steady-state rocprofv3 kernel statistics of bench.py (infer and train separately) with a warm tuner cache, so that
# the CSV holds no autotuning launches.  Usage (on the GPU box, from the repo root): bash tools/prof_r2.sh <tag>
set -e
export OUT=${OUT:-bench_out}   # output folder, relative to the repository root
mkdir -p $OUT
TAG=${1:-r02}
export TMPDIR=/tmp
CACHE=$PWD/$OUT/tune_${TAG}.txt
export SPK_TUNE_CACHE=$CACHE
# 1. warm the cache (tunes every problem of both modes once)
python3 bench.py --full --mode both --no-cpu-baseline --steps 3 --warmup 2 > $OUT/${TAG}_warm.json 2> $OUT/${TAG}_warm.err
for MODE in infer train; do
  rm -rf $OUT/prof_${TAG}_${MODE}
  rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_${TAG}_${MODE} -- python3 bench.py --full --mode $MODE --no-cpu-baseline --steps 20 --warmup 5 > $OUT/${TAG}_${MODE}_under_rocprof.json 2> $OUT/${TAG}_${MODE}_rocprof.err
  f=$(find $OUT/prof_${TAG}_${MODE} -name "*kernel_stats.csv" | head -1)
  cp "$f" $OUT/${TAG}_${MODE}_kernel_stats.csv
done
ls -la $OUT/${TAG}_*kernel_stats.csv
