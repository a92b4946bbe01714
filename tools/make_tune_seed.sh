#!/bin/bash
# Regenerates syke-pic_amd/sykepic_hip/tune_seed_gfx950.txt on one MI355X: every tuner times its candidates from an
# empty cache for the shapes of the shipped benchmarks (ResNet-50 inference in the calibrated and the mixed mode + the
# training step at batch 256, ResNet-18 both, EfficientNet-B0 / B4 inference at batch 128), the winners are written sorted
# under the file's header.  The two-stream forwards of the ResNets tune their half batches as pairs, so their "<tag>_p"
# lines (csrc/tune_table.h) come out of the same runs: they go to tune_seed_gfx950_paired.txt, a file of its own beside
# the seed.  Usage (repo root, on the GPU box): bash tools/make_tune_seed.sh ; the two results land beside the raw cache
# (the directory of SPK_TUNE_CACHE below) under the tracked files' names: copy them over the tracked files.
#   bash tools/make_tune_seed.sh paired : the paired file only - the ResNet inference runs start on the tracked seed,
#   so that what the seed answers is not timed again, and the seed stays as it is.
set -e
mkdir -p gpurun_out
export SPK_TUNE_SEED=0
export SPK_TUNE_CACHE=$PWD/gpurun_out/tune_seed_raw.txt
rm -f $SPK_TUNE_CACHE
OUT=$(dirname $SPK_TUNE_CACHE)
SEED=syke-pic_amd/sykepic_hip/tune_seed_gfx950.txt
PSEED=syke-pic_amd/sykepic_hip/tune_seed_gfx950_paired.txt
paired_out() {
  {
    grep "^#" $PSEED
    grep -E "^[a-z0-9]+_p " $SPK_TUNE_CACHE | sort -u
  } > $OUT/tune_seed_gfx950_paired.txt
  wc -l $OUT/tune_seed_gfx950_paired.txt
}
B="python3 bench.py --full --no-cpu-baseline --steps 3 --warmup 2"
if [ "$1" = paired ]; then
  grep -v "^#" $SEED > $SPK_TUNE_CACHE
  $B --mode infer > $OUT/seed_r50.json 2> $OUT/seed.err
  $B --mode infer --network resnet18 > $OUT/seed_r18.json 2>> $OUT/seed.err
  paired_out
  exit 0
fi
$B > gpurun_out/seed_r50.json 2> gpurun_out/seed.err
$B --network resnet18 > gpurun_out/seed_r18.json 2>> gpurun_out/seed.err
$B --mode infer --network efficientnet_b0 --batch 128 > gpurun_out/seed_b0.json 2>> gpurun_out/seed.err
$B --mode infer --network efficientnet_b4 --batch 128 > gpurun_out/seed_b4.json 2>> gpurun_out/seed.err
$B --mode infer --network efficientnet_b4 --batch 128 --precision fp8 > gpurun_out/seed_b4f8.json 2>> gpurun_out/seed.err || true
{
  grep "^#" $SEED
  grep -v "^#" $SPK_TUNE_CACHE | grep -vE "^[a-z0-9]+_p " | sort -u
} > gpurun_out/tune_seed_gfx950.txt
wc -l gpurun_out/tune_seed_gfx950.txt
paired_out
