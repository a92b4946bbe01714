#!/bin/bash
# The counter half of tools/evidence_r4.sh alone (its first run of the final sources stopped in tools/pmc_traffic.py: the
# step marks were matched on a kernel name that the input conversion no longer has).  Same box = same call as nothing else.
set -e
export OUT=${OUT:-bench_out}   # output folder, relative to the repository root
TAG=r04
export TMPDIR=/tmp
mkdir -p $OUT
export SPK_TUNE_CACHE=$PWD/$OUT/tune_${TAG}.txt
rm -f $SPK_TUNE_CACHE
python3 bench.py --full --mode both --no-cpu-baseline --steps 3 --warmup 2 > $OUT/${TAG}_warm.json 2> $OUT/${TAG}_warm.err
export SPK_EVAL_STREAMS=1
export SPK_WGRAD_STREAM=0
for MODE in infer train; do
  for C in FETCH_SIZE WRITE_SIZE; do
    rm -rf $OUT/pmc_${TAG}_${MODE}_$C
    rocprofv3 --pmc $C --output-format csv -d $OUT/pmc_${TAG}_${MODE}_$C -- python3 bench.py --full --mode $MODE --no-cpu-baseline --steps 2 --warmup 1 > /dev/null 2> $OUT/pmc_${TAG}_${MODE}_$C.err
    echo "pmc $MODE $C done"
  done
  F=$(find $OUT/pmc_${TAG}_${MODE}_FETCH_SIZE -name "*counter_collection.csv" | head -1)
  W=$(find $OUT/pmc_${TAG}_${MODE}_WRITE_SIZE -name "*counter_collection.csv" | head -1)
  NAME=$([ $MODE = infer ] && echo infer_calibrated || echo train_bf16)
  python3 tools/pmc_traffic.py "$F" "$W" $OUT/${TAG}_pmc_traffic_${NAME}.json $MODE > $OUT/${TAG}_pmc_traffic_${MODE}.log
  rm -rf $OUT/pmc_${TAG}_${MODE}_FETCH_SIZE $OUT/pmc_${TAG}_${MODE}_WRITE_SIZE
done
rm -rf $OUT/pmc_${TAG}_sq
rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES GRBM_GUI_ACTIVE SQ_WAIT_ANY SQ_WAVE_CYCLES SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY --output-format csv -d $OUT/pmc_${TAG}_sq -- python3 bench.py --full --mode infer --no-cpu-baseline --steps 2 --warmup 1 > /dev/null 2> $OUT/pmc_${TAG}_sq.err
S=$(find $OUT/pmc_${TAG}_sq -name "*counter_collection.csv" | head -1)
python3 tools/pmc_mfma.py "$S" $OUT/${TAG}_pmc_mfma_util_infer_calibrated.json > $OUT/${TAG}_pmc_mfma.log
rm -rf $OUT/pmc_${TAG}_sq
tail -n 4 $OUT/${TAG}_pmc_traffic_infer.log; tail -n 4 $OUT/${TAG}_pmc_mfma.log
