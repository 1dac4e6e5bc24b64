#!/bin/bash
# SQ counters of the headline in a counters-only rocprofv3 pass (no tracing
# combined with --pmc), run on the GPU box from the repo root:
#   OUT=dir [VARIANTS="base parent ..."] bash tools/sq_counters_headline.sh
# base = minotaur_amd/libmgpu.so, others tools/_stamps/<name>/libmgpu.so (as
# tools/ab_headline.sh); one pass per variant into $OUT/sq_<name> (OUT is the
# run's output directory, default prof_out/sq under the repo root).
# tools/sq_summary.py turns a pass into per-launch and per-LP figures.
set -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd)
O=${OUT:-$R/prof_out/sq}; mkdir -p $O; O=$(cd $O && pwd)
CTRS=${CTRS:-SQ_INSTS_VALU SQ_ACTIVE_INST_VALU SQ_WAVE_CYCLES}
ARGS=${ARGS:---steps 3 --warmup 1 --batch 524288}
cd /tmp && export TMPDIR=/tmp
for v in ${VARIANTS:-base}; do
  if [ "$v" = base ]; then L=$R/minotaur_amd/libmgpu.so; else L=$R/tools/_stamps/$v/libmgpu.so; fi
  MGPU_LIB=$L timeout -k 10 300 rocprofv3 --pmc $CTRS -d $O/sq_$v -o run --output-format csv -- python3 $R/bench.py $ARGS > $O/bench_sq_$v.log 2>&1 || { tail -20 $O/bench_sq_$v.log; exit 1; }
  find $O/sq_$v -name "*counter_collection.csv" | head -3
done
echo SQ DONE
