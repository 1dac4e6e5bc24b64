#!/bin/bash
# Persistent K1: time the headline batch with a wave refilling after 1 / 8 /
# 16 / 32 idle lanes (MGPU_FBBT_REFILL); run on the GPU box from the repo root.
# OUT names the output directory; --full: the sweep also reads the fixed batch.
export TMPDIR=/tmp
O=${OUT:?OUT: the directory for the logs and bench lines}; mkdir -p $O
timeout -k 10 300 python -u -m pytest -x -q --timeout 200 --timeout-method thread tests/test_fbbt_gpu.py > $O/t_refill.log 2>&1 || exit $?
for r in 1 8 16 32; do
  MGPU_FBBT_REFILL=$r timeout -k 10 200 python -u bench.py --full --steps 10 --warmup 2 --no-cpu-baseline --no-bnb --no-qp --no-glob --no-knapsack --no-convex --supp-out $O/b_refill${r}_supp.json > $O/b_refill$r.json 2> $O/b_refill$r.err || exit $?
done
