#!/bin/bash
# A/B of libmgpu variants on the headline (run on the GPU box from the repo
# root): VARIANTS="base name1 name2 ..." (base = minotaur_amd/libmgpu.so,
# others tools/_stamps/<name>/libmgpu.so from tools/variant_build.py; name+VAR=1
# adds environment settings); each
# runs the headline REPS times (default 2), alternating, one JSON summary line
# per run (also appended to $O/runs.txt).  ARGS="--steps 20 --warmup 3" is
# bench.py's plain run.  DUMP=1 adds --dump-outputs and prints the md5 of the
# last round's round_stats and open_nodes, which two builds that compute the
# same thing share.
set -o pipefail
R=${GRAFT_REPO_ROOT:-$(pwd)}
O=$R/gpurun_out/${TAG:-ab}; mkdir -p $O; cd $R; export TMPDIR=/tmp
ARGS=${ARGS:---full --steps 10 --warmup 2 --no-cpu-baseline --no-bnb --no-qp --no-convex --no-knapsack --no-glob --no-fixed}
for rep in $(seq 1 ${REPS:-2}); do
for v in ${VARIANTS:-base}; do
  # a variant is a library name, optionally followed by +VAR=value env settings
  lib=${v%%+*}; envs=""; [ "$lib" != "$v" ] && envs=$(echo "${v#*+}" | tr '+' ' ')
  if [ "$lib" = base ]; then L=$R/minotaur_amd/libmgpu.so; else L=$R/tools/_stamps/$lib/libmgpu.so; fi
  dump=""; [ -n "$DUMP" ] && { dump="--dump-outputs $TMPDIR/ab_dump_$lib"; rm -rf $TMPDIR/ab_dump_$lib; }
  env $envs MGPU_LIB=$L timeout -k 10 300 python -u bench.py $ARGS $dump --supp-out $O/${v}_supp.json > $O/$v.json 2> $O/$v.err || { tail -5 $O/$v.err; exit 1; }
  python3 -c "
import json
d = json.loads([l for l in open('$O/$v.json') if l.startswith('{')][-1])
k = d['kernels']
print('$v', 'rep $rep', round(d['value']/1e6, 3), 'M nodes/s', round(d['ms_per_step'], 2), 'ms/step', 'K3P', k['lp_pfi']['ms'], 'ovf', k['lp_pfi']['overflow_resolve_ms'], 'K1', k['fbbt']['ms'], 'piv', k['lp_pfi']['pivots_per_solve'], 'tree', d.get('tls4_oa_tree', {}).get('nodes_per_s'))
" | tee -a $O/runs.txt || exit 1
  cp $O/$v.json $O/${v}_rep$rep.json
  [ -n "$DUMP" ] && (cd $TMPDIR/ab_dump_$lib && md5sum round_stats.npy open_nodes.npy | sed "s/^/$v rep $rep /" | tee -a $O/runs.txt)
done
done
echo AB DONE
