"""Diagnostic: where K1's persistent kernel spends its wave-cycles on the
headline (tls4-OA, depth-first, warm 2, the root plus B seeded boxes, one
round per step): s_memtime sections of the stamped build summed over all
waves of the timed rounds.

    python tools/variant_build.py k1stamps fbbt_linear.hip '#include "wave.h"' \
        $'#define MGPU_K1_STAMPS 1\\n#include "wave.h"'
    MGPU_LIB=tools/_stamps/k1stamps/libmgpu.so python tools/k1_stamps.py OUT.json \
        [--batch 524288] [--steps 20] [--warmup 3] [--modes 2,3]

Run on the GPU; one JSON with the shares per tree mode (mgpu_bnb_fbbt_carry).
"""
import ctypes
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NAMES = ['row_loop', 'objective', 'tighten_ints_check', 'refill_box_in', 'retire_box_out', 'rest']


def opt(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def main():
    from minotaur_amd.problem import LinProblem, random_boxes
    from minotaur_amd.runtime import Context
    out = sys.argv[1]
    B, steps, warmup = int(opt('--batch', 524288)), int(opt('--steps', 20)), int(opt('--warmup', 3))
    modes = [int(m) for m in opt('--modes', '2,3').split(',')]
    p = LinProblem.load(os.path.join(ROOT, 'minotaur_amd', 'instances', 'tls4_oa.npz'))
    LB, UB = random_boxes(p, B, 20261017)
    ctx = Context(0)
    fn = ctx.lib.mgpu_debug_k1_stamps
    fn.argtypes = [ctypes.POINTER(ctypes.c_ulonglong), ctypes.c_int]
    buf = (ctypes.c_ulonglong * 8)()
    ctx.load(p)
    res = {'what': 's_memtime cycles of fbbt_linear_persist per section, all waves, over the '
                   f'timed rounds of the headline (batch {B}, {steps} steps after {warmup})',
           'modes': {}}
    for mode in modes:
        ctx.bnb_config(0, 2)
        ctx.bnb_brancher(0)
        ctx.bnb_fbbt_carry(mode)
        ctx.bnb_init(B * (warmup + steps + 2) + 2)
        ctx.bnb_import(LB, UB, np.full(B, -math.inf), np.zeros(B, dtype=np.int32))
        inc, k1 = math.inf, []
        for r in range(warmup + steps):
            if r == warmup:
                ctx.sync()
                assert fn(buf, 1) == 0
            st = ctx.bnb_round(B, inc)
            inc = min(inc, st.incumbent)
            ctx.sync()
            if r >= warmup:
                k1.append(ctx.last_kernel_ms('fbbt'))
        assert fn(buf, 1) == 0
        cyc = [int(buf[i]) for i in range(6)]
        tot = float(sum(cyc)) or 1.0
        res['modes'][str(mode)] = {'cycles': dict(zip(NAMES, cyc)),
                                   'share': {n: round(c / tot, 4) for n, c in zip(NAMES, cyc)},
                                   'k1_ms_stamped_build': round(float(np.mean(k1)), 3),
                                   'nodes': int(st.nodes)}
        print(mode, res['modes'][str(mode)]['share'], res['modes'][str(mode)]['k1_ms_stamped_build'],
              flush=True)
    ctx.close()
    with open(out, 'w') as fh:
        json.dump(res, fh, indent=1)
        fh.write('\n')


if __name__ == '__main__':
    main()
