"""Time Glob's relstronger on bilinear QCQPs to closure: kind 1 (one node per
round) at batch 1 against kind 2 (batched) at batches 1, 16, 128 and 512, on
the same library.  Per setting: a warm-up solve, then REPS timed solves;
prints the median, minimum and maximum time to proof with the tree's nodes,
rounds, LPs and strong-branching LPs.

    python tools/glob_rs_time.py [REPS [seed,nv0,ncon ...]]
"""
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from minotaur_amd import glob as mglob  # noqa: E402
from minotaur_amd.quad import random_qcqp  # noqa: E402
from minotaur_amd.runtime import Context  # noqa: E402

CASES = [(0, 14, 9), (3, 14, 9), (1, 14, 9)]
SETTINGS = [(1, 1), (2, 1), (2, 16), (2, 128), (2, 512)]   # (brancher, batch)
CAPACITY = 1 << 17


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    cases = [tuple(int(v) for v in a.split(',')) for a in sys.argv[2:]] or CASES
    ctx = Context(0)
    print('| case | brancher | batch | median ms | min ms | max ms | nodes | rounds | LPs | SB LPs '
          '| nodes/s |')
    print('|---|---|---|---|---|---|---|---|---|---|---|')
    for seed, nv0, ncon in cases:
        qp = random_qcqp(seed, nv0=nv0, ncon=ncon, squares=False)
        mglob.setup(ctx, qp, 0)
        for brancher, batch in SETTINGS:
            def solve():
                return mglob.solve(ctx, qp, batch=batch, capacity=CAPACITY, loaded=True, order=2,
                                   warm=1, qt=0, lin=1, obbt=1, brancher=brancher)
            solve()
            ts = []
            for _ in range(reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                obj, _, st, _ = solve()
                torch.cuda.synchronize()
                ts.append(time.perf_counter() - t0)
            ts.sort()
            med = ts[len(ts) // 2]
            print(f'| ({seed},{nv0},{ncon}) | {brancher} | {batch} | {1e3 * med:.1f} | '
                  f'{1e3 * ts[0]:.1f} | {1e3 * ts[-1]:.1f} | {st.nodes} | {st.rounds} | {st.lps} | '
                  f'{st.sb_lps} | {st.nodes / med:.0f} |', flush=True)
    ctx.close()


if __name__ == '__main__':
    main()
