"""CPU model of K1's changed-column skip on the headline's search.

Runs the CPU restatement of the batched tree (oracle/bnb.py: tls4-OA,
depth-first, warm 2, the root plus B seeded boxes, one round per step) and,
for each round's popped nodes in K1's order (grouped by branching variable, a
stable sort, 64 consecutive nodes per wave), runs tools/k1_cols_model.c twice:
over all columns and with the skip.  It asserts that lb, ub, infeas and nmods
of every node are identical in the two runs and equal to oracle.linear_fbbt,
and counts per wave-sweep (the nodes of a wave that run sweep s) the column
visits and the batches of 8 of tightenInts_ + checkBounds_: today (all
columns) and under the skip (the union over the wave's lanes of the columns
stored in that sweep, a fresh lane's clean column, or all columns when a fresh
lane has none).

    python tools/k1_cols_model.py OUT.json [--batch 16384] [--rounds 6]
"""
import ctypes
import json
import math
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'oracle'))

KBND, LANES, MAX_SWEEPS = 8, 64, 10


def opt(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def build_model():
    so = os.path.join(tempfile.mkdtemp(prefix='k1cols'), 'k1_cols_model.so')
    subprocess.run(['cc', '-O2', '-ffp-contract=off', '-shared', '-fPIC', '-o', so,
                    os.path.join(ROOT, 'tools', 'k1_cols_model.c'), '-lm'], check=True)
    return ctypes.CDLL(so)


def ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def run_model(lib, p, LB, UB, inc, clean, skip):
    import oracle
    B, n = LB.shape
    colptr, rowidx = p.csc_pattern()
    oi, ov = p.obj_sparse()
    olb, oub = np.empty_like(LB), np.empty_like(UB)
    infeas, nmods = np.zeros(B, np.int32), np.zeros(B, np.int32)
    sets = np.zeros((B, MAX_SWEEPS, 2), np.uint64)
    nsw = np.zeros(B, np.int32)
    has, incv = oracle._inc_ub(p, inc)
    arrs = [np.ascontiguousarray(a) for a in (p.rowptr, p.colidx, p.val, p.rlo, p.rhi, colptr,
                                              rowidx, p.vtype)]
    oi, ov = np.ascontiguousarray(oi, np.int32), np.ascontiguousarray(ov, np.float64)
    V, I, D = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    lib.k1_cols_model.argtypes = [I, I] + [V] * 8 + [I, V, V, I, I, V, V, V, V, I, D, V, I, V, V,
                                                    V, V]
    rc = lib.k1_cols_model(int(p.n), int(p.m), *[ptr(a) for a in arrs], len(oi), ptr(oi), ptr(ov),
                           int(p.cons_bad()), int(B), ptr(LB), ptr(UB), ptr(olb), ptr(oub), int(has),
                           float(incv), ptr(clean), int(skip), ptr(infeas), ptr(nmods),
                           ptr(sets), ptr(nsw))
    assert rc == 0
    return olb, oub, infeas, nmods, sets, nsw


def popcount(x):
    return bin(int(x)).count('1')


def batches(set2, chunks):
    """Batches of KBND over the 64-record chunks of the column lists."""
    return sum(-(-popcount(sum(1 << k for k, j in enumerate(ch)
                               if (int(set2[j >> 6]) >> (j & 63)) & 1)) // KBND)
               for ch in chunks)


def main():
    import oracle
    from bnb import CpuBnbContext
    from minotaur_amd.problem import LinProblem, random_boxes
    out = sys.argv[1]
    B, rounds = int(opt('--batch', 16384)), int(opt('--rounds', 6))
    p = LinProblem.load(os.path.join(ROOT, 'minotaur_amd', 'instances', 'tls4_oa.npz'))
    assert p.n <= 128
    lib = build_model()
    ints = [j for j in range(p.n) if p.vtype[j] in (0, 1)]
    cont = [j for j in range(p.n) if p.vtype[j] not in (0, 1)]
    chunks = [ints[i:i + LANES] for i in range(0, len(ints), LANES)] + \
             [cont[i:i + LANES] for i in range(0, len(cont), LANES)]
    full = [(1 << min(64, p.n)) - 1, (1 << max(0, p.n - 64)) - 1]
    today_b = batches(full, chunks)
    LB, UB = random_boxes(p, B, 20261017)
    c = CpuBnbContext(p, 32, order=0, warm=2)      # K3P's eta cap of the headline
    c.bnb_init(B * (rounds + 2) + 2)
    c.bnb_import(LB, UB, np.full(B, -math.inf), np.zeros(B, dtype=np.int32))
    res = {'what': f'tls4-OA, depth-first, warm 2, batch {B}: column visits of tightenInts_ + '
                   'checkBounds_ per wave-sweep, all columns (today) against the changed-column '
                   'set; every node\'s lb, ub, infeas, nmods equal with and without the skip',
           'columns': p.n, 'batches_per_wave_sweep_today': today_b, 'rounds': {}}
    for r in range(1, rounds + 1):
        nb = min(B, len(c.pool))
        nodes = c.pool[len(c.pool) - nb:]
        nlb = np.ascontiguousarray(np.stack([nd.lb for nd in nodes]))
        nub = np.ascontiguousarray(np.stack([nd.ub for nd in nodes]))
        clean = np.array([nd.pvar for nd in nodes], dtype=np.int32)
        inc = c.inc
        ref = oracle.linear_fbbt(p, nlb, nub, inc if math.isfinite(inc) else None, nthreads=8)
        a = run_model(lib, p, nlb, nub, inc, clean, 0)
        s = run_model(lib, p, nlb, nub, inc, clean, 1)
        for x, y, z in zip(a[:4], s[:4], (ref.lb, ref.ub, ref.infeas, ref.nmods)):
            assert np.array_equal(x.view(np.int64) if x.dtype == np.float64 else x,
                                  y.view(np.int64) if y.dtype == np.float64 else y)
            assert np.array_equal(x.view(np.int64) if x.dtype == np.float64 else x,
                                  np.ascontiguousarray(z).view(np.int64)
                                  if z.dtype == np.float64 else z)
        assert np.array_equal(a[4], s[4]) and np.array_equal(a[5], s[5])
        sets, nsw = s[4], s[5]
        order = np.argsort(clean, kind='stable')        # key + 1, -1 first
        ws = vt = vs = bt = bs = allcol = 0
        for w0 in range(0, nb, LANES):
            lanes = order[w0:w0 + LANES]
            for sw in range(int(nsw[lanes].max())):
                act = [b for b in lanes if nsw[b] > sw]
                u = [0, 0]
                for b in act:
                    u[0] |= int(sets[b, sw, 0])
                    u[1] |= int(sets[b, sw, 1])
                u = [u[0] & full[0], u[1] & full[1]]
                ws += 1
                vt += p.n
                bt += today_b
                vs += popcount(u[0]) + popcount(u[1])
                bs += batches(u, chunks)
                allcol += u == full
        res['rounds'][str(r)] = {
            'nodes': nb, 'clean_nodes': int(np.count_nonzero(clean >= 0)), 'wave_sweeps': ws,
            'column_visits_today': vt, 'column_visits_skip': vs, 'batches_today': bt,
            'batches_skip': bs, 'all_column_wave_sweeps': allcol,
            'sweeps_per_node': round(float(nsw.mean()), 3),
            'columns_in_set_per_node_sweep': round(float(sum(
                popcount(int(sets[b, k, 0]) & full[0]) + popcount(int(sets[b, k, 1]) & full[1])
                for b in range(nb) for k in range(int(nsw[b]))) / max(1, int(nsw.sum()))), 2)}
        print(r, res['rounds'][str(r)], flush=True)
        c.bnb_round(B, inc)
    with open(out, 'w') as fh:
        json.dump(res, fh, indent=1)
        fh.write('\n')


if __name__ == '__main__':
    main()
