"""GPU: the smallest LP runs in which a wrong wave reduction (csrc/wave.h)
changes a result, against oracle/lp_dual.c.

tls4-OA has m = 64 rows, so all four 16-lane rows of the wave carry products
in BTRAN's symmetric sum and entries in the ratio tests' maxima and minima.
256 random boxes go through mgpu_lp_solve_path (parents, then their children
on inherited paths, where the eta file is longest) at eta caps 16, 32 and 48
(the three K3P builds), and through the dense K3 on the shared warm start.
The product-form cases for wider problems follow: knapsack_oa(f=16, N=48) has
m = 49 and runs K3P with a partly filled fourth row; knapsack_oa(f=17, N=64)
has m = 69 and is the smallest instance here that runs K3PW (64 < m <= 128),
and K3L on the same boxes.

Bars are those of the existing parity tests: statuses and pivot counts equal;
objectives and x bit for bit on the path route; objectives bit for bit and x
within 1e-9 on K3PW; objectives within 1e-9 on the dense kernels.
"""
import math
import os

import numpy as np
import pytest

import oracle
from minotaur_amd.problem import LinProblem, knapsack_oa, random_boxes
from minotaur_amd.runtime import LP_PFI_MAX, LP_PFI_WIDE_MAX, PATH_INHERIT, PATH_MAX

pytestmark = pytest.mark.gpu

INST = os.path.join(os.path.dirname(__file__), '..', 'minotaur_amd', 'instances')
NBOX = 256


@pytest.fixture(scope='module')
def ctx():
    from minotaur_amd.runtime import Context
    c = Context(0)
    yield c
    c.close()


def _root(p):
    from minotaur_amd.runtime import WarmStart
    st, _, _, _, _, ows = oracle.dual_simplex_root(p)
    assert st == 0
    return WarmStart(ows.head, ows.st, ows.d, np.ascontiguousarray(ows.binv.T)), ows


@pytest.fixture(scope='module')
def tls4():
    p = LinProblem.load(os.path.join(INST, 'tls4_oa.npz'))
    assert p.m == 64
    LB, UB = random_boxes(p, NBOX, 20261021)
    return (p, LB, UB) + _root(p)


def _path_both(ctx, p, LB, UB, k, path, st, ws, ows, cap, inherit):
    g, gk, gp, gs = ctx.lp_solve_path(LB, UB, ws, k, path, st, inherit)
    o = oracle.dual_simplex_path(p, LB, UB, ows, k, path, st, cap, inherit)
    assert np.array_equal(g.status, o[0])
    assert np.array_equal(g.iters, o[2])
    ok = o[0] == 0
    assert np.array_equal(g.obj[ok].view(np.int64), o[1][ok].view(np.int64))
    assert np.array_equal(g.x[ok].view(np.int64), o[3][ok].view(np.int64))
    assert np.array_equal(gk, o[4])
    for b in np.nonzero(gk > 0)[0]:
        assert np.array_equal(gp[b, :gk[b]], o[5][b, :gk[b]])
        assert np.array_equal(gs[b], o[6][b])
    return g, gk, gp, gs


def _children(p, LB, UB, x, status, k, path, st):
    """Both children of every optimal node on its first fractional integer
    column, each carrying its parent's final path."""
    ints = np.isin(p.vtype, (0, 1))
    cl, cu, ck, cp, cs = [], [], [], [], []
    for b in np.nonzero(status == 0)[0]:
        fr = np.nonzero(ints & (np.abs(x[b] - np.round(x[b])) > 1e-6))[0]
        if fr.size == 0:
            continue
        j, v = fr[0], x[b][fr[0]]
        for up in (0, 1):
            lo, hi = LB[b].copy(), UB[b].copy()
            if up:
                lo[j] = math.ceil(v)
            else:
                hi[j] = math.floor(v)
            cl.append(lo)
            cu.append(hi)
            ck.append(k[b])
            cp.append(path[b])
            cs.append(st[b])
    return np.array(cl), np.array(cu), np.array(ck), np.array(cp), np.array(cs)


@pytest.mark.parametrize('cap', [16, 32, 48])
def test_path_route_bits_at_every_eta_build(ctx, tls4, cap):
    p, LB, UB, ws, ows = tls4
    ctx.load(p)
    inherit = min(cap, PATH_INHERIT)
    ctx.set_lp_pfi(cap)
    try:
        assert ctx.oracle_pfi() == cap
        N = p.n + p.m
        g, gk, gp, gs = _path_both(ctx, p, LB, UB, np.zeros(NBOX, np.int32),
                                   np.zeros((NBOX, PATH_MAX), np.uint32),
                                   np.zeros((NBOX, N), np.int8), ws, ows, cap, inherit)
        assert (g.iters >= 2).any()          # BTRAN ran against a nonempty eta file
        CL, CU, CK, CP, CS = _children(p, LB, UB, g.x, g.status, gk, gp, gs)
        assert CL.shape[0] > 0 and (CK > 0).any()
        _path_both(ctx, p, CL, CU, CK, CP, CS, ws, ows, cap, inherit)
    finally:
        ctx.set_lp_pfi(LP_PFI_MAX)


def test_dense_k3_on_shared_warm_start(ctx, tls4):
    p, LB, UB, ws, ows = tls4
    ctx.load(p)
    ctx.set_lp_variant(1)
    try:
        assert ctx.oracle_pfi() == 0
        r = ctx.lp_solve(LB, UB, ws)
    finally:
        ctx.set_lp_variant(0)
    st, obj, its, _ = oracle.dual_simplex(p, LB, UB, ows)
    assert np.array_equal(r.status, st) and np.array_equal(r.iters, its)
    ok = st == 0
    assert ok.any() and (its >= 2).any()
    assert np.all(np.abs(r.obj[ok] - obj[ok]) <= 1e-9 * np.maximum(1.0, np.abs(obj[ok])))


def _product_form(ctx, p, LB, UB, ws, ows, cap):
    ctx.set_lp_variant(3)
    try:
        assert ctx.oracle_pfi() == cap
        r = ctx.lp_solve(LB, UB, ws, want_x=True)
    finally:
        ctx.set_lp_variant(0)
    st, obj, its, x = oracle.dual_simplex(p, LB, UB, ows, pfi=cap, want_x=True)
    assert np.array_equal(r.status, st) and np.array_equal(r.iters, its)
    ok = st == 0
    assert ok.any() and (its >= 2).any()
    assert np.array_equal(r.obj[ok], obj[ok])
    assert np.allclose(r.x[ok], x[ok], rtol=1e-9, atol=1e-9)


def test_product_form_partly_filled_row(ctx):
    p = knapsack_oa(f=16, N=48)
    assert 48 < p.m <= 64                  # K3P, the fourth row of lanes partly used
    ctx.load(p)
    LB, UB = random_boxes(p, 64, 20261022)
    ws, ows = _root(p)
    _product_form(ctx, p, LB, UB, ws, ows, LP_PFI_MAX)


def test_k3pw_and_k3l(ctx):
    p = knapsack_oa(f=17, N=64)
    assert 64 < p.m <= 128                 # two basis rows per lane: K3PW
    ctx.load(p)
    LB, UB = random_boxes(p, 64, 20261023)
    ws, ows = _root(p)
    _product_form(ctx, p, LB, UB, ws, ows, LP_PFI_WIDE_MAX)
    ctx.set_lp_variant(2)                  # K3L, dense, on the same boxes
    try:
        r = ctx.lp_solve(LB, UB, ws)
    finally:
        ctx.set_lp_variant(0)
    st, obj, its, _ = oracle.dual_simplex(p, LB, UB, ows)
    assert np.array_equal(r.status, st) and np.array_equal(r.iters, its)
    ok = st == 0
    assert np.all(np.abs(r.obj[ok] - obj[ok]) <= 1e-9 * np.maximum(1.0, np.abs(obj[ok])))
