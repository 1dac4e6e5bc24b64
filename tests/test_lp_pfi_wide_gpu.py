"""GPU parity of K3PW (repo:minotaur_amd/csrc/lp_pfi_wide.hip): the
product-form dual simplex of K3P for relaxations with 64 < m <= 128 rows,
through the C ABI.

K3PW restates oracle/lp_dual.c's product-form mode (``pfi=k``: B^{-1} kept as
k eta columns on the shared root inverse); an LP that needs more than k
pivots stops and K3L continues it from its basis and explicit inverse, as the
oracle's two-stage solve does.  Statuses and pivot counts equal the oracle's,
objectives are summed in the oracle's order (bit-equal), HiGHS within the
north-star 1e-6.  Instances: the knapsack outer-approximation LPs of the
convex batch (config 5; f = 17 / 24 / 28 terms -> m = 69 / 97 / 113).
"""
import os
import sys

import numpy as np
import pytest

import oracle
from minotaur_amd.problem import knapsack_oa, random_boxes, random_problem
from minotaur_amd.runtime import LP_PFI_WIDE_MAX as WCAP

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, '..', 'oracle'))


@pytest.fixture(scope='module')
def ctx():
    from minotaur_amd.runtime import Context
    c = Context(0)
    yield c
    c.close()


class k3pw:
    """LP calls inside run on the product form (variant 3) with a K3PW eta
    cap of kmax; auto mode and the default cap afterwards."""

    def __init__(self, ctx, kmax=WCAP):
        self.ctx, self.kmax = ctx, kmax

    def __enter__(self):
        self.ctx.set_lp_variant(3)
        self.ctx.set_lp_pfi_wide(self.kmax)

    def __exit__(self, *a):
        self.ctx.set_lp_variant(0)
        self.ctx.set_lp_pfi_wide(WCAP)


def _root(p):
    from minotaur_amd.runtime import WarmStart
    st, _, _, _, _, ows = oracle.dual_simplex_root(p)
    assert st == 0
    ws = WarmStart(ows.head, ows.st, ows.d, np.ascontiguousarray(ows.binv.T))
    return ws, ows


def _check(ctx, p, LB, UB, kmax, iter_limit=0, want_x=False):
    ws, ows = _root(p)
    with k3pw(ctx, kmax):
        assert ctx.oracle_pfi() == kmax
        r = ctx.lp_solve(LB, UB, ws, iter_limit=iter_limit, want_x=want_x)
    st, obj, its, x = oracle.dual_simplex(p, LB, UB, ows, nthreads=8, pfi=kmax,
                                          iter_limit=iter_limit or 10000, want_x=want_x)
    assert np.array_equal(r.status, st)
    assert np.array_equal(r.iters, its)
    ok = st == 0
    assert np.array_equal(r.obj[ok], obj[ok])      # sequential sum: the oracle's bits
    if want_x:
        assert np.allclose(r.x[ok], x[ok], rtol=1e-9, atol=1e-9)
    return r, its


@pytest.mark.parametrize('f', [17, 24, 28])
def test_k3pw_is_auto_choice(ctx, f):
    p = knapsack_oa(f=f, N=max(64, 3 * f))
    assert 64 < p.m <= 128
    ctx.load(p)
    assert ctx.oracle_pfi() == WCAP


@pytest.mark.parametrize('f,kmax', [(24, WCAP), (28, WCAP), (28, 12), (17, 4)])
def test_k3pw_node_boxes_vs_oracle(ctx, f, kmax):
    """Random-branching boxes; the small caps send most LPs through the
    overflow list into K3L (continuation slots)."""
    p = knapsack_oa(f=f, N=max(64, 3 * f))
    ctx.load(p)
    LB, UB = random_boxes(p, 3001, 20261017 + f)
    r, its = _check(ctx, p, LB, UB, kmax, want_x=True)
    if kmax < 20:
        assert (its > kmax).any()   # the continuation ran
    for b in np.nonzero(r.status == 0)[0][:24]:
        hs, ho = oracle.highs(p, LB[b], UB[b])
        assert hs == 0 and abs(ho - r.obj[b]) <= 1e-6 * max(1.0, abs(ho))


def test_k3pw_four_column_slots_vs_oracle(ctx):
    """S = 4 column slots per lane (193 <= n + m <= 256): the knapsack OA
    shapes above give S = 2 and 3 only.  The smallest shape that selects it
    (m = 65, n = 128); most of its LPs overflow into K3L."""
    p = random_problem(1, n=128, m=65, density=min(0.15, 4.0 / 65))
    assert 64 < p.m <= 128 and (p.n + p.m + 63) // 64 == 4
    ctx.load(p)
    LB, UB = random_boxes(p, 300, 1)
    _check(ctx, p, LB, UB, WCAP, want_x=True)


def test_k3pw_iteration_limit(ctx):
    p = knapsack_oa(f=24, N=72)
    ctx.load(p)
    LB, UB = random_boxes(p, 777, 5)
    _check(ctx, p, LB, UB, WCAP, iter_limit=7)
    _check(ctx, p, LB, UB, 6, iter_limit=20)   # overflow, then the limit in K3L


def test_k3pw_skip_and_empty_box(ctx):
    p = knapsack_oa(f=24, N=72)
    ctx.load(p)
    LB, UB = random_boxes(p, 64, 11)
    LB[5, 3], UB[5, 3] = 9.0, 2.0     # empty box: infeasible before any pivot
    skip = (np.arange(64) % 7 == 0).astype(np.int32)
    ws, _ = _root(p)
    with k3pw(ctx):
        r = ctx.lp_solve(LB, UB, ws, skip=skip)
        full = ctx.lp_solve(LB, UB, ws)
    assert np.all(r.status[skip == 1] == 12) and np.all(np.isinf(r.obj[skip == 1]))
    assert np.array_equal(r.status[skip == 0], full.status[skip == 0])
    assert full.status[5] == 2 and full.iters[5] == 0


@pytest.mark.parametrize('kmax', [WCAP, 5])
def test_k3pw_bound_lps_vs_oracle(ctx, kmax):
    """Bound LPs (QuadHandler::tightenLP_ objectives +-x_j) on one box."""
    p = knapsack_oa(f=24, N=72)
    ctx.load(p)
    ws, ows = _root(p)
    cols = np.repeat(np.arange(p.n, dtype=np.int32), 2)
    signs = np.tile([1.0, -1.0], p.n)
    with k3pw(ctx, kmax):
        g = ctx.lp_bound(cols, signs, ws=ws, want_x=True)
    st, ob, it, xs = oracle.lp_bound(p, cols, signs, ws=ows, pfi=kmax)
    assert np.array_equal(g.status, st) and np.array_equal(g.iters, it)
    ok = st == 0
    assert np.allclose(g.obj[ok], ob[ok], rtol=1e-9, atol=1e-9)
    assert ok.any()
    # every LP, whatever its status: 23 of these 96 once came back as a false
    # "unbounded" from kernels and oracle alike
    for k in range(cols.size):
        c = np.zeros(p.n)
        c[cols[k]] = signs[k]
        hs, ho = oracle.highs_obj(p, c)
        assert hs in (0, 2, 4) and g.status[k] == hs
        if hs == 0:
            assert abs(ho - g.obj[k]) <= 1e-6 * max(1.0, abs(ho))


def test_k3pw_tree_matches_cpu_and_highs(ctx):
    """The batched tree's node LPs from the root basis run on K3PW (auto):
    the same tree as the CPU restatement in product-form mode (rounds, nodes,
    decisions), the same incumbent bits, the HiGHS MILP optimum."""
    from bnb import CpuBnbContext
    from minotaur_amd import bnb
    p = knapsack_oa(f=17, N=64)
    hs, hobj = oracle.highs_milp(p)
    ctx.load(p)
    assert ctx.oracle_pfi() == WCAP
    og, xg, sg, _ = bnb.solve(ctx, batch=512, capacity=1 << 17)
    oc, xc, sc, _ = bnb.solve(CpuBnbContext(p, WCAP), batch=512, capacity=1 << 17)
    assert sg.open == sc.open == 0
    assert (sg.rounds, sg.nodes, list(sg.ndec)) == (sc.rounds, sc.nodes, list(sc.ndec))
    assert og == oc
    assert hs == 0 and abs(og - hobj) <= 1e-6 * max(1.0, abs(hobj))
