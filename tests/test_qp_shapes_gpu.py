"""GPU: K5 (minotaur_amd/csrc/qp_kkt.hip) on every kernel variant and tile
edge, with a different box per node of a batch.

tests/qp_cases.py has one shape per variant of the launch plan (left- /
right-looking factor, W in LDS / in HBM, qp_step<2|4|8>), n and m on and
next to multiples of 16, m = 0 and m = 64; mgpu_qp_plan pins which kernels
each shape ran, so a moved threshold cannot drop the coverage unnoticed.
K5's answers are held against the restatement (oracle/qp_ipm.py, certified
by tests/test_qp_shapes_cpu.py), against the multiplier-free Wolfe bound
(test_qp_cpu.dual_bound) and, for the LPs, against HiGHS.  Further: a
node's result does not depend on its batch (bit for bit), on the workspace's
history or on what was loaded before; maxit; a non-symmetric Q; the size
limit of mgpu_load_qp."""
import numpy as np
import pytest

import qp_cases
from minotaur_amd import qp as qpm
from minotaur_amd import runtime

pytestmark = pytest.mark.gpu

_ALL = qp_cases.SHAPES + qp_cases.FAMILY
# max |iters(K5) - iters(restatement)| over every node of _ALL, measured on an
# MI355X; test_iteration_counts allows one more (a rounding flip at the
# convergence threshold)
ITER_DIFF_MEASURED = 0


@pytest.fixture(scope='module')
def ctx():
    c = runtime.Context(0)
    yield c
    c.close()


def _problem(key):
    return (qp_cases.case(*key) if len(key) == 2 else qp_cases.family_case(*key))[:3]


_solved = {}


def _solve(ctx, key):
    """K5 on all nodes of a case in one batch (once per process)."""
    if key not in _solved:
        P, LB, UB = _problem(key)
        ctx.load_qp(P)
        plan = ctx.qp_plan()
        st, ob, it, x = ctx.qp_solve(LB, UB)
        _solved[key] = (plan, st, ob, it, x)
    return _solved[key]


def _bits(*arrays):
    return [np.ascontiguousarray(a).view(np.uint8).tobytes() for a in arrays]


def _check_solution(P, LB, UB, st, ob, x, ref, dual):
    from test_qp_cpu import assert_convex, dual_bound
    assert np.all(st == 0), st
    tol_rows = 1e-7 * (1.0 + np.max(np.abs(P.b), initial=0.0))
    if dual:
        assert_convex(P)
    for b in range(LB.shape[0]):
        tol_box = 1e-9 * (1.0 + np.max(np.abs(UB[b])))
        assert np.max(np.abs(P.A @ x[b] - P.b), initial=0.0) <= tol_rows, b
        assert np.all(x[b] >= LB[b] - tol_box) and np.all(x[b] <= UB[b] + tol_box), b
        f = qp_cases.objective(P, x[b])
        assert abs(ob[b] - f) <= 1e-9 * max(1.0, abs(f)), (b, ob[b], f)
        fr = ref[b]['obj'] + P.k
        assert abs(ob[b] - fr) <= 1e-6 * max(1.0, abs(fr)), (b, ob[b], fr)
        if dual:
            # optimal whatever the restatement says: f meets the Wolfe bound
            D = dual_bound(P, LB[b], UB[b], x[b]) + P.k
            tol = 1e-6 * max(1.0, abs(f))
            assert -tol <= f - D <= tol, (b, f, D)


# ---- a. every shape -----------------------------------------------------------
@pytest.mark.parametrize('n,m', qp_cases.SHAPES)
def test_shape(ctx, n, m):
    P, LB, UB, _ = qp_cases.case(n, m)
    plan, st, ob, it, x = _solve(ctx, (n, m))
    assert plan == qp_cases.PLANS[(n, m)]
    _check_solution(P, LB, UB, st, ob, x, qp_cases.reference((n, m)), dual=n <= 100)


@pytest.mark.parametrize('key', qp_cases.FAMILY, ids=lambda k: '-'.join(f'{v:g}' if isinstance(
    v, float) else str(v) for v in k))
def test_family(ctx, key):
    P, LB, UB = qp_cases.family_case(*key)
    plan, st, ob, it, x = _solve(ctx, key)
    assert plan == (1, 1, 2)
    _check_solution(P, LB, UB, st, ob, x, qp_cases.reference(key), dual=True)
    if key[0] == 'lp':
        f = qp_cases.highs_lp(P, LB[0], UB[0])
        assert abs(ob[0] - f) <= 1e-6 * max(1.0, abs(f))


# ---- b. iteration counts --------------------------------------------------------
def test_iteration_counts(ctx, capsys):
    """K5 follows the restatement step for step, so both take the same number
    of iterations up to a rounding flip at the convergence threshold.
    Measured on an MI355X over all 107 nodes (80 of the shapes, 27 of the
    families): max |it_gpu - it_ref| = 0, every node took exactly the
    restatement's count; the most iterations of any node were 12."""
    worst, where, itmax = 0, None, 0
    for key in _ALL:
        it = _solve(ctx, key)[3]
        ref = qp_cases.reference(key)
        itmax = max(itmax, int(it.max()))
        for b, r in enumerate(ref):
            d = abs(int(it[b]) - r['iters'])
            if d > worst:
                worst, where = d, (key, b, int(it[b]), r['iters'])
    with capsys.disabled():
        print(f'\nK5 iteration counts: max |it_gpu - it_ref| = {worst} at {where}; '
              f'max it_gpu = {itmax}')
    assert itmax < 80
    assert worst <= ITER_DIFF_MEASURED + 1, where


# ---- c. a node's result does not depend on its batch ----------------------------
@pytest.mark.parametrize('n,m', [(33, 17), (305, 49), (1121, 5)])
def test_batch_isolation(ctx, n, m):
    P, LB, UB, x0 = qp_cases.case(n, m)
    empty_l, empty_u = P.l.copy(), P.u.copy()
    empty_l[n // 2], empty_u[n // 2] = 0.75, 0.25          # one l > u
    L = np.stack([LB[0], empty_l, LB[1], x0 + 0.1, LB[2], x0, LB[3]])
    U = np.stack([UB[0], empty_u, UB[1], x0 + 0.1, UB[2], x0, UB[3]])
    good = [0, 2, 4, 6]
    ctx.load_qp(P)
    st, ob, it, x = ctx.qp_solve(L, U)
    assert list(st) == [0, 2, 0, 6, 0, 0, 0]
    assert ob[1] == np.inf
    # every column fixed at x0: converged before any step, at f(x0).  K5 sums
    # the n^2 + n terms of f in another order than numpy: each sum is off by
    # at most n eps times the sum of its terms' magnitudes
    assert it[5] == 0 and np.array_equal(x[5], x0)
    mag = 0.5 * np.abs(x0) @ np.abs(P.Q) @ np.abs(x0) + np.abs(P.c) @ np.abs(x0)
    assert abs(ob[5] - qp_cases.objective(P, x0)) <= 4 * n * np.finfo(float).eps * mag
    # the four good nodes are the case's own: same bits as in their batch of four
    alone4 = _solve(ctx, (n, m))
    ctx.load_qp(P)
    assert _bits(st[good], ob[good], it[good], x[good]) == _bits(*alone4[1:])
    for k, b in enumerate(good):
        s1, o1, i1, x1 = ctx.qp_solve(L[b:b + 1], U[b:b + 1])
        assert _bits(s1, o1, i1, x1) == _bits(st[b:b + 1], ob[b:b + 1], it[b:b + 1],
                                              x[b:b + 1]), (k, s1, i1, o1, ob[b])


# ---- d. workspace growth and reload ---------------------------------------------
def test_workspace_growth_keeps_results(ctx):
    P, LB, UB, _ = qp_cases.case(33, 17)
    c = runtime.Context(0)      # a fresh context: its first batch sizes the workspace
    try:
        c.load_qp(P)
        first = c.qp_solve(LB[:2], UB[:2])
        big = c.qp_solve(np.tile(LB, (10, 1)), np.tile(UB, (10, 1)))
        again = c.qp_solve(LB[:2], UB[:2])
    finally:
        c.close()
    assert np.all(first[0] == 0) and np.all(big[0] == 0)
    assert _bits(*first) == _bits(*again)
    assert _bits(*first) == _bits(*(a[:2] for a in big))


def test_reload_keeps_results(ctx):
    big, small = qp_cases.case(305, 49), qp_cases.case(33, 17)
    out = []
    for P, LB, UB, _ in (big, small, big, small):
        ctx.load_qp(P)
        out.append(ctx.qp_solve(LB, UB))
    assert np.all(out[0][0] == 0) and np.all(out[1][0] == 0)
    assert _bits(*out[0]) == _bits(*out[2])
    assert _bits(*out[1]) == _bits(*out[3])


# ---- e. maxit --------------------------------------------------------------------
def test_maxit(ctx):
    # a node whose k - 1 and k + 2 are both no multiple of 4, the period of
    # the host loop's convergence read-back
    pick = None
    for key in [(33, 17), (17, 16), (65, 64), (80, 64), (16, 15)]:
        for b, r in enumerate(qp_cases.reference(key)):
            if pick is None and r['iters'] % 4 in (0, 3) and r['iters'] >= 4:
                pick = (key, b, r['iters'])
    assert pick is not None
    key, b, k = pick
    P, LB, UB, _ = qp_cases.case(*key)
    ctx.load_qp(P)
    lb, ub = LB[b:b + 1], UB[b:b + 1]
    default = ctx.qp_solve(lb, ub)
    assert default[0][0] == 0 and default[2][0] == k
    short = ctx.qp_solve(lb, ub, maxit=k - 1)
    assert short[0][0] == 6 and short[2][0] == k - 1
    enough = ctx.qp_solve(lb, ub, maxit=k + 2)
    assert _bits(*enough) == _bits(*default)


# ---- f. a non-symmetric Q ----------------------------------------------------------
def test_nonsymmetric_q_is_symmetrised(ctx):
    P, LB, UB, _ = qp_cases.case(33, 17)
    st, ob = _solve(ctx, (33, 17))[1:3]
    R = np.random.default_rng(5).normal(size=(33, 33))
    S = 0.5 * (R - R.T)
    P2 = qpm.QpProblem('skew', P.Q + S, P.c, P.k, P.A, P.b, P.l, P.u, P.vtype)
    ctx.load_qp(P2)
    st2, ob2, _, _ = ctx.qp_solve(LB, UB)
    assert np.all(st == 0) and np.all(st2 == 0)
    assert np.all(np.abs(ob2 - ob) <= 1e-12 * np.maximum(1.0, np.abs(ob))), (ob, ob2)


# ---- g. the size limit -------------------------------------------------------------
def test_size_limit(ctx):
    assert runtime.QP_MAX_N == 1248 and max(n for n, _ in qp_cases.SHAPES) == runtime.QP_MAX_N
    P, LB, UB, _ = qp_cases.case(33, 17)
    ctx.load_qp(P)
    before = ctx.qp_solve(LB, UB)
    n = runtime.QP_MAX_N + 1
    big = qpm.QpProblem('big', np.eye(n), np.zeros(n), 0.0, np.zeros((1, n)), np.zeros(1),
                        np.zeros(n), np.ones(n), np.full(n, 4, dtype=np.int32))
    with pytest.raises(runtime.MgpuError, match=r'rc=-1: .*n <= 1248 columns, m <= 64 rows'):
        ctx.load_qp(big)
    # refused before anything was touched: the loaded QP is still there
    assert ctx.qp_plan() == (1, 1, 2)
    assert _bits(*ctx.qp_solve(LB, UB)) == _bits(*before)
    # the largest accepted shape loads (its solve: test_shape[1248-1])
    ctx.load_qp(qp_cases.case(runtime.QP_MAX_N, 1)[0])
    assert ctx.qp_plan() == (0, 0, 8)
