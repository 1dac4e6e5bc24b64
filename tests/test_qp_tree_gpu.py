"""GPU: branch-and-bound over QP relaxations (the batched tree with K5 as its
node relaxation, mgpu_bnb_relaxation 1 — QPDRelaxer + BqpdEngine batched,
examples/QPDRelaxer.cpp:56-126), held round for round to its restatement
(oracle/bnb.py, CpuBnbContext with bnb_relaxation 1) and to brute force.

Bar: on the MIQPs of tests/qp_tree_cases.py (binaries, general integers,
trees of 7 to 501 nodes, a third of them settled by the phase-1 LP) the
engine's tree and the restatement agree after every round in rounds, nodes,
decision counts, pruned and open nodes and counted node solves, at orders 0
and 1 and batches 1, 3 and 16, from a start incumbent, and under every
clean-row mode with K1's persistent kernel forced (the one that takes the
masks); the incumbent agrees within 1e-6 and is the brute-force
optimum; K5's iterations per round stay within ITER_DIFF_MEASURED + 1 per
solved node of the restatement's.  tests/test_qp_tree_cpu.py shows that every
decision of these trees is at least MARGIN_FLOOR from its threshold, so
rounding differences between K5 and numpy cannot move one.  The reference's
order (order 2) has no restatement: there the optimum and the consistency of
the counts are pinned.  K5 alone is held to the restatement on the trees' own
node boxes (mostly fixed columns, FBBT-narrowed widths).  A feasible node QP
that K5 does not solve ends the round with MGPU_ERR_ENGINE.

Measured on an MI355X (2026-10-21): max |x_K5 - x_restatement| over the
status-0 node boxes of every case = X_DIFF_MEASURED (tests/qp_tree_cases.py);
the largest difference of a round's K5 iterations from the restatement's: see
test_parity.

BQPD is absent, so node-QP iterates stay "parity unpinned" against the
reference; the tree is pinned to the project's own restatement
and to brute force.
"""
import ctypes
import math
import os

import numpy as np
import pytest

import qp_ipm
import qp_tree_cases as tc
from minotaur_amd import qp as qpm
from minotaur_amd import runtime
from test_qp_shapes_gpu import ITER_DIFF_MEASURED

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
CAP = 1 << 14


@pytest.fixture(scope='module')
def ctx():
    c = runtime.Context(0)
    yield c
    c.close()


def _ids(params):
    return ['-'.join(tc.case_id(v) if isinstance(v, tuple) else str(v) for v in p)
            for p in params]


def engine_tree(ctx, P, order, batch, incumbent=math.inf, carry=3, max_rounds=10**9,
                rows=None):
    """The engine's tree over P's QP relaxations: ([stats_row per round],
    (incumbent, x)).  rows: the loaded LinProblem (default: P's rows with a
    zero objective)."""
    l, u = P.l, P.u
    ctx.load(qpm.rows_problem(P) if rows is None else rows)
    ctx.load_qp(P)
    ctx.bnb_relaxation(1)
    ctx.bnb_fbbt_carry(carry)
    try:
        ctx.bnb_config(order, 0)
        ctx.bnb_brancher(0)
        ctx.bnb_growth(0)
        ctx.bnb_init(CAP, l, u, incumbent)
        log = []
        for _ in range(max_rounds):
            st = ctx.bnb_round(batch)
            log.append(tc.stats_row(st))
            if st.open == 0:
                break
        return log, ctx.bnb_best()
    finally:
        ctx.bnb_relaxation(0)
        ctx.bnb_fbbt_carry(3)


def assert_parity(glog, clog, what):
    """Round by round: counts equal, incumbents within 1e-6, K5's iterations
    within (ITER_DIFF_MEASURED + 1) per node the interior point solved in the
    round (clog's last entry; a node the phase-1 LP settled takes the
    iteration limit on both sides, an empty box none).  Returns the largest
    difference of a round's iterations."""
    assert len(glog) == len(clog), (what, len(glog), len(clog), glog[-1], clog[-1])
    worst = 0
    gp = cp = (0, 0, (0,) * 5, 0, 0, 0, 0, math.inf, 0)
    for r, (g, c) in enumerate(zip(glog, clog)):
        assert g[:6] == c[:6], (what, 'round', r, g, c)
        if math.isinf(c[7]):
            assert g[7] == c[7], (what, r)
        else:
            assert abs(g[7] - c[7]) <= 1e-6 * max(1.0, abs(c[7])), (what, r, g[7], c[7])
        d = abs((g[6] - gp[6]) - (c[6] - cp[6]))
        assert d <= (ITER_DIFF_MEASURED + 1) * (c[8] - cp[8]), (what, 'round', r, g, c)
        worst = max(worst, d)
        gp, cp = g, c
    return worst


def assert_final_point(P, inc, x):
    ints = np.isin(P.vtype, (0, 1))
    assert np.all(np.abs(x[ints] - np.round(x[ints])) <= 1e-6)
    assert np.max(np.abs(P.A @ x - P.b)) <= 1e-7
    tol = 1e-9 * (1.0 + np.abs(P.u))
    assert np.all(x >= P.l - tol) and np.all(x <= P.u + tol)
    f = 0.5 * x @ P.Q @ x + P.c @ x + P.k
    assert abs(f - inc) <= 1e-9 * max(1.0, abs(inc)), (f, inc)


# ---- a. the existing bar: the optimum of brute force --------------------------
@pytest.mark.parametrize('seed', range(4))
def test_qp_tree_proves_brute_force_optimum(ctx, seed):
    case = (8, 0, 4, 2, seed)
    P = qpm.random_miqp(seed)
    opt = tc.brute_force(case)
    assert math.isfinite(opt) and abs(opt - tc.OPTIMA[case]) <= 1e-8 * max(1.0, abs(opt))
    for batch in (1, 16, 256):
        obj, x, st, _ = qpm.solve_tree(ctx, P, batch=batch, capacity=CAP)
        assert st.open == 0 and st.ndec[4] == 0
        assert abs(obj - opt) <= 1e-6 * max(1.0, abs(opt)), (batch, obj, opt)
        assert_final_point(P, obj, x)


def test_infeasible_node_qps(ctx):
    """Binary assignments whose rows cannot be met: K5 alone stops at its
    iteration limit (status 6, no certificate from the interior point);
    inside the tree the phase-1 LP over the node box settles them as
    infeasible (the trees below run through such nodes)."""
    P = qpm.random_miqp(1)
    ctx.load_qp(P)
    boxes = list(tc.assignments(P))
    bad = [(l, u) for l, u, ok in boxes if not ok][:16]
    good = [(l, u) for l, u, ok in boxes if ok][:16]
    assert bad and good
    LB = np.array([l for l, _ in bad + good])
    UB = np.array([u for _, u in bad + good])
    st, ob, it, _ = ctx.qp_solve(LB, UB)
    assert np.all(st[:len(bad)] == 6) and np.all(it[:len(bad)] == qp_ipm.MAXIT)
    assert np.all(st[len(bad):] == 0)
    ref = [qp_ipm.solve_node(P.Q, P.c, P.A, P.b, l, u)['obj'] + P.k for l, u in good]
    assert np.allclose(ob[len(bad):], ref, rtol=1e-6, atol=1e-6)


def test_color_lab2_tree_rounds(ctx):
    """The config-4 instance as a tree: rounds of node QPs with K1 presolve
    and MaxVio branching; every evaluated node ends with a decision, none
    with an engine problem."""
    P = tc.case_problem('color_lab2')
    obj, x, st, _ = qpm.solve_tree(ctx, P, batch=256, capacity=1 << 16, max_rounds=6)
    assert st.nodes > 0 and st.ndec[4] == 0
    assert st.lps > 0
    assert st.nodes == sum(st.ndec)


# ---- b. K5 on the trees' own node boxes ---------------------------------------
@pytest.mark.parametrize('case', tc.CASES, ids=[tc.case_id(c) for c in tc.CASES])
def test_k5_on_tree_boxes(ctx, case, capsys):
    """Every box the depth-first batch-16 tree of the restatement handed to the
    interior point, in one K5 batch: statuses (0 or 6) and iteration counts as
    the restatement's, objectives within 1e-6."""
    P = tc.problem(case)
    ref = tc.tree(case, 0, 16)[0].ipm
    LB = np.array([r['lb'] for r in ref])
    UB = np.array([r['ub'] for r in ref])
    ctx.load_qp(P)
    st, ob, it, x = ctx.qp_solve(LB, UB)
    rs = np.array([r['status'] for r in ref])
    ok = rs == 0
    xd = max((float(np.max(np.abs(x[b] - r['x']))) for b, r in enumerate(ref) if ok[b]),
             default=0.0)
    itd = max((abs(int(it[b]) - r['iters']) for b, r in enumerate(ref)), default=0)
    with capsys.disabled():
        print(f'\n{tc.case_id(case)}: {len(ref)} boxes, {int(ok.sum())} solved, '
              f'max |x_K5 - x_ref| = {xd:.3e}, max |it_K5 - it_ref| = {itd}')
    assert set(rs) <= {0, 6} and np.array_equal(st, rs)
    fr = np.array([r['obj'] for r in ref])
    assert np.all(np.abs(ob[ok] - fr[ok]) <= 1e-6 * np.maximum(1.0, np.abs(fr[ok])))
    assert itd <= ITER_DIFF_MEASURED + 1
    assert np.all(it[~ok] == qp_ipm.MAXIT)
    # MARGIN_FLOOR is a hundred times the largest of these differences as
    # measured: another order of K5's sums may move it, but not near the floor
    assert xd <= tc.MARGIN_FLOOR / 10


# ---- c. round-for-round parity ------------------------------------------------
_PARITY = ([(c, o, b) for c in tc.CASES for o in tc.ORDERS for b in (3, 16)]
           + [(c, o, 1) for c in tc.SMALL for o in tc.ORDERS])


@pytest.mark.parametrize('case,order,batch', _PARITY, ids=_ids(_PARITY))
def test_parity(ctx, case, order, batch, capsys):
    """The engine's tree against the restatement's after every round.
    Measured on an MI355X: the largest difference of a round's K5 iterations
    from the restatement's over all of these trees was 0."""
    P = tc.problem(case)
    cpu, clog = tc.tree(case, order, batch)
    glog, (inc, x) = engine_tree(ctx, P, order, batch)
    worst = assert_parity(glog, clog, (case, order, batch))
    with capsys.disabled():
        print(f'\n{tc.case_id(case)} order {order} batch {batch}: {clog[-1][1]} nodes in '
              f'{clog[-1][0]} rounds, largest iteration difference of a round {worst}')
    opt = tc.OPTIMA[case]
    assert glog[-1][4] == 0 and glog[-1][2][4] == 0
    assert abs(inc - opt) <= 1e-6 * max(1.0, abs(opt))
    assert_final_point(P, inc, x)


_INC = [(c, o) for c in tc.INC_CASES for o in tc.ORDERS]


@pytest.mark.parametrize('case,order', _INC, ids=_ids(_INC))
def test_parity_from_a_start_incumbent(ctx, case, order):
    """A start incumbent just above the optimum: K1 must not take it as an
    objective cut-off (the rows problem's objective is zero), the pool and
    the node decision prune by it."""
    P = tc.problem(case)
    opt = tc.OPTIMA[case]
    cpu, clog = tc.tree(case, order, 3, opt + tc.START_ABOVE)
    glog, (inc, x) = engine_tree(ctx, P, order, 3, incumbent=opt + tc.START_ABOVE)
    assert_parity(glog, clog, (case, order))
    assert clog != tc.tree(case, order, 3)[1]      # it pruned
    assert abs(inc - opt) <= 1e-6 * max(1.0, abs(opt))
    assert_final_point(P, inc, x)


@pytest.fixture(params=[0, 3], ids=['k1-auto', 'k1-persistent'])
def k1(ctx, request, monkeypatch):
    """K1 as the tree chooses it (at these batch sizes K1G, which takes no
    masks and answers "all rows"), or its persistent kernel on two waves
    forced: the kernel that takes the clean-row masks, the node order and the
    clean columns."""
    if request.param:
        monkeypatch.setenv('MGPU_FBBT_WAVES', '2')
    ctx.set_fbbt_variant(request.param)
    yield ctx
    ctx.set_fbbt_variant(0)
    ctx.bnb_fbbt_carry(3)


# (12, 0, 4, 3, 0) and (10, 0, 3, 3, 0) at batch 256: rounds of up to 226 and
# 112 nodes, past the 64 from which mode 2 groups a round's nodes
_CARRY = [((10, 0, 3, 3, 2), 16), ((12, 0, 4, 3, 1), 16), ((8, 2, 4, 3, 6), 16),
          ((12, 0, 4, 3, 0), 256), ((10, 0, 3, 3, 0), 256)]


@pytest.mark.parametrize('case,batch', _CARRY, ids=_ids(_CARRY))
def test_clean_row_modes_change_nothing(k1, case, batch):
    """mgpu_bnb_fbbt_carry 0 to 3 (off, clean-row masks, nodes grouped by
    branching variable in rounds above 64 nodes, clean columns): the same
    statistics and the same incumbent bits in every mode, and the rounds of
    the restatement.  Only under the persistent K1 kernel do the modes run
    different code; under the automatic choice they must agree all the more."""
    P = tc.problem(case)
    cpu, clog = tc.tree(case, 0, batch)
    if batch > 16:
        assert cpu.max_batch > 64
        for k, v in cpu.margins.items():      # (the CPU test has batches 1 to 16)
            assert v >= tc.MARGIN_FLOOR, (k, v)
    runs = [engine_tree(k1, P, 0, batch, carry=mode) for mode in (0, 1, 2, 3)]
    for log, (inc, x) in runs[1:]:
        assert log == runs[0][0]
        assert inc == runs[0][1][0] and np.array_equal(x, runs[0][1][1])
    assert_parity(runs[3][0], clog, (case, batch))
    assert abs(runs[3][1][0] - tc.OPTIMA[case]) <= 1e-6 * max(1.0, abs(tc.OPTIMA[case]))


@pytest.mark.parametrize('order', tc.ORDERS)
def test_rows_objective_is_not_propagated(k1, order):
    """include/mgpu.h: the loaded LP supplies the rows for K1 "without
    objective propagation: the objective is quadratic".  K1 skips an objective
    without nonzeros by itself (and one whose smallest value already exceeds
    the incumbent), so the rows here carry an objective that would bite:
    -4 x_j for a binary j that is 0 at the optimum.  Against an incumbent of
    -2.9 (found in the tree, or given at the start) K1's objective cut
    -4 x_j <= -2.9 would fix x_j = 1 and cut the optimum off; the tree must
    take the rounds of the restatement instead, under either K1 kernel."""
    import dataclasses
    case = (8, 0, 4, 2, 0)
    P = tc.problem(case)
    assert tc.OPTIMA[case] < -2.9
    xopt = tc.tree(case, order, 3)[0].best_x
    j = next(k for k in range(P.n) if P.vtype[k] == 0 and xopt[k] < 0.5)
    obj = np.zeros(P.n)
    obj[j] = -4.0
    rows = dataclasses.replace(qpm.rows_problem(P), obj=obj)
    for inc in (math.inf, tc.OPTIMA[case] + tc.START_ABOVE):
        glog, (best, x) = engine_tree(k1, P, order, 3, incumbent=inc, rows=rows)
        assert_parity(glog, tc.tree(case, order, 3, inc)[1], (case, order, inc))
        assert abs(best - tc.OPTIMA[case]) <= 1e-6 * abs(best) and x[j] < 0.5
        assert_final_point(P, best, x)


_ORDER2 = [(c, b) for c in tc.CASES for b in (16, 1)]


@pytest.mark.parametrize('case,batch', _ORDER2, ids=_ids(_ORDER2))
def test_reference_order(ctx, case, batch):
    """Order 2 (the reference's node heap) has no restatement with a QP
    relaxation: the optimum of brute force and consistent counts."""
    P = tc.problem(case)
    log, (inc, x) = engine_tree(ctx, P, 2, batch)
    opt = tc.OPTIMA[case]
    rounds, nodes, ndec, pruned, open_, lps, pivots, _ = log[-1]
    assert open_ == 0 and nodes == sum(ndec) and ndec[4] == 0
    assert lps <= nodes and ndec[3] >= 1
    assert abs(inc - opt) <= 1e-6 * max(1.0, abs(opt))
    assert_final_point(P, inc, x)


def test_color_lab2_dive(ctx, capsys):
    """color_lab2 (n = 300, m = 61: the n > 64 column loops of the children
    writer, K5 at np = 304): a 12-round dive at batch 1 against the
    restatement.  (At batch 8 this symmetric instance has MaxVio scores 5.5e-13
    apart: no parity there.)"""
    P = tc.case_problem('color_lab2')
    cpu, clog = tc.tree('color_lab2', 0, 1, math.inf, 12)
    for k, v in cpu.margins.items():
        assert v >= tc.MARGIN_FLOOR, (k, v)
    glog, _ = engine_tree(ctx, P, 0, 1, max_rounds=12)
    worst = assert_parity(glog, clog, 'color_lab2')
    with capsys.disabled():
        print(f'\ncolor_lab2 dive: largest iteration difference of a round {worst}')


# ---- d. a feasible node QP that K5 does not solve -------------------------------
def _engine_problems():
    P = tc.ill_conditioned(*tc.ENGINE_DRAW)
    yield 'ill-conditioned', P, P.l, P.u
    yield ('stalled',) + tc.stalled_box()


@pytest.mark.parametrize('which', ['ill-conditioned', 'stalled'])
def test_engine_problem_ends_the_round(ctx, which):
    """Feasible rows (HiGHS), K5 at status 6 on the root box: the phase-1 LP
    finds the rows feasible, so the node is an engine problem (status 12,
    decision 4): mgpu_bnb_round fills the statistics and returns
    MGPU_ERR_ENGINE, the node neither infeasible nor branched; the context
    runs a normal tree afterwards.

    'ill-conditioned': ENGINE_DRAW of tests/qp_tree_cases.py, Q with a
    spectrum spanning 10^14.  'stalled': a well-conditioned node QP on which
    the interior point stalls (STALLED)."""
    _, P, l, u = next(e for e in _engine_problems() if e[0] == which)
    assert tc.rows_feasible(P, l, u)
    ctx.load_qp(P)
    st, _, it, _ = ctx.qp_solve(l[None], u[None])
    assert st[0] == 6 and it[0] == qp_ipm.MAXIT
    ctx.load(qpm.rows_problem(P))
    ctx.load_qp(P)
    ctx.bnb_relaxation(1)
    try:
        ctx.bnb_config(0, 0)
        ctx.bnb_brancher(0)
        ctx.bnb_growth(0)
        ctx.bnb_init(64, l, u)
        s = runtime.BnbStats()
        rc = ctx.lib.mgpu_bnb_round(ctx.h, 1, ctypes.c_double(math.inf), ctypes.byref(s))
        assert rc == -5                                   # MGPU_ERR_ENGINE
        assert b'unknown status' in ctx.lib.mgpu_last_error(ctx.h)
        assert tuple(s.ndec) == (0, 0, 0, 0, 1)
        assert (s.rounds, s.nodes, s.open, s.last_batch) == (1, 1, 0, 1)
        assert (s.lps, s.pivots, s.pruned) == (0, 0, 0) and s.incumbent == math.inf
        assert np.all(np.isnan(ctx.bnb_best()[1]))
        ctx.bnb_init(64, l, u)
        with pytest.raises(runtime.MgpuError, match='rc=-5'):
            ctx.bnb_round(1)
    finally:
        ctx.bnb_relaxation(0)
    case = tc.CASES[0]
    glog, (inc, x) = engine_tree(ctx, tc.problem(case), 0, 3)
    assert_parity(glog, tc.tree(case, 0, 3)[1], 'after the engine problem')
