"""CPU: the restatement of K5's coupled step and of the retry pass
(tests/qp_retry_ref.py) on the cases of tests/qp_retry_cases.py, before
tests/test_qp_retry_gpu.py holds the engine to it.

The coupled step solves the six node QPs the separate step stalls on, to a
KKT certificate within the solver's own stopping tolerances and to a lower
objective than the stalled iterate's; where both rules converge they find the
same optimum; brute force with the retry values the seeds
tests/qp_tree_cases.py leaves out, and the trees with the retry prove it; the
retry trees finish without an engine problem, every one of them with a node
the retry solved, and every decision at least MARGIN_FLOOR from its
threshold."""
import math

import numpy as np
import pytest

import qp_ipm
import qp_retry_cases as rc
import qp_retry_ref as rr
import qp_tree_cases as tc

_box_ids = ['{}-{}'.format(tc.case_id(c), ''.join(map(str, v))) for c, v in rc.STALLED_BOXES]


def test_rule_0_is_the_oracle():
    """solve_node_rule is oracle/qp_ipm.py's solve_node with the rule as an
    argument: under rule 0 every output bit is solve_node's."""
    for case in (tc.CASES[0], (6, 3, 4, 2, 1)):
        for r in tc.tree(case, 0, 16)[0].ipm[:12]:
            P = tc.problem(case)
            with np.errstate(all='ignore'):
                a = qp_ipm.solve_node(P.Q, P.c, P.A, P.b, r['lb'], r['ub'])
                b = rr.solve_node_rule(P.Q, P.c, P.A, P.b, r['lb'], r['ub'], 0)
            assert (a['status'], a['iters'], a['obj']) == (b['status'], b['iters'], b['obj'])
            for k in ('x', 'y', 'zl', 'zu'):
                assert a[k].tobytes() == b[k].tobytes()


def test_stalled_is_among_the_boxes():
    assert tc.STALLED in rc.STALLED_BOXES


@pytest.mark.parametrize('case,vals', rc.STALLED_BOXES, ids=_box_ids)
def test_coupled_step_solves_the_stalled_boxes(case, vals, capsys):
    P, l, u = rc.box_of(case, vals)
    assert tc.rows_feasible(P, l, u)
    with np.errstate(all='ignore'):
        sep = qp_ipm.solve_node(P.Q, P.c, P.A, P.b, l, u)
    assert sep['status'] == 6
    r = rr.solve_node_coupled(P.Q, P.c, P.A, P.b, l, u)
    k = qp_ipm.kkt_certificate(P.Q, P.c, P.A, P.b, l, u, r['x'], r['y'], r['zl'], r['zu'])
    with capsys.disabled():
        print(f"\n{tc.case_id(case)} {vals}: {r['iters']} iterations, obj {r['obj']:.6f} "
              f"(separate: {sep['obj']:.6f}), rp {k['rp']:.1e} rd {k['rd']:.1e} gap {k['gap']:.1e}")
    assert r['status'] == 0 and 7 <= r['iters'] <= 21
    # the solver's own stopping test (qp_ipm.solve_node): scaled residuals, mu
    nf = int((l < u).sum())
    tp = max(qp_ipm.TOL_P * (1.0 + np.max(np.abs(P.b))),
             qp_ipm.TOL_P * (1.0 + np.max(np.abs(r['x']))))
    td = qp_ipm.TOL_D * (1.0 + np.max(np.abs(P.c)))
    assert k['rp'] <= tp and k['rd'] <= td and k['box'] == 0.0
    # gap = y'(Ax - b) + the complementarity sum (2 nf mu at the stop)
    assert abs(k['gap']) <= 2 * nf * qp_ipm.TOL_MU + np.sum(np.abs(r['y'])) * k['rp']
    assert k['zmin'] >= 0.0
    assert r['obj'] < sep['obj']


@pytest.mark.parametrize('case', [(10, 0, 3, 3, 1), (6, 3, 4, 2, 3)],
                         ids=[tc.case_id((10, 0, 3, 3, 1)), tc.case_id((6, 3, 4, 2, 3))])
def test_both_rules_find_the_same_optimum(case):
    """Where the separate step converges the coupled step converges too, on
    the same convex QP: objectives within 1e-8."""
    P = tc.problem(case)
    solved = [r for r in tc.tree(case, 0, 16)[0].ipm if r['status'] == 0]
    assert len(solved) >= 10
    for r in solved:
        c = rr.solve_node_coupled(P.Q, P.c, P.A, P.b, r['lb'], r['ub'])
        assert c['status'] == 0
        assert abs(c['obj'] + P.k - r['obj']) <= 1e-8 * max(1.0, abs(r['obj']))


@pytest.mark.parametrize('case', rc.LEFT_OUT, ids=[tc.case_id(c) for c in rc.LEFT_OUT])
def test_left_out_seeds(case):
    """Brute force with the retry values every row-feasible assignment, and
    the tree with the retry proves its optimum at every order and batch."""
    opt, nretry = rc.brute_force(case)
    assert abs(opt - rc.OPTIMA[case]) <= 1e-8 * max(1.0, abs(opt))
    assert nretry == rc.STALLED_ASSIGNMENTS.get(case, 0)
    P = tc.problem(case)
    ints = np.isin(P.vtype, (0, 1))
    for order in tc.ORDERS:
        for batch in tc.BATCHES:
            c, log = rc.tree(('full', case), order, batch)
            assert log[-1][4] == 0 and c.nstatus12 == 0 and log[-1][2][4] == 0, (order, batch)
            assert log[-1][1] == sum(log[-1][2])
            assert abs(c.inc - opt) <= 1e-6 * max(1.0, abs(opt)), (order, batch, c.inc, opt)
            x = c.best_x
            assert np.all(np.abs(x[ints] - np.round(x[ints])) <= 1e-6)
            assert np.max(np.abs(P.A @ x - P.b)) <= 1e-7
            for k, v in c.margins.items():
                assert v >= tc.MARGIN_FLOOR, (order, batch, k, v)


def test_left_out_seeds_are_the_left_out_seeds():
    assert not set(rc.LEFT_OUT) & set(tc.CASES)
    assert set(rc.LEFT_OUT) | set(tc.CASES) >= {(6, 3, 4, 2, s) for s in range(8)} \
        | {(8, 2, 4, 3, s) for s in range(8)}
    assert sum(c in rc.STALLED_ASSIGNMENTS for c in rc.LEFT_OUT) == 4


@pytest.mark.parametrize('spec,runs', rc.RETRY_TREES, ids=[rc.tree_id(s) for s, _ in rc.RETRY_TREES])
def test_retry_trees(spec, runs, capsys):
    """Every (order, batch) of the table meets a retried node, the others of
    the tree meet none; each retry tree finishes with no engine problem, its
    retried nodes solved, and its decisions at the margin."""
    for order in tc.ORDERS:
        for batch in tc.BATCHES:
            c, log = rc.tree(spec, order, batch)
            assert (c.nretried > 0) == ((order, batch) in runs), (order, batch, c.nretried)
            assert log[-1][4] == 0 and c.nstatus12 == 0 and log[-1][2][4] == 0
            if not c.nretried:
                continue
            assert c.nretry_solved == c.nretried >= 1
            assert all(r['status'] == 0 for r in c.retried)
            assert c.first_retry_round is not None
            for k, v in c.margins.items():
                assert v >= tc.MARGIN_FLOOR, (order, batch, k, v)
            with capsys.disabled():
                print(f'\n{rc.tree_id(spec)} order {order} batch {batch}: {log[-1][1]} nodes, '
                      f'{c.nretried} retried in round {c.first_retry_round}, smallest margin '
                      f'{min(c.margins.values()):.2e}')


def test_enough_retry_trees():
    """Conditions on the inputs: at least four trees with a retried node, one
    of them with more than 50 nodes."""
    trees = {spec for spec, _, _ in rc.RETRY_RUNS}
    assert len(trees) >= 4
    assert any(rc.tree(s, o, b)[1][-1][1] > 50 for s, o, b in rc.RETRY_RUNS)


def test_retry_counters():
    """A node the retry solves enters lps once and pivots with the first
    pass's limit plus the retry's own count."""
    spec, order, batch = rc.RETRY_RUNS[0]
    c, log = rc.tree(spec, order, batch)
    solved = [r for r in c.ipm if r['status'] == 0]
    assert log[-1][5] == len(c.ipm) == log[-1][1] - c.nskip
    assert len(c.ipm) - len(solved) == c.nsettled + c.nretried
    assert log[-1][6] == (sum(r['iters'] for r in solved) + qp_ipm.MAXIT * c.nsettled
                          + sum(qp_ipm.MAXIT + r['iters'] for r in c.retried))
    assert log[-1][8] == len(solved) + c.nretry_solved


def test_without_the_retry_the_tree_ends_in_an_engine_problem():
    for spec, order, batch in rc.RETRY_RUNS[:3]:
        c, _ = rc.tree(spec, order, batch)
        c0, log0 = rc.tree(spec, order, batch, False, c.first_retry_round + 1)
        assert c0.nstatus12 >= 1 and log0[-1][2][4] >= 1
        assert len(log0) == c.first_retry_round + 1
        _, log = rc.tree(spec, order, batch)
        assert log0[:-1] == log[:c.first_retry_round]
