"""CPU: the restatement of the branch-and-bound over QP relaxations
(oracle/bnb.py, CpuBnbContext with bnb_relaxation 1) on the cases of
tests/qp_tree_cases.py, before tests/test_qp_tree_gpu.py holds the engine's
tree to it round for round.

The restatement proves the brute-force optimum at every order and batch size;
no node ends as an engine problem; every decision of every tree keeps at
least MARGIN_FLOOR from its threshold (so a correct solver of the node QPs
that differs from the restatement by rounding takes the same tree); and the
cases together reach the paths the tree has: nodes settled by the phase-1 LP,
nodes K1 proves infeasible, general-integer branchings above 1, full rounds
of 16."""
import math

import numpy as np
import pytest

import qp_ipm
import qp_tree_cases as tc
from minotaur_amd import qp as qpm

_ids = [tc.case_id(c) for c in tc.CASES]


def _old_random_miqp(seed, nbin=8, ncont=4, m=2):
    """random_miqp before it had general integers: the same draws."""
    rng = np.random.default_rng(seed)
    n = nbin + ncont
    G = rng.normal(size=(n, n))
    Q = G @ G.T / n + 0.01 * np.eye(n)
    c = rng.normal(size=n)
    A = np.zeros((m, n))
    A[:, :nbin] = rng.uniform(0.5, 1.5, size=(m, nbin)) * (rng.random((m, nbin)) < 0.6)
    A[:, nbin:] = rng.uniform(0.5, 1.5, size=(m, ncont))
    b = A[:, :nbin].sum(axis=1) * 0.4 + A[:, nbin:].sum(axis=1) * 0.7
    u = np.concatenate([np.ones(nbin), np.full(ncont, 2.0)])
    return Q, c, A, b, np.zeros(n), u, np.array([0] * nbin + [4] * ncont, dtype=np.int32)


@pytest.mark.parametrize('seed', range(4))
def test_random_miqp_without_integers_is_unchanged(seed):
    P = qpm.random_miqp(seed)
    for new, old in zip((P.Q, P.c, P.A, P.b, P.l, P.u, P.vtype), _old_random_miqp(seed)):
        assert new.dtype == old.dtype and new.tobytes() == old.tobytes()
    assert P.k == 0.0 and P.name == f'miqp{seed}'


def test_random_miqp_general_integers():
    P = qpm.random_miqp(5, nbin=3, nint=2, ncont=2, m=3, iub=4)
    assert list(P.vtype) == [0, 0, 0, 1, 1, 4, 4]
    assert list(P.u) == [1, 1, 1, 4, 4, 2, 2] and not P.l.any()
    assert np.array_equal(P.b, (P.A[:, :5] * P.u[:5]).sum(axis=1) * 0.4
                          + P.A[:, 5:].sum(axis=1) * 0.7)


@pytest.mark.parametrize('case', tc.CASES, ids=_ids)
def test_restatement_proves_brute_force_optimum(case):
    opt = tc.brute_force(case)
    assert math.isfinite(opt)
    # the recorded value the GPU tests use: the interior point stops at a
    # complementarity of 1e-10, far inside this
    assert abs(opt - tc.OPTIMA[case]) <= 1e-8 * max(1.0, abs(opt))
    P = tc.problem(case)
    ints = np.isin(P.vtype, (0, 1))
    for order in tc.ORDERS:
        for batch in tc.BATCHES:
            c, log = tc.tree(case, order, batch)
            assert log[-1][4] == 0, 'open nodes left'
            assert c.nstatus12 == 0 and log[-1][2][4] == 0, (order, batch)
            assert log[-1][1] == sum(log[-1][2])
            assert abs(c.inc - opt) <= 1e-6 * max(1.0, abs(opt)), (order, batch, c.inc, opt)
            x = c.best_x
            assert np.all(np.abs(x[ints] - np.round(x[ints])) <= 1e-6)
            assert np.max(np.abs(P.A @ x - P.b)) <= 1e-7


@pytest.mark.parametrize('case', tc.CASES, ids=_ids)
def test_margins(case, capsys):
    worst = {}
    for order in tc.ORDERS:
        for batch in tc.BATCHES:
            for k, v in tc.tree(case, order, batch)[0].margins.items():
                if v < worst.get(k, (math.inf,))[0]:
                    worst[k] = (v, order, batch)
    with capsys.disabled():
        print(f'\n{tc.case_id(case)} margins: '
              + ', '.join(f'{k} {v[0]:.2e}' for k, v in worst.items()))
    for k, v in worst.items():
        assert v[0] >= tc.MARGIN_FLOOR, (k, v)


def test_small_cases_are_small():
    for case in tc.SMALL:
        assert case in tc.CASES
        for order in tc.ORDERS:
            assert tc.tree(case, order, 1)[1][-1][1] < 60, (case, order)


def test_cases_reach_the_paths():
    """Conditions on the inputs: which paths of the tree the cases run."""
    trees = [tc.tree(case, order, batch)[0] for case in tc.CASES for order in tc.ORDERS
             for batch in tc.BATCHES]
    per_case = {case: max(tc.tree(case, o, b)[0].nsettled for o in tc.ORDERS
                          for b in tc.BATCHES) for case in tc.CASES}
    assert sum(v >= 20 for v in per_case.values()) >= 3, per_case
    assert any(t.nskip > 0 for t in trees), 'no node K1 proved infeasible'
    assert any(t.int_branch > 0 for t in trees), 'no general-integer branching above 1'
    assert any(t.max_batch == 16 for t in trees), 'no round of 16 nodes'
    # both orders and every batch size meet infeasible nodes
    for order in tc.ORDERS:
        for batch in tc.BATCHES:
            assert any(tc.tree(case, order, batch)[0].nsettled > 0 for case in tc.CASES)


def test_counters_follow_the_statuses():
    """lps = nodes that end at status 0 or 2, pivots = their interior-point
    iterations (the limit for a node the phase-1 LP settled)."""
    c, log = tc.tree((10, 0, 3, 3, 1), 0, 16)
    solved = [r for r in c.ipm if r['status'] == 0]
    assert c.nstatus12 == 0
    assert log[-1][5] == len(c.ipm) == log[-1][1] - c.nskip
    assert len(c.ipm) - len(solved) == c.nsettled > 0
    assert log[-1][6] == sum(r['iters'] for r in solved) + qp_ipm.MAXIT * c.nsettled


def test_restatement_refuses_what_the_engine_refuses():
    import bnb as obnb
    P = tc.problem(tc.CASES[0])
    for kw in (dict(warm=1), dict(brancher=1), dict(order=2)):
        c = obnb.CpuBnbContext(qpm.rows_problem(P), **kw)
        c.load_qp(P)
        c.bnb_relaxation(1)
        with pytest.raises(ValueError):
            c.bnb_init(64, P.l, P.u)
    c = obnb.CpuBnbContext(qpm.rows_problem(P))
    c.bnb_relaxation(1)
    with pytest.raises(ValueError):      # no QP loaded
        c.bnb_init(64, P.l, P.u)
    with pytest.raises(ValueError):
        c.bnb_relaxation(2)


@pytest.mark.parametrize('case', tc.INC_CASES, ids=[tc.case_id(c) for c in tc.INC_CASES])
def test_start_incumbent(case):
    """A start incumbent just above the optimum prunes from the first round
    on, the tree still proves the optimum, and its decisions keep the
    margin."""
    opt = tc.OPTIMA[case]
    for order in tc.ORDERS:
        c, log = tc.tree(case, order, 3, opt + tc.START_ABOVE)
        c0, log0 = tc.tree(case, order, 3)
        assert abs(c.inc - opt) <= 1e-6 * max(1.0, abs(opt))
        assert log[-1][1] <= log0[-1][1] and log != log0     # it pruned
        assert c.nstatus12 == 0 and log[-1][4] == 0
        for k, v in c.margins.items():
            assert v >= tc.MARGIN_FLOOR, (order, k, v)


@pytest.mark.parametrize('which', ['ill-conditioned', 'stalled'])
def test_engine_problem_in_the_restatement(which):
    """A feasible node QP the interior point leaves at status 6: the phase-1
    LP finds the rows feasible, the node ends at status 12, decision 4."""
    if which == 'stalled':
        P, l, u = tc.stalled_box()
        with np.errstate(all='ignore'):
            assert qp_ipm.solve_node(P.Q, P.c, P.A, P.b, l, u, maxit=400)['status'] == 6
    else:
        P = tc.ill_conditioned(*tc.ENGINE_DRAW)
        l, u = P.l, P.u
        ev = np.linalg.eigvalsh(P.Q)
        assert ev[0] > 0 and 1e12 <= ev[-1] / ev[0] <= 1e16
    assert tc.rows_feasible(P, l, u)
    with np.errstate(all='ignore'):
        assert qp_ipm.solve_node(P.Q, P.c, P.A, P.b, l, u)['status'] == 6
    c = tc.cpu_context(P, which)
    c.bnb_init(64, l, u)
    st = c.bnb_round(1)
    assert c.nstatus12 == 1 and tuple(st.ndec) == (0, 0, 0, 0, 1)
    assert (st.nodes, st.open, st.lps, st.pivots) == (1, 0, 0, 0)


def test_color_lab2_dive_margins(capsys):
    c, log = tc.tree('color_lab2', 0, 1, math.inf, 12)
    with capsys.disabled():
        print('\ncolor_lab2 12-round dive margins: '
              + ', '.join(f'{k} {v:.2e}' for k, v in c.margins.items()))
    assert log[-1][0] == 12 and c.nstatus12 == 0
    for k, v in c.margins.items():
        assert v >= tc.MARGIN_FLOOR, (k, v)
