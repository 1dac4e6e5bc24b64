"""GPU: K5's coupled step (mgpu_qp_step_rule 1) and the retry pass (rule 2),
held to their restatement (tests/qp_retry_ref.py) on the cases of
tests/qp_retry_cases.py.

Bar: rule 1 solves the six node QPs the separate step stalls on, in the
restatement's iterations (+-1) and to its objective (1e-6), and follows it at
one shape per qp_step<J>; rule 2 leaves every slot the first pass settled
with rule 0's bits and gives every retried slot rule 1's bits, with iters =
the limit + rule 1's count, whatever the place of the retried nodes in the
batch (first, last, none, all, across the gather kernel's blocks); the trees
that meet a stalled node agree with the restatement round for round with the
retry and end in MGPU_ERR_ENGINE in the restatement's round without it; the
seeds tests/qp_tree_cases.py leaves out prove the brute-force optimum; a
second retry tree on a context allocates nothing.

Measured on an MI355X (2026-10-21): under rule 1 K5 took exactly the
restatement's iterations on the six boxes (7, 10, 11, 21, 9, 9) and at the
three shapes (10, 10; 10, 9; 10, 10); max |x_K5 - x_restatement| = 1.299e-14
(X_DIFF_COUPLED_MEASURED of tests/qp_retry_cases.py); every box the
restatement retries was at status 6 after K5's own first pass, so no retry
tree had to be dropped."""
import ctypes
import math

import numpy as np
import pytest

import qp_cases
import qp_ipm
import qp_retry_cases as rc
import qp_retry_ref as rr
import qp_tree_cases as tc
import test_qp_tree_gpu as tg
from minotaur_amd import qp as qpm
from minotaur_amd import runtime

pytestmark = pytest.mark.gpu
CAP = 1 << 14


@pytest.fixture(scope='module')
def ctx():
    c = runtime.Context(0)
    yield c
    c.qp_step_rule(0)
    c.close()


@pytest.fixture
def rule(ctx):
    """Sets the step rule for one test; 0 again afterwards."""
    yield ctx.qp_step_rule
    ctx.qp_step_rule(0)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8).tobytes()


def _assert_x_diff(xd):
    # a hundred times the largest difference as measured: another order of
    # K5's sums may move it, but not there
    assert xd <= 100 * rc.X_DIFF_COUPLED_MEASURED, xd


def _against_the_restatement(P, LB, UB, st, ob, it, x):
    """Rule 1's answers against solve_node_coupled's; returns max |x - x_ref|."""
    xd = 0.0
    for b in range(LB.shape[0]):
        r = rr.solve_node_coupled(P.Q, P.c, P.A, P.b, LB[b], UB[b])
        assert r['status'] == 0 and st[b] == 0, (b, st[b], r['status'])
        assert abs(int(it[b]) - r['iters']) <= 1, (b, it[b], r['iters'])
        f = r['obj'] + P.k
        assert abs(ob[b] - f) <= 1e-6 * max(1.0, abs(f)), (b, ob[b], f)
        xd = max(xd, float(np.max(np.abs(x[b] - r['x']))))
    return xd


# ---- a. rule 1 alone -----------------------------------------------------------
def test_rule1_solves_the_stalled_boxes(ctx, rule, capsys):
    """The six boxes, each problem's in one batch: status 6 at the limit under
    rule 0, the restatement's answer under rule 1."""
    worst = 0.0
    for case in sorted({c for c, _ in rc.STALLED_BOXES}):
        boxes = [rc.box_of(c, v) for c, v in rc.STALLED_BOXES if c == case]
        P = boxes[0][0]
        LB = np.array([l for _, l, _ in boxes])
        UB = np.array([u for _, _, u in boxes])
        ctx.load_qp(P)
        rule(0)
        st, _, it, _ = ctx.qp_solve(LB, UB)
        assert np.all(st == 6) and np.all(it == qp_ipm.MAXIT), (case, st, it)
        rule(1)
        st, ob, it, x = ctx.qp_solve(LB, UB)
        xd = _against_the_restatement(P, LB, UB, st, ob, it, x)
        with capsys.disabled():
            print(f'\n{tc.case_id(case)}: {len(boxes)} stalled boxes, rule 1 iterations '
                  f'{list(it)}, max |x_K5 - x_ref| = {xd:.3e}')
        worst = max(worst, xd)
    with capsys.disabled():
        print(f'\nstalled boxes: max |x_K5 - x_restatement| = {worst:.3e}')
    _assert_x_diff(worst)


@pytest.mark.parametrize('n,m,J', [(512, 3, 2), (513, 3, 4), (1025, 2, 8)])
def test_rule1_shapes(ctx, rule, n, m, J, capsys):
    """One shape per qp_step<J>, two node boxes: rule 1 against its
    restatement."""
    P, LB, UB, _ = qp_cases.case(n, m)
    LB, UB = LB[:2], UB[:2]
    ctx.load_qp(P)
    assert ctx.qp_plan()[2] == J
    rule(1)
    st, ob, it, x = ctx.qp_solve(LB, UB)
    xd = _against_the_restatement(P, LB, UB, st, ob, it, x)
    with capsys.disabled():
        print(f'\nn = {n}, m = {m}, qp_step<{J}>: rule 1 iterations {list(it)}, '
              f'max |x_K5 - x_ref| = {xd:.3e}')
    _assert_x_diff(xd)


def test_rule_argument(ctx):
    assert ctx.lib.mgpu_qp_step_rule(ctx.h, 3) == -1      # MGPU_ERR_ARG
    assert ctx.lib.mgpu_qp_step_rule(ctx.h, -1) == -1
    ctx.qp_step_rule(0)


# ---- b. rule 2 alone: the gather and scatter edges -----------------------------
_CASE2 = (6, 3, 4, 2, 2)      # the problem with two stalled boxes


def _kinds():
    """'S' / 'T': the two stalled boxes; 'G', 'H': two boxes the first pass
    solves (the first two its depth-first batch-16 tree solved); 'E': an empty
    box (l > u in one column)."""
    S, T = [rc.box_of(c, v)[1:] for c, v in rc.STALLED_BOXES if c == _CASE2]
    solved = [r for r in rc.tree(('full', _CASE2), 0, 16)[0].ipm if r['status'] == 0]
    G, H = [(r['lb'], r['ub']) for r in solved[:2]]
    P = tc.problem(_CASE2)
    el, eu = P.l.copy(), P.u.copy()
    el[P.n - 1], eu[P.n - 1] = 1.5, 0.5
    return dict(S=S, T=T, G=G, H=H, E=(el, eu))


_LAYOUTS = {
    '1-stalled': 'S', '1-solved': 'G', '1-empty': 'E',
    '3-first': 'SGE', '3-last': 'GES', '3-both': 'SGT', '3-none': 'GEH', '3-all': 'STS',
    '17-first': 'S' + 'GHE' * 5 + 'G', '17-last': 'GHE' * 5 + 'GS',
    '17-both': 'T' + 'GHE' * 5 + 'S', '17-none': 'GHE' * 5 + 'GH', '17-all': 'ST' * 8 + 'S',
    '17-mixed': 'GSTEGHSSEETGHGTEH',
    # across the gather kernel's blocks of 256 nodes: the last slot of the
    # first block, the first and the last of the second
    '300-blocks': 'S' + 'GHE' * 84 + 'GHT' + 'S' + 'GHE' * 14 + 'T',
}


@pytest.mark.parametrize('name', list(_LAYOUTS))
def test_rule2_gather_and_scatter(ctx, rule, name):
    kinds = _kinds()
    lay = _LAYOUTS[name]
    assert len(lay) == int(name.split('-')[0])
    P = tc.problem(_CASE2)
    LB = np.array([kinds[k][0] for k in lay])
    UB = np.array([kinds[k][1] for k in lay])
    ctx.load_qp(P)
    rule(0)
    r0 = ctx.qp_solve(LB, UB)
    rule(1)
    r1 = ctx.qp_solve(LB, UB)
    rule(2)
    r2 = ctx.qp_solve(LB, UB)
    stalled = np.array([k in 'ST' for k in lay])
    assert ctx.qp_retried() == int(stalled.sum())
    # the inputs are what their names say
    assert np.array_equal(r0[0], [6 if k in 'ST' else 2 if k == 'E' else 0 for k in lay])
    assert np.all(r1[0][stalled] == 0)
    keep = ~stalled
    for a0, a1, a2 in zip(r0, r1, r2):
        assert _bits(a2[keep]) == _bits(a0[keep])
    for k in (0, 1, 3):          # status, obj, x
        assert _bits(r2[k][stalled]) == _bits(r1[k][stalled])
    assert np.array_equal(r2[2][stalled], qp_ipm.MAXIT + r1[2][stalled])
    assert np.all(r1[2][stalled] < 30)


def test_rule2_counts_from_the_given_limit(ctx, rule):
    """maxit = 40: both passes run to the same limit, iters = 40 + the
    retry's count; a retry that does not converge either stays at status 6
    with twice the limit."""
    kinds = _kinds()
    P = tc.problem(_CASE2)
    LB = np.array([kinds[k][0] for k in 'GST'])
    UB = np.array([kinds[k][1] for k in 'GST'])
    ctx.load_qp(P)
    rule(0)
    st0, _, it0, _ = ctx.qp_solve(LB, UB, maxit=40)
    assert list(st0) == [0, 6, 6]
    rule(1)
    st1, _, it1, _ = ctx.qp_solve(LB, UB, maxit=40)
    assert np.all(st1 == 0)
    rule(2)
    st, _, it, _ = ctx.qp_solve(LB, UB, maxit=40)
    assert np.all(st == 0) and list(it) == [it0[0], 40 + it1[1], 40 + it1[2]]
    st, _, it, _ = ctx.qp_solve(LB, UB, maxit=4)
    assert list(st) == [6, 6, 6] and list(it) == [8, 8, 8]
    assert ctx.qp_retried() == 2 + 3


# ---- c. trees that meet a stalled node -----------------------------------------
def engine_tree(ctx, P, l, u, order, batch, max_rounds=10**9, load=True):
    """The engine's tree from the root box (l, u) under the context's step
    rule: ([stats_row per round], (incumbent, x)).  load=False: P and its
    rows are loaded already."""
    if load:
        ctx.load(qpm.rows_problem(P))
        ctx.load_qp(P)
    ctx.bnb_relaxation(1)
    try:
        ctx.bnb_config(order, 0)
        ctx.bnb_brancher(0)
        ctx.bnb_growth(0)
        ctx.bnb_init(CAP, l, u)
        log = []
        for _ in range(max_rounds):
            st = ctx.bnb_round(batch)
            log.append(tc.stats_row(st))
            if st.open == 0:
                break
        return log, ctx.bnb_best()
    finally:
        ctx.bnb_relaxation(0)


_RUN_IDS = [f'{rc.tree_id(s)}-{o}-{b}' for s, o, b in rc.RETRY_RUNS]


@pytest.mark.parametrize('spec,order,batch', rc.RETRY_RUNS, ids=_RUN_IDS)
def test_retry_tree_parity(ctx, rule, spec, order, batch):
    """With the retry: the restatement's rounds.  Without it: the
    restatement's rounds up to the one that first retries, which ends in
    MGPU_ERR_ENGINE.  Every box the restatement retries is at status 6 after
    K5's own first pass, so its stall and K5's coincide."""
    P, l, u = rc.tree_root(spec)
    cpu, clog = rc.tree(spec, order, batch)
    assert cpu.nretried >= 1 and cpu.nretry_solved == cpu.nretried
    ctx.load_qp(P)
    rule(0)
    st, _, it, _ = ctx.qp_solve(np.array([r['lb'] for r in cpu.retried]),
                                np.array([r['ub'] for r in cpu.retried]))
    assert np.all(st == 6) and np.all(it == qp_ipm.MAXIT), (st, it)
    rule(2)
    glog, (inc, x) = engine_tree(ctx, P, l, u, order, batch)
    assert ctx.qp_retried() == cpu.nretried
    tg.assert_parity(glog, clog, (spec, order, batch))
    assert glog[-1][4] == 0 and glog[-1][2][4] == 0
    assert abs(inc - cpu.inc) <= 1e-6 * max(1.0, abs(cpu.inc))
    tg.assert_final_point(P, inc, x)
    # the retry off
    rule(0)
    first = cpu.first_retry_round
    ctx.load(qpm.rows_problem(P))
    ctx.load_qp(P)
    ctx.bnb_relaxation(1)
    try:
        ctx.bnb_config(order, 0)
        ctx.bnb_brancher(0)
        ctx.bnb_growth(0)
        ctx.bnb_init(CAP, l, u)
        log = [tc.stats_row(ctx.bnb_round(batch)) for _ in range(first)]
        tg.assert_parity(log, clog[:first], (spec, order, batch, 'retry off'))
        s = runtime.BnbStats()
        rcode = ctx.lib.mgpu_bnb_round(ctx.h, batch, ctypes.c_double(math.inf), ctypes.byref(s))
        assert rcode == -5                                   # MGPU_ERR_ENGINE
        assert s.ndec[4] >= 1 and s.rounds == first + 1
    finally:
        ctx.bnb_relaxation(0)


@pytest.mark.parametrize('case', rc.LEFT_OUT, ids=[tc.case_id(c) for c in rc.LEFT_OUT])
def test_left_out_seeds(ctx, case):
    """The seeds tests/qp_tree_cases.py leaves out, through the public helper
    with retry=True at batch 16: the brute-force optimum, and the
    restatement's rounds."""
    P = tc.problem(case)
    opt = rc.OPTIMA[case]
    for order in tc.ORDERS:
        obj, x, st, _ = qpm.solve_tree(ctx, P, batch=16, capacity=CAP, order=order, retry=True)
        assert st.open == 0 and st.ndec[4] == 0
        assert abs(obj - opt) <= 1e-6 * max(1.0, abs(opt)), (order, obj, opt)
        tg.assert_final_point(P, obj, x)
        clog = rc.tree(('full', case), order, 16)[1]
        assert tc.stats_row(st)[:6] == clog[-1][:6], (order, tc.stats_row(st), clog[-1])
    # solve_tree leaves the rule at 0
    ctx.load_qp(tc.problem(_CASE2))
    S = _kinds()['S']
    assert ctx.qp_solve(S[0][None], S[1][None])[0][0] == 6


def test_second_retry_tree_allocates_nothing():
    """The retry's scratch lives with the loaded QP's state, sized with the
    batch: the same tree again on the context finds every buffer there."""
    spec, order, batch = next(r for r in rc.RETRY_RUNS if r[0][0] == 'sub' and r[2] == 16)
    P, l, u = rc.tree_root(spec)
    c = runtime.Context(0)
    try:
        c.qp_step_rule(2)
        first, _ = engine_tree(c, P, l, u, order, batch)
        assert c.qp_retried() >= 1
        a0 = runtime.alloc_stats()
        again, _ = engine_tree(c, P, l, u, order, batch, load=False)
        assert runtime.alloc_stats() == a0
        assert again == first
    finally:
        c.close()
