"""CPU: the dual-simplex restatement (oracle/lp_dual.c) on the edge-case LPs
of tests/lp_edge_cases.py against scipy's HiGHS, the only reference that was
not written by the hand that wrote the kernels.

Every case at every shape: cold from the slack basis, warm from its root
basis under another objective (no reduced costs) and as bound LPs min +-x_j
from the root basis, in the dense arithmetic and in the product form at the
caps the kernels run (16 and 32 for m <= 64, K3PW's for 64 < m <= 128; none
beyond: no kernel runs the product form there).  Bars: the status is HiGHS's
on every LP (never HiGHS 'unknown'); where it is 0 the objective is within
the project's 1e-6 and x satisfies the rows and the true bounds to 1e-6 of
each one's scale.

The 36 bound LPs of the golden knapsack LP are the bug these tests were
written for: free columns boxed for their first reduced cost, back at zero
reduced cost after a pivot, once grown to 1e13 and reported unbounded
(deviations)."""
import math

import numpy as np
import pytest

import lp_edge_cases as ec
import oracle
from golden_io import OBJ_TOL

FEAS_TOL = 1e-6


def _check(p, status, obj, x, ref, what, lb=None, ub=None):
    """One LP's oracle answer against HiGHS's (status, objective)."""
    hs, ho = ref
    assert hs in (0, 2, 4), (what, hs)          # never 'unknown'
    assert status == hs, (what, status, hs)
    if hs == 0:
        assert abs(obj - ho) <= OBJ_TOL * max(1.0, abs(ho)), (what, obj, ho)
        assert ec.residual(p, x, lb, ub) <= FEAS_TOL, (what, ec.residual(p, x, lb, ub))
    else:
        assert math.isinf(obj) and (obj > 0) == (hs == 2), (what, obj)


def _modes(m):
    return (0,) + tuple(ec.pfi_caps(m))


@pytest.mark.parametrize('cid', ec.case_ids())
def test_cold_vs_highs(cid):
    c = ec.case(cid)
    hs, ho = ec.highs_cold(cid)
    assert hs == c.core.status
    if hs == 0:
        assert abs(ho - c.core.objval) <= OBJ_TOL * max(1.0, abs(ho))
    st, obj, _, x = oracle.dual_simplex(c.p, c.p.vlb[None], c.p.vub[None], want_x=True)
    _check(c.p, st[0], obj[0], x[0], (hs, ho), cid)
    rs, robj, rx, _ = ec.root(cid)
    _check(c.p, rs, robj, rx, (hs, ho), cid + ' root')


@pytest.mark.parametrize('cid', ec.case_ids())
def test_warm_from_root_vs_highs(cid):
    """From the root basis where the root is optimal: the root box again (no
    pivot), boxes that cut the root solution off, and another objective on
    the old basis without reduced costs."""
    c = ec.case(cid)
    rs, robj, _, ws = ec.root(cid)
    if rs != 0:
        assert c.core.status != 0     # nothing to start from: by design
        return
    LB, UB = ec.warm_boxes(cid)
    refs = ec.highs_warm_boxes(cid)
    for pfi in _modes(c.m):
        st, obj, it, x = oracle.dual_simplex(c.p, LB, UB, ws, want_x=True, pfi=pfi)
        for b in range(LB.shape[0]):
            _check(c.p, st[b], obj[b], x[b], refs[b], (cid, pfi, b), LB[b], UB[b])
        assert it[0] == 0
    box = (c.p.vlb[None], c.p.vub[None])
    q = ec.new_objective(c)
    st, obj, _, x = oracle.dual_simplex(q, *box, oracle.WarmStart(ws.head, ws.st, ws.binv, None),
                                        want_x=True)
    _check(q, st[0], obj[0], x[0], ec.highs_new_objective(cid), cid + ' new objective')


def _bound_lps(p, cols, signs, ws, refs, modes, what):
    dense = None
    for pfi in modes:
        st, obj, _, x = oracle.lp_bound(p, cols, signs, ws=ws, pfi=pfi)
        for k in range(cols.size):
            _check(p, st[k], obj[k], x[k], refs[k], (what, pfi, int(cols[k]), signs[k]))
        # the product form never disagrees with the dense arithmetic on a status
        dense = st if dense is None else dense
        assert np.array_equal(st, dense), (what, pfi)


@pytest.mark.parametrize('cid', ec.case_ids())
def test_bound_lps_vs_highs(cid):
    c = ec.case(cid)
    rs, _, _, ws = ec.root(cid)
    cols, signs = ec.bound_lps(c)
    if rs == 0:
        _bound_lps(c.p, cols, signs, ws, ec.highs_bounds(cid), _modes(c.m), cid)
    else:   # no optimal root: from the slack basis, dense
        _bound_lps(c.p, cols, signs, None, ec.highs_bounds(cid), (0,), cid)


def test_knapsack_bound_lps_vs_highs():
    """Failed before the rule of DESIGN.md (deviations): 12 of the 36 came
    back as status 4 in the dense arithmetic, 9 and 10 of them in the product
    form at 16 and 32 etas, on LPs whose optimum HiGHS and the cold solve
    agree on."""
    p, cols, signs = ec.knapsack_bound_lps()
    rs, _, _, ws = ec.root('knapsack')
    assert rs == 0
    refs = ec.highs_bounds('knapsack')
    assert sorted(set(h[0] for h in refs)) == [0, 4]
    _bound_lps(p, cols, signs, ws, refs, _modes(p.m), 'knapsack')
    # and cold, each objective from the slack basis
    _bound_lps(p, cols, signs, None, refs, (0,), 'knapsack cold')
