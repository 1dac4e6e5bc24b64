"""The cases of tests/test_qp_retry_cpu.py and tests/test_qp_retry_gpu.py: node
QPs on which the separate-step interior point stalls (status 6 at any
iteration limit) and the coupled step (mgpu_qp_step_rule 1) converges, and
trees that meet such a node, run with the retry (rule 2) against the
restatement of tests/qp_retry_ref.py.

A case is (nbin, nint, ncont, m, seed) of qp.random_miqp, as in
tests/qp_tree_cases.py, whose helpers this file builds on."""
import functools
import math

import numpy as np

import qp_ipm
import qp_retry_ref as rr
import qp_tree_cases as tc

# (case, values of the integer columns): feasible node QPs that qp_ipm.solve_node
# leaves at status 6; the continuous columns keep the root bounds.  The second
# is tc.STALLED.
STALLED_BOXES = (
    ((6, 3, 4, 2, 0), (1, 1, 0, 1, 1, 0, 3, 0, 3)),
    ((6, 3, 4, 2, 2), (0, 0, 1, 1, 1, 0, 3, 1, 0)),
    ((6, 3, 4, 2, 2), (0, 1, 1, 1, 1, 0, 0, 0, 3)),
    ((8, 2, 4, 3, 2), (0, 1, 1, 1, 1, 0, 1, 0, 1, 1)),
    ((8, 2, 4, 3, 4), (0, 1, 0, 0, 1, 1, 0, 0, 3, 0)),
    ((8, 2, 4, 3, 4), (0, 1, 0, 0, 1, 1, 1, 0, 2, 0)),
)

# Trees that meet a retried node.  ('full', case): the whole tree of the case.
# ('sub', case, values, k): the tree from the root box with every integer
# column but the first k (k a tuple: but the columns k) fixed to ``values``.
_ALL_RUNS = tuple((o, b) for o in tc.ORDERS for b in tc.BATCHES)
# (tree, the (order, batch) at which the restatement's tree meets a retried
# node): stalled assignments are mostly pruned before they are reached, so the
# full tree meets its one only depth-first at batch 16 (147 nodes), and the
# k = 3 sub-box tree only depth-first.  test_qp_retry_cpu.py holds the
# restatement to this table.
RETRY_TREES = (
    (('full', (10, 0, 3, 3, 10)), ((0, 16),)),
    (('sub', (6, 3, 4, 2, 2), (0, 1, 1, 1, 1, 0, 0, 0, 3), 2), _ALL_RUNS),      # 5 nodes
    (('sub', (6, 3, 4, 2, 2), (0, 1, 1, 1, 1, 0, 0, 0, 3), 3), ((0, 1), (0, 3), (0, 16))),   # 9
    (('sub', (8, 2, 4, 3, 2), (0, 1, 1, 1, 1, 0, 1, 0, 1, 1), 2), _ALL_RUNS),   # 4 or 5
    (('sub', (8, 2, 4, 3, 2), (0, 1, 1, 1, 1, 0, 1, 0, 1, 1), 4), _ALL_RUNS),   # 13 or 15
    # around tc.STALLED, the one box whose stall on the device is on record:
    # its retried node is STALLED itself
    (('sub',) + tc.STALLED + ((0, 3),), _ALL_RUNS),                             # 7
)
RETRY_RUNS = tuple((spec, o, b) for spec, runs in RETRY_TREES for o, b in runs)

# the seeds tc.CASES leaves out of its general-integer families
LEFT_OUT = ([(6, 3, 4, 2, s) for s in (0, 2, 4, 5, 6)]
            + [(8, 2, 4, 3, s) for s in (2, 3, 4, 5, 7)])
# brute_force() of each as recorded on the CPU (test_qp_retry_cpu.py holds
# brute_force to them) and how many of its row-feasible assignments the
# separate step left to the retry
OPTIMA = {
    (6, 3, 4, 2, 0): -5.126157166767001, (6, 3, 4, 2, 2): -5.600916505379089,
    (6, 3, 4, 2, 4): 0.5026908362704359, (6, 3, 4, 2, 5): -2.4131269104780717,
    (6, 3, 4, 2, 6): 2.9055457297808642,
    (8, 2, 4, 3, 2): -4.6151182342948704, (8, 2, 4, 3, 3): -0.7856620792944167,
    (8, 2, 4, 3, 4): -6.434015804542069, (8, 2, 4, 3, 5): -4.976864907527926,
    (8, 2, 4, 3, 7): -3.9734994023462775,
}
STALLED_ASSIGNMENTS = {(6, 3, 4, 2, 0): 1, (6, 3, 4, 2, 2): 2, (8, 2, 4, 3, 2): 1,
                       (8, 2, 4, 3, 4): 2}     # the other six: none

# max |x_K5 - x_restatement| of the coupled step over the six stalled boxes
# and the shapes of test_rule1_shapes (tests/test_qp_retry_gpu.py prints it),
# measured on an MI355X on 2026-10-21
X_DIFF_COUPLED_MEASURED = 1.3e-14   # 1.299e-14, at (8, 2, 4, 3, 2); the shapes: 5.2e-15


def tree_id(spec):
    if spec[0] == 'full':
        return 'full-' + tc.case_id(spec[1])
    k = spec[3] if isinstance(spec[3], int) else 'c' + ''.join(map(str, spec[3]))
    return 'sub-{}-{}-k{}'.format(tc.case_id(spec[1]), ''.join(map(str, spec[2])), k)


def box_of(case, vals, free=0):
    """(P, l, u): the root box with the integer columns fixed to ``vals``,
    the first ``free`` of them (a tuple: the columns ``free``) left at their
    root bounds."""
    P = tc.problem(case)
    l, u = P.l.copy(), P.u.copy()
    cols = range(free) if isinstance(free, int) else free
    fix = [j for j in range(len(vals)) if j not in cols]
    l[fix] = u[fix] = np.array(vals, dtype=np.float64)[fix]
    return P, l, u


def tree_root(spec):
    if spec[0] == 'full':
        P = tc.problem(spec[1])
        return P, P.l.copy(), P.u.copy()
    return box_of(spec[1], spec[2], spec[3])


_node_cache = {}


@functools.lru_cache(maxsize=None)
def tree(spec, order, batch, retry=True, max_rounds=10**9):
    """The restatement's tree with the retry: (context after the last round,
    [per round tc.stats_row + (nodes the interior point solved so far,)])."""
    import bnb as obnb
    from minotaur_amd import qp as qpm
    P, l, u = tree_root(spec)
    c = (rr.RetryBnbContext if retry else obnb.CpuBnbContext)(qpm.rows_problem(P), order=order)
    c.load_qp(P, cache=_node_cache.setdefault(spec[1], {}))
    c.bnb_relaxation(1)
    c.bnb_init(1 << 14, l, u)
    log = []
    for _ in range(max_rounds):
        st = c.bnb_round(batch)
        log.append(tc.stats_row(st) + (c.nsolved,))
        if st.open == 0:
            break
    return c, tuple(log)


@functools.lru_cache(maxsize=None)
def brute_force(case):
    """(optimum, stalled assignments): the optimum over every integer
    assignment, each row-feasible assignment's QP by the separate step and,
    where that stalls, by the coupled step."""
    P = tc.problem(case)
    assert tc.count_assignments(P) <= 4096
    best, nretry = math.inf, 0
    for l, u, ok in tc.assignments(P):
        if not ok:
            continue
        r = rr.solve_node_retry(P.Q, P.c, P.A, P.b, l, u)
        assert r['status'] == 0
        nretry += r['retried']
        best = min(best, r['obj'] + P.k)
    return best, nretry
