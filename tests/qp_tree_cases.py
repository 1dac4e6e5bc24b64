"""The MIQPs of tests/test_qp_tree_cpu.py and tests/test_qp_tree_gpu.py: small
convex MIQPs (qp.random_miqp) whose branch-and-bound over QP relaxations the
restatement (oracle/bnb.py, CpuBnbContext with bnb_relaxation 1) follows node
for node, and whose optimum brute force over the integer assignments checks.

A case is (nbin, nint, ncont, m, seed).  Every case's decisions keep at least
MARGIN_FLOOR from their thresholds in the restatement (asserted by the CPU
test), so two correct solvers of the node QPs take the same tree.  The
restatement's trees and the brute-force optima are computed once per process
and shared."""
import functools
import itertools
import math

import numpy as np

import bnb as obnb
import qp_ipm
from minotaur_amd import qp as qpm

# max |x_K5 - x_restatement| over the status-0 nodes of every case's
# depth-first batch-16 tree (test_k5_on_tree_boxes prints it), measured on an
# MI355X on 2026-10-21
X_DIFF_MEASURED = 7.2e-12   # 7.141e-12, at (6, 3, 4, 2, 3)
# a decision closer than this to its threshold could differ between two
# correct solvers
MARGIN_FLOOR = 100 * X_DIFF_MEASURED

# sizes are the depth-first trees' at batches 1 to 16
CASES = (
    [(8, 0, 4, 2, s) for s in range(4)]          # 7 to 51 nodes
    + [(10, 0, 3, 3, s) for s in range(4)]       # 93 to 293 nodes, 29 to 105 settled by the LP
    + [(12, 0, 4, 3, s) for s in range(2)]       # 403 to 501 nodes
    # general integers in [0, 3], 27 to 159 nodes; the seeds left out have an
    # integer assignment whose feasible QP the interior point does not solve
    # (STALLED below is one), so brute force cannot value them
    + [(6, 3, 4, 2, s) for s in (1, 3, 7)]
    + [(8, 2, 4, 3, s) for s in (0, 1, 6)]
)
# the cases whose batch-1 trees stay under 60 nodes at both orders
SMALL = [c for c in CASES if c[:4] == (8, 0, 4, 2)] + [(6, 3, 4, 2, 3), (6, 3, 4, 2, 7),
                                                         (8, 2, 4, 3, 0)]

# brute_force() of every case as recorded on the CPU (test_qp_tree_cpu.py
# holds brute_force to them), so that the GPU tests need not enumerate again
OPTIMA = {
    (8, 0, 4, 2, 0): -2.9122199028250035, (8, 0, 4, 2, 1): -2.3418631380074357,
    (8, 0, 4, 2, 2): -2.3504926235915793, (8, 0, 4, 2, 3): -1.8019118148176196,
    (10, 0, 3, 3, 0): 0.23572888937763326, (10, 0, 3, 3, 1): 0.6427830842493736,
    (10, 0, 3, 3, 2): 0.04210946620313161, (10, 0, 3, 3, 3): 6.275780081866287,
    (12, 0, 4, 3, 0): -1.8316970635104237, (12, 0, 4, 3, 1): -3.700700352936919,
    (6, 3, 4, 2, 1): -0.8641838444496359, (6, 3, 4, 2, 3): 3.262296799318146,
    (6, 3, 4, 2, 7): -3.4230681191251877,
    (8, 2, 4, 3, 0): -1.54512383650491, (8, 2, 4, 3, 1): -0.16498930930059164,
    (8, 2, 4, 3, 6): -2.467992120680488,
}
# the cases that also run from a start incumbent of optimum + START_ABOVE
INC_CASES = [(8, 0, 4, 2, 0), (8, 0, 4, 2, 3), (10, 0, 3, 3, 0), (10, 0, 3, 3, 2), (12, 0, 4, 3, 1),
             (6, 3, 4, 2, 1), (8, 2, 4, 3, 6)]
START_ABOVE = 1e-3

ORDERS = (0, 1)
BATCHES = (1, 3, 16)

# A feasible, well-conditioned node QP the interior point does not solve: this
# integer assignment of random_miqp(2, nbin=6, nint=3, ncont=4, m=2) (cond Q =
# 104) leaves the four continuous columns a feasible set with an interior 0.18
# wide, K1 tightens nothing, and the iteration stalls next to two bounds with
# a dual residual of 0.24 (status 6 at any iteration limit).
STALLED = ((6, 3, 4, 2, 2), (0, 0, 1, 1, 1, 0, 3, 1, 0))
# (draw, span_exp) of ill_conditioned() for the engine-problem test: K5 ends
# at status 6 on its root box (measured on an MI355X on 2026-10-21)
ENGINE_DRAW = (2, 14)


def case_id(case):
    return 'b{}i{}c{}m{}s{}'.format(*case)


@functools.lru_cache(maxsize=None)
def problem(case):
    nbin, nint, ncont, m, seed = case
    P = qpm.random_miqp(seed, nbin=nbin, ncont=ncont, m=m, nint=nint)
    for a in (P.Q, P.c, P.A, P.b, P.l, P.u):
        a.setflags(write=False)
    return P


def assignments(P):
    """(l, u, feasible) for every assignment of the integer columns; the
    feasibility of its rows over the continuous columns by HiGHS."""
    from scipy.optimize import linprog
    ints = np.nonzero(np.isin(P.vtype, (0, 1)))[0]
    ranges = [range(int(P.l[j]), int(P.u[j]) + 1) for j in ints]
    for vals in itertools.product(*ranges):
        l, u = P.l.copy(), P.u.copy()
        l[ints] = u[ints] = vals
        r = linprog(np.zeros(P.n), A_eq=P.A, b_eq=P.b, bounds=list(zip(l, u)), method='highs')
        yield l, u, r.status == 0


def count_assignments(P):
    ints = np.isin(P.vtype, (0, 1))
    return int(np.prod(P.u[ints] - P.l[ints] + 1))


@functools.lru_cache(maxsize=None)
def brute_force(case):
    """The optimum over every integer assignment (at most 4096), each
    feasible assignment's QP by the interior-point restatement."""
    P = problem(case)
    assert count_assignments(P) <= 4096
    best = math.inf
    for l, u, ok in assignments(P):
        if not ok:
            continue
        r = qp_ipm.solve_node(P.Q, P.c, P.A, P.b, l, u)
        assert r['status'] == 0
        best = min(best, r['obj'] + P.k)
    return best


_node_cache = {}     # per QP: the interior point's answer per node box


def cpu_context(P, key, order=0):
    """A CpuBnbContext over P's rows with P loaded as the node relaxation;
    ``key`` names P for the cache of node solves."""
    c = obnb.CpuBnbContext(qpm.rows_problem(P), order=order)
    c.load_qp(P, cache=_node_cache.setdefault(key, {}))
    c.bnb_relaxation(1)
    return c


@functools.lru_cache(maxsize=None)
def tree(case, order, batch, incumbent=math.inf, max_rounds=10**9):
    """The restatement's tree: (context after the last round, [per round
    (rounds, nodes, ndec, pruned, open, lps, pivots, incumbent, nodes the
    interior point solved so far)])."""
    P = problem(case) if isinstance(case, tuple) else case_problem(case)
    c = cpu_context(P, case, order)
    c.bnb_init(1 << 14, P.l, P.u, incumbent)
    log = []
    for _ in range(max_rounds):
        st = c.bnb_round(batch)
        log.append(stats_row(st) + (c.nsolved,))
        if st.open == 0:
            break
    return c, tuple(log)


def stats_row(st):
    return (int(st.rounds), int(st.nodes), tuple(int(v) for v in st.ndec), int(st.pruned),
            int(st.open), int(st.lps), int(st.pivots), float(st.incumbent))


def stalled_box():
    """(P, l, u) of STALLED: the root box with the integer columns fixed."""
    case, vals = STALLED
    P = problem(case)
    l, u = P.l.copy(), P.u.copy()
    l[:len(vals)] = u[:len(vals)] = vals
    return P, l, u


@functools.lru_cache(maxsize=None)
def ill_conditioned(draw, span_exp):
    """A MIQP whose root QP is feasible but ill-conditioned: n = 10 (six
    binaries, four continuous columns in [0, 2]), m = 2, Q = U diag(e) U' with
    e spread evenly in the logarithm over a span of 10^span_exp around 1, c
    scaled by the square root of the span, b = A x0 for an interior x0."""
    rng = np.random.default_rng(7000 + draw)
    n, m, nbin = 10, 2, 6
    U = np.linalg.qr(rng.normal(size=(n, n)))[0]
    Q = (U * np.logspace(-span_exp / 2, span_exp / 2, n)) @ U.T
    Q = 0.5 * (Q + Q.T)
    c = rng.normal(size=n) * 10.0 ** (span_exp / 2)
    A = rng.uniform(0.5, 1.5, size=(m, n))
    l = np.zeros(n)
    u = np.concatenate([np.ones(nbin), np.full(n - nbin, 2.0)])
    b = A @ (rng.uniform(0.2, 0.8, size=n) * u)
    vtype = np.array([0] * nbin + [4] * (n - nbin), dtype=np.int32)
    return qpm.QpProblem(f'ill{draw}e{span_exp}', Q, c, 0.0, A, b, l, u, vtype)


def rows_feasible(P, l, u):
    """HiGHS on the rows over the box."""
    from scipy.optimize import linprog
    r = linprog(np.zeros(P.n), A_eq=P.A, b_eq=P.b, bounds=list(zip(l, u)), method='highs')
    return r.status == 0


@functools.lru_cache(maxsize=None)
def case_problem(name):
    """Named instances: 'color_lab2' (n = 300, m = 61, the benchmark's config 4)."""
    import os
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
    assert name == 'color_lab2'
    return qpm.load(os.path.join(root, 'minotaur_amd', 'instances', 'color_lab2_qp.npz'))
