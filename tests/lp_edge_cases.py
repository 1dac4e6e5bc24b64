"""The edge-case LPs of tests/test_lp_edge_cpu.py and tests/test_lp_edge_gpu.py:
tiny core LPs that reach the rarely taken branches of the dual simplex
(oracle/lp_dual.c and the kernels K3, K3L, K3P, K3PW that follow it pivot for
pivot), embedded among inert padding so that the interesting rows and columns
sit in chosen lanes, waves and strides of the kernels.

Which branch each core reaches (counted once in an instrumented build of the
oracle; the counters are not part of the repository):

  unbounded         artificial box grown at an "optimal" basis until 1e13,
                    then status 4 (ProvenUnbounded)
  far_opt           box grown at an optimum, the flagged column then enters
  free_enter        columns placed ST_FREE, ST_FREE columns enter the basis
  art_infeas_grow   dual unbounded with a boxed column: grown to 1e13, status 2
  art_infeas_enter  grown once, the boxed column enters, status 2 unboxed
  ties              pricing tie (lowest row) and Harris pass-2 tie (lowest
                    column): only x and the final head tell a wrong rule apart
  rays              bound LPs from the root basis: status 4 and ST_FREE columns
                    from a warm start
  box_release       a free column boxed for its first reduced cost, back at zero
                    reduced cost after the first pivot: released from its
                    artificial bound, optimal (the knapsack bug at every shape)
  knapsack (golden) bound LPs from the root basis: free columns whose reduced
                    cost returns to zero on an artificial bound (once reported
                    unbounded: DESIGN.md, deviations)

Padding: columns in [0, 1] with zero cost, rows x_pad <= 2.  They never bind
and never pivot, so an embedded core has the status, the objective and the
pivots of the bare one.
"""
import collections
import functools

import numpy as np

import oracle
from golden_io import load_lp
from minotaur_amd.problem import CONTINUOUS, LinProblem, from_rows

INF = np.inf

Core = collections.namedtuple('Core', 'name n rows rlo rhi vlb vub obj status objval')

CORES = {c.name: c for c in [
    # min -x0 - x1, x0 - x1 <= 1, x >= 0
    Core('unbounded', 2, [[(0, 1.0), (1, -1.0)]], [-INF], [1.0],
         [0.0, 0.0], [INF, INF], [-1.0, -1.0], 4, -INF),
    # min x0, x0 free, x0 - x1 >= -5e8, x1 in [0, 1]
    Core('far_opt', 2, [[(0, 1.0), (1, -1.0)]], [-5e8], [INF],
         [-INF, 0.0], [INF, 1.0], [1.0, 0.0], 0, -5e8),
    # x0, x1 free (cost 0), x2 in [0, 10] (cost 1); x0 + x2 >= 3, x0 - x1 = 1,
    # x1 >= 2.5 as a row
    Core('free_enter', 3, [[(0, 1.0), (2, 1.0)], [(0, 1.0), (1, -1.0)], [(1, 1.0)]],
         [3.0, 1.0, 2.5], [INF, 1.0, INF],
         [-INF, -INF, 0.0], [INF, INF, 10.0], [0.0, 0.0, 1.0], 0, 0.0),
    # x0 free (cost 1), x1, x2 in [0, 1]; x1 + x2 >= 5, x0 + x1 <= 100
    Core('art_infeas_grow', 3, [[(1, 1.0), (2, 1.0)], [(0, 1.0), (1, 1.0)]],
         [5.0, -INF], [INF, 100.0],
         [-INF, 0.0, 0.0], [INF, 1.0, 1.0], [1.0, 0.0, 0.0], 2, INF),
    # the same with the second row x0 - x1 >= -5e8
    Core('art_infeas_enter', 3, [[(1, 1.0), (2, 1.0)], [(0, 1.0), (1, -1.0)]],
         [5.0, -5e8], [INF, INF],
         [-INF, 0.0, 0.0], [INF, 1.0, 1.0], [1.0, 0.0, 0.0], 2, INF),
    # min x0 + x1, x in [0, 10], two identical rows x0 + x1 >= 3
    Core('ties', 2, [[(0, 1.0), (1, 1.0)], [(0, 1.0), (1, 1.0)]],
         [3.0, 3.0], [INF, INF],
         [0.0, 0.0], [10.0, 10.0], [1.0, 1.0], 0, 3.0),
    # min x0 + 2 x1, x0 free, x1 >= 0; x0 + 2 x1 >= 2: x0 starts on its
    # artificial lower bound, x1 enters (the larger pivot of a tied ratio) and
    # takes x0's reduced cost to zero
    Core('box_release', 2, [[(0, 1.0), (1, 2.0)]], [2.0], [INF],
         [-INF, 0.0], [INF, INF], [1.0, 2.0], 0, 2.0),
    # x0, x1 >= 0, x2, x3 free; x0 - x1 <= 1, 1 <= x1 + x2 <= 4, x2 - x3 >= 0
    Core('rays', 4, [[(0, 1.0), (1, -1.0)], [(1, 1.0), (2, 1.0)], [(2, 1.0), (3, -1.0)]],
         [-INF, 1.0, 0.0], [1.0, 4.0, INF],
         [0.0, 0.0, -INF, -INF], [INF, INF, INF, INF], [1.0, 1.0, 0.5, 0.0], 0, 0.5),
]}

# K3PW keeps B0^-1 (8 m^2 bytes) and eight waves' column state in 160 KiB of
# LDS: with n = m + 8 it fits up to m = 115, so 112 rows is the shape near its
# end; at 128 rows (its nominal limit) auto mode runs K3L
K3PW_ROWS = 112

# row counts: bare, one wave, the K3 / K3L boundary (64 | 65), K3PW's last
# shapes (112; 128 | 129), K3L's one-wave / four-wave boundary (256 | 257), 300
ROWS = (3, 40, 64, 65, K3PW_ROWS, 128, 129, 256, 257, 300)


def columns_for(m):
    """Padded column count: within 20 of m, and n + m <= 256 where a
    product-form kernel (m <= 128) has to hold every column in four slots."""
    return 120 if m == 128 else m + 8


def stride_of(m):
    """K3L gives column j to thread j % kT; K3, K3P and K3PW stride by 64."""
    return 64 if m <= 256 else 256


def _spread(k, size, big):
    """k indices in different waves, the last one at the end."""
    if big:                      # m > 256: four waves of rows
        at = [70, 200, 1, 140]
    else:
        at = [size // 4 + 1, (2 * size) // 3 + 1, 1, size // 2]
    at = at[:k - 1] + [size - 1]
    assert len(set(at)) == k and max(at) < size, (k, size, at)
    return at


def _strided(k, size, kT, start=3):
    """k indices in one lane, one stride apart while they fit, the rest
    counted down from the end."""
    at = [start + i * kT for i in range(k) if start + i * kT < size]
    j = size - 1
    while len(at) < k:
        if j not in at:
            at.append(j)
        j -= 1
    return at


def placements(core, m):
    """[(tag, row_at, col_at)] for core at m rows: one placement spread over
    the waves, one with rows and columns in the same lane a stride apart."""
    mr = len(core.rows)
    if m == 3:
        return [('bare', list(range(mr)), list(range(core.n)))]
    n, kT = columns_for(m), stride_of(m)
    out = [('spread', _spread(mr, m, m > 256), _spread(core.n, n, m > 256))]
    if m > 64:     # a second index in the same lane exists
        out.append(('stride', _strided(mr, m, kT), _strided(core.n, n, kT)))
    return out


def embed(core, m, n, row_at, col_at):
    """core's rows at row_at and columns at col_at of an m x n LP whose other
    columns lie in [0, 1] at zero cost and whose other rows read x_pad <= 2."""
    mr = len(core.rows)
    assert len(row_at) == mr and len(col_at) == core.n
    assert m >= mr and n >= core.n and (m == mr or n > core.n)
    pad = [j for j in range(n) if j not in col_at]
    rows = [None] * m
    rlo = np.full(m, -INF)
    rhi = np.full(m, 2.0)
    vlb = np.zeros(n)
    vub = np.ones(n)
    obj = np.zeros(n)
    for i, r in enumerate(row_at):
        rows[r] = [(col_at[j], a) for j, a in core.rows[i]]
        rlo[r], rhi[r] = core.rlo[i], core.rhi[i]
    k = 0
    for r in range(m):
        if rows[r] is None:
            rows[r] = [(pad[k % len(pad)], 1.0)]
            k += 1
    for j, c in enumerate(col_at):
        vlb[c], vub[c], obj[c] = core.vlb[j], core.vub[j], core.obj[j]
    return from_rows(f'{core.name}_m{m}', n, rows, rlo, rhi, vlb, vub,
                     np.full(n, CONTINUOUS, dtype=np.int32), obj)


Case = collections.namedtuple('Case', 'id core m p col_at row_at')


@functools.lru_cache(maxsize=None)
def all_cases():
    out = []
    for core in CORES.values():
        for m in ROWS:
            for tag, row_at, col_at in placements(core, m):
                mm = len(core.rows) if m == 3 else m
                nn = core.n if m == 3 else columns_for(m)
                p = embed(core, mm, nn, row_at, col_at)
                out.append(Case(f'{core.name}-{m}-{tag}', core, mm, p, tuple(col_at),
                                tuple(row_at)))
    return tuple(out)


def case_ids():
    return [c.id for c in all_cases()]


def case(cid):
    return next(c for c in all_cases() if c.id == cid)


def pfi_caps(m):
    """The eta-file caps the product-form kernels run with a shared warm
    start (Context.oracle_pfi): K3P's 16 and 32 for m <= 64, K3PW's for
    64 < m <= 128, none beyond (no kernel runs the product form there)."""
    from minotaur_amd.runtime import LP_PFI_MAX, LP_PFI_WIDE_MAX
    if m <= 64:
        return (16, LP_PFI_MAX)
    if m <= 128:
        return (LP_PFI_WIDE_MAX,)
    return ()


def bound_lps(c):
    """(cols, signs): min +-x_j over the core's columns."""
    cols = np.repeat(np.asarray(c.col_at, dtype=np.int32), 2)
    signs = np.tile([1.0, -1.0], len(c.col_at))
    return cols, signs


def new_objective(c):
    """Another objective on the core's columns (a warm basis without reduced
    costs: HipLPEngine after changeObj)."""
    import dataclasses
    obj = np.zeros(c.p.n)
    for k, j in enumerate(c.col_at):
        obj[j] = (-1.0) ** k * (0.5 + 0.25 * k)
    return dataclasses.replace(c.p, obj=obj)


def knapsack_bound_lps():
    """The golden knapsack LP (n = 18, m = 37, nine free columns) and its 36
    bound LPs min +-x_j."""
    p, _ = load_lp('knapsack')
    cols = np.repeat(np.arange(p.n, dtype=np.int32), 2)
    signs = np.tile([1.0, -1.0], p.n)
    return p, cols, signs


# ---- references, computed once per process and left unchanged ---------------
def _frozen(*arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def highs_cold(cid):
    return oracle.highs(case(cid).p)


@functools.lru_cache(maxsize=None)
def highs_bounds(cid):
    """HiGHS (status, objective) of every bound LP of a case ('knapsack': the
    golden LP's)."""
    if cid == 'knapsack':
        p, cols, signs = knapsack_bound_lps()
    else:
        p = case(cid).p
        cols, signs = bound_lps(case(cid))
    out = []
    for j, s in zip(cols, signs):
        cv = np.zeros(p.n)
        cv[j] = s
        out.append(oracle.highs_obj(p, cv))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def highs_new_objective(cid):
    return oracle.highs(new_objective(case(cid)))


@functools.lru_cache(maxsize=None)
def root(cid):
    """The oracle's root solve of a case ('knapsack': the golden LP):
    (status, objective, x, oracle.WarmStart)."""
    p = knapsack_bound_lps()[0] if cid == 'knapsack' else case(cid).p
    st, obj, x, _, _, ws = oracle.dual_simplex_root(p)
    _frozen(x, ws.head, ws.st, ws.binv, ws.d)
    return st, obj, x, ws


@functools.lru_cache(maxsize=None)
def warm_boxes(cid):
    """(LB, UB) [1 + 2 k][n] for a case whose root is optimal: the root box,
    then each of the core's k columns cut off half a unit below and above
    its root value (a branching step: the warm solves that pivot)."""
    c = case(cid)
    st, _, x, _ = root(cid)
    assert st == 0
    k = len(c.col_at)
    LB = np.tile(c.p.vlb, (1 + 2 * k, 1))
    UB = np.tile(c.p.vub, (1 + 2 * k, 1))
    for t, j in enumerate(c.col_at):
        UB[1 + 2 * t, j] = x[j] - 0.5
        LB[2 + 2 * t, j] = x[j] + 0.5
    return _frozen(LB, UB)


@functools.lru_cache(maxsize=None)
def highs_warm_boxes(cid):
    LB, UB = warm_boxes(cid)
    return tuple(oracle.highs(case(cid).p, LB[b], UB[b]) for b in range(LB.shape[0]))


def residual(p, x, lb=None, ub=None):
    """Largest violation of a row or a true column bound at x, each relative
    to its scale max(1, |bound|, sum |a_ij x_j|)."""
    lb = p.vlb if lb is None else lb
    ub = p.vub if ub is None else ub
    worst = 0.0
    for i in range(p.m):
        s, e = p.rowptr[i], p.rowptr[i + 1]
        t = p.val[s:e] * x[p.colidx[s:e]]
        act, scale = t.sum(), max(1.0, np.abs(t).sum())
        for b, v in ((p.rlo[i], p.rlo[i] - act), (p.rhi[i], act - p.rhi[i])):
            if np.isfinite(b):
                worst = max(worst, v / max(scale, abs(b)))
    for j in range(p.n):
        for b, v in ((lb[j], lb[j] - x[j]), (ub[j], x[j] - ub[j])):
            if np.isfinite(b):
                worst = max(worst, v / max(1.0, abs(b), abs(x[j])))
    return worst
