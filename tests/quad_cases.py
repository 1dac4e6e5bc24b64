"""Named inputs of K2 (minotaur_amd/csrc/quad_fbbt.hip) for
tests/test_quad_cases_cpu.py and tests/test_quad_cases_gpu.py: data only.

Every case is ``(QuadProblem, LB, UB, rows, incumbent, qt, mod_cap)`` with at
most 192 boxes.  The micro cases are hand-built (at most 6 original
variables) and each names, in its docstring, the arm of the kernel (and of
its C restatement oracle/quad_fbbt.c) it is there for; the seeded cases are
random_qcqp shapes beyond 64 and 128 variables; slow_* are the two
slow-contraction problems (mod-log overflow, propagation cap) and wide has
registry variables beyond the 1e12 default-bound threshold.

Cases are built once per process and are read-only."""
import functools
import math

import numpy as np

import oracle
from minotaur_amd.quad import (QuadProblem, from_functions, objective_at, random_qcqp,
                               random_quad_boxes)

INF = math.inf
BIN, INT, IBIN, IINT, C = 0, 1, 2, 3, 4   # Types.h VariableType
LDS_STRIDE = 65 * 8                       # bytes per [var] row of the LDS node state


def max_terms(qp):
    """Longest term list of the two tightenQuad_ programs that mgpu_load_quad
    compiles (with and without the objective), at least 1: a function takes
    part when it has a square and a linear part and some univariate term
    a x^2 + b x has been seen so far; linear terms of variables that were
    univariate so far are left out (getQfLfBnds_, QuadHandler.cpp:2361-2427)."""
    best = 1
    for with_obj in (False, True):
        isq, seen = set(), False
        order = ([qp.ncon] if with_obj and qp.has_obj else []) + list(range(qp.ncon))
        for c in order:
            q = range(qp.qptr[c], qp.qptr[c + 1])
            lin = [int(qp.lvar[k]) for k in range(qp.lptr[c], qp.lptr[c + 1])]
            if not lin or not any(qp.qv1[k] == qp.qv2[k] for k in q):
                continue
            for k in q:
                if qp.qv1[k] == qp.qv2[k] and int(qp.qv1[k]) in lin:
                    isq.add(int(qp.qv1[k]))
                    seen = True
            if seen:
                best = max(best, len(q) + sum(v not in isq for v in lin))
    return best


def lds_bytes(qp):
    """quad_lds_bytes: the LDS variant's node state, (2 nv + 2 maxt) x 520 B."""
    return (2 * qp.nv + 2 * max_terms(qp)) * LDS_STRIDE


def linear_only(qp):
    """Original variables with a linear weight somewhere and in no product."""
    return sorted(set(qp.lvar.tolist()) - set(qp.qv1.tolist()) - set(qp.qv2.tolist()))


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)


def _case(qp, LB, UB, incumbent=None, qt=1, mod_cap=64, rows=None):
    LB = np.ascontiguousarray(LB, dtype=np.float64)
    UB = np.ascontiguousarray(UB, dtype=np.float64)
    rows = oracle.quad_root_rows(qp) if rows is None else np.asarray(rows, dtype=np.float64)
    assert LB.shape == UB.shape and LB.shape[1] == qp.nv and LB.shape[0] <= 192
    _freeze(LB, UB, rows)
    return qp, LB, UB, rows, incumbent, qt, mod_cap


def _boxes(qp, edits):
    """One box per entry of edits: the root box with {var: (l, u)} applied."""
    LB = np.tile(qp.vlb, (len(edits), 1))
    UB = np.tile(qp.vub, (len(edits), 1))
    for b, e in enumerate(edits):
        for v, (l, u) in e.items():
            LB[b, v], UB[b, v] = l, u
    return LB, UB


# --------------------------------------------------------------------------
# micro cases
# --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def univar_linear():
    """calc_univar's |a| <= 1e-6 arm (bounds ly / b, uy / b): a of 1e-8 (the
    loader's smallest), 9e-7 and exactly +-1e-6 (the edge of <=), each with a
    linear term of either sign; a = 1.0000001e-6 next to it takes the convex
    arm."""
    vt = [C] * 6
    lb = [-4.0, -3.0, -5.0, -2.0, -6.0, -1.0]
    ub = [5.0, 6.0, 4.0, 7.0, 3.0, 2.0]
    A = [1e-8, 9e-7, 1e-6, -1e-6, -9e-7]
    Bc = [1.5, -2.0, 0.75, 1.25, -0.5]
    funcs, clb, cub = [], [], []
    for v, (a, b) in enumerate(zip(A, Bc)):
        funcs.append(({v: b, 5: 1.0}, {(v, v): a}))
        clb.append(-1.0)
        cub.append(1.5)
    funcs.append(({0: 1.0, 5: -1.0}, {(0, 0): 1.0000001e-6}))
    clb.append(-0.5)
    cub.append(0.75)
    qp = from_functions('univar_linear', vt, lb, ub, funcs, clb, cub)
    LB, UB = _boxes(qp, [{}, {5: (0.0, 0.0)}, {5: (0.5, 0.5)}, {5: (-1.0, -0.25)},
                         {5: (1.0, 2.0), 0: (0.0, 5.0)}, {5: (0.0, 0.0), 1: (-3.0, -1.0)},
                         {5: (0.0, 0.0), 3: (1.0, 7.0), 4: (-6.0, -4.0)}])
    return _case(qp, LB, UB)


# 1e-6 - 2^-22 is a double, and 2^-22 + it is 1e-6 exactly
_B_EDGE = 2.0 ** -11
_UY_EDGE = 1e-6 - 2.0 ** -22
assert _B_EDGE * _B_EDGE + _UY_EDGE == 1e-6


@functools.lru_cache(maxsize=None)
def univar_tangent():
    """calc_univar's tangent arms |delta| <= 1e-6, delta = b b + 4 a uy
    (a > 0) or b b + 4 a ly (a < 0): delta exactly 0, +-5e-7, exactly 1e-6
    (a = 1/4, b = 2^-11: the edge of <=), and +-2.4e-6 next to them (two
    roots; delta < -1e-6 is the infeasible return), on both curvatures.
    x1 in [0, 0] makes uy = cub and ly = clb exactly."""
    vt = [C, C]
    lb, ub = [-3.0, -1.0], [3.0, 1.0]
    conv = ({0: 2.0, 1: 1.0}, {(0, 0): 1.0})      # x0^2 + 2 x0 + x1: min -1
    conc = ({0: 2.0, 1: 1.0}, {(0, 0): -1.0})     # -x0^2 + 2 x0 + x1: max 1
    edge = ({0: _B_EDGE, 1: 1.0}, {(0, 0): 0.25})
    edgec = ({0: _B_EDGE, 1: 1.0}, {(0, 0): -0.25})
    rows = []
    for d in (0.0, 1.25e-7, -1.25e-7, 6e-7, -6e-7):
        rows.append((conv, -INF, -1.0 + d))
        rows.append((conc, 1.0 - d, INF))
    rows.append((edge, -INF, _UY_EDGE))
    rows.append((edgec, -_UY_EDGE, INF))
    out = []
    for i, (f, l, u) in enumerate(rows):
        qp = from_functions(f'univar_tangent{i}', vt, lb, ub, [f], [l], [u])
        LB, UB = _boxes(qp, [{1: (0.0, 0.0)}, {1: (0.0, 0.0), 0: (-3.0, 0.5)},
                             {1: (0.0, 0.0), 0: (-0.5, 3.0)}, {}])
        out.append(_case(qp, LB, UB))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def univar_open():
    """calc_univar with one side of the row open after the forward pass:
    cub = +inf with a > 0 (x1 unbounded below, so uy = +inf and ly finite)
    and clb = -inf with a < 0 (x1 unbounded above), x0's lx and ux on either
    side of the roots lb2 and ub2; the two-sided rows next to them put lx and
    ux on either side of the inner roots of the finite branches."""
    vt = [C, C]
    lb, ub = [-8.0, -4.0], [8.0, 4.0]
    funcs = [({0: 2.0, 1: 1.0}, {(0, 0): 1.0}),     # x0^2 + 2 x0 + x1 >= 5
             ({0: 2.0, 1: 1.0}, {(0, 0): -1.0}),    # -x0^2 + 2 x0 + x1 <= -5
             ({0: -1.0, 1: 0.5}, {(0, 0): 0.5}),    # 3 <= x0^2/2 - x0 + x1/2 <= 9
             ({0: 1.0, 1: 0.5}, {(0, 0): -0.5})]    # -9 <= -x0^2/2 + x0 + .. <= -3
    clb = [5.0, -INF, 3.0, -9.0]
    cub = [INF, -5.0, 9.0, -3.0]
    out = []
    for i in range(4):
        qp = from_functions(f'univar_open{i}', vt, lb, ub, [funcs[i]], [clb[i]], [cub[i]])
        x1 = [(-INF, 2.0), (-2.0, INF), (0.0, 0.0), (0.0, 0.0)][i]
        # roots of the open rows: x0^2 + 2 x0 = 3 -> -3, 1;  -x0^2 + 2 x0 = -3 -> -1, 3
        ed = []
        for x0 in ((-8.0, 8.0), (-2.0, 8.0), (-8.0, 0.5), (2.0, 8.0), (-8.0, -4.0),
                   (0.0, 8.0), (-8.0, 2.0), (4.0, 8.0), (-8.0, -2.0), (-1.0, 2.0),
                   (1.0, 3.0), (-3.0, 1.0)):
            ed.append({0: x0, 1: x1})
        ed.append({0: (-8.0, 8.0), 1: (-INF, INF)})
        ed.append({0: (-2.0, 8.0), 1: (-4.0, 4.0)})
        LB, UB = _boxes(qp, ed)
        out.append(_case(qp, LB, UB))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def square_neg():
    """prop_sqr with U(y) below zero: U(y) = -1 and just past -1e-8 (refused
    by update_pbounds), U(y) in [-1e-8, 0) (x goes to [0, 0]; 'uy < -1e-8' is
    not 'uy < 0'), and U(y) in (0, 1e-8]."""
    qp = from_functions('square_neg', [C, INT], [-2.0, -3.0], [3.0, 3.0],
                        [({0: 1.0, 1: 1.0}, {(0, 0): 1.0, (1, 1): 1.0})], [-INF], [40.0])
    y0, y1 = int(qp.sq_y[0]), int(qp.sq_y[1])
    LB, UB = _boxes(qp, [{y0: (-2.0, -1.0)}, {y0: (-1.0, -5e-9)}, {y0: (-1.0, -1e-8)},
                         {y0: (-1.0, np.nextafter(-1e-8, -1.0))}, {y0: (-1.0, 5e-9)},
                         {y0: (-1.0, 0.0)}, {y1: (-1.0, -5e-9)}, {y1: (-1.0, 0.5)},
                         {y0: (-1.0, -5e-9), 0: (0.5, 3.0)}, {y0: (-1.0, 1e-8)}, {}])
    return _case(qp, LB, UB)


@functools.lru_cache(maxsize=None)
def pure_square():
    """calc_var_bnd's pure-square branch (a square with no linear term of its
    variable, next to a univariate term): qub < -1e-8 (infeasible), qub in
    [-1e-8, 1e-8] (x to [0, 0]) and qub > 1e-8 with lx on either side of
    -sqrt(qlb), for a positive and a negative coefficient."""
    vt = [C, C, C]
    lb, ub = [-2.0, 0.0, -2.0], [2.0, 2.0, 2.0]
    out = []
    for i, cu in enumerate((-5e-7, -5e-9, 5e-9, 5e-7, 1.0)):
        # x0^2 + x1^2 + x1 <= cu: the forward lower bound of x1^2 + x1 is 0
        qp = from_functions(f'pure_square{i}', vt, lb, ub,
                            [({2: 1.0}, {(0, 0): 1.0}),      # no univariate term yet: skipped
                             ({1: 1.0}, {(0, 0): 1.0, (1, 1): 1.0}),
                             ({1: -1.0}, {(1, 1): -1.0, (2, 2): -2.0})],
                            [-INF, -INF, -2.0 * cu], [0.5, cu, INF])
        LB, UB = _boxes(qp, [{}, {0: (-2.0, 0.0)}, {0: (0.0, 2.0)}, {0: (0.5, 2.0)},
                             {0: (1e-4, 2.0)}, {0: (-2.0, -1e-4)},
                             {2: (0.25, 2.0)}, {0: (-2.0, -0.5), 2: (-2.0, -0.25)}])
        out.append(_case(qp, LB, UB))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def implied_int():
    """update_pbounds' rounding for ImplBin (2) and ImplInt (3) variables:
    fractional bounds from a square root, a quotient and a univariate row are
    ceiled / floored exactly as for Binary and Integer."""
    vt = [IBIN, IINT, IINT, C, BIN, INT]
    lb = [0.0, -3.0, 1.0, -2.0, 0.0, -4.0]
    ub = [1.0, 4.0, 6.0, 5.0, 1.0, 4.0]
    funcs = [({1: 1.0, 3: 1.0}, {(1, 1): 1.0, (0, 2): 1.0}),
             ({2: -1.0, 0: 0.5}, {(2, 2): 0.5, (1, 3): 1.0}),
             ({5: 1.0, 4: 2.0}, {(5, 5): 1.0, (2, 2): 1.0})]
    qp = from_functions('implied_int', vt, lb, ub, funcs, [-INF, -2.0, 1.5], [7.5, 6.3, 20.5])
    LB, UB = random_quad_boxes(qp, 40, 31, edge=True)
    LB, UB = LB.copy(), UB.copy()
    LB[0], UB[0] = qp.vlb, qp.vub
    ysq = {int(x): int(y) for x, y in zip(qp.sq_x, qp.sq_y)}
    for b in range(1, 40, 3):     # shrunk y = x^2 of the implied integers: sqrt is fractional
        for x in (1, 2):
            UB[b, ysq[x]] = min(UB[b, ysq[x]], 2.5 + 0.7 * b)
    return _case(qp, LB, UB)


@functools.lru_cache(maxsize=None)
def unbounded_linear():
    """sum_except1 with ninf of 1, 2 and 3 (one, two or three unbounded
    linear-only variables x3, x4, x5 in one row), the infinite term as the
    current term and as another term; term_bnds' infinite arms for either
    coefficient sign; update_pbounds with L = -inf or U = +inf and a finite
    new bound, both together and one at a time."""
    vt = [C] * 6
    lb = [-3.0, -2.0, 0.0, -5.0, -5.0, -5.0]
    ub = [4.0, 3.0, 4.0, 5.0, 5.0, 5.0]
    funcs = [({0: 1.0, 3: 1.0, 4: -2.0, 5: 0.5}, {(0, 0): 1.0, (1, 2): 1.0}),
             ({1: -1.0, 3: -1.5, 4: 1.0}, {(1, 1): 2.0}),
             ({2: 1.0, 5: -1.0}, {(2, 2): -1.0, (0, 0): 0.5})]
    qp = from_functions('unbounded_linear', vt, lb, ub, funcs, [-4.0, -INF, -6.0],
                        [9.0, 5.0, INF], obj=({0: 1.0, 3: 1.0}, {(0, 0): 1.0}))
    U = (-INF, INF)
    ed = [{}]
    for v in (3, 4, 5):
        ed += [{v: U}, {v: (-INF, 5.0)}, {v: (-5.0, INF)}, {v: (-INF, -1.0)}, {v: (1.0, INF)}]
    ed += [{3: U, 4: U}, {3: U, 5: U}, {4: U, 5: U}, {3: U, 4: U, 5: U},
           {3: (-INF, 0.0), 4: (-INF, 0.0)}, {3: (0.0, INF), 4: (-INF, 0.0)},
           {3: (-INF, 2.0), 4: (-2.0, INF), 5: U}, {3: U, 4: (-INF, 1.0), 5: (-1.0, INF)},
           {3: (-INF, 5.0), 4: (-5.0, INF), 5: (-INF, 5.0)},
           {3: U, 0: (0.0, 0.0)}, {4: U, 1: (1.0, 1.0)}, {5: U, 2: (2.0, 2.0), 0: (1.0, 1.0)}]
    LB, UB = _boxes(qp, ed)
    return _case(qp, LB, UB, incumbent=12.0)


@functools.lru_cache(maxsize=None)
def rel_tol():
    """update_pbounds' relative tolerance: a new bound past the old one by
    more than 1e-8 but less than 1e-7 |old| is not taken, on the lower side,
    the upper side and both, alone and next to a side that is taken."""
    vt = [C, C, C]
    lb, ub = [-1.0, 1000.0, -3000.0], [1.0, 2000.0, -1000.0]
    # x0 in [0, 0] makes the row x1 + x2-free: clb <= x1 <= cub
    funcs = [({0: 1.0, 1: 1.0}, {(0, 0): 1.0}), ({0: 1.0, 2: 1.0}, {(0, 0): 1.0})]
    out = []
    eps, big = 5e-5, 0.5
    for i, (dl, du) in enumerate(((eps, eps), (eps, big), (big, eps), (big, big), (eps, 0.0),
                                  (0.0, eps), (big, 0.0), (0.0, big))):
        qp = from_functions(f'rel_tol{i}', vt, lb, ub, funcs,
                            [1000.0 + dl if dl else -INF, -3000.0 + dl if dl else -INF],
                            [2000.0 - du if du else INF, -1000.0 - du if du else INF])
        LB, UB = _boxes(qp, [{0: (0.0, 0.0)}, {}])
        out.append(_case(qp, LB, UB))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def objective_forms():
    """tightenQuad_'s objective leg with an incumbent (the choice between the
    two compiled programs): no objective at all; an objective without a
    square; one with a square and no linear part; one with a square and a
    linear part but no univariate term (getQfLfBnds_ returns false); and a
    univariate one, with an incumbent that cuts and one that is +inf."""
    vt = [C, C, INT]
    lb, ub = [-3.0, -2.0, -2.0], [4.0, 3.0, 5.0]
    funcs = [({0: 1.0, 2: 1.0}, {(0, 0): 1.0, (1, 1): 1.0}),
             ({1: 2.0, 2: -1.0}, {(1, 1): -1.0, (0, 1): 0.5})]
    clb, cub = [-INF, -3.0], [9.0, INF]
    objs = [None, ({0: 1.0}, {(0, 1): 1.0}), ({}, {(0, 0): 1.0, (0, 1): 1.0}),
            ({2: 1.0}, {(0, 0): 1.0}), ({0: -1.0, 2: 1.0}, {(0, 0): 1.0}),
            ({0: -1.0, 2: 1.0}, {(0, 0): 1.0})]
    out = []
    for i, obj in enumerate(objs):
        qp = from_functions(f'objective_forms{i}', vt, lb, ub, funcs, clb, cub, obj=obj,
                            obj_const=0.25)
        LB, UB = random_quad_boxes(qp, 12, 40 + i, edge=True)
        out.append(_case(qp, LB, UB, incumbent=None if i == 5 else 1.5))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def inverted_tol():
    """bounds_on_recip's '|l0| < 1e-10 && u0 < 0' arm.  update_pbounds takes a
    new lower bound up to 1e-8 above the upper one: row 0 moves x0's lower
    bound from -1 to -5e-11, past its upper bound -2e-10, and row 1's
    bilinear term x0 x1 then divides by that box."""
    vt = [C, C, C, C]
    lb, ub = [-1.0, 1.0, -1.0, -1.0], [1.0, 2.0, 1.0, 1.0]
    funcs = [({0: 1.0, 2: 1.0}, {(2, 2): 1.0}),              # x0 + x2^2 + x2 >= -5e-11
             ({3: 1.0}, {(3, 3): 1.0, (0, 1): 1.0})]          # x3^2 + x3 + x0 x1 <= 1
    qp = from_functions('inverted_tol', vt, lb, ub, funcs, [-5e-11, -INF], [INF, 1.0])
    LB, UB = _boxes(qp, [{0: (-1.0, -2e-10), 2: (0.0, 0.0)}, {2: (0.0, 0.0)}, {},
                         {0: (-1.0, -2e-10), 2: (0.0, 0.0), 3: (0.5, 1.0)}])
    return _case(qp, LB, UB)


@functools.lru_cache(maxsize=None)
def mccormick_corners():
    """up_rows' rebuild tests corner by corner: a row state that is not that
    of an ancestor box (the root rows plus noise), so that each of the three
    corners of each McCormick row, and each end of a secant, is the only one
    that asks for the rebuild in some node."""
    qp = random_qcqp(11, nv0=6, ncon=4)
    LB, UB = random_quad_boxes(qp, 96, 12, edge=False)
    rng = np.random.default_rng(13)
    rows = oracle.quad_root_rows(qp)
    rows = rows + rng.uniform(-1.5, 1.5, size=rows.shape)
    # by hand on [0, 1]^2: row 1 fails at (u0, u1) only, row 3 at (u0, l1) only
    hp = from_functions('mccormick_hand', [C, C], [0.0, 0.0], [1.0, 1.0],
                        [({0: 1.0}, {(0, 1): 1.0})], [-INF], [2.0])
    hrows = np.array([0.0, 0.0, 0.0, 0.2, 0.2, 0.0, -1.0, 0.0, 0.0, -0.5, 0.25, 0.0])
    hLB, hUB = _boxes(hp, [{}, {0: (0.0, 0.5)}, {1: (0.5, 1.0)}, {0: (0.25, 1.0), 1: (0.0, 0.5)}])
    return _case(qp, LB, UB, rows=rows), _case(hp, hLB, hUB, rows=hrows)


# --------------------------------------------------------------------------
# seeded cases: nv beyond one and two staging trips, LDS need past 64 and 160 KiB
# --------------------------------------------------------------------------
# name -> (nv0, ncon, nv, quad_lds_bytes): pins against a drift of random_qcqp
SEEDED = {
    'seeded81': (40, 20, 81, 90480),
    'seeded142': (70, 40, 142, 153920),
    'seeded266': (120, 80, 266, 282880),
}


@functools.lru_cache(maxsize=None)
def seeded(name, B=160):
    """random_qcqp(7, ...) with edge boxes; in every third box the
    linear-only variables are unbounded on one or both sides."""
    nv0, ncon, nv, lds = SEEDED[name]
    qp = random_qcqp(7, nv0=nv0, ncon=ncon)
    assert qp.nv == nv, (name, qp.nv)
    assert lds_bytes(qp) == lds, (name, lds_bytes(qp))
    LB, UB = random_quad_boxes(qp, B, 700 + nv0, edge=True)
    LB, UB = LB.copy(), UB.copy()
    rng = np.random.default_rng(nv0)
    lo = linear_only(qp)
    for b in range(0, B, 3):
        for v in lo:
            r = rng.random()
            if r < 0.4:
                LB[b, v] = -INF
            elif r < 0.8:
                UB[b, v] = INF
            else:
                LB[b, v], UB[b, v] = -INF, INF
    x = 0.5 * (qp.vlb[:qp.nv0] + qp.vub[:qp.nv0])
    return _case(qp, LB, UB, incumbent=objective_at(qp, x), qt=1, mod_cap=96)


# --------------------------------------------------------------------------
# slow contraction: y2 = x0 x1 with x1 = c, y0 = x2 x3 with x3 = 1
# --------------------------------------------------------------------------
SLOW_CONVERGE_C = 0.999          # converges after about 11 500 passes, 23020 mods
SLOW_CAP_C = 1.0 - 1e-5          # about 690 000 passes away: the propagation cap
SLOW_LANES = (37, 64)            # in the first wave; alone in the ragged second wave


def slow_problem():
    i32 = lambda a: np.asarray(a, dtype=np.int32)
    f64 = lambda a: np.asarray(a, dtype=np.float64)
    # root box [0, 0]^4: the root row state is all zero
    return QuadProblem(name='slow', nv0=4, vtype=i32([C] * 4), vlb=f64([0, 0, 0, 0]),
                       vub=f64([0, 0, 0, 0]), sq_x=i32([]), sq_y=i32([]), bil_x0=i32([0, 2]),
                       bil_x1=i32([1, 3]), bil_y=i32([2, 0]), lptr=i32([0]), lvar=i32([]),
                       lval=f64([]), qptr=i32([0]), qv1=i32([]), qv2=i32([]), qval=f64([]),
                       clb=f64([]), cub=f64([]))


def slow_box(c):
    return np.array([0.0, c, 0.0, 1.0]), np.array([1.0, c, 1.0, 1.0])


@functools.lru_cache(maxsize=None)
def slow(c, lane, mod_cap=128):
    """65 nodes of the slow problem: 64 ordinary ones (x1 = c' <= 0.9 or an
    interval, x3 in [0.5, 1]: a few passes each) and, at ``lane``, the node
    whose bound on x0 shrinks by the factor c per pass."""
    qp = slow_problem()
    rng = np.random.default_rng(5)
    LB = np.zeros((65, 4))
    UB = np.ones((65, 4))
    for b in range(65):
        a, w = rng.uniform(0.1, 0.9), rng.uniform(0.0, 0.1) * (b % 2)
        LB[b, 1], UB[b, 1] = a, a + w
        LB[b, 3], UB[b, 3] = (1.0, 1.0) if b % 3 else (0.5, 1.0)
        if b % 5 == 0:
            UB[b, 0] = rng.uniform(0.2, 0.8)
        if b % 7 == 0:
            LB[b, 2] = 0.95          # x2 >= 0.95 > x0 x1: infeasible
    LB[lane], UB[lane] = slow_box(c)
    return _case(qp, LB, UB, qt=0, mod_cap=mod_cap)    # the root rows: all +-0


# --------------------------------------------------------------------------
# registry variables beyond 1e12 (addDefaultBounds_, reported as status 3)
# --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def wide():
    """Boxes where the x of a square or a factor of a bilinear has a bound
    beyond +-1e12: with rows that need a rebuild there (status 3) and rows
    that do not (the rows of that very box: status 0), wide on one variable
    and on several, and infeasible ones (status stays 1)."""
    vt = [C, C, C, INT]
    lb, ub = [-2.0, 1.0, -3.0, -2.0], [3.0, 4.0, 2.0, 5.0]
    funcs = [({0: 1.0}, {(0, 1): 1.0}),
             ({2: -1.5, 1: 0.5}, {(2, 2): 2.0, (0, 2): -1.0}),
             ({3: 1.0}, {(0, 0): -1.0, (3, 3): 0.5, (0, 1): 1.0})]
    # no row bounds |x0| from above, so a wide x0 stays wide
    qp = from_functions('wide', vt, lb, ub, funcs, [-INF, -1.0, -INF], [6.0, 3.0, 50.0])
    ysq = {int(x): int(y) for x, y in zip(qp.sq_x, qp.sq_y)}
    ybl = {(int(a), int(b)): int(y) for a, b, y in zip(qp.bil_x0, qp.bil_x1, qp.bil_y)}
    W = 1e13
    U = (-INF, INF)
    free = {ysq[0]: U, ybl[(0, 1)]: U, ybl[(0, 2)]: U}
    ed = [{},
          {0: (-W, 3.0), **free}, {0: (-2.0, W), **free}, {0: (-W, W), **free},
          {0: U, **free}, {0: (-2e12, 2e12), **free},
          {0: (-1e12, 1e12), **free},                       # exactly 1e12: not wide
          {0: (-W, 3.0), 1: (2.0, 3.0), **free},
          {0: (-W, W), **free, ysq[0]: (0.0, 4.0)},         # y pulls x back
          {0: (-W, W), **free, ysq[0]: (-3.0, -1.0)},       # infeasible
          {0: (-W, W), 2: (1.5, 2.0), 1: (1.0, 1.0), **free},
          {3: (-2.0, 5.0), 0: (-W, -1e12), **free},
          {0: (1e12, W), 3: (4.0, 5.0), **free},
          {2: (-3.0, -1.0)}, {1: (1.0, 2.0), 3: (0.0, 5.0)}]
    LB, UB = _boxes(qp, ed)
    # first the boxes with the row state of a box ten times wider in x0 (a
    # rebuild is due wherever x0 is finite), then the same boxes again with
    # the row state of their own propagated box (nothing is rebuilt)
    n = len(ed)
    rows = np.tile(oracle.quad_root_rows(qp), (2 * n, 1))
    for b in range(n):
        l, u = LB[b].copy(), UB[b].copy()
        if np.isfinite(l[0]) and np.isfinite(u[0]) and max(-l[0], u[0]) >= 1e12:
            l[0], u[0] = 10.0 * l[0], 10.0 * u[0]
            rows[b] = oracle.quad_root_rows(qp, l, u)
    o = oracle.quad_fbbt(qp, LB, UB, None, 1, rows[:n])
    for b in range(n):
        if np.isfinite(o.lb[b]).all() and np.isfinite(o.ub[b]).all():
            rows[n + b] = oracle.quad_root_rows(qp, o.lb[b], o.ub[b])
    return _case(qp, np.vstack([LB, LB]), np.vstack([UB, UB]), qt=1, mod_cap=64, rows=rows)


# --------------------------------------------------------------------------
# registry
# --------------------------------------------------------------------------
def _named(prefix, cs):
    return {f'{prefix}{i}': c for i, c in enumerate(cs)}


@functools.lru_cache(maxsize=None)
def micro_cases():
    d = {'univar_linear': univar_linear(), 'square_neg': square_neg(),
         'implied_int': implied_int(), 'unbounded_linear': unbounded_linear()}
    d.update(_named('univar_tangent', univar_tangent()))
    d.update(_named('univar_open', univar_open()))
    d.update(_named('pure_square', pure_square()))
    d.update(_named('rel_tol', rel_tol()))
    d.update(_named('objective_forms', objective_forms()))
    d['inverted_tol'] = inverted_tol()
    d.update(_named('mccormick_corners', mccormick_corners()))
    return d


@functools.lru_cache(maxsize=None)
def all_cases():
    """name -> case, every case the oracle can run to the end (slow_cap, whose
    slow node stops at the propagation cap, is apart: slow(SLOW_CAP_C, lane))."""
    d = dict(micro_cases())
    for name in SEEDED:
        d[name] = seeded(name)
    for lane in SLOW_LANES:
        d[f'slow_converge{lane}'] = slow(SLOW_CONVERGE_C, lane)
    d['wide'] = wide()
    return d


def reference_can_express(name):
    """The reference itself runs every case but those with a registry bound
    beyond 1e12 (it would add default bounds to its own state)."""
    return name != 'wide'


@functools.lru_cache(maxsize=None)
def oracle_result(name):
    """oracle.quad_fbbt of a case of all_cases(), computed once."""
    qp, LB, UB, rows, inc, qt, cap = all_cases()[name]
    r = oracle.quad_fbbt(qp, LB, UB, inc, qt, rows, cap)
    _freeze(r.lb, r.ub, r.rows, r.infeas, r.nmods, r.kind, r.idx, r.v1, r.v2)
    return r
