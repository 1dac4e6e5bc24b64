"""GPU parity of K3P on the paths whose instruction sequences the VALU trim
rewrote (DPP reductions without the dead "old" operand; the eta passes of
FTRAN, BTRAN, the primal recompute and the path replay), at small shapes.

Every case is the ``_both`` comparison of tests/test_lp_path_gpu.py against
oracle.dual_simplex_path: statuses, own pivot counts, objective bits, x bits,
the output path (length, columns) and the output statuses.  The oracle side
of a case (parents from the root basis, then both children of every parent
with a fractional integer column, each carrying its parent's path) is
computed once per module and shared; the children are derived from the
oracle's results, so the GPU's inputs do not depend on the GPU.

Covered: odd batch sizes (the odd tail of the sibling pairing and reuse),
eta caps around the 16 / 32 / 48-eta builds and the reinversion at a small
cap, a one-slot and a four-slot problem, and sparse etas (most eta products
exact zeros: boxes solved from the root basis).
"""
import functools
import math
import os

import numpy as np
import pytest

import oracle
from minotaur_amd.problem import LinProblem, random_boxes, random_mkp, random_problem
from minotaur_amd.runtime import LP_PFI_MAX, PATH_MAX

pytestmark = pytest.mark.gpu

INST = os.path.join(os.path.dirname(__file__), '..', 'minotaur_amd', 'instances')


@pytest.fixture(scope='module')
def ctx():
    from minotaur_amd.runtime import Context
    c = Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def _problem(name):
    if name in ('tls4_oa', 'tls4_lin'):
        return LinProblem.load(os.path.join(INST, name + '.npz'))
    if name == 'one_slot':      # n + m = 45: one column slot per lane
        return random_mkp(1, 40, 5)
    assert name == 'four_slot'  # n + m = 240: four column slots per lane
    return random_problem(1, n=200, m=40, density=0.1)


@functools.lru_cache(maxsize=None)
def _root(name):
    st, _, _, _, _, ows = oracle.dual_simplex_root(_problem(name))
    assert st == 0
    return ows


def _children(p, LB, UB, x, status, k, path, st):
    """Both children of every optimal node with a fractional integer column
    (the first one), each carrying its parent's final path: siblings are
    neighbours (2i, 2i + 1), as the batched tree pops them."""
    ints = np.isin(p.vtype, (0, 1))
    cl, cu, ck, cp, cs = [], [], [], [], []
    for b in np.nonzero(status == 0)[0]:
        fr = np.nonzero(ints & (np.abs(x[b] - np.round(x[b])) > 1e-6))[0]
        if fr.size == 0:
            continue
        j, v = fr[0], x[b][fr[0]]
        for up in (0, 1):
            lo, hi = LB[b].copy(), UB[b].copy()
            if up:
                lo[j] = math.ceil(v)
            else:
                hi[j] = math.floor(v)
            cl.append(lo)
            cu.append(hi)
            ck.append(k[b])
            cp.append(path[b])
            cs.append(st[b])
    return (np.array(cl), np.array(cu), np.array(ck, dtype=np.int32),
            np.array(cp, dtype=np.uint32).reshape(-1, PATH_MAX), np.array(cs, dtype=np.int8))


@functools.lru_cache(maxsize=None)
def _family(name, nbox, seed, cap):
    """(parents, children): each the inputs (LB, UB, k, path, st) and the
    oracle's outputs of one batch under eta cap ``cap`` (inherit =
    min(cap, PATH_MAX)).  Never modified by the tests."""
    p, ows = _problem(name), _root(name)
    inherit = min(cap, PATH_MAX)
    LB, UB = random_boxes(p, nbox, seed)
    f = oracle.linear_fbbt(p, LB, UB, None)
    keep = f.infeas == 0
    LB, UB = f.lb[keep], f.ub[keep]
    B, N = LB.shape[0], p.n + p.m
    pin = (LB, UB, np.zeros(B, np.int32), np.zeros((B, PATH_MAX), np.uint32),
           np.zeros((B, N), np.int8))
    po = oracle.dual_simplex_path(p, *pin[:2], ows, *pin[2:], cap, inherit, nthreads=8)
    cin = _children(p, LB, UB, po[3], po[0], po[4], po[5], po[6])
    co = oracle.dual_simplex_path(p, *cin[:2], ows, *cin[2:], cap, inherit, nthreads=8)
    return (pin, po), (cin, co)


def _ws(name):
    from minotaur_amd.runtime import WarmStart
    ows = _root(name)
    return WarmStart(ows.head, ows.st, ows.d, np.ascontiguousarray(ows.binv.T))


def _same(g, gk, gp, gs, o):
    assert np.array_equal(g.status, o[0])
    assert np.array_equal(g.iters, o[2])
    ok = o[0] == 0
    assert np.array_equal(g.obj[ok].view(np.int64), o[1][ok].view(np.int64))
    assert np.array_equal(g.x[ok].view(np.int64), o[3][ok].view(np.int64))
    assert np.array_equal(gk, o[4])
    for b in np.nonzero(gk > 0)[0]:
        assert np.array_equal(gp[b, :gk[b]], o[5][b, :gk[b]])
        assert np.array_equal(gs[b], o[6][b])


class _cap:
    """The eta-file cap of the LP calls inside; the default cap afterwards."""

    def __init__(self, ctx, cap):
        self.ctx, self.cap = ctx, cap

    def __enter__(self):
        self.ctx.set_lp_pfi(self.cap)

    def __exit__(self, *a):
        self.ctx.set_lp_pfi(LP_PFI_MAX)


def _run(ctx, name, batch, cap, sl=slice(None)):
    """One batch (inputs, oracle outputs), or its slice ``sl`` solved as a
    batch of its own: an LP's result does not depend on its batch."""
    ins, o = batch
    with _cap(ctx, cap):
        g, gk, gp, gs = ctx.lp_solve_path(ins[0][sl], ins[1][sl], _ws(name), ins[2][sl],
                                          ins[3][sl], ins[4][sl], min(cap, PATH_MAX))
    _same(g, gk, gp, gs, tuple(a[sl] for a in o))


@pytest.mark.parametrize('nb', [1, 2, 3, 129])
def test_odd_batches_of_children(ctx, nb):
    """tls4-OA children with their parents' paths in batches of 1, 2, 3 and
    129: whole sibling pairs (the second reuses the first's column
    replacements) and an odd tail."""
    ctx.load(_problem('tls4_oa'))
    _, ch = _family('tls4_oa', 300, 41, LP_PFI_MAX)
    (cin, co) = ch
    assert cin[0].shape[0] >= 129 + 1 and (cin[2][:129] > 0).mean() > 0.5
    _run(ctx, 'tls4_oa', ch, LP_PFI_MAX, slice(0, nb))
    # the same count from an odd offset: pairs (2i + 1, 2i + 2) are no siblings
    _run(ctx, 'tls4_oa', ch, LP_PFI_MAX, slice(1, 1 + nb))


@pytest.mark.parametrize('cap', [3, 16, 17, 32, 33, 48])
def test_eta_caps(ctx, cap):
    """Caps at and next to the 16-, 32- and 48-eta builds' limits, and cap 3,
    where the file fills at once (reinversion, dense continuation)."""
    ctx.load(_problem('tls4_oa'))
    par, ch = _family('tls4_oa', 200, 42, cap)
    # own pivots beyond the cap: the file filled up (oracle pivot counts)
    if cap <= 17:
        assert (par[1][2] > cap).any()
    _run(ctx, 'tls4_oa', par, cap)
    _run(ctx, 'tls4_oa', ch, cap)


@pytest.mark.parametrize('name,nbox', [('one_slot', 300), ('four_slot', 150)])
def test_slot_counts(ctx, name, nbox):
    p = _problem(name)
    assert (p.n + p.m + 63) // 64 == (1 if name == 'one_slot' else 4) and p.m <= 64
    ctx.load(p)
    par, ch = _family(name, nbox, 43, LP_PFI_MAX)
    _run(ctx, name, par, LP_PFI_MAX)
    if ch[0][0].shape[0]:
        _run(ctx, name, ch, LP_PFI_MAX)


@pytest.mark.parametrize('name', ['tls4_lin', 'one_slot'])
def test_sparse_etas_from_root(ctx, name):
    """Boxes solved from the root basis with cap 32: BTRAN starts from a unit
    vector, so most eta products are exact zeros (the skip test's cases)."""
    ctx.load(_problem(name))
    par, ch = _family(name, 400, 44, LP_PFI_MAX)
    assert (par[1][2] >= 2).any()     # some LPs run BTRAN through etas
    _run(ctx, name, par, LP_PFI_MAX)
    if ch[0][0].shape[0]:
        _run(ctx, name, ch, LP_PFI_MAX)
