"""GPU: the edge-case LPs of tests/lp_edge_cases.py through every dual-simplex
kernel that can run them, against the oracle in the matching arithmetic and
against HiGHS on every LP.

  K3    set_lp_variant(1), m <= 64
  K3L   set_lp_variant(2), every m (one wave for m <= 256, four beyond)
  K3P   set_lp_variant(3), shared warm start, m <= 64, eta caps 16 and 32
  K3PW  the automatic choice for 64 < m <= 128 with a shared warm start where
        its LDS state fits (65 and 112 rows here; at 128 rows auto mode runs
        K3L, and the test says so)

Cold solves (the product-form kernels take the slack basis as a shared warm
start), warm solves from the root basis on boxes that cut the root solution
off, bound LPs min +-x_j, and a warm basis without reduced costs under
another objective.  Bars: status and pivot count equal the oracle's;
objective and x bit-equal for K3L, within 1e-9 for K3, K3P and K3PW; the
final head and statuses equal the oracle's where the kernel gives a warm
start back (K3, K3L); and the status equals HiGHS's on every LP."""
import numpy as np
import pytest

import lp_edge_cases as ec
import oracle
from golden_io import OBJ_TOL
from minotaur_amd.runtime import LP_PFI_MAX, LP_PFI_WIDE_MAX, WarmStart

pytestmark = pytest.mark.gpu

K3, K3L = 1, 2
DENSE = [(c.id, v) for c in ec.all_cases() for v in (K3, K3L) if v == K3L or c.m <= 64]
PRODUCT = [c.id for c in ec.all_cases() if c.m <= 128]


@pytest.fixture(scope='module')
def ctx():
    from minotaur_amd.runtime import Context
    c = Context(0)
    yield c
    c.set_lp_variant(0)
    c.set_lp_pfi(LP_PFI_MAX)
    c.close()


def _gpu_ws(ows, d=True):
    """The oracle's warm start in the ABI's layout (B^-1 column-major)."""
    return WarmStart(ows.head, ows.st, ows.d if d else None, np.ascontiguousarray(ows.binv.T))


def _slack(p):
    """The slack basis as a warm start: what a cold solve starts from."""
    head = np.arange(p.n, p.n + p.m, dtype=np.int32)
    st = np.zeros(p.n + p.m, dtype=np.int8)
    st[p.n:] = 3
    d = np.concatenate([p.obj, np.zeros(p.m)])
    return oracle.WarmStart(head, st, -np.eye(p.m), d)


def _same(r, st, obj, it, x, refs, exact, what):
    """A kernel's batch against the oracle's and HiGHS's."""
    assert np.array_equal(r.status, st), (what, r.status, st)
    assert np.array_equal(r.iters, it), (what, r.iters, it)
    for b, (hs, ho) in enumerate(refs):
        assert hs in (0, 2, 4) and r.status[b] == hs, (what, b, r.status[b], hs)
        if hs == 0:
            assert abs(r.obj[b] - ho) <= OBJ_TOL * max(1.0, abs(ho)), (what, b, r.obj[b], ho)
    ok = st == 0
    assert np.array_equal(r.obj[~ok], obj[~ok]), what        # +inf / -inf
    if exact:
        assert np.array_equal(r.obj[ok], obj[ok]), (what, r.obj, obj)
        assert x is None or np.array_equal(r.x[ok], x[ok]), what
    else:
        assert np.allclose(r.obj[ok], obj[ok], rtol=1e-9, atol=1e-9), (what, r.obj, obj)
        assert x is None or np.allclose(r.x[ok], x[ok], rtol=1e-9, atol=1e-9), what


@pytest.mark.parametrize('cid,variant', DENSE)
def test_dense_kernels(ctx, cid, variant):
    c = ec.case(cid)
    p = c.p
    exact = variant == K3L
    box = (p.vlb[None], p.vub[None])
    rs, _, _, ows = ec.root(cid)
    cols, signs = ec.bound_lps(c)
    ctx.load(p)
    ctx.set_lp_variant(variant)
    try:
        cold = ctx.lp_solve(*box, want_x=True, want_ws=True)
        if rs == 0:
            LB, UB = ec.warm_boxes(cid)
            warm = ctx.lp_solve(LB, UB, _gpu_ws(ows), want_x=True)
            bnd = ctx.lp_bound(cols, signs, ws=_gpu_ws(ows), want_x=True)
            q = ec.new_objective(c)
            ctx.load(q)
            ctx.set_lp_variant(variant)
            newobj = ctx.lp_solve(*box, _gpu_ws(ows, d=False), want_x=True)
        else:
            bnd = ctx.lp_bound(cols, signs, want_x=True)
    finally:
        ctx.set_lp_variant(0)
    st, obj, it, x, wo = oracle.dual_simplex_nodes(p, *box, None)
    _same(cold, st, obj, it, x, [ec.highs_cold(cid)], exact, (cid, 'cold'))
    if st[0] == 0:      # the final basis: what tells a wrong tie-break apart
        assert np.array_equal(cold.ws.head[0], wo.head[0]), (cid, cold.ws.head[0], wo.head[0])
        assert np.array_equal(cold.ws.st[0], wo.st[0]), cid
    if rs == 0:
        st, obj, it, x = oracle.dual_simplex(p, LB, UB, ows, want_x=True)
        _same(warm, st, obj, it, x, ec.highs_warm_boxes(cid), exact, (cid, 'warm'))
        st, obj, it, x = oracle.lp_bound(p, cols, signs, ws=ows)
        _same(bnd, st, obj, it, x, ec.highs_bounds(cid), exact, (cid, 'bound'))
        st, obj, it, x = oracle.dual_simplex(q, *box, oracle.WarmStart(ows.head, ows.st, ows.binv,
                                                                       None), want_x=True)
        _same(newobj, st, obj, it, x, [ec.highs_new_objective(cid)], exact, (cid, 'new objective'))
    else:
        st, obj, it, x = oracle.lp_bound(p, cols, signs)
        _same(bnd, st, obj, it, x, ec.highs_bounds(cid), exact, (cid, 'bound'))


class product_form:
    """LP calls inside run on K3P with an eta cap of kmax (m <= 64), or on
    the automatic choice (64 < m <= 128: K3PW with its cap kmax, or kmax = 0,
    the dense K3L); auto mode and the default cap afterwards."""

    def __init__(self, ctx, m, kmax):
        self.ctx, self.m, self.kmax = ctx, m, kmax

    def __enter__(self):
        if self.m <= 64:
            self.ctx.set_lp_variant(3)
            self.ctx.set_lp_pfi(self.kmax)
        assert self.ctx.oracle_pfi() == self.kmax     # test_k3pw_is_auto_choice's check

    def __exit__(self, *a):
        self.ctx.set_lp_variant(0)
        self.ctx.set_lp_pfi(LP_PFI_MAX)


@pytest.mark.parametrize('cid', PRODUCT)
def test_product_form_kernels(ctx, cid):
    c = ec.case(cid)
    p = c.p
    box = (p.vlb[None], p.vub[None])
    rs, _, _, ows = ec.root(cid)
    cols, signs = ec.bound_lps(c)
    slack = _slack(p)
    ctx.load(p)
    caps = ec.pfi_caps(c.m) if c.m <= 64 else (LP_PFI_WIDE_MAX if c.m <= ec.K3PW_ROWS else 0,)
    for kmax in caps:
        with product_form(ctx, c.m, kmax):
            cold = ctx.lp_solve(*box, _gpu_ws(slack), want_x=True)
            # (a bound LP rebuilds the reduced costs from its objective)
            bnd = ctx.lp_bound(cols, signs, ws=_gpu_ws(ows if rs == 0 else slack), want_x=True)
            if rs == 0:
                LB, UB = ec.warm_boxes(cid)
                warm = ctx.lp_solve(LB, UB, _gpu_ws(ows), want_x=True)
        st, obj, it, x = oracle.dual_simplex(p, *box, slack, want_x=True, pfi=kmax)
        _same(cold, st, obj, it, x, [ec.highs_cold(cid)], False, (cid, kmax, 'cold'))
        st, obj, it, x = oracle.lp_bound(p, cols, signs, ws=ows if rs == 0 else slack, pfi=kmax)
        _same(bnd, st, obj, it, x, ec.highs_bounds(cid), False, (cid, kmax, 'bound'))
        if rs == 0:
            st, obj, it, x = oracle.dual_simplex(p, LB, UB, ows, want_x=True, pfi=kmax)
            _same(warm, st, obj, it, x, ec.highs_warm_boxes(cid), False, (cid, kmax, 'warm'))


@pytest.mark.parametrize('variant,kmax', [(K3, 0), (K3L, 0), (3, 16), (3, LP_PFI_MAX)])
def test_knapsack_bound_lps(ctx, variant, kmax):
    """The 36 bound LPs of the golden knapsack LP from its root basis: free
    columns whose reduced cost returns to zero on an artificial bound."""
    p, cols, signs = ec.knapsack_bound_lps()
    rs, _, _, ows = ec.root('knapsack')
    assert rs == 0
    ctx.load(p)
    ctx.set_lp_variant(variant)
    try:
        if kmax:
            ctx.set_lp_pfi(kmax)
            assert ctx.oracle_pfi() == kmax
        r = ctx.lp_bound(cols, signs, ws=_gpu_ws(ows), want_x=True)
    finally:
        ctx.set_lp_variant(0)
        ctx.set_lp_pfi(LP_PFI_MAX)
    st, obj, it, x = oracle.lp_bound(p, cols, signs, ws=ows, pfi=kmax)
    _same(r, st, obj, it, x, ec.highs_bounds('knapsack'), variant == K3L, ('knapsack', variant))

