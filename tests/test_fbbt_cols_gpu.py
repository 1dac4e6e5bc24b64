"""GPU: K1 with clean columns (mgpu_fbbt_cols_dev) computes what K1 computes
over all columns, bit for bit.

tightenInts_ changes a bound only when it is non-integral, and checkBounds_
tests lb > ub + tol per column; every sweep ends with both over all columns.
So a box that K1 left feasible has every integer column integral (or
infinite) and every column past the check, and a child that moves one bound
of column j needs, per sweep, only j and the columns a row or the objective
stored in that sweep.  Bar: lb, ub, infeas, nmods and carry_out with the hint
equal the run without it and the C restatement, on the one-shot and the
persistent kernel, in the identity order and grouped by branching variable,
in waves that mix clean and unclean nodes, at n = 64 / 65 / 105, and where
the hint is ignored (n > 128, m > 64).
"""
import math

import numpy as np
import pytest

import oracle
import test_fbbt_carry_gpu as tc
from golden_io import bits_equal, cases, load_fbbt
from minotaur_amd.problem import (BINARY, CONTINUOUS, INTEGER, from_rows, knapsack_oa, random_boxes,
                                  random_problem)

pytestmark = pytest.mark.gpu

ALL = tc.ALL
KERNELS = [(2, None), (3, 2), (3, 5)]   # one-shot; persistent on 2 and 5 waves


@pytest.fixture(scope='module')
def ctx():
    from minotaur_amd.runtime import Context
    c = Context(0)
    yield c
    c.close()


def _run(ctx, LB, UB, inc, variant, waves, monkeypatch, mask=None, order=None, clean=None,
         refill=None):
    """One K1 launch: (lb, ub, infeas, nmods, carry) as numpy."""
    import torch
    dev = torch.device('cuda', 0)
    B = LB.shape[0]
    lb = torch.from_numpy(np.array(LB, dtype=np.float64)).to(dev)
    ub = torch.from_numpy(np.array(UB, dtype=np.float64)).to(dev)
    olb, oub = torch.empty_like(lb), torch.empty_like(ub)
    inf = torch.zeros(B, dtype=torch.int32, device=dev)
    nm = torch.zeros(B, dtype=torch.int32, device=dev)
    carry = torch.zeros(B, dtype=torch.int64, device=dev)

    def dv(a, dt):
        return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
    tm, to, tcl = dv(mask, np.int64), dv(order, np.int32), dv(clean, np.int32)
    torch.cuda.synchronize()
    ctx.set_fbbt_variant(variant)
    if waves is not None:
        monkeypatch.setenv('MGPU_FBBT_WAVES', str(waves))
    if refill is not None:
        monkeypatch.setenv('MGPU_FBBT_REFILL', str(refill))
    try:
        ctx.fbbt_cols_dev(lb, ub, olb, oub, inf, nm, inc, tm, carry, to, tcl)
        ctx.sync()
    finally:
        ctx.set_fbbt_variant(0)
    return (olb.cpu().numpy(), oub.cpu().numpy(), inf.cpu().numpy(), nm.cpu().numpy(),
            carry.cpu().numpy())


def _same(r, ref, carry=None):
    assert bits_equal(r[0], ref.lb) and bits_equal(r[1], ref.ub)
    assert np.array_equal(r[2], ref.infeas) and np.array_equal(r[3], ref.nmods)
    if carry is not None:
        assert np.array_equal(r[4], carry)


def _three_ways(ctx, cl, cu, inc, mk, key, ref, variant, waves, monkeypatch, order=None, **kw):
    """No hints, masks only, masks + clean column: all equal the oracle, and
    the two masked runs carry the same mask out."""
    plain = _run(ctx, cl, cu, inc, variant, waves, monkeypatch, None, order, None, **kw)
    _same(plain, ref)
    masked = _run(ctx, cl, cu, inc, variant, waves, monkeypatch, mk, order, None, **kw)
    _same(masked, ref)
    cols = _run(ctx, cl, cu, inc, variant, waves, monkeypatch, mk, order, key, **kw)
    _same(cols, ref, masked[4])
    return cols


@pytest.mark.parametrize('order', ['null', 'sorted'])
@pytest.mark.parametrize('variant,waves', KERNELS)
@pytest.mark.parametrize('inc', [math.inf, 20.0])
@pytest.mark.parametrize('inst', ['tls4_oa', 'nvs08_oa', 'tls4_lin'])
def test_children_equal_all_columns(ctx, inst, inc, variant, waves, order, monkeypatch):
    f = tc._fixture(ctx, inst, inc, monkeypatch)
    od = tc._orders(f['key'], f['cl'].shape[0])[order]
    _three_ways(ctx, f['cl'], f['cu'], inc, f['mk'], f['key'], f['ref'], variant, waves,
                monkeypatch, od)


def _non_integral_pushes(p, res):
    """Nodes whose mod log holds a non-integral bound on an integer column: a
    row or the objective left it, tightenInts_ has to round it."""
    ints = np.isin(p.vtype, (0, 1))
    return sum(any(ints[v] and abs(x - math.floor(x + 0.5)) > 1e-6 for v, _, x in res.mods(b))
               for b in range(res.lb.shape[0]))


# incumbent at which varBndsFromObj_ changes a column of some child (the carry
# fixture's 20.0 is too weak for nvs08's objective)
OBJ_INC = {'tls4_oa': 20.0, 'nvs08_oa': 10.0, 'tls4_lin': 20.0}


@pytest.mark.parametrize('inst', ['tls4_oa', 'nvs08_oa', 'tls4_lin'])
def test_fixture_exercises_rounding_and_objective(ctx, inst, monkeypatch):
    """The children hold the cases a skipped column could lose, read from the
    oracle's mod log: a row visit leaves a non-integral bound on an integer
    column, which tightenInts_ must round, and varBndsFromObj_ changes a column
    (the log with the incumbent differs from the log without).  K1 with the
    hint equals the oracle at that incumbent too.

    No child fails checkBounds_ on a continuous column, and none can while it
    is clean: linBndTighten_ and varBndsFromObj_ clamp a new bound to the
    opposite one, so only tightenInts_'s rounding makes bounds cross, on an
    integer column.  test_hand_built_checks builds that case."""
    f = tc._fixture(ctx, inst, 20.0, monkeypatch)
    p = f['p']
    inc = OBJ_INC[inst]
    with_inc = oracle.linear_fbbt(p, f['cl'], f['cu'], inc, mod_cap=256, nthreads=8)
    without = oracle.linear_fbbt(p, f['cl'], f['cu'], None, mod_cap=256, nthreads=8)
    assert max(with_inc.nmods.max(), without.nmods.max()) <= 256
    assert _non_integral_pushes(p, with_inc) > 0
    B = f['cl'].shape[0]
    assert sum(with_inc.mods(b) != without.mods(b) for b in range(B)) > 0
    cont = ~np.isin(p.vtype, (0, 1))
    for r in (with_inc, without, f['ref']):
        assert not np.any((r.lb > r.ub + 1e-8) & cont)
    for variant, waves in ((2, None), (3, 2)):
        _three_ways(ctx, f['cl'], f['cu'], inc, f['mk'], f['key'], with_inc, variant, waves,
                    monkeypatch, tc._orders(f['key'], B)['sorted'])


def _hand_lp():
    """x binary, z integer in [0, 5], y continuous in [0, 10];
    10 z - 23 x >= 0, 10 z + 23 x <= 50, y - z >= 0.  The root is feasible and
    clean.  The child x >= 1 gets z in [2.3, 2.7] from the two rows, which
    tightenInts_ rounds to [3, 2]: its check fires on an integer column."""
    rows = [[(1, 10.0), (0, -23.0)], [(1, 10.0), (0, 23.0)], [(2, 1.0), (1, -1.0)]]
    return from_rows('cols-hand', 3, rows, [0.0, -math.inf, 0.0], [math.inf, 50.0, math.inf],
                     np.array([0.0, 0.0, 0.0]), np.array([1.0, 5.0, 10.0]),
                     np.array([BINARY, INTEGER, CONTINUOUS], dtype=np.int32),
                     np.array([0.0, 0.0, 1.0]))


@pytest.mark.parametrize('variant,waves', [(2, None), (3, 1)])
def test_hand_built_checks(ctx, variant, waves, monkeypatch):
    """checkBounds_ fires for a clean child on an integer column (after
    rounding), and for an unclean node on a continuous column whose bounds
    cross in its input box: both in one wave, between clean feasible children."""
    p = _hand_lp()
    ctx.load(p)
    root = oracle.linear_fbbt(p, p.vlb[None], p.vub[None], None)
    assert root.infeas[0] == 0
    down_u, up_l = root.ub[0].copy(), root.lb[0].copy()
    down_u[0], up_l[0] = 0.0, 1.0
    cross_l, frac_l = root.lb[0].copy(), root.lb[0].copy()
    cross_l[2] = root.ub[0][2] + 1.0        # y: lb > ub, nothing else wrong
    frac_l[1] = 0.3                         # z: needs rounding, not clean
    kinds = [(root.lb[0], down_u, 0), (up_l, root.ub[0], 0), (cross_l, root.ub[0], -1),
             (frac_l, root.ub[0], -1)]
    B = 100
    LB = np.array([kinds[b % 4][0] for b in range(B)])
    UB = np.array([kinds[b % 4][1] for b in range(B)])
    clean = np.array([kinds[b % 4][2] for b in range(B)], dtype=np.int32)
    ref = oracle.linear_fbbt(p, LB, UB, None, mod_cap=16)
    assert list(ref.infeas[:4]) == [0, 1, 1, 0]
    assert _non_integral_pushes(p, ref) >= B // 4          # the child x >= 1
    assert ref.lb[2][2] > ref.ub[2][2] + 1e-8              # the crossed continuous column
    r = _run(ctx, LB, UB, math.inf, variant, waves, monkeypatch, None, None, clean)
    _same(r, ref)
    # waves of clean nodes only: the up children alone, then the down children
    for k in (0, 1):
        sel = np.arange(k, B, 4)
        r = _run(ctx, LB[sel], UB[sel], math.inf, variant, waves, monkeypatch, None, None,
                 clean[sel])
        assert bits_equal(r[0], ref.lb[sel]) and bits_equal(r[1], ref.ub[sel])
        assert np.array_equal(r[2], ref.infeas[sel]) and np.array_equal(r[3], ref.nmods[sel])


@pytest.mark.parametrize('refill', [1, 16])
def test_mixed_waves(ctx, refill, monkeypatch):
    """B = 200: clean children interleaved with unclean nodes (no clean column,
    all rows, integer bounds such as 0.3 that need rounding); the persistent
    kernel on one wave takes fresh unclean nodes into a running wave."""
    inc = 20.0
    f = tc._fixture(ctx, 'tls4_oa', inc, monkeypatch)
    p = f['p']
    B = 200
    LB, UB = f['cl'][:B].copy(), f['cu'][:B].copy()
    mk, clean = f['mk'][:B].copy(), f['key'][:B].copy()
    ints = np.nonzero(np.isin(p.vtype, (0, 1)))[0]
    rng = np.random.default_rng(5)
    dirty = np.nonzero(rng.random(B) < 0.3)[0]
    assert 20 < dirty.size < 120
    for b in dirty:
        for j in rng.choice(ints, 3, replace=False):
            if UB[b, j] - LB[b, j] >= 1.0:
                LB[b, j] += 0.3
                UB[b, j] -= 0.3
        mk[b], clean[b] = ALL, -1
    ref = oracle.linear_fbbt(p, LB, UB, inc, nthreads=8)
    assert np.count_nonzero(ref.nmods[dirty]) > dirty.size // 2
    for waves in (1, 2):
        _three_ways(ctx, LB, UB, inc, mk, clean, ref, 3, waves, monkeypatch, refill=refill)
    _three_ways(ctx, LB, UB, inc, mk, clean, ref, 2, None, monkeypatch)


def test_grandchildren(ctx, monkeypatch):
    """The children's outputs, run with the hint, are clean boxes again."""
    inc = 20.0
    f = tc._fixture(ctx, 'tls4_oa', inc, monkeypatch)
    od = tc._orders(f['key'], f['cl'].shape[0])['sorted']
    lb1, ub1, inf1, _, carry1 = _run(ctx, f['cl'], f['cu'], inc, 3, 3, monkeypatch, f['mk'], od,
                                     f['key'])
    gl, gu, mk, key = tc._children(f['p'], lb1, ub1, inf1, carry1, 77)
    assert gl.shape[0] > 64
    ref = oracle.linear_fbbt(f['p'], gl, gu, inc, nthreads=8)
    for variant, waves in ((2, None), (3, 2)):
        _three_ways(ctx, gl, gu, inc, mk, key, ref, variant, waves, monkeypatch,
                    np.argsort(key, kind='stable').astype(np.int32))


def _random_family(p, seed):
    """Children (boxes, all-rows masks, clean columns) of seeded parents of a
    generated problem, the parents tightened by the oracle."""
    LB, UB = random_boxes(p, 96, seed)
    o = oracle.linear_fbbt(p, LB, UB, None, nthreads=8)
    return tc._children(p, o.lb, o.ub, o.infeas, np.full(96, ALL, dtype=np.int64), seed + 1)


@pytest.mark.parametrize('variant,waves', [(2, None), (3, 2)])
@pytest.mark.parametrize('n', [64, 65, 140])
def test_column_count_limits(ctx, n, variant, waves, monkeypatch):
    """n = 64 and 65 sit on the edge of the set's first 64 columns (tls4's
    n = 105 uses both halves); n = 140 > 128: the hint is ignored."""
    p = random_problem(7, n=n, m=30)
    ctx.load(p)
    cl, cu, mk, key = _random_family(p, 5)
    assert cl.shape[0] > 64
    ref = oracle.linear_fbbt(p, cl, cu, None, mod_cap=512, nthreads=8)
    assert _non_integral_pushes(p, ref) > 0
    _three_ways(ctx, cl, cu, math.inf, mk, key, ref, variant, waves, monkeypatch)


def test_more_than_64_rows_ignores_hint(ctx, monkeypatch):
    """m = 65: the byte-flag kernels take neither masks nor clean columns; a
    hint that would be wrong if honoured changes nothing."""
    p = knapsack_oa(f=16, N=48, points=(1.0, 8.0, 32.0, 48.0))
    assert p.m == 65
    ctx.load(p)
    LB, UB = random_boxes(p, 300, 3)
    ref = oracle.linear_fbbt(p, LB, UB, None, nthreads=8)
    for variant in (0, 2, 3):
        r = _run(ctx, LB, UB, math.inf, variant, 2, monkeypatch, None, None,
                 np.zeros(300, dtype=np.int32))
        _same(r, ref)


@pytest.mark.parametrize('variant', [2, 3])
@pytest.mark.parametrize('name', cases())
def test_null_and_minus_one_match_golden(ctx, name, variant, monkeypatch):
    p, g = load_fbbt(name)
    ctx.load(p)
    inc = math.inf if g['incumbent'] is None else g['incumbent']
    B = g['lb_in'].shape[0]
    for clean in (None, np.full(B, -1, dtype=np.int32)):
        lb, ub, inf, nm, _ = _run(ctx, g['lb_in'], g['ub_in'], inc, variant, 2, monkeypatch,
                                  None, None, clean)
        assert bits_equal(lb, g['lb_out']) and bits_equal(ub, g['ub_out'])
        assert np.array_equal(inf, g['infeas']) and np.array_equal(nm, g['nmods'])
