"""GPU: K1 with clean-row masks (mgpu_fbbt_masked_dev) computes what K1
computes from all rows, bit for bit.

A child's box is its parent's K1 output with one bound of the branching
variable moved, so its first sweep only needs the rows the parent left
unclean -- the flags left when its sweep loop ended plus every row whose last
visit proved the parent infeasible (simplePresolve ignores that verdict; a
child that revisits the row stops its sweep there again) -- and the rows that
hold the branching variable.  Bar: lb, ub, infeas and nmods of the masked run
equal the all-rows run and the C oracle bit for bit, for every kernel that
takes masks, every order, and batches that refill lanes mid-sweep.
"""
import math
import os

import numpy as np
import pytest

import oracle
from golden_io import bits_equal, cases, load_fbbt
from minotaur_amd.problem import LinProblem, knapsack_oa, random_boxes

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ALL = np.int64(-1)          # all-ones u64 mask as int64
NPAR = 256
# parents' seed per instance: chosen so that the fixture holds the
# infeasible-row case (test_fixture_has_infeasible_row_parents asserts it)
SEED = {'tls4_oa': 1, 'nvs08_oa': 4, 'tls4_lin': 1}


@pytest.fixture(scope='module')
def ctx():
    from minotaur_amd.runtime import Context
    c = Context(0)
    yield c
    c.close()


def _load(inst):
    return LinProblem.load(os.path.join(HERE, '..', 'minotaur_amd', 'instances', f'{inst}.npz'))


def _colmask(p):
    cm = np.zeros(p.n, dtype=np.uint64)
    for i in range(p.m):
        for k in range(p.rowptr[i], p.rowptr[i + 1]):
            cm[p.colidx[k]] |= np.uint64(1) << np.uint64(i)
    return cm.view(np.int64)


def _run(ctx, LB, UB, inc, variant, waves, monkeypatch, mask=None, order=None, want_carry=True):
    """One K1 launch on device tensors: (lb, ub, infeas, nmods, carry) as numpy."""
    import torch
    dev = torch.device('cuda', 0)
    B = LB.shape[0]
    lb = torch.from_numpy(np.array(LB, dtype=np.float64)).to(dev)
    ub = torch.from_numpy(np.array(UB, dtype=np.float64)).to(dev)
    olb, oub = torch.empty_like(lb), torch.empty_like(ub)
    inf = torch.zeros(B, dtype=torch.int32, device=dev)
    nm = torch.zeros(B, dtype=torch.int32, device=dev)
    carry = torch.zeros(B, dtype=torch.int64, device=dev) if want_carry else None
    tm = None if mask is None else torch.from_numpy(np.ascontiguousarray(mask)).to(dev)
    to = None if order is None else torch.from_numpy(
        np.ascontiguousarray(order, dtype=np.int32)).to(dev)
    torch.cuda.synchronize()
    ctx.set_fbbt_variant(variant)
    if waves is not None:
        monkeypatch.setenv('MGPU_FBBT_WAVES', str(waves))
    try:
        ctx.fbbt_masked_dev(lb, ub, olb, oub, inf, nm, inc, tm, carry, to)
        ctx.sync()
    finally:
        ctx.set_fbbt_variant(0)
    return (olb.cpu().numpy(), oub.cpu().numpy(), inf.cpu().numpy(), nm.cpu().numpy(),
            None if carry is None else carry.cpu().numpy())


def _children(p, plb, pub, pinf, carry, seed):
    """Two children per feasible parent: an integer column with lb < ub,
    floor / ceil at a seeded fractional point.  Returns (LB, UB, mask, key)."""
    rng = np.random.default_rng(seed)
    cm = _colmask(p)
    ints = np.nonzero(np.isin(p.vtype, (0, 1)))[0]
    LB, UB, mk, key = [], [], [], []
    for b in np.nonzero(pinf == 0)[0]:
        free = [j for j in ints if plb[b, j] < pub[b, j] and np.isfinite(plb[b, j])
                and np.isfinite(pub[b, j])]
        if not free:
            continue
        j = int(rng.choice(free))
        x = plb[b, j] + (math.floor(rng.uniform(0.0, pub[b, j] - plb[b, j])) + rng.uniform(0.1, 0.9))
        x = min(x, pub[b, j] - 0.05)
        for up in (0, 1):
            l, u = plb[b].copy(), pub[b].copy()
            if up:
                l[j] = math.ceil(x)
            else:
                u[j] = math.floor(x)
            LB.append(l)
            UB.append(u)
            mk.append(carry[b] | cm[j])
            key.append(j)
    return (np.array(LB), np.array(UB), np.array(mk, dtype=np.int64),
            np.array(key, dtype=np.int32))


_FIX = {}


def _fixture(ctx, inst, inc, monkeypatch):
    """Parents tightened from all rows (variant 2: the carry), their children,
    and the children's all-rows reference (the C oracle), computed once."""
    k = (inst, inc)
    if k not in _FIX:
        p = _load(inst)
        ctx.load(p)
        LB, UB = random_boxes(p, NPAR, SEED[inst])
        plb, pub, pinf, pnm, carry = _run(ctx, LB, UB, inc, 2, None, monkeypatch)
        o = oracle.linear_fbbt(p, LB, UB, None if math.isinf(inc) else inc, nthreads=8)
        assert bits_equal(plb, o.lb) and bits_equal(pub, o.ub)
        assert np.array_equal(pinf, o.infeas) and np.array_equal(pnm, o.nmods)
        cl, cu, mk, key = _children(p, plb, pub, pinf, carry, 1000 + SEED[inst])
        ref = oracle.linear_fbbt(p, cl, cu, None if math.isinf(inc) else inc, nthreads=8)
        _FIX[k] = dict(p=p, plb=plb, pub=pub, pinf=pinf, carry=carry, cl=cl, cu=cu, mk=mk,
                       key=key, ref=ref)
    f = _FIX[k]
    ctx.load(f['p'])
    return f


def _assert_same(r, ref, idx=None):
    lb, ub, inf, nm = r[:4]
    sel = slice(None) if idx is None else idx
    assert bits_equal(lb, ref.lb[sel]) and bits_equal(ub, ref.ub[sel])
    assert np.array_equal(inf, ref.infeas[sel])
    assert np.array_equal(nm, ref.nmods[sel])


def _orders(key, B):
    return {'null': None, 'reversed': np.arange(B - 1, -1, -1, dtype=np.int32),
            'sorted': np.argsort(key[:B], kind='stable').astype(np.int32)}


@pytest.mark.parametrize('order', ['null', 'reversed', 'sorted'])
@pytest.mark.parametrize('variant,waves', [(2, None), (3, 2), (3, 5)])
@pytest.mark.parametrize('inc', [math.inf, 20.0])
@pytest.mark.parametrize('inst', ['tls4_oa', 'nvs08_oa', 'tls4_lin'])
def test_children_masked_equal_all_rows(ctx, inst, inc, variant, waves, order, monkeypatch):
    """Masked K1 on the children = plain K1 = the oracle, bit for bit; the
    persistent kernel on 2 and 5 waves refills its lanes mid-sweep."""
    f = _fixture(ctx, inst, inc, monkeypatch)
    B = f['cl'].shape[0]
    assert B > 4 * 64
    od = _orders(f['key'], B)[order]
    r = _run(ctx, f['cl'], f['cu'], inc, variant, waves, monkeypatch, f['mk'], od)
    _assert_same(r, f['ref'])
    if order == 'null':   # plain K1 (no masks) on the same kernel
        _assert_same(_run(ctx, f['cl'], f['cu'], inc, variant, waves, monkeypatch,
                          want_carry=False), f['ref'])


@pytest.mark.parametrize('B', [1, 63, 200])
@pytest.mark.parametrize('variant,waves', [(2, None), (3, 2)])
def test_children_masked_small_batches(ctx, variant, waves, B, monkeypatch):
    f = _fixture(ctx, 'tls4_oa', 20.0, monkeypatch)
    for name, od in _orders(f['key'], B).items():
        r = _run(ctx, f['cl'][:B], f['cu'][:B], 20.0, variant, waves, monkeypatch, f['mk'][:B], od)
        _assert_same(r, f['ref'], slice(0, B))


def _row_verdicts(p, lb, ub):
    """Rows whose activity at the box proves infeasibility (linBndTighten_'s
    test on getLfBnds_'s ascending-column sums), as a bit mask."""
    out = 0
    for i in range(p.m):
        ll = uu = 0.0
        for k in range(p.rowptr[i], p.rowptr[i + 1]):
            a, j = float(p.val[k]), int(p.colidx[k])
            if a > 0:
                ll += a * lb[j]
                uu += a * ub[j]
            else:
                ll += a * ub[j]
                uu += a * lb[j]
        if ll > p.rhi[i] + 1e-8 or uu < p.rlo[i] - 1e-8:
            out |= 1 << i
    return out


@pytest.mark.parametrize('inst', ['tls4_oa', 'nvs08_oa', 'tls4_lin'])
def test_fixture_has_infeasible_row_parents(ctx, inst, monkeypatch):
    """The case that breaks the plain clean-row argument is in the fixture: a
    parent that K1 did not call infeasible (checkBounds_ is the only verdict
    simplePresolve keeps) although a row proves it at the output box -- the
    row's last visit returned the verdict, nothing moved since, so its flag is
    clear.  Every such row must be in the carried mask."""
    f = _fixture(ctx, inst, 20.0, monkeypatch)
    p = f['p']
    found = 0
    for b in np.nonzero(f['pinf'] == 0)[0]:
        v = _row_verdicts(p, f['plb'][b], f['pub'][b])
        if v:
            found += 1
            assert (int(f['carry'][b]) & ((1 << 64) - 1)) & v == v
    assert found >= 1


def test_grandchildren(ctx, monkeypatch):
    """The carry a masked run writes feeds a second generation."""
    inc = 20.0
    f = _fixture(ctx, 'tls4_oa', inc, monkeypatch)
    p = f['p']
    od = _orders(f['key'], f['cl'].shape[0])['sorted']
    lb1, ub1, inf1, nm1, carry1 = _run(ctx, f['cl'], f['cu'], inc, 3, 3, monkeypatch, f['mk'], od)
    gl, gu, mk, key = _children(p, lb1, ub1, inf1, carry1, 77)
    assert gl.shape[0] > 64
    ref = oracle.linear_fbbt(p, gl, gu, inc, nthreads=8)
    for variant, waves in ((2, None), (3, 2)):
        r = _run(ctx, gl, gu, inc, variant, waves, monkeypatch, mk,
                 np.argsort(key, kind='stable').astype(np.int32))
        _assert_same(r, ref)


def test_more_than_64_rows_ignores_masks(ctx, monkeypatch):
    """m = 65: byte flags; the masks are ignored, outputs are plain K1's and
    the carry comes back all-ones."""
    # (the default tangent points drop 64 > N; four points <= N give 1 + 16 * 4 rows)
    p = knapsack_oa(f=16, N=48, points=(1.0, 8.0, 32.0, 48.0))
    assert p.m == 65
    ctx.load(p)
    LB, UB = random_boxes(p, 300, 3)
    ref = oracle.linear_fbbt(p, LB, UB, None, nthreads=8)
    for variant in (0, 2, 3):
        r = _run(ctx, LB, UB, math.inf, variant, 2, monkeypatch,
                 np.zeros(300, dtype=np.int64), np.arange(299, -1, -1, dtype=np.int32))
        _assert_same(r, ref)
        assert np.all(r[4] == ALL)


@pytest.mark.parametrize('variant', [1, 2, 3])
@pytest.mark.parametrize('name', cases())
def test_all_ones_and_null_mask_match_golden(ctx, name, variant, monkeypatch):
    """An all-ones mask and no mask give today's bits on the reference's own
    presolveNode outputs."""
    p, g = load_fbbt(name)
    ctx.load(p)
    inc = math.inf if g['incumbent'] is None else g['incumbent']
    B = g['lb_in'].shape[0]
    for mask in (None, np.full(B, ALL, dtype=np.int64)):
        lb, ub, inf, nm, _ = _run(ctx, g['lb_in'], g['ub_in'], inc, variant, 2, monkeypatch, mask)
        assert bits_equal(lb, g['lb_out']) and bits_equal(ub, g['ub_out'])
        assert np.array_equal(inf, g['infeas']) and np.array_equal(nm, g['nmods'])
