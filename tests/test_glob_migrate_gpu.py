"""GPU: the spatial tree across GPUs (mgpu_glob_shard / _pick / _export_dev /
_import_dev / _count / _row_width / _rebalance, glob.solve_distributed).

The yardstick is the CPU restatement oracle/glob_tree.py (CpuGlobContext),
which is never migrated: agreement with it shows that a migrated node lost
nothing -- box, secant / McCormick row state, tangent slots, bound, depth,
the parent's basis (warm 1), the branching record (relstronger).

The invariance tests rest on one condition: MaxVio, qt 1, lin 0 and the
incumbent held from glob_init on at the free run's final value (+inf where the
tree finds none).  Then every node's processing depends on its own record
only, and the tree's totals (nodes, decisions, LPs, pivots, branchings, cuts,
re-solves) do not depend on the order or grouping in which nodes are
processed.  ``invariant`` asserts exactly that on the CPU, at two batch sizes
and both orders, before any GPU run is held to those totals."""
import functools
import math
import os
import socket

import numpy as np
import pytest
import torch

from minotaur_amd import glob as mglob
from minotaur_amd.quad import random_qcqp

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))

SLOTS = 8
# (seed, nv0, ncon), squares
CASES = {'A': ((2, 6, 4), False), 'B': ((0, 8, 5), False), 'C': ((2, 8, 5), True),
         'D': ((17, 10, 6), False)}
CAP = 1 << 14


def make_qp(name):
    (seed, nv0, ncon), squares = CASES[name]
    return random_qcqp(seed, nv0=nv0, ncon=ncon, squares=squares)


def totals(s):
    return (s.nodes, list(s.ndec), s.lps, s.pivots, s.br_int, s.br_cont, s.cuts, s.resolves)


def round_key(s):
    return (s.rounds, s.nodes, list(s.ndec), s.br_int, s.br_cont, s.lps, s.pivots, s.cuts,
            s.resolves, s.open, np.float64(s.incumbent).tobytes())


def add_totals(*ts):
    out = None
    for sign, t in ts:
        flat = [t[0]] + list(t[1]) + list(t[2:])
        out = [sign * v for v in flat] if out is None else [a + sign * v for a, v in zip(out, flat)]
    return out


def flat(t):
    return [t[0]] + list(t[1]) + list(t[2:])


def cpu_tree(name, order, warm, inc):
    from glob_tree import CpuGlobContext
    c = CpuGlobContext(make_qp(name), tan_slots=SLOTS)
    c.glob_config(order, warm, 1, 0, 0)
    c.glob_init(CAP, inc)
    return c


def cpu_run(name, order, warm, inc, batch):
    c = cpu_tree(name, order, warm, inc)
    for _ in range(100000):
        st = c.glob_round(batch)
        if st.open == 0:
            return st
    raise AssertionError('the CPU tree did not end')


@functools.lru_cache(maxsize=None)
def invariant(name, warm):
    """(the fixed incumbent, the tree's totals) of an instance, after the CPU
    pre-check of the condition the invariance tests rest on."""
    inc = cpu_run(name, 0, warm, math.inf, 8).incumbent
    runs = [cpu_run(name, order, warm, inc, batch) for order in (0, 2) for batch in (8, 64)]
    for st in runs:
        assert st.incumbent == inc, (name, warm, st.incumbent, inc)      # it never moved
        assert totals(st) == totals(runs[0]), (name, warm)
    return inc, totals(runs[0])


@pytest.fixture(scope='module')
def ctxs():
    from minotaur_amd.runtime import Context
    cs = [Context(0), Context(0)]
    yield cs
    for c in cs:
        c.close()


def start(ctx, name, order, warm, inc=math.inf, lin=0, brancher=0, cap=CAP):
    qp = make_qp(name)
    p, _ = mglob.setup(ctx, qp, SLOTS)
    ctx.glob_config(order, warm, 1, lin, 0)
    ctx.glob_brancher(brancher)
    ctx.glob_init(cap, inc)
    return qp, p


def drop_root(ctx):
    assert len(ctx.glob_pick(1)) == 1
    ctx.glob_export_rows([0])
    assert ctx.glob_count()[0] == 0


def finish(ctx, batch):
    for _ in range(100000):
        st = ctx.glob_round(batch)
        if st.open == 0:
            return st
    raise AssertionError('the tree did not end')


def width_formula(qp, p, warm, brancher):
    nv, m = qp.nv, p.m
    T = 2 * qp.nsq * SLOTS
    return (2 * nv + qp.nrow_state + T + 2 + (1 + m + (nv + m + 15) // 16 if warm else 0) +
            (6 if brancher else 0))


@pytest.mark.parametrize('name,warm', [('A', 0), ('A', 1), ('C', 0)])
def test_identity_round_trip_round_for_round(ctxs, name, warm):
    """Every third round the stack's top 24 nodes leave as rows and come back
    (reversed, so the former top is on top again): every round's statistics
    stay those of the restatement, which a lost bit of box, row state,
    tangent slot, bound, depth or basis (warm 1: the pivots) would move."""
    ctx = ctxs[0]
    qp, p = start(ctx, name, 0, warm)
    cpu = cpu_tree(name, 0, warm, math.inf)
    assert ctx.glob_row_width() == width_formula(qp, p, warm, 0)
    trips = 0
    for r in range(1, 41):
        sg, sc = ctx.glob_round(16), cpu.glob_round(16)
        assert round_key(sg) == round_key(sc), (r, round_key(sg), round_key(sc))
        if sg.open == 0:
            break
        if r % 3 == 0:
            lbs = ctx.glob_pick(24)
            assert len(lbs) == min(24, sg.open)
            rows = ctx.glob_export_rows(np.arange(len(lbs)))
            assert rows.shape == (len(lbs), ctx.glob_row_width())
            assert ctx.glob_count()[0] == sg.open - len(lbs)
            nb = 2 * qp.nv + qp.nrow_state + 2 * qp.nsq * SLOTS
            assert np.array_equal(rows[:, nb].cpu().numpy(), lbs)
            ctx.glob_import_rows(torch.flip(rows, dims=[0]))
            assert ctx.glob_count()[0] == sg.open
            trips += len(lbs)
    assert trips > 24


IDEM = [(n, o, w, 0) for n in ('A', 'C') for o in (0, 2) for w in (0, 1)] + [('D', 2, 1, 2)]


@pytest.mark.parametrize('name,order,warm,brancher', IDEM)
def test_rows_are_idempotent(ctxs, name, order, warm, brancher):
    """Rows exported from one context, imported into a second one and exported
    again are bit-identical as multisets, in every configuration."""
    a, b = ctxs
    lin = 1 if brancher else 0
    batch = 4 if brancher else 8
    qp, p = start(a, name, order, warm, lin=lin, brancher=brancher)
    start(b, name, order, warm, lin=lin, brancher=brancher)
    assert a.glob_row_width() == b.glob_row_width() == width_formula(qp, p, warm, brancher)
    for _ in range(6):
        a.glob_round(batch)
    k = 5
    assert len(a.glob_pick(8)) >= k
    n_open = a.glob_count()[0]
    rows1 = a.glob_export_rows(np.arange(k))
    assert a.glob_count()[0] == n_open - k
    drop_root(b)
    b.glob_import_rows(rows1)
    assert b.glob_count()[0] == k
    assert len(b.glob_pick(8)) == k
    rows2 = b.glob_export_rows(np.arange(k))
    r1, r2 = rows1.cpu().numpy(), rows2.cpu().numpy()
    assert sorted(r.tobytes() for r in r1) == sorted(r.tobytes() for r in r2)
    nb = 2 * qp.nv + qp.nrow_state + 2 * qp.nsq * SLOTS
    if warm:
        assert (r1[:, nb + 2] == 1.0).any()          # a basis travelled
    if brancher:
        assert (r1[:, -6] >= 0).any()                # a branching record travelled


@pytest.mark.parametrize('warm', [0, 1])
def test_partial_export_and_stack_compaction(ctxs, warm):
    """Picks {1, 3, 4} of 6 leave the stack for a second context; the gaps
    close; both trees together do the single tree's work exactly."""
    inc, want = invariant('A', warm)
    a, b = ctxs
    qp, _ = start(a, 'A', 0, warm, inc)
    start(b, 'A', 0, warm, inc)
    for _ in range(10):
        sa = a.glob_round(8)
    assert sa.open >= 6
    lbs = a.glob_pick(6)
    rows = a.glob_export_rows([1, 3, 4])
    assert np.array_equal(rows[:, 2 * qp.nv + qp.nrow_state].cpu().numpy(), lbs[[1, 3, 4]])
    assert a.glob_count()[0] == sa.open - 3
    drop_root(b)
    b.glob_import_rows(rows)
    sa, sb = finish(a, 8), finish(b, 8)
    assert sa.incumbent == inc and sb.incumbent == inc
    assert add_totals((1, totals(sa)), (1, totals(sb))) == flat(want)


@pytest.mark.parametrize('order', [0, 2])
@pytest.mark.parametrize('name', ['A', 'B'])
def test_shard(ctxs, name, order):
    """Two contexts run the same first rounds, then each keeps its share: the
    shares partition the open nodes and together do the single tree's work."""
    inc, want = invariant(name, 0)
    a, b = ctxs
    start(a, name, order, 0, inc)
    start(b, name, order, 0, inc)
    for _ in range(6):
        sa, sb = a.glob_round(8), b.glob_round(8)
    assert round_key(sa) == round_key(sb) and sa.open > 2
    shared, n_open = totals(sa), sa.open
    ka, kb = a.glob_shard(0, 2), b.glob_shard(1, 2)
    assert ka + kb == n_open and ka == (n_open + 1) // 2
    assert a.glob_count()[0] == ka and b.glob_count()[0] == kb
    sa, sb = finish(a, 8), finish(b, 8)
    assert sa.incumbent == inc and sb.incumbent == inc
    assert add_totals((1, totals(sa)), (1, totals(sb)), (-1, shared)) == flat(want)


@pytest.mark.parametrize('order', [0, 2])
def test_import_that_does_not_fit(ctxs, order):
    """MGPU_ERR_NOMEM before the pool is touched: the count and the next
    round's statistics are those of a twin that never saw the call."""
    from minotaur_amd.runtime import MgpuError
    a, b = ctxs
    start(a, 'A', order, 1, cap=64)
    start(b, 'A', order, 1, cap=64)
    for _ in range(4):
        sa, sb = a.glob_round(4), b.glob_round(4)
    assert round_key(sa) == round_key(sb) and sa.open >= 4
    n_open, spare = a.glob_count()
    assert n_open == sa.open and 0 < spare <= 64
    rows = torch.zeros((spare + 1, a.glob_row_width()), dtype=torch.float64, device='cuda')
    with pytest.raises(MgpuError, match='rc=-4'):
        a.glob_import_rows(rows)
    assert a.glob_count() == (n_open, spare) == b.glob_count()
    for _ in range(3):
        assert round_key(a.glob_round(4)) == round_key(b.glob_round(4))


@pytest.mark.parametrize('order,warm', [(0, 0), (2, 1)])
def test_world1_rebalance_leaves_the_tree(ctxs, order, warm):
    """A world of one: mgpu_glob_rebalance returns before touching the pool,
    and the torch-carrier path (dist.rebalance(tree='glob')) deals every
    picked node back to its owner; the tree runs on like the restatement."""
    from minotaur_amd import dist as mdist
    ctx = ctxs[0]
    start(ctx, 'A', order, warm)
    cpu = cpu_tree('A', order, warm, math.inf)
    for r in range(1, 13):
        sg, sc = ctx.glob_round(8), cpu.glob_round(8)
        assert round_key(sg) == round_key(sc), r
        if r == 4:
            after, moved, picked, got = ctx.glob_rebalance(50)
            assert (after, moved, picked.size, got.size) == (sg.open, 0, 0, 0)
        if r == 8 and order == 0:
            after, moved, picked, got = mdist.rebalance(ctx, mdist.Comm(0, 1), 8, tree='glob')
            assert (after, moved, got.size) == (sg.open, 0, 0)
            assert np.array_equal(picked, ctx.glob_pick(100))


# ---- world 2 on one device over the host transport ---------------------------
def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _solve_worker(rank, world, port, out, name, kw):
    import sys
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, 'oracle'))
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    dist.init_process_group('gloo', rank=rank, world_size=world)
    from minotaur_amd import dist as mdist
    from minotaur_amd.runtime import Context
    try:
        ctx = Context(0)
        comm = mdist.NativeComm(ctx, rank, world, 'host')
        inc, x, st, rounds, mine = mglob.solve_distributed(
            ctx, make_qp(name), kw.pop('batch'), rank, world, comm, capacity=CAP,
            tan_slots=SLOTS, max_rounds=2000, **kw)
        out[rank] = (inc, None if x is None else x.tolist(), rounds, mine, st.open)
        ctx.close()
    finally:
        dist.destroy_process_group()


def _world2(name, **kw):
    import torch.multiprocessing as mp
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_solve_worker, args=(2, _free_port(), out, name, kw), nprocs=2, join=True)
    return out[0], out[1]


def _check_receipts(log0, log1):
    from test_dist_cpu import _expected_receipts
    assert len(log0) == len(log1) > 0
    for (p0, g0), (p1, g1) in zip(log0, log1):
        e0, e1 = _expected_receipts([p0, p1], 2)
        assert g0 == e0 and g1 == e1


@pytest.mark.parametrize('order,warm', [(0, 0), (2, 1)])
def test_world2_solve_distributed_does_the_single_trees_work(order, warm):
    """glob.solve_distributed on two ranks with a rebalance every third round:
    the ranks' own totals add up to the CPU tree's, nodes really move, and
    every rebalance delivers what LoadBalance_'s deal assigns."""
    inc, want = invariant('A', warm)
    r0, r1 = _world2('A', batch=8, order=order, warm=warm, incumbent=inc, lb_every=3)
    (inc0, _, _, m0, open0), (inc1, _, _, m1, open1) = r0, r1
    assert inc0 == inc1 == inc and open0 == open1 == 0
    assert m0['moved'] == m1['moved'] > 0
    _check_receipts(m0['lb_log'], m1['lb_log'])
    nodes, ndec, lps, pivots, _, _, cuts, resolves = want
    for key, val in (('nodes', nodes), ('lps', lps), ('pivots', pivots), ('cuts', cuts),
                     ('resolves', resolves)):
        assert m0[key] + m1[key] == val, (key, m0[key], m1[key], val)
    assert [u + v for u, v in zip(m0['ndec'], m1['ndec'])] == ndec


def test_world2_relstronger_free_run():
    """A free relstronger run on two ranks (per-rank pseudocosts make the
    trees legitimately differ from a single GPU's): both ranks end on one
    incumbent, nodes move by the deal, and the incumbent's point is feasible
    for the original QCQP."""
    from test_glob_gpu import _qcqp_value
    r0, r1 = _world2('D', batch=4, order=2, warm=1, lin=1, brancher=2, lb_every=2, shard_at=4)
    (inc0, x0, rounds0, m0, open0), (inc1, x1, rounds1, m1, open1) = r0, r1
    assert open0 == open1 == 0 and rounds0 == rounds1 < 2000
    assert inc0 == inc1 and math.isfinite(inc0)
    assert m0['moved'] == m1['moved'] > 0
    _check_receipts(m0['lb_log'], m1['lb_log'])
    holders = [x for x in (x0, x1) if x is not None]
    assert holders
    qp = make_qp('D')
    for x in holders:
        x = np.asarray(x)
        for c in range(qp.ncon):
            act = _qcqp_value(qp, x, c)
            assert qp.clb[c] - 1e-5 <= act <= qp.cub[c] + 1e-5, (c, act)
        ints = qp.vtype[:qp.nv0] != 4
        assert np.all(np.abs(x[:qp.nv0][ints] - np.round(x[:qp.nv0][ints])) <= 1e-6)
        if qp.has_obj:
            val = _qcqp_value(qp, x, qp.ncon) + qp.obj_const
            assert abs(val - inc0) <= 1e-5 * max(1.0, abs(inc0)), (val, inc0)


def _alloc_worker(rank, world, port, out, order):
    import sys
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, 'oracle'))
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    dist.init_process_group('gloo', rank=rank, world_size=world)
    from minotaur_amd import dist as mdist
    from minotaur_amd.runtime import Context, alloc_stats
    try:
        ctx = Context(0)
        mdist.NativeComm(ctx, rank, world, 'host')
        start(ctx, 'A', order, 1)
        if rank > 0:
            drop_root(ctx)             # the root belongs to rank 0
        for _ in range(6):
            ctx.glob_round(8)
        S = 100
        first = ctx.glob_rebalance(S)  # sizes the exchange for S
        a1 = alloc_stats()
        moved = [ctx.glob_rebalance(S)[1] for _ in range(2)]
        a2 = alloc_stats()
        trips = []
        for _ in range(2):
            got = len(ctx.glob_pick(S))
            k = min(4, got)
            rows = ctx.glob_export_rows(np.arange(k))
            ctx.glob_import_rows(rows)
            torch.cuda.synchronize()
            trips.append(alloc_stats())
        out[rank] = (a1, a2, first[1], moved, trips, ctx.glob_count()[0])
        ctx.close()
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize('order', [0, 2])
def test_world2_warm_rebalance_allocates_nothing(order):
    """After the first mgpu_glob_rebalance at a pick size S, further
    rebalances at S and equal-size export / import round trips make no device
    (or pinned host) allocation."""
    import torch.multiprocessing as mp
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_alloc_worker, args=(2, _free_port(), out, order), nprocs=2, join=True)
    assert out[0][2] == out[1][2] > 0          # the first rebalance moved nodes to rank 1
    for r in range(2):
        a1, a2, _, moved, trips, n_open = out[r]
        assert a2 == a1, (r, a1, a2)
        assert trips[1] == trips[0] == a2, (r, trips)
        assert n_open > 0
