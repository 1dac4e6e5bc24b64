"""GPU: the batched tree with clean columns (mgpu_bnb_fbbt_carry mode 3) is
the tree of mode 2.

Mode 3 passes every pool slot's key -- the branching variable for the two
children of a branched node, -1 for every other slot writer (the root,
imports, the receiving side of a rebalance, nodes the reliability brancher
modified) -- to K1 as the node's clean column.  Bar: equal mgpu_bnb_stats
(nodes, decisions, open nodes, incumbent, LPs, pivots) after every round and
equal pool rows at the end, also after nodes left and re-entered the pool and
after a shard.  K1's persistent kernel is forced (the auto choice at these
batch sizes is K1G, which takes no hints).
"""
import os

import numpy as np
import pytest

import test_bnb_carry_gpu as tb
from minotaur_amd.problem import LinProblem, random_mkp

pytestmark = pytest.mark.gpu

B = 2048
ROUNDS = 6


@pytest.fixture(scope='module')
def ctx():
    from minotaur_amd.runtime import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture()
def persistent(ctx, monkeypatch):
    monkeypatch.setenv('MGPU_FBBT_WAVES', '8')
    ctx.set_fbbt_variant(3)
    yield ctx
    ctx.set_fbbt_variant(0)
    ctx.bnb_fbbt_carry(3)     # the library's default
    ctx.bnb_config(0, 0)
    ctx.bnb_brancher(0)


@pytest.mark.parametrize('disturb', [False, True])
def test_mode3_is_mode2(persistent, disturb):
    """tls4-OA, depth-first, warm 2, batch 2 048 from the root plus 256 seeded
    boxes; with disturb, 100 rows leave and come back after round 3 and the
    pool is sharded in two after round 4."""
    c = persistent
    p = LinProblem.load(os.path.join(tb.HERE, '..', 'minotaur_amd', 'instances', 'tls4_oa.npz'))
    c.load(p)
    res = {}
    for mode in (2, 3):
        tb._start(c, p, mode, cap=1 << 16)
        out = []
        for r in range(ROUNDS):
            st = c.bnb_round(B)
            out.append(tb._key(st))
            if disturb and r == 3:
                k = len(c.bnb_pick(100))
                assert k == 100
                c.bnb_import_rows(c.bnb_export_rows(np.arange(k)))
            if disturb and r == 4:
                assert c.bnb_shard(0, 2) > 0
        res[mode] = (out, tb._pool_rows(c))
    assert res[2][0][-1][1] > B       # the tree got wider than one batch
    assert res[3][0] == res[2][0]
    assert res[3][1].shape == res[2][1].shape
    assert np.array_equal(res[3][1].view(np.int64), res[2][1].view(np.int64))


@pytest.mark.parametrize('order,warm,brancher', [(1, 2, 0), (0, 0, 1), (0, 1, 1)])
def test_other_orders_and_reliability(persistent, order, warm, brancher):
    """Best-first passes no hints; reliability branching resets the key of the
    nodes it modifies: mode 3 against mode 0 on a complete small tree."""
    c = persistent
    p = random_mkp(5, 22, 3)
    c.load(p)
    res = {}
    for mode in (0, 3):
        tb._start(c, p, mode, order=order, warm=warm, brancher=brancher, seeds=0, cap=1 << 15)
        out = []
        for _ in range(400):
            st = c.bnb_round(16)
            out.append(tb._key(st))
            if st.open == 0:
                break
        res[mode] = out
    assert res[0][-1][3] == 0 and len(res[0]) > 5
    assert res[3] == res[0]
