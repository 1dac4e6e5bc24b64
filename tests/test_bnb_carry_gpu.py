"""GPU: the batched tree with clean-row masks (mgpu_bnb_fbbt_carry) is the
same tree in every mode.

Mode 0 starts every node's K1 from all rows, mode 1 starts a child from its
parent's carried mask plus the rows of its branching variable, mode 2 also
works through a round's nodes grouped by branching variable.  Bar: equal
mgpu_bnb_stats after every round, equal pool rows at the end, and mode 2
equal to the CPU restatement (oracle/bnb.py) -- also after nodes left and
re-entered the pool and after a shard, which must move the masks with their
nodes or reset them to all rows.  K1's persistent kernel is forced (the auto
choice at these batch sizes is K1G, which takes no masks).
"""
import math
import os

import numpy as np
import pytest

from minotaur_amd.problem import LinProblem, random_boxes, random_mkp

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
B = 256
ROUNDS = 12


@pytest.fixture(scope='module')
def ctx():
    from minotaur_amd.runtime import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope='module')
def tls4_oa():
    return LinProblem.load(os.path.join(HERE, '..', 'minotaur_amd', 'instances', 'tls4_oa.npz'))


def _key(st):
    return (st.rounds, st.nodes, tuple(st.ndec), st.open, st.last_batch, st.incumbent, st.pruned,
            st.lps, st.pivots, st.sb_lps, st.sb_pivots, st.sb_pruned, st.sb_modified)


def _start(c, p, mode, order=0, warm=2, brancher=0, seeds=B, cap=1 << 14):
    c.bnb_config(order, warm)
    c.bnb_brancher(brancher)
    if mode is not None:
        c.bnb_fbbt_carry(mode)
    c.bnb_init(cap)
    if seeds:
        LB, UB = random_boxes(p, seeds, 31)
        c.bnb_import(LB, UB, np.full(seeds, -math.inf), np.zeros(seeds, dtype=np.int32))


def _pool_rows(c):
    """Every open node as a migration row, topmost first (empties the pool)."""
    k = len(c.bnb_pick(1 << 20))
    rows = c.bnb_export_rows(np.arange(k))
    return rows.cpu().numpy() if hasattr(rows, 'cpu') else np.asarray(rows)


def _tree(c, p, mode, disturb=False, rounds=ROUNDS, batch=B, **kw):
    """Stats after every round and the final pool rows."""
    _start(c, p, mode, **kw)
    out = []
    for r in range(rounds):
        st = c.bnb_round(batch)
        out.append(_key(st))
        if disturb and r == 3:      # rows leave and come back (a rebalance's moves)
            k = len(c.bnb_pick(100))
            assert k == 100
            c.bnb_import_rows(c.bnb_export_rows(np.arange(k)))
        if disturb and r == 7:
            assert c.bnb_shard(0, 2) > 0
    return out, _pool_rows(c)


@pytest.fixture()
def persistent(ctx, monkeypatch):
    """K1's persistent kernel on two waves: the kernel that takes masks, its
    lanes refilled from the queue mid-sweep."""
    monkeypatch.setenv('MGPU_FBBT_WAVES', '2')
    ctx.set_fbbt_variant(3)
    yield ctx
    ctx.set_fbbt_variant(0)
    ctx.bnb_fbbt_carry(2)
    ctx.bnb_config(0, 0)
    ctx.bnb_brancher(0)


@pytest.mark.parametrize('disturb', [False, True])
def test_tree_parity_across_modes(persistent, tls4_oa, disturb):
    """tls4-OA, depth-first, warm 2, batch 256, twelve rounds from the root
    plus 256 seeded boxes: modes 0, 1 and 2 and the CPU restatement agree
    after every round and on the whole pool at the end."""
    from bnb import CpuBnbContext
    c, p = persistent, tls4_oa
    c.load(p)
    res = {mode: _tree(c, p, mode, disturb) for mode in (0, 1, 2)}
    assert res[0][0][-1][1] > 6 * B       # the tree is wide: full batches
    for mode in (1, 2):
        assert res[mode][0] == res[0][0]
        assert res[mode][1].shape == res[0][1].shape
        assert np.array_equal(res[mode][1].view(np.int64), res[0][1].view(np.int64))
    cpu = CpuBnbContext(p, c.oracle_pfi())
    cs, crows = _tree(cpu, p, None, disturb)
    cmp = [(k[0], k[1], k[2], k[3], k[7], k[8]) for k in res[2][0]]
    assert cmp == [(k[0], k[1], k[2], k[3], k[7], k[8]) for k in cs]
    assert np.array_equal(res[2][1].view(np.int64), crows.view(np.int64))


@pytest.mark.parametrize('order,warm,brancher', [(1, 2, 0), (2, 1, 0), (0, 0, 1), (0, 1, 1)])
def test_other_orders_and_reliability(persistent, order, warm, brancher):
    """Best-first, the reference-heap order and reliability branching (its
    modified nodes restart from all rows): mode 2 against mode 0."""
    c = persistent
    p = random_mkp(5, 22, 3)
    c.load(p)
    res = {}
    for mode in (0, 2):
        _start(c, p, mode, order=order, warm=warm, brancher=brancher, seeds=0, cap=1 << 15)
        out = []
        for _ in range(400):
            st = c.bnb_round(16)
            out.append(_key(st))
            if st.open == 0:
                break
        res[mode] = out
    assert res[0][-1][3] == 0 and len(res[0]) > 5
    assert res[2] == res[0]


def test_no_device_allocation_after_warm_up(persistent, tls4_oa):
    """Mode 2's buffers (masks, keys, the grouping sort's workspace) are sized
    at init and at the first full batch: nothing is allocated between round
    3 and the last round."""
    from minotaur_amd.runtime import alloc_stats
    c, p = persistent, tls4_oa
    c.load(p)
    _start(c, p, 2)
    for _ in range(3):
        c.bnb_round(B)
    a0 = alloc_stats()
    for _ in range(ROUNDS - 3):
        st = c.bnb_round(B)
    assert st.last_batch == B
    assert alloc_stats() == a0
