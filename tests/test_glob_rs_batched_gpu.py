"""GPU: the batched relstronger (mgpu_glob_brancher 2; glob_rel.hip and the
lockstep driver of glob_runtime.cpp) against its CPU restatement
(tests/glob_rs_batched.py) round for round -- nodes, decisions, branchings,
LPs and pivots, strong-branching and OBBT LPs, tangent cuts, re-solves, open
nodes, the round's width, the incumbent's bits -- and at the end the best
point bit for bit and the LP log (node-major) solve for solve: status and
pivots equal, values to 1e-9 max(1, max |value|), the bound of
tests/test_glob_rs_squares_gpu.py.  Widths 2, 4 and 16 (partial last rounds)
on bilinear trees and on trees with squares (separation and re-solves inside
wide rounds), rounds of 64 and 128 nodes, and rounds past the 256 lanes of a
block of the lane-per-node kernels.  Kind 2 at batch 1 and kind 1 take the same
lockstep one node wide, the root's OBBT hook included: batch 1 over ONE_CASES,
which with OBBT on reach its three outcomes (tests/test_glob_rs_batched_cpu.py
holds the case lists to that)."""
import math

import numpy as np
import pytest

from minotaur_amd.quad import random_qcqp
from glob_rs_batched import BatchedRsContext, same_incumbent, stats_key

pytestmark = pytest.mark.gpu

SLOTS = 8
BIL_CASES = [(2, 10, 6), (0, 8, 5), (4, 8, 5), (1, 8, 5), (7, 8, 5), (11, 6, 4)]
SQ_CASES = [(3, 5, 3), (33, 6, 4), (12, 5, 3)]
CASES = [(False, c) for c in BIL_CASES] + [(True, c) for c in SQ_CASES]
# batch 1 (trees of 19 nodes at most)
ONE_CASES = [(False, (4, 8, 5)), (False, (1, 8, 5)), (True, (3, 5, 3)), (True, (14, 5, 3))]


@pytest.fixture(scope='module')
def ctx():
    from minotaur_amd.runtime import Context
    c = Context(0)
    yield c
    c.close()


def start(ctx, squares, case, obbt, capacity=1 << 15, brancher=2):
    from minotaur_amd import glob as mglob
    seed, nv0, ncon = case
    qp = random_qcqp(seed, nv0=nv0, ncon=ncon, squares=squares)
    slots = SLOTS if squares else 0
    mglob.setup(ctx, qp, slots)
    ctx.glob_config(2, 1, 0, 1, obbt)
    ctx.glob_brancher(brancher)
    cpu = BatchedRsContext(qp, tan_slots=slots)
    cpu.glob_config(2, 1, 0, 1, obbt)
    cpu.glob_brancher(2)
    ctx.glob_init(capacity)
    cpu.glob_init(capacity)
    return cpu


def compare(ctx, cpu, batch, max_rounds=5000, close=True, wide=True):
    """Round for round; returns the widths of the rounds.  wide: some round
    must hold two nodes or more."""
    widths = []
    for _ in range(max_rounds):
        sg, sc = ctx.glob_round(batch), cpu.glob_round(batch)
        assert stats_key(sg) == stats_key(sc), (len(widths), stats_key(sg), stats_key(sc))
        assert sg.last_batch == sc.last_batch
        assert same_incumbent(sg.incumbent, sc.incumbent)
        widths.append(sg.last_batch)
        if sg.open == 0:
            break
    if close:
        assert sg.open == 0
    og, xg = ctx.glob_best()
    oc, xc = cpu.glob_best()
    assert same_incumbent(og, oc)
    if math.isfinite(og):
        assert np.array_equal(xg, xc)
    gs, gv, gi = ctx.glob_lp_log()
    assert [int(v) for v in gs] == [r[0] for r in cpu.lplog]
    assert [int(v) for v in gi] == [r[2] for r in cpu.lplog]
    cv = np.array([r[1] for r in cpu.lplog])
    fin = np.isfinite(cv)
    assert np.array_equal(fin, np.isfinite(gv))
    assert np.allclose(gv[fin], cv[fin], rtol=0,
                       atol=1e-9 * max(1.0, np.abs(cv[fin]).max(initial=0)))
    # a silent fall-back to one node per round fails here
    assert not wide or max(widths) >= 2
    return widths


@pytest.mark.parametrize('obbt', [0, 1])
@pytest.mark.parametrize('batch', [2, 4, 16])
@pytest.mark.parametrize('squares,case', CASES)
def test_batched_relstronger_matches_cpu_restatement(ctx, squares, case, batch, obbt):
    cpu = start(ctx, squares, case, obbt)
    widths = compare(ctx, cpu, batch)
    assert max(widths) <= batch


@pytest.mark.parametrize('obbt', [0, 1])
@pytest.mark.parametrize('squares,case', ONE_CASES)
def test_batch_one_matches_cpu_restatement(ctx, squares, case, obbt):
    """Kind 2 with every round one node wide: the lockstep on the reference's
    own sequence, at the root with OBBT tightening and leaving the point
    infeasible (bilinear (1,8,5)), feasible ((4,8,5), squares (3,5,3)) or
    changing nothing (squares (14,5,3))."""
    cpu = start(ctx, squares, case, obbt)
    assert max(compare(ctx, cpu, 1, wide=False)) == 1


def test_rounds_of_64_nodes(ctx):
    cpu = start(ctx, False, (2, 10, 6), 1)
    assert max(compare(ctx, cpu, 128)) == 64


def test_rounds_of_128_nodes(ctx):
    cpu = start(ctx, False, (0, 14, 9), 1)
    assert max(compare(ctx, cpu, 128)) == 128


def test_rounds_past_256_nodes(ctx):
    """Widths 1, 2, 4, ... 164, 306, 512, 434, 512: the strong branching of
    the narrower rounds, then masks and slot assignment past one block."""
    cpu = start(ctx, False, (1, 14, 9), 1)
    widths = compare(ctx, cpu, 512, max_rounds=13, close=False)
    assert max(widths) == 512 and sum(1 for w in widths if w > 256) >= 3


def test_no_allocation_in_a_round_of_a_width_seen(ctx):
    """A second tree at the same batch allocates nothing inside
    mgpu_glob_round: the round-sized buffers of the first tree are kept."""
    from minotaur_amd.runtime import alloc_stats
    batch = 128
    cpu = start(ctx, False, (0, 14, 9), 1)
    widths = []
    for _ in range(5000):
        s = ctx.glob_round(batch)
        widths.append(s.last_batch)
        if s.open == 0:
            break
    assert max(widths) == batch
    ctx.glob_init(1 << 15)
    for k in range(len(widths)):
        a0 = alloc_stats()
        s = ctx.glob_round(batch)
        assert alloc_stats() == a0, (k, s.last_batch)
        assert s.last_batch == widths[k]
    assert s.open == 0


def test_brancher_one_allocates_nothing_in_a_round(ctx):
    """Kind 1 sizes the lockstep's buffers with the round as kind 2 does: a
    second tree allocates nothing inside mgpu_glob_round."""
    from minotaur_amd.runtime import alloc_stats
    start(ctx, False, (0, 8, 5), 1, brancher=1)
    rounds = 0
    for _ in range(5000):
        s = ctx.glob_round(1)
        rounds += 1
        if s.open == 0:
            break
    # (the last call may pop only nodes the incumbent prunes)
    assert s.open == 0 and s.nodes == 47 <= rounds
    ctx.glob_init(1 << 15)
    for k in range(rounds):
        a0 = alloc_stats()
        s = ctx.glob_round(1)
        assert alloc_stats() == a0, k
        assert s.last_batch == 1
    assert s.open == 0


def test_brancher_one_stays_one_node_per_round(ctx):
    from minotaur_amd import glob as mglob
    qp = random_qcqp(2, nv0=10, ncon=6, squares=False)
    mglob.setup(ctx, qp, 0)
    ctx.glob_config(2, 1, 0, 1, 1)
    ctx.glob_brancher(1)
    ctx.glob_init(1 << 15)
    for _ in range(5):
        s = ctx.glob_round(64)
        assert s.last_batch == 1
    assert s.nodes == 5 and s.rounds == 5
