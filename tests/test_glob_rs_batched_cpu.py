"""CPU: the restatement of the batched relstronger (tests/glob_rs_batched.py,
mgpu_glob_brancher 2).  At batch 1 it is the node-at-a-time restatement
(oracle/glob_tree.py, brancher 1) round for round and solve for solve; at
wider batches every tree closes, with the reference-order optimum where no
node closes at decision 5; and the trees the GPU tests compare against are
not trivial: their wide rounds hold most of the strong branching, every
findBranches outcome, and nodes that need different numbers of lockstep
steps."""
import math

import pytest

from minotaur_amd.quad import random_qcqp
from glob_rs_batched import BatchedRsContext, same_incumbent, stats_key

SLOTS = 8
# (squares, (seed, nv0, ncon))
PIN_CASES = [(False, (2, 10, 6)), (False, (0, 8, 5)), (False, (7, 8, 5)),
             (True, (3, 5, 3)), (True, (33, 6, 4))]
ALL_CASES = PIN_CASES + [(False, (4, 8, 5)), (False, (1, 8, 5)), (False, (11, 6, 4)),
                         (True, (12, 5, 3))]


def make(squares, case, brancher, obbt=1, cls=BatchedRsContext):
    seed, nv0, ncon = case
    qp = random_qcqp(seed, nv0=nv0, ncon=ncon, squares=squares)
    c = cls(qp, tan_slots=SLOTS if squares else 0)
    c.glob_config(2, 1, 0, 1, obbt)
    c.glob_brancher(brancher)
    c.glob_init(1 << 15)
    return c


def run(c, batch, max_rounds=5000):
    for _ in range(max_rounds):
        s = c.glob_round(batch)
        if s.open == 0:
            break
    return s


_trees = {}


def tree(squares, case, batch):
    """The closed batched tree of a case (computed once, shared, read only)."""
    k = (squares, case, batch)
    if k not in _trees:
        c = make(squares, case, 2)
        s = run(c, batch)
        _trees[k] = (c, s)
    return _trees[k]


@pytest.mark.parametrize('obbt', [0, 1])
@pytest.mark.parametrize('squares,case', PIN_CASES)
def test_batch_one_is_the_node_at_a_time_restatement(squares, case, obbt):
    from glob_tree import CpuGlobContext
    a = make(squares, case, 2, obbt)
    b = make(squares, case, 1, obbt, cls=CpuGlobContext)
    for _ in range(5000):
        sa, sb = a.glob_round(1), b.glob_round(1)
        assert stats_key(sa) == stats_key(sb)
        assert sa.last_batch == sb.last_batch == 1
        assert same_incumbent(sa.incumbent, sb.incumbent)
        if sa.open == 0:
            break
    assert sa.open == 0
    assert a.lplog == b.lplog
    oa, xa = a.glob_best()
    ob, xb = b.glob_best()
    assert same_incumbent(oa, ob)
    assert all(p == q or (math.isnan(p) and math.isnan(q)) for p, q in zip(xa, xb))


def test_gpu_cases_reach_every_root_obbt_outcome():
    """The trees of tests/test_glob_rs_batched_gpu.py (its wide cases and its
    batch-1 cases) at obbt 1 reach the three outcomes of the lockstep's root
    OBBT hook: the box tightened and the root's point infeasible to the new
    relaxation, tightened and still feasible, nothing changed."""
    import test_glob_rs_batched_gpu as g

    class Recording(BatchedRsContext):
        def _root_obbt(self, lb, ub, rec, x):
            r = super()._root_obbt(lb, ub, rec, x)
            seen.add((bool(r[0]), bool(r[1])))
            return r

    seen = set()
    for squares, case in g.CASES + g.ONE_CASES:
        make(squares, case, 2, cls=Recording).glob_round(1)   # the root's round
    assert seen == {(True, False), (True, True), (False, True)}


@pytest.mark.parametrize('batch', [4, 16])
@pytest.mark.parametrize('squares,case', ALL_CASES)
def test_wide_batches_close_with_the_same_optimum(squares, case, batch):
    c1, s1 = tree(squares, case, 1)
    cb, sb = tree(squares, case, batch)
    assert s1.open == 0 and sb.open == 0
    assert max(r[0] for r in cb.round_log) >= 2
    if s1.ndec[5] == 0 and sb.ndec[5] == 0:
        v1, vb = s1.incumbent, sb.incumbent
        assert same_incumbent(v1, vb) or abs(vb - v1) <= 1e-6 * max(1.0, abs(v1)), (v1, vb)


def _wide(c):
    return [r for r in c.round_log if r[0] >= 2]


def test_wide_rounds_hold_every_findbranches_outcome():
    c, s = tree(False, (2, 10, 6), 16)
    seen = {o for r in _wide(c) for n in r[1] for o in n[2]}
    assert seen == {'branch', 'mod', 'prune', 'nocand'}


@pytest.mark.parametrize('squares,case', PIN_CASES)
def test_wide_rounds_hold_most_of_the_strong_branching(squares, case):
    c, s = tree(squares, case, 16)
    wide = sum(n[1] for r in _wide(c) for n in r[1])
    assert s.sb_lps > 0 and 2 * wide >= s.sb_lps, (wide, s.sb_lps)


@pytest.mark.parametrize('squares,case', PIN_CASES)
def test_a_wide_round_has_nodes_of_different_lengths(squares, case):
    c, s = tree(squares, case, 16)
    assert any(len({n[1] for n in r[1]}) > 1 for r in _wide(c))
