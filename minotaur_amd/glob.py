"""Batched spatial branch-and-bound over a QCQP's McCormick relaxation (the
glob path; mgpu_glob_*, minotaur_amd/csrc/glob_runtime.cpp).

The reference's glob solver (src/solvers/Glob.cpp:134-220) runs
BranchAndBound with NodeIncRelaxer, PCBProcessor, the handlers IntVarHandler
/ LinearHandler / QuadHandler of SimpleTransformer and (option
brancher=maxvio) MaxVioBrancher.  Here one round evaluates the top ``batch``
nodes of an HBM stack at once: optionally LinearHandler::presolveNode on the
node's relaxation rows (glob_linear), K2 (QuadHandler::presolveNode, rows
rewritten from the parent's), K3R + K3 (each node's LP with its own rows), the decision,
the squares' separation loop (tangent cuts, re-solve), MaxVio branching,
children pushed.

``solve`` runs one tree on one GPU; ``solve_distributed`` is the node-sharded
multi-GPU form (the MpiBranchAndBound analogue: shared first rounds, a
round-robin shard, one packed all-reduce per round, bound-aware rebalancing
of the open nodes as device rows; mgpu_glob_shard / _rebalance).
"""
from __future__ import annotations

import math
import time

from .quad import relaxation_lp


TAN_SLOTS = 8   # tangent-cut rows per square (QuadHandler::separate's cuts)


def setup(ctx, qp, tan_slots=None):
    """Load a QuadProblem for the glob tree: the quadratic problem, the LP
    relaxation at the root box (QuadHandler::relax_'s rows) and the map of
    the per-node rewritten entries; with squares, ``tan_slots`` tangent-cut
    rows per square for the separation loop (default TAN_SLOTS; 0: none).
    Returns (LinProblem, NodeRows)."""
    ctx.load_quad(qp)
    rows0 = ctx.quad_rows()
    S = (TAN_SLOTS if tan_slots is None else int(tan_slots)) if qp.nsq > 0 else 0
    p, nr = relaxation_lp(qp, rows0, S)
    ctx.load(p)
    ctx.set_node_rows(nr)
    return p, nr


def solve(ctx, qp, batch=1024, capacity=None, max_rounds=10**9, incumbent=math.inf,
          loaded=False, tan_slots=None, order=0, warm=0, qt=1, lin=0, obbt=0, brancher=0):
    """Runs the tree until the stack is empty (or max_rounds): returns
    (incumbent, x or None, stats, seconds).  order / warm / qt / lin / obbt:
    mgpu_glob_config (order 2, warm 1 at batch 1: the reference's own glob
    tree node for node; lin 1: LinearHandler's node presolve too; obbt 1:
    root OBBT).  brancher 2: Glob's relstronger on the device, up to ``batch``
    nodes per round in lockstep under the round rule of mgpu_glob_brancher
    (include/mgpu.h), root OBBT inside the same loop; brancher 1: the same
    with one node per round whatever ``batch`` is (the reference's sequence).
    Both need order 2, warm 1, lin 1."""
    if not loaded:
        setup(ctx, qp, tan_slots)
    cap = capacity or 64 * batch
    t0 = time.perf_counter()
    ctx.glob_config(order, warm, qt, lin, obbt)
    ctx.glob_brancher(brancher)
    ctx.glob_init(cap, incumbent)
    st = None
    for _ in range(max_rounds):
        st = ctx.glob_round(batch)
        if st.open == 0:
            break
    obj, x = ctx.glob_best()
    # a finite objective from an outside incumbent comes without our point
    ok = math.isfinite(obj) and x is not None and not any(math.isnan(v) for v in x)
    return obj, (x if ok else None), st, time.perf_counter() - t0


_MINE = ('nodes', 'lps', 'pivots', 'cuts', 'resolves', 'sb_lps')


def solve_distributed(ctx, qp, batch, rank, world, comm, capacity=None, max_rounds=10**9,
                      loaded=False, tan_slots=None, order=0, warm=0, qt=1, lin=0, obbt=0,
                      brancher=0, incumbent=math.inf, lb_every=0, shard_at=None, trace=None):
    """Node-sharded spatial tree (the MpiBranchAndBound analogue of ``solve``,
    modelled on bnb.solve_distributed).  Every rank runs the same
    deterministic rounds until the pool holds at least ``shard_at`` (default
    4 * world) open nodes, then keeps nodes i = rank (mod world)
    (mgpu_glob_shard) and searches its share.  After every round ONE
    collective (``comm.round_reduce``: minotaur_amd.dist.NativeComm or Comm)
    carries the incumbent (MIN), the open counts and the error flag.  With
    lb_every > 0, every lb_every rounds -- and whenever some rank ran out of
    nodes while another holds more than a batch -- the open nodes are
    rebalanced by their bounds (dist.rebalance(tree='glob'):
    MpiBranchAndBound::LoadBalance_); a migrated node keeps its row state,
    tangent cuts, parent basis and branching record.  Under relstronger every
    rank keeps its own pseudocosts.  A rank whose round fails makes every rank
    raise in the same round.  Returns (incumbent, x or None, stats, rounds,
    mine): x is this rank's point when it holds the incumbent's, mine = this
    rank's own {nodes, ndec, lps, pivots, cuts, resolves, sb_lps, moved,
    lb_log: per rebalance the bounds picked and received}, the shared first
    rounds counted on rank 0 only (sums over ranks are exact).  ``trace`` (a
    list) receives (perf_counter time, all-reduced incumbent) per round."""
    from . import dist as mdist
    if not loaded:
        setup(ctx, qp, tan_slots)
    cap = capacity or 64 * batch
    shard_at = shard_at or 4 * world
    ctx.glob_config(order, warm, qt, lin, obbt)
    ctx.glob_brancher(brancher)
    ctx.glob_init(cap, incumbent)
    inc = incumbent
    sharded = world == 1
    st = None
    rounds = 0
    moved = 0
    shared = None
    lb_log = []

    def counters(s):
        return [getattr(s, k) for k in _MINE] + list(s.ndec)

    while rounds < max_rounds:
        err, exc = 0, None
        try:
            st = ctx.glob_round(batch, inc)
        except Exception as e:              # reported to every rank below
            if world == 1:
                raise
            err, exc = 1, e
        rounds += 1
        open_now = st.open if not err else 0
        if not err and not sharded and (open_now >= shard_at or open_now == 0):
            shared = counters(st)                             # identical on every rank
            open_now = ctx.glob_shard(rank, world)
            sharded = True
        inc_r = st.incumbent if st is not None and not err else math.inf
        inc, most, least, failed = comm.round_reduce(inc_r, open_now, err)
        if failed:
            raise exc if exc is not None else RuntimeError(
                'glob.solve_distributed: a peer rank failed in round %d' % rounds)
        if trace is not None:
            trace.append((time.perf_counter(), inc))
        if most == 0.0:
            break
        # the trigger uses only all-reduced values: every rank agrees
        if sharded and world > 1 and lb_every > 0 and (
                rounds % lb_every == 0 or (least == 0 and most > batch)):
            open_now, k, picked, got = mdist.rebalance(ctx, comm, batch, tree='glob')
            moved += k
            lb_log.append((picked.tolist(), got.tolist()))
    obj, x = ctx.glob_best()
    now = counters(st)
    sub = shared if (rank != 0 and shared is not None) else [0] * len(now)
    own = [v - w for v, w in zip(now, sub)]
    mine = dict(zip(_MINE, own[:len(_MINE)]))
    mine['ndec'] = own[len(_MINE):]
    mine['moved'] = moved
    mine['lb_log'] = lb_log
    ok = obj == inc and math.isfinite(obj) and not any(math.isnan(v) for v in x)
    return inc, (x if ok else None), st, rounds, mine
