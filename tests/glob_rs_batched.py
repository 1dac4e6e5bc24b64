"""CPU restatement of the batched relstronger (mgpu_glob_brancher 2): the rule
for a round of nb > 1 nodes, on top of oracle/glob_tree.py's node-at-a-time
restatement (CpuGlobContext._process_rs).  A helper, not a test.

The rule (include/mgpu.h): the round pops up to ``batch`` nodes in
the reference's order with the round-start incumbent; every node is processed
by _process_rs seeing the round-start incumbent, best_x and pseudocosts plus
its own observations; then, node by node in pop order, the node's observation
log is folded into the shared pseudocosts (updatePCost_'s running mean, in
the order made), its incumbent candidate is taken when strictly better, its
decision is counted and its children are pushed with consecutive ids.  With
one node popped this is brancher 1's sequence."""
import math

from glob_tree import CpuGlobContext


class BatchedRsContext(CpuGlobContext):
    """CpuGlobContext whose glob_brancher(2) rounds take up to ``batch`` nodes."""

    def glob_init(self, capacity, incumbent=math.inf):
        super().glob_init(capacity, incumbent)
        self._obs = None
        # per round: width, per node (decision, strong-branching LPs, the
        # findBranches outcomes in order)
        self.round_log = []
        self._fb = None

    def glob_round(self, batch, incumbent=math.inf):
        if self.brancher != 2:
            return super().glob_round(batch, incumbent)
        if incumbent < self.inc:
            self.inc = incumbent
        return self._round_rs(batch)

    def _upd_pc(self, j, c, down):
        if self._obs is not None:
            self._obs.append((j, c, down))
        super()._upd_pc(j, c, down)

    def _strong(self, lb, ub, rec, x, objval, eng):
        r = super()._strong(lb, ub, rec, x, objval, eng)
        if self._fb is not None:
            self._fb.append(r[0])
        return r

    def _round_rs(self, batch):
        if self.order != 2 or self.warm != 1 or self.lin != 1:
            raise ValueError('relstronger: order 2, warm 1, lin 1')
        tops = []
        while len(tops) < batch and len(self.heap):
            top = self.heap.pop()
            if top['lb'] > self.inc - 1e-6 or \
                    abs(self.inc - top['lb']) / (abs(self.inc) + 1e-6) * 100.0 < 1e-6:
                continue
            tops.append(top)
        if not tops:
            self.tot.open = 0
            return self.tot
        snap = (self.pd.copy(), self.pu.copy(), self.td.copy(), self.tu.copy(), self.inc,
                self.best_x.copy())

        def restore():
            self.pd, self.pu, self.td, self.tu = (snap[0].copy(), snap[1].copy(), snap[2].copy(),
                                                  snap[3].copy())
            self.inc, self.best_x = snap[4], snap[5].copy()

        results = []
        for top in tops:
            restore()
            self._obs, self._fb = [], []
            sb0 = self.tot.sb_lps
            d, kids = self._process_rs(top['node'], top['id'])
            cand = (self.inc, self.best_x.copy()) if self.inc < snap[4] else None
            results.append((d, kids, self._obs, cand, self.tot.sb_lps - sb0, self._fb))
        self._obs = self._fb = None
        restore()
        for d, kids, obs, cand, _, _ in results:
            for j, c, down in obs:
                CpuGlobContext._upd_pc(self, j, c, down)
            if cand is not None and cand[0] < self.inc:
                self.inc, self.best_x = cand
            self.tot.ndec[d] += 1
            for k in kids:
                self.heap.push({'lb': k[3], 'depth': k[4], 'id': self.next_id, 'node': k})
                self.next_id += 1
        self.round_log.append((len(tops), [(r[0], r[4], r[5]) for r in results]))
        self.tot.rounds += 1
        self.tot.nodes += len(tops)
        self.tot.open = len(self.heap)
        self.tot.last_batch = len(tops)
        self.tot.incumbent = self.inc
        return self.tot


def stats_key(s):
    """The per-round comparison tuple of tests/test_glob_rs_squares_gpu.py."""
    return (s.rounds, s.nodes, list(s.ndec), s.br_int, s.br_cont, s.lps, s.pivots, s.sb_lps,
            s.obbt_lps, s.cuts, s.resolves, s.open)


def same_incumbent(a, b):
    return a == b or (math.isinf(a) and math.isinf(b))
