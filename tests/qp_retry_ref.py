"""CPU restatement of K5's coupled step (mgpu_qp_step_rule 1) and of the retry
pass (rule 2) in the branch-and-bound over QP relaxations.

``solve_node_rule`` is oracle/qp_ipm.py's solve_node, operation for operation,
with the step rule as an argument: rule 0 is solve_node itself (the CPU test
compares the bits), rule 1 takes one common step length min(ap, ad) for the
corrected step, after the fraction to the boundary and the cap at 1.  The
predictor's two step lengths, which enter mu_aff, stay separate under either
rule.

``RetryBnbContext`` places the retry where qp_solve_nodes of
minotaur_amd/csrc/qp_runtime.cpp places it in a tree: after the phase-1 LP has
settled the infeasible nodes among those the first pass left at status 6, on
the remainder only.
"""
import numpy as np

import bnb as obnb
import oracle
import qp_ipm
from qp_ipm import MAXIT, REG, STEP, TOL_D, TOL_MU, TOL_P, _bwd, _chol, _fwd, _max_step


def solve_node_rule(Q, c, A, b, l, u, rule, maxit=MAXIT):
    """One node: returns dict(status, obj, x, y, zl, zu, iters).
    status 0 converged, 6 iteration limit."""
    n = Q.shape[0]
    fixed = l >= u
    free = ~fixed
    nf = int(free.sum())
    x = np.where(free, 0.5 * (l + u), l)
    y = np.zeros(A.shape[0])
    zl = np.where(free, 1.0, 0.0)
    zu = np.where(free, 1.0, 0.0)
    Af = A.copy()
    Af[:, fixed] = 0.0
    tp = TOL_P * (1.0 + np.max(np.abs(b), initial=0.0))
    td = TOL_D * (1.0 + np.max(np.abs(c), initial=0.0))
    status = 6
    it = 0
    for it in range(maxit):
        sl = np.where(free, x - l, 1.0)
        su = np.where(free, u - x, 1.0)
        rd = np.where(free, Q @ x + c - A.T @ y - zl + zu, 0.0)
        rp = b - A @ x
        mu = float((sl[free] @ zl[free] + su[free] @ zu[free]) / max(2 * nf, 1))
        tpx = max(tp, TOL_P * (1.0 + float(np.max(np.abs(x), initial=0.0))))
        if np.max(np.abs(rp), initial=0.0) <= tpx and np.max(np.abs(rd), initial=0.0) <= td \
                and mu <= TOL_MU:
            status = 0
            break
        D = np.where(free, zl / sl + zu / su, 0.0)
        K = Q + np.diag(D)
        K[fixed, :] = 0.0
        K[:, fixed] = 0.0
        K[fixed, fixed] = 1.0
        L = _chol(K)
        W = _fwd(L, Af.T)
        M = W.T @ W
        M += REG * (1.0 + np.max(np.diag(M), initial=0.0)) * np.eye(M.shape[0])
        Lm = _chol(M)

        def solve(r1):
            v = _fwd(L, r1)
            dy = _bwd(Lm, _fwd(Lm, rp - W.T @ v))
            dx = _bwd(L, v + W @ dy)
            return np.where(free, dx, 0.0), dy

        # predictor (affine scaling): separate step lengths under either rule
        r1 = np.where(free, -rd - zl + zu, 0.0)
        dx, dy = solve(r1)
        dzl = np.where(free, -zl - (zl / sl) * dx, 0.0)
        dzu = np.where(free, -zu + (zu / su) * dx, 0.0)
        ap = min(_max_step(sl[free], dx[free]), _max_step(su[free], -dx[free]))
        ad = min(_max_step(zl[free], dzl[free]), _max_step(zu[free], dzu[free]))
        mu_aff = float(((sl + ap * dx)[free] @ (zl + ad * dzl)[free]
                        + (su - ap * dx)[free] @ (zu + ad * dzu)[free]) / max(2 * nf, 1))
        sigma = (mu_aff / mu) ** 3 if mu > 0 else 0.0
        # corrector
        rl = sigma * mu - sl * zl - dx * dzl
        ru = sigma * mu - su * zu + dx * dzu
        r1 = np.where(free, -rd + rl / sl - ru / su, 0.0)
        dx, dy = solve(r1)
        dzl = np.where(free, (rl - zl * dx) / sl, 0.0)
        dzu = np.where(free, (ru + zu * dx) / su, 0.0)
        ap = STEP * min(_max_step(sl[free], dx[free]), _max_step(su[free], -dx[free]))
        ad = STEP * min(_max_step(zl[free], dzl[free]), _max_step(zu[free], dzu[free]))
        ap, ad = min(ap, 1.0), min(ad, 1.0)
        if rule:
            ap = ad = min(ap, ad)
        x = x + ap * dx
        y = y + ad * dy
        zl = zl + ad * dzl
        zu = zu + ad * dzu
    obj = float(0.5 * x @ Q @ x + c @ x)
    return dict(status=status, obj=obj, x=x, y=y, zl=zl, zu=zu, iters=it)


def solve_node_coupled(Q, c, A, b, l, u, maxit=MAXIT):
    """Rule 1: the coupled step."""
    return solve_node_rule(Q, c, A, b, l, u, 1, maxit)


def solve_node_retry(Q, c, A, b, l, u, maxit=MAXIT):
    """Rule 2 on one node, as mgpu_qp_solve counts it: the separate step, and
    where that ends at status 6 the coupled step from the start; then iters =
    the first pass's limit + the second's own count.  'retried' tells which."""
    with np.errstate(all='ignore'):
        r = qp_ipm.solve_node(Q, c, A, b, l, u, maxit)
    if r['status'] == 0:
        return dict(r, retried=False)
    with np.errstate(all='ignore'):
        r = solve_node_coupled(Q, c, A, b, l, u, maxit)
    r['iters'] = maxit + (r['iters'] if r['status'] == 0 else maxit)
    return dict(r, retried=True)


class RetryBnbContext(obnb.CpuBnbContext):
    """CpuBnbContext with mgpu_qp_step_rule 2: a node the first pass left at
    status 6 and the phase-1 LP found feasible is solved again with the
    coupled step.  ``nretried`` / ``nretry_solved`` count those nodes and
    ``retried`` records their boxes as ``ipm`` records the first pass's;
    ``first_retry_round`` is the round (from 0) of the first of them."""

    def bnb_init(self, *a, **kw):
        super().bnb_init(*a, **kw)
        self.nretried = self.nretry_solved = 0
        self.retried = []
        self.first_retry_round = None

    def _qp_nodes(self, f, keep, status, obj, x):
        p, P = self.problem, self.qp
        self.nskip += len(status) - len(keep)
        unsettled = []
        for i in keep:
            l, u = f.lb[i], f.ub[i]
            if np.any(l > u):     # qp_init: infeasible before any iteration
                status[i] = 2
                self.tot.lps += 1
                continue
            key = (l.tobytes(), u.tobytes())
            r = self.qp_cache.get(key)
            if r is None:
                with np.errstate(all='ignore'):
                    r = qp_ipm.solve_node(P.Q, P.c, P.A, P.b, l, u)
                r['iters'] = r['iters'] if r['status'] == 0 else MAXIT
                self.qp_cache[key] = r
            self.ipm.append(dict(lb=l.copy(), ub=u.copy(), status=r['status'],
                                 obj=r['obj'] + P.k, x=r['x'], iters=r['iters']))
            if r['status'] == 0:
                status[i], obj[i], x[i] = 0, r['obj'] + P.k, r['x']
                self.nsolved += 1
                self.tot.lps += 1
                self.tot.pivots += r['iters']
            else:
                unsettled.append(i)
        if not unsettled:
            return
        lst = oracle.dual_simplex(p, f.lb[unsettled], f.ub[unsettled], None)[0]
        for i, s in zip(unsettled, lst):
            if s == 2:
                status[i] = 2
                self.nsettled += 1
                self.tot.lps += 1
                self.tot.pivots += MAXIT
                continue
            # feasible rows: the retry, from the start, at the same limit
            l, u = f.lb[i], f.ub[i]
            key = ('coupled', l.tobytes(), u.tobytes())
            r = self.qp_cache.get(key)
            if r is None:
                with np.errstate(all='ignore'):
                    r = solve_node_coupled(P.Q, P.c, P.A, P.b, l, u)
                r['iters'] = r['iters'] if r['status'] == 0 else MAXIT
                self.qp_cache[key] = r
            self.nretried += 1
            if self.first_retry_round is None:
                self.first_retry_round = int(self.tot.rounds)
            self.retried.append(dict(lb=l.copy(), ub=u.copy(), status=r['status'],
                                     obj=r['obj'] + P.k, x=r['x'], iters=r['iters']))
            if r['status'] == 0:
                status[i], obj[i], x[i] = 0, r['obj'] + P.k, r['x']
                self.nretry_solved += 1
                self.nsolved += 1
                self.tot.lps += 1
                self.tot.pivots += MAXIT + r['iters']   # the steps taken in both passes
            else:             # still a feasible QP the interior point did not solve
                status[i] = 12
                self.nstatus12 += 1
