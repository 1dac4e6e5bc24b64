"""CPU: the interior-point restatement (oracle/qp_ipm.py) solves every case
of tests/qp_cases.py -- each kernel-variant shape of K5 with its four node
boxes, and the 'lp' / 'bigc' families -- with a KKT certificate, and meets
HiGHS on the LPs.  tests/test_qp_shapes_gpu.py compares K5 with these
answers, so a case the restatement could not solve would check nothing."""
import numpy as np
import pytest

import qp_cases
import qp_ipm


def _certified(P, LB, UB, ref):
    sp = 1.0 + np.max(np.abs(P.b), initial=0.0)   # as the solver scales its tolerances
    sd = 1.0 + np.max(np.abs(P.c), initial=0.0)
    for b, r in enumerate(ref):
        assert r['status'] == 0, b
        cert = qp_ipm.kkt_certificate(P.Q, P.c, P.A, P.b, LB[b], UB[b], r['x'], r['y'], r['zl'],
                                      r['zu'])
        assert cert['rp'] <= 1e-8 * sp and cert['rd'] <= 1e-8 * sd, (b, cert)
        assert cert['box'] == 0.0 and cert['zmin'] >= 0.0, (b, cert)


@pytest.mark.parametrize('n,m', qp_cases.SHAPES)
def test_restatement_solves_every_shape(n, m):
    P, LB, UB, x0 = qp_cases.case(n, m)
    assert (P.n, P.m) == (n, m) and LB.shape == (4, n)
    assert np.all(LB <= x0) and np.all(x0 <= UB)          # every node is feasible
    assert np.array_equal(LB[0], P.l) and np.array_equal(UB[0], P.u)
    _certified(P, LB, UB, qp_cases.reference((n, m)))


@pytest.mark.parametrize('key', qp_cases.FAMILY, ids=lambda k: '-'.join(f'{v:g}' if isinstance(
    v, float) else str(v) for v in k))
def test_restatement_solves_the_families(key):
    P, LB, UB = qp_cases.family_case(*key)
    ref = qp_cases.reference(key)
    _certified(P, LB, UB, ref)
    if key[0] == 'lp':
        f = qp_cases.highs_lp(P, LB[0], UB[0])
        assert abs(ref[0]['obj'] + P.k - f) <= 1e-6 * max(1.0, abs(f))


def test_case_counts():
    """Nothing is filtered: 20 shapes of four nodes, 18 LPs, 9 'bigc' QPs."""
    assert len(qp_cases.SHAPES) == 20 and len(set(qp_cases.FAMILY)) == 27
    assert sum(k[0] == 'lp' for k in qp_cases.FAMILY) == 18
