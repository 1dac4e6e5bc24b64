"""CPU: the inputs of tests/quad_cases.py reach every branch of the C
restatement of K2 (oracle/quad_fbbt.c mirrors minotaur_amd/csrc/
quad_fbbt.hip function for function, so its branch coverage under the test
inputs is the measure of how much of the kernel they reach), and the
restatement agrees with the reference itself on every case the reference can
express."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import oracle
import quad_cases as qc
from golden_io import assert_quad_equal, cases, load_quad

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
SRC = os.path.join(ROOT, 'oracle', 'quad_fbbt.c')

# Runs in a fresh python: every quad_cases case, slow_cap, and the inputs of
# tests/test_quad_gpu.py and tests/test_quad_oracle.py, through the
# instrumented build.
CHILD = r'''
import ctypes, sys
sys.path[:0] = sys.argv[2:]
import numpy as np
import oracle
oracle._lib = ctypes.CDLL(sys.argv[1])
import quad_cases as qc
from golden_io import cases, load_quad
from minotaur_amd.quad import objective_at, random_qcqp, random_quad_boxes

for name, (qp, LB, UB, rows, inc, qt, cap) in qc.all_cases().items():
    oracle.quad_fbbt(qp, LB, UB, inc, qt, rows, cap)
for lane in qc.SLOW_LANES:
    qp, LB, UB, rows, inc, qt, cap = qc.slow(qc.SLOW_CAP_C, lane)
    try:
        oracle.quad_fbbt(qp, LB, UB, inc, qt, rows, cap)
    except RuntimeError:
        pass
    else:
        raise SystemExit('slow_cap did not reach the propagation cap')
for name in cases('quad_'):
    qp, g = load_quad(name)
    oracle.quad_root_rows(qp)
    oracle.quad_fbbt(qp, g['lb_in'], g['ub_in'], g['incumbent'], g['qt'], g['rows_in'],
                     g['mod_cap'])
qp = random_qcqp(5, nv0=16, ncon=9)
LB, UB = random_quad_boxes(qp, 5000, 99, edge=True)
inc = objective_at(qp, 0.5 * (qp.vlb[:qp.nv0] + qp.vub[:qp.nv0]))
for qt in (0, 1):
    oracle.quad_fbbt(qp, LB, UB, inc, qt, oracle.quad_root_rows(qp), 96)
qp = random_qcqp(3, nv0=14, ncon=8)
LB, UB = random_quad_boxes(qp, 777, 5, edge=True)
rows0 = np.tile(oracle.quad_root_rows(qp), (777, 1))
o1 = oracle.quad_fbbt(qp, LB, UB, None, 1, rows0)
oracle.quad_fbbt(qp, o1.lb, o1.ub, None, 0, o1.rows)
oracle.quad_update_rows(qp, o1.lb[0], o1.ub[0], rows0[0])
'''

# Branch directions that no valid input reaches: (function, source line, which
# line with that text in the function, branch number as gcov counts it) -> why.
# A valid input is a box with lb <= ub and no NaN and a problem that
# mgpu_load_quad accepts.  At most ALLOW_CAP; if more seem unreachable, the
# cases are incomplete.
UNREACHABLE = {
    ('prop_sqr', '} else if (s->ub[y] < -B_TOL) {', 1, 0):
        'U(y) < -1e-8 here needs update_pbounds(y, lb >= 0, .) just above to have passed, '
        'but lb >= 0 > U(y) + 1e-8 is its infeasible return; a new U(y) is an x^2 >= 0',
    ('calc_var_bnd_univar', 'if (lx > lb2 + B_TOL && lx < ub2 - B_TOL) lb = ub2;', 2, 2):
        'concave arm, ly = -inf: a < 0 gives lb2 - ub2 = sqrt(delta) / |a| > 0, so no lx is '
        'above lb2 and below ub2',
    ('calc_var_bnd_univar', 'if (ux > lb2 + B_TOL && ux < ub2 - B_TOL) ub = lb2;', 2, 2):
        'the same roots: lb2 > ub2, so no ux is above lb2 and below ub2',
    ('tighten_quad', 'clb = clb > il ? clb : il;', 1, 0):
        'objective leg: clb is -inf there and -inf > il is false for every il',
}
ALLOW_CAP = 10


def _gcov_branches(text):
    """[(function, source text, which line with that text in the function
    (from 1), branch no, taken)] of a gcov -b -c listing."""
    out = []
    fn, src, seen = None, None, {}
    for line in text.splitlines():
        m = re.match(r'function (\w+) called', line)
        if m:
            fn = m.group(1)
            continue
        m = re.match(r'\s*(?:[\d#=\-*]+):\s*\d+:(.*)$', line)
        if m:
            src = m.group(1).strip()
            seen[(fn, src)] = seen.get((fn, src), 0) + 1
            continue
        m = re.match(r'branch\s+(\d+) (never executed|taken (\d+))', line)
        if m:
            out.append((fn, src, seen[(fn, src)], int(m.group(1)), int(m.group(3) or 0)))
    return out


def coverage(tmp_path):
    """Builds the instrumented restatement in tmp_path, runs CHILD, returns
    (branches, lines executed, lines) of oracle/quad_fbbt.c."""
    t = str(tmp_path)
    flags = ['-O0', '--coverage', '-fPIC', '-ffp-contract=off', '-std=c11',
             '-Wno-unknown-pragmas']
    subprocess.run(['gcc', *flags, '-I', os.path.dirname(SRC), '-c', SRC, '-o',
                    os.path.join(t, 'quad_fbbt.o')], check=True, cwd=t)
    so = os.path.join(t, 'libquadcov.so')
    subprocess.run(['gcc', '-shared', '--coverage', '-o', so, os.path.join(t, 'quad_fbbt.o'),
                    '-lm'], check=True, cwd=t)
    r = subprocess.run([sys.executable, '-c', CHILD, so, os.path.join(ROOT, 'tests'),
                        os.path.join(ROOT, 'oracle'), ROOT], cwd=t, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run(['gcov', '-b', '-c', '-o', t, SRC], cwd=t, capture_output=True, text=True,
                       check=True)
    m = re.search(r'Lines executed:([\d.]+)% of (\d+)', r.stdout)
    listing = open(os.path.join(t, 'quad_fbbt.c.gcov')).read()
    return _gcov_branches(listing), float(m.group(1)), int(m.group(2))


@pytest.mark.skipif(shutil.which('gcc') is None or shutil.which('gcov') is None,
                    reason='gcc and gcov are needed to measure branch coverage')
def test_quad_cases_take_every_branch(tmp_path):
    br, pct, nlines = coverage(tmp_path)
    assert len(br) > 300, len(br)          # the listing was parsed
    missed = [(f, s, k, n) for (f, s, k, n, taken) in br if taken == 0]
    print(f'oracle/quad_fbbt.c: lines {pct} % of {nlines}; branch directions '
          f'{len(br) - len(missed)} of {len(br)} taken')
    assert len(UNREACHABLE) <= ALLOW_CAP
    stale = [k for k in UNREACHABLE if k not in missed]
    assert not stale, f'allow-listed but taken, or no such line: {stale}'
    allowed = [k for k in missed if k in UNREACHABLE]
    assert len(allowed) <= ALLOW_CAP, allowed
    left = [k for k in missed if k not in UNREACHABLE]
    assert not left, 'branch directions never taken:\n' + '\n'.join(map(str, left))


def _as_golden(r, cap):
    return dict(lb_out=r.lb, ub_out=r.ub, rows_out=r.rows, infeas=r.infeas, nmods=r.nmods,
                mod_kind=r.kind, mod_idx=r.idx, mod_v1=r.v1, mod_v2=r.v2, mod_cap=cap)


@pytest.mark.skipif(not oracle.have_ref(), reason='reference build not present')
@pytest.mark.parametrize('name', [n for n in qc.all_cases() if qc.reference_can_express(n)])
def test_quad_cases_oracle_matches_reference(name):
    """The restatement against the reference's own QuadHandler, bit for bit."""
    qp, LB, UB, rows, inc, qt, cap = qc.all_cases()[name]
    assert rows.ndim == 1
    r = oracle.ref_quad_fbbt(qp, LB, UB, inc, qt, rows, cap)
    o = qc.oracle_result(name)
    assert_quad_equal(o.lb, o.ub, o.rows, o.infeas, o.nmods, o.kind, o.idx, o.v1, o.v2,
                      _as_golden(r, cap))


def test_quad_cases_pins():
    """What the cases are there for, checked on the restatement's answers."""
    for name, (nv0, ncon, nv, lds) in qc.SEEDED.items():
        qp = qc.seeded(name)[0]
        assert qp.nv == nv and qc.lds_bytes(qp) == lds
    assert 64 * 1024 < qc.SEEDED['seeded81'][3] <= 160 * 1024
    assert 64 * 1024 < qc.SEEDED['seeded142'][3] <= 160 * 1024
    assert qc.SEEDED['seeded266'][3] > 160 * 1024
    for lane in qc.SLOW_LANES:
        o = qc.oracle_result(f'slow_converge{lane}')
        assert o.nmods[lane] == 23020 and o.infeas[lane] == 0
        assert (np.delete(o.nmods, lane) < 1000).all()     # the others are ordinary nodes
    o = qc.oracle_result('wide')
    assert {0, 1} <= set(o.infeas.tolist())
