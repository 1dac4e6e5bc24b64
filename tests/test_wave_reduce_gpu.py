"""GPU: the wave64 reductions of csrc/wave.h, one wave at a time
(mgpu_wave_selftest), against a numpy restatement of their contract.

wave_sum_sym's association is the oracle's (oracle/lp_dual.c eta_dot):
partners i^1, i^2, i^7, i^15, then (a[0] + a[16]) + (a[32] + a[48]); sums are
compared bit for bit.  For the maxima: the larger value wins, equal values go
to the lowest lane (wave_argmax_lane) or the lowest index (wave_argmax_idx,
wave_argmax_dpp).  Every helper must leave its result in all 64 lanes, as one
wave of a 64-thread block and as wave 5 of a 1024-thread block.
"""
import os
import re

import numpy as np
import pytest

from minotaur_amd import runtime

pytestmark = pytest.mark.gpu

INT_MAX = np.iinfo(np.int32).max
LANES = np.arange(64)
LAUNCHES = ((64, 0), (1024, 5))
SUM, MAX, MIN, AMAX_LANE, AMAX_IDX, AMAX_DPP, MIN_I32 = range(7)


def rows_sym(x):
    """The four in-row steps: every lane of row k ends with r_k."""
    a = np.asarray(x, np.float64).copy()
    for k in (1, 2, 7, 15):
        a = a + a[LANES ^ k]
    return a


def sum_sym(x):
    a = rows_sym(x)
    return (a[0] + a[16]) + (a[32] + a[48])


def sum_rows_chain(x):
    a = rows_sym(x)
    return ((a[0] + a[16]) + a[32]) + a[48]


def sum_rows_cross(x):
    a = rows_sym(x)
    return (a[0] + a[32]) + (a[16] + a[48])


def sum_lane_order(x):
    s = np.float64(0.0)
    for v in x:
        s = s + v
    return s


def bits(v):
    return np.asarray(v, np.float64).view(np.int64)


def random_vectors():
    out = []
    for s in range(16):
        rng = np.random.default_rng(s)
        out.append(rng.standard_normal(64) * 2.0 ** rng.integers(-20, 21, 64))
    return out


def one_hot(lane, v):
    x = np.zeros(64)
    x[lane] = v
    return x


def sum_cases():
    cs = random_vectors()
    cs += [one_hot(l, 1.0 + l / 64.0) for l in (0, 15, 16, 31, 32, 47, 48, 63)]
    for a, b in ((3, 40), (17, 63), (0, 16)):   # two rows cancel exactly
        x = np.zeros(64)
        x[a], x[b] = 0.1, -0.1
        cs.append(x)
    cs.append(np.zeros(64))
    cs.append(-np.zeros(64))
    cs.append(np.where(LANES % 3 == 0, -0.0, 0.0))
    cs.append(np.where(LANES < 32, -0.0, 0.0))
    return cs


def max_cases():
    """(x, idx) pairs for the max / min / arg-max helpers."""
    cs = []
    for s, x in enumerate(random_vectors()):
        rng = np.random.default_rng(100 + s)
        cs.append((x, rng.permutation(64).astype(np.int32) * 3 + 7))
    for l in (0, 15, 16, 31, 32, 47, 48, 63):
        cs.append((one_hot(l, 2.5), (LANES[::-1] + 64).astype(np.int32)))
        cs.append((one_hot(l, -2.5) + 1.0 - one_hot(l, 1.0), (LANES + 64).astype(np.int32)))
    base = np.random.default_rng(7).uniform(-1.0, 1.0, 64)
    for holders in ((55, 20), (17, 16), (16, 17, 63), (0, 63), (31, 32)):
        # the maximum tied between rows 3 and 1, lanes 17 and 16, ...; the
        # lower lane carries the higher index and the other way round
        for idx in (LANES + 100, 1000 - LANES):
            x = base.copy()
            x[list(holders)] = 4.0
            cs.append((x, idx.astype(np.int32)))
            x = base.copy()
            x[list(holders)] = -4.0    # the same ties for the minimum
            cs.append((x, idx.astype(np.int32)))
    for z in (np.zeros(64), -np.zeros(64), np.where(LANES % 2 == 0, -0.0, 0.0)):
        cs.append((z, (LANES + 5).astype(np.int32)))
    # INFINITY alongside finite values (the ratio test's "no candidate" lanes)
    x = np.full(64, np.inf)
    x[[9, 41]] = 3.0, 2.0
    cs.append((x, (LANES + 1).astype(np.int32)))
    cs.append((np.full(64, np.inf), (LANES + 1).astype(np.int32)))
    # INT_MAX indices: a single holder, all holders of a tie, one holder of a tie
    for holders, imax in (((23,), (23,)), ((5, 50), (5, 50)), ((5, 50), (5,)), ((18, 33), (33,))):
        x = base.copy()
        x[list(holders)] = 9.0
        idx = (LANES * 2 + 11).astype(np.int32)
        idx[list(imax)] = INT_MAX
        cs.append((x, idx))
    cs.append((base.copy(), np.full(64, INT_MAX, np.int32)))
    return cs


def test_rows_constant_matches_header():
    hdr = open(os.path.join(os.path.dirname(__file__), '..', 'include', 'mgpu.h')).read()
    m = re.search(r'#define MGPU_WAVE_SELFTEST_ROWS (\d+)', hdr)
    assert m and int(m.group(1)) == runtime.WAVE_SELFTEST_ROWS


def test_fixtures_tell_the_associations_apart():
    """Each wrong order differs from the symmetric sum on at least one of the
    sixteen random vectors, so a wrong association cannot pass below."""
    vs = random_vectors()
    for wrong in (sum_rows_chain, sum_rows_cross, sum_lane_order):
        assert sum(bits(wrong(x)) != bits(sum_sym(x)) for x in vs) >= 1, wrong.__name__


@pytest.mark.parametrize('block,wave', LAUNCHES)
def test_sum_sym_bits(block, wave):
    k = np.zeros(64, np.int32)
    for n, x in enumerate(sum_cases()):
        d, _ = runtime.wave_selftest(x, k, block, wave)
        want = bits(sum_sym(x))
        assert np.all(bits(d[SUM]) == want), (n, 'wave_sum_sym')


@pytest.mark.parametrize('block,wave', LAUNCHES)
def test_max_min_argmax(block, wave):
    for n, (x, idx) in enumerate(max_cases()):
        d, i = runtime.wave_selftest(x, idx, block, wave)
        mx, mn = x.max(), x.min()
        hold = x == mx
        assert np.all(d[MAX] == mx), (n, 'wave_max_dpp')
        assert np.all(d[MIN] == mn), (n, 'wave_min_dpp')
        assert np.all(d[AMAX_LANE] == mx), (n, 'wave_argmax_lane value')
        assert np.all(i[AMAX_LANE] == np.nonzero(hold)[0][0]), (n, 'wave_argmax_lane')
        for row, name in ((AMAX_IDX, 'wave_argmax_idx'), (AMAX_DPP, 'wave_argmax_dpp')):
            assert np.all(d[row] == mx), (n, name + ' value')
            assert np.all(i[row] == idx[hold].min()), (n, name)
        assert np.all(i[MIN_I32] == idx.min()), (n, 'wave_min_i32_dpp')
        if not np.isinf(mx):
            # finite maxima and minima are one of the inputs, bit for bit
            # (a signed zero may be either zero)
            assert np.all(np.isin(bits(d[MAX]), bits(x[hold])))
            assert np.all(np.isin(bits(d[MIN]), bits(x[x == mn])))
