"""GPU: K2 (minotaur_amd/csrc/quad_fbbt.hip) on the named cases of
tests/quad_cases.py, bit for bit against the C restatement: bounds, rows,
status, mod counts and the first min(nmods, cap) log entries, in the auto,
LDS and scratch variants; which variant a shape takes; batch and context
edges; the mod log past its capacity; the propagation cap (status 2) and the
default-bound report (status 3)."""
import numpy as np
import pytest

import oracle
import quad_cases as qc
from golden_io import bits_equal
from minotaur_amd.quad import QuadProblem

pytestmark = pytest.mark.gpu

NAMES = [n for n in qc.all_cases() if n != 'wide']


@pytest.fixture(scope='module')
def ctx():
    from minotaur_amd.runtime import Context
    c = Context(0)
    yield c
    c.close()


def run(ctx, case, variant=0, n=None, mod_cap=None):
    """Loads the case's problem and runs its first n boxes through K2."""
    qp, LB, UB, rows, inc, qt, cap = case
    cap = cap if mod_cap is None else mod_cap
    n = LB.shape[0] if n is None else n
    ctx.load_quad(qp)
    ctx.set_fbbt_variant(variant)
    try:
        return ctx.quad_fbbt(LB[:n], UB[:n], rows if rows.ndim == 1 else rows[:n],
                             np.inf if inc is None else inc, qt, mod_cap=cap)
    finally:
        ctx.set_fbbt_variant(0)


def same_log(r, o, cap, nodes=None):
    """The first min(nmods, cap) entries are the oracle's (the slots past
    them are unspecified on the host path, which copies the device log back
    whole; test_quad_mod_log_overflow checks them on device buffers)."""
    for b in (range(len(o.nmods)) if nodes is None else nodes):
        k = min(int(o.nmods[b]), cap)
        assert np.array_equal(r.kind[b, :k], o.kind[b, :k]), b
        assert np.array_equal(r.idx[b, :k], o.idx[b, :k]), b
        assert bits_equal(r.v1[b, :k], o.v1[b, :k]), b
        assert bits_equal(r.v2[b, :k], o.v2[b, :k]), b


def same(r, o, cap, n=None):
    """r (GPU) against the first n nodes of o (oracle), bit for bit."""
    n = len(o.nmods) if n is None else n
    assert np.array_equal(r.infeasible, o.infeas[:n])
    assert np.array_equal(r.nmods, o.nmods[:n])
    assert bits_equal(r.lb, o.lb[:n]) and bits_equal(r.ub, o.ub[:n])
    assert bits_equal(r.rows, o.rows[:n])
    if cap > 0:
        same_log(r, o, cap, range(n))


@pytest.mark.parametrize('variant', [0, 1, 2])
@pytest.mark.parametrize('name', NAMES)
def test_quad_case_matches_oracle(ctx, name, variant):
    from minotaur_amd.runtime import MgpuError
    case = qc.all_cases()[name]
    if name == 'seeded266' and variant == 1:
        # 282880 B of node state do not fit the CU's LDS: refused, by name
        with pytest.raises(MgpuError, match=str(qc.SEEDED[name][3])):
            run(ctx, case, 1)
        return
    same(run(ctx, case, variant), qc.oracle_result(name), case[6])


def plain_problem(nv):
    """nv continuous variables, no product and no function: maxt = 1, so the
    LDS need is (2 nv + 2) * 520 B."""
    i32 = lambda a: np.asarray(a, dtype=np.int32)
    f64 = lambda a: np.asarray(a, dtype=np.float64)
    return QuadProblem(name=f'plain{nv}', nv0=nv, vtype=i32([4] * nv), vlb=f64([-1.0] * nv),
                       vub=f64([1.0] * nv), sq_x=i32([]), sq_y=i32([]), bil_x0=i32([]),
                       bil_x1=i32([]), bil_y=i32([]), lptr=i32([0]), lvar=i32([]), lval=f64([]),
                       qptr=i32([0]), qv1=i32([]), qv2=i32([]), qval=f64([]), clb=f64([]),
                       cub=f64([]))


def test_quad_variant_choice(ctx):
    """Auto takes LDS while the node state needs at most 40 KiB and scratch
    above; LDS can be forced up to 160 KiB and is refused past it."""
    from minotaur_amd.runtime import MgpuError

    def plans(qp):
        ctx.load_quad(qp)
        out = []
        for v in (0, 1, 2):
            ctx.set_fbbt_variant(v)
            out.append(ctx.quad_plan())
        ctx.set_fbbt_variant(0)
        return out

    for name, (nv0, ncon, nv, lds) in qc.SEEDED.items():
        qp = qc.seeded(name)[0]
        forced = 1 if lds <= 160 * 1024 else 0
        assert plans(qp) == [(2, lds), (forced, lds), (2, lds)], name
    for name, case in qc.micro_cases().items():
        assert plans(case[0]) == [(1, qc.lds_bytes(case[0]))] * 2 + [(2, qc.lds_bytes(case[0]))]
    # the two thresholds, one even step of (2 nv + 2 maxt) on either side
    for nv, auto, forced in ((38, 1, 1), (39, 2, 1), (156, 2, 1), (157, 2, 0)):
        qp = plain_problem(nv)
        lds = (2 * nv + 2) * 520
        assert (lds <= 40 * 1024) == (auto == 1) and (lds <= 160 * 1024) == (forced == 1)
        assert plans(qp) == [(auto, lds), (forced, lds), (2, lds)], nv
        LB, UB = np.tile(qp.vlb, (3, 1)), np.tile(qp.vub, (3, 1))
        LB[1, nv - 1], UB[2, 0] = 0.5, -0.25
        for v in (0, 1, 2):
            ctx.set_fbbt_variant(v)
            try:
                if v == 1 and not forced:
                    with pytest.raises(MgpuError, match=str(lds)):
                        ctx.quad_fbbt(LB, UB, qt=1)
                    continue
                r = ctx.quad_fbbt(LB, UB, qt=1)
            finally:
                ctx.set_fbbt_variant(0)
            assert bits_equal(r.lb, LB) and bits_equal(r.ub, UB) and not r.infeasible.any()
    # auto solves the shape that LDS refuses
    same(run(ctx, qc.seeded('seeded266'), 0), qc.oracle_result('seeded266'), 96)


@pytest.mark.parametrize('variant', [1, 2])
def test_quad_batch_edges(ctx, variant):
    """A node's answer does not depend on the batch it is in: batches of 1,
    63, 64, 65 and 130 against the same nodes of the full batch of 160."""
    case = qc.seeded('seeded81')
    o = qc.oracle_result('seeded81')
    full = run(ctx, case, variant)
    same(full, o, case[6])
    for n in (1, 63, 64, 65, 130):
        r = run(ctx, case, variant, n=n)
        same(r, o, case[6], n)
        assert bits_equal(r.lb, full.lb[:n]) and bits_equal(r.ub, full.ub[:n])
        assert bits_equal(r.rows, full.rows[:n]) and np.array_equal(r.nmods, full.nmods[:n])


def test_quad_buffers_regrow():
    """A fresh context: a small batch, a larger one with a longer mod log,
    then a small one again (scratch and staging buffers grow, then are
    reused larger than needed)."""
    from minotaur_amd.runtime import Context
    c = Context(0)
    try:
        case = qc.seeded('seeded81')
        o = qc.oracle_result('seeded81')
        for variant in (2, 0):
            for n, cap in ((3, 96), (160, 96), (2, 96), (65, 0), (160, 96)):
                r = run(c, case, variant, n=n, mod_cap=cap)
                same(r, o, cap, n)
    finally:
        c.close()


def test_quad_reload_problem(ctx):
    """Problem A, then B, then A again on one context: A's answers are the
    same (nothing of B's registries, programs or scratch is left)."""
    A, B = qc.unbounded_linear(), qc.seeded('seeded142')
    for variant in (1, 2):
        a1 = run(ctx, A, variant)
        same(run(ctx, B, variant), qc.oracle_result('seeded142'), B[6])
        a2 = run(ctx, A, variant)
        same(a1, qc.oracle_result('unbounded_linear'), A[6])
        same(a2, qc.oracle_result('unbounded_linear'), A[6])
        assert bits_equal(a1.lb, a2.lb) and bits_equal(a1.rows, a2.rows)


@pytest.mark.parametrize('variant', [0, 2])
@pytest.mark.parametrize('lane', qc.SLOW_LANES)
def test_quad_mod_log_overflow(ctx, lane, variant):
    """23020 mods into 16 slots: the count is the oracle's, the first 16
    entries too, and no other node's slots are written."""
    case = qc.slow(qc.SLOW_CONVERGE_C, lane, 16)
    qp, LB, UB, rows, inc, qt, cap = case
    o = oracle.quad_fbbt(qp, LB, UB, inc, qt, rows, 16)
    assert o.nmods[lane] == 23020
    r = run(ctx, case, variant)
    same(r, o, 16)
    # on device buffers: the slots past min(nmods, 16) of every node, the
    # slow node's neighbours included, keep the caller's fill
    import torch
    dev = torch.device('cuda', 0)
    t = lambda a: torch.from_numpy(np.array(a)).to(dev)
    lb, ub = t(LB), t(UB)
    olb, oub = torch.empty_like(lb), torch.empty_like(ub)
    orow = torch.empty((65, qp.nrow_state), dtype=torch.float64, device=dev)
    inf = torch.zeros(65, dtype=torch.int32, device=dev)
    nm = torch.zeros(65, dtype=torch.int32, device=dev)
    # one spare slot behind the last node's, which must stay as it is too
    flat = [torch.full((65 * 16 + 1,), -7, dtype=d, device=dev)
            for d in (torch.int32, torch.int32, torch.float64, torch.float64)]
    kind, idx, v1, v2 = (f[:65 * 16].view(65, 16) for f in flat)
    torch.cuda.synchronize()
    ctx.set_fbbt_variant(variant)
    try:
        ctx.quad_fbbt_dev(lb, ub, t(rows), olb, oub, orow, inf, nm, qt=qt, mod_kind=kind,
                          mod_idx=idx, mod_v1=v1, mod_v2=v2)
        ctx.sync()
    finally:
        ctx.set_fbbt_variant(0)
    assert np.array_equal(nm.cpu().numpy(), o.nmods)
    assert all(float(f[-1]) == -7 for f in flat)
    kind, idx, v1, v2 = (a.cpu().numpy() for a in (kind, idx, v1, v2))
    for b in range(65):
        k = min(int(o.nmods[b]), 16)
        assert np.array_equal(kind[b, :k], o.kind[b, :k]) and bits_equal(v1[b, :k], o.v1[b, :k])
        assert (kind[b, k:] == -7).all() and (idx[b, k:] == -7).all(), b
        assert (v1[b, k:] == -7.0).all() and (v2[b, k:] == -7.0).all(), b
    # no log at all through the host path
    r0 = run(ctx, case, variant, mod_cap=0)
    assert r0.kind is None
    same(r0, o, 0)


@pytest.mark.parametrize('variant', [0, 2])
@pytest.mark.parametrize('lane', qc.SLOW_LANES)
def test_quad_propagation_cap(ctx, lane, variant):
    """The node that would need about 690 000 passes stops at 100 000 with
    status 2 (its bounds and rows are unspecified); the other 64 nodes are
    those of the oracle run without it."""
    case = qc.slow(qc.SLOW_CAP_C, lane)
    qp, LB, UB, rows, inc, qt, cap = case
    keep = np.arange(65) != lane
    o = oracle.quad_fbbt(qp, LB[keep], UB[keep], inc, qt, rows, cap)
    r = run(ctx, case, variant)
    print(f"slow_cap lane {lane} variant {variant}: {ctx.last_kernel_ms('quad'):.1f} ms")
    assert r.infeasible[lane] == 2
    assert np.array_equal(r.infeasible[keep], o.infeas)
    assert np.array_equal(r.nmods[keep], o.nmods)
    assert bits_equal(r.lb[keep], o.lb) and bits_equal(r.ub[keep], o.ub)
    assert bits_equal(r.rows[keep], o.rows)
    for f in ('kind', 'idx', 'v1', 'v2'):
        setattr(r, f, getattr(r, f)[keep])
    same_log(r, o, cap)


@pytest.mark.parametrize('variant', [0, 1, 2])
def test_quad_default_bound_status(ctx, variant):
    """Status 3 exactly where the oracle's run of the same box is feasible
    and rewrites a row of a variable beyond 1e12 (the reference would add a
    default bound there); bounds are the oracle's everywhere, rows wherever
    no wide variable is involved, and infeasible wide nodes stay 1."""
    case = qc.wide()
    qp, LB, UB, rows, inc, qt, cap = case
    o = qc.oracle_result('wide')
    assert int(o.nmods.max()) <= cap
    r = run(ctx, case, variant)
    wide_var = (o.lb < -1e12) | (o.ub > 1e12)                 # [B, nv]
    xs = ([(int(x),) for x in qp.sq_x] +
          [(int(a), int(b)) for a, b in zip(qp.bil_x0, qp.bil_x1) for _ in range(4)])
    wide_row = np.array([[wide_var[b, list(v)].any() for v in xs] for b in range(len(LB))])
    want = o.infeas.copy()
    for b in range(len(LB)):
        k = int(o.nmods[b])
        rebuilt = o.idx[b, :k][o.kind[b, :k] == 3]
        if o.infeas[b] == 0 and wide_row[b, rebuilt].any():
            want[b] = 3
    assert {0, 1, 3} <= set(want.tolist())
    assert ((want == 0) & wide_var.any(axis=1)).any()        # wide, nothing rebuilt
    assert ((want == 1) & wide_var.any(axis=1)).any()        # wide and infeasible
    assert np.array_equal(r.infeasible, want)
    assert np.array_equal(r.nmods, o.nmods)
    assert bits_equal(r.lb, o.lb) and bits_equal(r.ub, o.ub)
    # row state entries of each relaxation row: 2 per square, 3 per McCormick row
    ent = np.repeat(np.arange(len(xs)), [2] * qp.nsq + [3] * (4 * qp.nbil))
    for b in range(len(LB)):
        ok = ~wide_row[b][ent]
        assert bits_equal(r.rows[b][ok], o.rows[b][ok]), b
    same_log(r, o, cap)
