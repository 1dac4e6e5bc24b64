"""GPU: a plain bench.py run (small batch, two timed rounds) prints the line
with the headline fields and none of the --full objects, and --dump-outputs
writes the last round's outputs as float64 arrays."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))

pytestmark = pytest.mark.gpu


def test_dump_leaves_the_pool_as_it_was(tmp_path, monkeypatch):
    """dump_outputs takes the top of the depth-first stack out and puts it
    back: a second dump, and a larger pick after it, see the same nodes in
    the same order."""
    sys.path.insert(0, ROOT)
    import bench
    from minotaur_amd.problem import LinProblem, random_boxes
    from minotaur_amd.runtime import Context
    p = LinProblem.load(os.path.join(ROOT, 'minotaur_amd', 'instances', 'tls4_oa.npz'))
    LB, UB = random_boxes(p, 300, 5)
    ctx = Context(0)
    try:
        ctx.load(p)
        ctx.bnb_config(0, 2)
        ctx.bnb_brancher(0)
        ctx.bnb_init(4096)
        ctx.bnb_import(LB, UB, np.full(300, -np.inf), np.zeros(300, dtype=np.int32))
        st = ctx.bnb_round(256)
        assert st.open > 32
        before = ctx.bnb_pick(st.open)
        # a budget of 32 rows: the dump moves a part of the pool only
        monkeypatch.setattr(bench, 'DUMP_MAX_BYTES', 32 * 8 * ctx.bnb_row_width())
        bench.dump_outputs(ctx, 0, 1, st, str(tmp_path / 'a'))
        after = ctx.bnb_pick(st.open)
        bench.dump_outputs(ctx, 0, 1, st, str(tmp_path / 'b'))
        a, b = np.load(tmp_path / 'a' / 'open_nodes.npy'), np.load(tmp_path / 'b' / 'open_nodes.npy')
        assert a.shape == (32, ctx.bnb_row_width()) and np.array_equal(a, b)
        assert np.array_equal(before, after)
        # topmost first: the rows' bounds are the pick's
        assert np.array_equal(a[:, 2 * p.n], before[:32])
        assert ctx.bnb_count()[0] == st.open
    finally:
        ctx.close()


def test_plain_run_line_and_dumped_outputs(tmp_path):
    out = tmp_path / 'dump'
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps',
                        '2', '--warmup', '1', '--batch', '4096', '--dump-outputs', str(out)],
                       cwd=str(tmp_path), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d['steps'] == 2 and d['unit'] == 'nodes/s' and d['dtype'] == 'f64'
    assert d['higher_is_better'] is True and d['value'] > 0 and d['ms_per_step'] > 0
    # value is nodes per second of the two timed rounds (the line keeps four
    # significant digits of the node count)
    assert abs(d['value'] * d['ms_per_step'] * 1e-3 * 2 - d['tree_rounds']['nodes']) \
        <= 1e-3 * d['tree_rounds']['nodes']
    for k in ('cpu_baseline', 'tls4_oa_tree', 'tls4_oa_rel_tree', 'supplementary'):
        assert k not in d
    # a plain run writes nothing but the dump
    assert sorted(os.listdir(tmp_path)) == ['dump']
    rs = np.load(out / 'round_stats.npy')
    rows = np.load(out / 'open_nodes.npy')
    assert rs.dtype == np.float64 and rows.dtype == np.float64
    # rounds: 1 warm-up + 2 timed; the open count is the pool the rows come from
    assert rs[0] == 3 and rows.ndim == 2 and 0 < rows.shape[0] <= rs[7]
    n = 105                                   # tls4-oa columns: rows are [lb | ub | ...]
    assert np.all(rows[:, :n] <= rows[:, n:2 * n])
    assert sum(os.path.getsize(out / f) for f in os.listdir(out)) <= 64 << 20
