"""CPU: bench.py's PMC traffic lookup (bench.py:73).  The
roofline's HBM traffic comes only from a summary measured at the same batch
and eta cap, and is marked stale when the summary's engine-source digest
differs from the sources in the tree.  Also --dump-outputs' writer
(bench.dump_outputs) on a stub context."""
import json
import os
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
sys.path.insert(0, ROOT)


def _summary(path, args, digest, bytes_):
    d = {"bench_args": args, "workload": "tree_rounds",
         "kernels": {"lp_pfi_kernel": {"hbm_bytes_per_launch": bytes_}}}
    if digest is not None:
        d["source_digest"] = digest
    with open(path, 'w') as fh:
        json.dump(d, fh)


def test_pmc_traffic_matches_batch_cap_and_digest(tmp_path, monkeypatch):
    import bench
    from minotaur_amd.build import source_digest
    prof = tmp_path / 'profiles'
    prof.mkdir()
    monkeypatch.setattr(bench, 'ROOT', str(tmp_path))
    cur = source_digest()
    _summary(prof / 'r01_pmc.json', '--batch 1024', None, 1.0)
    _summary(prof / 'r02_pmc.json', '--batch 1024 --eta-cap 24', cur, 2.0)
    _summary(prof / 'r03_pmc.json', '--batch 2048', 'not-this-tree', 3.0)
    _summary(prof / 'r04_pmc.json', '--batch 4096', cur, 4.0)
    cap = bench.PFI_DEFAULT
    # default cap, batch 1024: r02 is at another cap, r01 predates digests
    assert bench.pmc_traffic('lp_pfi', 1024, cap, tree=True) == (1.0, 'r01_pmc.json', None)
    assert bench.pmc_traffic('lp_pfi', 1024, 24, tree=True) == (2.0, 'r02_pmc.json', True)
    assert bench.pmc_traffic('lp_pfi', 2048, cap, tree=True) == (3.0, 'r03_pmc.json', False)
    assert bench.pmc_traffic('lp_pfi', 4096, cap, tree=True) == (4.0, 'r04_pmc.json', True)
    assert bench.pmc_traffic('lp_pfi', 8192, cap, tree=True) == (None, None, None)


def test_dump_outputs_writes_float64_arrays_within_budget(tmp_path):
    """--dump-outputs: the last round's stats, the incumbent point and the
    top of the pool as float64 .npy, the rows put back; the pick is capped so
    that open_nodes stays under DUMP_MAX_BYTES."""
    import numpy as np
    import torch
    import bench
    from minotaur_amd.runtime import BnbStats

    class Ctx:
        W, count, imported = 256, 10, None

        def bnb_row_width(self):
            return self.W

        def bnb_best(self):
            return 3.2, np.arange(5.0)

        def bnb_pick(self, S):
            self.S = S
            return np.zeros(min(S, self.count))

        def bnb_export_rows(self, idx):
            # row t is the pick's entry idx[t]; entry i holds i in every column
            return torch.tensor(idx.copy(), dtype=torch.float64)[:, None].repeat(1, self.W)

        def bnb_import_rows(self, rows):
            self.imported = rows

    st = BnbStats()
    st.rounds, st.nodes, st.open, st.incumbent, st.pfi_pivots = 7, 1000, 10, 3.2, 55
    for k in range(5):
        st.ndec[k] = 10 + k
    ctx = Ctx()
    bench.dump_outputs(ctx, 0, 1, st, str(tmp_path / 'out'))
    got = {f: np.load(tmp_path / 'out' / f) for f in os.listdir(tmp_path / 'out')}
    assert sorted(got) == ['incumbent_x.npy', 'open_nodes.npy', 'round_stats.npy']
    assert all(a.dtype == np.float64 for a in got.values())
    rs = got['round_stats.npy']
    assert rs.shape == (len(bench.STATS_FIELDS) + 4,)
    assert rs[:7].tolist() == [7, 1000, 10, 11, 12, 13, 14] and rs[7] == 10 and rs[9] == 3.2
    assert rs[-1] == 55
    assert got['open_nodes.npy'].shape == (10, 256)
    # written topmost first, put back bottom row first (the import stacks
    # row t on row t - 1)
    assert got['open_nodes.npy'][:, 0].tolist() == list(range(10))
    assert ctx.imported[:, 0].tolist() == list(range(9, -1, -1))
    assert ctx.S * ctx.W * 8 <= bench.DUMP_MAX_BYTES < 64 << 20
    assert np.array_equal(got['incumbent_x.npy'], np.arange(5.0))
    # rank r > 0 writes its own files; no incumbent, no incumbent_x
    ctx.bnb_best = lambda: (float('inf'), np.full(5, np.nan))
    bench.dump_outputs(ctx, 1, 8, st, str(tmp_path / 'out1'))
    assert 8 * ctx.S * ctx.W * 8 <= bench.DUMP_MAX_BYTES      # the budget is over all ranks
    assert sorted(os.listdir(tmp_path / 'out1')) == ['open_nodes.rank1.npy',
                                                     'round_stats.rank1.npy']


def test_source_digest_tracks_engine_sources():
    from minotaur_amd import build
    d = build.source_digest()
    assert len(d) == 16 and d == build.source_digest()
