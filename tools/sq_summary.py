"""Summarise counters-only rocprofv3 passes of the headline
(tools/sq_counters_headline.sh) into one JSON: per engine kernel the counters
per launch (sum over a dispatch's rows, mean over the dispatches of the
dominant grid size) and, for lp_pfi_kernel, per LP of the round (--batch
nodes per launch).

    python tools/sq_summary.py OUT.json NAME=DIR [NAME=DIR ...] [--batch 524288]
"""
import collections
import csv
import glob
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__))))
from pmc_summary import short  # noqa: E402


def one(src):
    files = glob.glob(os.path.join(src, '**', '*counter_collection.csv'), recursive=True)
    assert files, f'no counter_collection.csv under {src}'
    # kernel -> grid -> dispatch -> counter -> sum
    acc = collections.defaultdict(lambda: collections.defaultdict(
        lambda: collections.defaultdict(lambda: collections.defaultdict(float))))
    for f in files:
        for r in csv.DictReader(open(f)):
            k = short(r['Kernel_Name'])
            if k:
                acc[k][str(r['Grid_Size'])][r['Dispatch_Id']][r['Counter_Name']] += \
                    float(r['Counter_Value'])
    out = {}
    for k, grids in acc.items():
        g = max(grids, key=lambda x: len(grids[x]))
        disp = grids[g]
        names = sorted({c for d in disp.values() for c in d})
        rec = {c: sum(d.get(c, 0.0) for d in disp.values()) / len(disp) for c in names}
        rec['launches'] = len(disp)
        rec['grid_size'] = g
        if rec.get('SQ_WAVE_CYCLES') and 'SQ_ACTIVE_INST_VALU' in rec:
            rec['valu_share'] = rec['SQ_ACTIVE_INST_VALU'] / rec['SQ_WAVE_CYCLES']
        out[k] = rec
    return out


def main():
    argv = sys.argv[1:]
    batch = 524288
    if '--batch' in argv:
        i = argv.index('--batch')
        batch = int(argv[i + 1])
        del argv[i:i + 2]
    dst, pairs = argv[0], [a.split('=', 1) for a in argv[1:]]
    res = {"what": "SQ counters per launch of the headline (bench.py --steps 3 --warmup 1 "
                   f"--batch {batch}), one counters-only rocprofv3 pass per build; "
                   "valu_share = SQ_ACTIVE_INST_VALU / SQ_WAVE_CYCLES; per_lp = per launch / "
                   "batch", "batch": batch, "builds": {}}
    for name, src in pairs:
        ks = one(src)
        p = ks.get('lp_pfi_kernel')
        if p and 'SQ_INSTS_VALU' in p:
            p['SQ_INSTS_VALU_per_lp'] = p['SQ_INSTS_VALU'] / batch
        res["builds"][name] = ks
    with open(dst, 'w') as fh:
        json.dump(res, fh, indent=1)
        fh.write('\n')
    for name, ks in res["builds"].items():
        p = ks.get('lp_pfi_kernel', {})
        print(name, 'lp_pfi_kernel SQ_INSTS_VALU per LP', round(p.get('SQ_INSTS_VALU_per_lp', 0), 1),
              'valu_share', round(p.get('valu_share', 0), 4), 'launches', p.get('launches'))


if __name__ == '__main__':
    main()
