"""Static ISA statistics of K3P (lp_pfi_kernel), no GPU needed.

Cross-compiles csrc/lp_pfi.hip to gfx950 assembly with the flags of
minotaur_amd/build.py and prints, per lp_pfi_kernel<S, K> instantiation, the
register figures of the code object's metadata (.vgpr_count,
.vgpr_spill_count, .sgpr_spill_count), the static count of vector (v_*)
instructions, and how many of those are lane writes / lane reads of the
VGPRs that hold spilled scalar registers.  The kernel's sources never write
a single lane themselves, so every VGPR that is the destination of a
v_writelane_b32 is such a spill register.  K3P's vector pipe is ~93 % busy
(profiles/r06al_sq_counters.json), so these counts are what its time follows.

    python tools/k3p_isa_stats.py [--csrc DIR] [--out FILE.json] [--keep-asm FILE.s]
"""
import argparse
import collections
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

META_KEYS = ('.vgpr_count', '.vgpr_spill_count', '.sgpr_spill_count', '.sgpr_count',
             '.private_segment_fixed_size')


def assemble(csrc, asm_path):
    from minotaur_amd import build as b
    flags = [f for f in b.FLAGS if f != '-shared']
    cmd = ([b.HIPCC] + flags + ['-I', os.path.join(ROOT, 'include'), '--cuda-device-only', '-S',
                                '-o', asm_path, os.path.join(csrc, 'lp_pfi.hip')])
    subprocess.run(cmd, check=True)


def tmpl(sym):
    """lp_pfi_kernel<S, K> from the mangled name (...lp_pfi_kernelILi3ELi32EE...)."""
    m = re.search(r'lp_pfi_kernelILi(\d+)ELi(\d+)EE', sym)
    return f'lp_pfi_kernel<{m.group(1)},{m.group(2)}>' if m else None


def parse(asm_path):
    lines = open(asm_path).read().split('\n')
    # kernel bodies: from the symbol's label to its s_endpgm-terminated end
    body = collections.OrderedDict()
    cur = None
    for ln in lines:
        m = re.match(r'^(_Z\w+):', ln)
        if m:
            cur = m.group(1) if tmpl(m.group(1)) else None
            if cur:
                body[cur] = []
            continue
        if cur is not None:
            if ln.startswith('.Lfunc_end'):
                cur = None
                continue
            s = ln.strip()
            if s and not s.startswith(('.', ';')) and not s.endswith(':'):
                body[cur].append(s)
    # metadata: one YAML record per kernel, opened by a list item at the
    # kernels' indentation ("  - .agpr_count: ...")
    meta = {}
    rec = {}
    for ln in lines:
        if re.match(r'^  - \.', ln) or ln.startswith('amdhsa.target'):
            if tmpl(rec.get('.name', '')):
                meta[rec['.name']] = rec
            rec = {}
        m = re.match(r'^\s+(?:- )?(\.\w+):\s+(\S+)\s*$', ln)
        if not m:
            continue
        k, v = m.groups()
        if k in META_KEYS and len(ln) - len(ln.lstrip()) <= 4:
            rec[k] = int(v)
        elif k == '.name' and len(ln) - len(ln.lstrip()) <= 4:
            rec['.name'] = v
    if tmpl(rec.get('.name', '')):
        meta[rec['.name']] = rec
    out = collections.OrderedDict()
    for sym, ins in sorted(body.items(), key=lambda kv: tmpl(kv[0])):
        spill = set()
        for s in ins:
            m = re.match(r'v_writelane_b32\s+(v\d+),', s)
            if m:
                spill.add(m.group(1))
        valu = [s for s in ins if s.startswith('v_')]
        wl = sum(1 for s in valu if re.match(r'v_writelane_b32\s+(v\d+),', s))
        rl_all = [s for s in valu if s.startswith('v_readlane_b32')]
        rl_spill = sum(1 for s in rl_all
                       if re.match(r'v_readlane_b32\s+\S+,\s*(v\d+),', s).group(1) in spill)
        mnem = collections.Counter(s.split()[0] for s in ins)
        md = meta.get(sym, {})
        out[tmpl(sym)] = {
            'vgpr_count': md.get('.vgpr_count'),
            'vgpr_spill_count': md.get('.vgpr_spill_count'),
            'sgpr_spill_count': md.get('.sgpr_spill_count'),
            'scratch_bytes_per_lane': md.get('.private_segment_fixed_size'),
            'valu': len(valu),
            'spill_regs': len(spill),
            'spill_lane_writes': wl,
            'spill_lane_reads': rl_spill,
            'v_readlane': len(rl_all),
            'v_mov_b32': mnem['v_mov_b32_e32'],
            'v_mov_b32_dpp': mnem['v_mov_b32_dpp'],
            'v_cmp_lt_i32': mnem['v_cmp_lt_i32_e32'] + mnem['v_cmp_lt_i32_e64'],
            's_and_saveexec': mnem['s_and_saveexec_b64'],
        }
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--csrc', default=os.path.join(ROOT, 'minotaur_amd', 'csrc'),
                    help='source directory holding lp_pfi.hip (a tools/_stamps/<name>/csrc copy '
                         'for a variant)')
    ap.add_argument('--out', default=None, help='also write the table as JSON')
    ap.add_argument('--keep-asm', default=None, help='keep the assembly at this path')
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as td:
        asm = args.keep_asm or os.path.join(td, 'lp_pfi.s')
        assemble(args.csrc, asm)
        tab = parse(asm)
    cols = ['vgpr_count', 'vgpr_spill_count', 'sgpr_spill_count', 'valu', 'spill_lane_writes',
            'spill_lane_reads', 'v_readlane', 'v_mov_b32', 's_and_saveexec']
    print(f"{'kernel':22s}" + ''.join(f'{c:>18s}' for c in cols))
    for k, r in tab.items():
        print(f'{k:22s}' + ''.join(f'{str(r[c]):>18s}' for c in cols))
    if args.out:
        with open(args.out, 'w') as fh:
            json.dump(tab, fh, indent=1)
            fh.write('\n')


if __name__ == '__main__':
    main()
