#!/usr/bin/env python3
"""The device code of a tree as a table, to compare two trees after a refactor that must not change a kernel (no GPU needed).

    python scripts/kernel_table.py --root . --out tree.json            # compile + print the summary, write the table
    python scripts/kernel_table.py --diff parent.json tree.json        # names, register / LDS / scratch numbers, bodies

Every .hip of drecpy_amd.build.SOURCES is compiled with the library's flags plus --cuda-device-only --no-gpu-bundle-output into a
plain elf64-amdgpu object.  Table: mangled kernel name -> sorted list of distinct
[vgpr, agpr, sgpr, LDS bytes, scratch bytes, sha1 of the body's instruction words] over all code objects, and per unit its names.
"""
import argparse, hashlib, importlib.util, json, os, re, subprocess, sys, tempfile

LLVM = os.environ.get('LLVM_BIN', '/opt/rocm/llvm/bin')
FIELDS = ('.vgpr_count', '.agpr_count', '.sgpr_count', '.group_segment_fixed_size', '.private_segment_fixed_size')


def run(*cmd):
    return subprocess.run(cmd, check=True, capture_output=True, text=True).stdout


def unit_table(obj):
    """{kernel: [five numbers, body hash]} of one code object."""
    meta, cur = {}, None
    for line in run(f'{LLVM}/llvm-readelf', '--notes', obj).splitlines():
        m = re.match(r'\s+(?:- )?(\.\w+):\s+(\S+)$', line)
        if not m:
            continue
        if m.group(1) == '.agpr_count':              # (keys come sorted: the first of a kernel's record)
            cur = {}
        if cur is not None and m.group(1) in FIELDS + ('.symbol',):
            cur[m.group(1)] = m.group(2)
        if cur is not None and m.group(1) == '.vgpr_count':
            meta[cur['.symbol'][:-3]] = [int(cur[f]) for f in FIELDS]
            cur = None
    body, name = {}, None
    for line in run(f'{LLVM}/llvm-objdump', '-d', obj).splitlines():
        m = re.match(r'[0-9a-f]+ <(\S+)>:$', line)
        if m:
            name = m.group(1)
            body[name] = []
        elif name and '//' in line:
            body[name] += re.sub(r'<.*>', '', line.split('//')[1].split(':', 1)[1]).split()
    for words in body.values():                      # (the s_nop padding up to the next function's alignment is not the body)
        while words and words[-1] == 'BF800000':
            words.pop()
    return {k: v + [hashlib.sha1(' '.join(body[k]).encode()).hexdigest()[:16]] for k, v in meta.items()}


def tree_table(root):
    spec = importlib.util.spec_from_file_location('drx_build', os.path.join(root, 'drecpy_amd', 'build.py'))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    units, procs = {}, []
    with tempfile.TemporaryDirectory() as tmp:
        for src in (s for s in b.SOURCES if s.endswith('.hip')):
            obj = os.path.join(tmp, src + '.o')
            cmd = [b.HIPCC, f'--offload-arch={b.ARCH}'] + b.COMMON + ['--cuda-device-only', '--no-gpu-bundle-output', '-c',
                                                                       os.path.join(b.CSRC, src), '-o', obj]
            procs.append((src, obj, subprocess.Popen(cmd, stderr=subprocess.DEVNULL)))
        for src, obj, p in procs:
            if p.wait() != 0:
                sys.exit(f'device-only compile failed: {src}')
            units[src] = unit_table(obj)
    kernels = {}
    for t in units.values():
        for k, v in t.items():
            if v not in kernels.setdefault(k, []):
                kernels[k].append(v)
    return {'units': {u: sorted(t) for u, t in units.items()}, 'kernels': {k: sorted(v) for k, v in sorted(kernels.items())}}


def summary(t):
    return ', '.join(f'{u} {len(n)}' for u, n in t['units'].items()) + f" | {len(t['kernels'])} distinct names"


def diff(a, b):
    ka, kb = a['kernels'], b['kernels']
    bad = [f'only in {w}: {k}' for w, x, y in (('first', ka, kb), ('second', kb, ka)) for k in x if k not in y]
    for k in ka.keys() & kb.keys():
        if [v[:5] for v in ka[k]] != [v[:5] for v in kb[k]]:
            bad.append(f'numbers differ: {k}: {ka[k]} vs {kb[k]}')
        elif ka[k] != kb[k]:
            bad.append(f'body differs: {k}')
    print('first:  ' + summary(a) + '\nsecond: ' + summary(b))
    print('\n'.join(sorted(bad)) if bad else f'all equal: {len(ka)} names, registers / LDS / scratch and bodies')
    if bad:
        print(f'{len(ka.keys() & kb.keys())} common names: ' + ', '.join(f'{sum(b.startswith(w) for b in bad)} {w}' for w in ('only in', 'numbers differ', 'body differs')))
    return 1 if bad else 0


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--root', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument('--out')
    ap.add_argument('--diff', nargs=2, metavar=('A.json', 'B.json'))
    args = ap.parse_args()
    if args.diff:
        sys.exit(diff(*(json.load(open(f)) for f in args.diff)))
    table = tree_table(args.root)
    print(summary(table))
    if args.out:
        json.dump(table, open(args.out, 'w'), indent=1)
