"""The families' own measure scripts on two builds of the library in one job, alternating, for a same-time check.  Needs a GPU.

    python profiles/set_body/rates.py <library built from the parent commit> [--rounds 3] [--dir build/set_body_rates] [--out FILE]

Per round and family: profiles/<family>/measure.py at its default sizes on the parent's library (STTODE_HIP_LIB), then on this tree's, each a
fresh child process under its own time limit; the job stops at the first child that fails.  sample_spread, sampler_objective and
sampler_joint run their `kernel` step (their other steps time evaluation and training loops).  Every median the scripts report for a
device entry (names with `torch` are compositions of torch ops and are left out) is collected per build and round.  Table: the median over
the rounds per build, new / parent, and the parent's own spread (max - min over its rounds, relative to its median): a new median above the
parent's by more than that spread is marked SLOWER.
"""
import argparse
import json
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
FAMILIES = [('sample_spread', ['--step', 'kernel']), ('weighted_set', []), ('large_set', []), ('reduce', []), ('reduce_scenes', []),
            ('sampler_objective', ['--step', 'kernel']), ('sampler_joint', ['--step', 'kernel']), ('multimodal', [])]
LIMIT = 300   # seconds per child


def medians(text):
    """{name: value in us} of one script's output: a JSON document (every leaf `median_us` / `median_ms`, and the `*_ms` / `*_us` leaves
    outside the per-pass lists), or weighted_set's table (the median of its rounds per size and pass)."""
    out = {}
    start = max(text.rfind('\n{'), 0) if not text.lstrip().startswith('{') else 0
    try:
        doc = json.loads(text[start:])
    except ValueError:
        size, rows = '', {}
        for line in text.splitlines():
            m = re.match(r'agents \d+, (K \d+, Tf \d+)', line)
            if m:
                size = m.group(1).replace(', ', ' ').replace(' ', '')
            m = re.match(r'\s+round \d+\s+(\w+)\s+([\d.]+) ', line)
            if m:
                rows.setdefault(f'{size}.{m.group(1)}', []).append(float(m.group(2)))
        return {k: float(np.median(v)) for k, v in rows.items()}

    def walk(d, path):
        for k, v in d.items():
            if isinstance(v, dict):
                walk(v, path + [k])
            elif isinstance(v, (int, float)) and not isinstance(v, bool):
                if k.startswith(('min_', 'max_')) or not k.endswith(('_ms', '_us')):
                    continue
                name = '.'.join(path + ([] if k in ('median_us', 'median_ms') else [k[:-3]]))
                out[name] = float(v) * (1e3 if k.endswith('_ms') else 1.0)
    walk(doc, [])
    return {k: v for k, v in out.items() if 'torch' not in k}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('parent_lib')
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--dir', default=os.path.join(ROOT, 'build', 'set_body_rates'))
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.abspath(__file__)), 'rates.txt'))
    a = ap.parse_args()
    os.makedirs(a.dir, exist_ok=True)
    got = {}   # (family, name) -> {'parent': [...], 'new': [...]}
    for rnd in range(a.rounds):
        for fam, extra in FAMILIES:
            for build in ('parent', 'new'):
                env = dict(os.environ)
                env.pop('STTODE_HIP_LIB', None)
                if build == 'parent':
                    env['STTODE_HIP_LIB'] = os.path.abspath(a.parent_lib)
                tag = os.path.join(a.dir, f'{fam}_{build}_{rnd}')
                if os.path.exists(tag + '.out'):
                    os.remove(tag + '.out')
                cmd = [sys.executable, os.path.join(ROOT, 'profiles', fam, 'measure.py'), *extra, '--out', tag + '.out']
                try:
                    p = subprocess.run(cmd, env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=LIMIT)
                except subprocess.TimeoutExpired:
                    sys.exit(f'{fam} ({build}, round {rnd}): no result within {LIMIT} s; stopping')
                with open(tag + '.log', 'w') as f:
                    f.write(p.stdout + p.stderr)
                if p.returncode != 0:
                    sys.exit(f'{fam} ({build}, round {rnd}): exit status {p.returncode}; stopping ({tag}.log)')
                text = open(tag + '.out').read() if os.path.exists(tag + '.out') else p.stdout
                for name, v in medians(text).items():
                    got.setdefault((fam, name), {'parent': [], 'new': []})[build].append(v)
                print(f'round {rnd} {fam} {build}: ok', flush=True)
    lines = [f'{a.rounds} rounds per build, alternating (parent first), one child process per script and round; us per call / launch as the',
             'scripts report them; spread = (max - min) / median of the parent\'s rounds',
             f'{"family.entry":58s} {"parent":>10s} {"new":>10s} {"new/parent":>10s} {"spread":>8s}']
    slower = 0
    for (fam, name), v in got.items():
        p, q = float(np.median(v['parent'])), float(np.median(v['new']))
        spread = (max(v['parent']) - min(v['parent'])) / p
        mark = ''
        if q > p * (1.0 + spread):
            mark, slower = '  SLOWER', slower + 1
        lines.append(f'{fam + "." + name:58s} {p:10.2f} {q:10.2f} {q / p:10.4f} {100 * spread:7.2f}%{mark}')
        lines.append(f'{"":58s} parent {" ".join("%.2f" % x for x in v["parent"])} | new {" ".join("%.2f" % x for x in v["new"])}')
    lines.append(f'entries marked SLOWER: {slower} of {len(got)}')
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    print('\n'.join(lines))


if __name__ == '__main__':
    main()
