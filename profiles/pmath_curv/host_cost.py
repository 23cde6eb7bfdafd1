#!/usr/bin/env python3
"""Host cost of pmath's autograd paths: Python-level forward plus backward of mobius_add and dist, with a float c and with
a tensor c that requires grad, at 8192 x 64 (kernel-bound) and 64 x 16 (launch-bound).

    python profiles/pmath_curv/host_cost.py run --tree TREE --out RUN.json      one process: TREE's sttode_amd, microseconds per call
    python profiles/pmath_curv/host_cost.py report --parent P*.json --child C*.json [--out rates.txt]

`run` is started once per tree and round by the caller, parent and child alternating (A B A B ...), each process under its own time
limit.  A call is fn(x, y, c=c).sum().backward(); a run times CALLS calls back to back between two device synchronisations with the host
clock, REPEATS times after every case has been warmed up, and keeps the fastest (the box is shared: other work on its host can only add
time to a window).  `report` gives, per case and side, the median over the runs and their spread
(max - min) / median; the child's median has to lie within the parent's own spread of the parent's median."""
import argparse
import json
import os
import statistics
import sys
import time

SHAPES, WARMUP, CALLS, REPEATS = ((8192, 64), (64, 16)), 30, 200, 7


def run(tree, out):
    tree = os.path.abspath(tree)
    sys.path.insert(0, tree)
    import torch
    import sttode_amd
    from sttode_amd import pmath
    assert os.path.abspath(sttode_amd.__file__).startswith(tree + os.sep), sttode_amd.__file__
    dev = torch.device('cuda:0')
    gen = torch.Generator().manual_seed(3)
    cases = {}
    for rows, d in SHAPES:
        pts = lambda: (torch.nn.functional.normalize(torch.randn(rows, d, generator=gen), dim=-1) * (0.05 + 0.8 * torch.rand(rows, 1, generator=gen))).to(dev)
        x, y = pts().requires_grad_(True), pts().requires_grad_(True)
        for fname in ('mobius_add', 'dist'):
            fn = getattr(pmath, fname)
            for cname, c in (('float c', 1.0), ('tensor c', torch.ones(1, device=dev, requires_grad=True))):
                def call(fn=fn, x=x, y=y, c=c):
                    x.grad = y.grad = None
                    fn(x, y, c=c).sum().backward()
                cases['%s %d x %d, %s' % (fname, rows, d, cname)] = call
    for call in cases.values():
        for _ in range(WARMUP):
            call()
    res = {}
    for name, call in cases.items():
        ts = []
        for _ in range(REPEATS):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(CALLS):
                call()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e6 / CALLS)
        res[name] = min(ts)
    with open(out, 'w') as f:
        json.dump(dict(tree=tree, device=torch.cuda.get_device_name(0), us_per_call=res), f)
    print(out, ' '.join('%.1f' % v for v in res.values()))


def report(parent, child, out):
    sides = {'parent': [json.load(open(p)) for p in parent], 'child': [json.load(open(p)) for p in child]}
    lines = ['forward + backward through autograd, microseconds per call (host clock around %d calls, fastest of %d repeats per process);' % (CALLS, REPEATS),
             'per side the median over %d processes (parent and child alternating) and the spread (max - min) / median' % len(parent),
             'device: ' + sides['parent'][0]['device'], '']
    ok = True
    for case in sides['parent'][0]['us_per_call']:
        med, spread = {}, {}
        for side, runs in sides.items():
            v = [r['us_per_call'][case] for r in runs]
            med[side], spread[side] = statistics.median(v), (max(v) - min(v)) / statistics.median(v)
        ratio = med['child'] / med['parent']
        within = abs(ratio - 1.0) <= spread['parent']
        ok &= within or ratio < 1.0
        lines.append('%-34s parent %8.1f us (spread %4.1f%%)   child %8.1f us (spread %4.1f%%)   child / parent %.3f  %s'
                     % (case, med['parent'], 100 * spread['parent'], med['child'], 100 * spread['child'], ratio,
                        'within the parent\'s spread' if within else ('FASTER than the parent\'s spread' if ratio < 1.0 else 'SLOWER than the parent\'s spread')))
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    with open(out, 'w') as f:
        f.write(text)
    return 0 if ok else 1


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest='cmd', required=True)
    r = sub.add_parser('run')
    r.add_argument('--tree', required=True)
    r.add_argument('--out', required=True)
    p = sub.add_parser('report')
    p.add_argument('--parent', nargs='+', required=True)
    p.add_argument('--child', nargs='+', required=True)
    p.add_argument('--out', default=os.path.join(os.path.dirname(os.path.abspath(__file__)), 'rates.txt'))
    a = ap.parse_args()
    sys.exit(run(a.tree, a.out) if a.cmd == 'run' else report(a.parent, a.child, a.out))
