#!/usr/bin/env python3
"""Time per RiemannianAdam step on the MI355X:

    python profiles/riemannian/measure.py [--steps 200] [--rounds 5] > profiles/riemannian/rates.txt

Two tables of parameters: 64 Poincare-ball parameters [1024, 16] (4 MB of parameters; a step reads x, g, m, v and writes x, m, v: 20 MB),
and the three-parameter case of the tests ([9, 16] Oblique, [2, 3, 65] ball, [2100, 8] ball: a step of overheads).  For each:
  riemannian      sttode_amd.optim.RiemannianAdam, eager: one launch for the table
  riemannian/g    the same step captured into a HIP graph and replayed (two launches: the device step count, the table)
  adam            sttode_amd.optim.Adam over the SAME tensors as plain parameters: the Euclidean rule, what a one-launch update of that
                  many bytes costs here
  composed        the same Riemannian update from sttode_amd.manifolds op calls and torch elementwise ops, per parameter
Gradients are static.  A figure is the host clock around `steps` steps ending in a device synchronise, per step; the variants alternate
within a round, and the median and the range over the rounds are printed.  Nothing here is a pass condition.
"""
import argparse
import math
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from sttode_amd import manifolds as mf, optim  # noqa: E402

LR, B1, B2, EPS = 1e-3, 0.9, 0.999, 1e-8


def make(table, dev, plain=False):
    gen = torch.Generator(device='cpu').manual_seed(7)
    ps = []
    for man, shape in table:
        x = torch.randn(*shape, generator=gen)
        x = x / x.norm(dim=-1, keepdim=True) * (1.0 if isinstance(man, mf.Oblique) else 0.5 / man.c ** 0.5)
        p = torch.nn.Parameter(x.to(dev)) if plain else mf.ManifoldParameter(x.to(dev), True, man)
        p.grad = torch.randn(*shape, generator=gen).to(dev)
        ps.append(p)
    return ps


class Composed:
    """The update of RiemannianAdam from the public op calls: what a user would write without the fused step."""

    def __init__(self, ps):
        self.ps, self.t = ps, 0
        self.m = [torch.zeros_like(p) for p in ps]
        self.v = [torch.zeros(p.shape[:-1] + (1,), device=p.device) for p in ps]

    @torch.no_grad()
    def step(self):
        self.t += 1
        bc1, bc2 = 1 - B1 ** self.t, 1 - B2 ** self.t
        for p, m, v in zip(self.ps, self.m, self.v):
            man = p.manifold
            r = man.egrad2rgrad(p, p.grad)
            m.mul_(B1).add_(r, alpha=1 - B1)
            rr = man.inner(p, r, keepdim=True) if isinstance(man, mf.PoincareBall) else (r * r).sum(-1, keepdim=True)
            v.mul_(B2).add_(rr, alpha=1 - B2)
            y, mt = man.retr_transp(p, (m / bc1) / ((v / bc2).sqrt() + EPS) * -LR, m)
            p.copy_(y)
            m.copy_(mt)


def timed(step, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--rounds', type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('measure.py needs the GPU: a CPU run gives no time')
    dev = torch.device('cuda:0')
    tables = {'64 x ball [1024, 16]': [(mf.PoincareBall(1.0), (1024, 16))] * 64,
              'three parameters': [(mf.Oblique(), (9, 16)), (mf.PoincareBall(0.5), (2, 3, 65)), (mf.PoincareBall(1.0), (2100, 8))]}
    print('device: %s; %d steps per figure, %d rounds, us per step: median [min .. max]' % (torch.cuda.get_device_name(0), a.steps, a.rounds))
    for name, table in tables.items():
        ra = optim.RiemannianAdam(make(table, dev), lr=LR)
        rg = optim.RiemannianAdam(make(table, dev), lr=LR)
        ad = optim.Adam(make(table, dev, plain=True), lr=LR)
        co = Composed(make(table, dev))
        rg.step()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            rg.step()
        variants = {'riemannian': ra.step, 'riemannian/g': graph.replay, 'adam': ad.step, 'composed': co.step}
        for fn in variants.values():
            for _ in range(10):
                fn()
        res = {k: [] for k in variants}
        for _ in range(a.rounds):
            for k, fn in variants.items():
                res[k].append(timed(fn, a.steps))
        nbytes = sum(4 * 5 * math.prod(s) for _, s in table)
        print('%s (%d parameters, %.2f MB moved per step by x, g, m in and x, m out):' % (name, len(table), nbytes / 1e6))
        for k, v in res.items():
            print('  %-14s %9.1f  [%9.1f .. %9.1f]' % (k, statistics.median(v), min(v), max(v)))
        print('  launches per step: riemannian 1, riemannian/g 2 (in one graph), adam 1, composed about a dozen per parameter')


if __name__ == '__main__':
    main()
