#!/usr/bin/env python3
"""Forward + backward times of the opt-in gradients on the MI355X:

    python profiles/manifold_grad/measure.py [--iters 200] [--rounds 5] > profiles/manifold_grad/rates.txt    (writes resource_usage.txt too)

For each case two variants alternate within a round:
  hip        the public function with its HIP backward (sttode_amd.pmath / sttode_amd.manifolds, differentiable)
  torch      the same operation composed from torch ops with torch autograd, float32, on the same device: tests/riemannian_ref.py's
             functions and the few-line poincare_mean of tests/manifold_grad_cases.py
Cases: poincare_mean at [5, 64, 64] and [20, 512, 128] over dim 0; the manifold row ops at [8192, 64] on both manifolds; oblique_dist at
[1, 512, 512, 64].  A figure is the host clock around `iters` forward + backward passes ending in a device synchronise, per pass; the
median and the range over the rounds are printed.  The launches of one backward pass are counted once from capi.call.  For the row
kernels the bytes a backward pass must move (operands and upstream gradients in, gradients out, once each) over the time of the backward
launches alone (device events around `iters` launches of the entry point) is set against the device's copy rate, measured the same way
in the same run with a 256 MB torch copy; the shader clock is read on both sides.  Nothing here is a pass condition.
"""
import argparse
import os
import statistics
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import manifold_grad_cases as mc  # noqa: E402
import riemannian_ref as rr  # noqa: E402
from sttode_amd import capi, manifolds as mf, pmath  # noqa: E402


def sclk():
    """The shader clock as rocm-smi reports it (a read, no setting is touched); '?' where the tool is missing."""
    try:
        out = subprocess.run(['rocm-smi', '--showclocks', '-d', '0'], capture_output=True, text=True, timeout=20).stdout
        return next((ln.split(':')[-1].strip() for ln in out.splitlines() if 'sclk' in ln), '?')
    except Exception:
        return '?'


def timed(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e6


def event_us(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def count_launch_calls(fn):
    """The entry points one forward + backward pass calls, in order."""
    names, orig = [], capi.call

    def spy(name, *a, **k):
        names.append(name)
        return orig(name, *a, **k)
    capi.call = pmath.capi.call = spy
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        capi.call = orig
    return names


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', default=os.path.dirname(os.path.abspath(__file__)), help='where resource_usage.txt goes')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('measure.py needs the GPU: a CPU run gives no time')
    dev = torch.device('cuda:0')
    gen = torch.Generator(device='cpu').manual_seed(11)

    def ball(shape, c, r=0.7):
        v = torch.randn(*shape, generator=gen)
        return (v / v.norm(dim=-1, keepdim=True) * r * torch.rand(*shape[:-1], 1, generator=gen) / c ** 0.5).to(dev)

    def unit(shape):
        v = torch.randn(*shape, generator=gen)
        return (v / v.norm(dim=-1, keepdim=True)).to(dev)

    cases = {}
    for shape in ((5, 64, 64), (20, 512, 128)):
        x, g = ball(shape, 1.0).requires_grad_(), torch.randn(*shape[1:], generator=gen).to(dev)

        def hip(x=x, g=g):
            torch.autograd.grad(pmath.poincare_mean(x, dim=0, c=1.0, differentiable=True), [x], g)

        def ref(x=x, g=g):
            torch.autograd.grad(mc.pmean(x, 0, 1.0), [x], g)
        cases['poincare_mean %s' % (shape,)] = (hip, ref, None)
    rows, d = 8192, 64
    def manifold_cases(mname, c):      # (a function: the closures below bind this call's tensors)
        man = mf.differentiable(mf.Oblique() if mname == 'oblique' else mf.PoincareBall(c))
        refman = rr.ObliqueRef() if mname == 'oblique' else rr.BallRef(c)
        if mname == 'oblique':
            p, y = unit((rows, d)), unit((rows, d))
            u, w = [t - (t * p).sum(-1, keepdim=True) * p for t in (0.5 * unit((rows, d)), 0.5 * unit((rows, d)))]
        else:
            p, y, u, w = ball((rows, d), c), ball((rows, d), c), ball((rows, d), c, 0.2), ball((rows, d), c, 0.2)
        p, y, u, w = [t.contiguous().requires_grad_() for t in (p, y, u, w)]
        g, g2 = torch.randn(rows, d, generator=gen).to(dev), torch.randn(rows, d, generator=gen).to(dev)
        ops = {'egrad2rgrad': (lambda m: (m.egrad2rgrad(p, u),), [p, u], 5), 'expmap': (lambda m: (m.expmap(u, p),), [p, u], 5),
               'ptransp': (lambda m: (m.ptransp(p, y, w),), [p, y, w], 7), 'retr': (lambda m: (m.retr(p, u),), [p, u], 5),
               'retr_transp': (lambda m: m.retr_transp(p, u, w), [p, u, w], 8)}
        for op, (call, operands, arrays) in ops.items():
            if mname == 'poincare' and op == 'expmap':
                continue        # the ball's expmap is pmath.expmap's own backward

            def hip(call=call, operands=operands, man=man):
                outs = call(man)
                torch.autograd.grad(list(outs), operands, [g, g2][:len(outs)], allow_unused=True)

            def ref(call=call, operands=operands, refman=refman):
                outs = call(refman)
                torch.autograd.grad(list(outs), operands, [g, g2][:len(outs)], allow_unused=True)
            code = capi.MANIFOLD_OPS['proj_tan' if op == 'egrad2rgrad' else op]
            three = op in ('ptransp', 'retr_transp')
            buf = [torch.empty_like(p) for _ in range(3)]
            args = (code, capi.MANIFOLDS[mname], p.detach(), (y if op == 'ptransp' else u).detach(), w.detach() if three else None, g,
                    g2 if op == 'retr_transp' else None, buf[0], buf[1], buf[2] if three else None, rows, d, c)
            cases['%s %s [%d, %d]' % (mname, op, rows, d)] = (hip, ref, (args, arrays * rows * d * 4))
    for mname, c in (('oblique', 1.0), ('poincare', 1.0)):
        manifold_cases(mname, c)
    p1, p2 = unit((1, 512, 64)).requires_grad_(), unit((1, 512, 64)).requires_grad_()
    gd = torch.randn(1, 512, 512, generator=gen).to(dev)
    cases['oblique_dist [1, 512, 512, 64]'] = (
        lambda: torch.autograd.grad(pmath.oblique_dist(p1, p2, differentiable=True), [p1, p2], gd),
        lambda: torch.autograd.grad(torch.acos((p2 @ p1.transpose(-1, -2)).clamp(-1 + 1e-4, 1 - 1e-4)), [p1, p2], gd), None)

    print('device: %s; %d passes per figure, %d rounds; us per forward + backward pass: median [min .. max]' %
          (torch.cuda.get_device_name(0), a.iters, a.rounds))
    src, dst = torch.empty(64 << 20, device=dev), torch.empty(64 << 20, device=dev)
    for _ in range(5):
        dst.copy_(src)
    clk0 = sclk()
    copy_us = statistics.median(event_us(lambda: dst.copy_(src), 50) for _ in range(a.rounds))
    copy_rate = 2 * src.numel() * 4 / copy_us / 1e3          # GB/s, read + write
    print('device copy of 256 MB (torch, read + write): %.1f us, %.0f GB/s; sclk before: %s' % (copy_us, copy_rate, clk0))
    resource = []
    for name, (hip, ref, kern) in cases.items():
        for fn in (hip, ref):
            for _ in range(10):
                fn()
        res = {'hip': [], 'torch': []}
        for _ in range(a.rounds):
            res['hip'].append(timed(hip, a.iters))
            res['torch'].append(timed(ref, a.iters))
        calls = count_launch_calls(hip)
        print('%s' % name)
        for k, v in res.items():
            print('  %-6s %9.1f  [%9.1f .. %9.1f]' % (k, statistics.median(v), min(v), max(v)))
        print('  entry points of one pass: %s' % ', '.join(calls))
        if kern is not None:
            args, nbytes = kern
            st = capi.stream_ptr()
            us = statistics.median(event_us(lambda: capi.call('sttode_manifold_rowop_bwd', *args, st), a.iters) for _ in range(a.rounds))
            rate = nbytes / us / 1e3
            resource.append('%-34s backward launch %7.1f us, %6.1f MB moved, %6.0f GB/s = %.2f of the copy rate' %
                            (name, us, nbytes / 1e6, rate, rate / copy_rate))
    print('sclk after: %s' % sclk())
    with open(os.path.join(a.out, 'resource_usage.txt'), 'w') as f:
        f.write('achieved bytes/s of the one-launch manifold backward kernels against the device copy rate of the same run\n')
        f.write('device copy (256 MB, read + write): %.0f GB/s; sclk before %s, after %s\n' % (copy_rate, clk0, sclk()))
        f.write('\n'.join(resource) + '\n')
    print('\n'.join(resource))


if __name__ == '__main__':
    main()
