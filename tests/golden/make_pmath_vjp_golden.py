#!/usr/bin/env python3
"""Generate tests/golden/pmath_vjp_rows.npz and pmath_vjp.npz (vector-Jacobian products of the Poincare-ball operations) by IMPORTING
THE REFERENCE's hyptorch/pmath.py and hyptorch/nn.py and differentiating them with torch autograd on the CPU:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_pmath_vjp_golden.py

Data only.  Inputs and upstream gradients are float32.  For every case two sets of reference gradients are stored: `*64`, the reference
run in FLOAT64 on the float32 inputs (the yardstick), and `*32`, the reference's own float32 run.  Both are stored as float32 -- rounding
the yardstick costs 6e-8 relative, three orders below the bound the tests hold the kernels to, and halves the file.

pmath_vjp_rows.npz -- the 12 row ops over the whole product d in {1, 2, 16, 65, 130} x n in {1, 9} x c in {1.0, 0.5}; three arrays per shape
<sh> = d<d>.n<n>.c<c>:
  in.<sh>      [4,n,d]   x, y (points), u (tangent), g (upstream gradient of vector results): random directions, sqrt(c) |.| uniform in
                         [0.05, 0.9]; g ~ N(0,1)
  gs.<sh>      [n]       upstream gradient of scalar results
  grads.<sh>   [32,n,d]  for op in ROW_OPS, for each operand of the op: the float64 gradient, then the fp32 one (k2p on x / 2; expmap on
                         (x, u); scalar results take gs)
pmath_vjp.npz -- everything else (the curvature of a case is in its name or in the list below):
  clip.project.c<c>.{x,g,gx64,gx32}   project with rows at sqrt(c) |x| = 1.2 (the clipped branch), n 9, d 16
  zero.<op>.{x,(y,)g,gx..,(gy..)}     one all-zero row (row 4 of 9, d 16, c 1.0): expmap0, logmap0 (x) and expmap (u = 0).  On logmap0's zero
                                      row the reference's OWN fp32 gradient is 5e-4 relative off (its fp32 artanh(1e-5), a difference of
                                      two logs of 1 +- 1e-5 rounded to fp32); the float64 yardstick is exact there
  bcast.mobius_add.{x[9,16],y[16],g,..}   bcast.dist.{x[2,3,16],y[3,16],g[2,3],..}      broadcast operands, c 1.0
  mv.<tag>.{m,x,g,gm..,gx..}          mobius_matvec, m ~ 0.3 N(0,1), c 1.0 but d5O33 at c 0.5: d16O16, d5O33, d64O7 (9 rows), big (2100 rows, d = O = 8), and zero
                                      (d16O16 with x row `mv.zero.row` all zero: the reference is run WITHOUT that row -- it gives NaN
                                      there, and through the sum over rows in gm -- and the stored gx row is zero)
  dm.P<P>R<R>d<d>.{x,y,g,gx..,gy..}   dist_matrix, (P, R, d) in {(1,1,2), (5,9,16), (67,3,65)} and (3,2,300) (rows longer than the 256
                                      elements a wave keeps in registers), c 1.0
  comp.topoincare.{x,g,gx..}          hyptorch.nn.ToPoincare(c 1.0, riemannian=True) on Euclidean x [9,16]
  comp.hyplinear.{w,b,x,g,gw..,gb..,gx..}   hyptorch.nn.HypLinear(16, 8, c 0.5) with bias; weights drawn here, not by the module's init
  comp.distlayer.{x,y,g,gx..,gy..}    hyptorch.nn.HyperbolicDistanceLayer(c 1.0): dist(keepdim=True), g [9,1]
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get('STTODE_REFERENCE', '/root/reference')

ROW_OPS = ('project', 'lambda_x', 'mobius_add', 'dist', 'dist0', 'expmap', 'expmap0', 'logmap', 'logmap0', 'p2k', 'k2p', 'lorenz')
SCALAR_OPS = ('lambda_x', 'dist', 'dist0', 'lorenz')
TWO_OPS = ('mobius_add', 'dist', 'expmap', 'logmap')
ROW_SHAPES = [(d, n, c) for d in (1, 2, 16, 65, 130) for n in (1, 9) for c in (1.0, 0.5)]


def reference():
    if REF not in sys.path:
        sys.path.insert(0, REF)
    import hyptorch.nn as hnn
    import hyptorch.pmath as pm
    return pm, hnn


def ball_points(rng, shape, c, lo=0.05, hi=0.9):
    v = rng.standard_normal(shape)
    v = v / np.linalg.norm(v, axis=-1, keepdims=True) * rng.uniform(lo, hi, shape[:-1] + (1,)) / np.sqrt(c)
    return v.astype(np.float32)


def row_fn(pm, op, c):
    if op == 'lorenz':
        return lambda x: pm.lorenz_factor(x, c=c)
    if op in ('p2k', 'k2p'):
        return lambda x: getattr(pm, op)(x, c)
    return lambda *a: getattr(pm, op)(*a, c=c)


def vjp(fn, inputs, g, dtype):
    """Gradients of sum(fn(*inputs) * g) with respect to every input, the computation in `dtype`."""
    import torch
    ts = [torch.from_numpy(np.asarray(a)).to(dtype).requires_grad_() for a in inputs]
    out = fn(*ts)
    out.backward(torch.from_numpy(np.asarray(g)).to(dtype).reshape(out.shape))
    return [t.grad.numpy().astype(np.float32) for t in ts]


def store(out, case, names, fn, inputs, g, c):
    import torch
    for tag, dt in (('64', torch.float64), ('32', torch.float32)):
        for n, v in zip(names, vjp(fn, inputs, g, dt)):
            out['%s.%s%s' % (case, n, tag)] = v


def main():
    pm, hnn = reference()
    import torch
    out = {}
    rng = np.random.default_rng(20261018)
    rows = {}
    for d, n, c in ROW_SHAPES:
        sh = 'd%d.n%d.c%s' % (d, n, c)
        x, y, u = (ball_points(rng, (n, d), c) for _ in range(3))
        g, gs = rng.standard_normal((n, d)).astype(np.float32), rng.standard_normal(n).astype(np.float32)
        rows['in.' + sh], rows['gs.' + sh] = np.stack([x, y, u, g]), gs
        grads = []
        for op in ROW_OPS:
            ins = [x * np.float32(0.5)] if op == 'k2p' else [x]
            if op in TWO_OPS:
                ins.append(u if op == 'expmap' else y)
            g64, g32 = (vjp(row_fn(pm, op, c), ins, gs if op in SCALAR_OPS else g, dt) for dt in (torch.float64, torch.float32))
            for a64, a32 in zip(g64, g32):
                grads += [a64, a32]
        rows['grads.' + sh] = np.stack(grads)
    # branch rows
    rng = np.random.default_rng(20261019)
    for c in (1.0, 0.5):
        x = ball_points(rng, (9, 16), c, 1.2, 1.2)
        g = rng.standard_normal((9, 16)).astype(np.float32)
        out.update({'clip.project.c%s.x' % c: x, 'clip.project.c%s.g' % c: g})
        store(out, 'clip.project.c%s' % c, ('gx',), row_fn(pm, 'project', c), [x], g, c)
    for op in ('expmap0', 'logmap0', 'expmap'):
        x, u = ball_points(rng, (9, 16), 1.0), ball_points(rng, (9, 16), 1.0)
        g = rng.standard_normal((9, 16)).astype(np.float32)
        if op == 'expmap':
            u[4] = 0
            ins, names = [x, u], ('x', 'y')
        else:
            x[4] = 0
            ins, names = [x], ('x',)
        out.update({'zero.%s.%s' % (op, k): v for k, v in zip(names, ins)})
        out['zero.%s.g' % op] = g
        store(out, 'zero.%s' % op, ('gx', 'gy'), row_fn(pm, op, 1.0), ins, g, 1.0)
    # broadcast
    x, y, g = ball_points(rng, (9, 16), 1.0), ball_points(rng, (16,), 1.0), rng.standard_normal((9, 16)).astype(np.float32)
    out.update({'bcast.mobius_add.x': x, 'bcast.mobius_add.y': y, 'bcast.mobius_add.g': g})
    store(out, 'bcast.mobius_add', ('gx', 'gy'), row_fn(pm, 'mobius_add', 1.0), [x, y], g, 1.0)
    x, y, g = ball_points(rng, (2, 3, 16), 1.0), ball_points(rng, (3, 16), 1.0), rng.standard_normal((2, 3)).astype(np.float32)
    out.update({'bcast.dist.x': x, 'bcast.dist.y': y, 'bcast.dist.g': g})
    store(out, 'bcast.dist', ('gx', 'gy'), row_fn(pm, 'dist', 1.0), [x, y], g, 1.0)
    # mobius_matvec
    rng = np.random.default_rng(20261020)
    for tag, d, O, n, c in (('d16O16', 16, 16, 9, 1.0), ('d5O33', 5, 33, 9, 0.5), ('d64O7', 64, 7, 9, 1.0), ('big', 8, 8, 2100, 1.0),
                            ('zero', 16, 16, 9, 1.0)):
        m = (0.3 * rng.standard_normal((O, d))).astype(np.float32)
        x, g = ball_points(rng, (n, d), c), rng.standard_normal((n, O)).astype(np.float32)
        case = 'mv.' + tag
        fn = lambda mm, xx, c=c: pm.mobius_matvec(mm, xx, c=c)
        if tag == 'zero':
            keep = np.arange(n) != 4
            x[4] = 0
            out[case + '.row'] = np.int64(4)
            for t, dt in (('64', torch.float64), ('32', torch.float32)):
                gm, gx = vjp(fn, [m, x[keep]], g[keep], dt)
                full = np.zeros_like(x)
                full[keep] = gx
                out[case + '.gm' + t], out[case + '.gx' + t] = gm, full
        else:
            store(out, case, ('gm', 'gx'), fn, [m, x], g, c)
        out.update({case + '.m': m, case + '.x': x, case + '.g': g})
    # dist_matrix
    for P, R, d in ((1, 1, 2), (5, 9, 16), (67, 3, 65), (3, 2, 300)):
        case = 'dm.P%dR%dd%d' % (P, R, d)
        x, y, g = ball_points(rng, (P, d), 1.0), ball_points(rng, (R, d), 1.0), rng.standard_normal((P, R)).astype(np.float32)
        out.update({case + '.x': x, case + '.y': y, case + '.g': g})
        store(out, case, ('gx', 'gy'), lambda a, b: pm.dist_matrix(a, b, c=1.0), [x, y], g, 1.0)
    # compositions: the reference's own modules
    rng = np.random.default_rng(20261021)
    x, g = (0.6 * rng.standard_normal((9, 16)) / 4.0).astype(np.float32), rng.standard_normal((9, 16)).astype(np.float32)
    out.update({'comp.topoincare.x': x, 'comp.topoincare.g': g})
    store(out, 'comp.topoincare', ('gx',), hnn.ToPoincare(c=1.0, riemannian=True), [x], g, 1.0)
    w = rng.uniform(-0.25, 0.25, (8, 16)).astype(np.float32)
    b = rng.uniform(-0.25, 0.25, 8).astype(np.float32)
    x, g = ball_points(rng, (9, 16), 0.5), rng.standard_normal((9, 8)).astype(np.float32)

    def hyplinear(ww, bb, xx):
        lin = hnn.HypLinear(16, 8, c=0.5)
        del lin.weight, lin.bias
        lin.weight, lin.bias = ww, bb          # plain tensors of the run's dtype in place of the parameters
        return lin(xx)
    out.update({'comp.hyplinear.w': w, 'comp.hyplinear.b': b, 'comp.hyplinear.x': x, 'comp.hyplinear.g': g})
    store(out, 'comp.hyplinear', ('gw', 'gb', 'gx'), hyplinear, [w, b, x], g, 0.5)
    x, y, g = ball_points(rng, (9, 16), 1.0), ball_points(rng, (9, 16), 1.0), rng.standard_normal((9, 1)).astype(np.float32)
    out.update({'comp.distlayer.x': x, 'comp.distlayer.y': y, 'comp.distlayer.g': g})
    store(out, 'comp.distlayer', ('gx', 'gy'), hnn.HyperbolicDistanceLayer(c=1.0), [x, y], g, 1.0)
    path = os.path.join(HERE, 'pmath_vjp.npz')
    np.savez_compressed(path, **out)
    np.savez_compressed(os.path.join(HERE, 'pmath_vjp_rows.npz'), **rows)
    print('wrote pmath_vjp_rows.npz', os.path.getsize(os.path.join(HERE, 'pmath_vjp_rows.npz')), 'bytes,', len(rows), 'arrays')
    worst = 0.0
    for k in out:
        if k.endswith('64') and k[:-2] + '32' in out:
            worst = max(worst, float(np.max(np.abs(out[k[:-2] + '32'].astype(np.float64) - out[k]) / (1 + np.abs(out[k])))))
    print('wrote', path, os.path.getsize(path), 'bytes,', len(out), 'arrays; worst reference fp32 error %.2e' % worst)


if __name__ == '__main__':
    main()
