#!/usr/bin/env python3
"""Generate tests/golden/pmath_cgrad.npz: the gradient of the curvature c through the Poincare-ball operations and the hyperbolic layers,
by IMPORTING THE REFERENCE's hyptorch/pmath.py and hyptorch/nn.py and differentiating them with torch autograd on the CPU:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_pmath_cgrad_golden.py

Data only.  The yardstick is the reference run in FLOAT64 on the float32 inputs with c a float64 leaf holding the float32 value of the
curvature; the reference's own float32 run (c a float32 leaf) is stored beside it.  Every `gc` array is float64 [2]: (gc64, gc32).  The
script asserts that every stored case has gc32 within 1e-4 of gc64 on |a - b| / (1 + |b|), the bound the kernels are held to: a case
that fails is given other inputs (another seed), never another bound.

  row.gc                  [2,12,20]  the 12 row ops over the 20 shapes of pmath_vjp_rows.npz, whose in.* / gs.* arrays are the inputs
  <case>.gc               the clip.*, zero.*, bcast.*, mv.* and dm.* cases of pmath_vjp.npz (inputs there; mv.zero without its zero row,
                          as there: the reference gives NaN on it, the kernels a zero gradient)
  edge.in [3,1030,5], edge.gs [1030], edge.<op>.n<rows>.gc
                          mobius_add and dist at c = 2.0 on the first rows in {255, 256, 257, 1030} rows of x, y, g = edge.in
  pair.B<B>C<C>d<d>.{X,A,P,g,g3}, hs.<sh>.gc, mab.<sh>.gc
                          _hyperbolic_softmax(X, A, P, c) with upstream g [B,C] and _mobius_addition_batch(X, P, c) with g3 [B,C,d],
                          c = 0.7, (B, C, d) in {(1,1,2), (9,7,16), (67,3,65)}
  mod.<tag>.{x,g,<param>,g<name>}   the reference's modules at c = 0.7, every parameter gradient and the input gradient as [2,...]
                          (float64, float32): to = ToPoincare(0.7, train_c=True); to_xp_clip = ToPoincare(0.7, train_c=True, train_x=True,
                          ball_dim=16, clip_r=2.3) with xp = mod.to_xp_clip.xp; from = FromPoincare(0.7, train_c=True); from_xp = the same with
                          train_x; net = ToPoincare(c) -> HypLinear(16, 8)(., c=c) -> HyperbolicMLR(8, 5)(., c=c), one leaf c shared by the
                          three (w, b = HypLinear's weight and bias, a, p = a_vals, p_vals)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from make_pmath_vjp_golden import ball_points, reference, row_fn  # noqa: E402
from pmath_cgrad_cases import (BOUND, CLIP_R, EDGE_C, EDGE_D, EDGE_OPS, EDGE_ROWS, MODULE_C, PAIR_C, PAIR_SHAPES, ROW_OPS, ROW_SHAPES,  # noqa: E402
                               SCALAR_OPS, err, vjp_cases)


def c_grad(fn, inputs, g, c, dtype):
    """d sum(fn(*inputs, c) * g) / dc, the computation in `dtype`."""
    import torch
    ts = [torch.from_numpy(np.ascontiguousarray(a)).to(dtype) for a in inputs]
    ct = torch.tensor(float(np.float32(c)), dtype=dtype, requires_grad=True)
    out = fn(*ts, ct)
    out.backward(torch.from_numpy(np.ascontiguousarray(g)).to(dtype).reshape(out.shape))
    return float(ct.grad)


def both(fn, inputs, g, c, what):
    import torch
    gc = np.array([c_grad(fn, inputs, g, c, torch.float64), c_grad(fn, inputs, g, c, torch.float32)])
    assert np.isfinite(gc).all(), what
    e = err(gc[1], gc[0])
    assert e <= BOUND, '%s: the reference fp32 c gradient is %.2e off its float64 one: draw other inputs' % (what, e)
    return gc, e


def op_fn(pm, op):
    if op == 'mobius_matvec':
        return lambda m, x, c: pm.mobius_matvec(m, x, c=c)
    if op == 'dist_matrix':
        return lambda x, y, c: pm.dist_matrix(x, y, c=c)
    if op == '_hyperbolic_softmax':
        return lambda X, A, P, c: pm._hyperbolic_softmax(X, A, P, c)
    if op == '_mobius_addition_batch':
        return lambda x, y, c: pm._mobius_addition_batch(x, y, c)
    return lambda *a: row_fn(pm, op, a[-1])(*a[:-1])


def module_grads(build, params, x, g, dtype):
    """build(dtype) -> (module, the leaf c if it is not one of the module's parameters, how to run it).  Returns the gradients of
    every parameter in `params`, of c and of the input, and the output's shape."""
    import torch
    mod, c_leaf, run = build(dtype)
    with torch.no_grad():
        for name, v in params.items():
            dict(mod.named_parameters())[name].copy_(torch.from_numpy(v).to(dtype))
    xt = torch.from_numpy(x).to(dtype).requires_grad_()
    out = run(mod, xt)
    out.backward(torch.from_numpy(g).to(dtype).reshape(out.shape))
    named = dict(mod.named_parameters())
    gc = c_leaf.grad if c_leaf is not None else named['c'].grad
    return {**{k: named[k].grad.numpy().astype(np.float64) for k in params}, 'c': gc.numpy().astype(np.float64).reshape(1),
            'x': xt.grad.numpy().astype(np.float64)}, tuple(out.shape)


def main():
    pm, hnn = reference()
    import torch
    import torch.nn as nn
    z = np.load(os.path.join(HERE, 'pmath_vjp.npz'))
    zr = np.load(os.path.join(HERE, 'pmath_vjp_rows.npz'))
    out, worst = {}, {}

    def note(op, e):
        worst[op] = max(worst.get(op, 0.0), e)
    rows = np.zeros((2, len(ROW_OPS), len(ROW_SHAPES)))
    for case in vjp_cases(z, zr):
        ins, g = case['inputs'], case['g']
        if case['zero_row'] is not None:                    # mv.zero: the reference without the zero row
            keep = np.arange(len(ins[1])) != case['zero_row']
            ins, g = [ins[0], ins[1][keep]], g[keep]
        gc, e = both(op_fn(pm, case['op']), ins, g, case['c'], case['name'])
        note(case['op'], e)
        if case['name'].startswith('row.'):
            sh = [s for s in ROW_SHAPES if case['name'] == 'row.%s.d%d.n%d.c%s' % ((case['op'],) + s)][0]
            rows[:, ROW_OPS.index(case['op']), ROW_SHAPES.index(sh)] = gc
        else:
            out[case['name'] + '.gc'] = gc
    out['row.gc'] = rows
    # row counts around the finishing kernel's 256 threads
    rng = np.random.default_rng(20261101)
    n = max(EDGE_ROWS)
    x, y = ball_points(rng, (n, EDGE_D), EDGE_C), ball_points(rng, (n, EDGE_D), EDGE_C)
    g, gs = rng.standard_normal((n, EDGE_D)).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    out['edge.in'], out['edge.gs'] = np.stack([x, y, g]), gs
    for k in EDGE_ROWS:
        for op in EDGE_OPS:
            name = 'edge.%s.n%d' % (op, k)
            out[name + '.gc'], e = both(op_fn(pm, op), [x[:k], y[:k]], gs[:k] if op in SCALAR_OPS else g[:k], EDGE_C, name)
            note(op, e)
    # the pair functions
    rng = np.random.default_rng(20261102)
    for B, C, d in PAIR_SHAPES:
        sh = 'B%dC%dd%d' % (B, C, d)
        X, P = ball_points(rng, (B, d), PAIR_C), ball_points(rng, (C, d), PAIR_C)
        A = (0.5 * rng.standard_normal((C, d))).astype(np.float32)
        g, g3 = rng.standard_normal((B, C)).astype(np.float32), rng.standard_normal((B, C, d)).astype(np.float32)
        out.update({'pair.%s.X' % sh: X, 'pair.%s.A' % sh: A, 'pair.%s.P' % sh: P, 'pair.%s.g' % sh: g, 'pair.%s.g3' % sh: g3})
        out['hs.%s.gc' % sh], e = both(op_fn(pm, '_hyperbolic_softmax'), [X, A, P], g, PAIR_C, 'hs.' + sh)
        note('_hyperbolic_softmax', e)
        out['mab.%s.gc' % sh], e = both(op_fn(pm, '_mobius_addition_batch'), [X, P], g3, PAIR_C, 'mab.' + sh)
        note('_mobius_addition_batch', e)
    # the reference's modules
    rng = np.random.default_rng(20261103)
    xs = (0.6 * rng.standard_normal((9, 16)) / 4.0).astype(np.float32)          # Euclidean features
    xe = xs.copy()
    xe[::2] *= np.float32(12.0)                                                 # ... every other row beyond clip_r
    xb = ball_points(rng, (9, 16), MODULE_C)                                    # points of the ball
    xp = (0.2 * rng.standard_normal(16)).astype(np.float32)
    net = dict(w=rng.uniform(-0.25, 0.25, (8, 16)).astype(np.float32), b=rng.uniform(-0.25, 0.25, 8).astype(np.float32),
               a=rng.uniform(-0.35, 0.35, (5, 8)).astype(np.float32), p=rng.uniform(-0.35, 0.35, (5, 8)).astype(np.float32))

    def plain(make):
        return lambda dtype: (make().to(dtype), None, lambda m, t: m(t))

    def build_net(dtype):
        c = torch.tensor(MODULE_C, dtype=dtype, requires_grad=True)
        m = nn.ModuleDict(dict(lin=hnn.HypLinear(16, 8, c=1.0), mlr=hnn.HyperbolicMLR(8, 5, c=1.0))).to(dtype)
        to = hnn.ToPoincare(c=c)
        return m, c, lambda mm, t: mm['mlr'](mm['lin'](to(t), c=c), c=c)
    mods = {
        'mod.to': (plain(lambda: hnn.ToPoincare(MODULE_C, train_c=True)), {}, xs, 16),
        'mod.to_xp_clip': (plain(lambda: hnn.ToPoincare(MODULE_C, train_c=True, train_x=True, ball_dim=16, clip_r=CLIP_R)), dict(xp=xp), xe, 16),
        'mod.from': (plain(lambda: hnn.FromPoincare(MODULE_C, train_c=True)), {}, xb, 16),
        'mod.from_xp': (plain(lambda: hnn.FromPoincare(MODULE_C, train_c=True, train_x=True, ball_dim=16)), dict(xp=xp), xb, 16),
        'mod.net': (build_net, {'lin.weight': net['w'], 'lin.bias': net['b'], 'mlr.a_vals': net['a'], 'mlr.p_vals': net['p']}, xs, 5),
    }
    short = {'lin.weight': 'w', 'lin.bias': 'b', 'mlr.a_vals': 'a', 'mlr.p_vals': 'p'}
    try:
        for name, (build, params, x, width) in mods.items():
            g = rng.standard_normal((9, width)).astype(np.float32)
            g64, shape = module_grads(build, params, x, g, torch.float64)
            g32, _ = module_grads(build, params, x, g, torch.float32)
            assert shape == g.shape, (name, shape)
            out[name + '.x'], out[name + '.g'] = x.astype(np.float32), g
            for k, v in params.items():
                out['%s.%s' % (name, short.get(k, k))] = v
            for k in g64:
                e = err(g32[k], g64[k])
                assert np.isfinite(g64[k]).all() and e <= BOUND, '%s d/d%s: the reference fp32 gradient is %.2e off: draw other inputs' % (name, k, e)
                note(name, e)
                out['%s.g%s' % (name, short.get(k, k))] = np.stack([g64[k], g32[k]])
    finally:
        pm.RiemannianGradient.c = 1
    path = os.path.join(HERE, 'pmath_cgrad.npz')
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < 300 * 1000, size
    print('wrote', path, size, 'bytes,', len(out), 'arrays')
    print('reference fp32 against its float64, worst per op: ' + ', '.join('%s %.1e' % kv for kv in sorted(worst.items())))


if __name__ == '__main__':
    main()
