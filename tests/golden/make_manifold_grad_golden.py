#!/usr/bin/env python3
"""Generate tests/golden/manifold_grad.npz by IMPORTING THE REFERENCE on the CPU -- hyptorch.pmath.poincare_mean and core.manifolds.Oblique
(proj, proj_tan, expmap, dist, inner; ptransp and retr_transp under the loops of tests/riemannian_ref.py, as make_riemannian_golden.py
does) -- and differentiating its functions by torch autograd:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_manifold_grad_golden.py

Data only.  Inputs and upstream gradients are float32.  `*64`: the run in FLOAT64 on the float32 inputs (the yardstick, stored as float32);
`*32`: the float32 run of the same code, stored as `*32d`, its distance from the stored yardstick in units of the last place
(riemannian_ref.Fixture).  The upstream gradients are N(0, 1) from the seed manifold_grad_cases.SEED.

poincare_mean (manifold_grad_cases.mean_cases(): [R, W, d] over R in {1, 2, 9}, W in {1, 5}, d in {1, 2, 16, 65, 130}, dim in {0, 1}, c in
{1, 0.5}; [2, 3, 2, 16] with dim 1):
  x                                 the input, sqrt(c) |x| uniform in [0.05, 0.95]; in [2, 5, 16]: x[1, 1] = -x[0, 1], x[0, 3] = 0
  g / out64 / out32                 upstream gradient and value
  gx64 / gx32, gc64 / gc32          dL/dx, and dL/dc [1] with c a tensor that requires grad
  each stored ONCE for all cases as the flat array mean.<kind>, the cases' arrays one after the other in mean_cases() order (x: one per
  shape and c, in the order of first use): manifold_grad_cases.MeanFixture cuts them apart
Oblique row ops (inputs p, y, u, w: riemannian_ops.npz `op.obl.d<d>.in`, d in {2, 16, 63, 64, 65, 130, 300}, 9 rows):
  obl.d<d>.g [2, 9, d]              upstream gradients (the second: of retr_transp's transported vector)
  obl.d<d>.<op>.grads64 / .grads32  [k, 9, d]: the gradients of the operands in manifold_grad_cases.OBL_OPERANDS[op] order
                                    proj(w), proj_tan(u, p), expmap(u, p), ptransp(p, y, w), retr_transp(p, u, w)
  obl.edge.*                        the same for expmap and retr_transp at op.obl.d16's inputs with u[4] = 0: expmap's proj(p + u) branch,
                                    differentiated AS TAKEN (manifold_grad_cases.TakenOblique: torch.where gives NaN there)
  obl.inner.gu64 / .gv64 / ...      Oblique.inner(p, u, w) = u w^T as the [9, 9] matrix it is, at d 16, upstream obl.inner.g
Oblique.dist (manifold_grad_cases.OBL_DIST: (nb, n1, n2, d)):
  dist.<nb>.<n1>.<n2>.<d>.p1 / .p2 / .g   unit rows; in (1, 9, 5, 16): p2[0, 0] = p1[0, 0], p2[0, 1] = -p1[0, 1] (clamped: zero gradient)
  ....out64 / .out32, .g164 / .g132, .g264 / .g232
The float64 runs take the reference's float32 thresholds (see reference()).  Asserted here in float64: no un-clamped inner product within 1e-5 of +-(1 - 1e-4); every Oblique |u| is 0 or >= 1e-3.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get('STTODE_REFERENCE', '/root/reference')
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import manifold_grad_cases as mc  # noqa: E402
import riemannian_ref as rr  # noqa: E402


def reference():
    if REF not in sys.path:
        sys.path.insert(0, REF)
    import hyptorch.pmath as pm
    import core.manifolds.oblique as oblique
    # the reference keys its thresholds by dtype (oblique.py:7: 1e-4 for float32, 1e-7 for float64).  The yardstick is the float64 run of the
    # FLOAT32 function, so the float64 run takes the float32 thresholds: dist's clamp at +-(1 - 1e-4), expmap's branch at |u| = 1e-4.
    oblique.EPS[torch.float64] = oblique.EPS[torch.float32]
    return pm, oblique.Oblique()


def unit_rows(rng, shape):
    v = rng.standard_normal(shape)
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(np.float32)


def main():
    pm, obl = reference()
    rng = np.random.default_rng(mc.SEED)
    z = {}
    f32 = lambda shape: rng.standard_normal(shape).astype(np.float32)   # noqa: E731

    # ---- poincare_mean
    xs, flat = {}, {k: [] for k in mc.MEAN_KINDS}
    for name, shape, dim, c in mc.mean_cases():
        key = mc.mean_input_key(name)
        if key not in xs:
            v = rng.standard_normal(shape)
            x = v / np.linalg.norm(v, axis=-1, keepdims=True) * rng.uniform(0.05, 0.95, shape[:-1] + (1,)) / np.sqrt(c)
            if shape == mc.MEAN_SPECIAL:
                x[1, 1] = -x[0, 1]
                x[0, 3] = 0
            xs[key] = x.astype(np.float32)
            flat['x'].append(xs[key])
            assert (np.sqrt(c) * np.linalg.norm(xs[key].astype(np.float64), axis=-1) <= 0.95 + 1e-6).all()
        x = xs[key]
        g = f32(shape[:dim] + shape[dim + 1:])
        flat['g'].append(g)
        for dt, tag in ((torch.float64, '64'), (torch.float32, '32')):
            xt = torch.from_numpy(x).to(dt).requires_grad_()
            ct = torch.tensor([c], dtype=dt, requires_grad=True)
            out = pm.poincare_mean(xt, dim=dim, c=ct)
            gx, gc = torch.autograd.grad((out * torch.from_numpy(g).to(dt)).sum(), (xt, ct))
            for kind, a in zip(('out', 'gx', 'gc'), (out, gx, gc)):
                flat[kind + tag].append(a.detach().to(torch.float32).numpy())
                assert np.isfinite(flat[kind + tag][-1]).all(), name
    for kind, arrs in flat.items():
        z['mean.' + kind] = np.concatenate([a.ravel() for a in arrs])

    # ---- Oblique row ops, on the inputs of riemannian_ops.npz
    ops = np.load(os.path.join(HERE, 'riemannian_ops.npz'))
    man = mc.TakenOblique(obl)

    def obl_case(name, ins, which):
        un = np.linalg.norm(ins[2].astype(np.float64), axis=-1)
        assert ((un == 0) | (un >= 1e-3)).all(), name
        gs = z[name + '.g'] = f32((2,) + ins.shape[1:])
        for op in which:
            for dt, tag in ((torch.float64, '64'), (torch.float32, '32')):
                outs, grads = mc.vjp(lambda *t: mc.obl_run(man, op, *t), list(ins), list(gs), dt)
                z['%s.%s.grads%s' % (name, op, tag)] = np.stack(grads)
                assert np.isfinite(grads).all(), (name, op)

    for name, key, d in mc.obl_cases():
        obl_case(name, ops[key], mc.OBL_OPS)
    ins = ops['op.obl.d16.in'].copy()
    ins[2, mc.EDGE_ZERO_ROW] = 0
    z['obl.edge.in'] = ins
    obl_case('obl.edge', ins, ('expmap', 'retr_transp'))
    # Oblique.inner as the matrix it is
    p, _, u, w = ops['op.obl.d16.in']
    g = z['obl.inner.g'] = f32((9, 9))
    for dt, tag in ((torch.float64, '64'), (torch.float32, '32')):
        ut, wt = [torch.from_numpy(a).to(dt).requires_grad_() for a in (u, w)]
        out = obl.inner(torch.from_numpy(p).to(dt), ut, wt)
        gu, gv = torch.autograd.grad((out * torch.from_numpy(g).to(dt)).sum(), (ut, wt))
        z['obl.inner.gu' + tag], z['obl.inner.gv' + tag] = gu.to(torch.float32).numpy(), gv.to(torch.float32).numpy()

    # ---- Oblique.dist
    for nb, n1, n2, d in mc.OBL_DIST:
        name = 'dist.%d.%d.%d.%d' % (nb, n1, n2, d)
        p1, p2 = unit_rows(rng, (nb, n1, d)), unit_rows(rng, (nb, n2, d))
        if (nb, n1, n2, d) == mc.OBL_DIST_SPECIAL:
            p2[0, 0], p2[0, 1] = p1[0, 0], -p1[0, 1]
        s = np.einsum('bid,bjd->bij', p2.astype(np.float64), p1.astype(np.float64))
        assert (np.abs(np.abs(s) - (1 - 1e-4)) > 1e-5).all(), name
        g = f32((nb, n2, n1))
        z[name + '.p1'], z[name + '.p2'], z[name + '.g'] = p1, p2, g
        for dt, tag in ((torch.float64, '64'), (torch.float32, '32')):
            a, b = [torch.from_numpy(t).to(dt).requires_grad_() for t in (p1, p2)]
            out = obl.dist(a, b)
            g1, g2 = torch.autograd.grad((out * torch.from_numpy(g).to(dt)).sum(), (a, b))
            z[name + '.out' + tag], z[name + '.g1' + tag], z[name + '.g2' + tag] = [t.detach().to(torch.float32).numpy() for t in (out, g1, g2)]
        if (nb, n1, n2, d) == mc.OBL_DIST_SPECIAL:
            assert abs(s[0, 0, 0]) > 1 - 1e-5 and abs(s[0, 1, 1]) > 1 - 1e-5

    for k in [k for k in z if k.endswith('32')]:
        z[k + 'd'] = rr.Fixture.pack(z.pop(k), z[k[:-2] + '64'])
    out = os.path.join(HERE, 'manifold_grad.npz')
    np.savez_compressed(out, **z)
    print('wrote %s: %d arrays, %d bytes' % (out, len(z), os.path.getsize(out)))


if __name__ == '__main__':
    main()
