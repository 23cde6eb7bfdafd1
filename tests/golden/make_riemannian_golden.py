#!/usr/bin/env python3
"""Generate tests/golden/riemannian.npz (Riemannian Adam / SGD trajectories, the edge and broadcast op cases) and riemannian_ops.npz (the
manifold row operations over the product of shapes) by IMPORTING THE REFERENCE on the
CPU -- core.manifolds.Oblique (proj, proj_tan, expmap, egrad2rgrad) and hyptorch.pmath (project, expmap, lambda_x) -- and running the
loops of tests/riemannian_ref.py (the closed-form gyration and the two update rules, which the reference does not have) on top of them:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_riemannian_golden.py

Data only.  Inputs and gradients are float32.  For every case two results are stored: `*64`, the run in FLOAT64 on the float32 inputs (the
yardstick), and `*32`, the float32 run of the same code.  The yardstick is stored as float32 (6e-8 relative, three orders below the tests'
bound), the float32 run as `*32d`, its exact distance from the stored yardstick in units of the last place (riemannian_ref.Fixture
gives it back bit for bit; small integers compress to a third).

Op cases (riemannian_ref.op_shapes(): d in {1, 2, 16, 63, 64, 65, 130, 300}, Oblique from d = 2, the ball at c in {1, 0.5}; each stored ONCE
with 9 rows: the cases with rows in {1, 5, 9} of riemannian_ref.op_cases() are its first rows, rows being independent):
  <case>.in     [4,9,d]  p, y (points), u, w (tangent vectors at p)
                            ball: points with sqrt(c) |.| uniform in [0.05, 0.9]; u, w random directions with sqrt(c) |.| uniform in
                            [0.05, 0.9] times (1 - c |p|^2), so that a unit step is a geodesic distance below 2
                            Oblique: unit rows; u, w projected on the tangent space of p in float64, |.| uniform in [0.1, 2]
  <case>.out64/.out32  [5,9,d]  riemannian_ref.OP_NAMES: egrad2rgrad(p, u), expmap(u, p), ptransp(p, y, w), retr_transp(p, u, w) (y, then v)
  <case>.inner64/.inner32  [9]  inner_p(u, w) (ball only)
  op.obl.edge   [9,16]: row 4 has u = 0, row 6 has |u| = 5e-5 (the proj(p + u) branch of expmap; no other row is within a factor 2 of 1e-4)
  op.ball.bcast p [2,3,16], y [3,16], u [3,16], w [16] as .p / .y / .u / .w, c 1.0: broadcast operands, results [5,2,3,16]
Optimiser cases (riemannian_ref.OPT_CASES, 8 steps, weight decay 0.01, rules adam / sgdm (momentum 0.9) / sgd0):
  opt.<case>.p<k>.x0 / .g [8,...]   start and the gradients, N(0,1) times the per-step scales (1, 1, 3, 0.1, 1, 1e-3, 1, 1)
  opt.<case>.p<k>.<rule>.{x,s1,s2}{64,32}  [8,...]  the parameter and its state buffers after every step (s1: exp_avg or momentum_buffer,
                                    s2: exp_avg_sq [..., 1])
  three: [9,16] Oblique, [2,3,65] ball c 0.5, [2100,8] ball c 1 (rows of period 25, stored in full: they compress)
  clip:  ball rows at sqrt(c) |x| = 0.99, gradients pointing inward with |g| uniform in [300, 600] (an SGD step is a geodesic distance of 3 to 6), lr 1: the retraction is clipped by
         project (Adam's steps are shorter than a geodesic distance of 1 whatever the gradient: its first three approach the sphere, the other
         five are clipped)
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get('STTODE_REFERENCE', '/root/reference')
sys.path.insert(0, os.path.dirname(HERE))
import riemannian_ref as rr  # noqa: E402


def reference():
    if REF not in sys.path:
        sys.path.insert(0, REF)
    import hyptorch.pmath as pm
    from core.manifolds import Oblique
    return pm, Oblique()


def ball_points(rng, shape, c, lo=0.05, hi=0.9):
    v = rng.standard_normal(shape)
    return v / np.linalg.norm(v, axis=-1, keepdims=True) * rng.uniform(lo, hi, shape[:-1] + (1,)) / np.sqrt(c)


def unit_rows(rng, shape):
    v = rng.standard_normal(shape)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def tangent(rng, p, lo=0.1, hi=2.0):
    """Tangent vectors at the float32-rounded unit rows p, of norm uniform in [lo, hi]."""
    p = p.astype(np.float32).astype(np.float64)
    v = rng.standard_normal(p.shape)
    v = v - (v * p).sum(-1, keepdims=True) * p / (p * p).sum(-1, keepdims=True)
    return v / np.linalg.norm(v, axis=-1, keepdims=True) * rng.uniform(lo, hi, p.shape[:-1] + (1,))


def both(fn):
    """fn(dtype) -> tensors; returns its float64 and float32 results as float32 arrays."""
    out = []
    for dt in (torch.float64, torch.float32):
        with torch.no_grad():
            res = fn(dt)
        out.append([None if r is None else r.to(torch.float32).numpy() for r in res])
    return out


def main():
    pm, obl = reference()
    rng = np.random.default_rng(20261201)
    z = {}

    def man_of(name, c):
        return rr.make_manifold(name, c, oblique_impl=obl, pm=pm)

    def op_case(name, man, p, y, u, w):
        arrs = [np.ascontiguousarray(a, dtype=np.float32) for a in (p, y, u, w)]
        (v64, i64), (v32, i32) = both(lambda dt: rr.run_ops(man, *[torch.from_numpy(a).to(dt) for a in arrs]))
        z[name + '.out64'], z[name + '.out32'] = v64, v32
        if man.name == 'poincare':
            z[name + '.inner64'], z[name + '.inner32'] = i64, i32
        return arrs

    rows = rr.MAX_ROWS
    for name, mname, c, d in rr.op_shapes():
        if mname == 'oblique':
            p, y = unit_rows(rng, (rows, d)), unit_rows(rng, (rows, d))
            u, w = tangent(rng, p), tangent(rng, p)
        else:
            p, y = ball_points(rng, (rows, d), c), ball_points(rng, (rows, d), c)
            room = 1 - c * (p.astype(np.float32).astype(np.float64) ** 2).sum(-1, keepdims=True)
            u, w = ball_points(rng, (rows, d), c) * room, ball_points(rng, (rows, d), c) * room
        z[name + '.in'] = np.stack(op_case(name, man_of(mname, c), p, y, u, w))
    # the two branches of Oblique.expmap
    p, y = unit_rows(rng, (9, 16)), unit_rows(rng, (9, 16))
    u, w = tangent(rng, p), tangent(rng, p)
    u[4] = 0
    u[6] *= 5e-5 / np.linalg.norm(u[6])
    z['op.obl.edge.in'] = np.stack(op_case('op.obl.edge', man_of('oblique', 1.0), p, y, u, w))
    n = np.linalg.norm(z['op.obl.edge.in'][2], axis=-1)
    assert n[4] == 0 and abs(n[6] - 5e-5) < 1e-9 and all(v > 2e-4 for i, v in enumerate(n) if i not in (4, 6))
    # broadcast operands
    p, y = ball_points(rng, (2, 3, 16), 1.0), ball_points(rng, (3, 16), 1.0)
    u, w = ball_points(rng, (3, 16), 1.0) * 0.1, ball_points(rng, (16,), 1.0) * 0.1
    for k, a in zip('pyuw', op_case('op.ball.bcast', man_of('poincare', 1.0), p, y, u, w)):
        z['op.ball.bcast.' + k] = a

    # optimiser trajectories
    for case, (params, lr) in rr.OPT_CASES.items():
        for k, (mname, c, shape) in enumerate(params):
            if mname == 'oblique':
                x0 = unit_rows(rng, shape)
            elif case == 'clip':
                x0 = ball_points(rng, shape, c, 0.99, 0.99)
            else:
                x0 = ball_points(rng, shape, c)
            g = rng.standard_normal((rr.STEPS,) + shape) * np.asarray(rr.SCALES).reshape((-1,) + (1,) * len(shape))
            if case == 'clip':
                g = -x0 / np.linalg.norm(x0, axis=-1, keepdims=True) * rng.uniform(300, 600, (rr.STEPS,) + shape[:-1] + (1,))
            if shape[0] > rr.BIG_PERIOD:
                reps = shape[0] // rr.BIG_PERIOD
                assert reps * rr.BIG_PERIOD == shape[0]
                x0, g = np.tile(x0[:rr.BIG_PERIOD], (reps, 1)), np.tile(g[:, :rr.BIG_PERIOD], (1, reps, 1))
            x0, g = x0.astype(np.float32), g.astype(np.float32)
            z['opt.%s.p%d.x0' % (case, k)], z['opt.%s.p%d.g' % (case, k)] = x0, g
            man = man_of(mname, c)
            for rule in rr.RULES:
                def run(dt):
                    steps = rr.run_rule(rule, man, torch.from_numpy(x0).to(dt), list(torch.from_numpy(g).to(dt)), lr)
                    return [None if steps[0][i] is None else torch.stack([s[i] for s in steps]) for i in range(3)]
                r64, r32 = both(run)
                for what, a64, a32 in zip(('x', 's1', 's2'), r64, r32):
                    if a64 is not None:
                        z[rr.opt_key(case, k, rule, what, 64)], z[rr.opt_key(case, k, rule, what, 32)] = a64, a32
    for k in [k for k in z if k.endswith('32')]:              # a float32 run is stored as its distance from the yardstick (rr.Fixture)
        z[k + 'd'] = rr.Fixture.pack(z.pop(k), z[k[:-2] + '64'])
    shapes = tuple(s[0] + '.' for s in rr.op_shapes())
    for fname, keys in (('riemannian_ops.npz', [k for k in z if k.startswith(shapes)]), ('riemannian.npz', [k for k in z if not k.startswith(shapes)])):
        out = os.path.join(HERE, fname)
        np.savez_compressed(out, **{k: z[k] for k in keys})
        print('wrote %s: %d arrays, %d bytes' % (out, len(keys), os.path.getsize(out)))


if __name__ == '__main__':
    main()
