#!/usr/bin/env python3
"""Generate tests/golden/hypnn.npz (gradients of the hyperbolic layers, their surface and one short training run) by IMPORTING THE REFERENCE's
hyptorch/nn.py and hyptorch/pmath.py and differentiating them with torch autograd on the CPU:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_hypnn_golden.py

Data only.  The cases and the layout of a stored case are in tests/hypnn_cases.py.  Inputs are float32; for every case
the reference is run in FLOAT64 on the float32 inputs (the yardstick, stored rounded to float32) and in its own float32 (stored as its
difference from the yardstick, `32d`, which has few significant bits and compresses; hypnn_cases.case_grads adds it back).  Upstream gradients
are drawn, rounded to float16 and stored as float16 (exact in float32).

  hs.<shape>    _hyperbolic_softmax(X, A, P, c): X on the ball with sqrt(c) |.| in [0.05, 0.9], A ~ 0.3 N(0,1), P on the ball with sqrt(c) |.| in
                [0.05, 0.7] -- at 0.9 the reference's own fp32 gradients leave the bound (3e-4); g [B,C] ~ N(0,1)
  mab.<shape>   _mobius_addition_batch(x [B,d], y [C,d], c), both on the ball ([0.05, 0.9]); g [B,C,d]
  clip.<kind>   x min(1, r / (|x| + 1e-5)), r = 2.3: rows of norm [2.6, 5] (clipped), [0.1, 2] (unclipped), and [0.1, 5] with one zero row (mixed)
  mod.<name>    the reference's modules (hypnn_cases.MODULES) with drawn parameters; mod.mlr.<shape>: HyperbolicMLR with a_vals ~ 0.3 N(0,1) and
                tangent p_vals with sqrt(c) |.| in [0.05, 0.9].  Every mod.* case also stores the module's forward value, <case>.out64 /
                out32d, coded like the gradients
  init.<name>   state_dict names (.names), and values under torch.manual_seed(0), of every module of hypnn_cases.INIT_MODULES
  train.*       ToPoincare(c=1, clip_r=2.3) -> HypLinear(16, 8) -> HyperbolicMLR(8, 5) on 32 rows, cross-entropy, torch.optim.Adam(lr=1e-2), 5
                steps: the initial state_dict (train.sd.<key>), x, labels, and the 5 losses of the float64 and of the float32 run
The generator asserts that the reference's fp32 gradients and module forward values are within the bound of its float64 ones for every case.
"""
import copy
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from hypnn_cases import (BOUND, CLIP_R, INIT_MODULES, MODULES, SHAPES, TRAIN_LR, TRAIN_ROWS, TRAIN_STEPS, err, shape_tag,  # noqa: E402
                         train_model)
from make_pmath_vjp_golden import ball_points, reference  # noqa: E402


def store(out, case, fn, inputs, g, module=None):
    """Run fn(*inputs) (fn: a function, or the module itself) in float64 and float32 and store inputs, parameters, g, every gradient and,
    for a module, its forward value (<case>.out64 / out32d)."""
    import torch
    for k, a in enumerate(inputs):
        out['%s.in.%d' % (case, k)] = a
    out[case + '.g'] = g.astype(np.float16)
    if module is not None:
        for n, p in module.state_dict().items():
            out['%s.p.%s' % (case, n)] = p.numpy().copy()
    for tag, dt in (('64', torch.float64), ('32', torch.float32)):
        m = copy.deepcopy(module).to(dt) if module is not None else None
        ts = [torch.from_numpy(a).to(dt).requires_grad_() for a in inputs]
        res = (m if m is not None else fn)(*ts)
        res.backward(torch.from_numpy(g).to(dt).reshape(res.shape))
        if m is not None:
            out['%s.out%s' % (case, tag)] = res.detach().numpy().astype(np.float32)     # the module's forward value
        for k, t in enumerate(ts):
            out['%s.gin.%d%s' % (case, k, tag)] = t.grad.numpy().astype(np.float32)
        if m is not None:
            for n, p in m.named_parameters():
                out['%s.gp.%s%s' % (case, n, tag)] = p.grad.numpy().astype(np.float32)
    for k in [k for k in out if (k.startswith(case + '.g') or k == case + '.out32') and k.endswith('32')]:
        out[k + 'd'] = out.pop(k) - out[k[:-2] + '64']      # stored as the difference from the yardstick: few significant bits, it compresses


def set_params(module, values):
    import torch
    with torch.no_grad():
        for n, p in module.named_parameters():
            p.copy_(torch.from_numpy(values[n]))


def main():
    pm, hnn = reference()
    import torch
    out = {}
    rng = np.random.default_rng(20261022)
    f32 = lambda a: np.asarray(a, np.float32)
    f16 = lambda a: np.asarray(a, np.float16).astype(np.float32)
    for B, C, d, c in SHAPES:
        sh = shape_tag(B, C, d, c)
        ct = lambda t, c=c: torch.as_tensor(c, dtype=t.dtype)
        X, P, A = ball_points(rng, (B, d), c), ball_points(rng, (C, d), c, 0.05, 0.7), f32(0.3 * rng.standard_normal((C, d)))
        store(out, 'hs.' + sh, lambda x, a, p: pm._hyperbolic_softmax(x, a, p, ct(x)), [X, A, P], f16(rng.standard_normal((B, C))))
        x, y = ball_points(rng, (B, d), c), ball_points(rng, (C, d), c)
        store(out, 'mab.' + sh, lambda a, b, c=c: pm._mobius_addition_batch(a, b, c), [x, y], f16(rng.standard_normal((B, C, d))))
        m = MODULES['mlr.' + sh](hnn)
        set_params(m, {'a_vals': f32(0.3 * rng.standard_normal((C, d))), 'p_vals': ball_points(rng, (C, d), c)})
        store(out, 'mod.mlr.' + sh, None, [ball_points(rng, (B, d), c)], f16(rng.standard_normal((B, C))), module=m)

    def clip(x):
        n = torch.norm(x, dim=-1, keepdim=True) + 1e-5
        return x * torch.minimum(torch.ones_like(n), CLIP_R / n)      # the formula of the issue; ToPoincare(clip_r) is held to the module below

    def rows_of_norm(n, d, lo, hi):
        v = rng.standard_normal((n, d))
        return f32(v / np.linalg.norm(v, axis=-1, keepdims=True) * rng.uniform(lo, hi, (n, 1)))
    mixed = rows_of_norm(9, 130, 0.1, 5.0)
    mixed[7] = 0
    for kind, x in (('clipped', rows_of_norm(9, 16, 2.6, 5.0)), ('unclipped', rows_of_norm(9, 16, 0.1, 2.0)), ('mixed', mixed)):
        store(out, 'clip.' + kind, clip, [x], f16(rng.standard_normal(x.shape)))

    def uni(*shape):
        return f32(rng.uniform(-0.25, 0.25, shape))
    tangent = ball_points(rng, (16,), 1.0, 0.3, 0.3)
    for name, params, inputs, gshape in (
            ('hyplinear', {'weight': uni(8, 16), 'bias': uni(8)}, [ball_points(rng, (9, 16), 0.5)], (9, 8)),
            ('hyplinear_nobias', {'weight': uni(7, 65)}, [ball_points(rng, (70, 65), 1.0)], (70, 7)),
            ('concat', {'l1.weight': uni(8, 16), 'l2.weight': uni(8, 5)}, [ball_points(rng, (9, 16), 1.0), ball_points(rng, (9, 5), 1.0)], (9, 8)),
            ('distlayer', {}, [ball_points(rng, (9, 16), 0.5), ball_points(rng, (9, 16), 0.5)], (9, 1)),
            ('topoincare', {}, [rows_of_norm(9, 16, 0.5, 4.0)], (9, 16)),
            ('topoincare_euclidean_grad', {}, [rows_of_norm(9, 16, 0.1, 1.5)], (9, 16)),
            ('topoincare_train_x', {'xp': tangent}, [rows_of_norm(9, 16, 0.1, 1.0)], (9, 16)),
            ('frompoincare', {}, [ball_points(rng, (9, 16), 1.0)], (9, 16)),
            ('frompoincare_train_x', {'xp': tangent}, [ball_points(rng, (9, 16), 1.0)], (9, 16))):
        m = MODULES[name](hnn)
        set_params(m, params)
        store(out, 'mod.' + name, None, inputs, f16(rng.standard_normal(gshape)), module=m)

    for name, make in INIT_MODULES.items():
        torch.manual_seed(0)
        sd = make(hnn).state_dict()
        out['init.%s.names' % name] = np.array(list(sd), dtype=np.str_)
        for k, v in sd.items():
            out['init.%s.%s' % (name, k)] = v.numpy().copy()

    torch.manual_seed(0)
    model = train_model(hnn)
    x, labels = f32(0.6 * rng.standard_normal((TRAIN_ROWS, 16))), rng.integers(0, 5, TRAIN_ROWS)
    out['train.x'], out['train.labels'] = x, labels.astype(np.int64)
    for k, v in model.state_dict().items():
        out['train.sd.' + k] = v.numpy().copy()
    for tag, dt in (('64', torch.float64), ('32', torch.float32)):
        m = copy.deepcopy(model).to(dt)
        opt = torch.optim.Adam(m.parameters(), lr=TRAIN_LR)
        losses = []
        for _ in range(TRAIN_STEPS):
            opt.zero_grad()
            loss = torch.nn.functional.cross_entropy(m(torch.from_numpy(x).to(dt)), torch.from_numpy(labels))
            loss.backward()
            opt.step()
            losses.append(float(loss))
        out['train.loss' + tag] = np.array(losses, np.float64)
    assert out['train.loss64'][-1] < out['train.loss64'][0]

    worst = {}
    for k in out:
        if k.endswith('64') and k[:-2] + '32d' in out:
            assert np.isfinite(out[k]).all() and np.isfinite(out[k[:-2] + '32d']).all(), k
            e = err(out[k] + out[k[:-2] + '32d'], out[k])
            assert e <= BOUND, ('the reference fp32 %s is outside the bound' % ('forward value' if k.endswith('.out64') else 'gradient'), k, e)
            fam = k.split('.')[0] + ('.' + k.split('.')[1] if k.startswith('mod.') else '') + (' forward' if k.endswith('.out64') else '')
            worst[fam] = max(worst.get(fam, 0.0), e)
    path = os.path.join(HERE, 'hypnn.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes,', len(out), 'arrays')
    for fam in sorted(worst):
        print('  %-32s worst reference fp32 error %.2e' % (fam, worst[fam]))
    print('  training losses float64', out['train.loss64'], ' fp32 off by %.2e' % err(out['train.loss32'], out['train.loss64']))


if __name__ == '__main__':
    main()
