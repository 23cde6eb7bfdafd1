#!/usr/bin/env python3
"""Generate tests/golden/delta.npz (Gromov delta-hyperbolicity) by IMPORTING THE REFERENCE's hyptorch/delta.py and hyptorch/pmath.py:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_delta_golden.py

hyptorch/delta.py imports torchvision at module level for get_delta's VGG16 (never called here); an empty stand-in module is put into
sys.modules first.  Stored (inputs float32, reference outputs float64):
  dh_<tag>_X / dh_<tag>_delta / dh_<tag>_diam   delta_hyp(distance_matrix(X, X)) and its maximum, X float32 as stored (scipy in float64)
      tags: gauss (n 300, d 128), circle (n 257, d 2), clusters (n 240, d 16), n1 / n2 / n3 / n65 (Gaussian, d 8)
  ns_D / ns_delta                                 delta_hyp of a non-symmetric positive matrix, n 129
  bt_X, bt_seed, bt_mean, bt_std, bt_next         batched_delta_hyp(X 3000 x 16, n_tries 4, batch_size 300) under np.random.seed(bt_seed),
                                                  and the np.random.rand() that follows (pins the RNG state)
  pc_X / pc_c / pc_delta / pc_diam                delta_hyp of the reference's pmath.dist_matrix (float64) of X inside the ball (|x| < 0.9),
                                                  n 200, d 8, and that matrix's maximum
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get('STTODE_REFERENCE', '/root/reference')


def reference_delta():
    if REF not in sys.path:
        sys.path.insert(0, REF)
    sys.modules.setdefault('torchvision', types.ModuleType('torchvision'))
    from hyptorch import delta, pmath
    return delta, pmath


def main():
    delta, pmath = reference_delta()
    import torch
    from scipy.spatial import distance_matrix
    rng = np.random.default_rng(20261016)
    out = {}
    cases = {'gauss': rng.standard_normal((300, 128)),
             'circle': np.stack([np.cos(np.linspace(0, 2 * np.pi, 257, endpoint=False)),
                                 np.sin(np.linspace(0, 2 * np.pi, 257, endpoint=False))], 1) * 3.0,
             'clusters': (rng.standard_normal((6, 1, 16)) * 5.0 + rng.standard_normal((6, 40, 16)) * 0.3).reshape(240, 16)}
    for n in (1, 2, 3, 65):
        cases['n%d' % n] = rng.standard_normal((n, 8))
    for tag, X in cases.items():
        X = X.astype(np.float32)
        D = distance_matrix(X.astype(np.float64), X.astype(np.float64))
        out['dh_%s_X' % tag] = X
        out['dh_%s_delta' % tag] = np.float64(delta.delta_hyp(D))
        out['dh_%s_diam' % tag] = np.float64(D.max())
    ns = rng.uniform(0.5, 4.0, (129, 129)).astype(np.float32)
    out['ns_D'] = ns
    out['ns_delta'] = np.float64(delta.delta_hyp(ns.astype(np.float64)))
    Xb = rng.standard_normal((3000, 16)).astype(np.float32)
    seed = 1234
    np.random.seed(seed)
    m, s = delta.batched_delta_hyp(Xb.astype(np.float64), n_tries=4, batch_size=300)
    out.update(bt_X=Xb, bt_seed=np.int64(seed), bt_mean=np.float64(m), bt_std=np.float64(s), bt_next=np.float64(np.random.rand()))
    Xp = rng.standard_normal((200, 8))
    Xp = Xp / np.linalg.norm(Xp, axis=1, keepdims=True) * rng.uniform(0.05, 0.9, (200, 1))
    Xp = Xp.astype(np.float32)
    c = 1.0
    Dp = pmath.dist_matrix(torch.from_numpy(Xp.astype(np.float64)), torch.from_numpy(Xp.astype(np.float64)), c=c).numpy()
    out.update(pc_X=Xp, pc_c=np.float64(c), pc_delta=np.float64(delta.delta_hyp(Dp)), pc_diam=np.float64(Dp.max()))
    path = os.path.join(HERE, 'delta.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes;', {k: float(v) for k, v in out.items() if np.ndim(v) == 0})


if __name__ == '__main__':
    main()
