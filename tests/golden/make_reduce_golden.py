"""Writes tests/golden/reduce.npz: the stored cases of oversample-and-reduce (tests/test_reduce.py CASES).  NumPy and scipy only; the inputs
and the float64 yardstick are the functions of tests/test_reduce.py, and every stored case is cross-checked against
scipy.cluster.vq.kmeans2 before it is written.

Per case the seeds are searched upwards from the case's start: a full-run seed (iters = 10) is kept when every sample at every iteration
holds the near-tie margin 1e-3 on the float64 path (and, for maximin, every pick's top two candidates do); a one-step seed when at most
1 % of its samples fall below it.  Stored per case: seeds [n], x [n,M,Tf,2] f32, init [n,K,Tf,2] f32 (the initial centroids: samples for
'first' / 'maximin', the caller's for one-step cases), centroids [n,K,Tf,2] f64, labels [n,M], counts [n,K], and for one-step cases
sure [n,M] (margin >= 1e-3).

    python tests/golden/make_reduce_golden.py
"""
import os
import sys
import warnings

import numpy as np
from scipy.cluster.vq import kmeans2

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from test_reduce import CASES, MARGIN, case_agent  # noqa: E402


def main():
    out = {'cases': np.array(sorted(CASES))}
    for tag, (kind, start, n, M, K, Tf, t0, init) in CASES.items():
        rows, seed, tried = [], start, 0
        while len(rows) < n:
            x, c0, iters, (c, lab, cnt, marg), ok = case_agent(seed, M, K, Tf, t0, init, kind)
            tried += 1
            if ok:
                with warnings.catch_warnings():
                    warnings.simplefilter('ignore')
                    book, code = kmeans2(x[:, t0:].reshape(M, -1).astype(np.float64), c0[:, t0:].reshape(K, -1).astype(np.float64),
                                         iter=iters, minit='matrix')
                assert (code == lab).all() and np.abs(book - c[:, t0:].reshape(K, -1)).max() <= 1e-12 * np.abs(x).max(), (tag, seed)
                rows.append((seed, x, c0, c, lab, cnt, marg[-1] >= MARGIN))
            seed += 1
            assert seed - start < 100, f'{tag}: fewer than {n} qualifying seeds among 100'
        print(f'{tag}: {n} of {tried} seeds kept')
        for i, name in enumerate(('seeds', 'x', 'init', 'centroids', 'labels', 'counts')):
            out[f'{tag}/{name}'] = np.stack([np.asarray(r[i]) for r in rows])
        if kind == 'step':
            out[f'{tag}/sure'] = np.stack([r[6] for r in rows])
    path = os.path.join(HERE, 'reduce.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
