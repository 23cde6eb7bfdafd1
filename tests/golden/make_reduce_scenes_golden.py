"""Writes tests/golden/reduce_scenes.npz: the stored cases of the scene-level oversample-and-reduce (tests/test_reduce_scenes.py CASES and
SHAPES).  NumPy and scipy only; the inputs and the float64 yardstick are the functions of tests/test_reduce.py applied to a segment's samples
as scene futures ([M, Tf, 2 A], tests/test_reduce_scenes.py scene_points), and every stored full-run segment is cross-checked against
scipy.cluster.vq.kmeans2 before it is written.

Per segment the seeds are searched upwards from the case's start (every segment takes the first qualifying seed behind its predecessor's):
a full-run seed (iters = 10) is kept when every sample at every iteration holds the near-tie margin 1e-3 on the float64 path (and, for
maximin, every pick's top two candidates do); a one-step seed when at most 1 % of the segment's samples fall below it.  Stored per full-run
case: seeds [S], seg_ptr [S+1], init [n,K,Tf,2] f32 (the initial centroids: the scene futures 'first' / 'maximin' pick), centroids
[n,K,Tf,2] f64, labels [S,M], counts [S,K].  Per one-step shape: seeds [S] only -- the test regenerates the rest.

    python tests/golden/make_reduce_scenes_golden.py
"""
import os
import sys
import warnings

import numpy as np
from scipy.cluster.vq import kmeans2

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from test_reduce_scenes import CASES, SHAPES, scene_points, seg_ptr_of, segment_case  # noqa: E402


def search(tag, start, sizes, M, K, Tf, t0, init, kind):
    rows, seed, tried = [], start, 0
    for A in sizes:
        while True:
            x, c0, iters, (c, lab, cnt, marg), ok = segment_case(seed, A, M, K, Tf, t0, init, kind)
            seed += 1
            tried += 1
            assert tried < 40 * len(sizes) + 200, f'{tag}: too few qualifying seeds'
            if ok:
                break
        if kind == 'full':
            with warnings.catch_warnings():
                warnings.simplefilter('ignore')
                book, code = kmeans2(scene_points(x)[:, t0:].reshape(M, -1).astype(np.float64),
                                     scene_points(c0)[:, t0:].reshape(K, -1).astype(np.float64), iter=iters, minit='matrix')
            assert (code == lab).all() and np.abs(book - scene_points(c)[:, t0:].reshape(K, -1)).max() <= 1e-12 * np.abs(x).max(), (tag, seed)
        rows.append((seed - 1, c0, c, lab, cnt))
    print(f'{tag}: {len(sizes)} of {tried} seeds kept')
    return rows


def main():
    out = {'cases': np.array(sorted(CASES)), 'shapes': np.array(sorted(SHAPES))}
    for tag, (start, sizes, M, K, Tf, t0, init) in CASES.items():
        rows = search(tag, start, sizes, M, K, Tf, t0, init, 'full')
        out[f'{tag}/seeds'] = np.array([r[0] for r in rows])
        out[f'{tag}/seg_ptr'] = seg_ptr_of(sizes)
        out[f'{tag}/init'] = np.concatenate([r[1] for r in rows])
        out[f'{tag}/centroids'] = np.concatenate([r[2] for r in rows])
        out[f'{tag}/labels'] = np.stack([r[3] for r in rows])
        out[f'{tag}/counts'] = np.stack([r[4] for r in rows])
    for tag, (start, sizes, R, K_in, K, Tf, t0) in SHAPES.items():
        out[f'{tag}/seeds'] = np.array([r[0] for r in search(tag, start, sizes, R * K_in, K, Tf, t0, None, 'step')])
    path = os.path.join(HERE, 'reduce_scenes.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
