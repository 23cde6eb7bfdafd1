#!/usr/bin/env python3
"""Generate tests/golden/selection.npz (best-of-K selection) by IMPORTING THE REFERENCE's utils/metrics.py (as make_golden.py does):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_selection_golden.py

Stored per case <tag>: seeded inputs pred [n, K, Tf, 2] / gt [n, Tf, 2] (float32) and a ragged scene CSR scene_ptr [S+1], and the
reference's outputs on them -- get_best_idx over all agents, per scene compute_ADE / compute_FDE, per scene count_miss_samples at the
thresholds in `thresholds` ([len(thresholds), S]).  Cases cover K = 1, 20, 64 and Tf = 1, 12, 20, and two cases with deliberate exact ties
(duplicated samples) that pin the first-index rule of np.argmin.  Apart from the deliberate ties, every agent's best and second-best ADE
differ by more than 1e-5 relative, so the index of any fp32 evaluation is the reference's.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get('STTODE_REFERENCE', '/root/reference')
THRESHOLDS = np.array([0.5, 1.0, 2.0])


def reference_metrics():
    if REF not in sys.path:
        sys.path.insert(0, REF)
    from utils.metrics import compute_ADE, compute_FDE, count_miss_samples, get_best_idx
    return compute_ADE, compute_FDE, count_miss_samples, get_best_idx


def ragged_ptr(rng, S, lo, hi):
    return np.concatenate([[0], np.cumsum(rng.integers(lo, hi + 1, S))]).astype(np.int32)


def draw(rng, n, K, Tf, spread):
    """Futures: a straight walk; samples: the future plus a random offset that grows along the horizon (FDE near the thresholds)."""
    start, vel = rng.uniform(-5, 5, (n, 1, 2)), rng.normal(0, 0.4, (n, 1, 2))
    gt = start + vel * np.arange(1, Tf + 1)[None, :, None]
    drift = rng.normal(0, spread, (n, K, 1, 2)) * np.linspace(0.3, 1.0, Tf)[None, None, :, None]
    pred = gt[:, None] + drift + rng.normal(0, 0.05 * spread, (n, K, Tf, 2))
    return pred.astype(np.float32), gt.astype(np.float32)


def ade_np(pred, gt):
    return np.linalg.norm(pred - gt[:, None], axis=-1).mean(axis=-1)      # [n, K], the reference's arithmetic


def separate(rng, pred, gt, keep=None):
    """Redraw the agents (other than `keep`) whose best and second-best ADE are closer than 1e-5 relative."""
    for _ in range(50):
        d = np.sort(ade_np(pred, gt), axis=1)
        if d.shape[1] < 2:
            return pred
        bad = (d[:, 1] - d[:, 0]) <= 1e-5 * d[:, 1]
        if keep is not None:
            bad &= ~keep
        if not bad.any():
            return pred
        pred[bad] += rng.normal(0, 0.01, pred[bad].shape).astype(np.float32)
    raise RuntimeError('could not separate near-ties')


def main():
    compute_ADE, compute_FDE, count_miss_samples, get_best_idx = reference_metrics()
    rng = np.random.default_rng(20261015)
    out = {'thresholds': THRESHOLDS}
    cases = []
    # tag, S, scene sizes, K, Tf, spread
    for tag, S, lo, hi, K, Tf, spread in (('k20_t12', 10, 1, 12, 20, 12, 4.0), ('k1_t12', 9, 1, 9, 1, 12, 1.5),
                                          ('k64_t12', 5, 1, 8, 64, 12, 8.0), ('k64_t20', 3, 2, 6, 64, 20, 8.0),
                                          ('k20_t1', 10, 1, 12, 20, 1, 4.0), ('k6_t12', 30, 1, 4, 6, 12, 2.0)):
        sp = ragged_ptr(rng, S, lo, hi)
        pred, gt = draw(rng, int(sp[-1]), K, Tf, spread)
        cases.append((tag, sp, separate(rng, pred, gt), gt))
    # deliberate exact ties: the best sample of every agent duplicated into three later slots
    sp = ragged_ptr(rng, 8, 1, 8)
    n, K, Tf = int(sp[-1]), 20, 12
    pred, gt = draw(rng, n, K, Tf, 4.0)
    tie = np.zeros(n, bool)
    for a in range(n):
        k0 = int(rng.integers(0, K - 3))
        pred[a, k0] = gt[a] + rng.normal(0, 0.3 if a % 2 else 0.8, (Tf, 2)).astype(np.float32)      # clearly the best sample
        for k in rng.choice(np.arange(k0 + 1, K), 3, replace=False):
            pred[a, k] = pred[a, k0]
        tie[a] = True
    pred[0] = pred[0, :1]                                                          # one agent: all K samples identical -> index 0
    cases.append(('ties_k20_t12', sp, separate(rng, pred, gt, keep=tie), gt))
    sp = ragged_ptr(rng, 4, 1, 5)
    n, K, Tf = int(sp[-1]), 64, 12
    pred, gt = draw(rng, n, K, Tf, 8.0)
    pred[:, 40:] = pred[:, :24]                                                     # samples 40..63 repeat 0..23: the minimum appears twice
    cases.append(('ties_k64_t12', sp, pred, gt))

    for tag, sp, pred, gt in cases:
        S = len(sp) - 1
        fde = np.linalg.norm(pred[:, :, -1] - gt[:, None, -1], axis=-1).min(axis=1)
        assert (np.abs(fde[:, None] - THRESHOLDS[None]) > 1e-4 * THRESHOLDS[None]).all(), tag    # miss counts do not hinge on rounding
        agents = [pred[a] for a in range(pred.shape[0])]
        out[tag + '/pred'], out[tag + '/gt'], out[tag + '/scene_ptr'] = pred, gt, sp
        out[tag + '/best_idx'] = np.asarray(get_best_idx(agents, gt), dtype=np.int64)
        out[tag + '/scene_ade'] = np.array([compute_ADE(agents[sp[s]:sp[s + 1]], gt[sp[s]:sp[s + 1]]) for s in range(S)], dtype=np.float64)
        out[tag + '/scene_fde'] = np.array([compute_FDE(agents[sp[s]:sp[s + 1]], gt[sp[s]:sp[s + 1]]) for s in range(S)], dtype=np.float64)
        out[tag + '/scene_miss'] = np.array([[count_miss_samples(agents[sp[s]:sp[s + 1]], gt[sp[s]:sp[s + 1]], mr_threshold=t)
                                              for s in range(S)] for t in THRESHOLDS], dtype=np.int64)
        print('%-14s n=%3d S=%2d K=%2d Tf=%2d  misses at %s: %s' % (tag, pred.shape[0], S, pred.shape[1], pred.shape[2], THRESHOLDS.tolist(),
                                                                  out[tag + '/scene_miss'].sum(axis=1).tolist()))
    out['cases'] = np.array([c[0] for c in cases])
    np.savez_compressed(os.path.join(HERE, 'selection.npz'), **out)


if __name__ == '__main__':
    main()
