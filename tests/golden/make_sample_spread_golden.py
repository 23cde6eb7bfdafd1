#!/usr/bin/env python3
"""Generate tests/golden/sample_spread.npz (spread of the samples among themselves) on the CPU, with NumPy and the
REFERENCE's samplerloss.diversity_loss (imported, as make_selection_golden.py imports utils/metrics.py):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_sample_spread_golden.py

Stored per case <tag>: seeded float32 inputs pred [n, K, Tf, 2] / gt [n, Tf, 2], scale and div_scale, and in float64 on the coordinates
(double)(x * scale) (the product in float32):

  apd, fpd, pade, dlow [n]      the means over the K (K-1) / 2 pairs, written with array operations (np.linalg.norm over all pairs at once),
                                independently of the kernel's order of operations
  es_ade, es_fde [n]            (1/K) sum_k D(x_k, y) - ((K-1) / (2K)) pair mean; es_ade_mag / es_fde_mag: the two terms ADDED (the magnitude
                                the tolerance of the GPU test is taken of)
  es_ade_double, es_fde_double  the same score from the explicit 1/K^2 double sum over all ordered pairs (the diagonal included)
  ade_k, fde_k [n, K]           per-sample ADE / FDE in float64 (NaN where the sample has a NaN)
  ade_at_k, fde_at_k [n, K]     their running minima with NaN skipped; +inf while every sample so far is NaN
  dlow_ref                      the reference's diversity_loss(x, n, weight=1, scale=div_scale)[1] in float64 (its loss_unweighted)

The restatement of dlow is asserted here to agree with the reference's function to 1e-12 relative.

Cases are the smallest at which the kernel (one workgroup per agent, pair p on thread p mod 256, frames in LDS tiles of TILE = 32) can go
wrong: K = 2 (one pair), 3, 23 (253 pairs: just under one per thread), 24 (276: just over), 64 (2016: eight rounds, the last ragged);
Tf = 1 (d_traj == d_fde == Tf d_ade), TILE - 1, TILE, TILE + 1, 40 at K = 64; n = 1, 5, 70; scale 1, 0.5, 50; duplicated samples (distance
zero, DLow term 1); NaN samples (the prefix minima); a ground truth 60 m away.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get('STTODE_REFERENCE', '/root/reference')
TILE = 32


def reference_diversity_loss():
    if REF not in sys.path:
        sys.path.insert(0, REF)
    from samplerloss import diversity_loss
    return diversity_loss


def draw(rng, n, K, Tf, spread):
    start, vel = rng.uniform(-6, 6, (n, 1, 2)), rng.normal(0, 0.4, (n, 1, 2))
    gt = start + vel * np.arange(1, Tf + 1)[None, :, None]
    drift = rng.normal(0, spread, (n, K, 1, 2)) * np.linspace(0.3, 1.0, Tf)[None, None, :, None]
    pred = gt[:, None] + drift + rng.normal(0, 0.1 * spread, (n, K, Tf, 2))
    return pred.astype(np.float32), gt.astype(np.float32)


def coords(x, scale):
    return (np.asarray(x, np.float32) * np.float32(scale)).astype(np.float64)


def spread_np(pred, gt, scale, div_scale):
    X, Y = coords(pred, scale), coords(gt, scale)
    n, K, Tf = X.shape[:3]
    iu = np.triu_indices(K, 1)                                        # F.pdist order
    D = np.linalg.norm(X[:, :, None] - X[:, None], axis=-1)           # [n, K, K, Tf]
    d_traj2 = (D ** 2).sum(axis=-1)
    d_ade, d_fde = D.mean(axis=-1), D[..., -1]
    out = {'apd': np.sqrt(d_traj2)[:, iu[0], iu[1]].mean(axis=1), 'fpd': d_fde[:, iu[0], iu[1]].mean(axis=1),
           'pade': d_ade[:, iu[0], iu[1]].mean(axis=1), 'dlow': np.exp(-d_traj2 / div_scale)[:, iu[0], iu[1]].mean(axis=1)}
    G = np.linalg.norm(X - Y[:, None], axis=-1)                       # [n, K, Tf]
    c = (K - 1) / (2.0 * K)
    for name, per, pair, full in (('ade', G.mean(axis=-1), out['pade'], d_ade), ('fde', G[..., -1], out['fpd'], d_fde)):
        A = per.mean(axis=1)
        out['es_' + name], out['es_' + name + '_mag'] = A - c * pair, A + c * pair
        out['es_' + name + '_double'] = A - 0.5 * full.sum(axis=(1, 2)) / (K * K)
        out[name + '_k'] = per
        run = np.fmin.accumulate(per, axis=1)
        out[name + '_at_k'] = np.where(np.isnan(run), np.inf, run)
    return out


def main():
    rng = np.random.default_rng(20261018)
    diversity_loss = reference_diversity_loss()
    import torch
    out, tags = {}, []

    def add(tag, n, K, Tf, scale, div_scale, spread=0.3, edit=None):
        pred, gt = draw(rng, n, K, Tf, spread)
        if edit is not None:
            edit(pred, gt)
        res = spread_np(pred, gt, scale, div_scale)
        with torch.no_grad():
            ref = float(diversity_loss(torch.from_numpy(coords(pred, scale)), n, 1, div_scale)[1])
        mine = res['dlow'].sum() / n
        assert (np.isnan(ref) and np.isnan(mine)) or abs(mine - ref) <= 1e-12 * abs(ref), (tag, mine, ref)
        out[tag + '/pred'], out[tag + '/gt'] = pred, gt
        out[tag + '/scale'], out[tag + '/div_scale'], out[tag + '/dlow_ref'] = np.float64(scale), np.float64(div_scale), np.float64(ref)
        for k, v in res.items():
            out[tag + '/' + k] = v
        tags.append(tag)
        print('%-14s n=%2d K=%2d Tf=%2d scale=%4.1f div=%5.1f  apd %.4f  dlow %.3e (ref rel diff %.1e)  es_ade %.4f' % (
            tag, n, K, Tf, scale, div_scale, np.nanmean(res['apd']), mine, 0.0 if np.isnan(ref) else abs(mine - ref) / abs(ref),
            np.nanmean(res['es_ade'])))

    def duplicates(pred, gt):
        pred[:, 1] = pred[:, 0]                                        # distance zero, DLow term 1
        pred[0, :] = pred[0, :1]                                       # every sample of agent 0 the same: apd 0, dlow 1

    def far(pred, gt):
        gt[::2] += 60.0

    def nans(pred, gt):
        pred[0, 3] = np.nan                                            # one whole sample
        pred[1, 0, 5, 1] = np.nan                                      # the first sample, one coordinate: the k = 1 prefix has no value
        pred[2, :2] = np.nan                                           # the first two samples
        pred[3] = np.nan                                               # every sample

    add('k2_t1', 3, 2, 1, 1.0, 1.0)
    add('k2_t12', 5, 2, 12, 1.0, 1.0)
    add('k3_t1', 5, 3, 1, 0.5, 0.5, spread=1.0)
    add('k23_t31', 5, 23, TILE - 1, 1.0, 2.0, spread=0.1)
    add('k24_t32', 5, 24, TILE, 50.0, 2000.0, spread=0.02)
    add('k20_t33', 5, 20, TILE + 1, 1.0, 10.0, spread=0.2)
    add('k64_t40', 2, 64, 40, 0.5, 10.0, spread=0.5)
    add('k64_t1', 1, 64, 1, 1.0, 1.0, spread=1.0)
    add('k7_t3_n70', 70, 7, 3, 1.0, 1.0)
    add('dup_k20_t12', 5, 20, 12, 1.0, 1.0, edit=duplicates)
    add('far_k20_t12', 5, 20, 12, 1.0, 1.0, edit=far)
    add('nan_k20_t12', 5, 20, 12, 1.0, 1.0, edit=nans)
    out['cases'] = np.array(tags)
    out['tile'] = np.int64(TILE)
    path = os.path.join(HERE, 'sample_spread.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
