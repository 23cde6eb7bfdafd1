#!/usr/bin/env python3
"""Generate tests/golden/multimodal.npz (multi-modal ground truth over a dataset: MMADE / MMFDE) on the CPU, with NumPy only
(the reference computes nothing like it):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_multimodal_golden.py

Stored per case <tag>: seeded float32 inputs pred [n, K, Tf, 2] / past [n, Tp, 2] / gt [n, Tf, 2], scale, eps, h (hist_frames), seg_ptr where
used, and in float64 on the coordinates (double)(x * scale) (the product in float32), written with array operations (all pairs of histories at
once, all neighbours, samples and frames of an agent at once), independently of the kernel's order of operations:

  count [n]            |S_i|: the agents of i's segment with d_hist(i, j) <= eps, and i itself
  mmade, mmfde [n]     the mean over S_i of min_k D_ade / D_fde(i, k, j) (a NaN distance counts as +inf)
  cmag                 the largest |coordinate| of the case (the magnitude in the tolerance of the GPU test)
  margin               the smallest |d_hist - eps| / eps over the pairs of a segment (eps > 0 only)

Histories are drawn from a few velocity prototypes plus noise, so that the neighbour sets are non-trivial.  The threshold decision is the only
discontinuity of the metric: a case with eps > 0 in which some pair of a segment has |d_hist - eps| < MARGIN * eps is drawn again from the
next seed (a condition on the inputs, seven orders of magnitude above the float64 rounding of a sum of 2h <= 400 terms; not a tolerance).

Cases are the smallest at which the kernel (one wave per agent, four agents per workgroup, j in tiles of TILE = 64, history components in
chunks of CHUNK = 8) can go wrong: n = 1, 63, 64, 65, 257 (a ragged last workgroup, five j tiles); K = 1, 3, 20, 64; Tf = 1, 12, 33;
(Tp, h) = (2, 1), (8, 3), (8, 4) (one whole chunk), (8, 7) (a chunk and a short one), (20, 19); eps = 0 with two agents that share one
history bit for bit; eps huge; a seg_ptr with segments of 1, 64, 65 and 64 agents, the third straddling workgroups and j tiles, at a moderate
and at a huge eps; a NaN sample, an agent whose samples are all NaN, a NaN in a history; scale 0.5 and 50; a ground truth 60 m away.
"""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TILE, CHUNK = 64, 8
MARGIN = 1e-9


def coords(x, scale):
    return (np.asarray(x, np.float32) * np.float32(scale)).astype(np.float64)


def draw(rng, n, K, Tp, Tf, protos, noise=0.05, spread=0.3):
    vel = rng.normal(0, 0.5, (protos, 2))
    turn = rng.normal(0, 0.04, (protos, 3, 2))                          # three ways on from every prototype: the futures are multi-modal
    p = rng.integers(0, protos, n)
    start = rng.uniform(-6, 6, (n, 1, 2))
    past = start + vel[p][:, None] * np.arange(-(Tp - 1), 1)[None, :, None] + rng.normal(0, noise, (n, Tp, 2))
    tf = np.arange(1, Tf + 1)[None, :, None]
    gt = past[:, -1:] + vel[p][:, None] * tf + turn[p, rng.integers(0, 3, n)][:, None] * tf ** 2 + rng.normal(0, noise, (n, Tf, 2))
    drift = rng.normal(0, spread, (n, K, 1, 2)) * np.linspace(0.3, 1.0, Tf)[None, None, :, None]
    pred = gt[:, None] + drift + rng.normal(0, 0.1 * spread, (n, K, Tf, 2))
    return pred.astype(np.float32), past.astype(np.float32), gt.astype(np.float32)


def hist_dist(past, scale, h):
    """a [n, 2], d_hist [n, n] in array form."""
    P = coords(past, scale)
    A = P[:, -1]
    H = (P[:, P.shape[1] - 1 - h:P.shape[1] - 1] - A[:, None]).reshape(len(P), 2 * h)
    with np.errstate(invalid='ignore'):
        return A, np.sqrt(((H[:, None] - H[None]) ** 2).sum(axis=-1))


def same_segment(n, seg_ptr):
    seg = np.zeros(n, np.int64) if seg_ptr is None else np.repeat(np.arange(len(seg_ptr) - 1), np.diff(seg_ptr))
    return seg[:, None] == seg[None]


def multimodal_np(pred, past, gt, scale, eps, h, seg_ptr=None):
    X, Y = coords(pred, scale), coords(gt, scale)
    n = len(X)
    A, Dh = hist_dist(past, scale, h)
    with np.errstate(invalid='ignore'):
        M = ((Dh <= eps) & same_segment(n, seg_ptr)) | np.eye(n, dtype=bool)
    count, mmade, mmfde = M.sum(axis=1).astype(np.int32), np.empty(n), np.empty(n)
    for i in range(n):
        js = np.nonzero(M[i])[0]
        G = (Y[js] - A[js][:, None]) + A[i]                           # [m, Tf, 2]
        D = np.linalg.norm(X[i][None] - G[:, None], axis=-1)          # [m, K, Tf]
        ade, fde = D.mean(axis=-1), D[..., -1]
        mmade[i] = np.where(np.isnan(ade), np.inf, ade).min(axis=1).mean()
        mmfde[i] = np.where(np.isnan(fde), np.inf, fde).min(axis=1).mean()
    return count, mmade, mmfde, Dh


def margin_of(Dh, eps, seg_ptr):
    """The smallest |d_hist - eps| / eps over the pairs i != j of a segment (NaN distances never match and are left out)."""
    n = len(Dh)
    pair = same_segment(n, seg_ptr) & ~np.eye(n, dtype=bool) & ~np.isnan(Dh)
    return float((np.abs(Dh[pair] - eps) / eps).min()) if pair.any() else np.inf


def main():
    out, tags = {}, []

    def add(tag, seed, n, K, Tp, h, Tf, scale, eps, protos=8, seg_ptr=None, edit=None):
        while True:
            rng = np.random.default_rng(seed)
            pred, past, gt = draw(rng, n, K, Tp, Tf, protos)
            if edit is not None:
                edit(pred, past, gt)
            sp = None if seg_ptr is None else np.asarray(seg_ptr, np.int32)
            count, mmade, mmfde, Dh = multimodal_np(pred, past, gt, scale, eps, h, sp)
            margin = margin_of(Dh, eps, sp) if eps > 0 else np.inf
            if margin >= MARGIN:
                break
            seed += 1000                                               # a pair on the threshold: another draw
        for k, v in (('pred', pred), ('past', past), ('gt', gt), ('scale', np.float64(scale)), ('eps', np.float64(eps)), ('h', np.int64(h)),
                     ('count', count), ('mmade', mmade), ('mmfde', mmfde), ('margin', np.float64(margin)),
                     ('cmag', np.float64(max(np.nanmax(np.abs(coords(a, scale))) for a in (pred, past, gt))))):
            out[tag + '/' + k] = v
        if sp is not None:
            out[tag + '/seg_ptr'] = sp
        tags.append(tag)
        fin = np.isfinite(mmade)
        print('%-12s seed %5d n=%3d K=%2d Tp=%2d h=%2d Tf=%2d scale=%4.1f eps=%8.3g  count %3d..%3d (mean %5.1f)  mmade %.4f  margin %.1e' % (
            tag, seed, n, K, Tp, h, Tf, scale, eps, count.min(), count.max(), count.mean(), mmade[fin].mean(), margin))

    def twins(pred, past, gt):
        past[40] = past[3]                                             # one history bit for bit (and one anchor); futures and samples differ

    def nans(pred, past, gt):
        pred[0, 3] = np.nan                                            # one whole sample
        pred[1] = np.nan                                               # every sample: +inf
        past[2, 4, 0] = np.nan                                         # a history frame: agent 2 keeps only itself, enters nobody's set
        pred[4, 0, 5, 1] = np.nan                                      # one coordinate of one sample

    def far(pred, past, gt):
        gt[::2] += 60.0

    SEG = [0, 1, 65, 130, 194]
    add('n1', 1, 1, 20, 8, 7, 12, 1.0, 0.3)
    add('n63_k1_t1', 2, 63, 1, 2, 1, 1, 1.0, 0.15, protos=6)
    add('n64_k3_h3', 3, 64, 3, 8, 3, 12, 0.5, 0.12, protos=6)
    add('n65_k20_h19', 4, 65, 20, 20, 19, 12, 1.0, 0.6, protos=6)
    add('n8_k64_t33', 5, 8, 64, 8, 7, 33, 1.0, 0.45, protos=2)
    add('n257_k3', 6, 257, 3, 8, 7, 12, 1.0, 0.4, protos=12)
    add('eps0_twins', 7, 65, 3, 8, 7, 12, 1.0, 0.0, edit=twins)
    add('huge_h4', 8, 65, 3, 8, 4, 12, 1.0, 1e6)
    add('seg', 9, 194, 3, 8, 7, 12, 1.0, 0.4, seg_ptr=SEG)
    add('seg_huge', 10, 194, 1, 8, 4, 12, 1.0, 1e6, seg_ptr=SEG)
    add('nan_k5', 11, 65, 5, 8, 7, 12, 1.0, 0.4, edit=nans)
    add('scale50', 12, 64, 3, 8, 7, 12, 50.0, 20.0)
    add('far', 13, 63, 3, 8, 7, 12, 1.0, 0.4, edit=far)
    out['cases'] = np.array(tags)
    out['tile'], out['chunk'], out['margin_required'] = np.int64(TILE), np.int64(CHUNK), np.float64(MARGIN)
    path = os.path.join(HERE, 'multimodal.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
