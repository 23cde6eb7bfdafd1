#!/usr/bin/env python3
"""Generate tests/golden/scene_metrics.npz (joint best-of-K, collisions, KDE NLL) with NumPy and scipy.stats.gaussian_kde:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_scene_metrics_golden.py

Stored per case <tag>: seeded inputs pred [n, K, Tf, 2] / gt [n, Tf, 2] (float32), a ragged segment CSR seg_ptr [S+1], scale and collision
radius, and the expected outputs: seg_jade / seg_jfde [S] (float64 here), seg_jade_idx / seg_jfde_idx [S], seg_col / seg_gt_col [S], and
kde_nll [n] (float64).  The values are computed here independently of the kernels' order of operations:

- joint: per-(agent, sample) displacements in float64 (np.linalg.norm), the mean over the segment's agents, np.argmin over k.  Apart from
  the deliberate ties (duplicated samples: exactly equal values), the best and second-best joint value of every segment differ by more than
  1e-5 relative, so the index of any evaluation is this one.
- collisions: every pair of the segment's agents per sample and frame, in float32 on the scaled coordinates, strictly below radius^2.  The
  radius of a case is chosen so that no squared distance lies within 1e-3 relative of radius^2 (lattice cases: integer squared distances).
- KDE NLL: Trajectron++'s compute_kde_nll, agent by agent and frame by frame, through scipy.stats.gaussian_kde on float64 data
  (float32 pred * scale, converted).  An agent is NaN where gaussian_kde raises LinAlgError -- the degenerate frames below are built from
  zeros so that its covariance is exactly singular -- and, for K = 2 (two points always lie on a line), wherever the covariance of the
  contract (unbiased, summed in sample order) has det <= 0: scipy's Cholesky factorisation of such a matrix passes or fails on rounding.

Cases: ragged segments with 1-agent segments, one segment of 720 agents, K = 2 / 6 / 20 / 64, Tf = 1 / 12 / 40, duplicated samples for exact
joint ties, ground-truth points 60 m away from every sample (the -20 clip), exactly degenerate frames (all samples at the origin; all samples
on the x axis) and lattice positions.
"""
import os

import numpy as np
from scipy.stats import gaussian_kde

HERE = os.path.dirname(os.path.abspath(__file__))


def ragged_ptr(rng, sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)


def draw(rng, n, K, Tf, spread, lattice=False):
    if lattice:
        start = rng.integers(0, 400, (n, 1, 2)).astype(np.float64)
        vel = rng.integers(-1, 2, (n, 1, 2)).astype(np.float64)
        gt = start + vel * np.arange(1, Tf + 1)[None, :, None]
        pred = gt[:, None] + rng.integers(-3, 4, (n, K, Tf, 2))
        return pred.astype(np.float32), gt.astype(np.float32)
    start, vel = rng.uniform(-6, 6, (n, 1, 2)), rng.normal(0, 0.4, (n, 1, 2))
    gt = start + vel * np.arange(1, Tf + 1)[None, :, None]
    drift = rng.normal(0, spread, (n, K, 1, 2)) * np.linspace(0.3, 1.0, Tf)[None, None, :, None]
    pred = gt[:, None] + drift + rng.normal(0, 0.1 * spread, (n, K, Tf, 2))
    return pred.astype(np.float32), gt.astype(np.float32)


def per_sample(pred, gt, scale):
    d = np.linalg.norm((pred.astype(np.float64) - gt[:, None].astype(np.float64)) * scale, axis=-1)   # [n, K, Tf]
    return d.mean(axis=-1), d[..., -1]


def joint(pred, gt, sp, scale):
    ade, fde = per_sample(pred, gt, scale)
    out = {k: [] for k in ('seg_jade', 'seg_jfde', 'seg_jade_idx', 'seg_jfde_idx')}
    for a0, a1 in zip(sp[:-1], sp[1:]):
        for v, name in ((ade, 'jade'), (fde, 'jfde')):
            m = v[a0:a1].mean(axis=0)
            out['seg_' + name + '_idx'].append(int(np.argmin(m)))
            out['seg_' + name].append(float(m.min()))
    return {k: np.array(v) for k, v in out.items()}


def joint_gaps(pred, gt, sp, scale):
    """Per segment the relative gap between the best and the second-best joint ADE and FDE (the smaller of the two)."""
    ade, fde = per_sample(pred, gt, scale)
    gaps = []
    for a0, a1 in zip(sp[:-1], sp[1:]):
        g = np.inf
        for v in (ade, fde):
            m = np.sort(v[a0:a1].mean(axis=0))
            if len(m) > 1:
                g = min(g, (m[1] - m[0]) / max(m[1], 1e-30))
        gaps.append(g)
    return np.array(gaps)


def seg_d2(pos, a0, a1):
    """Squared distances [na, na, ...] between the agents of one segment, float32, pos [n, ..., 2] already scaled."""
    q = pos[a0:a1]
    d = q[:, None] - q[None]
    return d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]


def collisions(pred, gt, sp, scale, r):
    P, G = pred * np.float32(scale), gt * np.float32(scale)
    r2 = np.float32(r) * np.float32(r)
    col, gcol = [], []
    for a0, a1 in zip(sp[:-1], sp[1:]):
        na = a1 - a0
        off = ~np.eye(na, dtype=bool)
        c = 0
        for k in range(P.shape[1]):
            d2 = seg_d2(P[:, k], a0, a1)                           # [na, na, Tf]
            c += int(((d2 < r2).any(axis=-1) & off).any(axis=1).sum())
        d2 = seg_d2(G, a0, a1)
        col.append(c)
        gcol.append(int(((d2 < r2).any(axis=-1) & off).any(axis=1).sum()))
    return np.array(col), np.array(gcol)


def radius_margin(pred, gt, sp, scale, r):
    """Smallest |d^2 - r^2| / r^2 over every pair, sample and frame."""
    P, G = pred * np.float32(scale), gt * np.float32(scale)
    r2 = float(r) ** 2
    worst = np.inf
    for a0, a1 in zip(sp[:-1], sp[1:]):
        if a1 - a0 < 2:
            continue
        for k in range(P.shape[1]):
            worst = min(worst, float(np.abs(seg_d2(P[:, k], a0, a1).astype(np.float64) - r2).min()) / r2)
        worst = min(worst, float(np.abs(seg_d2(G, a0, a1).astype(np.float64) - r2).min()) / r2)
    return worst


def contract_singular(X):
    """X [K, 2] float64: C00 <= 0 or det C <= 0 for the unbiased covariance summed in sample order (the kernels' test)."""
    K = X.shape[0]
    m = np.zeros(2)
    for k in range(K):
        m += X[k]
    m /= K
    c = np.zeros(3)
    for k in range(K):
        d = X[k] - m
        c += (d[0] * d[0], d[0] * d[1], d[1] * d[1])
    c /= (K - 1)
    return not (c[0] > 0.0) or not (c[0] * c[2] - c[1] * c[1] > 0.0)


def compute_kde_nll(predicted_trajs, gt_traj):
    """Trajectron++ (evaluation/evaluation.py compute_kde_nll): predicted_trajs [1, K, Tf, 2], gt_traj [Tf, 2]."""
    kde_ll = 0.
    log_pdf_lower_bound = -20
    num_timesteps = gt_traj.shape[0]
    num_batches = predicted_trajs.shape[0]
    for batch_num in range(num_batches):
        for timestep in range(num_timesteps):
            try:
                kde = gaussian_kde(predicted_trajs[batch_num, :, timestep].T)
                pdf = np.clip(kde.logpdf(gt_traj[timestep].T), a_min=log_pdf_lower_bound, a_max=None)[0]
                kde_ll += pdf / (num_timesteps * num_batches)
            except np.linalg.LinAlgError:
                kde_ll = np.nan
    return -kde_ll


def kde(pred, gt, scale):
    X = (pred * np.float32(scale)).astype(np.float64)
    G = (gt * np.float32(scale)).astype(np.float64)
    n, K, Tf = pred.shape[:3]
    out = np.empty(n)
    for a in range(n):
        sing = any(contract_singular(X[a, :, t]) for t in range(Tf))
        v = compute_kde_nll(X[a][None], G[a])
        if K > 2:
            assert np.isnan(v) == sing, (a, v, sing)   # the zero-built degenerate frames make gaussian_kde raise; nothing else does
        out[a] = np.nan if sing else v
    return out


def main():
    rng = np.random.default_rng(20261016)
    out = {}
    cases = []

    def add(tag, sizes, K, Tf, scale, spread=3.0, lattice=False, radius=None, edit=None, ties=False):
        sp = ragged_ptr(rng, sizes)
        n = int(sp[-1])
        pred, gt = draw(rng, n, K, Tf, spread, lattice)
        if edit is not None:
            edit(pred, gt, sp)
        if not ties and not lattice:                                   # separate near-ties of the joint values
            for _ in range(50):
                bad = np.nonzero(joint_gaps(pred, gt, sp, scale) <= 1e-5)[0]
                if not len(bad):
                    break
                for s in bad:
                    pred[sp[s]:sp[s + 1]] += rng.normal(0, 0.02, pred[sp[s]:sp[s + 1]].shape).astype(np.float32)
        if not ties:
            assert (joint_gaps(pred, gt, sp, scale) > 1e-5).all(), tag
        if radius is None:                                             # the first radius well away from every squared distance
            radius = next(r for r in (0.75, 0.6, 0.9, 0.5, 1.1, 0.4) if radius_margin(pred, gt, sp, scale, r) > 1e-3)
        assert radius_margin(pred, gt, sp, scale, radius) > 1e-3, tag
        cases.append((tag, sp, pred, gt, scale, radius))

    def far_and_degenerate(pred, gt, sp):
        n, K, Tf = pred.shape[:3]
        for a in range(0, n, 5):                                       # ground truth 60 m from every sample at two frames: the clip
            gt[a, [0, Tf - 1]] += 60.0
        for a in range(3, n, 11):                                      # every sample at the origin at one frame
            pred[a, :, Tf // 2] = 0.0
        for a in range(7, n, 13):                                      # every sample on the x axis at one frame
            pred[a, :, Tf // 3, 1] = 0.0

    add('k20_t12', [1, 1, 9, 4, 16, 1, 12, 7, 3, 20, 2, 5], 20, 12, 1.0, edit=far_and_degenerate)
    add('k6_t12', [1, 3, 6, 2, 5, 1, 4, 6, 2, 3, 5, 1, 6, 4], 6, 12, 1.5, spread=2.0, edit=far_and_degenerate)
    add('k64_t40', [1, 5, 8, 3], 64, 40, 1.0, spread=4.0, edit=far_and_degenerate)
    add('k20_t1', [1, 7, 3, 10, 1, 5, 2, 8], 20, 1, 1.0, edit=far_and_degenerate)

    def dyadic(pred, gt, sp):                                          # K = 2: exactly representable sums, det C == 0 exactly
        pred[:] = np.round(pred * 4) / 4
        gt[:] = np.round(gt * 4) / 4
    add('k2_t12', [1, 4, 6, 2, 3, 5], 2, 12, 1.0, edit=dyadic, radius=0.7)
    add('lattice_big_k20_t12', [1, 720, 5], 20, 12, 1.0, lattice=True, radius=1.2)

    def ties(pred, gt, sp):                                            # per segment the best sample duplicated into two later slots
        K = pred.shape[1]
        for s in range(len(sp) - 1):
            a0, a1 = sp[s], sp[s + 1]
            k0 = int(rng.integers(0, K - 2))
            pred[a0:a1, k0] = gt[a0:a1] + rng.normal(0, 0.2, (a1 - a0,) + gt.shape[1:]).astype(np.float32)
            for k in rng.choice(np.arange(k0 + 1, K), 2, replace=False):
                pred[a0:a1, k] = pred[a0:a1, k0]
        a0, a1 = sp[2], sp[3]                                          # one segment: every sample of every agent the same -> index 0
        pred[a0:a1] = 0.0
    add('ties_k20_t12', [1, 6, 4, 9, 2, 7], 20, 12, 1.0, edit=ties, ties=True)

    for tag, sp, pred, gt, scale, radius in cases:
        j = joint(pred, gt, sp, scale)
        col, gcol = collisions(pred, gt, sp, scale, radius)
        nll = kde(pred, gt, scale)
        out[tag + '/pred'], out[tag + '/gt'], out[tag + '/seg_ptr'] = pred, gt, sp
        out[tag + '/scale'], out[tag + '/radius'] = np.float64(scale), np.float64(radius)
        for k, v in j.items():
            out[tag + '/' + k] = v
        out[tag + '/seg_col'], out[tag + '/seg_gt_col'], out[tag + '/kde_nll'] = col, gcol, nll
        print('%-22s n=%4d S=%2d K=%2d Tf=%2d r=%.2f  colliding agent-samples %5d / %5d, gt %3d / %3d, kde NaN %3d' % (
            tag, pred.shape[0], len(sp) - 1, pred.shape[1], pred.shape[2], radius, col.sum(), pred.shape[0] * pred.shape[1], gcol.sum(),
            pred.shape[0], np.isnan(nll).sum()))
    out['cases'] = np.array([c[0] for c in cases])
    np.savez_compressed(os.path.join(HERE, 'scene_metrics.npz'), **out)


if __name__ == '__main__':
    main()
