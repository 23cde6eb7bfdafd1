#!/usr/bin/env python3
"""Generate tests/golden/weighted_set.npz (weighted sample sets) with NumPy and scipy.stats.gaussian_kde(weights=):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_weighted_set_golden.py

Stored per case <tag>: seeded inputs pred [n, K, Tf, 2] / weights [n, K] / gt [n, Tf, 2] (float32), scale, and the expected outputs in
float64, computed here independently of the kernel's order of operations:

- eade / efde, es_ade / es_fde, apd / fpd, neff: array form, the pair terms as the full K x K double sum (the diagonal is zero) over the
  positive-weight samples; es_*_mag = the sum of the magnitudes of the two terms of the energy scores.
- ade_k / fde_k [n, K] (float64 per-sample errors, +inf at zero weight), ade_top / fde_top [n, K]: a stable sort by descending weight and
  np.minimum.accumulate; brier_ade / brier_fde from np.argmin.  Outside deliberate duplicates the best and the second-best ADE_k / FDE_k of
  every agent differ by more than 1e-5 relative (asserted), so k* is the same for any evaluation.
- kde_nll: Trajectron++'s compute_kde_nll through gaussian_kde(dataset, weights=w) over the positive-weight samples.  NaN where the
  contract says so: fewer than three positive weights (not asked of scipy: two points are collinear and its Cholesky passes or fails on
  rounding) or a frame whose weighted covariance, summed in sample order, has C00 <= 0 or det C <= 0 -- the maker asserts that gaussian_kde
  raises exactly there, that every other frame has det C >= 1e-3 C00 C11, and that tests/weighted_ref.py agrees with scipy to 1e-8.
- A row with a negative, NaN or infinite weight, or with all weights zero: NaN everywhere.

Cases: K 1 / 3 / 6 / 20 / 23 / 24 / 64, Tf 1 / 12 / 33 / 40, n 1 / 5 / 37; integer counts with zeros, equal weights, one dominant weight,
exact ties among non-adjacent samples, one and two positive weights, all-zero / negative / NaN / infinite rows; ground truth 60 m from every
sample at two frames (the -20 clip); frames whose positive-weight samples are all at the origin or all on the x axis, built from zeros.
"""
import os
import sys

import numpy as np
from scipy.stats import gaussian_kde

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from weighted_ref import coords, weighted_set_np  # noqa: E402

F64 = ('eade', 'efde', 'es_ade', 'es_fde', 'apd', 'fpd', 'kde_nll', 'brier_ade', 'brier_fde', 'neff')


def draw(rng, n, K, Tf, spread):
    start, vel = rng.uniform(-6, 6, (n, 1, 2)), rng.normal(0, 0.4, (n, 1, 2))
    gt = start + vel * np.arange(1, Tf + 1)[None, :, None]
    drift = rng.normal(0, spread, (n, K, 1, 2)) * np.linspace(0.3, 1.0, Tf)[None, None, :, None]
    pred = gt[:, None] + drift + rng.normal(0, 0.1 * spread, (n, K, Tf, 2))
    return pred.astype(np.float32), gt.astype(np.float32)


def bad_row(w):
    return bool((w < 0).any() or not np.isfinite(w).all() or not w.astype(np.float64).sum() > 0)


def weighted_cov(x, p):
    """The contract's covariance of x [P, 2] under p [P] (sum 1 over the whole row), sums in sample order: (c00, c01, c11)."""
    s2 = 0.0
    for v in p:
        s2 += v * v
    m = np.zeros(2)
    for k in range(len(p)):
        m += p[k] * x[k]
    c = np.zeros(3)
    for k in range(len(p)):
        d = x[k] - m
        c += p[k] * np.array((d[0] * d[0], d[0] * d[1], d[1] * d[1]))
    return c / (1.0 - s2)


def kde(X, Y, w, degenerate):
    """kde_nll [n] through scipy; `degenerate` [n, Tf] marks the frames built singular."""
    n, K, Tf = X.shape[:3]
    out = np.full(n, np.nan)
    for a in range(n):
        if bad_row(w[a]):
            continue
        pos = w[a] > 0
        if pos.sum() < 3:
            continue                                                   # NaN by contract, not by scipy
        p = (w[a].astype(np.float64) / w[a].astype(np.float64).sum())[pos]
        ll, nan = 0.0, False
        for t in range(Tf):
            c = weighted_cov(X[a, pos, t], p)
            det = c[0] * c[2] - c[1] * c[1]
            sing = not c[0] > 0.0 or not det > 0.0
            assert sing == bool(degenerate[a, t]), (a, t, c)
            if not sing:
                assert det >= 1e-3 * c[0] * c[2], (a, t, det, c)
            try:
                k = gaussian_kde(X[a, pos, t].T, weights=w[a, pos].astype(np.float64))
                ll += np.clip(k.logpdf(Y[a, t]), a_min=-20, a_max=None)[0] / Tf
                assert not sing, (a, t)
            except np.linalg.LinAlgError:
                assert sing, (a, t)                                    # gaussian_kde raises exactly where the contract says NaN
                nan = True
        out[a] = np.nan if nan else -ll
    return out


def expected(pred, w, gt, scale, dup_ok):
    X, Y = coords(pred, scale), coords(gt, scale)
    n, K, Tf = X.shape[:3]
    out = {k: np.full(n, np.nan) for k in F64 + ('es_ade_mag', 'es_fde_mag')}
    for k in ('ade_k', 'fde_k', 'ade_top', 'fde_top'):
        out[k] = np.full((n, K), np.nan)
    for a in range(n):
        if bad_row(w[a]):
            continue
        wa = w[a].astype(np.float64)
        p = wa / wa.sum()
        pos = wa > 0
        s2 = (p * p).sum()
        G = np.linalg.norm(X[a] - Y[a][None], axis=-1)                  # [K, Tf]
        D = np.linalg.norm(X[a][:, None] - X[a][None], axis=-1)         # [K, K, Tf]
        pp = np.where(np.outer(pos, pos), np.outer(p, p), 0.0)
        ade, fde = np.where(pos, G.mean(axis=1), np.inf), np.where(pos, G[:, -1], np.inf)
        pa = 0.5 * np.where(pp > 0, pp * D.mean(axis=2), 0.0).sum()
        pf = 0.5 * np.where(pp > 0, pp * D[..., -1], 0.0).sum()
        pt = 0.5 * np.where(pp > 0, pp * np.sqrt((D * D).sum(axis=2)), 0.0).sum()
        out['eade'][a], out['efde'][a] = (p[pos] * ade[pos]).sum(), (p[pos] * fde[pos]).sum()
        out['es_ade'][a], out['es_fde'][a] = out['eade'][a] - pa, out['efde'][a] - pf
        out['es_ade_mag'][a], out['es_fde_mag'][a] = out['eade'][a] + pa, out['efde'][a] + pf
        if pos.sum() > 1:
            out['apd'][a], out['fpd'][a] = 2.0 * pt / (1.0 - s2), 2.0 * pf / (1.0 - s2)
        out['neff'][a] = 1.0 / s2
        order = np.argsort(-wa, kind='stable')                         # descending weight, ties to the lower index, zeros last
        out['ade_k'][a], out['fde_k'][a] = ade, fde
        out['ade_top'][a], out['fde_top'][a] = np.minimum.accumulate(ade[order]), np.minimum.accumulate(fde[order])
        for name, v in (('ade', ade), ('fde', fde)):
            ks = int(np.argmin(v))
            s = np.sort(v[pos])
            if len(s) > 1 and not dup_ok:
                assert (s[1] - s[0]) > 1e-5 * s[1], (a, name, s[:2])  # k* is unambiguous
            out['brier_' + name][a] = v[ks] + (1.0 - p[ks]) ** 2
    return out


def main():
    rng = np.random.default_rng(20261021)
    out, cases = {}, []

    def counts(n, K, M):
        """Cluster sizes of M draws over K clusters with uneven shares: integers, several of them zero."""
        share = rng.dirichlet(np.full(K, 0.4), n)
        return np.stack([rng.multinomial(M, s) for s in share]).astype(np.float32)

    def far_and_degenerate(pred, gt, w, deg):
        n, K, Tf = pred.shape[:3]
        for a in range(0, n, 5):                                       # ground truth 60 m from every sample at two frames: the clip
            gt[a, [0, Tf - 1]] += 60.0
        for a in range(3, n, 11):                                      # every sample at the origin at one frame
            pred[a, :, Tf // 2] = 0.0
            deg[a, Tf // 2] = True
        for a in range(7, n, 13):                                      # every sample on the x axis at one frame
            pred[a, :, Tf // 3, 1] = 0.0
            deg[a, Tf // 3] = True

    def add(tag, n, K, Tf, scale, w, spread=3.0, edit=None, dup_ok=False):
        pred, gt = draw(rng, n, K, Tf, spread)
        deg = np.zeros((n, Tf), bool)
        if edit is not None:
            edit(pred, gt, w, deg)
        cases.append((tag, pred, np.asarray(w, np.float32), gt, scale, deg, dup_ok))

    def at_least(w, k):
        """Rows with fewer than k positive counts get ones in their first k slots (a KDE row needs three points)."""
        for row in w:
            if (row > 0).sum() < k:
                row[:k] = np.maximum(row[:k], 1.0)
        return w

    add('counts_k20_t12', 37, 20, 12, 1.0, at_least(counts(37, 20, 40), 3), edit=far_and_degenerate)
    add('one_k20_t12', 1, 20, 12, 1.3, at_least(counts(1, 20, 40), 3))
    add('equal_k20_t12', 5, 20, 12, 1.0, np.full((5, 20), 2.0, np.float32))
    dom = np.ones((5, 6), np.float32)
    dom[np.arange(5), [4, 0, 5, 2, 3]] = [50.0, 9.0, 120.0, 33.0, 1000.0]
    add('dominant_k6_t12', 5, 6, 12, 1.5, dom, spread=2.0)
    ties = counts(5, 23, 60) + 1.0
    ties[:, [2, 9, 17]] = 4.0                                          # exact ties among non-adjacent samples
    ties[:, [0, 22]] = 7.0
    add('ties_k23_t33', 5, 23, 33, 1.0, ties, edit=far_and_degenerate)
    add('counts_k24_t12', 5, 24, 12, 0.5, at_least(counts(5, 24, 48), 3))
    add('counts_k64_t40', 5, 64, 40, 1.0, at_least(counts(5, 64, 128), 3), spread=4.0, edit=far_and_degenerate)
    add('k1_t12', 5, 1, 12, 1.0, np.array([[1.0], [0.25], [40.0], [3.0], [1e-3]], np.float32))
    add('k3_t1', 5, 3, 1, 1.0, np.array([[1, 1, 1], [5, 2, 9], [3, 3, 1], [1, 20, 2], [2, 7, 7]], np.float32))

    def special(K):
        w = counts(10, K, 2 * K) + 1.0
        w[0] = 0.0
        w[0, K - 2] = 5.0                                              # exactly one positive weight
        w[1] = 0.0
        w[1, [1, K - 1]] = [3.0, 2.0]                                  # exactly two positive weights
        w[2] = 0.0                                                     # all zero
        w[3, 2] = -1.0                                                 # a negative weight
        w[4, K - 1] = np.nan
        w[5, 0] = np.inf
        w[6] = 0.0
        w[6, [0, 2, K - 1]] = [1.0, 1.0, 6.0]                          # three positive weights: the smallest set with a KDE
        return w                                                       # rows 7 .. 9: ordinary
    add('special_k6_t12', 10, 6, 12, 1.0, special(6))
    add('special_k24_t33', 10, 24, 33, 2.0, special(24))

    def duplicate(pred, gt, w, deg):                                   # the best sample twice: the first index wins the Brier term
        pred[:, 4] = gt + 0.05
        pred[:, 11] = pred[:, 4]
    add('dup_k20_t12', 5, 20, 12, 1.0, counts(5, 20, 40) + 1.0, edit=duplicate, dup_ok=True)

    for tag, pred, w, gt, scale, deg, dup_ok in cases:
        e = expected(pred, w, gt, scale, dup_ok)
        e['kde_nll'] = kde(coords(pred, scale), coords(gt, scale), w, deg)
        r = weighted_set_np(pred, w, gt, scale)
        assert np.array_equal(np.isnan(r['kde_nll']), np.isnan(e['kde_nll'])), tag
        ok = ~np.isnan(e['kde_nll'])
        worst = float(np.abs(r['kde_nll'][ok] - e['kde_nll'][ok]).max()) if ok.any() else 0.0
        assert worst <= 1e-8, (tag, worst)
        out[tag + '/pred'], out[tag + '/weights'], out[tag + '/gt'] = pred, w, gt
        out[tag + '/scale'], out[tag + '/degenerate'] = np.float64(scale), deg
        for k, v in e.items():
            out[tag + '/' + k] = v
        print('%-18s n=%2d K=%2d Tf=%2d  kde NaN %2d / %2d, clipped frames present %s, restatement vs scipy %.1e' % (
            tag, pred.shape[0], pred.shape[1], pred.shape[2], np.isnan(e['kde_nll']).sum(), pred.shape[0], bool((gt > 40).any()), worst))
    out['cases'] = np.array([c[0] for c in cases])
    out['tile'] = np.int64(32)
    np.savez_compressed(os.path.join(HERE, 'weighted_set.npz'), **out)


if __name__ == '__main__':
    main()
