"""NumPy restatement of sttode_weighted_set (include/sttode_hip.h), in the contract's order: weights summed in sample order,
frames in frame order, pairs in F.pdist order dealt to 256 threads (pair q on thread q mod 256, a thread's pairs in pair order), the
partials of lane l, l + 64, l + 128, l + 192 added in that order and the 64 lanes by the xor tree; the KDE frames in tiles of 32 through
the same tree, tiles in order.  The loops over frames, samples and rounds are explicit; what is independent (the pairs of one frame, the
frames of one tile) is an array.  ``ade_k`` / ``fde_k`` restate bok_dist in float32 (a fused multiply-add, rounded once).

``uniform_spread_np`` restates DESIGN.md 4s's formulas (the pair means and the energy scores of sttode_sample_spread) for the identities at
equal weights."""
import numpy as np

F64 = ('eade', 'efde', 'es_ade', 'es_fde', 'apd', 'fpd', 'kde_nll', 'brier_ade', 'brier_fde', 'neff')
TILE = 32
_LANES = np.arange(64)


def coords(x, scale):
    return (np.asarray(x, np.float32) * np.float32(scale)).astype(np.float64)


def xor_tree(v):
    """The sum of 64 lane values as `for o in 32, 16, ... 1: v += shfl_xor(v, o)` leaves it in lane 0."""
    v = np.array(v, np.float64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[_LANES ^ o]
    return v[0]


def fma_f32(a, b, c):
    """float32 fma(a, b, c) for c >= 0 and a b >= 0, rounded once: the exact product and sum in float64, rounded to odd, then to float32."""
    x = a.astype(np.float64) * b.astype(np.float64)                    # exact: 48 bits
    y = c.astype(np.float64)
    s = x + y
    bb = s - x
    e = (x - (s - bb)) + (y - bb)                                      # TwoSum: x + y == s + e exactly
    t = np.where(e < 0, np.nextafter(s, 0.0), s)
    bits = t.view(np.int64) | (e != 0)
    return bits.view(np.float64).astype(np.float32)


def bok_f32(pred_a, gt_a, scale):
    """(ADE_k, FDE_k) [K] float32 of one agent as bok_select_kernel computes them; pred_a [K, Tf, 2], gt_a [Tf, 2] float32."""
    s = np.float32(scale)
    K, Tf = pred_a.shape[:2]
    fa = np.zeros(K, np.float32)
    fl = np.zeros(K, np.float32)
    with np.errstate(invalid='ignore'):
        for t in range(Tf):
            dx = (pred_a[:, t, 0] - gt_a[t, 0]) * s
            dy = (pred_a[:, t, 1] - gt_a[t, 1]) * s
            ok = ~(np.isnan(dx) | np.isnan(dy))
            fl = np.full(K, np.nan, np.float32)
            fl[ok] = np.sqrt(fma_f32(dx[ok], dx[ok], dy[ok] * dy[ok]))
            fa = (fa + fl).astype(np.float32)
    return (fa / np.float32(Tf)).astype(np.float32), fl


def pair_index(K):
    return [(i, j) for i in range(K) for j in range(i + 1, K)]


def agent_np(pred_a, w_a, gt_a, scale):
    """One agent: a dict of the ten float64 values, 'ade_top' / 'fde_top' [K] float32, and 'es_ade_mag' / 'es_fde_mag' (the sum of the
    magnitudes of the two terms of the energy scores)."""
    K, Tf = pred_a.shape[:2]
    w32 = np.asarray(w_a, np.float32)
    out = {k: np.nan for k in F64 + ('es_ade_mag', 'es_fde_mag')}
    out['ade_top'] = np.full(K, np.nan, np.float32)
    out['fde_top'] = np.full(K, np.nan, np.float32)
    W = 0.0
    for k in range(K):
        W += float(w32[k])
    if (w32 < 0).any() or not np.isfinite(w32).all() or not W > 0.0:
        return out
    p = w32.astype(np.float64) / W
    s2 = 0.0
    for k in range(K):
        s2 += p[k] * p[k]
    om = 1.0 - s2
    pos = w32 > 0
    X, Y = coords(pred_a, scale), coords(gt_a, scale)
    # pairs
    pairs = pair_index(K)
    terms = np.zeros((3, 256 * max(1, -(-len(pairs) // 256))))
    live = [q for q, (i, j) in enumerate(pairs) if p[i] * p[j] != 0.0]
    if live:
        I, J = np.array([pairs[q][0] for q in live]), np.array([pairs[q][1] for q in live])
        s2p, s1, dl = np.zeros(len(live)), np.zeros(len(live)), np.zeros(len(live))
        for t in range(Tf):
            dx, dy = X[I, t, 0] - X[J, t, 0], X[I, t, 1] - X[J, t, 1]
            d2 = dx * dx + dy * dy
            dl = np.sqrt(d2)
            s2p += d2
            s1 += dl
        pp = p[I] * p[J]
        terms[0, live], terms[1, live], terms[2, live] = pp * (s1 / Tf), pp * dl, pp * np.sqrt(s2p)
    part = np.zeros((3, 256))
    for r in range(terms.shape[1] // 256):
        part += terms[:, 256 * r:256 * (r + 1)]
    v = [xor_tree(((part[q, :64] + part[q, 64:128]) + part[q, 128:192]) + part[q, 192:]) for q in range(3)]
    # distances to the ground truth, lane = sample
    da, df = np.zeros(64), np.zeros(64)
    for k in np.nonzero(pos)[0]:
        ga = gl = 0.0
        for t in range(Tf):
            dx, dy = X[k, t, 0] - Y[t, 0], X[k, t, 1] - Y[t, 1]
            gl = np.sqrt(dx * dx + dy * dy)
            ga += gl
        da[k], df[k] = p[k] * (ga / Tf), p[k] * gl
    eade, efde = xor_tree(da), xor_tree(df)
    ade_k = np.full(K, np.inf, np.float32)
    fde_k = np.full(K, np.inf, np.float32)
    ade_k[pos], fde_k[pos] = bok_f32(pred_a[pos], gt_a, scale)
    # rank by counting, scatter, inclusive prefix fminf
    rank = [sum(1 for j in range(K) if w32[j] > w32[k] or (w32[j] == w32[k] and j < k)) for k in range(K)]
    for name, val in (('ade', ade_k), ('fde', fde_k)):
        slots = np.full(64, np.inf, np.float32)
        slots[rank] = val
        pre = np.fmin.accumulate(slots)
        pre[:63] = np.fmin(pre[:63], np.float32(np.inf))
        out[name + '_top'] = pre[:K].copy()
        m = pre[63]
        hit = [k for k in range(K) if pos[k] and val[k] == m]
        out['brier_' + name] = float(m) + (1.0 - p[hit[0]]) ** 2 if hit else np.nan
    out.update(eade=eade, efde=efde, es_ade=eade - v[0], es_fde=efde - v[1], es_ade_mag=abs(eade) + abs(v[0]),
               es_fde_mag=abs(efde) + abs(v[1]), neff=1.0 / s2)
    if om > 0.0:
        out['apd'], out['fpd'] = 2.0 * v[2] / om, 2.0 * v[1] / om
    # KDE NLL, lane = frame of the tile
    if pos.sum() >= 3 and om > 0.0:
        f2 = np.cbrt(s2)
        ks = np.nonzero(pos)[0]
        logp = np.log(np.where(pos, p, 1.0))
        acc, sing = 0.0, False
        for t0 in range(0, Tf, TILE):
            lp = np.zeros(64)
            for t in range(t0, min(t0 + TILE, Tf)):
                mx = my = 0.0
                for k in ks:
                    mx += p[k] * X[k, t, 0]
                    my += p[k] * X[k, t, 1]
                c00 = c01 = c11 = 0.0
                for k in ks:
                    dx, dy = X[k, t, 0] - mx, X[k, t, 1] - my
                    c00 += p[k] * (dx * dx)
                    c01 += p[k] * (dx * dy)
                    c11 += p[k] * (dy * dy)
                c00, c01, c11 = c00 / om, c01 / om, c11 / om
                det = c00 * c11 - c01 * c01
                if not c00 > 0.0 or not det > 0.0:
                    sing = True
                    continue
                inv = 1.0 / (f2 * det)
                dx, dy = Y[t, 0] - X[ks, t, 0], Y[t, 1] - X[ks, t, 1]
                e = logp[ks] - 0.5 * ((c11 * dx * dx - 2.0 * c01 * dx * dy + c00 * dy * dy) * inv)
                m = e.max()
                sm = 0.0
                for x in e:
                    sm += np.exp(x - m)
                tf2 = 6.283185307179586 * f2
                lp[t - t0] = max(np.log(sm) + m - 0.5 * np.log(tf2 * tf2 * det), -20.0)
            acc += xor_tree(lp)
        out['kde_nll'] = np.nan if sing else -acc / Tf
    return out


def weighted_set_np(pred, weights, gt, scale):
    """Every agent of pred [n, K, Tf, 2], weights [n, K], gt [n, Tf, 2] (float32): a dict name -> array over the agents."""
    rows = [agent_np(pred[a], weights[a], gt[a], scale) for a in range(pred.shape[0])]
    return {k: np.stack([np.asarray(r[k]) for r in rows]) for k in rows[0]}


def uniform_spread_np(pred, gt, scale):
    """DESIGN.md 4s at equal weights: apd / fpd (pair means of the trajectory / final distance), the energy scores
    (1/K) sum_k D_k - ((K-1)/(2K)) pair mean, and the unweighted KDE NLL of sttode_kde_nll (NaN where C is singular), array form."""
    X, Y = coords(pred, scale), coords(gt, scale)
    n, K, Tf = X.shape[:3]
    I, J = np.triu_indices(K, 1)
    d = np.sqrt(((X[:, I] - X[:, J]) ** 2).sum(axis=-1))                # [n, P, Tf]
    G = np.sqrt(((X - Y[:, None]) ** 2).sum(axis=-1))                    # [n, K, Tf]
    c = (K - 1) / (2.0 * K)
    out = {'apd': np.sqrt((d * d).sum(axis=-1)).mean(axis=1), 'fpd': d[..., -1].mean(axis=1),
           'es_ade': G.mean(axis=2).mean(axis=1) - c * d.mean(axis=2).mean(axis=1),
           'es_fde': G[..., -1].mean(axis=1) - c * d[..., -1].mean(axis=1)}
    nll = np.zeros(n)
    f2 = float(K) ** (-1.0 / 3.0)
    for a in range(n):
        for t in range(Tf):
            x = X[a, :, t]
            C = np.cov(x.T, bias=False)
            det = C[0, 0] * C[1, 1] - C[0, 1] * C[0, 1]
            if not C[0, 0] > 0 or not det > 0:
                nll[a] = np.nan
                continue
            r = Y[a, t] - x
            q = (C[1, 1] * r[:, 0] ** 2 - 2 * C[0, 1] * r[:, 0] * r[:, 1] + C[0, 0] * r[:, 1] ** 2) / (f2 * det)
            e = -0.5 * q
            lp = np.log(np.exp(e - e.max()).sum()) + e.max() - np.log(K) - 0.5 * np.log((2 * np.pi * f2) ** 2 * det)
            nll[a] -= max(lp, -20.0) / Tf
    out['kde_nll'] = nll
    return out
