"""Cases and NumPy yardsticks of the large-set scores (sttode_large_select / _kde_nll / _spread, csrc/large_set.hip), shared
by tests/golden/make_large_set_golden.py and the tests.

The inputs of a case are not stored: they regenerate from the seed the maker found (``case_inputs``), and tests/golden/large_set.npz keeps
the seed, a float64 checksum of the inputs and the expected outputs -- a 2000- or 4096-sample case would not fit the fixture otherwise.

Everything here is float64 on x = (double)(x * scale) with the product in float32 (``coords``), written with array operations and NumPy's
own (pairwise) sums: independent of any kernel's order.  The float32 per-sample ADE / FDE of the selection are tests/weighted_ref.py's
``bok_f32`` (bok_dist with its fused multiply-add, frames in frame order)."""
import numpy as np

from weighted_ref import bok_f32, coords

EPS32 = 2.0 ** -23
GAP = 16.0          # near-tie rule: best and runner-up differ by a relative gap of at least GAP * Tf * 2^-23

# tag -> seed-search start, n (None: the sum of sizes), R, K_in, Tf, scale, div_scale, miss threshold, segment sizes (None: no joint part), the
# parts computed ('s' selection, 'k' KDE NLL, 'p' pair statistics), the spread of the samples, the edit
CASES = {
    'm3_t1':        dict(seed=100, n=4, R=1, K_in=3, Tf=1, scale=1.0, div=1.0, thr=0.2, sizes=(1, 3), parts='skp', spread=0.5, edit=None),
    'm64_t12':      dict(seed=200, n=6, R=2, K_in=32, Tf=12, scale=0.5, div=2.0, thr=0.1, sizes=(1, 1, 3, 0, 1), parts='skp', spread=0.3, edit=None),
    'm65_t40':      dict(seed=300, n=304, R=1, K_in=65, Tf=40, scale=1.0, div=10.0, thr=0.5, sizes=(1, 0, 2, 300, 1), parts='skp', spread=0.3,
                         edit=None),
    'm256_t12':     dict(seed=400, n=3, R=2, K_in=128, Tf=12, scale=1.0, div=1.0, thr=0.1, sizes=(3,), parts='skp', spread=0.3, edit=None),
    'm257_t33':     dict(seed=500, n=3, R=1, K_in=257, Tf=33, scale=50.0, div=5000.0, thr=5.0, sizes=(2, 1), parts='skp', spread=0.3, edit=None),
    'm400_r20_dup': dict(seed=600, n=7, R=20, K_in=20, Tf=12, scale=1.0, div=1.0, thr=0.1, sizes=(2, 1, 4), parts='skp', spread=0.3, edit='dup'),
    'm2000_t12':    dict(seed=700, n=3, R=16, K_in=125, Tf=12, scale=1.0, div=1.0, thr=0.05, sizes=(1, 2), parts='sk', spread=0.3, edit=None),
    'm4096_t2':     dict(seed=800, n=2, R=2, K_in=2048, Tf=2, scale=1.0, div=1.0, thr=0.02, sizes=(2,), parts='skp', spread=0.3, edit=None),
    'm65_nan':      dict(seed=900, n=5, R=1, K_in=65, Tf=12, scale=1.0, div=1.0, thr=0.1, sizes=(1, 1, 1, 2), parts='s', spread=0.3, edit='nan'),
    'm65_far':      dict(seed=1000, n=4, R=1, K_in=65, Tf=12, scale=1.0, div=1.0, thr=1.0, sizes=(4,), parts='skp', spread=0.3, edit='far'),
    'm65_degen':    dict(seed=1100, n=4, R=1, K_in=65, Tf=12, scale=0.5, div=1.0, thr=0.1, sizes=None, parts='k', spread=0.3, edit='degen'),
}
DEGEN_FRAMES = {0: (3,), 2: (0, 11)}     # 'degen': agent -> frames whose samples all have x = 0 (agent 0: C00 = 0) or y = 0 (agent 2: det = 0)
NAN_ALL = 3                              # 'nan': the agent whose samples are all NaN


def case_ks(c):
    M = c['R'] * c['K_in']
    return sorted({k for k in (1, c['K_in'], 64, 65, M) if 1 <= k <= M})


def seg_ptr_of(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)


def flat(pred5):
    """[R, n, K_in, Tf, 2] -> [n, M, Tf, 2], sample m = r K_in + k."""
    R, n, K_in, Tf = pred5.shape[:4]
    return np.ascontiguousarray(np.transpose(pred5, (1, 0, 2, 3, 4)).reshape(n, R * K_in, Tf, 2))


def case_inputs(tag, seed):
    """(pred [R, n, K_in, Tf, 2] float32, gt [n, Tf, 2] float32, info) of a case from a seed.  info: for 'dup' the (agent, source sample,
    copy) triples."""
    c = CASES[tag]
    n, R, K_in, Tf, s = c['n'], c['R'], c['K_in'], c['Tf'], c['spread']
    M = R * K_in
    rng = np.random.default_rng(seed)
    start, vel = rng.uniform(-6, 6, (n, 1, 2)), rng.normal(0, 0.4, (n, 1, 2))
    gt = (start + vel * np.arange(1, Tf + 1)[None, :, None]).astype(np.float32)
    drift = rng.normal(0, s, (n, M, 1, 2)) * np.linspace(0.3, 1.0, Tf)[None, None, :, None]
    x = (gt[:, None].astype(np.float64) + drift + rng.normal(0, 0.1 * s, (n, M, Tf, 2))).astype(np.float32)
    info = []
    if c['edit'] == 'dup':
        # the best sample by ADE (agents 0, 2) / by FDE (agent 1) copied into another round, once behind it and once in front of it
        ade, fde = select_f64(x, gt, c['scale'])
        for a, val in ((0, ade), (1, fde), (2, ade)):
            b = int(np.argmin(val[a]))
            to = (b + 7 * K_in + 3) % M if a != 2 else (b - 5 * K_in - 2) % M
            x[a, to] = x[a, b]
            info.append((a, b, to))
    elif c['edit'] == 'nan':
        x[0, 7] = np.nan                                   # one whole sample
        x[1, 0, 5, 1] = np.nan                             # the first sample, one coordinate: the k = 1 prefix has no value
        x[2, :2] = np.nan                                  # the first two samples
        x[NAN_ALL] = np.nan                                # every sample
        x[4, 64] = np.nan                                  # the last sample
    elif c['edit'] == 'far':
        gt[::2] += 60.0
    elif c['edit'] == 'degen':
        x[0, :, DEGEN_FRAMES[0][0], 0] = 0.0
        for t in DEGEN_FRAMES[2]:
            x[2, :, t, 1] = 0.0
    pred5 = np.ascontiguousarray(np.transpose(x.reshape(n, R, K_in, Tf, 2), (1, 0, 2, 3, 4)))
    return pred5, gt, info


def checksum(pred5, gt):
    return float(np.nansum(pred5.astype(np.float64)) + np.nansum(gt.astype(np.float64)) + np.isnan(pred5).sum())


# ----- selection -----------------------------------------------------------------------------------------------------------------------

def first_min(v):
    """(minimum, lowest index) by the entry's rule: a value wins only by being smaller (<) than the best so far, which starts at +inf with
    index 0 -- NaN and +inf never win."""
    w = np.where(np.isnan(v), np.inf, v)
    i = int(np.argmin(w))
    return (w[i], i) if w[i] < np.inf else (w.dtype.type(np.inf), 0)


def runner_up_gap(v, exclude=()):
    """Relative gap between the minimum of v and the smallest other value (NaN skipped; ``exclude``: indices that are exact copies of the
    best sample); inf when there is no other value."""
    w = np.where(np.isnan(v), np.inf, np.asarray(v, np.float64))
    i = int(np.argmin(w))
    rest = np.delete(w, [i] + ([e for e in exclude if e != i] if i in exclude else []))
    if rest.size == 0 or not np.isfinite(rest.min()) or not np.isfinite(w[i]):
        return np.inf
    return (rest.min() - w[i]) / max(abs(w[i]), np.finfo(np.float64).tiny)


def select_f64(x, gt, scale):
    """Per-sample (ADE, FDE) [n, M] in float64, by bok_dist's formula |(x - g) scale| (the selection scales the difference; the KDE and the
    pair statistics scale the coordinates)."""
    D = np.linalg.norm((x.astype(np.float64) - gt.astype(np.float64)[:, None]) * float(np.float32(scale)), axis=-1)
    return D.mean(axis=-1), D[..., -1]


def select_f32(x, gt, scale):
    """Per-sample (ADE, FDE) [n, M] float32 as bok_select_kernel computes them."""
    out = [bok_f32(x[a], gt[a], scale) for a in range(x.shape[0])]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def select_from(va, vf, thr, ks, seg_ptr=None):
    """The entry's outputs from per-sample values [n, M] (float32: the expected bits; float64: the yardstick)."""
    n, M = va.shape
    out = {}
    for name, v in (('ade', va), ('fde', vf)):
        mi = [first_min(v[a]) for a in range(n)]
        out[name] = np.array([m for m, _ in mi], v.dtype)
        out[name + '_idx'] = np.array([i for _, i in mi], np.int32)
        out[name + '_at'] = np.array([[first_min(v[a, :k])[0] for k in ks] for a in range(n)], v.dtype).reshape(n, len(ks))
    out['miss'] = out['fde'] > v.dtype.type(thr)
    if seg_ptr is not None:
        S = len(seg_ptr) - 1
        for name, v in (('jade', va), ('jfde', vf)):
            val, idx = np.full(S, np.nan), np.full(S, -1, np.int32)
            for s in range(S):
                a0, a1 = seg_ptr[s], seg_ptr[s + 1]
                if a1 > a0:
                    tot = np.zeros(M)
                    for a in range(a0, a1):                          # in agent order, in double
                        tot = tot + v[a].astype(np.float64)
                    val[s], idx[s] = first_min(tot / float(a1 - a0))
            out['seg_' + name], out['seg_' + name + '_idx'] = val, idx
    return out


# ----- KDE NLL -------------------------------------------------------------------------------------------------------------------------

def kde_np(x, gt, scale, reverse=False):
    """nll [n] float64 by 4l's formulas (NaN where C00 <= 0 or det C <= 0 at some frame); ``reverse``: the samples in reversed order."""
    X, Y = coords(x, scale), coords(gt, scale)
    if reverse:
        X = X[:, ::-1]
    n, M, Tf = X.shape[:3]
    f2 = float(M) ** (-1.0 / 3.0)
    out = np.zeros(n)
    with np.errstate(invalid='ignore', divide='ignore'):
        for a in range(n):
            acc, bad = 0.0, False
            for t in range(Tf):
                P = X[a, :, t]
                d = P - P.sum(axis=0) / M
                c00, c01, c11 = (d[:, 0] * d[:, 0]).sum() / (M - 1), (d[:, 0] * d[:, 1]).sum() / (M - 1), (d[:, 1] * d[:, 1]).sum() / (M - 1)
                det = c00 * c11 - c01 * c01
                if not c00 > 0.0 or not det > 0.0:
                    bad = True
                    continue
                g = Y[a, t] - P
                e = -0.5 * (c11 * g[:, 0] * g[:, 0] - 2.0 * c01 * g[:, 0] * g[:, 1] + c00 * g[:, 1] * g[:, 1]) / (f2 * det)
                m = e.max()
                lp = np.log(np.exp(e - m).sum()) + m - np.log(M) - 0.5 * np.log((2.0 * np.pi * f2) ** 2 * det)
                acc += max(lp, -20.0)
            out[a] = np.nan if bad else -acc / Tf
    return out


def kde_scipy(x, gt, scale):
    """(nll [n] float64 over scipy.stats.gaussian_kde, NaN where it raises; the (agent, frame) pairs where it raised)."""
    from scipy.stats import gaussian_kde
    X, Y = coords(x, scale), coords(gt, scale)
    n, M, Tf = X.shape[:3]
    out, raised = np.zeros(n), []
    for a in range(n):
        acc = 0.0
        for t in range(Tf):
            try:
                acc += max(float(gaussian_kde(X[a, :, t].T).logpdf(Y[a, t])[0]), -20.0)
            except np.linalg.LinAlgError:
                raised.append((a, t))
        out[a] = np.nan if any(r[0] == a for r in raised) else -acc / Tf
    return out, raised


# ----- pair statistics -----------------------------------------------------------------------------------------------------------------

def spread_np(x, gt, scale, div_scale, rows=128):
    """4s's values over all M (M-1) / 2 pairs, float64 [n] each, plus es_*_mag (the two terms of the energy score ADDED: what the GPU
    test's tolerance is taken of).  The pair space goes through blocks of ``rows`` rows."""
    X, Y = coords(x, scale), coords(gt, scale)
    n, M, Tf = X.shape[:3]
    out = {k: np.zeros(n) for k in ('apd', 'fpd', 'pade', 'dlow')}
    npairs = M * (M - 1) / 2.0
    for a in range(n):
        tot = np.zeros(4)
        for i0 in range(0, M, rows):
            D = np.linalg.norm(X[a, i0:i0 + rows, None] - X[a, None], axis=-1)        # [rows, M, Tf]
            up = np.arange(i0, min(i0 + rows, M))[:, None] < np.arange(M)[None]
            t2 = (D * D).sum(axis=-1)
            tot += [np.sqrt(t2)[up].sum(), D[..., -1][up].sum(), (D.sum(axis=-1) / Tf)[up].sum(), np.exp(-t2 / div_scale)[up].sum()]
        for k, v in zip(('apd', 'fpd', 'pade', 'dlow'), tot):
            out[k][a] = v / npairs
    G = np.linalg.norm(X - Y[:, None], axis=-1)
    c = (M - 1) / (2.0 * M)
    for name, per, pair in (('ade', G.mean(axis=-1), out['pade']), ('fde', G[..., -1], out['fpd'])):
        A = per.mean(axis=1)
        out['es_' + name], out['es_' + name + '_mag'] = A - c * pair, A + c * pair
    return out


def energy_double_sum(x, gt, scale):
    """The energy scores from the explicit 1 / M^2 double sum over all ordered pairs, the diagonal included (small M only)."""
    X, Y = coords(x, scale), coords(gt, scale)
    M = X.shape[1]
    D = np.linalg.norm(X[:, :, None] - X[:, None], axis=-1)
    G = np.linalg.norm(X - Y[:, None], axis=-1)
    return (G.mean(axis=-1).mean(axis=1) - 0.5 * D.mean(axis=-1).sum(axis=(1, 2)) / (M * M),
            G[..., -1].mean(axis=1) - 0.5 * D[..., -1].sum(axis=(1, 2)) / (M * M))
