"""Plain torch restatement of sttode_sampler_objective_joint / _bwd (csrc/sampler_joint.hip), shared by
tests/golden/make_sampler_joint_golden.py and tests/test_sampler_joint*.py, and the seeded inputs of their cases.  The restatement runs in
the dtype of its inputs: float64 is the yardstick, float32 torch's own evaluation of the same statements (tests/train_ref.py:
assert_f64_close).  The reference project has no joint form; tests/test_sampler_joint.py pins this restatement against NumPy loops."""
import numpy as np
import torch

# (K, nz, Tf): one pair | the training shape | K nz no multiple of 64 | K D = 4096 | Tf = 1
SHAPES = [(2, 5, 2), (20, 32, 12), (3, 5, 10), (64, 32, 32), (20, 32, 1)]
MASKS = ('none', 'ragged')
SCALES = (2.0, 0.5)
TERMS = ('kld', 'div', 'rec', 'es')
# the fixture's segment sizes per shape (ragged and equal, one-agent segments among them), and the masks it stores
GOLDEN_SEGS = {(2, 5, 2): (1, 2, 11, 3, 3), (20, 32, 12): (1, 2, 2, 3), (3, 5, 10): (1, 2, 11, 3, 3), (64, 32, 32): (2, 2, 2, 1),
               (20, 32, 1): (1, 2, 11, 3, 3)}
GOLDEN_MASKS = {s: (('ragged',) if s == (64, 32, 32) else MASKS) for s in SHAPES}
# the GPU tests' segment sizes: one wave's agents (64), the four-wave split and its remainder (65), more agents than any LDS staging
# would hold (257, at the training shape only), ragged and equal segments in one batch
GPU_SEGS = {s: (1, 2, 11, 64, 65) + ((257,) if s == (20, 32, 12) else ()) + (3, 3) for s in SHAPES}


def tag(shape, mask):
    return 'k%d_z%d_t%d_%s' % (*shape, mask)


def seg_ptr_of(segs):
    return np.concatenate([[0], np.cumsum(segs)]).astype(np.int32)


def _safe_sqrt(v):
    """sqrt with the subgradient 0 at 0 (R = 0 contributes no gradient)."""
    pos = v > 0
    return torch.where(pos, torch.where(pos, v, torch.ones_like(v)).sqrt(), torch.zeros_like(v))


def objective(mu, logvar, pmu, plogvar, motion, gt, mask, seg_ptr, scale, g=None, best=None):
    """motion [n,K,Tf,2], gt [n,Tf,2], mask [n,Tf] or None, latents [n K, nz], seg_ptr [S+1] (ints); g: dict term -> upstream (kld [n],
    the others [S]; missing = zero) or None (no backward).  ``best`` [S]: the sample that takes rec's gradient (default: the first minimum).
    -> kld [n], div, rec, es [S], best [S] (int64), J [S,K], and with g: dmu, dlogvar, dmotion."""
    n, K, Tf = motion.shape[:3]
    sp = [int(v) for v in seg_ptr]
    S = len(sp) - 1
    dt = motion.dtype
    m, lv, mo = (v.detach().clone().requires_grad_(True) for v in (mu, logvar, motion))
    pm = 0.0 if pmu is None else pmu
    ps = (1.0 if plogvar is None else torch.exp(0.5 * plogvar)) + 1e-8
    t1, t2 = (m - pm) / ps, torch.exp(0.5 * lv) / ps
    kld = (0.5 * (t1 * t1 + t2 * t2) - 0.5 - torch.log(t2)).reshape(n, -1).sum(1)
    w = torch.ones(n, Tf, dtype=dt) if mask is None else mask.to(dt)
    iu = torch.triu_indices(K, K, 1)
    nan = torch.tensor(float('nan'), dtype=dt)
    div, rec, es, bests, Js = [], [], [], [], []
    for s in range(S):
        a0, a1 = sp[s], sp[s + 1]
        ng = a1 - a0
        if ng <= 0:
            div.append(nan), rec.append(nan), es.append(nan), bests.append(0), Js.append(torch.full((K,), float('nan'), dtype=dt))
            continue
        x, ws = mo[a0:a1], w[a0:a1, None, :, None]
        pd = x[:, iu[0]] - x[:, iu[1]]                                                     # [ng,P,Tf,2], F.pdist order
        d2 = pd.pow(2).sum(-1).sum(-1).sum(0) / ng
        div.append((-d2 / scale).exp().mean())
        diff = (x - gt[a0:a1, None]) * ws
        J = diff.pow(2).sum(-1).sum(-1).sum(0)                                             # [K]
        b = int(np.argmin(J.detach().numpy())) if best is None else int(best[s])           # the first minimum
        rec.append(J[b])
        rg = _safe_sqrt(J / (ng * Tf))
        rp = _safe_sqrt((pd * ws).pow(2).sum(-1).sum(-1).sum(0) / (ng * Tf))
        es.append(rg.sum() / K - rp.sum() / (K * K))
        bests.append(b), Js.append(J.detach())
    div, rec, es = torch.stack(div), torch.stack(rec), torch.stack(es)
    out = dict(kld=kld.detach(), div=div.detach(), rec=rec.detach(), es=es.detach(), best=torch.tensor(bests, dtype=torch.int64),
               J=torch.stack(Js))
    if g is not None:
        terms = dict(kld=kld, div=div, rec=rec, es=es)
        total = sum((terms[k] * g[k].to(dt)).sum() for k in TERMS if g.get(k) is not None)
        total = total + 0.0 * (m.sum() + lv.sum() + mo.sum())                              # (every leaf gets a gradient, zeros included)
        total.backward()
        out.update(dmu=m.grad, dlogvar=lv.grad, dmotion=mo.grad)
    return out


def roles(segs, K):
    """(tie segment, equal segment): the first two multi-agent segments; the others are free.  K = 2 has no tie (one pair)."""
    multi = [i for i, c in enumerate(segs) if c > 1]
    return (multi[0] if K > 2 else None), multi[1]


def draw(seed, shape, segs, mask_kind):
    """Seeded float32 inputs of one case.  Samples are the ground truth plus noise of sigma = sqrt(1 / (4 Tf)), so that an agent's
    E |x_i - x_j|^2 = 1 and d2_g / scale is of order 1 at both scales.  Constructed: in the tie segment, samples 1 and K-1 of EVERY agent
    are the ground truth plus 0.05 sigma noise and identical bit for bit (best = 1; a pair with R = 0); in the equal segment sample 0 of
    every agent IS the ground truth (R_g(x_0, y) = 0, rec = 0, best = 0).  'ragged': 0/1 masks with the first agent of the first free
    multi-agent segment masked entirely and the last frame of that segment's every agent masked (Tf = 1: that segment is masked whole)."""
    K, nz, Tf = shape
    n = int(sum(segs))
    sp = seg_ptr_of(segs)
    rng = np.random.default_rng(seed)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    mu, lv, pmu, plv = f(n * K, nz), np.float32(0.5) * f(n * K, nz), np.float32(0.5) * f(n * K, nz), np.float32(0.5) * f(n * K, nz)
    sigma = np.float32(np.sqrt(1.0 / (4 * Tf)))
    gt = (f(n, 1, 2) + np.float32(0.3) * np.cumsum(f(n, Tf, 2), axis=1)).astype(np.float32)
    motion = (gt[:, None] + sigma * f(n, K, Tf, 2)).astype(np.float32)
    tie, eq = roles(segs, K)
    if tie is not None:
        a0, a1 = sp[tie], sp[tie + 1]
        motion[a0:a1, K - 1] = gt[a0:a1] + np.float32(0.05) * sigma * f(a1 - a0, Tf, 2)
        motion[a0:a1, 1] = motion[a0:a1, K - 1]
    motion[sp[eq]:sp[eq + 1], 0] = gt[sp[eq]:sp[eq + 1]]
    mask = None
    if mask_kind == 'ragged':
        mask = (rng.random((n, Tf)) < 0.8).astype(np.float32)
        free = [i for i, c in enumerate(segs) if c > 1 and i not in (tie, eq)][0]
        mask[sp[free]] = 0
        mask[sp[free]:sp[free + 1], -1] = 0
        if tie is not None:
            mask[sp[tie]:sp[tie + 1], 0] = 1                                               # (the tie segment keeps a live frame)
        mask[sp[eq]:sp[eq + 1], 0] = 1
    S = len(segs)
    g = dict(kld=f(n), div=f(S), rec=f(S), es=f(S))
    return dict(mu=mu, logvar=lv, pmu=pmu, plogvar=plv, motion=motion, gt=gt, mask=mask, seg_ptr=sp, g=g, sigma=float(sigma))


def conditions(inp, shape, segs, r64):
    """The input conditions of a case (None if they hold, else why not), on the float64 restatement's J [S,K] and best at scale 0.5 / 2:
    apart from the constructed tie the two smallest J_g differ by more than 1e-5 relative; every R_g not constructed to be zero is at least
    1e-3 of the samples' spread; some multi-agent segment's best differs from the own argmin of one of its agents; at least half of a
    segment's pairs have exp(-d2_g / scale) > 1e-6 at the smaller scale."""
    K, nz, Tf = shape
    sp = inp['seg_ptr']
    tie, eq = roles(segs, K)
    mo, gt = inp['motion'].astype(np.float64), inp['gt'].astype(np.float64)
    w = np.ones(mo.shape[:1] + (Tf,)) if inp['mask'] is None else inp['mask'].astype(np.float64)
    iu = np.triu_indices(K, 1)
    differs = False
    for s, c in enumerate(segs):
        a0, a1 = int(sp[s]), int(sp[s + 1])
        if not w[a0:a1].any():
            continue                                                                       # a segment masked whole: every J, R is zero
        J = np.sort(r64['J'][s].numpy())
        if s == tie:
            if not (J[0] == J[1] and r64['best'][s] == 1 and J[2] - J[1] > 1e-5 * J[2]):
                return f'segment {s}: the constructed tie is not the minimum'
        elif J[1] - J[0] <= 1e-5 * J[1]:
            return f'segment {s}: the two smallest J_g are within 1e-5'
        if s == eq and not (J[0] == 0 and r64['best'][s] == 0):
            return f'segment {s}: sample 0 is not the ground truth'
        x, ws = mo[a0:a1], w[a0:a1, None, :, None]
        rg = np.sqrt(r64['J'][s].numpy() / (c * Tf))
        pd = x[:, iu[0]] - x[:, iu[1]]
        rp = np.sqrt(((pd * ws) ** 2).sum((0, 2, 3)) / (c * Tf))
        zero_p = (iu[0] == 1) & (iu[1] == K - 1) if s == tie else np.zeros(len(iu[0]), bool)
        zero_g = np.arange(K) == 0 if s == eq else np.zeros(K, bool)
        if (rp[~zero_p] < 1e-3 * inp['sigma']).any() or (rg[~zero_g] < 1e-3 * inp['sigma']).any():
            return f'segment {s}: an R_g below 1e-3 of the spread'
        if not ((rp[zero_p] == 0).all() and (rg[zero_g] == 0).all()):
            return f'segment {s}: a constructed zero R_g is not zero'
        d2 = (pd ** 2).sum((0, 2, 3)) / c
        if (np.exp(-d2 / min(SCALES)) > 1e-6).mean() < 0.5:
            return f'segment {s}: fewer than half of the pairs above 1e-6'
        if c > 1:
            own = ((x - gt[a0:a1, None]) * ws) ** 2
            differs |= bool((np.argmin(own.sum((2, 3)), axis=1) != int(r64['best'][s])).any())
    if any(c > 1 for c in segs) and not differs:
        return 'no multi-agent segment whose best differs from an agent\'s own argmin'
    return None


def make_case(shape, segs, mask_kind, seed0):
    """The first seed >= seed0 whose inputs meet the conditions -> (inputs as numpy, float64 restatement at scale 2 with no upstream)."""
    for seed in range(seed0, seed0 + 50):
        inp = draw(seed, shape, segs, mask_kind)
        r64 = objective(*as_torch(inp, torch.float64), 2.0)
        why = conditions(inp, shape, segs, r64)
        if why is None:
            return inp, seed
    raise AssertionError(f'no seed in [{seed0}, {seed0 + 50}) meets the input conditions of {shape} {segs} {mask_kind}: {why}')


def as_torch(inp, dtype=torch.float32, prior=True):
    """(mu, logvar, pmu, plogvar, motion, gt, mask, seg_ptr) of a case in ``dtype``."""
    c = lambda k: None if inp[k] is None else torch.from_numpy(np.asarray(inp[k])).to(dtype)
    return (c('mu'), c('logvar'), c('pmu') if prior else None, c('plogvar') if prior else None, c('motion'), c('gt'), c('mask'),
            np.asarray(inp['seg_ptr']))


def upstream(inp):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in inp['g'].items()}
