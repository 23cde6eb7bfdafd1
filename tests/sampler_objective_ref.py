"""Plain torch restatement of sttode_sampler_objective / _bwd (csrc/sampler_objective.hip), shared by
tests/golden/make_sampler_objective_golden.py and tests/test_sampler_objective*.py.  It runs in the dtype of its inputs: float64 is the
yardstick, float32 torch's own evaluation of the same statements (tests/train_ref.py: assert_f64_close)."""
import numpy as np
import torch
import torch.nn.functional as F

# (n, K, nz, Tf): one pair | the training shape | K nz no multiple of 64 | K D = 4096, all of the LDS | Tf = 1 (es_ade == es_fde)
CASES = [(1, 2, 5, 2), (19, 20, 32, 12), (3, 3, 5, 10), (2, 64, 32, 32), (4, 20, 32, 1)]
MASKS = ('none', 'ragged')
SCALES = (2.0, 0.5)                      # samplerloss.get_diversity_config(None) and ('sdd')
TERMS = ('kld', 'div', 'rec', 'es_ade', 'es_fde')


def tag(case, mask):
    return 'n%d_k%d_z%d_t%d_%s' % (*case, mask)


def objective(mu, logvar, pmu, plogvar, motion, gt, mask, scale, g=None, best=None):
    """motion [n,K,Tf,2], gt [n,Tf,2], mask [n,Tf] or None, latents [n K, nz]; g: dict term -> upstream [n] (missing = zero) or None (no
    backward).  ``best`` [n]: the sample that takes rec's gradient (default: the first minimum, np.argmin).
    -> kld, div, rec, es_ade, es_fde [n], best [n] (int64), rec_k [n,K], and with g: dmu, dlogvar, dmotion."""
    n, K, Tf = motion.shape[:3]
    m, lv, mo = (v.detach().clone().requires_grad_(True) for v in (mu, logvar, motion))
    pm = 0.0 if pmu is None else pmu
    ps = (1.0 if plogvar is None else torch.exp(0.5 * plogvar)) + 1e-8
    t1, t2 = (m - pm) / ps, torch.exp(0.5 * lv) / ps
    kld = (0.5 * (t1 * t1 + t2 * t2) - 0.5 - torch.log(t2)).reshape(n, -1).sum(1)
    div = torch.stack([(-(F.pdist(mo[a].reshape(K, -1), 2) ** 2) / scale).exp().mean() for a in range(n)])
    w = torch.ones(n, Tf, dtype=motion.dtype) if mask is None else mask.to(motion.dtype)
    diff = (mo - gt[:, None]) * w[:, None, :, None]                                    # the mask multiplies the difference
    rec_k = diff.pow(2).sum(-1).sum(-1)
    if best is None:
        best = torch.from_numpy(np.argmin(rec_k.detach().numpy(), axis=1))             # the first minimum
    rec = rec_k.gather(1, best[:, None])[:, 0]
    gd = diff.norm(dim=-1)                                                             # [n,K,Tf]; subgradient 0 at 0
    iu = torch.triu_indices(K, K, 1)
    pd = ((mo[:, iu[0]] - mo[:, iu[1]]) * w[:, None, :, None]).norm(dim=-1)            # [n,P,Tf], F.pdist order
    c = (K - 1) / (2.0 * K)
    es_ade = gd.mean(-1).mean(1) - c * pd.mean(-1).mean(1)
    es_fde = gd[..., -1].mean(1) - c * pd[..., -1].mean(1)
    out = dict(kld=kld.detach(), div=div.detach(), rec=rec.detach(), es_ade=es_ade.detach(), es_fde=es_fde.detach(), best=best,
               rec_k=rec_k.detach())
    if g is not None:
        terms = dict(kld=kld, div=div, rec=rec, es_ade=es_ade, es_fde=es_fde)
        total = sum((terms[k] * g[k].to(motion.dtype)).sum() for k in TERMS if g.get(k) is not None)
        total = total + 0.0 * (m.sum() + lv.sum() + mo.sum())                          # (every leaf gets a gradient, zeros included)
        total.backward()
        out.update(dmu=m.grad, dlogvar=lv.grad, dmotion=mo.grad)
    return out


def load_case(z, case, mask):
    """Inputs of one fixture case as torch float32 tensors (mask None for 'none') and its stored float64 results."""
    t, s = tag(case, mask), 'n%d_k%d_z%d_t%d' % case
    f = lambda k: torch.from_numpy(np.asarray(z[k]))
    inp = dict(mu=f(s + '/mu'), logvar=f(s + '/logvar'), pmu=f(s + '/pmu'), plogvar=f(s + '/plogvar'), motion=f(s + '/motion'), gt=f(s + '/gt'),
               mask=None if mask == 'none' else f(t + '/mask'), g={k: f(s + '/g_' + k) for k in TERMS})
    keys = ('rec', 'best', 'es_ade', 'es_fde', 'd_es_ade', 'd_es_fde_last', 'd_rec_best', 'ref_recon', 'ref_recon_grad_best', 'ties',
            'tie_grad_on_lowest')
    return inp, {k: np.asarray(z[t + '/' + k]) for k in keys}


def stored_jacobians(st, shape):
    """The fixture's per-agent gradients d term[a] / d motion[a], expanded to [n,K,Tf,2] float64: rec's sits on the best sample, es_fde's on
    the last frame; everything else is zero (asserted by the maker)."""
    n, K, Tf, _ = shape
    d_rec, d_fde = np.zeros(shape), np.zeros(shape)
    d_rec[np.arange(n), st['best']] = st['d_rec_best']
    d_fde[:, :, -1] = st['d_es_fde_last']
    return dict(rec=d_rec, es_ade=st['d_es_ade'], es_fde=d_fde)
