#!/usr/bin/env python3
"""Generate tests/golden/sampler_objective.npz (the stage-2 objective's ground-truth terms) on the CPU, with the REFERENCE's
samplerloss.recon_loss (imported, as make_sample_spread_golden.py imports its diversity_loss) and a float64 torch restatement
(tests/sampler_objective_ref.py):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_sampler_objective_golden.py

Per shape (n, K, nz, Tf) of sampler_objective_ref.CASES, <shape>/...: seeded float32 inputs mu, logvar, pmu, plogvar [n K, nz],
motion [n,K,Tf,2], gt [n,Tf,2] and upstream gradients g_<term> [n].  Per (shape, mask) with mask 'none' | 'ragged', <shape>_<mask>/...:

  mask [n,Tf]                    float32 zeros and ones ('ragged' only): agent 0 has its last frame masked, agent n-1 every frame (n >= 2)
  rec [n], best [n]              float64 restatement: min_k sum_t (m_t (x_k,t - y_t))^2 and the first k that has it
  es_ade, es_fde [n]             float64 restatement, pair-mean form; asserted here against BOTH closed forms of
                                 make_sample_spread_golden.spread_np on the masked coordinates (pair mean and the 1/K^2 double sum)
  d_es_ade [n,K,Tf,2]            d es_ade[a] / d motion[a]
  d_es_fde_last [n,K,2]          d es_fde[a] / d motion[a] at the last frame (asserted zero at every other frame)
  d_rec_best [n,Tf,2]            d rec[a] / d motion[a, best[a]] (asserted zero at every other sample)
  ref_recon                      the reference's recon_loss(gt, motion, mask, 1)[1] in float64: asserted == mean(rec) to 1e-12 relative
  ref_recon_grad_best [n,Tf,2]   n times its autograd gradient at the best sample (asserted zero elsewhere, but for a tie that torch
                                 resolves to another index: see tie_grad_on_lowest)
  ties [m,3]                     constructed bit-for-bit duplicates (agent, sample, its duplicate)
  tie_grad_on_lowest             whether the reference's gradient of every tied agent lands on the lowest tied index in this torch build

Constructed: for K > 2, agent 0's sample K-1 is the ground truth plus noise of 0.05 of the spread and sample 1 its bit-for-bit duplicate (two identical
samples: a zero pair distance at every frame, and a tie of the minimum that must resolve to 1); sample 0 of agent n // 2 equals the ground
truth at frame 0.  Asserted per case, so that no branch is an accident of a seed (the seed moves on until they hold): apart from the tie,
every agent's smallest and second-smallest rec candidates differ by more than 1e-5 relative; every per-frame distance that is not zero by
construction (duplicates, the equal frame, masked frames) is at least 1e-3 of the coordinate spread (the standard deviation of the samples
about their agent's ground truth)."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
REF = os.environ.get('STTODE_REFERENCE', '/root/reference')

import sampler_objective_ref as SR                                   # noqa: E402
from make_sample_spread_golden import spread_np                      # noqa: E402


def reference_recon_loss():
    if REF not in sys.path:
        sys.path.insert(0, REF)
    from samplerloss import recon_loss
    return recon_loss


def draw(seed, case):
    n, K, nz, Tf = case
    rng = np.random.default_rng(seed)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    mu, lv, pmu, plv = f(n * K, nz), np.float32(0.5) * f(n * K, nz), np.float32(0.5) * f(n * K, nz), np.float32(0.5) * f(n * K, nz)
    sigma = np.float32(np.sqrt(1.0 / (4 * Tf)))                      # E |m_i - m_j|^2 = 1: every pair's DLow term counts at scale 2 and 0.5
    gt = (f(n, 1, 2) + np.float32(0.3) * np.cumsum(f(n, Tf, 2), axis=1)).astype(np.float32)
    motion = (gt[:, None] + sigma * f(n, K, Tf, 2)).astype(np.float32)
    ties = []
    if K > 2:
        motion[0, K - 1] = gt[0] + np.float32(0.05) * sigma * f(Tf, 2)
        motion[0, 1] = motion[0, K - 1]
        ties.append((0, 1, K - 1))
    motion[n // 2, 0, 0] = gt[n // 2, 0]
    mask = (rng.random((n, Tf)) < 0.7).astype(np.float32)
    mask[0, -1] = 0.0
    if Tf > 1:
        mask[0, 0] = 1.0
    if n >= 2:
        mask[n - 1] = 0.0
    if n >= 3:
        mask[1, -1] = 1.0                                            # ... and an agent whose last frame counts
    g = {k: f(n) for k in SR.TERMS}
    return dict(mu=mu, logvar=lv, pmu=pmu, plogvar=plv, motion=motion, gt=gt, g=g), mask, np.array(ties, np.int64).reshape(-1, 3), float(sigma)


def conditions(case, inp, mask, ties, sigma, r64):
    """None if the input conditions hold, else why not."""
    n, K, nz, Tf = case
    w = np.ones((n, Tf)) if mask is None else mask.astype(np.float64)
    X, Y = inp['motion'].astype(np.float64), inp['gt'].astype(np.float64)
    tied = {int(a) for a in ties[:, 0]}
    rk = np.sort(r64['rec_k'].numpy(), axis=1)
    for a in range(n):
        if not w[a].any():
            assert (rk[a] == 0).all() and int(r64['best'][a]) == 0
            continue
        if a in tied:
            if rk[a, 0] != rk[a, 1]:
                return 'agent %d: the constructed tie is not the minimum' % a
            rest = rk[a, 2:]
        else:
            rest = rk[a, 1:]
        if rest.size and not rest[0] - rk[a, 0] > 1e-5 * rest[0]:
            return 'agent %d: rec candidates %r too close' % (a, rk[a, :3])
    for a, lo, hi in ties:
        if w[a].any() and int(r64['best'][a]) != min(lo, hi):
            return 'tie of agent %d resolved to %d' % (a, int(r64['best'][a]))
    G = np.linalg.norm((X - Y[:, None]) * w[:, None, :, None], axis=-1)                       # [n,K,Tf]
    P = np.linalg.norm((X[:, :, None] - X[:, None]) * w[:, None, None, :, None], axis=-1)     # [n,K,K,Tf]
    zero_g = np.zeros_like(G, bool)
    zero_g[n // 2, 0, 0] = True
    zero_p = np.zeros_like(P, bool)
    zero_p[:, np.arange(K), np.arange(K)] = True
    for a, lo, hi in ties:
        zero_p[a, lo, hi] = zero_p[a, hi, lo] = True
    zero_g |= (w == 0)[:, None, :]
    zero_p |= (w == 0)[:, None, None, :]
    if not ((G == 0) == zero_g).all() or not ((P == 0) == zero_p).all():
        return 'a distance is zero (or not) against the construction'
    small = min(G[~zero_g].min() if (~zero_g).any() else np.inf, P[~zero_p].min() if (~zero_p).any() else np.inf)
    if small < 1e-3 * sigma:
        return 'a per-frame distance of %.2e < 1e-3 x %.3f' % (small, sigma)
    return None


def main():
    recon_loss = reference_recon_loss()
    out, tags = {}, []
    for case in SR.CASES:
        n, K, nz, Tf = case
        seed = 20261020 + 1000 * n + K
        for attempt in range(50):
            inp, ragged, ties, sigma = draw(seed + 7919 * attempt, case)
            t32 = {k: torch.from_numpy(v) for k, v in inp.items() if k != 'g'}
            res = {}
            for mk in SR.MASKS:
                mask = None if mk == 'none' else ragged
                a64 = [t32[k].double() for k in ('mu', 'logvar', 'pmu', 'plogvar', 'motion', 'gt')]
                res[mk] = SR.objective(*a64, None if mask is None else torch.from_numpy(mask).double(), 2.0)
                why = conditions(case, inp, mask, ties, sigma, res[mk])
                if why:
                    break
            if not why:
                break
            print('%s seed +%d: %s' % (SR.tag(case, mk), attempt, why))
        assert not why, (case, why)
        s = 'n%d_k%d_z%d_t%d' % case
        for k in ('mu', 'logvar', 'pmu', 'plogvar', 'motion', 'gt'):
            out[s + '/' + k] = inp[k]
        for k, v in inp['g'].items():
            out[s + '/g_' + k] = v
        for mk in SR.MASKS:
            mask = None if mk == 'none' else ragged
            w64 = torch.ones(n, Tf, dtype=torch.float64) if mask is None else torch.from_numpy(mask).double()
            r, t = res[mk], SR.tag(case, mk)
            mo64, gt64 = t32['motion'].double(), t32['gt'].double()
            # the energy scores against both closed forms of the sample_spread fixture's maker, on the masked coordinates
            sp = spread_np((mo64 * w64[:, None, :, None]).numpy(), (gt64 * w64[:, :, None]).numpy(), 1.0, 1.0)
            for k in ('es_ade', 'es_fde'):
                for form in (k, k + '_double'):
                    assert np.allclose(r[k].numpy(), sp[form], rtol=1e-12, atol=1e-14), (t, form, r[k].numpy(), sp[form])
            # per-agent gradients of rec, es_ade, es_fde: one backward each with ones upstream (an agent's terms read only its own samples)
            jac = {}
            for k in ('rec', 'es_ade', 'es_fde'):
                jac[k] = SR.objective(*a64, None if mask is None else w64, 2.0, g={k: torch.ones(n, dtype=torch.float64)})['dmotion'].numpy()
            best = r['best'].numpy()
            others = np.ones((n, K), bool)
            others[np.arange(n), best] = False
            assert (jac['rec'][others] == 0).all() and (jac['es_fde'][:, :, :-1] == 0).all()
            # the reference's own function and its autograd
            x = mo64.clone().requires_grad_(True)
            _, uw = recon_loss(gt64, x, w64, 1)
            uw.backward()
            ref_val, ref_grad = float(uw.detach()), x.grad.numpy() * n
            mine = float(r['rec'].mean())
            assert abs(mine - ref_val) <= 1e-12 * abs(ref_val), (t, mine, ref_val)
            live = [a for a, _, _ in ties if w64[a].any()]
            on_lowest = all((ref_grad[a, best[a]] != 0).any() and (ref_grad[a][others[a]] == 0).all() for a in live)
            keep = np.ones(n, bool)
            if not on_lowest:
                keep[live] = False
            assert (ref_grad[keep][others[keep]] == 0).all()
            assert np.allclose(ref_grad[keep][~others[keep]], jac['rec'][keep][~others[keep]], rtol=1e-12, atol=1e-15), t
            if mask is not None:
                out[t + '/mask'] = mask
            out[t + '/rec'], out[t + '/best'] = r['rec'].numpy(), best.astype(np.int32)
            out[t + '/es_ade'], out[t + '/es_fde'] = r['es_ade'].numpy(), r['es_fde'].numpy()
            out[t + '/d_es_ade'], out[t + '/d_es_fde_last'] = jac['es_ade'], jac['es_fde'][:, :, -1]
            out[t + '/d_rec_best'] = jac['rec'][np.arange(n), best]
            out[t + '/ref_recon'], out[t + '/ref_recon_grad_best'] = np.float64(ref_val), ref_grad[np.arange(n), best]
            out[t + '/ties'], out[t + '/tie_grad_on_lowest'] = ties, np.bool_(on_lowest)
            tags.append(t)
            print('%-24s rec %.4e (ref rel diff %.1e)  es_ade %.4f  es_fde %.4f  best[0] %d  tie grad on lowest: %s' % (
                t, mine, abs(mine - ref_val) / max(abs(ref_val), 1e-300), r['es_ade'].mean(), r['es_fde'].mean(), best[0], on_lowest))
        if Tf == 1:
            assert all(np.array_equal(res[mk]['es_ade'].numpy(), res[mk]['es_fde'].numpy()) for mk in SR.MASKS)
    out['cases'] = np.array(tags)
    path = os.path.join(HERE, 'sampler_objective.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
