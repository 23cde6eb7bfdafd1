"""Raw outputs of every entry point whose kernels take pieces from csrc/set_body.hpp / sampler_body.hpp, for a bit-for-bit comparison of two
builds of the library.  Needs a GPU.

    STTODE_HIP_LIB=<library built from the parent commit> python profiles/set_body/bits.py dump parent.npz
    python profiles/set_body/bits.py dump new.npz
    python profiles/set_body/bits.py compare parent.npz new.npz profiles/set_body/bits.txt

dump: one process calls every entry on the inputs of the families' fixtures under tests/golden/ (those that store inputs: scene_metrics,
sample_spread, weighted_set, reduce, multimodal, sampler_objective, sampler_joint) and on small seeded edge shapes: K = 2, 23, 24, 64 with
Tf = 1, 32, 33; M = 64, 65, 257 for the large-set entries; M = 65 with K = 3 and 5 (and M = 257, K = 20) for the two reductions, both init
modes, whole trajectories and from_frame = -1; segments [0, 0, n] (one empty, one of all n agents); a weights row with a zero and one with
a single positive weight; a NaN coordinate in one sample.  compare: every array of the two files as unsigned integers of its item size (NaN
payloads included); per entry the number of values compared and of values that differ; exit status 1 if any differs.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, 'tests', 'golden')


def cases_of(name):
    z = np.load(os.path.join(GOLDEN, name + '.npz'))
    out = {}
    for k in z.files:
        c, _, s = k.rpartition('/')
        out.setdefault(c, {})[s] = z[k]
    return out


def dump(path):
    import torch
    from sttode_amd import capi, metrics
    dev = torch.device('cuda:0')
    T = lambda a, dt=torch.float32: torch.as_tensor(np.ascontiguousarray(a)).to(dt).to(dev).contiguous()
    res = {}

    def put(entry, case, **arrays):
        for k, v in arrays.items():
            if v is not None:
                res[f'{entry}|{case}|{k}'] = v.detach().cpu().numpy()

    def slots(o):
        return {s: getattr(o, s) for s in o.__slots__ if isinstance(getattr(o, s, None), torch.Tensor)}

    def per_agent(case, pred, gt, seg_ptr, weights, scale=1.0, radius=0.5, div_scale=1.0):
        n, K, Tf = pred.shape[:3]
        p, g = T(pred), T(gt)
        if K <= 64 and seg_ptr is not None:
            put('joint_select', case, **slots(metrics.joint_select(p, g, seg_ptr, scale=scale, collision_radius=radius)))
        if 2 <= K <= 64:
            put('kde_nll', case, nll=metrics.kde_nll(p, g, scale=scale))
            put('sample_spread', case, **slots(metrics.sample_spread(p, g, scale=scale, div_scale=div_scale)))
            put('sample_spread_nogt', case, **slots(metrics.sample_spread(p, None, scale=scale, div_scale=div_scale)))
        if weights is not None:
            put('weighted_set', case, **slots(metrics.weighted_set(p, T(weights), g, scale=scale)))

    def sampler(case, mu, logvar, pmu, plogvar, motion, gt, mask, seg_ptr, scale=1.0):
        n, K, Tf = motion.shape[:3]
        nz, D = mu.shape[-1], 2 * Tf
        st = capi.stream_ptr()
        mu, logvar, motion, gt = T(mu), T(logvar), T(motion), T(gt)
        pmu, plogvar = (None, None) if pmu is None else (T(pmu), T(plogvar))
        mask = None if mask is None else T(mask)
        f = lambda m: torch.empty(m, device=dev)
        rng = np.random.default_rng(5)
        g = [T(rng.normal(size=n)) for _ in range(5)]
        kld, div = f(n), f(n)
        capi.call('sttode_sampler_loss', mu, logvar, pmu, plogvar, motion, n, K, nz, D, scale, kld, div, st)
        dmu, dlv, dmo = torch.empty_like(mu), torch.empty_like(logvar), torch.empty_like(motion)
        capi.call('sttode_sampler_loss_bwd', mu, logvar, pmu, plogvar, motion, g[0], g[1], n, K, nz, D, scale, dmu, dlv, dmo, st)
        put('sampler_loss', case, kld=kld, div=div, dmu=dmu, dlogvar=dlv, dmotion=dmo)
        kld, div, rec, ea, ef = (f(n) for _ in range(5))
        best = torch.empty(n, dtype=torch.int32, device=dev)
        capi.call('sttode_sampler_objective', mu, logvar, pmu, plogvar, motion, gt, mask, n, K, nz, D, scale, kld, div, rec, best, ea, ef, st)
        dmu, dlv, dmo = torch.empty_like(mu), torch.empty_like(logvar), torch.empty_like(motion)
        capi.call('sttode_sampler_objective_bwd', mu, logvar, pmu, plogvar, motion, gt, mask, *g, n, K, nz, D, scale, dmu, dlv, dmo, st)
        put('sampler_objective', case, kld=kld, div=div, rec=rec, best=best, es_ade=ea, es_fde=ef, dmu=dmu, dlogvar=dlv, dmotion=dmo)
        sp = T(seg_ptr, torch.int32)
        S = sp.numel() - 1
        ws = torch.empty((capi.sampler_joint_ws(n, K, S) + 7) // 8, dtype=torch.float64, device=dev)
        kld, (div, rec, es) = f(n), (f(S) for _ in range(3))
        best = torch.empty(S, dtype=torch.int32, device=dev)
        capi.call('sttode_sampler_objective_joint', mu, logvar, pmu, plogvar, motion, gt, mask, sp, S, n, K, nz, D, scale, ws, ws.numel() * 8,
                  kld, div, rec, best, es, st)
        gs = [T(rng.normal(size=S)) for _ in range(3)]
        dmu, dlv, dmo = torch.empty_like(mu), torch.empty_like(logvar), torch.empty_like(motion)
        capi.call('sttode_sampler_objective_joint_bwd', mu, logvar, pmu, plogvar, motion, gt, mask, sp, S, g[0], *gs, n, K, nz, D, scale, ws,
                  ws.numel() * 8, dmu, dlv, dmo, st)
        put('sampler_objective_joint', case, kld=kld, div=div, rec=rec, best=best, es=es, dmu=dmu, dlogvar=dlv, dmotion=dmo)

    def multimodal(case, pred, past, gt, eps, h, scale, seg_ptr=None):
        put('multimodal', case, **slots(metrics.multimodal(T(pred), T(past), T(gt), float(eps), hist_frames=int(h), scale=float(scale),
                                                           seg_ptr=seg_ptr)))

    def large(case, pred, gt, ks, seg_ptr):
        p, g = T(pred), T(gt)
        M = p.shape[0] * p.shape[2] if p.dim() == 5 else p.shape[1]
        put('large_select', case, **slots(metrics.large_select(p, g, ks=ks, seg_ptr=seg_ptr)))
        if M >= 3:
            put('large_kde_nll', case, nll=metrics.large_kde_nll(p, g))
        if M >= 2:
            put('large_spread', case, **slots(metrics.large_spread(p, g)))
            put('large_spread_nogt', case, **slots(metrics.large_spread(p, None)))

    def reductions(case, pred, K, seg_ptrs, inits=('first', 'maximin'), frames=(0, -1)):
        p = T(pred)
        for init in inits:
            for ff in frames:
                tag = f'{case}_{init if isinstance(init, str) else "given"}_f{ff}'
                i = init if isinstance(init, str) else T(init)
                r = metrics.reduce_samples(p, K, iters=10, from_frame=ff, init=i)
                put('reduce_samples', tag, centroids=r.centroids, labels=r.labels, counts=r.counts)
                for si, sp in enumerate(seg_ptrs):
                    r = metrics.reduce_scenes(p, sp, K, iters=10, from_frame=ff, init=i)
                    # (an agent outside every segment and the agents of an empty one keep what the allocation held)
                    inside = torch.zeros(p.shape[-4], dtype=torch.bool, device=dev)
                    inside[sp[0]:sp[-1]] = True
                    put('reduce_scenes', f'{tag}_s{si}', centroids=torch.where(inside[:, None, None, None], r.centroids, torch.zeros(())),
                        labels=r.labels, counts=r.counts)

    # ---- the fixtures that store inputs
    for c, d in cases_of('scene_metrics').items():
        if 'pred' in d:
            per_agent('golden_scene_metrics_' + c, d['pred'], d['gt'], d['seg_ptr'].tolist(), None, float(d['scale']), float(d['radius']))
    for c, d in cases_of('sample_spread').items():
        if 'pred' in d:
            per_agent('golden_sample_spread_' + c, d['pred'], d['gt'], None, None, float(d['scale']), div_scale=float(d['div_scale']))
    for c, d in cases_of('weighted_set').items():
        if 'pred' in d:
            per_agent('golden_weighted_set_' + c, d['pred'], d['gt'], None, d['weights'], float(d['scale']))
    for c, d in cases_of('reduce').items():
        if 'x' in d:
            n = d['x'].shape[0]
            reductions('golden_reduce_' + c, d['x'], d['init'].shape[1], [[0, 0, n], [0, n // 2, n]], inits=('first', 'maximin', d['init']))
    for c, d in cases_of('multimodal').items():
        if 'pred' in d:
            multimodal('golden_' + c, d['pred'], d['past'], d['gt'], d['eps'], d['h'], d['scale'], d['seg_ptr'].tolist() if 'seg_ptr' in d else None)
    so = cases_of('sampler_objective')
    for c, d in so.items():
        if 'motion' in d:
            n = d['motion'].shape[0]
            for tag, mask in (('none', None), ('ragged', so[c + '_ragged']['mask'])):
                sampler(f'golden_objective_{c}_{tag}', d['mu'], d['logvar'], d['pmu'], d['plogvar'], d['motion'], d['gt'], mask, [0, 0, n])
    for c, d in cases_of('sampler_joint').items():
        if 'motion' in d:
            n, K = d['motion'].shape[:2]
            rng = np.random.default_rng(int(d['seed']))
            mu, lv = rng.normal(size=(n * K, 8)), 0.3 * rng.normal(size=(n * K, 8))
            sampler('golden_joint_' + c, mu, lv, None, None, d['motion'], d['gt'], d.get('mask'), d['seg_ptr'].tolist())

    # ---- seeded edge shapes
    rng = np.random.default_rng(20240)
    n = 9
    for K in (2, 23, 24, 64):
        for Tf in (1, 32, 33):
            gt = np.cumsum(rng.normal(0, 0.4, (n, Tf, 2)), axis=1).astype(np.float32)
            pred = (gt[:, None] + rng.normal(0, 0.5, (n, K, Tf, 2))).astype(np.float32)
            pred[2, 1, 0, 0] = np.nan
            w = rng.integers(0, 5, (n, K)).astype(np.float32) + 1.0
            w[0, 0] = 0.0                                      # a row with a zero
            w[1] = 0.0
            w[1, K - 1] = 3.0                                  # a row with a single positive weight
            case = f'edge_k{K}_t{Tf}'
            per_agent(case, pred, gt, [0, 0, n], w)
            past = np.cumsum(rng.normal(0, 0.4, (n, 8, 2)), axis=1).astype(np.float32)
            multimodal(case, pred, past, gt, 1.5, 3, 1.0, [0, 0, n])
            if K * 2 * Tf <= 4096:
                nz = 5
                mu, lv = rng.normal(size=(n * K, nz)), 0.3 * rng.normal(size=(n * K, nz))
                pmu, plv = rng.normal(size=(n * K, nz)), 0.3 * rng.normal(size=(n * K, nz))
                mask = (rng.random((n, Tf)) < 0.8).astype(np.float32)
                sampler(case + '_prior_mask', mu, lv, pmu, plv, pred, gt, mask, [0, 0, n])
                sampler(case, mu, lv, None, None, pred, gt, None, [0, 0, n])
    n = 5
    for R, K_in in ((4, 16), (5, 13), (1, 257)):
        for Tf in (1, 32, 33):
            M = R * K_in
            gt = np.cumsum(rng.normal(0, 0.4, (n, Tf, 2)), axis=1).astype(np.float32)
            pred = (gt[None, :, None] + rng.normal(0, 0.5, (R, n, K_in, Tf, 2))).astype(np.float32)
            pred[0, 2, 1, 0, 0] = np.nan
            large(f'edge_m{M}_t{Tf}', pred, gt, (1, 20, M), [0, 0, n])
    for R, K_in, K in ((5, 13, 3), (5, 13, 5), (1, 257, 20)):
        for Tf in (1, 12):
            pred = np.cumsum(rng.normal(0, 0.4, (R, n, K_in, Tf, 2)), axis=3).astype(np.float32)
            reductions(f'edge_m{R * K_in}_k{K}_t{Tf}', pred, K, [[0, 0, n], [0, 2, n]])
    torch.cuda.synchronize()
    np.savez(path, **res)
    print(f'{len(res)} arrays of {len({k.split("|")[0] for k in res})} entries -> {path} (library: {capi.LIB_PATH})')


def compare(a_path, b_path, out_path):
    a, b = np.load(a_path), np.load(b_path)
    count = {}
    missing = sorted(set(a.files) ^ set(b.files))
    for k in sorted(set(a.files) & set(b.files)):
        x, y = a[k], b[k]
        e = count.setdefault(k.split('|')[0], [0, 0, 0])
        e[0] += 1
        if x.shape != y.shape or x.dtype != y.dtype:
            e[1] += x.size
            e[2] += x.size
            continue
        u = np.dtype(f'u{x.dtype.itemsize}')
        e[1] += x.size
        e[2] += int((np.ascontiguousarray(x).view(u) != np.ascontiguousarray(y).view(u)).sum())
    lines = [f'{a_path} against {b_path}: arrays as unsigned integers of their item size (NaN payloads included)',
             f'{"entry":28s} {"arrays":>8s} {"values":>10s} {"differing":>10s}']
    lines += [f'{k:28s} {v[0]:8d} {v[1]:10d} {v[2]:10d}' for k, v in sorted(count.items())]
    lines.append(f'arrays in one file only: {len(missing)}' + ''.join('\n  ' + m for m in missing))
    bad = sum(v[2] for v in count.values()) + len(missing)
    lines.append('every count is 0' if bad == 0 else f'DIFFERENT: {bad}')
    text = '\n'.join(lines) + '\n'
    with open(out_path, 'w') as f:
        f.write(text)
    print(text, end='')
    return 1 if bad else 0


if __name__ == '__main__':
    if len(sys.argv) == 3 and sys.argv[1] == 'dump':
        dump(sys.argv[2])
    elif len(sys.argv) == 5 and sys.argv[1] == 'compare':
        sys.exit(compare(*sys.argv[2:]))
    else:
        sys.exit(__doc__)
