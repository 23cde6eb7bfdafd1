"""Cost of the weighted-set pass (csrc/weighted.hip weighted_set_kernel) beside the two unweighted passes whose pair and KDE
work it does in one launch.  Writes profiles/weighted_set/rates.txt (or --out); needs a GPU (no fallback).

    python profiles/weighted_set/measure.py

Two sizes: the 8 729 agents of 512 ETH-shaped scenes at K = 20, Tf = 12 (the size every pass of this family is measured at), and the same
agents at K = 64, Tf = 40.  Weights: cluster counts of 2 K draws (some zero).  Per size, on the same tensors: sttode_weighted_set,
sttode_sample_spread, sttode_kde_nll, each warmed, then `--reps` windows of `--launches` back-to-back launches between two device events;
the median window / launches is the kernel's time (launch gaps included: the kernels are short).  The three are measured twice, alternated,
so that a drift of the box shows.  ratio = weighted_set / (sample_spread + kde_nll).
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def event_median(fn, launches, reps):
    import numpy as np
    import torch
    for _ in range(20):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(launches):
            fn()
        e1.record()
        e1.synchronize()
        us.append(1e3 * e0.elapsed_time(e1) / launches)
    return float(np.median(us)), float(min(us)), float(max(us))


def measure(K, Tf, a, lines):
    import numpy as np
    import torch
    from sttode_amd import capi, metrics, scenes
    dev = torch.device('cuda:0')
    sb = scenes.make_scene_batch(range(20000, 20512), 'eth')
    n = sb.n_agents
    rng = np.random.default_rng(0)
    fut = sb.future if Tf == sb.future.shape[1] else np.cumsum(rng.normal(0, 0.4, (n, Tf, 2)), axis=1).astype(np.float32)
    gt = torch.from_numpy(fut).to(dev)
    drift = rng.normal(0, 1.0, (n, K, 1, 2)) * np.linspace(0.3, 1.0, Tf)[None, None, :, None]
    pred = (gt[:, None] + torch.from_numpy((drift + rng.normal(0, 0.1, (n, K, Tf, 2))).astype(np.float32)).to(dev)).contiguous()
    share = rng.dirichlet(np.full(K, 0.4), n)
    w_np = np.stack([rng.multinomial(2 * K, s) for s in share]).astype(np.float32)
    w = torch.from_numpy(w_np).to(dev)
    st = capi.stream_ptr()
    ws = metrics.WeightedSet(n, K, dev)
    ss = metrics.SampleSpread(n, K, dev, 1.0, True)
    nll = torch.empty(n, dtype=torch.float64, device=dev)
    fns = {'weighted_set': lambda: capi.call('sttode_weighted_set', pred, w, gt, n, K, Tf, 1.0, *ws.args(), st),
           'sample_spread': lambda: capi.call('sttode_sample_spread', pred, gt, n, K, Tf, 1.0, *ss.args(), st),
           'kde_nll': lambda: capi.call('sttode_kde_nll', pred, gt, n, K, Tf, 1.0, nll, st)}
    lines.append(f'agents {n}, K {K}, Tf {Tf}; weights: counts of {2 * K} draws, {float((w_np == 0).mean()):.2f} of them zero; '
                 f'{a.reps} windows of {a.launches} launches, median (min .. max) us per launch')
    med = {}
    for rnd in (1, 2):
        for name in ('weighted_set', 'sample_spread', 'kde_nll'):
            m, lo, hi = event_median(fns[name], a.launches, a.reps)
            med.setdefault(name, []).append(m)
            lines.append(f'  round {rnd}  {name:14s} {m:8.2f} ({lo:.2f} .. {hi:.2f})')
    t = {k: float(np.median(v)) for k, v in med.items()}
    lines.append(f'  weighted_set {t["weighted_set"]:.2f} us; sample_spread + kde_nll {t["sample_spread"] + t["kde_nll"]:.2f} us; '
                 f'ratio {t["weighted_set"] / (t["sample_spread"] + t["kde_nll"]):.3f}')
    out = metrics.weighted_set(pred, w, gt)
    lines.append('  means over agents: eade %.4f, es_ade %.4f, neff %.2f, kde_nll NaN agents %d' % (
        float(out.eade.mean()), float(out.es_ade.mean()), float(out.neff.mean()), int(torch.isnan(out.kde_nll).sum())))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--launches', type=int, default=200)
    ap.add_argument('--reps', type=int, default=15)
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.abspath(__file__)), 'rates.txt'))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        print('no GPU: nothing measured', file=sys.stderr)
        return 1
    lines = ['weighted_set_kernel beside sample_spread_kernel + kde_nll_kernel on the same tensors (' + torch.cuda.get_device_name(0) + ')']
    for K, Tf in ((20, 12), (64, 40)):
        measure(K, Tf, a, lines)
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text)
    return 0


if __name__ == '__main__':
    sys.exit(main())
