"""Cost of the multi-modal ground truth pass (csrc/multimodal.hip).  Writes profiles/multimodal/rate.json (or --out).

    python profiles/multimodal/measure.py

The agents of 512 ETH-shaped scenes (the benchmark's dataset size), K = 20, Tp = 8, Tf = 12, hist_frames = 7.  eps is the first of a doubling
ladder at which the mean neighbour count lies in [5, 50].  sttode_multimodal (its two launches) at that eps, at eps = 0 (the neighbour search
alone: every agent scores its own future only) and at 4 eps, and on the same tensors sttode_kde_nll and sttode_sample_spread; each warmed,
then `--reps` windows of `--launches` back-to-back calls between two device events; the median window / launches is the time.  The shader
clock (sttode_clock_probe) is read behind every measurement.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def event_median(fn, launches, reps, warm):
    import numpy as np
    import torch
    from sttode_amd import capi
    for _ in range(warm):
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
    clk = torch.zeros(2, dtype=torch.int64, device='cuda:0')
    capi.call('sttode_clock_probe', clk, capi.stream_ptr())
    c = clk.tolist()
    return {'median_us': float(np.median(us)), 'min_us': float(min(us)), 'max_us': float(max(us)), 'clock_ghz': c[0] / (10.0 * c[1]) if c[1] else None}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--scenes', type=int, default=512)
    ap.add_argument('--launches', type=int, default=10)
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.abspath(__file__)), 'rate.json'))
    a = ap.parse_args()
    import numpy as np
    import torch
    from sttode_amd import capi, metrics, scenes
    dev = torch.device('cuda:0')
    sb = scenes.make_scene_batch(range(20000, 20000 + a.scenes), 'eth')
    n, K, Tp, Tf, h = sb.n_agents, 20, int(sb.past.shape[1]), int(sb.future.shape[1]), int(sb.past.shape[1]) - 1
    rng = np.random.default_rng(0)
    past, gt = torch.from_numpy(sb.past).to(dev), torch.from_numpy(sb.future).to(dev)
    drift = rng.normal(0, 1.0, (n, K, 1, 2)) * np.linspace(0.3, 1.0, Tf)[None, None, :, None]
    pred = (gt[:, None] + torch.from_numpy((drift + rng.normal(0, 0.1, (n, K, Tf, 2))).astype(np.float32)).to(dev)).contiguous()
    eps, ladder = None, []
    for e in (0.025 * 2 ** i for i in range(12)):
        mc = float(metrics.multimodal(pred, past, gt, e).count.double().mean().item())
        ladder.append([e, mc])
        if 5.0 <= mc <= 50.0:
            eps = e
            break
    if eps is None:
        raise SystemExit(f'no eps of the ladder gives a mean count in [5, 50]: {ladder}')
    out = {'scenes': a.scenes, 'agents': n, 'K': K, 'Tp': Tp, 'Tf': Tf, 'hist_frames': h, 'eps': eps, 'eps_ladder': ladder,
           'launches_per_window': a.launches, 'windows': a.reps}
    st = capi.stream_ptr()
    mm = metrics.MultiModal(n, dev, eps, h)
    ws = torch.empty((2 * h + 2) * n, dtype=torch.float64, device=dev)
    nll = torch.empty(n, dtype=torch.float64, device=dev)
    ss = metrics.SampleSpread(n, K, dev, 1.0, True)

    def multimodal(e):
        return lambda: capi.call('sttode_multimodal', pred, past, gt, None, 0, n, K, Tp, Tf, h, 1.0, e, ws, int(ws.numel()), *mm.args(), st)
    fns = [('multimodal', multimodal(eps)), ('multimodal_eps0', multimodal(0.0)), ('multimodal_4eps', multimodal(4 * eps)),
           ('kde_nll', lambda: capi.call('sttode_kde_nll', pred, gt, n, K, Tf, 1.0, nll, st)),
           ('sample_spread', lambda: capi.call('sttode_sample_spread', pred, gt, n, K, Tf, 1.0, *ss.args(), st)),
           ('multimodal_again', multimodal(eps))]
    for name, fn in fns:
        out[name] = event_median(fn, a.launches if name.startswith('multimodal') else 20 * a.launches, a.reps, 3 if name.startswith('multimodal') else 20)
        if name.startswith('multimodal'):
            out[name]['mean_count'] = float(mm.count.double().mean().item())
            out[name]['mmade_mean'] = float(mm.mmade.sum().item() / n)
        print(name, json.dumps(out[name]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(json.dumps(out) + '\n')
    print(json.dumps(out))
    return 0


if __name__ == '__main__':
    sys.exit(main())
