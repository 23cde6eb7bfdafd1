"""Cost of the sample-spread pass (csrc/metrics.hip sample_spread_kernel).  One job of two steps, each a fresh child process
under its own time limit; the job stops at the first step that fails.  Writes profiles/sample_spread/rate.json (or --out).

    python profiles/sample_spread/measure.py                 # both steps
    python profiles/sample_spread/measure.py --step kernel   # one step, prints its JSON line

  kernel  512 ETH-shaped scenes, K = 20, Tf = 12: sttode_sample_spread (with and without a ground truth) and, on the same tensors,
          sttode_kde_nll and sttode_best_of_k_select; each warmed, then `--reps` windows of `--launches` back-to-back launches between two
          device events; the median window / launches is the kernel's time (launch gaps included: the kernels are short).
  loop    evaluate.eval_scenes_report with spread off / on, alternated, `--calls` calls of 512 scenes, each loop timed from a device
          synchronise to a device synchronise (as profiles/exp_scene_metrics_rate.py).
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'profiles'))

LIMITS = {'kernel': 240, 'loop': 420}   # seconds per step


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
    return {'median_us': float(np.median(us)), 'min_us': float(min(us)), 'max_us': float(max(us))}


def step_kernel(a):
    import numpy as np
    import torch
    from sttode_amd import metrics, scenes
    dev = torch.device('cuda:0')
    sb = scenes.make_scene_batch(range(20000, 20512), 'eth')
    n, K, Tf = sb.n_agents, 20, 12
    rng = np.random.default_rng(0)
    gt = torch.from_numpy(sb.future).to(dev)
    drift = rng.normal(0, 1.0, (n, K, 1, 2)) * np.linspace(0.3, 1.0, Tf)[None, None, :, None]
    pred = (gt[:, None] + torch.from_numpy((drift + rng.normal(0, 0.1, (n, K, Tf, 2))).astype(np.float32)).to(dev)).contiguous()
    out = {'scenes': 512, 'agents': n, 'K': K, 'Tf': Tf, 'launches_per_window': a.launches, 'windows': a.reps}
    # preallocated outputs and the entry points themselves: the host's share of a launch is one ctypes call
    from sttode_amd import capi
    st = capi.stream_ptr()
    ss = metrics.SampleSpread(n, K, dev, 1.0, True)
    s0 = metrics.SampleSpread(n, K, dev, 1.0, False)
    nll = torch.empty(n, dtype=torch.float64, device=dev)
    sel = metrics.Selection(n, 0, Tf, dev, False)
    fns = {'sample_spread': lambda: capi.call('sttode_sample_spread', pred, gt, n, K, Tf, 1.0, *ss.args(), st),
           'sample_spread_no_gt': lambda: capi.call('sttode_sample_spread', pred, None, n, K, Tf, 1.0, *s0.args(), st),
           'kde_nll': lambda: capi.call('sttode_kde_nll', pred, gt, n, K, Tf, 1.0, nll, st),
           'select': lambda: capi.call('sttode_best_of_k_select', pred, gt, n, K, Tf, 1.0, 1.0, None, 0, *sel.args(), st)}
    for name in ('sample_spread', 'sample_spread_no_gt', 'kde_nll', 'select', 'sample_spread'):
        out[name + ('_again' if name in out else '')] = event_median(fns[name], a.launches, a.reps)
    ss = metrics.sample_spread(pred, gt)
    out['apd_mean'], out['dlow_mean'], out['es_ade_mean'] = (float(t.sum().item() / n) for t in (ss.apd, ss.dlow, ss.es_ade))
    return out


def step_loop(a):
    import numpy as np
    import torch
    from exp_selection_rate import dataset
    from helpers import make_args
    from sttode_amd import STTODENet
    from sttode_amd.evaluate import eval_scenes_report
    from sttode_amd.weights import make_weights, to_torch_state_dict
    torch.manual_seed(0)
    m = STTODENet(make_args('eth', 8, 12), torch.device('cuda:0')).eval()
    m.load_state_dict(to_torch_state_dict(make_weights(1234)), strict=True)
    ds = dataset(512 * a.calls)
    n = int(ds.obs_traj.shape[0])
    eval_scenes_report(m, ds, scenes_per_call=512)                      # warm-up of every shape both loops use
    rep = eval_scenes_report(m, ds, scenes_per_call=512, spread=True)
    t = {'off': [], 'on': []}
    for _ in range(a.rounds):
        for name, kw in (('off', {}), ('on', {'spread': True})):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eval_scenes_report(m, ds, scenes_per_call=512, **kw)
            torch.cuda.synchronize()
            t[name].append(time.perf_counter() - t0)
    out = {'calls': a.calls, 'scenes_per_call': 512, 'agents': n, 'trajectories': n * m.args.sample_k, 'rounds': a.rounds,
           'apd': rep.apd, 'fpd': rep.fpd, 'dlow': rep.dlow, 'energy_ade': rep.energy_ade, 'ade_at_k': {str(k): v for k, v in rep.ade_at_k.items()},
           'ade': rep.ade}
    for name, v in t.items():
        out[name] = {'seconds': v, 'median_ms_per_call': 1e3 * float(np.median(v)) / a.calls}
    out['on_over_off_median'] = float(np.median(t['on']) / np.median(t['off']))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--step', choices=sorted(LIMITS))
    ap.add_argument('--launches', type=int, default=200)
    ap.add_argument('--reps', type=int, default=15)
    ap.add_argument('--calls', type=int, default=16)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.abspath(__file__)), 'rate.json'))
    a = ap.parse_args()
    if a.step:
        print(json.dumps({'kernel': step_kernel, 'loop': step_loop}[a.step](a)))
        return 0
    res = {}
    for step in ('kernel', 'loop'):
        cmd = [sys.executable, os.path.abspath(__file__), '--step', step, '--launches', str(a.launches), '--reps', str(a.reps), '--calls',
               str(a.calls), '--rounds', str(a.rounds)]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=LIMITS[step])
        except subprocess.TimeoutExpired:
            print(f'step {step}: no result within {LIMITS[step]} s; stopping', file=sys.stderr)
            return 124
        if p.returncode != 0:
            print(f'step {step}: exit status {p.returncode}; stopping\n{p.stderr[-4000:]}', file=sys.stderr)
            return p.returncode if p.returncode > 0 else 1
        res[step] = json.loads(p.stdout.strip().splitlines()[-1])
        print(step, json.dumps(res[step]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(json.dumps(res) + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
