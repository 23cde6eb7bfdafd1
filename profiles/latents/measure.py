"""Latent sets on the MI355X.  In ONE process, by HIP events after a warm-up:

  draw        latents.draw at the benchmark's headline shape, 8 729 agents x K = 20 x zdim = 32 (512 ETH-shaped scenes), for the default
              (Sobol, nested uniform scrambling), the digital shift, the i.i.d. kind and antithetic + centred + truncated; and at
              rounds = 20 (M = 400 points per agent)
  randn       torch.randn of the same size on the device, beside it
  host sobol  torch.quasirandom.SobolEngine on the host (ONE scrambled sequence of n K points, not one per agent -- it has no such
              notion), ndtri, and the copy to the device: host clock around a synchronise, `--host-passes` times
  eval        evaluate.eval_scenes over 512 ETH-shaped scenes with the default latents (torch.randn) and with a LatentSource as z_fn,
              pipelined, in alternating pairs, at 512 and at 64 scenes per call (wall clock, host packing of the batches included)

and, labelled as what it is -- the SEEDED RANDOM-WEIGHT model on the synthetic scenes, no accuracy claim (the tree has no trained
checkpoint) -- mean and standard deviation over 8 seeds of best-of-20 ADE / FDE for i.i.d. (torch.randn), Sobol, and Sobol + antithetic.

    python profiles/latents/measure.py [--out FILE] [--passes 20] [--pairs 6] [--scenes 512]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from sttode_amd import STTODENet, datasets, latents, scenes  # noqa: E402
from sttode_amd.evaluate import eval_scenes  # noqa: E402
from sttode_amd.weights import make_weights, to_torch_state_dict  # noqa: E402


def timed(fn, passes, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(passes):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return {'median_ms': float(np.median(ms)), 'min_ms': float(min(ms)), 'max_ms': float(max(ms))}


def host_timed(fn, passes):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(passes):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0))
    return {'median_ms': float(np.median(ms)), 'min_ms': float(min(ms)), 'max_ms': float(max(ms))}


class Scenes(datasets._SceneDataset):
    def __init__(self, ids):
        sb = scenes.make_scene_batch(ids, 'eth')
        cnt = np.diff(sb.scene_ptr)
        ends = np.cumsum(cnt)
        self.seq_start_end = list(zip((ends - cnt).tolist(), ends.tolist()))
        self.num_seq = len(cnt)
        self.obs_traj = torch.from_numpy(np.ascontiguousarray(sb.past.transpose(0, 2, 1)))
        self.pred_traj = torch.from_numpy(np.ascontiguousarray(sb.future.transpose(0, 2, 1)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--passes', type=int, default=20)
    ap.add_argument('--host-passes', type=int, default=3)
    ap.add_argument('--pairs', type=int, default=6)
    ap.add_argument('--scenes', type=int, default=512)
    ap.add_argument('--seeds', type=int, default=8)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('profiles/latents/measure.py needs the GPU: nothing here is measured without one')
    from helpers import make_args
    dev = torch.device('cuda:0')
    ds = Scenes(range(a.scenes))
    n, K, zdim = int(ds.obs_traj.shape[0]), 20, 32
    res = {'scenes': a.scenes, 'agents': n, 'K': K, 'zdim': zdim, 'passes': a.passes}
    for name, kw in (('sobol_owen', {}), ('sobol_shift', dict(scramble='shift')), ('random', dict(kind='random')),
                     ('sobol_owen_antithetic_center_truncate2', dict(antithetic=True, center=True, truncate=2.0)),
                     ('sobol_owen_bits', dict(return_bits=True))):
        res['draw_' + name] = timed(lambda: latents.draw(n, K, zdim, seed=1, device=dev, **kw), a.passes)
    res['randn'] = timed(lambda: torch.randn(n * K, zdim, device=dev), a.passes)
    res['draw_sobol_owen_rounds20'] = timed(lambda: latents.draw(n, K, zdim, rounds=20, seed=1, device=dev), a.passes)
    res['draw_random_rounds20'] = timed(lambda: latents.draw(n, K, zdim, rounds=20, seed=1, kind='random', device=dev), a.passes)
    res['randn_rounds20'] = timed(lambda: torch.randn(20, n * K, zdim, device=dev), a.passes)
    res['values_per_draw'] = n * K * zdim

    def host_sobol(points):
        u = torch.quasirandom.SobolEngine(zdim, scramble=True, seed=1).draw(points, dtype=torch.float64)
        return torch.special.ndtri(u.clamp(2.0 ** -33, 1.0 - 2.0 ** -33)).float().to(dev)
    res['host_sobolengine_ndtri_copy'] = host_timed(lambda: host_sobol(n * K), a.host_passes)
    print(json.dumps(res), flush=True)

    m = STTODENet(make_args('eth', 8, 12), dev).eval()
    m.load_state_dict(to_torch_state_dict(make_weights(1234)), strict=True)
    src = latents.LatentSource(K, zdim, seed=7, device=dev)

    def rate(z_fn, per_call):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eval_scenes(m, ds, z_fn=z_fn, pipelined=True, scenes_per_call=per_call)
        torch.cuda.synchronize()
        return n * K / (time.perf_counter() - t0) / 1e6
    for per_call in (512, 64):                                           # one call per pass, and eight calls in flight behind one another
        for _ in range(2):
            rate(None, per_call), rate(src, per_call)
        pairs = []
        for _ in range(a.pairs):
            pairs.append({'default_Mtraj_s': rate(None, per_call), 'source_Mtraj_s': rate(src, per_call)})
        key = 'eval_scenes_pipelined_%d_per_call' % per_call
        res[key + '_pairs'] = pairs
        res[key + '_median'] = {k: float(np.median([p[k] for p in pairs])) for k in pairs[0]}
        print(json.dumps({key: res[key + '_median']}), flush=True)

    # seeded random-weight model, synthetic scenes: NOT an accuracy result
    acc = {}
    for name, make in (('iid_randn', lambda sd: None), ('sobol_owen', lambda sd: latents.LatentSource(K, zdim, seed=sd, device=dev)),
                       ('sobol_owen_antithetic', lambda sd: latents.LatentSource(K, zdim, seed=sd, antithetic=True, device=dev))):
        vals = []
        for sd in range(a.seeds):
            torch.manual_seed(1000 + sd)
            ade, fde, _ = eval_scenes(m, ds, z_fn=make(1000 + sd), pipelined=True)
            vals.append((ade, fde))
        v = np.array(vals)
        acc[name] = {'ade_mean': float(v[:, 0].mean()), 'ade_std': float(v[:, 0].std(ddof=1)), 'fde_mean': float(v[:, 1].mean()),
                     'fde_std': float(v[:, 1].std(ddof=1))}
    res['best_of_20_random_weight_model_synthetic_scenes_no_accuracy_claim'] = acc
    txt = json.dumps(res, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, 'w').write(txt + '\n')
    print(txt)


if __name__ == '__main__':
    main()
