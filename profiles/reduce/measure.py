"""Oversample and reduce on the MI355X: 512 ETH-shaped scenes (the benchmark's headline batch), rounds = 50 calls of
K_in = 20 samples (M = 1000 per agent) reduced to K = 20 by 10 Lloyd iterations.  In ONE process, alternating, `--passes` times each:

  reduced     evaluate.eval_scenes_reduced (pipelined): 50 generating calls, the reduction, the selection;
  generation  the same loop with the reduction removed (metrics.reduce_samples replaced by a stub that hands back round 0);
  kernel      metrics.reduce_samples alone on the round buffer the loop filled (HIP events), whole trajectories and endpoints,
              'first' and 'maximin';
  torch       a torch.cdist / argmin / index_add_ composition of the same ten iterations on the same tensor (HIP events), and the share
              of labels on which it agrees with the kernel (it uses the expanded distance form: near-ties differ, the figure is a cost
              comparison, not a check).

    python profiles/reduce/measure.py [--out FILE] [--passes 3] [--scenes 512] [--rounds 50] [--once]

--once: one warmed call of each reduction form and nothing else (for `rocprofv3 --kernel-trace --stats`).
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
from helpers import make_args  # noqa: E402
from sttode_amd import STTODENet, evaluate, metrics, scenes  # noqa: E402
from sttode_amd.weights import make_weights, to_torch_state_dict  # noqa: E402


class Scenes:
    """The smallest thing eval_scenes_reduced takes: len() and scene_batch(indices)."""

    def __init__(self, ids):
        self.sb = scenes.make_scene_batch(ids, 'eth')

    def __len__(self):
        return self.sb.n_scenes

    def scene_batch(self, idx):
        idx = list(idx)
        return self.sb.slice_scenes(idx[0], idx[-1] + 1)


def torch_kmeans(x, K, iters):
    """x [n, M, D] -> (centroids [n, K, D], labels [n, M]): Lloyd from the first K samples with torch ops."""
    n, M, D = x.shape
    c = x[:, :K].clone()
    base = (torch.arange(n, device=x.device) * K)[:, None]
    flat = x.reshape(n * M, D)
    for _ in range(iters):
        lab = torch.cdist(x, c).argmin(dim=2)
        idx = (lab + base).reshape(-1)
        sums = torch.zeros(n * K, D, device=x.device).index_add_(0, idx, flat)
        cnt = torch.bincount(idx, minlength=n * K).reshape(n, K, 1)
        c = torch.where(cnt > 0, sums.reshape(n, K, D) / cnt.clamp(min=1), c)
    return c, lab


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--passes', type=int, default=3)
    ap.add_argument('--scenes', type=int, default=512)
    ap.add_argument('--rounds', type=int, default=50)
    ap.add_argument('--once', action='store_true')
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    m = STTODENet(make_args('eth', 8, 12), dev).eval()
    m.load_state_dict(to_torch_state_dict(make_weights(1234)), strict=True)
    ds = Scenes(range(a.scenes))
    n, Ks, K, iters = ds.sb.n_agents, m.args.sample_k, 20, 10
    kw = dict(K=K, iters=iters, scenes_per_call=a.scenes)
    real = metrics.reduce_samples

    def stub(pred, K, **_):
        class R:
            centroids = pred[0, :, :K]
        return R

    def loop(reduced):
        metrics.reduce_samples = real if reduced else stub
        try:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rep = evaluate.eval_scenes_reduced(m, ds, a.rounds, **kw)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3, rep
        finally:
            metrics.reduce_samples = real

    loop(True)                                                          # warm: packing, workspaces, the round buffer
    buf = m._round_buffer(a.rounds, n)                                  # [rounds, n, Ks, Tf, 2] as the loop left it
    forms = {'whole_first': dict(from_frame=0, init='first'), 'whole_maximin': dict(from_frame=0, init='maximin'),
             'endpoint_first': dict(from_frame=-1, init='first'), 'endpoint_maximin': dict(from_frame=-1, init='maximin')}
    for f in forms.values():
        real(buf, K, iters=iters, **f)
    torch.cuda.synchronize()
    if a.once:
        print('once: done')
        return
    x = buf.permute(1, 0, 2, 3, 4).reshape(n, a.rounds * Ks, -1).contiguous()
    torch_kmeans(x, K, iters)
    res = {'scenes': a.scenes, 'agents': n, 'rounds': a.rounds, 'K_in': Ks, 'M': a.rounds * Ks, 'K': K, 'iters': iters, 'passes': []}
    for _ in range(a.passes):
        row = {}
        row['reduced_loop_ms'], rep = loop(True)
        row['generation_only_ms'], rep0 = loop(False)
        for name, f in forms.items():
            row['kernel_%s_ms' % name], red = event_ms(lambda: real(buf, K, iters=iters, **f))
            if name == 'whole_first':
                first = red
        row['torch_composition_ms'], (tc, tl) = event_ms(lambda: torch_kmeans(x, K, iters))
        row['torch_label_agreement'] = float((tl == first.labels).float().mean())
        row['ade_reduced'], row['ade_round0'] = rep.ade, rep0.ade
        res['passes'].append(row)
        print(json.dumps(row), flush=True)
    keys = [k for k in res['passes'][0] if k.endswith('_ms')]
    res['median'] = {k: float(np.median([p[k] for p in res['passes']])) for k in keys}
    res['reduction_share_of_generation'] = res['median']['kernel_whole_first_ms'] / res['median']['generation_only_ms']
    flop = 3.0 * a.rounds * Ks * K * 2 * m.args.future_length * n * iters
    res['assign_gflop'] = flop / 1e9
    res['assign_tflops_whole_first'] = flop / (res['median']['kernel_whole_first_ms'] * 1e-3) / 1e12
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, 'w').write(txt + '\n')


if __name__ == '__main__':
    main()
