"""Scene-level oversample and reduce on the MI355X: 512 ETH-shaped scenes (the benchmark's headline batch), rounds = 20
calls of K_in = 20 samples (M = 400 scene futures per scene) reduced to K = 20 by 10 Lloyd iterations.  In ONE process, on ONE round buffer
(filled by evaluate.eval_scenes_reduced), alternating, `--passes` times each, by HIP events:

  scenes      metrics.reduce_scenes over the batch's scene_ptr: whole trajectories and endpoints, 'first' and 'maximin';
  agents      metrics.reduce_samples on the same buffer, the same four forms (the per-agent kernel: the same per-agent arithmetic, one
              workgroup per agent instead of one per scene);
  singles     metrics.reduce_scenes with one-agent segments (the scene kernel doing the per-agent kernel's work, bits included);
  one_segment metrics.reduce_scenes of the first `--segment` agents (default 300) as ONE segment: one workgroup, the size limit of nothing.

    python profiles/reduce_scenes/measure.py [--out FILE] [--passes 5] [--scenes 512] [--rounds 20] [--segment 300] [--once]

--once: one warmed call of each form and nothing else (for `rocprofv3 --kernel-trace --stats`).
"""
import argparse
import json
import os
import sys

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
    ap.add_argument('--passes', type=int, default=5)
    ap.add_argument('--scenes', type=int, default=512)
    ap.add_argument('--rounds', type=int, default=20)
    ap.add_argument('--segment', type=int, default=300)
    ap.add_argument('--once', action='store_true')
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    m = STTODENet(make_args('eth', 8, 12), dev).eval()
    m.load_state_dict(to_torch_state_dict(make_weights(1234)), strict=True)
    ds = Scenes(range(a.scenes))
    n, Ks, K, iters = ds.sb.n_agents, m.args.sample_k, 20, 10
    evaluate.eval_scenes_reduced(m, ds, a.rounds, K=K, iters=iters, scenes_per_call=a.scenes, level='scene', joint=True)   # fills the round buffer
    buf = m._round_buffer(a.rounds, n)                                  # [rounds, n, Ks, Tf, 2] as the loop left it
    sp = torch.as_tensor(ds.sb.scene_ptr, dtype=torch.int32).to(dev)
    singles = torch.arange(n + 1, dtype=torch.int32, device=dev)
    A = min(a.segment, n)
    seg_buf = buf[:, :A].contiguous()
    seg_sp = torch.tensor([0, A], dtype=torch.int32, device=dev)
    forms = {'whole_first': dict(from_frame=0, init='first'), 'whole_maximin': dict(from_frame=0, init='maximin'),
             'endpoint_first': dict(from_frame=-1, init='first'), 'endpoint_maximin': dict(from_frame=-1, init='maximin')}
    calls = {}
    for name, f in forms.items():
        calls['scenes_' + name] = lambda f=f: metrics.reduce_scenes(buf, sp, K, iters=iters, **f)
        calls['agents_' + name] = lambda f=f: metrics.reduce_samples(buf, K, iters=iters, **f)
    calls['singles_whole_first'] = lambda: metrics.reduce_scenes(buf, singles, K, iters=iters)
    calls['one_segment_whole_first'] = lambda: metrics.reduce_scenes(seg_buf, seg_sp, K, iters=iters)
    calls['one_segment_whole_maximin'] = lambda: metrics.reduce_scenes(seg_buf, seg_sp, K, iters=iters, init='maximin')
    for fn in calls.values():
        fn()
    torch.cuda.synchronize()
    if a.once:
        print('once: done')
        return
    one = metrics.reduce_scenes(buf, singles, K, iters=iters)
    per = metrics.reduce_samples(buf, K, iters=iters)
    res = {'scenes': a.scenes, 'agents': n, 'largest_scene': int(np.diff(ds.sb.scene_ptr).max()), 'rounds': a.rounds, 'K_in': Ks,
           'M': a.rounds * Ks, 'K': K, 'iters': iters, 'one_segment_agents': A,
           'singles_have_the_bits_of_reduce_samples': bool(torch.equal(one.centroids, per.centroids) and torch.equal(one.labels, per.labels)),
           'passes': []}
    for _ in range(a.passes):
        row = {name + '_ms': event_ms(fn)[0] for name, fn in calls.items()}
        res['passes'].append(row)
        print(json.dumps(row), flush=True)
    res['median'] = {k: float(np.median([p[k] for p in res['passes']])) for k in res['passes'][0]}
    med = res['median']
    res['scenes_over_agents'] = {name: med['scenes_%s_ms' % name] / med['agents_%s_ms' % name] for name in forms}
    res['singles_over_agents_whole_first'] = med['singles_whole_first_ms'] / med['agents_whole_first_ms']
    flop = 3.0 * a.rounds * Ks * K * 2 * m.args.future_length * n * iters
    res['assign_gflop'] = flop / 1e9
    res['assign_tflops'] = {k: flop / (med[k + '_whole_first_ms'] * 1e-3) / 1e12 for k in ('scenes', 'agents')}
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, 'w').write(txt + '\n')


if __name__ == '__main__':
    main()
