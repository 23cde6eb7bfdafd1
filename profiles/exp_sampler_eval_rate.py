"""Stage-2 evaluation rate (test_sampler.py:117-212): evaluate.eval_sampler (Q-net on the lagged launch's stream, pipelined, fused metrics)
at 128 / 512 / 2048 scenes per call, beside eval_scenes on the same data and the composed Sampler.forward loop (Q-net on linear_cols, five-
kernel decode; one batch per call), all in one process.  Usage: python profiles/exp_sampler_eval_rate.py [n_scenes] [repeats]"""
import sys
import time

import numpy as np
import torch

sys.path.insert(0, '.')
sys.path.insert(0, 'tests')
from helpers import make_args, sampler_args  # noqa: E402
from sttode_amd import STTODENet, Sampler, datasets, scenes  # noqa: E402
from sttode_amd.evaluate import eval_sampler, eval_scenes  # noqa: E402
from sttode_amd.weights import make_sampler_weights, make_weights, to_torch_state_dict  # noqa: E402

n_scenes = int(sys.argv[1]) if len(sys.argv) > 1 else 12288
repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 2
dev = torch.device('cuda')
m = STTODENet(make_args('eth', 8, 12), dev).eval()
m.load_state_dict(to_torch_state_dict(make_weights(1234)))
smp = Sampler(sampler_args('eth', 8, 12))
smp.load_state_dict(to_torch_state_dict(make_sampler_weights()))
smp.set_device(dev)
smp.eval()


class DS(datasets._SceneDataset):
    def __init__(self, n):
        sb = scenes.make_scene_batch(range(512), 'eth')
        reps = max(1, n // 512)
        cnt = np.tile(np.diff(sb.scene_ptr), reps)
        ends = np.cumsum(cnt)
        self.seq_start_end = list(zip((ends - cnt).tolist(), ends.tolist()))
        self.num_seq = len(cnt)
        self.obs_traj = torch.from_numpy(np.ascontiguousarray(np.tile(sb.past.transpose(0, 2, 1), (reps, 1, 1))))
        self.pred_traj = torch.from_numpy(np.ascontiguousarray(np.tile(sb.future.transpose(0, 2, 1), (reps, 1, 1))))


ds = DS(n_scenes)


def timed(what, fn):
    best = None
    for _ in range(repeats + 1):                       # the first round warms up (packing, workspaces, code objects)
        torch.manual_seed(0)
        torch.cuda.synchronize()
        t = time.perf_counter()
        a, f, n = fn()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t
        if _ > 0 and (best is None or dt < best):
            best = dt
    print(f'{what:<44s} {len(ds)} scenes, {n} agents: {best * 1e3:8.1f} ms  {n * 20 / best / 1e6:6.1f} M trajectories/s  ADE {a:.4f} FDE {f:.4f}',
          flush=True)
    return n * 20 / best


def composed(spc):
    """The composed stage-2 path: per batch set_scene_batch + Sampler.forward (mean) + best_of_k."""
    tot_a = tot_f = 0.0
    tot_n = 0
    with torch.no_grad():
        for s0 in range(0, len(ds), spc):
            sb = ds.scene_batch(range(s0, min(s0 + spc, len(ds))))
            m.set_scene_batch(sb.past, sb.future, sb.scene_ptr)
            dec = smp.forward(m, mean=True)[0]
            ade, fde = m.best_of_k(dec, scale=1.0)
            tot_a += float(ade.double().sum())
            tot_f += float(fde.double().sum())
            tot_n += sb.n_agents
    return tot_a / tot_n, tot_f / tot_n, tot_n


if len(sys.argv) > 3 and sys.argv[3] == 'trace':
    for _ in range(repeats + 1):
        print(eval_sampler(m, smp, ds, scenes_per_call=512), flush=True)
    torch.cuda.synchronize()
    sys.exit(0)
rates = {}
for spc in (128, 512, 2048):
    rates[('scenes', spc)] = timed(f'eval_scenes  scenes_per_call={spc}', lambda: eval_scenes(m, ds, scenes_per_call=spc))
    rates[('sampler', spc)] = timed(f'eval_sampler scenes_per_call={spc}', lambda: eval_sampler(m, smp, ds, scenes_per_call=spc))
rates[('composed', 512)] = timed('Sampler.forward loop  scenes_per_call=512', lambda: composed(512))
for spc in (128, 512, 2048):
    print(f'eval_sampler / eval_scenes at {spc} scenes per call: {rates[("sampler", spc)] / rates[("scenes", spc)]:.3f}')
print(f'eval_sampler / Sampler.forward loop at 512: {rates[("sampler", 512)] / rates[("composed", 512)]:.2f}x')
