"""Cost of the best-of-K selection pass on the evaluation loop: evaluate.eval_scenes against evaluate.eval_scenes_report (the same pipelined
calls plus one selection pass per call, csrc/frontend.hip sttode_best_of_k_select) on one synthetic ETH-shaped dataset at 512 scenes per
call, alternated, each timed from a device synchronise to a device synchronise.  Prints one JSON line.

    python profiles/exp_selection_rate.py [--calls 16] [--rounds 3]
    rocprofv3 --kernel-trace --stats -d <dir> -- python profiles/exp_selection_rate.py --once     # one report loop, for kernel times
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def dataset(n_scenes):
    from sttode_amd import datasets, scenes

    class DS(datasets._SceneDataset):
        def __init__(self):
            sb = scenes.make_scene_batch(range(20000, 20000 + n_scenes), 'eth')
            cnt = np.diff(sb.scene_ptr)
            ends = np.cumsum(cnt)
            self.seq_start_end = list(zip((ends - cnt).tolist(), ends.tolist()))
            self.num_seq = len(cnt)
            self.obs_traj = torch.from_numpy(np.ascontiguousarray(sb.past.transpose(0, 2, 1)))
            self.pred_traj = torch.from_numpy(np.ascontiguousarray(sb.future.transpose(0, 2, 1)))
    return DS()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=16, help='512-scene calls per loop')
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--once', action='store_true', help='one eval_scenes_report loop only (profiling)')
    a = ap.parse_args()
    from helpers import make_args
    from sttode_amd import STTODENet
    from sttode_amd.evaluate import eval_scenes, eval_scenes_report
    from sttode_amd.weights import make_weights, to_torch_state_dict
    torch.manual_seed(0)
    m = STTODENet(make_args('eth', 8, 12), torch.device('cuda:0')).eval()
    m.load_state_dict(to_torch_state_dict(make_weights(1234)), strict=True)
    ds = dataset(512 * a.calls)
    n = int(ds.obs_traj.shape[0])
    traj = n * m.args.sample_k
    if a.once:
        rep = eval_scenes_report(m, ds, scenes_per_call=512)
        torch.cuda.synchronize()
        print(json.dumps({'calls': a.calls, 'agents': n, 'ade': rep.ade, 'miss_rate': rep.miss_rate}))
        return
    eval_scenes(m, ds, scenes_per_call=512)                             # warm-up of every shape both loops use
    eval_scenes_report(m, ds, scenes_per_call=512)
    t = {'eval_scenes': [], 'eval_scenes_report': []}
    for _ in range(a.rounds):
        for name, fn in (('eval_scenes', eval_scenes), ('eval_scenes_report', eval_scenes_report)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(m, ds, scenes_per_call=512)
            torch.cuda.synchronize()
            t[name].append(time.perf_counter() - t0)
    out = {'calls': a.calls, 'scenes_per_call': 512, 'agents': n, 'trajectories': traj}
    for name, v in t.items():
        out[name] = {'seconds': v, 'best_traj_per_s': traj / min(v), 'median_ms_per_call': 1e3 * float(np.median(v)) / a.calls}
    out['report_over_eval_scenes_median'] = float(np.median(t['eval_scenes_report']) / np.median(t['eval_scenes']))
    print(json.dumps(out))


if __name__ == '__main__':
    main()
