"""Cost of the scene-level metric passes (csrc/metrics.hip) on the evaluation loops: evaluate.eval_scenes_report with the new
options off and with all of them on (joint=True, kde=True, collision_radius=0.2), alternated, on one synthetic ETH-shaped dataset at 512
scenes per call; then eval_nba_report the same way at bench.py's nba_128 shape (loader batches of 128 games x 11 players, obs 5 / pred 10).
Each loop is timed from a device synchronise to a device synchronise.  Prints one JSON line.

    python profiles/exp_scene_metrics_rate.py [--calls 16] [--rounds 3]
    rocprofv3 --kernel-trace --stats -d <dir> -- python profiles/exp_scene_metrics_rate.py --once     # one loop with everything on
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
sys.path.insert(0, os.path.join(ROOT, 'profiles'))

ON = {'joint': True, 'kde': True, 'collision_radius': 0.2}


def nba_loader(batches, B=128, N=11):
    from sttode_amd import scenes
    out = []
    for i in range(batches):
        d = scenes.nba_batch(7000 + i, B, N=N, obs_len=5, pred_len=10)
        out.append({'past_traj': torch.from_numpy(d['past_traj']), 'future_traj': torch.from_numpy(d['future_traj'])})
    return out


def alternate(rounds, fns):
    t = {name: [] for name in fns}
    for _ in range(rounds):
        for name, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            t[name].append(time.perf_counter() - t0)
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=16, help='512-scene calls per loop')
    ap.add_argument('--nba-batches', type=int, default=32, help='loader batches of 128 games per NBA loop')
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--once', action='store_true', help='one eval_scenes_report loop with every option on (profiling)')
    a = ap.parse_args()
    from exp_selection_rate import dataset
    from helpers import make_args
    from sttode_amd import STTODENet
    from sttode_amd.evaluate import eval_nba_report, eval_scenes_report
    from sttode_amd.weights import make_weights, to_torch_state_dict
    torch.manual_seed(0)
    m = STTODENet(make_args('eth', 8, 12), torch.device('cuda:0')).eval()
    m.load_state_dict(to_torch_state_dict(make_weights(1234)), strict=True)
    ds = dataset(512 * a.calls)
    n = int(ds.obs_traj.shape[0])
    traj = n * m.args.sample_k
    if a.once:
        rep = eval_scenes_report(m, ds, scenes_per_call=512, **ON)
        torch.cuda.synchronize()
        print(json.dumps({'calls': a.calls, 'agents': n, 'ade': rep.ade, 'joint_ade': rep.joint_ade, 'collision_rate': rep.collision_rate,
                          'kde_nll': rep.kde_nll, 'kde_invalid': rep.kde_invalid}))
        return
    eval_scenes_report(m, ds, scenes_per_call=512)                      # warm-up of every shape both loops use
    rep = eval_scenes_report(m, ds, scenes_per_call=512, **ON)
    t = alternate(a.rounds, {'off': lambda: eval_scenes_report(m, ds, scenes_per_call=512),
                             'on': lambda: eval_scenes_report(m, ds, scenes_per_call=512, **ON)})
    out = {'eth': {'calls': a.calls, 'scenes_per_call': 512, 'agents': n, 'trajectories': traj, 'options_on': ON,
                   'joint_ade': rep.joint_ade, 'collision_rate': rep.collision_rate, 'gt_collision_rate': rep.gt_collision_rate,
                   'kde_nll': rep.kde_nll, 'kde_invalid': rep.kde_invalid}}
    for name, v in t.items():
        out['eth'][name] = {'seconds': v, 'best_traj_per_s': traj / min(v), 'median_ms_per_call': 1e3 * float(np.median(v)) / a.calls}
    out['eth']['on_over_off_median'] = float(np.median(t['on']) / np.median(t['off']))
    mn = STTODENet(make_args('nba', 5, 10), torch.device('cuda:0')).eval()
    mn.load_state_dict(to_torch_state_dict(make_weights(1234, past_length=5, future_length=10)), strict=True)
    loader = nba_loader(a.nba_batches)
    eval_nba_report(mn, loader)
    eval_nba_report(mn, loader, **ON)
    t = alternate(a.rounds, {'off': lambda: eval_nba_report(mn, loader), 'on': lambda: eval_nba_report(mn, loader, **ON)})
    ntraj = a.nba_batches * 128 * 11 * mn.args.sample_k
    out['nba'] = {'loader_batches': a.nba_batches, 'games_per_batch': 128, 'players': 11, 'trajectories': ntraj}
    for name, v in t.items():
        out['nba'][name] = {'seconds': v, 'best_traj_per_s': ntraj / min(v)}
    out['nba']['on_over_off_median'] = float(np.median(t['on']) / np.median(t['off']))
    print(json.dumps(out))


if __name__ == '__main__':
    main()
