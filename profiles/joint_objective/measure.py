"""Step time of the training step in both best-of-K modes: 'marginal' (the reference's term) and 'joint' (the scene-level
term).  One step = set_data, forward, zero_grad, backward, Adam (train.py:72-95), on two models with the same weights, one per mode, in one
process.  A sample is the wall time of `--steps` steps ending in a device synchronise; the two modes alternate (marginal, joint, marginal,
joint, ...), so a pair shares whatever else the box was doing.  Printed per shape: median (min .. max) per mode, the marginal step's own
pair-to-pair spread, and the paired differences joint - marginal.

    python profiles/joint_objective/measure.py [--steps 300] [--pairs 9] > profiles/joint_objective/rates.txt

Shapes: one ETH scene of 32 agents (Tp 8, Tf 12) and an NBA batch of 32 games x 11 agents (Tp 5, Tf 10)."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=300)
    ap.add_argument('--pairs', type=int, default=9)
    a = ap.parse_args()
    from helpers import make_args
    from sttode_amd import STTODENet, scenes
    from sttode_amd.optim import Adam
    from sttode_amd.weights import make_weights, to_torch_state_dict
    if not torch.cuda.is_available():
        raise SystemExit('measure.py times the GPU: no device found')
    dev = torch.device('cuda:0')

    def stepper(dataset, Tp, Tf, mode):
        m = STTODENet(make_args(dataset, Tp, Tf), dev)
        m.load_state_dict(to_torch_state_dict(make_weights(1234, past_length=Tp, future_length=Tf)), strict=True)
        m.train()
        m.diverse_mode = mode
        opt = Adam(m.parameters(), lr=1e-4)
        if dataset == 'eth':
            ob, pr = (torch.from_numpy(v) for v in scenes.eth_scene(1, n_min=32, n_max=32))
            mk = (torch.ones(32, Tp), torch.ones(32, Tf))
            feed = lambda: m.set_data(None, ob, pr, *mk)
        else:
            d = {k: (torch.from_numpy(v) if isinstance(v, np.ndarray) else v) for k, v in scenes.nba_batch(7, 32).items()}
            feed = lambda: m.set_data_nba(d)
        last = [None]

        def step():
            feed()
            out = m.forward()
            opt.zero_grad()
            out[0].backward()
            opt.step()
            last[0] = out
        return step, last

    print(f'{torch.cuda.get_device_name(0)}; ms per training step (set_data, forward, zero_grad, backward, Adam; graphs replayed), wall time of '
          f'{a.steps} steps ending in a synchronise; {a.pairs} alternating pairs per shape: median (min .. max)')
    for label, dataset, Tp, Tf in (('one scene, 32 agents', 'eth', 8, 12), ('NBA 32 x 11 agents', 'nba', 5, 10)):
        forms = {mode: stepper(dataset, Tp, Tf, mode) for mode in ('marginal', 'joint')}
        ms = {mode: [] for mode in forms}
        for r in range(a.pairs + 1):                                 # pair 0 warms both modes up (eager step, capture, replay)
            for mode, (step, last) in forms.items():
                for _ in range(5 if r == 0 else 0):
                    step()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    step()
                torch.cuda.synchronize()
                if r:
                    ms[mode].append((time.perf_counter() - t0) * 1e3 / a.steps)
        for mode in forms:
            v = ms[mode]
            print(f'{label:22s} {mode:9s} {statistics.median(v):8.4f} ({min(v):.4f} .. {max(v):.4f})   diverse term at the last step '
                  f'{forms[mode][1][0][4]:.4f}')
        diff = [j - m_ for j, m_ in zip(ms['joint'], ms['marginal'])]
        mm = ms['marginal']
        print(f'{label:22s} marginal pair-to-pair spread {max(mm) - min(mm):.4f} ms ({100 * (max(mm) - min(mm)) / statistics.median(mm):.2f} %);  '
              f'joint - marginal per pair: median {statistics.median(diff):+.4f} ms ({min(diff):+.4f} .. {max(diff):+.4f})')


if __name__ == '__main__':
    main()
