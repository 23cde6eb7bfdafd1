"""Training-step rate under the encoder integrators (net.ode_method / net.ode_steps): ms per step (set_data + forward + backward + Adam,
hipGraph replay on) for one configuration per run.
  --case scene: one ETH scene of 32 agents (attention length 1);  --case nba: 32 scenes x 11 agents (attention over the batch)
Prints one JSON line; profiles/ode_train/rate.txt collects them.  Usage: python profiles/exp_ode_train_rate.py --case scene --method rk4 --steps 1"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from helpers import make_args                                   # noqa: E402
from sttode_amd import STTODENet, scenes                        # noqa: E402
from sttode_amd.weights import make_weights, to_torch_state_dict  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--case', choices=('scene', 'nba'), default='scene')
ap.add_argument('--method', default='euler')
ap.add_argument('--steps', type=int, default=1)
ap.add_argument('--reps', type=int, default=50)
ap.add_argument('--warmup', type=int, default=5)
a = ap.parse_args()

dev = torch.device('cuda')
ds, Tp, Tf = ('eth', 8, 12) if a.case == 'scene' else ('nba', 5, 10)
m = STTODENet(make_args(ds, Tp, Tf), dev)
m.load_state_dict(to_torch_state_dict(make_weights(1234, past_length=Tp, future_length=Tf)))
m.train()
m.ode_method, m.ode_steps = a.method, a.steps
if a.case == 'scene':
    ob, pr = scenes.eth_scene(1, n_min=32, n_max=32)
    feed = lambda: m.set_data(None, torch.from_numpy(ob), torch.from_numpy(pr), torch.ones(32, Tp), torch.ones(32, Tf))
else:
    d = scenes.nba_batch(1, 32)
    data = {k: (torch.from_numpy(v) if hasattr(v, 'shape') else v) for k, v in d.items()}
    feed = lambda: m.set_data_nba(data)
opt = torch.optim.Adam(m.parameters(), lr=1e-4)


def step():
    feed()
    tot = m.forward()[0]
    opt.zero_grad()
    tot.backward()
    opt.step()


for _ in range(a.warmup):
    step()
torch.cuda.synchronize()
t = time.perf_counter()
for _ in range(a.reps):
    step()
torch.cuda.synchronize()
dt = (time.perf_counter() - t) / a.reps
print(json.dumps({'case': a.case, 'agents': 32 if a.case == 'scene' else 352, 'method': a.method, 'steps': a.steps, 'graphs': True,
                  'ms_per_step': round(dt * 1e3, 4), 'reps': a.reps}))
