"""Host cost of the eager training step (train_graphs = False: graph replay would hide the Python side): ms per step of forward + backward
+ sttode_amd.optim.Adam over 300 steps, host clock, ending in a synchronise -- an ETH scene of 32 agents, an NBA batch of 32 x 11, and the
same NBA batch under ('rk4', 2).  One line per configuration.
usage: python profiles/train_layer/rates.py <tree root> <label>   (alternate the two trees, one process each, on one built library)"""
import gc, os, sys, time
root, label = os.path.abspath(sys.argv[1]), sys.argv[2]
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, 'tests'))
import torch
from helpers import make_args
import sttode_amd
assert os.path.dirname(os.path.abspath(sttode_amd.__file__)) == os.path.join(root, 'sttode_amd'), sttode_amd.__file__
from sttode_amd import STTODENet, scenes
from sttode_amd.optim import Adam
from sttode_amd.weights import make_weights, to_torch_state_dict
dev = torch.device('cuda')
STEPS = 300

for name, ds, Tp, Tf, ode in (('eth32', 'eth', 8, 12, ('euler', 1)), ('nba32x11', 'nba', 5, 10, ('euler', 1)), ('nba32x11_rk4x2', 'nba', 5, 10, ('rk4', 2))):
    torch.manual_seed(7)
    m = STTODENet(make_args(ds, Tp, Tf), dev)
    m.load_state_dict(to_torch_state_dict(make_weights(1234, past_length=Tp, future_length=Tf)), strict=True)
    m.train()
    m.train_graphs = False
    m.ode_method, m.ode_steps = ode
    opt = Adam(m.parameters(), lr=1e-4)
    if ds == 'eth':
        ob, pr = (torch.from_numpy(t).to(dev) for t in scenes.eth_scene(1, n_min=32, n_max=32))
        feed = lambda: m.set_data(None, ob, pr, None, None)
    else:
        d = scenes.nba_batch(1, 32)
        data = {k: (torch.from_numpy(v) if hasattr(v, 'shape') else v) for k, v in d.items()}
        feed = lambda: m.set_data_nba(data)

    def step():
        feed()
        tot = m.forward()[0]
        opt.zero_grad()
        tot.backward()
        opt.step()
    for _ in range(30):
        step()
    gc.collect()
    gc.freeze()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(STEPS):
        step()
    torch.cuda.synchronize()
    print(f'{label} {name} {1e3 * (time.perf_counter() - t0) / STEPS:.4f} ms/step', flush=True)
    gc.unfreeze()
    del m, opt
