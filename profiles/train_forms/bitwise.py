"""One eager step + five replayed steps with sttode_amd.optim.Adam, seeded and with explicit noise and dropout masks; writes a digest of every
loss value, every .grad after the first step and every parameter after the last.  usage: python profiles/train_forms/bitwise.py <tree root> <out file>  (run once per tree on one built library, STTODE_HIP_LIB; diff the files)"""
import hashlib, os, sys
root, out = os.path.abspath(sys.argv[1]), sys.argv[2]
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, 'tests'))
import numpy as np, torch
from helpers import make_args
import sttode_amd
assert os.path.dirname(os.path.abspath(sttode_amd.__file__)) == os.path.join(root, 'sttode_amd'), sttode_amd.__file__
from sttode_amd import STTODENet, scenes
from sttode_amd.optim import Adam
from sttode_amd.weights import make_weights, to_torch_state_dict
dev = torch.device('cuda')
lines = []


def dig(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()[:24]


for name, ds, Tp, Tf, n in (('eth32', 'eth', 8, 12, 32), ('nba32x11', 'nba', 5, 10, 352)):
    torch.manual_seed(7); np.random.seed(7)
    m = STTODENet(make_args(ds, Tp, Tf), dev)
    m.load_state_dict(to_torch_state_dict(make_weights(1234, past_length=Tp, future_length=Tf)))
    m.train()
    opt = Adam(m.parameters(), lr=1e-4)
    if ds == 'eth':
        ob, pr = scenes.eth_scene(1, n_min=32, n_max=32)
        feed = lambda: m.set_data(None, torch.from_numpy(ob), torch.from_numpy(pr), torch.ones(n, Tp), torch.ones(n, Tf), theta=0.3)
    else:
        d = scenes.nba_batch(1, 32)
        data = {k: (torch.from_numpy(v) if hasattr(v, 'shape') else v) for k, v in d.items()}
        feed = lambda: m.set_data_nba(data)
    gen = torch.Generator().manual_seed(99)
    for s in range(6):
        eq, ep, e20 = torch.randn(n, 32, generator=gen), torch.randn(n, 32, generator=gen), torch.randn(n * 20, 32, generator=gen)
        dp = (torch.rand(n * Tp, 64, generator=gen) < 0.9).float() / 0.9
        df = (torch.rand(n * Tf, 64, generator=gen) < 0.9).float() / 0.9
        feed()
        assert m._past.shape[0] == n, m._past.shape
        vals = m.forward(eps_q=eq, eps_p=ep, eps20=e20, drop_past=dp, drop_future=df)
        opt.zero_grad()
        vals[0].backward()
        torch.cuda.synchronize()
        replayed = len(getattr(m, '_graphs', {})) > 0
        lines.append(f'{name} step {s} replayed={replayed} losses ' + ' '.join(float(v).hex() for v in [float(vals[0].detach())] + list(vals[1:])))
        if s == 0:
            for k, p in m.named_parameters():
                lines.append(f'{name} grad0 {k} ' + ('None' if p.grad is None else dig(p.grad)))
        opt.step()
    assert replayed
    torch.cuda.synchronize()
    for k, p in m.named_parameters():
        lines.append(f'{name} param5 {k} ' + dig(p))
open(out, 'w').write('\n'.join(lines) + '\n')
print('digest written:', out, len(lines), 'lines')
