"""Ordered entry-point tags of one eager step for four cases.  usage: python profiles/train_forms/tags.py <tree root> <out file>  (run once per tree, both on one built library through STTODE_HIP_LIB; compare the files)"""
import os, sys
root, out = os.path.abspath(sys.argv[1]), sys.argv[2]
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, 'tests'))
import numpy as np, torch
from helpers import make_args, sampler_args, dims_case_inputs, dims_case_weights
import sttode_amd
assert os.path.dirname(os.path.abspath(sttode_amd.__file__)) == os.path.join(root, 'sttode_amd'), sttode_amd.__file__
from sttode_amd import STTODENet, scenes, capi, Sampler, samplerloss
from sttode_amd.weights import make_weights, make_sampler_weights, to_torch_state_dict
dev = torch.device('cuda')
lines = []


def collect(name, fn):
    torch.cuda.synchronize()
    capi.TIMING = []
    fn()
    torch.cuda.synchronize()
    tags = [t for t, _, _ in capi.TIMING]
    capi.TIMING = None
    lines.append(f'## {name}: {len(tags)} entry-point calls')
    lines.extend(tags)


def model(ds, Tp, Tf):
    m = STTODENet(make_args(ds, Tp, Tf), dev)
    m.load_state_dict(to_torch_state_dict(make_weights(1234, past_length=Tp, future_length=Tf)))
    m.train()
    m.train_graphs = False
    return m


def step(m, feed):
    feed()
    tot = m.forward()[0]
    m.zero_grad()
    tot.backward()


# ETH 32
m = model('eth', 8, 12)
ob, pr = scenes.eth_scene(1, n_min=32, n_max=32)
feed = lambda: m.set_data(None, torch.from_numpy(ob), torch.from_numpy(pr), torch.ones(32, 8), torch.ones(32, 12))
step(m, feed)
collect('eth N=32', lambda: step(m, feed))
# NBA 32 x 11
m = model('nba', 5, 10)
d = scenes.nba_batch(1, 32)
data = {k: (torch.from_numpy(v) if hasattr(v, 'shape') else v) for k, v in d.items()}
feed = lambda: m.set_data_nba(data)
step(m, feed)
collect('nba B=32 N=11', lambda: step(m, feed))
# generic widths
for tag in ('hd32', 'nd3'):
    for ds in ('eth', 'nba'):
        a, inputs, z, (eq, ep, e20) = dims_case_inputs(tag, ds)
        m = STTODENet(a, dev)
        m.load_state_dict(to_torch_state_dict(dims_case_weights(a)), strict=True)
        m.train()
        m.train_graphs = False
        if ds == 'eth':
            feed = lambda: m.set_data(None, torch.from_numpy(inputs[0]), torch.from_numpy(inputs[1]))
        else:
            dd = {k: (torch.from_numpy(v) if isinstance(v, np.ndarray) else v) for k, v in inputs.items()}
            feed = lambda: m.set_data_nba(dd)
        step(m, feed)
        collect(f'generic {tag} {ds}', lambda: step(m, feed))
        # generic staged API: inference + decode
        m.eval()

        def ev():
            feed()
            m.inference(dd if ds == 'nba' else None, z=torch.from_numpy(z))
        ev()
        collect(f'generic {tag} {ds} inference', ev)
# stage-2 sampler training step
net = STTODENet(make_args('eth', 8, 12), dev).eval()
net.load_state_dict(to_torch_state_dict(make_weights(1234)))
smp = Sampler(sampler_args('eth', 8, 12))
smp.load_state_dict(to_torch_state_dict(make_sampler_weights()), strict=True)
smp.set_device(dev)
smp.train()
ob, pr = scenes.eth_scene(3, n_min=9, n_max=9)
n = 9
fut = torch.from_numpy(np.ascontiguousarray(pr.transpose(0, 2, 1))).to(dev)
cfg = {'weight': 1, 'scale': 1.0}
for mean in (True, False):
    def sstep():
        net.set_data(None, torch.from_numpy(ob), torch.from_numpy(pr), torch.ones(n, 8), torch.ones(n, 12))
        smp.zero_grad()
        dec, sd, vd, _ = smp.forward(net, mean=mean)
        tot, ld, _ = samplerloss.compute_sampler_loss(smp.args, fut, dec.reshape(-1, 20, 12, 2), 1, None, vd, sd, cfg)
        tot.backward()
    sstep()
    collect(f'sampler stage-2 step mean={mean}', sstep)
open(out, 'w').write('\n'.join(lines) + '\n')
print('tags written:', out, len(lines), 'lines')
