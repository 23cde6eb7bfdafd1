"""Digests of the training step on every trunk path of training.Engine: per case seeded inputs with explicit eps_q / eps_p / eps20 and dropout
masks, one eager step, the five loss values as hex floats and a SHA-256 of every .grad; for an ETH scene of 32 agents and an NBA batch of
32 x 11 then one more eager and five replayed steps with sttode_amd.optim.Adam and a digest of every parameter after the last.  The small cases are those of
tests/test_training_call_sequence_gpu.py.
usage: python profiles/train_layer/bitwise.py <tree root> <out file>   (once per tree on one built library, STTODE_HIP_LIB; diff the files)"""
import hashlib, os, sys
root, out = os.path.abspath(sys.argv[1]), sys.argv[2]
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, 'tests'))
import numpy as np, torch
from helpers import dims_case_inputs, dims_case_weights, make_args, sampler_args
import sttode_amd
assert os.path.dirname(os.path.abspath(sttode_amd.__file__)) == os.path.join(root, 'sttode_amd'), sttode_amd.__file__
from sttode_amd import STTODENet, Sampler, scenes, training
from sttode_amd.optim import Adam
from sttode_amd.weights import make_sampler_weights, make_weights, to_torch_state_dict
dev = torch.device('cuda')
lines = []


def dig(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()[:24]


def model(a, w, train=True):
    m = STTODENet(a, dev)
    m.load_state_dict(to_torch_state_dict(w), strict=True)
    return m.train(train)


def feeder(m, ds, Tp, Tf, n_eth, B, N):
    if ds == 'eth':
        ob, pr = scenes.eth_scene(1, obs_len=Tp, pred_len=Tf, n_min=n_eth, n_max=n_eth)
        return lambda: m.set_data(None, torch.from_numpy(ob), torch.from_numpy(pr), torch.ones(n_eth, Tp), torch.ones(n_eth, Tf), theta=0.3)
    d = scenes.nba_batch(1, B, N=N, obs_len=Tp, pred_len=Tf)
    data = {k: (torch.from_numpy(v) if hasattr(v, 'shape') else v) for k, v in d.items()}
    return lambda: m.set_data_nba(data)


def noise(gen, n, Tp, Tf, zd=32, hd=64):
    eps = [torch.randn(r, zd, generator=gen) for r in (n, n, n * 20)]
    return eps + [(torch.rand(n * T, hd, generator=gen) < 0.9).float() / 0.9 for T in (Tp, Tf)]


def record(name, m, vals, grads=True):
    lines.append(f'{name} losses ' + ' '.join(float(v).hex() for v in [float(vals[0].detach())] + list(vals[1:])))
    if grads:
        for k, p in m.named_parameters():
            lines.append(f'{name} grad0 {k} ' + ('None' if p.grad is None else dig(p.grad)))


def reference_case(name, ds, Tp, Tf, ode=('euler', 1), fused=True, chunk=None, n_eth=3, B=3, N=4, replay=0):
    torch.manual_seed(7); np.random.seed(7)
    m = model(make_args(ds, Tp, Tf), make_weights(1234, past_length=Tp, future_length=Tf))
    m.ode_method, m.ode_steps = ode
    opt = Adam(m.parameters(), lr=1e-4)
    feed = feeder(m, ds, Tp, Tf, n_eth, B, N)
    gen = torch.Generator().manual_seed(99)
    was = training._ode_chunk_stages
    if chunk is not None:
        training._ode_chunk_stages = lambda nst, per_stage: chunk
    try:
        # step 0, whose .grad digests are recorded: eager, graphs off.  Then, graphs on: the shape's first step (eager again), and `replay` replayed
        for s in range(1 + (replay + 1 if replay else 0)):
            m.train_graphs = s > 0
            feed()
            n = m._past.shape[0]
            eq, ep, e20, dp, df = noise(gen, n, Tp, Tf)
            if s == 0 and not fused:                                    # the engine exists after a first forward: one with the same inputs
                m.forward(eps_q=eq, eps_p=ep, eps20=e20, drop_past=dp, drop_future=df)
                m._engine.fused_trunk = False
                feed()
            vals = m.forward(eps_q=eq, eps_p=ep, eps20=e20, drop_past=dp, drop_future=df)
            opt.zero_grad()
            vals[0].backward()
            torch.cuda.synchronize()
            record(f'{name} step {s} replayed={len(getattr(m, "_graphs", {})) > 0}', m, vals, grads=s == 0)
            opt.step()
    finally:
        training._ode_chunk_stages = was
    if replay:
        assert len(m._graphs) > 0 and sum('replayed=True' in l for l in lines if l.startswith(name + ' step')) == replay
        torch.cuda.synchronize()
        for k, p in m.named_parameters():
            lines.append(f'{name} param_after_step_{replay + 1} {k} ' + dig(p))


def generic_case(tag):
    a, inputs, _, eps = dims_case_inputs(tag, 'eth')
    torch.manual_seed(7); np.random.seed(7)
    m = model(a, dims_case_weights(a), train=False)                     # (eval: no augmentation of the case's own scene)
    m.train_graphs = False
    m.set_data(None, torch.from_numpy(inputs[0]), torch.from_numpy(inputs[1]))
    n = m._past.shape[0]
    gen = torch.Generator().manual_seed(99)
    dp, df = noise(gen, n, a.past_length, a.future_length, a.zdim, a.hidden_dim)[3:]
    vals = m.forward(*[torch.from_numpy(e) for e in eps], drop_past=dp, drop_future=df)
    vals[0].backward()
    torch.cuda.synchronize()
    record(f'generic_{tag} step 0', m, vals)


def sampler_case():
    torch.manual_seed(7); np.random.seed(7)
    m = model(make_args('eth', 8, 12), make_weights(1234), train=False)
    smp = Sampler(sampler_args('eth', 8, 12))
    smp.load_state_dict(to_torch_state_dict(make_sampler_weights()), strict=True)
    smp.set_device(dev)
    smp.train()
    ob, pr = scenes.eth_scene(1, n_min=3, n_max=3)
    m.set_data(None, torch.from_numpy(ob), torch.from_numpy(pr))
    dec, q, _, _ = smp.forward(m, mean=True)
    (dec.square().sum() + q.mu.square().sum() + q.logvar.sum()).backward()
    torch.cuda.synchronize()
    lines.append('sampler_mean values ' + ' '.join(dig(t) for t in (dec, q.mu, q.logvar)))
    for k, p in smp.named_parameters():
        lines.append(f'sampler_mean grad0 {k} ' + ('None' if p.grad is None else dig(p.grad)))


eth, nba = ('eth', 8, 12), ('nba', 5, 10)
reference_case('eth3_fused', *eth)
reference_case('eth3_layers', *eth, fused=False)
reference_case('nba3x4_fused', *nba)
reference_case('nba3x4_layers', *nba, fused=False)
reference_case('eth3_rk4x1_fused', *eth, ode=('rk4', 1))
reference_case('eth3_rk4x1_layers', *eth, ode=('rk4', 1), fused=False)
reference_case('nba3x4_rk4x2', *nba, ode=('rk4', 2))
reference_case('nba3x4_rk4x2_chunk3', *nba, ode=('rk4', 2), chunk=3)
generic_case('hd32')
generic_case('nd1')
sampler_case()
reference_case('eth32', *eth, n_eth=32, replay=5)
reference_case('nba32x11', *nba, B=32, N=11, replay=5)
open(out, 'w').write('\n'.join(lines) + '\n')
print('digest written:', out, len(lines), 'lines')
