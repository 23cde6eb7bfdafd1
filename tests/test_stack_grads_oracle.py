"""CPU: the oracle's restatements of the geodesic transformer blocks (DecoderLayer, EncoderLayer, ODEGDecoder, ODEGEncoder over
HypAttention) reproduce the reference's own gradients recorded in tests/golden/stack_grads.npz (make_stack_grads_golden.py) under fp32
autograd.  This pins the yardstick the GPU autograd tests (test_stack_autograd.py) compare the HIP backward with."""
import os

import numpy as np
import pytest
import torch

from helpers import yardstick_close

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope='module')
def g():
    return np.load(os.path.join(HERE, 'golden', 'stack_grads.npz'))


def decoder_state():
    from sttode_amd.weights import make_decoder_layer_weights, to_torch_state_dict
    return to_torch_state_dict(make_decoder_layer_weights(61, d=64, ff=256))


def encoder_state():
    sd = {k: v for k, v in decoder_state().items() if not k.startswith('cross_attn') and not k.startswith('norm3')}
    return {k: (v * 0.3 if k.endswith('weight') and 'norm' not in k else v) for k, v in sd.items()}


def build(tag):
    """The oracle module of a fixture case and its forward on the case's inputs."""
    from oracle.sttode_ref import DecoderLayer, EncoderLayer, ODEGDecoder, ODEGEncoder
    if tag in ('dec', 'deceq', 'odeg'):
        layer = DecoderLayer(64, 8, 256)
        layer.load_state_dict(decoder_state(), strict=True)
        if tag == 'odeg':
            import copy
            m = ODEGDecoder([copy.deepcopy(layer) for _ in range(2)], 3.0)
            return m, lambda t, mem: m(t, mem)
        return layer, lambda t, mem: layer(t, mem)[0]
    layer = EncoderLayer(64, 8, 256)
    layer.load_state_dict(encoder_state(), strict=True)
    m = ODEGEncoder(layer, 1, 0.9)
    return m, lambda s: m(s)


def seeded(seed, shape):
    """make_stack_grads_golden.seeded: a case's inputs and loss weight G are drawn from the seeds the fixture records."""
    return np.random.default_rng(int(seed)).standard_normal(tuple(int(d) for d in shape)).astype(np.float32)


def digest(g):
    """make_stack_grads_golden.digest: [L2 norm, max |g|, 64 entries at evenly spaced flat positions] of a weight-matrix gradient."""
    f = np.asarray(g, np.float64).ravel()
    idx = np.linspace(0, f.size - 1, 64).astype(np.int64)
    return np.concatenate([[np.linalg.norm(f), np.abs(f).max()], f[idx]])


def case_inputs(g, tag):
    """(inputs, G) of a fixture case."""
    seed = int(g[f'{tag}_seed'])
    inputs = [seeded(seed + 1 + i, sh) for i, sh in enumerate(g[f'{tag}_shapes'])]
    return inputs, seeded(seed, g[f'{tag}_out'].shape)


def fixture_grads(g, tag):
    """name -> ('full', gradient) | ('digest', digest) as stored."""
    out = {}
    for k in g.files:
        if k.startswith(tag + '_grad::'):
            out[k[len(tag) + 7:]] = ('full', g[k])
        elif k.startswith(tag + '_gradd::'):
            out[k[len(tag) + 8:]] = ('digest', g[k])
    return out


def oracle_grads(g, tag, double):
    m, run = build(tag)
    inputs, G = case_inputs(g, tag)
    xs, G = [torch.from_numpy(x) for x in inputs], torch.from_numpy(G)
    if double:
        m, xs, G = m.double(), [x.double() for x in xs], G.double()
    xs = [x.requires_grad_(True) for x in xs]
    y = run(*xs)
    (y * G).sum().backward()
    grads = {name.replace('odeblock.odefunc.', ''): p.grad.detach().numpy() for name, p in m.named_parameters()}
    return y.detach().numpy(), grads, [x.grad.numpy() for x in xs]


@pytest.mark.parametrize('tag', ['dec', 'deceq', 'odeg', 'enc'])
def test_oracle_reproduces_reference_gradients(g, tag):
    y, grads, dxs = oracle_grads(g, tag, False)
    y64, g64, dx64 = oracle_grads(g, tag, True)
    yardstick_close(y, g[f'{tag}_out'], y64, rtol=1e-5, atol=1e-5, what=f'{tag} out')
    fix = fixture_grads(g, tag)
    assert sorted(fix) == sorted(grads), (tag, set(fix) ^ set(grads))
    for name, (kind, ref) in fix.items():
        got, r64 = (grads[name], g64[name]) if kind == 'full' else (digest(grads[name]), digest(g64[name]))
        for part in ((slice(None),) if kind == 'full' else (slice(0, 2), slice(2, None))):     # digest: [norm, max] and the entries
            scale = float(np.abs(ref[part]).max()) + 1e-30
            yardstick_close(got[part], ref[part], r64[part], rtol=1e-4, atol=1e-5 * scale, what=f'{tag} grad {name} ({kind})')
    for i, (d, d64) in enumerate(zip(dxs, dx64)):
        ref = g[f'{tag}_dinput::{i}']
        yardstick_close(d, ref, d64, rtol=1e-4, atol=1e-5 * float(np.abs(ref).max()), what=f'{tag} d input {i}')
