"""GPU: autograd through the op-level geodesic transformer drop-ins (sttode_amd.hypertransformer, ops.mhgsa) on the HIP backward.

Gradients are compared per tensor with float64 autograd of the oracle restatements (oracle/sttode_ref.py) through helpers.yardstick_close:
the HIP result may sit from the float64 value as far as a correct fp32 evaluation (torch autograd of the oracle in fp32) does, times a
factor, plus a small floor relative to the tensor's largest entry.  Where the reference's own gradients exist (tests/golden/stack_grads.npz,
pinned to the oracle by test_stack_grads_oracle.py) they are the fp32 side of the comparison."""
import copy
import os

import numpy as np
import pytest
import torch

from helpers import yardstick_close
from test_stack_grads_oracle import case_inputs, digest, fixture_grads

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
LO, HI = -1 + 1e-4, 1 - 1e-4


def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def golden():
    return np.load(os.path.join(HERE, 'golden', 'stack_grads.npz'))


def decoder_state():
    from sttode_amd.weights import make_decoder_layer_weights, to_torch_state_dict
    return to_torch_state_dict(make_decoder_layer_weights(61, d=64, ff=256))


def encoder_state():
    sd = {k: v for k, v in decoder_state().items() if not k.startswith('cross_attn') and not k.startswith('norm3')}
    return {k: (v * 0.3 if k.endswith('weight') and 'norm' not in k else v) for k, v in sd.items()}


def attn_state(prefix='cross_attn.'):
    return {k[len(prefix):]: v for k, v in decoder_state().items() if k.startswith(prefix)}


def close(got, g32, g64, what, floor=3e-4):
    """HIP vs float64 within what fp32 autograd (or the reference's fp32 fixture) reaches, x4, plus floor * max |g64|."""
    got, g32, g64 = (np.asarray(t.detach().double().cpu() if isinstance(t, torch.Tensor) else t, np.float64) for t in (got, g32, g64))
    scale = float(np.abs(g64).max()) + 1e-30
    yardstick_close(got, g32, g64, rtol=1e-4, atol=floor * scale, what=what, factor=4.0)


def hip_run(module, inputs, run, G, trainable=True):
    """loss = sum(run(*inputs) * G) on the HIP drop-in -> (out, {param: grad}, [input grads])."""
    from sttode_amd import hypertransformer as ht
    if trainable:
        ht.trainable(module)
    module.zero_grad()
    xs = [torch.from_numpy(x).to(dev()).requires_grad_(True) for x in inputs]
    y = run(*xs)
    (y * torch.from_numpy(G).to(dev())).sum().backward()
    torch.cuda.synchronize()
    return y.detach().cpu().numpy(), {k: p.grad.detach().cpu() for k, p in module.named_parameters()}, [x.grad.cpu() for x in xs]


def oracle_run(module, inputs, run, G, double):
    m = copy.deepcopy(module)
    xs = [torch.from_numpy(x) for x in inputs]
    Gt = torch.from_numpy(G)
    if double:
        m, xs, Gt = m.double(), [x.double() for x in xs], Gt.double()
    xs = [x.requires_grad_(True) for x in xs]
    m.zero_grad()
    y = run(m, *xs)
    (y * Gt).sum().backward()
    return y.detach().numpy(), {k: p.grad.detach() for k, p in m.named_parameters()}, [x.grad for x in xs]


def compare(hip, o32, o64, what, name_map=lambda k: k, golden=None, tag=None, floor=3e-4):
    """Every parameter and input gradient (and the output) of `hip` against the oracle; against the fixture where `golden` is given."""
    y, gp, gx = hip
    y32, g32, x32 = o32
    y64, g64, x64 = o64
    close(y, y32, y64, what + ' out', floor=1e-4)
    assert sorted(name_map(k) for k in gp) == sorted(g64), what
    for k, v in gp.items():
        close(v, g32[name_map(k)], g64[name_map(k)], f'{what} grad {k}', floor)
        if golden is not None:                                  # the fixture keeps vectors whole, weight matrices as digests
            kind, ref = fixture_grads(golden, tag)[k]
            if kind == 'full':
                close(v, ref, g64[name_map(k)], f'{what} grad {k} vs reference fixture', floor)
            else:
                dv, d64 = digest(v.double().numpy()), digest(g64[name_map(k)].double().numpy())
                for part in (slice(0, 2), slice(2, None)):
                    close(dv[part], ref[part], d64[part], f'{what} grad {k} vs reference fixture (digest)', floor)
    for i, (a, b, c) in enumerate(zip(gx, x32, x64)):
        close(a, b, c, f'{what} d input {i}', floor)
        if golden is not None:
            close(a, golden[f'{tag}_dinput::{i}'], c, f'{what} d input {i} vs reference fixture', floor)


# ---------------------------------------------------------------------------------------------------------------------------------
# the kernel: sttode_mhgsa_attn_rc_bwd against float64 autograd of the attention core
# ---------------------------------------------------------------------------------------------------------------------------------
def core(R, C, V, rs, cs):
    """out[r] = sum_c softmax_c(-acos(clamp(rho^ . gam^))) V[c] per (slot, head); operands [len, Nb, 64]."""
    rows, Nb, _ = R.shape
    cols = C.shape[0]
    r = (R * rs).view(rows, Nb, 8, 8)
    c = (C * cs).view(cols, Nb, 8, 8)
    r = r / r.norm(dim=-1, keepdim=True)
    c = c / c.norm(dim=-1, keepdim=True)
    x = torch.einsum('rbhd,cbhd->bhrc', r, c)
    P = torch.softmax(-torch.acos(x.clamp(LO, HI)), dim=-1)
    return torch.einsum('bhrc,cbhd->rbhd', P, V.view(cols, Nb, 8, 8)).reshape(rows, Nb, 64), x


def core_grads(R, C, V, dO, rs, cs, double):
    ts = [torch.from_numpy(t) for t in (R, C, V)]
    d = torch.from_numpy(dO)
    if double:
        ts, d = [t.double() for t in ts], d.double()
    ts = [t.requires_grad_(True) for t in ts]
    out, x = core(*ts, rs, cs)
    out.backward(d)
    return [t.grad.numpy() for t in ts], x.detach()


def hip_core_bwd(R, C, V, dO, rs, cs, packed=False):
    """The new entry point; `packed`: R, C, V are column blocks of one [len * Nb, 192] tensor (self-attention layout, rows == cols)."""
    from sttode_amd import capi
    rows, Nb, E = R.shape
    cols = C.shape[0]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev())
    if packed:
        qkv = t(np.concatenate([C, R, V], axis=-1).reshape(rows * Nb, 192))
        d = torch.full_like(qkv, float('nan'))
        Rd, Cd, Vd, dR, dC, dV = qkv[:, 64:128], qkv[:, :64], qkv[:, 128:], d[:, 64:128], d[:, :64], d[:, 128:]
        ss = (Nb * 192, 192)
    else:
        Rd, Cd, Vd = t(R), t(C), t(V)
        dR, dC, dV = (torch.full_like(a, float('nan')) for a in (Rd, Cd, Vd))
        ss = (Nb * E, E)
    dOd = t(dO)
    capi.call('sttode_mhgsa_attn_rc_bwd', Rd, Cd, Vd, dOd, dR, dC, dV, rows, cols, Nb, *ss, *ss, *ss, Nb * E, E, rs, cs, capi.stream_ptr())
    torch.cuda.synchronize()
    return [a.cpu().numpy().reshape(-1, Nb, E) for a in (dR, dC, dV)]


@pytest.mark.parametrize('rows,cols,Nb', [(6, 9, 10), (9, 6, 10), (1, 5, 3), (12, 8, 640), (7, 7, 4), (16, 16, 2), (128, 128, 2)])
def test_attention_core_backward_vs_float64(rows, cols, Nb):
    rng = np.random.default_rng(rows * 1000 + cols)
    R, C = rng.standard_normal((rows, Nb, 64)).astype(np.float32), rng.standard_normal((cols, Nb, 64)).astype(np.float32)
    V, dO = rng.standard_normal((cols, Nb, 64)).astype(np.float32), rng.standard_normal((rows, Nb, 64)).astype(np.float32)
    rs, cs = (1.0, 8 ** -0.5) if rows == cols else (8 ** -0.5, 1.0)          # the two orientations of ops.mhgsa
    got = hip_core_bwd(R, C, V, dO, rs, cs, packed=rows == cols == 16 or rows == cols == 128)
    g32, _ = core_grads(R, C, V, dO, rs, cs, False)
    g64, _ = core_grads(R, C, V, dO, rs, cs, True)
    for nm, a, b, c in zip(('dR', 'dC', 'dV'), got, g32, g64):
        assert np.isfinite(a).all(), nm
        close(a, b, c, f'attention core {rows}x{cols} Nb={Nb} {nm}')


def test_attention_core_tied_operands_zero_gradient_on_the_clamp():
    """R == C (W_q = W_k, b_q = b_k, query = key): every diagonal inner product is 1, outside the clamp, and contributes nothing."""
    rng = np.random.default_rng(9)
    R = rng.standard_normal((7, 4, 64)).astype(np.float32)
    V, dO = rng.standard_normal((7, 4, 64)).astype(np.float32), rng.standard_normal((7, 4, 64)).astype(np.float32)
    cs = 8 ** -0.5
    g64, x = core_grads(R, R, V, dO, 1.0, cs, True)
    assert (torch.diagonal(x, dim1=-2, dim2=-1) > HI).all()
    got = hip_core_bwd(R, R.copy(), V, dO, 1.0, cs)
    g32, _ = core_grads(R, R, V, dO, 1.0, cs, False)
    for nm, a, b, c in zip(('dR', 'dC', 'dV'), got, g32, g64):
        close(a, b, c, f'tied attention core {nm}')


def test_attention_core_refuses_shapes_over_the_lds_budget():
    from sttode_amd import capi
    rows = cols = 500
    a = torch.zeros(rows, 1, 64, device=dev())
    d = torch.full_like(a, 7.0)
    with pytest.raises(capi.SttodeError, match='sttode_mhgsa_attn_rc_bwd.*64 KiB'):
        capi.call('sttode_mhgsa_attn_rc_bwd', a, a, a, a, d, d, d, rows, cols, 1, 64, 64, 64, 64, 64, 64, 64, 64, 1.0, 1.0, capi.stream_ptr())
    torch.cuda.synchronize()
    assert (d == 7.0).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# modules
# ---------------------------------------------------------------------------------------------------------------------------------
def test_mhgsa_differentiable_vs_float64():
    from oracle.sttode_ref import mhgsa as mhgsa_ref
    from sttode_amd.ops import mhgsa
    sd = attn_state()
    rng = np.random.default_rng(3)
    for L, S in ((5, 8), (6, 6)):
        q, k, v = (rng.standard_normal((n, 12, 64)).astype(np.float32) for n in (L, S, S))
        G = rng.standard_normal((L, 12, 64)).astype(np.float32)
        names = ('temporal_attention_before.in_proj_weight', 'temporal_attention_before.in_proj_bias', 'temporal_attention_before.out_proj.weight',
                 'temporal_attention_before.out_proj.bias')
        P = [sd[n].to(dev()).requires_grad_(True) for n in names]
        xs = [torch.from_numpy(a).to(dev()).requires_grad_(True) for a in (q, k, v)]
        out, w = mhgsa(*xs, *P, need_weights=True, differentiable=True)
        assert out.requires_grad and not w.requires_grad
        (out * torch.from_numpy(G).to(dev())).sum().backward()
        got = [t.grad.cpu() for t in xs + P]

        def ref(double):
            ts = [torch.from_numpy(a) for a in (q, k, v)] + [sd[n].clone() for n in names]
            ts = [(t.double() if double else t).requires_grad_(True) for t in ts]
            o, _ = mhgsa_ref(*ts[:3], 8, *ts[3:])
            (o * (torch.from_numpy(G).double() if double else torch.from_numpy(G))).sum().backward()
            return [t.grad for t in ts]
        for i, (a, b, c) in enumerate(zip(got, ref(False), ref(True))):
            close(a, b, c, f'mhgsa L={L} S={S} grad {i}')


@pytest.mark.parametrize('form', ['self', 'cross', 'cross_equal'])
def test_hypattention_grads_vs_float64(form):
    from oracle.sttode_ref import HypAttention as Ref
    from sttode_amd.hypertransformer import Hypattention
    rng = np.random.default_rng(11)
    m = Hypattention(64, 8)
    m.load_state_dict(attn_state(), strict=True)
    o = Ref(64, 8)
    o.load_state_dict(attn_state(), strict=True)
    x = rng.standard_normal((6, 5, 2, 64)).astype(np.float32)
    G = rng.standard_normal((6, 5, 2, 64)).astype(np.float32)
    if form == 'self':
        inputs, run_h, run_o = [x], lambda a: m(a, a, a)[0], lambda mm, a: mm(a, a, a)[0]
    else:
        mem = rng.standard_normal((9 if form == 'cross' else 6, 5, 2, 64)).astype(np.float32)
        inputs, run_h, run_o = [x, mem], lambda a, b: m(a, b, b)[0], lambda mm, a, b: mm(a, b, b)[0]
    compare(hip_run(m.to(dev()), inputs, run_h, G), oracle_run(o, inputs, run_o, G, False), oracle_run(o, inputs, run_o, G, True),
            f'Hypattention {form}')


def test_encoder_layer_grads_vs_float64():
    from oracle.sttode_ref import EncoderLayer
    from sttode_amd.hypertransformer import TransformerEncoderLayer
    rng = np.random.default_rng(12)
    m = TransformerEncoderLayer(64, 8, 256)
    m.load_state_dict(encoder_state(), strict=True)
    o = EncoderLayer(64, 8, 256)
    o.load_state_dict(encoder_state(), strict=True)
    x, G = rng.standard_normal((8, 6, 3, 64)).astype(np.float32), rng.standard_normal((8, 6, 3, 64)).astype(np.float32)
    compare(hip_run(m.to(dev()), [x], lambda a: m(a), G), oracle_run(o, [x], lambda mm, a: mm(a), G, False),
            oracle_run(o, [x], lambda mm, a: mm(a), G, True), 'TransformerEncoderLayer')


def _decoder_pair():
    from oracle.sttode_ref import DecoderLayer
    from sttode_amd.hypertransformer import TransformerDecoderLayer
    m = TransformerDecoderLayer(64, 8, 256)
    m.load_state_dict(decoder_state(), strict=True)
    o = DecoderLayer(64, 8, 256)
    o.load_state_dict(decoder_state(), strict=True)
    return m.to(dev()), o


@pytest.mark.parametrize('tag', ['dec', 'deceq'])
def test_decoder_layer_grads_vs_reference_fixture(golden, tag):
    m, o = _decoder_pair()
    inputs, G = case_inputs(golden, tag)
    run_h, run_o = (lambda a, b: m(a, b, seq_mask=True)[0]), (lambda mm, a, b: mm(a, b)[0])
    hip = hip_run(m, inputs, run_h, G)
    close(hip[0], golden[f'{tag}_out'], oracle_run(o, inputs, run_o, G, True)[0], f'{tag} out vs reference fixture', floor=1e-4)
    compare(hip, oracle_run(o, inputs, run_o, G, False), oracle_run(o, inputs, run_o, G, True), f'TransformerDecoderLayer {tag}',
            golden=golden, tag=tag)


def test_decoder_layer_grads_large_vs_float64():
    m, o = _decoder_pair()
    rng = np.random.default_rng(13)
    tgt, mem = rng.standard_normal((12, 32, 20, 64)).astype(np.float32), rng.standard_normal((8, 32, 20, 64)).astype(np.float32)
    G = rng.standard_normal(tgt.shape).astype(np.float32)
    run_h, run_o = (lambda a, b: m(a, b)[0]), (lambda mm, a, b: mm(a, b)[0])
    compare(hip_run(m, [tgt, mem], run_h, G), oracle_run(o, [tgt, mem], run_o, G, False), oracle_run(o, [tgt, mem], run_o, G, True),
            'TransformerDecoderLayer 12/8 x 32 x 20')


def test_odeg_two_layers_vs_reference_fixture(golden):
    from oracle.sttode_ref import ODEGDecoder
    from sttode_amd.hypertransformer import ODEG
    m, o = _decoder_pair()
    ode = ODEG(m, 2, 3).to(dev())
    ref = ODEGDecoder([copy.deepcopy(o) for _ in range(2)], 3.0)
    inputs, G = case_inputs(golden, 'odeg')
    run_h, run_o = (lambda a, b: ode(a, b, seq_mask=True)[0]), (lambda mm, a, b: mm(a, b))
    compare(hip_run(ode, inputs, run_h, G), oracle_run(ref, inputs, run_o, G, False), oracle_run(ref, inputs, run_o, G, True), 'ODEG x2',
            golden=golden, tag='odeg')


@pytest.mark.parametrize('method,steps', [('euler', 1), ('euler', 3), ('rk4', 1), ('rk4', 2), ('rk4_classic', 2)])
def test_odeg_encoder_integrators_vs_float64(golden, method, steps):
    from oracle.sttode_ref import EncoderLayer, ode_integrate_ref
    from sttode_amd.hypertransformer import ODEG_Encoder, TransformerEncoderLayer
    layer = TransformerEncoderLayer(64, 8, 256)
    layer.load_state_dict(encoder_state(), strict=True)
    o = EncoderLayer(64, 8, 256)
    o.load_state_dict(encoder_state(), strict=True)
    enc = ODEG_Encoder(layer, 1, 0.9, method=method, steps=steps).to(dev())
    inputs, G = case_inputs(golden, 'enc')
    run_o = lambda mm, a: torch.relu(ode_integrate_ref(mm, a, 0.9, method, steps))
    pin = method == 'euler' and steps == 1                      # the reference's one Euler step: its own gradients are in the fixture
    compare(hip_run(enc, inputs, lambda a: enc(a), G), oracle_run(o, inputs, run_o, G, False), oracle_run(o, inputs, run_o, G, True),
            f'ODEG_Encoder {method} x{steps}', name_map=lambda k: k[len('layers.0.'):], golden=golden if pin else None, tag='enc')


# ---------------------------------------------------------------------------------------------------------------------------------
# default path, semantics, refusals
# ---------------------------------------------------------------------------------------------------------------------------------
def test_default_is_unchanged_and_bitwise_equal_to_the_graph_path():
    from sttode_amd import hypertransformer as ht
    m, _ = _decoder_pair()
    rng = np.random.default_rng(21)
    tgt = torch.from_numpy(rng.standard_normal((6, 5, 2, 64)).astype(np.float32)).to(dev()).requires_grad_(True)
    mem = torch.from_numpy(rng.standard_normal((9, 5, 2, 64)).astype(np.float32)).to(dev()).requires_grad_(True)
    y0 = m(tgt, mem)[0]
    assert not y0.requires_grad
    enc_l = ht.TransformerEncoderLayer(64, 8, 256)
    enc_l.load_state_dict(encoder_state(), strict=True)
    x = tgt.detach()[:, :, :1].clone().requires_grad_(True)
    encs = [ht.ODEG_Encoder(enc_l, 1, 0.9, method=me, steps=s).to(dev()) for me, s in (('euler', 1), ('rk4', 2), ('rk4_classic', 1))]
    e0 = [e(x) for e in encs]
    odeg = ht.ODEG(m, 2, 3)
    z0 = odeg(tgt, mem)[0]
    assert not any(t.requires_grad for t in e0 + [z0])
    for mod in [m, odeg] + encs:
        assert ht.trainable(mod) is mod
    assert all(l._trainable for l in odeg.layers) and copy.deepcopy(odeg).layers[0].cross_attn._trainable
    y1 = m(tgt, mem)[0]
    e1 = [e(x) for e in encs]
    z1 = odeg(tgt, mem)[0]
    assert all(t.requires_grad for t in [y1, z1] + e1)
    assert torch.equal(y0, y1.detach()) and torch.equal(z0, z1.detach())
    assert all(torch.equal(a, b.detach()) for a, b in zip(e0, e1))
    with torch.no_grad():
        assert not m(tgt, mem)[0].requires_grad
    ht.trainable(m, False)
    assert not m(tgt, mem)[0].requires_grad


def test_autograd_semantics():
    from sttode_amd import hypertransformer as ht
    m, _ = _decoder_pair()
    ht.trainable(m)
    rng = np.random.default_rng(22)
    tgt = torch.from_numpy(rng.standard_normal((6, 5, 2, 64)).astype(np.float32)).to(dev()).requires_grad_(True)
    mem = torch.from_numpy(rng.standard_normal((9, 5, 2, 64)).astype(np.float32)).to(dev())
    G = torch.from_numpy(rng.standard_normal((6, 5, 2, 64)).astype(np.float32)).to(dev())
    y, ws, wc = m(tgt, mem)
    assert y.requires_grad and not ws.requires_grad and not wc.requires_grad
    loss = (y * G).sum()
    loss.backward(retain_graph=True)
    g1 = {k: p.grad.clone() for k, p in m.named_parameters()}
    gt1 = tgt.grad.clone()
    loss.backward()                                                         # retain_graph: the same graph again; .grad accumulates
    for k, p in m.named_parameters():
        assert torch.equal(p.grad, 2 * g1[k]), k
    assert torch.equal(tgt.grad, 2 * gt1) and mem.grad is None
    with pytest.raises(RuntimeError):
        loss.backward()                                                     # the graph was freed
    # torch.autograd.grad, frozen parameters
    m.zero_grad()
    m.linear1.weight.requires_grad_(False)
    y = m(tgt, mem)[0]
    gw, gx = torch.autograd.grad((y * G).sum(), [m.norm3.weight, tgt])
    assert m.norm3.weight.grad is None
    (m(tgt, mem)[0] * G).sum().backward()
    assert m.linear1.weight.grad is None and torch.equal(m.norm3.weight.grad, gw)
    np.testing.assert_array_equal(gx.cpu().numpy(), gt1.cpu().numpy())
    m.linear1.weight.requires_grad_(True)
    # double backward is refused
    y = m(tgt, mem)[0]
    (g,) = torch.autograd.grad((y * y).sum(), [tgt], create_graph=True)    # dL/dy = 2 y carries a graph into the HIP backward
    with pytest.raises(RuntimeError, match='differentiate twice|once_differentiable'):
        g.sum().backward()


def test_refusals():
    from sttode_amd import capi, hypertransformer as ht
    m = ht.trainable(ht.TransformerDecoderLayer(64, 8, 256))
    x = torch.zeros(3, 2, 1, 64, requires_grad=True)
    with pytest.raises(capi.SttodeError):
        m(x, x)
    with pytest.raises(NotImplementedError):
        ht.TransformerDecoderLayer(64, 8, 256, dropout=0.1)
    with pytest.raises(NotImplementedError):
        ht.Hypattention(64, 8, dropout=0.1)


# ---------------------------------------------------------------------------------------------------------------------------------
# training
# ---------------------------------------------------------------------------------------------------------------------------------
def test_sgd_steps_match_float64_oracle_and_adam_lowers_the_loss():
    from sttode_amd import hypertransformer as ht
    m, o = _decoder_pair()
    ht.trainable(m)
    rng = np.random.default_rng(31)
    tgt, mem = rng.standard_normal((6, 4, 2, 64)).astype(np.float32), rng.standard_normal((9, 4, 2, 64)).astype(np.float32)
    target = (0.5 * rng.standard_normal((6, 4, 2, 64))).astype(np.float32)

    def sgd(model, t, mm, tg, n):
        opt = torch.optim.SGD(model.parameters(), lr=0.05)
        for _ in range(n):
            opt.zero_grad()
            loss = ((model(t, mm)[0] - tg) ** 2).mean()
            loss.backward()
            opt.step()
        return {k: p.detach().double().cpu() for k, p in model.named_parameters()}
    d = dev()
    got = sgd(m, torch.from_numpy(tgt).to(d), torch.from_numpy(mem).to(d), torch.from_numpy(target).to(d), 5)
    r32 = sgd(copy.deepcopy(o), torch.from_numpy(tgt), torch.from_numpy(mem), torch.from_numpy(target), 5)
    o64 = copy.deepcopy(o).double()
    r64 = sgd(o64, torch.from_numpy(tgt).double(), torch.from_numpy(mem).double(), torch.from_numpy(target).double(), 5)
    p0 = {k: v.double() for k, v in decoder_state().items()}
    for k in got:                                   # the parameters' movement over the five steps
        close(got[k] - p0[k], r32[k] - p0[k], r64[k] - p0[k], f'SGD x5 update of {k}', floor=1e-3)
    m2, _ = _decoder_pair()
    ht.trainable(m2)
    opt = torch.optim.Adam(m2.parameters(), lr=1e-2)
    t, mm, tg = torch.from_numpy(tgt).to(d), torch.from_numpy(mem).to(d), torch.from_numpy(target).to(d)
    losses = []
    for _ in range(20):
        opt.zero_grad()
        loss = ((m2(t, mm)[0] - tg) ** 2).mean()
        loss.backward()
        opt.step()
        losses.append(float(loss))
    assert losses[-1] < losses[0], losses
