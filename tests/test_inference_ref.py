"""CPU pin of tests/inference_ref.py: the stage restatements composed in float64 reproduce the float64 oracle to 1e-11 relative, composed
in fp32 they reproduce the reference's own vectors (tests/golden/eth_N7, nba_B4, ops) at the band of tests/test_oracle_golden.py, the
integrator agrees with oracle.sttode_ref.ode_integrate_ref and the attention with tests/attention_ref.py."""
import numpy as np
import pytest
import torch

import attention_ref as A
import inference_ref as I
from helpers import ORACLE_ATOL, assert_close, make_args

F64 = torch.float64


def _rel(a, b, what, tol=1e-11):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)
    assert err <= tol, f'{what}: {err:.3e} relative'


def _tight(a, b, what):
    assert_close(a, b, rtol=1e-5, atol=ORACLE_ATOL, what=what)


def _oracle64_scene(net, past, fut, z):
    """The float64 oracle on one scene (loader layout in, test.py:171-186): (past_feature, scene_orig, inference [K, N, Tf, 2])."""
    tr = {}
    with torch.no_grad():
        net.set_data(None, torch.from_numpy(past.transpose(0, 2, 1)).double(), torch.from_numpy(fut.transpose(0, 2, 1)).double())
        out = net.inference(None, z=torch.from_numpy(z).double(), trace=tr)
    return tr['past_feature'].numpy(), net.scene_orig.numpy(), out.numpy()


@pytest.mark.parametrize('Tp,Tf', [(8, 12), (5, 10), (10, 40)])
@pytest.mark.parametrize('sizes', [(7,), (1, 15, 16, 3)], ids=['one-scene', 'ragged'])
def test_float64_stages_reproduce_the_float64_oracle_scenes(Tp, Tf, sizes):
    from sttode_amd import scenes
    net = I.nets(1234, Tp, Tf)['f64']
    past, fut, ptr = I.scene_case(list(sizes), Tp, Tf, seed=Tp)
    n = past.shape[0]
    z = scenes.latents(11 + Tp, n)
    with torch.no_grad():
        o = I.inference_scenes(net, past, ptr, z)
    pred = o['pred'].reshape(n, 20, Tf, 2).permute(1, 0, 2, 3).numpy()
    for s in range(len(sizes)):                                            # the oracle takes one scene at a time
        a, b = int(ptr[s]), int(ptr[s + 1])
        pf, so, out = _oracle64_scene(net, past[a:b], fut[a:b], z[20 * a:20 * b])
        _rel(o['pf'][a:b].numpy(), pf, f'past_feature scene {s}')
        _rel(o['scene_orig'][s], so, f'scene_orig scene {s}')
        _rel(pred[:, a:b], out, f'inference scene {s}')


@pytest.mark.parametrize('Tp,Tf,B,N', [(5, 10, 3, 11), (10, 40, 2, 10), (8, 12, 4, 11)])
def test_float64_stages_reproduce_the_float64_oracle_nba(Tp, Tf, B, N):
    from sttode_amd import scenes
    net = I.nets(1234, Tp, Tf, 'nba')['f64']
    past, fut = I.nba_case(B, N, Tp, Tf)
    z = scenes.latents(5, B * N)
    data = {'past_traj': torch.from_numpy(past).double().reshape(B, N, Tp, 2), 'future_traj': torch.from_numpy(fut).double().reshape(B, N, Tf, 2)}
    tr = {}
    with torch.no_grad():
        net.set_data_nba(data)
        out = net.inference(data, z=torch.from_numpy(z).double(), trace=tr).numpy()
        o = I.inference_nba(net, past, B, N, z)
    _rel(o['pf'].numpy(), tr['past_feature'].numpy(), 'past_feature')
    _rel(o['pred'].reshape(B * N, 20, Tf, 2).permute(1, 0, 2, 3).numpy(), out, 'inference')
    _rel(o['enc_in'], net.inputs.numpy(), 'inputs')


def test_fp32_stages_reproduce_the_reference_vectors(golden):
    from sttode_amd import scenes
    g = golden('eth_N7')
    net = I.nets(1234, 8, 12)['f32']
    past = np.ascontiguousarray(g['obs'].transpose(0, 2, 1))
    with torch.no_grad():
        o = I.inference_scenes(net, past, np.array([0, past.shape[0]], np.int32), g['z'])
    n = past.shape[0]
    _tight(o['pf'].numpy(), g['past_feature'], 'eth_N7 past_feature')
    _tight(o['scene_orig'][0], g['scene_orig'], 'eth_N7 scene_orig')
    _tight(o['pred'].reshape(n, 20, 12, 2).permute(1, 0, 2, 3).numpy(), g['out'], 'eth_N7 inference')
    # x_hat0 = x_true - dbuf, y_hat0 = ybuf (Decoder.forward's trace)
    xt = torch.from_numpy(o['xpad'][:, :16]).repeat_interleave(20, dim=0)
    _tight((xt - o['dbuf']).numpy().reshape(n * 20, 8, 2), g['x_hat0'], 'eth_N7 x_hat0')
    _tight(o['ybuf'][:, :24].numpy().reshape(n * 20, 12, 2), g['y_hat0'], 'eth_N7 y_hat0')
    g = golden('nba_B4')
    net = I.nets(1234, 5, 10, 'nba')['f32']
    d = scenes.nba_batch(int(g['nba_seed']), 4)
    z = scenes.latents(int(g['z_seed']), 44)
    with torch.no_grad():
        o = I.inference_nba(net, d['past_traj'].reshape(44, 5, 2), 4, 11, z)
    st = int(g['stride'])
    _tight(o['pf'].numpy()[::st], g['past_feature'], 'nba_B4 past_feature')
    _tight(o['pred'].reshape(44, 20, 10, 2).permute(1, 0, 2, 3).numpy()[:, ::st], g['out'], 'nba_B4 inference')


def test_fp32_attention_and_layer_reproduce_the_reference_ops(golden):
    from torch.nn import functional as F
    g = golden('ops')
    Wi, bi, Wo, bo = (torch.from_numpy(g[k]) for k in ('w_in_proj_weight', 'w_in_proj_bias', 'w_out_proj.weight', 'w_out_proj.bias'))
    sc = 8.0 ** -0.5
    for L in (1, 6, 128):
        x = torch.from_numpy(g[f'self{L}_x'])
        q, k, v = (F.linear(x, Wi[64 * i:64 * i + 64], bi[64 * i:64 * i + 64]) for i in range(3))
        o = I.attention(k, q, v, 1.0, sc)                               # L == S: rows are keys
        _tight(F.linear(o['out'], Wo, bo).numpy(), g[f'self{L}_out'], f'self-attn L={L}')
        _tight(o['weights'].numpy(), g[f'self{L}_w'], f'self-attn weights L={L}')
    xq, xkv = torch.from_numpy(g['cross_q']), torch.from_numpy(g['cross_kv'])
    q = F.linear(xq, Wi[:64], bi[:64])
    k, v = (F.linear(xkv, Wi[64 * i:64 * i + 64], bi[64 * i:64 * i + 64]) for i in (1, 2))
    o = I.attention(q, k, v, sc, 1.0)
    _tight(F.linear(o['out'], Wo, bo).numpy(), g['cross_out'], 'cross-attn')
    _tight(o['weights'].numpy(), g['cross_w'], 'cross-attn weights')
    # ODEG_Encoder on [L, N, 1, D]: self-attention over L per agent, then the layer and one Euler step
    tr = I.nets(1234, 8, 12)['f32'].past_encoder
    x = torch.from_numpy(g['ode_x'])
    L, N = x.shape[0], x.shape[1]
    with torch.no_grad():
        flat = x.reshape(L * N, 64)
        mha = I._layer(tr).self_attn.temporal_attention_before
        qkv = F.linear(flat, mha.in_proj_weight, mha.in_proj_bias)
        q, k, v = (qkv[:, 64 * i:64 * i + 64].reshape(L, N, 64) for i in range(3))
        attn = I.attention(k, q, v, 1.0, sc)['out'].reshape(L * N, 64)
        pf = I.post_attn(tr, flat, attn)
    _tight(pf[:, 64:].reshape(x.shape).numpy(), g['ode_out'], 'ODEG_Encoder')


@pytest.mark.parametrize('method', [0, 1, 2])
@pytest.mark.parametrize('steps', [1, 3])
def test_post_attn_ode_agrees_with_the_oracle_integrator(method, steps):
    from oracle.sttode_ref import ode_integrate_ref
    tr = I.nets(1234)['f64'].past_encoder
    g = torch.from_numpy(I.trunk_state_case(17)['g']).double()
    with torch.no_grad():
        got = I.post_attn_ode(tr, g, method, steps)
        layer = I._layer(tr)
        f = lambda y: layer(y[None, :, None, :])[0, :, 0, :]             # the oracle's EncoderLayer at attention length 1
        yT = ode_integrate_ref(f, g, I.ODE_TIME, I.ODE_METHODS[method], steps)
        _rel(got.numpy(), torch.cat([g, torch.relu(yT)], -1).numpy(), f'method {method} steps {steps}')
        if (method, steps) == (0, 1):
            _rel(got.numpy(), I.post_attn(tr, g, I.value_of(tr, g)).numpy(), 'Euler, one step == post_attn')


@pytest.mark.parametrize('rows,cols,Nb', [(1, 1, 1), (5, 5, 3), (6, 9, 2), (65, 129, 1)])
def test_attention_agrees_with_attention_ref(rows, cols, Nb):
    rng = np.random.default_rng(rows + cols)
    R, C, V = (torch.from_numpy(rng.standard_normal((l, Nb, 64))) for l in (rows, cols, cols))
    for rs, cs in ((1.0, 8 ** -0.5), (8 ** -0.5, 1.0)):
        o = I.attention(R, C, V, rs, cs)
        out, w = A.core(R, C, V, rs, cs, 0)
        _rel(o['out'].numpy(), out.numpy(), 'out')
        _rel(o['weights'].numpy(), w.numpy(), 'weights')
    for hd in (4, 16):                                                   # other head widths: against the per-head formula written out
        R, C, V = (torch.from_numpy(rng.standard_normal((l, Nb, 8 * hd))) for l in (rows, cols, cols))
        o = I.attention(R, C, V, 1.0, hd ** -0.5, hd)
        for h in (0, 7):
            r, c = R[:, 0, h * hd:(h + 1) * hd], C[:, 0, h * hd:(h + 1) * hd]
            s = -torch.acos(((r / r.norm(dim=-1, keepdim=True)) @ (c / c.norm(dim=-1, keepdim=True)).T).clamp(A.LO, A.HI))
            _rel(o['out'][:, 0, h * hd:(h + 1) * hd].numpy(), (torch.softmax(s, -1) @ V[:, 0, h * hd:(h + 1) * hd]).numpy(), f'hd {hd} head {h}')
            _rel(o['rowsum'][0, h].numpy(), torch.exp(s).sum(-1).numpy(), f'hd {hd} rowsum')


def test_frontend_modes_and_rotation():
    """The NumPy front-end against the oracle's set_data / set_data_nba (float64), both velocity conventions, and the rotation."""
    from oracle.sttode_ref import STTODENetRef
    past, fut, ptr = I.scene_case([6], 8, 12)
    net = STTODENetRef(make_args('eth', 8, 12)).double()
    T64 = lambda a: torch.from_numpy(a.transpose(0, 2, 1)).double()
    net.set_data(None, T64(past), T64(fut))
    fe = I.frontend_scenes(past, ptr, 0)
    _rel(fe['enc_in'], net.inputs.numpy(), 'inputs (world velocities)')
    _rel(fe['cur'], net.cur_location[:, 0].numpy(), 'cur_location')
    ff = I.frontend_future(fut, past[:, -1], 0, fe['scene_orig'], fe['agent_scene'])
    _rel(ff, net.inputs_for_posterior.numpy(), 'inputs_for_posterior')
    fe1 = I.frontend_scenes(past, ptr, 1)
    _rel(fe1['enc_in'][..., 2:], fe['enc_in'][..., 2:], 'velocities of the normalised track', 1e-9)
    th = 0.7
    net.set_data(None, T64(past), T64(fut), theta=th)
    rp, rf = I.rotate_scene(past, fut, np.cos(th), np.sin(th))
    _rel(rp - fe['scene_orig'][0], net.past_traj.numpy(), 'rotated past')
    _rel(rf - fe['scene_orig'][0], net.future_traj.numpy(), 'rotated future')
    pastn, futn = I.nba_case(3, 11)
    netn = STTODENetRef(make_args('nba', 5, 10)).double()
    netn.set_data_nba({'past_traj': torch.from_numpy(pastn).double().reshape(3, 11, 5, 2), 'future_traj': torch.from_numpy(futn).double().reshape(3, 11, 10, 2)})
    fn = I.frontend_nba(pastn, 11)
    _rel(fn['enc_in'], netn.inputs.numpy(), 'nba inputs')
    _rel(I.frontend_future(futn, pastn[:, -1], 1), netn.inputs_for_posterior.numpy(), 'nba inputs_for_posterior')
    assert fn['last'].tolist() == ([0] * 10 + [1]) * 3 and fe['last'].tolist() == [0] * 5 + [1]


def test_stage_functions_are_the_composed_chain():
    """Each decoder stage on the inputs the case generator made reproduces the composed float64 chain's tensor when fed float64 inputs."""
    net = I.nets(1234, 8, 12)['f64']
    c = I.decoder_case(5, 7, 8, 12)
    with torch.no_grad():
        o = I.decode(net, c['pf'], c['z'], c['xpad'], c['cur'], c['orig'], 7, 8, 12)
        b0 = I.mlp_block0(net.decoder, o['A0x'], o['A0y'], c['z'], c['xpad'], 7, 8, 12)
        _rel(b0['dbuf'].numpy(), o['dbuf'].numpy(), 'dbuf')
        # Decoder.forward itself on the same inputs
        pf = torch.from_numpy(c['pf']).double()
        xt = torch.from_numpy(c['xpad'][:, :16]).double().reshape(5, 8, 2)
        out, _ = net.decoder(pf.repeat_interleave(7, 0), torch.from_numpy(c['z']).double(), xt, torch.from_numpy(c['cur']).double()[:, None, :], 7)
        pred = o['pred'] - torch.from_numpy(c['orig']).double().repeat_interleave(7, 0)[:, None, :]
        _rel(pred.numpy(), out.numpy(), 'Decoder.forward', 1e-10)
        xm = I.mlp_cols(net.decoder.decompose[1].decoder_x, torch.zeros(5, 512, dtype=F64), c['z'], o['state1'], 7, 1)
        assert xm.shape == (35, 16)
