"""GPU parity tests (run on a real MI355X: ``pytest -m gpu``).

Every test drives the HIP kernels through the C ABI (sttode_amd.capi -> libsttode_hip.so) and compares with
  (a) the golden vectors produced by the reference itself (tests/golden/*.npz), and
  (b) the CPU oracle (oracle/) on the same seeded inputs.
Tolerance = BASELINE.json north_star: 1e-4 relative on predicted coordinates (plus 1e-4 absolute floor for
values near zero), fp32.  Nothing here reads /root/reference.
"""
import numpy as np
import pytest
import torch

from helpers import (ATOL, RTOL, SAMPLER_CASES, assert_close, grad_case_setup, grad_digest, make_args, oracle_grads, oracle_model,
                     oracle_sampler, oracle_sampler_case, oracle_scene_inference, sampler_args, sampler_case_inputs)

pytestmark = pytest.mark.gpu


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    return torch.device('cuda:0')


_MODELS = {}


def hip_model(dataset='eth', Tp=8, Tf=12, seed=1234):
    from sttode_amd import STTODENet
    from sttode_amd.weights import make_weights, to_torch_state_dict
    key = (dataset, Tp, Tf, seed)
    if key not in _MODELS:
        m = STTODENet(make_args(dataset, Tp, Tf), _gpu()).eval()
        m.load_state_dict(to_torch_state_dict(make_weights(seed, past_length=Tp, future_length=Tf)), strict=True)
        _MODELS[key] = m
    return _MODELS[key]


@pytest.mark.gpu
def test_serial_inference_sees_a_weight_change_made_between_two_calls():
    """inference() compares the parameter versions AFTER enqueueing its launch (the host is the critical path of the one-scene loop) and
    launches again when they changed: the call after an in-place update, a load_state_dict and an optimizer-style step must each return
    the NEW weights' predictions -- bitwise those of a model built on them -- for the one-launch scene form and for a scene batch."""
    from sttode_amd import STTODENet, scenes
    from sttode_amd.weights import make_weights, to_torch_state_dict
    dev = _gpu()
    m = STTODENet(make_args('eth', 8, 12), dev).eval()
    m.load_state_dict(to_torch_state_dict(make_weights(1234)), strict=True)
    obs, pred = scenes.eth_scene(777, n_min=5, n_max=5)
    sb = scenes.make_scene_batch(list(range(900, 940)), 'eth')
    z1 = torch.from_numpy(scenes.latents(3, 5)).to(dev)
    zb = torch.from_numpy(scenes.latents(4, sb.n_agents)).to(dev)

    def both(mod):
        mod.set_data(None, torch.from_numpy(obs), torch.from_numpy(pred))
        a = mod.inference(None, z=z1).clone()
        mod.set_scene_batch(sb.past, sb.future, sb.scene_ptr)
        return a, mod.inference(None, z=zb).clone()

    def fresh():
        f = STTODENet(make_args('eth', 8, 12), dev).eval()
        f.load_state_dict({k: v.detach().clone() for k, v in m.state_dict().items()}, strict=True)
        return both(f)
    base = both(m)
    with torch.no_grad():                                              # in place, as an optimizer step does
        m.decoder.decompose[1].decoder_y.layers[0].weight.mul_(1.25)
        m.past_encoder.input_fc.bias.add_(0.05)
    got, want = both(m), fresh()
    assert not torch.equal(got[0], base[0]) and not torch.equal(got[1], base[1])
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    m.load_state_dict(to_torch_state_dict(make_weights(99)), strict=True)
    got, want = both(m), fresh()
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    again = both(m)                                                    # unchanged weights: one launch, the same bits
    assert torch.equal(again[0], got[0]) and torch.equal(again[1], got[1])


@pytest.mark.gpu
def test_futures_to_host_by_the_copy_kernel_are_the_device_futures():
    """futures_to_host_async: the pinned copies of six pipelined (lagged) calls, made by a few persistent workgroups on the calls' own
    streams, are bitwise the device predictions; odd sizes (n K Tf 2 floats not a multiple of the copy's trip) and a caller-owned pinned
    buffer included; sttode_copy_to_host refuses unaligned / odd-sized arguments."""
    from sttode_amd import scenes, capi
    dev = _gpu()
    m = hip_model('eth')
    sbs = [scenes.make_scene_batch(list(range(7000 + 50 * i, 7000 + 50 * i + 37 + i)), 'eth') for i in range(6)]
    hs, mine = [], torch.empty(sbs[2].n_agents, 20, 12, 2).pin_memory()
    m.native().set_chain(1)
    try:
        for i, sb in enumerate(sbs):
            m.set_scene_batch(sb.past, sb.future, sb.scene_ptr)
            h = m.inference_async(z=torch.from_numpy(scenes.latents(i, sb.n_agents)))
            hs.append(h)
            if i >= 3:
                m.futures_to_host_async(hs[i - 3], out=mine if i - 3 == 2 else None, workgroups=3 + i)
        for i in range(3, 6):
            m.futures_to_host_async(hs[i])
        for i, h in enumerate(hs):
            host = m.wait_host_copy(h)
            assert host.is_pinned() or host._base is not None
            dev_pred = m.wait(h)
            torch.cuda.synchronize()
            assert torch.equal(host, dev_pred.cpu()), i
        assert torch.equal(mine, hs[2]['pred'].cpu())
    finally:
        m.reset_async()
        m.native().set_chain(-1)
    buf = torch.empty(64, device=dev)
    with pytest.raises(capi.SttodeError):
        capi.call('sttode_copy_to_host', mine, buf, 40, 8, capi.stream_ptr())          # not a multiple of 16 bytes
    with pytest.raises(capi.SttodeError):
        capi.call('sttode_copy_to_host', mine.data_ptr() + 4, buf, 64, 8, capi.stream_ptr())   # unaligned destination


@pytest.mark.gpu
def test_eval_scenes_pipelined_equals_serial_over_many_batch_shapes():
    """evaluate.eval_scenes over a stored dataset whose 22 batches all have different agent counts (chain-sized: lagged launches, fused
    metrics): the pipelined loop -- which has to drop its per-shape slot buffers on the way -- returns the serial loop's ADE / FDE."""
    from sttode_amd import datasets, scenes
    from sttode_amd.evaluate import eval_scenes
    _gpu()

    class DS(datasets._SceneDataset):
        def __init__(self):
            sb = scenes.make_scene_batch(range(3000, 3000 + 22 * 70), 'eth')
            cnt = np.diff(sb.scene_ptr)
            ends = np.cumsum(cnt)
            self.seq_start_end = list(zip((ends - cnt).tolist(), ends.tolist()))
            self.num_seq = len(cnt)
            self.obs_traj = torch.from_numpy(np.ascontiguousarray(sb.past.transpose(0, 2, 1)))
            self.pred_traj = torch.from_numpy(np.ascontiguousarray(sb.future.transpose(0, 2, 1)))
    ds = DS()
    m = hip_model('eth')
    zall = scenes.latents(77, int(ds.obs_traj.shape[0]))
    pos = [0]

    def z_fn(rows):                      # the same latents for the same batch in both loops
        z = torch.from_numpy(zall[pos[0]:pos[0] + rows])
        pos[0] += rows
        return z
    a_p, f_p, n_p = eval_scenes(m, ds, scenes_per_call=70, z_fn=z_fn, pipelined=True)
    pos[0] = 0
    a_s, f_s, n_s = eval_scenes(m, ds, scenes_per_call=70, z_fn=z_fn, pipelined=False)
    assert n_p == n_s == ds.obs_traj.shape[0]
    assert abs(a_p - a_s) <= 1e-5 * abs(a_s) and abs(f_p - f_s) <= 1e-5 * abs(f_s), (a_p, a_s, f_p, f_s)


def test_library_loaded_and_fails_loudly_on_cpu():
    from sttode_amd import STTODENet, capi
    _gpu()
    assert capi.lib().sttode_abi_version() == capi.ABI_VERSION
    m = STTODENet(make_args(), 'cpu')
    m.set_data(None, torch.zeros(3, 2, 8), torch.zeros(3, 2, 12))
    with pytest.raises(capi.SttodeError):
        m.inference(None)
    with pytest.raises(capi.SttodeError):
        capi.call('sttode_best_of_k', None, None, 0, 0, 0, 1.0, None, None, None)


def test_linear_cols_mfma_layout():
    """PK16 packing + v_mfma_f32_16x16x4_f32 lane map: asymmetric random W, ragged column count, two K segments."""
    from sttode_amd import capi, packing
    dev = _gpu()
    rng = np.random.default_rng(0)
    for ncols, K1, K2, N in ((37, 128, 96, 512), (16, 64, 0, 192), (5, 16, 16, 16)):
        W = rng.standard_normal((N, K1 + K2)).astype(np.float32)
        b = rng.standard_normal(N).astype(np.float32)
        X1 = rng.standard_normal((ncols, K1)).astype(np.float32)
        X2 = rng.standard_normal((ncols, max(K2, 4))).astype(np.float32)
        out = torch.zeros(ncols, N, device=dev)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        capi.call('sttode_linear_cols', t(X1), K1, K1, t(X2) if K2 else None, X2.shape[1], K2, t(packing.pk16(W)), t(b), out, N,
                  ncols, N, 0, capi.stream_ptr())
        ref = np.concatenate([X1, X2[:, :K2]], 1).astype(np.float64) @ W.T.astype(np.float64) + b
        assert_close(out.cpu().numpy(), ref, rtol=1e-5, atol=1e-4, what=f'linear_cols {ncols}x{K1}+{K2}->{N}')


@pytest.mark.parametrize('Tp,ncols', [(8, 50), (5, 16), (10, 33)])
def test_gru_cols_vs_torch(Tp, ncols):
    """conv1d+relu+GRU final state (model/STTODE.py:62-69) vs torch CPU ops on the same weights."""
    from sttode_amd import capi, packing
    from sttode_amd.weights import make_weights
    dev = _gpu()
    sd = make_weights(1234, past_length=Tp, future_length=12)
    P = packing.pack_block(sd, 1, Tp, 12, first=False)
    TPX = packing.tiles_x(Tp)
    rng = np.random.default_rng(Tp)
    x = rng.standard_normal((ncols, Tp, 2)).astype(np.float32)
    xin = np.zeros((ncols, 16 * TPX), np.float32)
    xin[:, :2 * Tp] = x.reshape(ncols, -1)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    state = torch.zeros(ncols, 96, device=dev)
    capi.call('sttode_gru_cols', t(xin), t(P['convP']), t(P['convB']), t(P['wihP']), t(P['whhP']), t(P['gbias']), state, ncols, Tp, TPX,
              capi.stream_ptr())
    from oracle.sttode_ref import DecomposeBlock
    blk = DecomposeBlock(Tp, 12, 160)
    blk.load_state_dict({k[len('decoder.decompose.1.'):]: torch.from_numpy(v) for k, v in sd.items() if k.startswith('decoder.decompose.1.')})
    with torch.no_grad():
        e = torch.relu(blk.conv_past(torch.from_numpy(x).transpose(1, 2))).transpose(1, 2)
        ref = blk.encoder_past(e)[1].squeeze(0).numpy()
    assert_close(state.cpu().numpy(), ref, rtol=1e-4, atol=2e-5, what='gru state')


@pytest.mark.parametrize('Tp,ncols', [(8, 300), (5, 129), (10, 31)])
def test_streaming_gru_cols32_vs_resident_form(Tp, ncols):
    """sttode_gru_cols32 (32-column tiles, weights streamed per step) == sttode_gru_cols (16-column tiles, weights resident in LDS) on
    the same inputs: ragged column counts, Tp 5 / 8 / 10 (ldx 16 and 32)."""
    from sttode_amd import capi, packing
    from sttode_amd.weights import make_weights
    dev = _gpu()
    sd = make_weights(1234, past_length=Tp, future_length=12)
    P = packing.pack_block(sd, 0, Tp, 12, first=True)
    G = packing.gru32_stream(sd, 0, Tp)
    TPX = packing.tiles_x(Tp)
    rng = np.random.default_rng(100 + Tp)
    xin = np.zeros((ncols, 16 * TPX), np.float32)
    xin[:, :2 * Tp] = rng.standard_normal((ncols, 2 * Tp)).astype(np.float32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    x = t(xin)
    ref, got = torch.zeros(ncols, 96, device=dev), torch.zeros(ncols, 96, device=dev)
    capi.call('sttode_gru_cols', x, t(P['convP']), t(P['convB']), t(P['wihP']), t(P['whhP']), t(P['gbias']), ref, ncols, Tp, TPX, capi.stream_ptr())
    capi.call('sttode_gru_cols32', x, 16 * TPX, t(G['pool']), t(G['prog']), G['prog_len'], t(G['consts']), got, ncols, Tp, capi.stream_ptr())
    assert_close(got.cpu().numpy(), ref.cpu().numpy(), rtol=2e-5, atol=2e-5, what=f'gru_cols32 Tp={Tp}')


@pytest.mark.parametrize('N', [2, 7, 32])
def test_eth_scene_vs_reference_golden(golden, N):
    g = golden(f'eth_N{N}')
    m = hip_model('eth', 8, 12)
    m.set_data(None, torch.from_numpy(g['obs']), torch.from_numpy(g['pred']))
    out = m.inference(None, z=torch.from_numpy(g['z']))
    assert tuple(out.shape) == (20, N, 12, 2)
    assert_close(m.scene_orig.cpu().numpy(), g['scene_orig'], what='scene_orig')
    assert_close(m.past_feature.cpu().numpy(), g['past_feature'], what='past_feature')
    # intermediates of the decomposition decoder
    xpad = m._ws['xpad'].cpu().numpy()[:, :16].reshape(N, 1, 8, 2)
    x_hat0 = (xpad - m._dbg['dbuf'].cpu().numpy()[:, :16].reshape(N, 20, 8, 2)).reshape(N * 20, 8, 2)
    assert_close(x_hat0, g['x_hat0'], what='x_hat0')
    assert_close(m._dbg['ybuf'].cpu().numpy()[:, :24].reshape(N * 20, 12, 2), g['y_hat0'], what='y_hat0')
    assert_close(out.cpu().numpy(), g['out'], what='inference output')
    # metrics on device vs the reference's utils/metrics.py numbers
    ade, fde = m.best_of_k(out.permute(1, 0, 2, 3), torch.from_numpy(g['pred'].transpose(0, 2, 1).copy()))
    assert abs(float(ade.mean()) - float(g['ade'])) < 1e-4 * max(1.0, float(g['ade']))
    assert abs(float(fde.mean()) - float(g['fde'])) < 1e-4 * max(1.0, float(g['fde']))


def test_sdd_ragged_batched_vs_reference_golden(golden):
    """Four ragged scenes (N = 1, 3, 17, 40) in ONE batched call == the reference's per-scene outputs."""
    g = golden('sdd_ragged')
    m = hip_model('eth', 8, 12)
    past = np.concatenate([g[f's{i}_obs'].transpose(0, 2, 1) for i in range(4)])
    fut = np.concatenate([g[f's{i}_pred'].transpose(0, 2, 1) for i in range(4)])
    z = np.concatenate([g[f's{i}_z'] for i in range(4)])
    ptr = np.cumsum([0] + [g[f's{i}_obs'].shape[0] for i in range(4)]).astype(np.int32)
    m.set_scene_batch(past, fut, ptr)
    out = m.inference(None, z=torch.from_numpy(z)).cpu().numpy()
    pf = m.past_feature.cpu().numpy()
    for i in range(4):
        a, b = ptr[i], ptr[i + 1]
        assert_close(pf[a:b], g[f's{i}_past_feature'], what=f'sdd scene {i} past_feature')
        assert_close(out[:, a:b], g[f's{i}_out'], what=f'sdd scene {i}')


@pytest.mark.parametrize('B', [4, 32, 128])
def test_nba_batch_attention_vs_reference_golden(golden, B):
    """NBA path: batch-as-sequence geodesic attention (L = B) with the untransposed-score quirk."""
    from sttode_amd import scenes
    g = golden(f'nba_B{B}')
    m = hip_model('nba', 5, 10)
    d = scenes.nba_batch(int(g['nba_seed']), B)
    z = scenes.latents(int(g['z_seed']), B * 11)
    data = {'past_traj': torch.from_numpy(d['past_traj']), 'future_traj': torch.from_numpy(d['future_traj'])}
    m.set_data_nba(data)
    out = m.inference(data, z=torch.from_numpy(z)).cpu().numpy()
    st = int(g['stride'])
    assert_close(m.past_feature.cpu().numpy()[::st], g['past_feature'], what='past_feature')
    assert_close(out[:, ::st], g['out'], what='nba inference')


def test_long_horizon_vs_reference_golden(golden):
    """BASELINE config-5 shapes: Tp=10, Tf=40, N=10 (TPX=2, NOY=5 instantiation)."""
    from sttode_amd import scenes
    g = golden('nba_long_B8')
    m = hip_model('nba', 10, 40)
    d = scenes.nba_batch(8, 8, N=10, obs_len=10, pred_len=40)
    z = scenes.latents(4100, 80)
    data = {'past_traj': torch.from_numpy(d['past_traj']), 'future_traj': torch.from_numpy(d['future_traj'])}
    m.set_data_nba(data)
    out = m.inference(data, z=torch.from_numpy(z)).cpu().numpy()
    assert_close(out, g['out'], what='long horizon')


def test_mhgsa_op_vs_reference_golden(golden):
    """Stand-alone MHGSA op (Hyp_mhsa.forward): self-attention L in {1,6,128} and cross-attention L=6,S=9."""
    from sttode_amd.ops import mhgsa
    dev = _gpu()
    g = golden('ops')
    W = [torch.from_numpy(g[k]).to(dev) for k in ('w_in_proj_weight', 'w_in_proj_bias', 'w_out_proj.weight', 'w_out_proj.bias')]
    for L in (1, 6, 128):
        x = torch.from_numpy(g[f'self{L}_x']).to(dev)
        o, w = mhgsa(x, x, x, *W, need_weights=True)
        assert_close(o.cpu().numpy(), g[f'self{L}_out'], what=f'mhgsa self L={L}')
        assert_close(w.cpu().numpy(), g[f'self{L}_w'], rtol=1e-4, atol=1e-6, what=f'mhgsa weights L={L}')
    q, kv = torch.from_numpy(g['cross_q']).to(dev), torch.from_numpy(g['cross_kv']).to(dev)
    o, w = mhgsa(q, kv, kv, *W, need_weights=True)
    assert_close(o.cpu().numpy(), g['cross_out'], what='mhgsa cross')
    assert_close(w.cpu().numpy(), g['cross_w'], rtol=1e-4, atol=1e-6, what='mhgsa cross weights')


def test_best_of_k_vs_reference_golden(golden):
    g = golden('metrics')
    m = hip_model('eth', 8, 12)
    ade, fde = m.best_of_k(torch.from_numpy(g['pred']).to(m.device), torch.from_numpy(g['gt']))
    assert abs(float(ade.double().mean()) - float(g['ade'])) < 1e-5
    assert abs(float(fde.double().mean()) - float(g['fde'])) < 1e-5


def test_batched_scenes_full_size_properties():
    """BASELINE config[1] size: 512 ETH-shaped scenes, K=20, one call.
    (1) a sample of scenes equals the CPU oracle run scene by scene (test.py:171-184 structure);
    (2) scene independence: the batched result equals per-scene HIP calls bit for bit, for BOTH forms of the per-trajectory
        stage (fused chain kernel, csrc/chain32.hip; three-kernel form, csrc/decoder.hip) -- the two forms use different MFMA
        shapes, i.e. different summation orders, so across forms the results agree to rounding (checked at 2e-5), not bitwise;
    (3) determinism: two runs are bitwise identical;  (4) device ADE/FDE equal the NumPy oracle."""
    from oracle.metrics_ref import best_of_k_ade_fde
    from sttode_amd import scenes
    m = hip_model('eth', 8, 12)
    sb = scenes.make_scene_batch(range(512), 'eth')
    z = scenes.latents(99, sb.n_agents)
    ora = oracle_model('eth', 8, 12)
    per_form = {}
    try:
        for form in (1, 0):
            m.native().set_chain(form)
            m.set_scene_batch(sb.past, sb.future, sb.scene_ptr)
            out = m.inference(None, z=torch.from_numpy(z))
            out2 = m.inference(None, z=torch.from_numpy(z))
            assert torch.equal(out, out2)
            o = out.cpu().numpy()
            assert np.isfinite(o).all()
            per_form[form] = o
            for s in (0, 1, 17, 255, 511):
                a, b = int(sb.scene_ptr[s]), int(sb.scene_ptr[s + 1])
                obs, pred = sb.scene(s)
                ref = oracle_scene_inference(ora, obs, pred, z[a * 20:b * 20])
                assert_close(o[:, a:b], ref, what=f'form {form} scene {s} vs oracle')
                m.set_data(None, torch.from_numpy(obs), torch.from_numpy(pred))
                single = m.inference(None, z=torch.from_numpy(z[a * 20:b * 20])).cpu().numpy()
                assert np.array_equal(single, o[:, a:b]), f'form {form} scene {s}: batched != per-scene'
        assert_close(per_form[1], per_form[0], rtol=2e-5, atol=2e-5, what='fused chain vs three-kernel form')
    finally:
        m.native().set_chain(-1)
    m.set_scene_batch(sb.past, sb.future, sb.scene_ptr)
    out = m.inference(None, z=torch.from_numpy(z))     # automatic mode picks the fused chain at this size
    assert np.array_equal(out.cpu().numpy(), per_form[1])
    o = per_form[1]
    ade, fde = m.best_of_k(out.permute(1, 0, 2, 3))
    ra, rf = best_of_k_ade_fde(o.transpose(1, 0, 2, 3), sb.future)
    assert_close(ade.cpu().numpy(), ra, rtol=1e-5, atol=1e-5, what='ade')
    assert_close(fde.cpu().numpy(), rf, rtol=1e-5, atol=1e-5, what='fde')


@pytest.mark.parametrize('case', ['eth_ragged', 'tiny', 'nba', 'nba_long', 'k_not_20'])
def test_fused_trajectory_chain_vs_three_kernel_form_and_oracle(case):
    """sttode_traj_chain (one persistent kernel: decoder_x -> d -> decoder_y -> conv+GRU -> decoder_y -> epilogue, 32x32x2 MFMA,
    all weights streamed) against the three-kernel form on identical inputs and against the CPU oracle: ragged column counts
    (not a multiple of the 128-trajectory group), fewer columns than one group, the NBA shapes (Tp 5 / Tf 10) and the
    long-horizon shapes (Tp 10 / Tf 40: ldx = 32, three output tiles)."""
    from sttode_amd import scenes
    if case in ('eth_ragged', 'tiny', 'k_not_20'):
        m, ora = hip_model('eth', 8, 12), oracle_model('eth', 8, 12)
        sb = scenes.make_scene_batch(range(900, 900 + (1 if case == 'tiny' else 61)), 'eth')
        z = scenes.latents(31, sb.n_agents)
        if case == 'k_not_20':      # K = 7 samples per agent (the kernels take K as an argument; the reference hard-codes 20)
            from sttode_amd import STTODENet
            a7 = make_args('eth', 8, 12)
            a7.sample_k = 7
            m7 = STTODENet(a7, _gpu()).eval()
            m7.load_state_dict(m.state_dict(), strict=True)
            m, z = m7, scenes.latents(31, sb.n_agents, K=7)
        feed = lambda: m.set_scene_batch(sb.past, sb.future, sb.scene_ptr)
    else:
        Tp, Tf, B, N = (5, 10, 24, 11) if case == 'nba' else (10, 40, 12, 10)
        m, ora = hip_model('nba', Tp, Tf), oracle_model('nba', Tp, Tf)
        d = scenes.nba_batch(41, B, N=N, obs_len=Tp, pred_len=Tf)
        z = scenes.latents(32, B * N)
        data = {'past_traj': torch.from_numpy(d['past_traj']), 'future_traj': torch.from_numpy(d['future_traj'])}
        feed = lambda: m.set_data_nba(data)
    outs = {}
    try:
        for form in (0, 1):
            m.native().set_chain(form)
            feed()
            outs[form] = m.inference(None, z=torch.from_numpy(z)).cpu().numpy()
            feed()
            assert np.array_equal(m.inference(None, z=torch.from_numpy(z)).cpu().numpy(), outs[form])
    finally:
        m.native().set_chain(-1)
    assert np.isfinite(outs[1]).all()
    assert_close(outs[1], outs[0], rtol=2e-5, atol=2e-5, what=f'{case}: fused chain vs three-kernel form')
    if case in ('eth_ragged', 'tiny'):
        for s in range(0, sb.n_scenes, 9):
            a, b = int(sb.scene_ptr[s]), int(sb.scene_ptr[s + 1])
            obs, pred = sb.scene(s)
            assert_close(outs[1][:, a:b], oracle_scene_inference(ora, obs, pred, z[a * 20:b * 20]), what=f'{case} scene {s} vs oracle')
    elif case == 'k_not_20':
        # the reference's inference() hard-codes 20 samples (model/STTODE.py:600), so the oracle is driven through the components it is made
        # of: PastEncoder.forward (:214-236) and Decoder.forward (:320-347) with sample_num = 7, scene by scene
        from oracle.sttode_ref import first_diff_dup
        for s in range(0, sb.n_scenes, 9):
            a, b = int(sb.scene_ptr[s]), int(sb.scene_ptr[s + 1])
            obs, pred = sb.scene(s)
            with torch.no_grad():
                ora.set_data(None, torch.from_numpy(obs), torch.from_numpy(pred))
                pt = ora.past_traj
                pf = ora.past_encoder(torch.cat((pt, first_diff_dup(pt)), dim=-1), 1, ora.agent_num)
                out, _ = ora.decoder(pf.repeat_interleave(7, dim=0), torch.from_numpy(z[a * 7:b * 7]), pt, pt[:, -1:], sample_num=7, mode='inference')
                ref = (out.permute(1, 0, 2, 3) + ora.scene_orig).numpy()
            assert_close(outs[1][:, a:b], ref, what=f'{case} scene {s} vs oracle components')
            assert_close(outs[0][:, a:b], ref, what=f'{case} scene {s} (three-kernel form) vs oracle components')
    else:
        with torch.no_grad():
            ora.set_data_nba(data)
            ref = ora.inference(data, z=torch.from_numpy(z)).numpy()
        assert_close(outs[1], ref, what=f'{case} vs oracle')


@pytest.mark.parametrize('case', ['eth_1', 'eth_7', 'eth_32', 'eth_3scenes', 'nba', 'nba_long'])
def test_latency_forms_are_bitwise_the_throughput_forms_and_match_oracle(case):
    """The few-column (single scene, test.py:171-188) forms of embed_qkv / gru_cols / mlp_block0 / mlp_block1 -- one 16-column tile per WORKGROUP,
    rows split over its waves -- sum in the order of the throughput forms (a tile per wave): identical bits with the crossover
    forced either way (sttode_set_latency_tiles), and both match the CPU oracle."""
    from sttode_amd import capi, scenes
    if case.startswith('eth'):
        m, ora = hip_model('eth', 8, 12), oracle_model('eth', 8, 12)
        if case == 'eth_3scenes':
            sb = scenes.make_scene_batch(range(700, 703), 'eth')
        else:
            n = int(case.split('_')[1])
            o, p_ = scenes.eth_scene(5100 + n, n_min=n, n_max=n)
            sb = scenes.SceneBatch(np.ascontiguousarray(o.transpose(0, 2, 1)), np.ascontiguousarray(p_.transpose(0, 2, 1)),
                                   np.asarray([0, n], np.int32))
        z = scenes.latents(77, sb.n_agents)
        feed = lambda: m.set_scene_batch(sb.past, sb.future, sb.scene_ptr)
    else:
        Tp, Tf, B, N = (5, 10, 2, 11) if case == 'nba' else (10, 40, 3, 10)
        m, ora = hip_model('nba', Tp, Tf), oracle_model('nba', Tp, Tf)
        d = scenes.nba_batch(43, B, N=N, obs_len=Tp, pred_len=Tf)
        z = scenes.latents(33, B * N)
        data = {'past_traj': torch.from_numpy(d['past_traj']), 'future_traj': torch.from_numpy(d['future_traj'])}
        feed = lambda: m.set_data_nba(data)
    outs = {}
    try:
        m.native().set_chain(0)
        for tiles in (0, 1 << 30):
            capi.call('sttode_set_latency_tiles', tiles, tiles, tiles)
            feed()
            outs[tiles] = m.inference(None, z=torch.from_numpy(z)).cpu().numpy()
    finally:
        capi.call('sttode_set_latency_tiles', 512, 1024, 1024)
        m.native().set_chain(-1)
    assert np.isfinite(outs[0]).all()
    assert np.array_equal(outs[0], outs[1 << 30]), f'{case}: max diff {np.abs(outs[0] - outs[1 << 30]).max():.3e}'
    if case.startswith('eth'):
        for s in range(sb.n_scenes):
            a, b = int(sb.scene_ptr[s]), int(sb.scene_ptr[s + 1])
            obs, pred = sb.scene(s)
            assert_close(outs[0][:, a:b], oracle_scene_inference(ora, obs, pred, z[a * 20:b * 20]), what=f'{case} scene {s} vs oracle')
    else:
        with torch.no_grad():
            ora.set_data_nba(data)
            ref = ora.inference(data, z=torch.from_numpy(z)).numpy()
        assert_close(outs[0], ref, what=f'{case} vs oracle')


def test_pmath_op_library_vs_reference_golden(golden):
    """Every hyptorch/pmath.py primitive on HIP vs values produced by the reference's own functions."""
    import sttode_amd.pmath as pm
    dev = _gpu()
    g = golden('pmath')
    T = lambda a: torch.from_numpy(a).to(dev)
    for c in (1.0, 0.5):
        t = f'c{c}_'
        x, y, u, mat = (T(g[t + k]) for k in ('x', 'y', 'u', 'm'))
        xb, yb = pm.project(x, c=c), pm.project(y, c=c)
        checks = {
            'project': xb, 'lambda_x': pm.lambda_x(xb, c=c), 'mobius_add': pm.mobius_add(xb, yb, c=c), 'dist': pm.dist(xb, yb, c=c),
            'dist0': pm.dist0(xb, c=c), 'expmap': pm.expmap(xb, u, c=c), 'expmap0': pm.expmap0(u, c=c), 'logmap': pm.logmap(xb, yb, c=c),
            'logmap0': pm.logmap0(xb, c=c), 'mobius_matvec': pm.mobius_matvec(mat, xb, c=c), 'p2k': pm.p2k(xb, c),
            'k2p': pm.k2p(pm.p2k(xb, c), c), 'lorenz': pm.lorenz_factor(pm.p2k(xb, c), c=c),
            'poincare_mean': pm.poincare_mean(xb, dim=0, c=c), 'dist_matrix': pm.dist_matrix(xb, yb[:9], c=c),
            'mobius_addition_batch': pm._mobius_addition_batch(xb[:6], yb[:5], c),
            'hyperbolic_softmax': pm._hyperbolic_softmax(xb, mat * 0.5, pm.project(mat * 0.3, c=c), c),
        }
        # Rows that project() clipped to the ball boundary (|x| = (1-1e-3)/sqrt(c): x row 2 by construction plus any random row
        # that happened to fall outside) are ILL-CONDITIONED for every op that forms 1 - c|x|^2 or artanh(|.|) near 1: a 1-ulp
        # change of the input moves the fp32 result by 1e-3..1e-1 relative, so two correct fp32 implementations disagree there.
        # Yardstick for those entries: the same op evaluated in FLOAT64 (oracle/pmath_ref.py is dtype-generic) on the very fp32
        # inputs each implementation used.  Required: HIP's error against that truth is no more than twice the error of the
        # reference's own fp32 result against ITS truth (or 1e-4 relative, whichever is larger).  All other entries: 1e-4.
        import oracle.pmath_ref as pref
        maxn = (1 - 1e-3) / np.sqrt(c)
        bx = (xb.norm(dim=-1) > 0.99 * maxn).cpu().numpy()
        by = (yb.norm(dim=-1) > 0.99 * maxn).cpu().numpy()
        D = lambda a: torch.from_numpy(np.asarray(a)).double()
        u64, m64 = D(g[t + 'u']), D(g[t + 'm'])

        def truth(xq, yq, kq):                # every op in float64 on the fp32 values each op actually received: projected points
            xq, yq, k = D(xq), D(yq), D(kq)   # xq, yq [33,16]; kq = the fp32 Klein coordinates fed to k2p / lorenz_factor
            return {'project': xq, 'lambda_x': pref.lambda_x(xq, c), 'mobius_add': pref.mobius_add(xq, yq, c), 'dist': pref.dist(xq, yq, c),
                    'dist0': pref.dist0(xq, c), 'expmap': pref.expmap(xq, u64, c), 'expmap0': pref.expmap0(u64, c),
                    'logmap': pref.logmap(xq, yq, c), 'logmap0': pref.logmap0(xq, c), 'mobius_matvec': pref.mobius_matvec(m64, xq, c),
                    'p2k': pref.p2k(xq, c), 'k2p': pref.k2p(k, c), 'lorenz': pref.lorenz_factor(k, c), 'poincare_mean': pref.poincare_mean(xq, c),
                    'dist_matrix': pref.dist_matrix(xq, yq[:9], c), 'mobius_addition_batch': pref.mobius_addition_batch(xq[:6], yq[:5], c),
                    'hyperbolic_softmax': pref.hyperbolic_softmax(xq, m64 * 0.5, pref.project(m64 * 0.3, c), c)}
        t_hip = {k: v.numpy() for k, v in truth(xb.cpu().numpy(), yb.cpu().numpy(), checks['p2k'].cpu().numpy()).items()}
        t_ref = {k: v.numpy() for k, v in truth(g[t + 'project'], pref.project(torch.from_numpy(g[t + 'y']), c).numpy(), g[t + 'p2k']).items()}

        def rel_rows(a, tr):                  # per leading-index relative error (max over the trailing axes), float64
            a, tr = np.asarray(a, np.float64), np.asarray(tr, np.float64)
            a, tr = a.reshape(a.shape[0], -1) if a.ndim > 1 else a[:, None], tr.reshape(tr.shape[0], -1) if tr.ndim > 1 else tr[:, None]
            return np.abs(a - tr).max(1) / (np.abs(tr).max(1) + 1e-6)

        for k, v in checks.items():
            got, ref = v.cpu().numpy(), g[t + k]
            if k == 'poincare_mean':
                # the Lorenz factors of the boundary rows (~20x the others, themselves ill-conditioned) weight the whole mean
                e_hip = np.abs(got - t_hip[k]).max() / np.abs(t_hip[k]).max()
                e_ref = np.abs(ref - t_ref[k]).max() / np.abs(t_ref[k]).max()
                assert e_hip <= max(2 * e_ref, 1e-4), (k, c, e_hip, e_ref)
                inner = xb[torch.from_numpy(~bx).to(xb.device)]
                np.testing.assert_allclose(pm.poincare_mean(inner, dim=0, c=c).cpu().numpy(), pref.poincare_mean(inner.cpu(), c).numpy(),
                                           rtol=1e-4, atol=2e-6, err_msg=f'{k} c={c} (interior rows vs oracle)')
                continue
            if k in ('dist_matrix', 'mobius_addition_batch'):
                bad = bx[:ref.shape[0], None] | by[None, :ref.shape[1]]
            elif k == 'expmap0':
                bad = np.zeros(ref.shape[0], bool)
            else:
                bad = bx | by if k in ('mobius_add', 'dist', 'logmap') else bx
            np.testing.assert_allclose(got[~bad], ref[~bad], rtol=1e-4, atol=2e-6, err_msg=f'{k} c={c}', equal_nan=True)
            if bad.any():
                if bad.ndim == 2:             # pairwise ops: entry-wise (flatten the [P, R] index)
                    sel = bad.reshape(-1)
                    shp = (-1,) + got.shape[2:]
                    e_hip = rel_rows(got.reshape(shp)[sel], t_hip[k].reshape(shp)[sel])
                    e_ref = rel_rows(ref.reshape(shp)[sel], t_ref[k].reshape(shp)[sel])
                else:
                    e_hip, e_ref = rel_rows(got[bad], t_hip[k][bad]), rel_rows(ref[bad], t_ref[k][bad])
                ok = e_hip <= np.maximum(2 * e_ref, 1e-4)
                assert ok.all(), f'{k} c={c} boundary entries: HIP error vs float64 {e_hip[~ok]} > 2 x reference fp32 error {e_ref[~ok]}'
    s = T(g['scalar_in'])
    np.testing.assert_allclose(pm.tanh(s).cpu().numpy(), g['tanh'], rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(pm.artanh(s).cpu().numpy(), g['artanh'], rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(pm.arsinh(s * 30).cpu().numpy(), g['arsinh'], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose([pm.auto_select_c(d) for d in (2, 8, 16, 64)], g['auto_select_c'], rtol=1e-12)
    o = golden('ops')
    a, b = T(o['obl_a']), T(o['obl_b'])
    np.testing.assert_allclose(pm.oblique_proj(a).cpu().numpy(), o['obl_proj_a'], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(pm.oblique_dist(pm.oblique_proj(a), pm.oblique_proj(b)).cpu().numpy(), o['obl_dist'], rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize('case', ['eth_61', 'eth_512', 'eth_long', 'nba_128', 'nba_long'])
def test_fused_launch_is_bitwise_the_separate_per_agent_launches(case):
    """Round 3: the per-agent stage as leading workgroups of the chain launch (csrc/chain32.hip agent_role; one flag per 16-agent tile,
    sc1 payload stores, consumer poll + agent-scope acquire) against the separate per-agent launches: predictions AND every per-agent
    intermediate (g, qkv, pf, state0, the three layer-1 tables) bit for bit.  Scene batches (the roles run the embedding too), a long
    horizon (Tp 10: two input tiles), and the NBA branch (attention groups > 1: embedding and attention stay launches in front).
    The hand-off is exercised the way the guide asks (uneven load, warm caches, every word): the SAME workspace is reused by
    back-to-back calls with DIFFERENT inputs, serially and with three calls in flight, so a stale L1 / L2 line or a flag that overtakes
    its payload shows up as a mismatch."""
    from sttode_amd import scenes
    variants = []
    if case.startswith('eth'):
        Tp, Tf = (10, 40) if case == 'eth_long' else (8, 12)
        m = hip_model('eth', Tp, Tf)
        nsc = {'eth_61': 61, 'eth_512': 512, 'eth_long': 40}[case]
        sb = scenes.make_scene_batch(range(2000, 2000 + nsc), 'eth', obs_len=Tp, pred_len=Tf) if case == 'eth_long' else \
            scenes.make_scene_batch(range(2000, 2000 + nsc), 'eth')
        n, S = sb.n_agents, sb.n_scenes
        for v in range(4):                                    # same shapes (one workspace), different numbers
            past = (sb.past * (1.0 + 0.03 * v) + 0.1 * v).astype(np.float32)
            variants.append(((torch.from_numpy(past).to(m.device), torch.from_numpy(sb.future).to(m.device),
                              torch.from_numpy(sb.scene_ptr).to(m.device)), torch.from_numpy(scenes.latents(300 + v, n)).to(m.device)))
        feed = lambda inp: m.set_scene_batch(*inp)
    else:
        Tp, Tf, B, N = (5, 10, 128, 11) if case == 'nba_128' else (10, 40, 64, 10)
        m = hip_model('nba', Tp, Tf)
        n, S = B * N, 0
        for v in range(4):
            d = scenes.nba_batch(60 + v, B, N=N, obs_len=Tp, pred_len=Tf)
            variants.append(({'past_traj': torch.from_numpy(d['past_traj']).to(m.device), 'future_traj': torch.from_numpy(d['future_traj']).to(m.device)},
                             torch.from_numpy(scenes.latents(300 + v, n)).to(m.device)))
        feed = lambda inp: m.set_data_nba(inp)
    names = (('g', 64), ('qkv', 192), ('pf', 128), ('state0', 96), ('A0x', 512), ('A0y', 512), ('A1y', 512),
             ('xpad', 16 * (1 if 2 * Tp <= 16 else 2)), ('enc_in', 4 * Tp), ('cur', 2), ('orig', 2))

    def run(v, fused):
        inp, z = variants[v]
        m.native().set_fused(fused)
        feed(inp)
        out = m.inference(None, z=z).clone()
        buf, off = m._workspace(n, S)
        inter = {k: m._view(buf, off, k, n, w).clone() for k, w in names}
        if S:
            inter['scene_orig'] = m._view(buf, off, 'scene_orig', S, 2).clone()
        return out, inter
    # Tp > 8 (two 16-wide input tiles): the separate launches run block 0's GRU in its streaming 32-column form (another summation order),
    # the role in the 16-column latency form -> agreement to rounding there, bitwise everywhere else; the fused launch itself must
    # reproduce its own bits on every repetition either way
    bitwise = case not in ('eth_long', 'nba_long')
    try:
        m.native().set_chain(1)                           # some of the batches are below the automatic chain threshold
        ref = [run(v, 0) for v in range(4)]
        if not bitwise:
            first = [run(v, 1) for v in range(4)]
            for v in range(4):
                assert_close(first[v][0].cpu().numpy(), ref[v][0].cpu().numpy(), rtol=2e-5, atol=2e-5, what=f'{case} variant {v}: fused vs separate launches')
                for k in first[v][1]:
                    assert_close(first[v][1][k].cpu().numpy(), ref[v][1][k].cpu().numpy(), rtol=2e-5, atol=2e-5, what=f'{case} variant {v}: {k}')
            ref = first
        for rep in range(4):
            for v in (0, 3, 1, 2):
                out, inter = run(v, 1)
                assert torch.isfinite(out).all()
                assert torch.equal(out, ref[v][0]), f'{case} variant {v} rep {rep}: fused launch != separate launches'
                for k in inter:
                    assert torch.equal(inter[k], ref[v][1][k]), f'{case} variant {v} rep {rep}: {k} differs'
        # three calls in flight on the pipeline's streams, workspace slots reused every third call (the round-3 pipelined form: one call
        # per fused launch; the default lagged form has its own tests below)
        m.native().set_lagged(0)
        m.reset_async()
        handles, outs, order = [], [], [0, 1, 2, 3, 2, 0, 3, 1, 1, 0]
        for v in order:
            inp, z = variants[v]
            feed(inp)
            handles.append(m.inference_async(z=z))
            if len(handles) >= 3:
                outs.append(m.wait(handles.pop(0)).clone())
        while handles:
            outs.append(m.wait(handles.pop(0)).clone())
        torch.cuda.synchronize()
        for i, v in enumerate(order):
            assert torch.equal(outs[i], ref[v][0]), f'{case} pipelined call {i} (variant {v}): fused launch != separate launches'
    finally:
        m.native().set_fused(1)
        m.native().set_chain(-1)
        m.reset_async()
        m.native().set_lagged(3)


GOLDEN_INFERENCE_CASES = ['eth_N2', 'eth_N7', 'eth_N32', 'sdd_ragged', 'nba_B4', 'nba_B32', 'nba_B128', 'nba_long_B8']


def _golden_inference_case(golden, case, what):
    """-> (model, feed(), z, check(out)) of one reference-golden inference case (tests/golden/*.npz: inputs, injected latents and the
    REFERENCE's own inference() output): ETH N = 2 / 7 / 32, the four ragged SDD scenes in one batch, NBA B = 4 / 32 / 128, the long horizon."""
    from sttode_amd import scenes
    g = golden(case)
    if case.startswith('eth_N'):
        m = hip_model('eth', 8, 12)
        feed = lambda: m.set_data(None, torch.from_numpy(g['obs']), torch.from_numpy(g['pred']))
        z, check = g['z'], lambda out: assert_close(out, g['out'], what=f'{case}: {what} vs reference')
    elif case == 'sdd_ragged':
        m = hip_model('eth', 8, 12)
        past = np.concatenate([g[f's{i}_obs'].transpose(0, 2, 1) for i in range(4)])
        fut = np.concatenate([g[f's{i}_pred'].transpose(0, 2, 1) for i in range(4)])
        z = np.concatenate([g[f's{i}_z'] for i in range(4)])
        ptr = np.cumsum([0] + [g[f's{i}_obs'].shape[0] for i in range(4)]).astype(np.int32)
        feed = lambda: m.set_scene_batch(past, fut, ptr)

        def check(out):
            for i in range(4):
                assert_close(out[:, ptr[i]:ptr[i + 1]], g[f's{i}_out'], what=f'{case} scene {i}: {what} vs reference')
    else:
        Tp, Tf, N = (10, 40, 10) if case == 'nba_long_B8' else (5, 10, 11)
        m = hip_model('nba', Tp, Tf)
        if case == 'nba_long_B8':
            d, z, st = scenes.nba_batch(8, 8, N=10, obs_len=10, pred_len=40), scenes.latents(4100, 80), 1
        else:
            B = int(case[5:])
            d, z, st = scenes.nba_batch(int(g['nba_seed']), B), scenes.latents(int(g['z_seed']), B * 11), int(g['stride'])
        data = {'past_traj': torch.from_numpy(d['past_traj']), 'future_traj': torch.from_numpy(d['future_traj'])}
        feed = lambda: m.set_data_nba(data)
        check = lambda out: assert_close(out[:, ::st], g['out'], what=f'{case}: {what} vs reference')
    return m, feed, z, check


@pytest.mark.parametrize('case', GOLDEN_INFERENCE_CASES)
def test_exploratory_bf16x3_mode_vs_reference_golden(golden, case):
    """The exploratory mode against the REFERENCE's own vectors (tests/golden/*.npz), at the same rtol 1e-4 + atol 1e-4 as the fp32 path:
    every golden inference case pushed through the fused chain launch (forced: these batches are below the automatic threshold) with the
    three-way bf16 split -- ETH N = 2 / 7 / 32, the four ragged SDD scenes in one batch, NBA B = 4 / 32 / 128, the long horizon."""
    m, feed, z, check = _golden_inference_case(golden, case, 'bf16x3')
    try:
        m.native().set_chain(1)
        m.mfma_mode = 'bf16x3'
        feed()
        out = m.inference(None, z=torch.from_numpy(z)).cpu().numpy()
    finally:
        m.mfma_mode = 'f32'
        m.native().set_chain(-1)
    check(out)


@pytest.mark.parametrize('case', GOLDEN_INFERENCE_CASES)
def test_headline_f32_chain_launch_vs_reference_golden(golden, case):
    """The HEADLINE kernel (the fp32 chain launch that carries `value` in bench.py: traj_chain_kernel, model/STTODE.py:574-623 as one launch
    per call) against the REFERENCE's own vectors at rtol 1e-4 + atol 1e-4: every golden inference case is forced through it (these batches
    sit below the automatic threshold, where the per-scene and three-kernel forms would run) -- once as a serial call and once through the
    pipelined product path (inference_async / wait: the form bench.py times), which must agree with the serial call to fp32 rounding."""
    m, feed, z, check = _golden_inference_case(golden, case, 'f32 chain launch')
    zt = torch.from_numpy(z)
    try:
        m.native().set_chain(1)
        m.reset_async()
        feed()
        out = m.inference(None, z=zt).cpu().numpy()
        hs = []
        for _ in range(3):                                  # three calls in flight, as in the bench; every one must carry the same answer
            feed()
            hs.append(m.inference_async(z=zt))
        outs = [m.wait(h).cpu().numpy() for h in hs]
    finally:
        m.native().set_chain(-1)
        m.reset_async()
    assert np.isfinite(out).all()
    check(out)
    for o in outs:
        check(o)
        assert_close(o, out, rtol=2e-5, atol=2e-5, what=f'{case}: pipelined vs serial chain launch')


@pytest.mark.parametrize('case', ['ucy_256', 'sdd_256', 'nba_128', 'nba_long_64'])
def test_headline_f32_chain_launch_vs_oracle_at_leg_sizes(case):
    """The fp32 chain launch at the per-GPU sizes of bench.py's secondary legs (BASELINE configs 2-5: UCY-mixed 256 scenes, SDD 256 ragged
    scenes, NBA B = 128 x 11, NBA long horizon at obs 10 / pred 40), DIRECTLY against the CPU oracle at rtol 1e-4 + atol 1e-4
    (sampled scenes for the scene batches; the NBA groups are one attention group, so the oracle runs the whole batch -- the long-horizon
    group is compared on a 64-scene attention group of the same shapes, which the oracle finishes in seconds), serial and pipelined."""
    from sttode_amd import scenes
    if case in ('ucy_256', 'sdd_256'):
        m, ora = hip_model('eth', 8, 12), oracle_model('eth', 8, 12)
        sb = scenes.make_scene_batch(range(0, 256), case[:3])
        z = scenes.latents(77, sb.n_agents)
        feed = lambda: m.set_scene_batch(sb.past, sb.future, sb.scene_ptr)
    else:
        Tp, Tf, B, N = (5, 10, 128, 11) if case == 'nba_128' else (10, 40, 64, 10)
        m, ora = hip_model('nba', Tp, Tf), oracle_model('nba', Tp, Tf)
        d = scenes.nba_batch(7000, B, N=N, obs_len=Tp, pred_len=Tf)
        z = scenes.latents(78, B * N)
        data = {'past_traj': torch.from_numpy(d['past_traj']), 'future_traj': torch.from_numpy(d['future_traj'])}
        feed = lambda: m.set_data_nba(data)
    zt = torch.from_numpy(z)
    try:
        m.native().set_chain(1)
        m.reset_async()
        feed()
        out = m.inference(None, z=zt).cpu().numpy()
        feed()
        h = m.inference_async(z=zt)
        outp = m.wait(h).cpu().numpy()
    finally:
        m.native().set_chain(-1)
        m.reset_async()
    assert np.isfinite(out).all() and np.isfinite(outp).all()
    assert_close(outp, out, rtol=2e-5, atol=2e-5, what=f'{case}: pipelined vs serial chain launch')
    if case in ('ucy_256', 'sdd_256'):
        for s in range(0, sb.n_scenes, 19):
            a, b = int(sb.scene_ptr[s]), int(sb.scene_ptr[s + 1])
            obs, pred = sb.scene(s)
            ref = oracle_scene_inference(ora, obs, pred, z[a * 20:b * 20])
            assert_close(out[:, a:b], ref, what=f'{case} scene {s}: f32 chain launch vs oracle')
            assert_close(outp[:, a:b], ref, what=f'{case} scene {s}: pipelined f32 chain launch vs oracle')
    else:
        with torch.no_grad():
            ora.set_data_nba(data)
            ref = ora.inference(data, z=zt).numpy()
        assert_close(out, ref, what=f'{case}: f32 chain launch vs oracle')
        assert_close(outp, ref, what=f'{case}: pipelined f32 chain launch vs oracle')


@pytest.mark.parametrize('case', ['eth_512', 'eth_61', 'sdd', 'nba_128', 'nba_long'])
def test_exploratory_bf16x3_mode_vs_fp32_and_oracle(case):
    """EXPLORATORY opt-in mode (STTODENet.mfma_mode = 'bf16x3', sttode_set_mfma_mode): the two block-0 decoder MLPs of the fused launch as a
    three-way bf16 split on the bf16 matrix cores (six products, fp32 accumulate).  Held to the SAME bar as the fp32 path: the CPU oracle
    at rtol 1e-4 + atol 1e-4 on sampled scenes / the whole NBA batch, and against the fp32 mode of the same launch (agreement far inside
    that bar is expected: the split carries 24 mantissa bits).  Deterministic: two runs give the same bits."""
    from sttode_amd import scenes
    if case in ('eth_512', 'eth_61', 'sdd'):
        m, ora = hip_model('eth', 8, 12), oracle_model('eth', 8, 12)
        sb = scenes.make_scene_batch(range(3000, 3512), 'eth') if case == 'eth_512' else \
            scenes.make_scene_batch(range(3000, 3061), 'eth') if case == 'eth_61' else scenes.make_scene_batch(range(0, 96), 'sdd')
        z = scenes.latents(55, sb.n_agents)
        feed = lambda: m.set_scene_batch(sb.past, sb.future, sb.scene_ptr)
    else:
        Tp, Tf, B, N = (5, 10, 128, 11) if case == 'nba_128' else (10, 40, 48, 10)
        m, ora = hip_model('nba', Tp, Tf), oracle_model('nba', Tp, Tf)
        d = scenes.nba_batch(91, B, N=N, obs_len=Tp, pred_len=Tf)
        z = scenes.latents(56, B * N)
        data = {'past_traj': torch.from_numpy(d['past_traj']), 'future_traj': torch.from_numpy(d['future_traj'])}
        feed = lambda: m.set_data_nba(data)
    outs = {}
    try:
        m.native().set_chain(1)
        for mode in ('f32', 'bf16x3'):
            m.mfma_mode = mode
            feed()
            outs[mode] = m.inference(None, z=torch.from_numpy(z)).cpu().numpy()
            feed()
            assert np.array_equal(m.inference(None, z=torch.from_numpy(z)).cpu().numpy(), outs[mode]), f'{case} {mode}: not deterministic'
    finally:
        m.mfma_mode = 'f32'
        m.native().set_chain(-1)
    assert np.isfinite(outs['bf16x3']).all()
    assert not np.array_equal(outs['bf16x3'], outs['f32'])           # the mode really ran (different summation: not the same bits)
    assert_close(outs['bf16x3'], outs['f32'], rtol=2e-5, atol=2e-5, what=f'{case}: bf16x3 vs fp32 mode')
    if case in ('eth_512', 'eth_61', 'sdd'):
        for s in range(0, sb.n_scenes, 37 if case == 'eth_512' else 11):
            a, b = int(sb.scene_ptr[s]), int(sb.scene_ptr[s + 1])
            obs, pred = sb.scene(s)
            assert_close(outs['bf16x3'][:, a:b], oracle_scene_inference(ora, obs, pred, z[a * 20:b * 20]), what=f'{case} scene {s}: bf16x3 vs oracle')
    else:
        with torch.no_grad():
            ora.set_data_nba(data)
            ref = ora.inference(data, z=torch.from_numpy(z)).numpy()
        assert_close(outs['bf16x3'], ref, what=f'{case}: bf16x3 vs oracle')


def test_fused_launch_gives_up_instead_of_hanging_when_a_producer_never_signals():
    """The exit condition of the in-launch hand-off: with the flag of ONE 16-agent tile withheld (fault injection,
    sttode_debug_drop_role_flag) the trajectory groups that read that tile run into the bound of their spin (~1 s), poison THEIR
    predictions with NaN and set the time-out word; the launch ends, every other group's predictions are the bits of a healthy run, and
    the next healthy launch on the same workspace is clean again."""
    import time
    from sttode_amd import capi, scenes
    m = hip_model('eth', 8, 12)
    sb = scenes.make_scene_batch(range(4000, 4061), 'eth')
    n, S, K = sb.n_agents, sb.n_scenes, 20
    z = torch.from_numpy(scenes.latents(77, n)).to(m.device)
    try:
        m.native().set_chain(1)
        m.set_scene_batch(sb.past, sb.future, sb.scene_ptr)
        good = m.inference(None, z=z).clone()
        tile = 3                                              # agents 48..63
        capi.call('sttode_debug_drop_role_flag', m.native().h, tile)
        m.set_scene_batch(sb.past, sb.future, sb.scene_ptr)
        t0 = time.perf_counter()
        bad = m.inference(None, z=z).clone()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert dt < 30.0, f'the launch took {dt:.1f} s: the spin is not bounded'
        buf, off = m._workspace(n, S)
        ntiles = (n + 15) // 16
        flags = m._view(buf, off, 'flags', ntiles + 1, dtype=torch.int32).cpu().numpy()
        assert flags[ntiles] == 1
        assert flags[tile] == 0 and (np.delete(flags[:ntiles], tile) == 1).all()
        # groups of 128 trajectories (= agents*K): the poisoned ones are exactly those whose agents touch the withheld tile
        a_lo, a_hi = 16 * tile, min(16 * tile + 15, n - 1)
        g_lo, g_hi = (a_lo * K) // 128, (a_hi * K + K - 1) // 128
        flat_bad, flat_good = bad.permute(1, 0, 2, 3).reshape(n * K, -1), good.permute(1, 0, 2, 3).reshape(n * K, -1)
        rows = torch.arange(n * K, device=m.device)
        hit = (rows // 128 >= g_lo) & (rows // 128 <= g_hi)
        assert torch.isnan(flat_bad[hit]).all()
        assert torch.equal(flat_bad[~hit], flat_good[~hit])
    finally:
        capi.call('sttode_debug_drop_role_flag', m.native().h, -1)
        m.native().set_fused(1)
        m.native().set_chain(-1)
    m.native().set_chain(1)
    try:
        m.set_scene_batch(sb.past, sb.future, sb.scene_ptr)
        # round 5: the give-up reaches the drop-in caller -- the call AFTER the poisoned one raises (the model's host-visible time-out word, no
        # synchronisation on the hot path), once; the next healthy launch on the same workspace is clean again
        with pytest.raises(capi.SttodeError, match='gave up'):
            m.inference(None, z=z)
        assert torch.equal(m.inference(None, z=z), good)
    finally:
        m.native().set_chain(-1)


def test_async_pipeline_is_bitwise_identical_to_serial():
    """sttode_inference_scenes_async (two-slot cross-call pipeline) == serial inference(), bit for bit, over several
    back-to-back calls with different batches in flight."""
    from sttode_amd import scenes
    m = hip_model('eth', 8, 12)
    batches = [scenes.make_scene_batch(range(s0, s0 + 40), 'eth') for s0 in (0, 100, 200, 300, 400)]
    zs = [torch.from_numpy(scenes.latents(1000 + i, b.n_agents)).to(m.device) for i, b in enumerate(batches)]
    serial = []
    for b, z in zip(batches, zs):
        m.set_scene_batch(b.past, b.future, b.scene_ptr)
        serial.append(m.inference(None, z=z).clone())
    m.reset_async()
    handles, outs = [], []
    for b, z in zip(batches, zs):
        m.set_scene_batch(b.past, b.future, b.scene_ptr)
        handles.append(m.inference_async(z=z))
        if len(handles) > 1:
            outs.append(m.wait(handles.pop(0)).clone())
    outs.append(m.wait(handles.pop(0)).clone())
    torch.cuda.synchronize()
    for i, (a, b) in enumerate(zip(serial, outs)):
        assert torch.equal(a, b), f'batch {i}: async != serial'
    m.reset_async()


def test_forward_loss_values_vs_reference_golden(golden):
    """forward() objective values (posterior encoder, K=1 decode with recover_traj, K=20 decode,
    four losses) against the reference's own forward() with injected noise."""
    g = golden('eth_forward_losses')
    m = hip_model('eth', 8, 12)
    m.set_data(None, torch.from_numpy(g['obs']), torch.from_numpy(g['pred']))
    for grad_path in (False, True):        # fused inference kernels (no_grad) and the training kernels (autograd) give the same values
        with torch.set_grad_enabled(grad_path):
            tot, lp, lr, lk, ld = m.forward(eps_q=torch.from_numpy(g['eps_q']), eps_p=torch.from_numpy(g['eps_p1']),
                                            eps20=torch.from_numpy(g['eps_p20']))
        assert tot.requires_grad == grad_path
        assert_close(m.qz_param.cpu().numpy(), g['qz_param'], what='qz_param')
        assert_close(m.pred_traj.cpu().numpy(), g['pred_traj'], what='pred_traj')
        assert_close(m.recover_traj.cpu().numpy(), g['recover_traj'], what='recover_traj')
        assert_close(m.diverse_pred_traj.cpu().numpy(), g['diverse_pred_traj'], what='diverse_pred_traj')
        np.testing.assert_allclose([float(tot.detach()), lp, lr, lk, ld], g['losses'], rtol=1e-4)


def test_nba_single_scene_batch_vs_oracle():
    """NBA branch with B = 1 (attention length 1 inside the NBA code path) and an odd agent count."""
    from sttode_amd import scenes
    m = hip_model('nba', 5, 10)
    ora = oracle_model('nba', 5, 10)
    for B, N in ((1, 11), (3, 7)):
        d = scenes.nba_batch(50 + B, B, N=N)
        z = scenes.latents(60 + B, B * N)
        data = {'past_traj': torch.from_numpy(d['past_traj']), 'future_traj': torch.from_numpy(d['future_traj'])}
        m.set_data_nba(data)
        out = m.inference(data, z=torch.from_numpy(z)).cpu().numpy()
        with torch.no_grad():
            ora.set_data_nba(data)
            ref = ora.inference(data, z=torch.from_numpy(z)).numpy()
        assert_close(out, ref, what=f'nba B={B} N={N}')


def test_random_latents_follow_torch_generator():
    """z=None draws from torch's global generator like Normal.rsample (model/STTODE.py:89-93): seeding reproduces the call."""
    from sttode_amd import scenes
    m = hip_model('eth', 8, 12)
    obs, pred = scenes.eth_scene(77, n_min=5, n_max=5)
    m.set_data(None, torch.from_numpy(obs), torch.from_numpy(pred))
    torch.manual_seed(3)
    a = m.inference(None).clone()
    torch.manual_seed(3)
    b = m.inference(None).clone()
    c = m.inference(None)
    assert torch.equal(a, b) and not torch.equal(a, c)
    assert tuple(a.shape) == (20, 5, 12, 2) and bool(torch.isfinite(a).all())


@pytest.mark.parametrize('case', ['one_agent', 'two_agents', 'eth_scene', 'tile_edge_16', 'tile_edge_17', 'three_scenes', 'sdd_like_40', 'k_7',
                                  'long_16_24', 'short_4_6', 'twenty_small_scenes'])
def test_one_launch_scene_form_is_bitwise_the_six_launch_form(case):
    """A serial scene call below the chain threshold -- the reference's evaluation loop hands over ONE scene per call (test.py:171-188) --
    runs as ONE launch whose workgroups take the roles front-end + per-agent stage / block-0 decoder_y / block-0 decoder_x -> block-1 GRU
    -> block-1 decoder_y (csrc/scene_lat.hip).  Its bodies are the six launches' code and sum every element in the same order, so the
    predictions must be the SAME BITS as the six-launch form (which the golden-vector and oracle tests pin), not merely close; and the
    oracle comparison of the result itself at 1e-4."""
    from sttode_amd import scenes
    Tp, Tf, K = 8, 12, 20
    if case == 'one_agent':
        ids = None
    elif case == 'two_agents':
        ids = [s for s in range(6000, 6400) if scenes.eth_scene(s)[0].shape[0] == 2][:1] or [6001]
    elif case == 'eth_scene':
        ids = [6002]
    elif case in ('tile_edge_16', 'tile_edge_17', 'sdd_like_40'):
        ids = None
    elif case == 'three_scenes':
        ids = [6003, 6004, 6005]
    else:
        ids = [6006, 6007]
    if case == 'k_7':
        K = 7
    if case == 'long_16_24':
        Tp, Tf = 16, 24
    if case == 'short_4_6':
        Tp, Tf = 4, 6
    m = hip_model('eth', Tp, Tf)
    if K != 20:
        from sttode_amd import STTODENet
        a7 = make_args('eth', Tp, Tf)
        a7.sample_k = K
        m7 = STTODENet(a7, _gpu()).eval()
        m7.load_state_dict(m.state_dict(), strict=True)
        m = m7
    if case == 'twenty_small_scenes':   # 20 scenes of 1-4 agents each (61 agents): every 16-agent tile spans several scenes, the roles' scene search runs deep
        parts, ptr = [], [0]
        for i, sid in enumerate(range(6300, 6320)):
            o, p_ = scenes.eth_scene(sid)
            k = 1 + (i * 7) % 4
            parts.append((o[:k].transpose(0, 2, 1), p_[:k].transpose(0, 2, 1)))
            ptr.append(ptr[-1] + k)
        past = np.ascontiguousarray(np.concatenate([a for a, _ in parts]))
        fut = np.ascontiguousarray(np.concatenate([b for _, b in parts]))
        ptr = np.asarray(ptr, dtype=np.int32)
        ids, sb = 'built', None
    if ids is None:     # scenes accumulated until the agent count is exactly the wanted one (the last scene is cut): tile edges
        want = {'one_agent': 1, 'tile_edge_16': 16, 'tile_edge_17': 17, 'sdd_like_40': 40}[case]
        sb = scenes.make_scene_batch(range(6100, 6140), 'eth', Tp, Tf)
        ptr = [int(p) for p in sb.scene_ptr if int(p) < want] + [want]
        past, fut, ptr = sb.past[:want], sb.future[:want], np.asarray(ptr, dtype=np.int32)
    elif ids != 'built':
        sb = scenes.make_scene_batch(ids, 'eth', Tp, Tf)
        past, fut, ptr = sb.past, sb.future, sb.scene_ptr
    n = past.shape[0]
    z = torch.from_numpy(scenes.latents(31, n, K=K)).to(m.device) if K != 20 else torch.from_numpy(scenes.latents(31, n)).to(m.device)
    nat = m.native()
    outs = {}
    try:
        for mode in (0, -1, 0, -1):
            nat.set_scene_launch(mode)
            m.set_scene_batch(past, fut, ptr)
            outs.setdefault(mode, []).append(m.inference(None, z=z).clone())
    finally:
        nat.set_scene_launch(-1)
    assert torch.equal(outs[-1][0], outs[-1][1]), 'one-launch form is not reproducible run to run'
    assert torch.equal(outs[0][0], outs[0][1])
    assert bool(torch.isfinite(outs[-1][0]).all())
    if Tp <= 8:
        assert torch.equal(outs[-1][0], outs[0][0]), f'one-launch form differs from the six launches: max |d| = {(outs[-1][0] - outs[0][0]).abs().max().item():.3e}'
    else:   # Tp > 8: the six-launch form takes the STREAMING conv + GRU (gru32, another summation order); the one-launch form the 16-column one
        assert_close(outs[-1][0].cpu().numpy(), outs[0][0].cpu().numpy(), rtol=2e-5, atol=2e-5, what=f'{case}: one-launch vs six-launch form')
    buf, off = m._workspace(n, len(ptr) - 1)
    A = (n + 15) // 16
    C = (n * K + 15) // 16
    # the scene form's flag words (behind the fused launch's region, api_util.hpp stt_scene_flags_offset): E [A] | time-out | G [A] | E2 [A] |
    # Y [C] | exit counter | initialised word.  The launch's last workgroup has zeroed them again -- no memset per launch, replayable --
    # nobody timed out, and the workspace carries the mark sttode_workspace_init left
    flags = m._view(buf, off, 'flags', 5 * A + 4 + 3 * A + 1 + C + 2, dtype=torch.int32).cpu().numpy().view(np.uint32)[5 * A + 4:]
    assert (flags[:-1] == 0).all() and flags[-1] == 0x5774F1A6, 'flag words not back to zero after the launch / workspace not marked initialised'
    if case in ('eth_scene', 'three_scenes'):      # and against the CPU oracle, scene by scene (reference call pattern)
        ora = oracle_model('eth', 8, 12)
        out = outs[-1][0].cpu().numpy()
        zz = z.cpu().numpy()
        for si in range(sb.n_scenes):
            a, b = int(sb.scene_ptr[si]), int(sb.scene_ptr[si + 1])
            obs, pred = sb.scene(si)
            assert_close(out[:, a:b], oracle_scene_inference(ora, obs, pred, zz[a * 20:b * 20]), what=f'{case} scene {si}: one-launch form vs oracle')


def test_one_launch_scene_form_gives_up_instead_of_hanging():
    """Fault injection on the one-launch scene form: the per-agent role of tile 1 never publishes; the trajectory tiles that read agents
    16.. poison their predictions with NaN and set the time-out word, the others carry the bits of a healthy run, the launch ends."""
    import time
    from sttode_amd import capi, scenes
    m = hip_model('eth', 8, 12)
    sb = scenes.make_scene_batch(range(6200, 6204), 'eth')
    n, K = sb.n_agents, 20
    assert 20 < n <= 100, n                                   # two or more agent tiles, and few enough trajectory tiles for the one-launch form
    z = torch.from_numpy(scenes.latents(5, n)).to(m.device)
    m.set_scene_batch(sb.past, sb.future, sb.scene_ptr)
    good = m.inference(None, z=z).clone()
    try:
        capi.call('sttode_debug_drop_role_flag', m.native().h, 1)
        m.set_scene_batch(sb.past, sb.future, sb.scene_ptr)
        t0 = time.perf_counter()
        bad = m.inference(None, z=z).clone()
        torch.cuda.synchronize()
        assert time.perf_counter() - t0 < 30.0
    finally:
        capi.call('sttode_debug_drop_role_flag', m.native().h, -1)
    # STTODENet.inference() surfaces it: the call after the dropped flag raises (host load of the model's time-out word), the one after is clean
    m.set_scene_batch(sb.past, sb.future, sb.scene_ptr)
    with pytest.raises(capi.SttodeError, match='gave up'):
        m.inference(None, z=z)
    assert torch.equal(m.inference(None, z=z), good)
    flat_bad, flat_good = bad.permute(1, 0, 2, 3).reshape(n * K, -1), good.permute(1, 0, 2, 3).reshape(n * K, -1)
    rows = torch.arange(n * K, device=m.device)
    t_lo, t_hi = rows // 16 * 16, torch.clamp(rows // 16 * 16 + 15, max=n * K - 1)
    hit = ((t_hi // K) // 16 >= 1) & ((t_lo // K) // 16 <= 1)       # the tile's agent range touches agent tile 1
    assert bool(hit.any()) and bool((~hit).any())
    assert torch.isnan(flat_bad[hit]).all()
    assert torch.equal(flat_bad[~hit], flat_good[~hit])
    m.set_scene_batch(sb.past, sb.future, sb.scene_ptr)
    assert torch.equal(m.inference(None, z=z), good)


@pytest.mark.parametrize('lagged', [0, 2, 3])
def test_async_best_of_k_on_the_calls_stream_matches_the_kernel_on_the_callers_stream(lagged):
    """(lagged = 0: the round-3 pipelined form, bitwise the serial calls; 2 / 3: the default lagged form -- the metrics of a call whose
    trajectory groups nobody has enqueued yet trigger that launch themselves -- fp32 rounding of the serial calls.)
    best_of_k_async: the metrics of a pipelined call enqueued on the call's own pipeline stream (behind its launch, in stream order) are
    the bits of best_of_k on the waited predictions; the slot's completion event covers them, so a slot reused four calls later never sees
    its metric buffers or its ground truth overwritten early (ten calls through four slots, three batches of one shape in rotation)."""
    from sttode_amd import scenes
    m = hip_model('eth', 8, 12)
    batches = []
    for v in range(3):
        sb = scenes.make_scene_batch(range(7000, 7064), 'eth')
        past = torch.from_numpy((sb.past * (1.0 + 0.05 * v)).astype(np.float32)).to(m.device)
        fut = torch.from_numpy((sb.future * (1.0 + 0.05 * v)).astype(np.float32)).to(m.device)
        batches.append((past, fut, torch.from_numpy(sb.scene_ptr).to(m.device), torch.from_numpy(scenes.latents(40 + v, sb.n_agents)).to(m.device)))
    ref = []
    for past, fut, ptr, z in batches:
        m.set_scene_batch(past, fut, ptr)
        out = m.inference(None, z=z)
        a, f = m.best_of_k(out.permute(1, 0, 2, 3), gt=fut)
        ref.append((a.clone(), f.clone()))
    m.native().set_lagged(lagged)
    m.reset_async()
    pend, got = [], []
    for i in range(10):
        v = (2 * i + i // 3) % 3
        past, fut, ptr, z = batches[v]
        m.set_scene_batch(past, fut, ptr)
        h = m.inference_async(z=z)
        pend.append((v, h, fut))
        if len(pend) >= 4:
            vv, hh, ff = pend.pop(0)
            a, f = m.best_of_k_async(hh, gt=ff)
            m.wait(hh)
            got.append((vv, a.clone(), f.clone()))
    while pend:
        vv, hh, ff = pend.pop(0)
        a, f = m.best_of_k_async(hh)                          # default ground truth: the futures set with the batch
        m.wait(hh)
        got.append((vv, a.clone(), f.clone()))
    torch.cuda.synchronize()
    assert len(got) == 10
    for i, (vv, a, f) in enumerate(got):
        if lagged == 0:
            assert torch.equal(a, ref[vv][0]) and torch.equal(f, ref[vv][1]), f'call {i} (batch {vv}): metrics on the call\'s stream differ'
        else:
            assert_close(a.cpu().numpy(), ref[vv][0].cpu().numpy(), rtol=2e-5, atol=2e-5, what=f'call {i} (batch {vv}): ADE')
            assert_close(f.cpu().numpy(), ref[vv][1].cpu().numpy(), rtol=2e-5, atol=2e-5, what=f'call {i} (batch {vv}): FDE')
    with pytest.raises(ValueError):
        m.best_of_k_async(h, gt=np.zeros((3, 12, 2), np.float32))
    m.reset_async()
    m.native().set_lagged(3)


@pytest.mark.parametrize('lagged', [0, 2, 3])
def test_pipelined_calls_prepared_on_their_own_pipeline_stream_match_serial(lagged):
    """(lagged = 0: the round-3 pipelined form, three streams, bitwise; 2 / 3: the default lagged form on that many streams, fp32 rounding.)
    next_async_stream: the H2D copy of a call's inputs, its latents and the call itself all enqueued on the pipeline stream the call
    will run on (no cross-stream event anywhere), metrics on that stream too -- nine calls over the three streams, depth 3 -- give the
    predictions and best-of-K values of the serial calls, bit for bit, with latents from the same generator sequence."""
    from sttode_amd import scenes
    m = hip_model('eth', 8, 12)
    old_depth = m.async_depth
    host = []
    for v in range(3):
        sb = scenes.make_scene_batch(range(7200 + 70 * v, 7270 + 70 * v), 'eth')
        host.append((torch.from_numpy(sb.past).pin_memory(), torch.from_numpy(sb.future).pin_memory(), torch.from_numpy(sb.scene_ptr).to(m.device)))
    try:
        m.native().set_chain(1)
        torch.manual_seed(21)
        ref = []
        for i in range(9):
            past, fut, ptr = host[i % 3]
            m.set_scene_batch(past.to(m.device), fut.to(m.device), ptr)
            out = m.inference(None)
            a, f = m.best_of_k(out.permute(1, 0, 2, 3))
            ref.append((out.clone(), a.clone(), f.clone()))
        m.native().set_lagged(lagged)
        m.reset_async()
        m.async_depth = 3 if lagged == 0 else 2 * lagged
        m.device_latents = False                                  # the serial calls' torch.randn sequence (device latents: their own test)
        torch.manual_seed(21)
        pend, got = [], []
        for i in range(9):
            past, fut, ptr = host[i % 3]
            if len(pend) >= 3:
                h = pend.pop(0)
                got.append((h, m.best_of_k_async(h)))             # on the stream of call i-3 == the stream of call i, ahead of it
            st = m.next_async_stream(past.shape[0])
            assert st is not None
            with torch.cuda.stream(st):
                m.set_scene_batch(past.to(m.device, non_blocking=True), fut.to(m.device, non_blocking=True), ptr)
                pend.append(m.inference_async())
        while pend:
            h = pend.pop(0)
            got.append((h, m.best_of_k_async(h)))
        for h, _ in got:
            m.wait(h)
        torch.cuda.synchronize()
        # slots are reused every third call: only the last three calls' buffers still hold their own results
        for i in (6, 7, 8):
            h, (a, f) = got[i]
            if lagged == 0:
                assert torch.equal(h['pred'].permute(1, 0, 2, 3), ref[i][0]), f'call {i}: predictions differ'
                assert torch.equal(a, ref[i][1]) and torch.equal(f, ref[i][2]), f'call {i}: metrics differ'
            else:
                assert_close(h['pred'].permute(1, 0, 2, 3).cpu().numpy(), ref[i][0].cpu().numpy(), rtol=2e-5, atol=2e-5, what=f'call {i}: predictions')
                assert_close(a.cpu().numpy(), ref[i][1].cpu().numpy(), rtol=2e-5, atol=2e-5, what=f'call {i}: ADE')
    finally:
        m.async_depth = old_depth
        m.device_latents = True
        m.native().set_chain(-1)
        m.reset_async()
        m.native().set_lagged(3)


@pytest.mark.parametrize('case', ['eth_61', 'eth_512', 'eth_long', 'sdd_96', 'nba_128', 'nba_long'])
def test_lagged_launch_vs_serial_forms_and_oracle(case):
    """Round 4, the default pipelined form: a call's launch = its per-agent stage in THROUGHPUT form (csrc/role32.hpp: 128 agents per
    workgroup on 32-column MFMA tiles, host-folded embedding; PastEncoder.forward model/STTODE.py:214-236, block 0 of Decoder.forward
    :320-347) + the trajectory groups of the call made `streams` calls earlier.  Against the serial form (latency-form roles, 16-column
    tiles, unfolded embedding) on the same inputs: predictions AND the per-agent intermediates the roles write (pf, state0, the three
    layer-1 tables) to fp32 rounding; against the CPU oracle at rtol 1e-4 + atol 1e-4.  Calls with DIFFERENT inputs share the rotation
    (slots reused, 2 and 3 streams); the launch order is exercised three ways: later calls carry the groups, wait() right after the call
    (the groups become a launch of their own), metrics first.  The same call gives the same bits every time."""
    from sttode_amd import scenes
    variants = []
    if not case.startswith('nba'):
        Tp, Tf = (10, 40) if case == 'eth_long' else (8, 12)
        m, ora = hip_model('eth', Tp, Tf), oracle_model('eth', Tp, Tf)
        if case == 'sdd_96':
            sb = scenes.make_scene_batch(range(0, 96), 'sdd')
        else:
            nsc = {'eth_61': 61, 'eth_512': 512, 'eth_long': 40}[case]
            sb = scenes.make_scene_batch(range(2000, 2000 + nsc), 'eth', obs_len=Tp, pred_len=Tf)
        n, S = sb.n_agents, sb.n_scenes
        for v in range(3):
            past = (sb.past * (1.0 + 0.03 * v) + 0.1 * v).astype(np.float32)
            variants.append(((torch.from_numpy(past).to(m.device), torch.from_numpy(sb.future).to(m.device),
                              torch.from_numpy(sb.scene_ptr).to(m.device)), torch.from_numpy(scenes.latents(300 + v, n)).to(m.device)))
        feed = lambda inp: m.set_scene_batch(*inp)
    else:
        Tp, Tf, B, N = (5, 10, 128, 11) if case == 'nba_128' else (10, 40, 24, 10)
        m, ora = hip_model('nba', Tp, Tf), oracle_model('nba', Tp, Tf)
        n, S = B * N, 0
        for v in range(3):
            d = scenes.nba_batch(60 + v, B, N=N, obs_len=Tp, pred_len=Tf)
            variants.append(({'past_traj': torch.from_numpy(d['past_traj']).to(m.device), 'future_traj': torch.from_numpy(d['future_traj']).to(m.device)},
                             torch.from_numpy(scenes.latents(300 + v, n)).to(m.device)))
        feed = lambda inp: m.set_data_nba(inp)
    names = (('pf', 128), ('state0', 96), ('A0x', 512), ('A0y', 512), ('A1y', 512))
    fe_names = (('xpad', 16 * (1 if 2 * Tp <= 16 else 2)), ('enc_in', 4 * Tp), ('cur', 2), ('orig', 2))   # set_data's outputs (scene batches: written by the roles)
    nat = m.native()
    try:
        nat.set_chain(1)
        ref = []
        for inp, z in variants:                              # serial form: one launch with latency-form roles
            feed(inp)
            out = m.inference(None, z=z).clone()
            buf, off = m._workspace(n, S)
            inter = {k: m._view(buf, off, k, n, w).clone() for k, w in names + fe_names}
            if S:
                inter['scene_orig'] = m._view(buf, off, 'scene_orig', S, 2).clone()
            ref.append((out, inter))
        first = {}
        for streams in (2, 3):
            nat.set_lagged(streams)
            m.reset_async()
            m.async_depth = 2 * streams
            order = [0, 1, 2, 2, 0, 1, 1, 0, 2, 0, 1]
            pend, outs = [], []
            for i, v in enumerate(order):
                inp, z = variants[v]
                feed(inp)
                h = m.inference_async(z=z)
                pend.append((v, h))
                if i == 3:                                   # wait right behind the call: nobody else has enqueued its groups
                    vv, hh = pend.pop()
                    outs.append((vv, hh, m.wait(hh).clone()))
                elif len(pend) > streams:                    # steady state: the groups came with a later call's launch
                    vv, hh = pend.pop(0)
                    if i % 2:
                        m.best_of_k_async(hh)
                    outs.append((vv, hh, m.wait(hh).clone()))
            while pend:
                vv, hh = pend.pop(0)
                outs.append((vv, hh, m.wait(hh).clone()))
            torch.cuda.synchronize()
            assert len(outs) == len(order)
            for vv, hh, o in outs:
                assert torch.isfinite(o).all()
                assert_close(o.cpu().numpy(), ref[vv][0].cpu().numpy(), rtol=2e-5, atol=2e-5, what=f'{case} {streams} streams variant {vv}: lagged vs serial form')
                if vv in first:
                    assert torch.equal(o, first[vv]), f'{case} {streams} streams variant {vv}: the lagged form is not deterministic'
                first.setdefault(vv, o)
            # the per-agent intermediates of the last call of every slot still in its workspace
            seen = set()
            for vv, hh, o in reversed(outs):
                if hh['slot'] in seen:
                    continue
                seen.add(hh['slot'])
                buf = m._async_bufs[(n, S, hh['slot'])][0]
                off, _ = nat.layout(n, S)
                for k, w in names:
                    got = m._view(buf, off, k, n, w).cpu().numpy()
                    want = ref[vv][1][k].cpu().numpy()
                    # pf's second half is the x12-amplified FFN output: two correct fp32 evaluations differ by a few 1e-5 there
                    assert_close(got, want, rtol=5e-5, atol=5e-5, what=f'{case} {streams} streams variant {vv}: {k}')
                for k, w in fe_names + ((('scene_orig', 2),) if S else ()):   # same arithmetic in the same order as the front-end kernels: same bits
                    got = m._view(buf, off, k, S if k == 'scene_orig' else n, w)
                    assert torch.equal(got, ref[vv][1][k]), f'{case} {streams} streams variant {vv}: front-end output {k} differs'
        # the oracle, directly
        inp, z = variants[0]
        got = first[0].cpu().numpy()
        if not case.startswith('nba'):
            zn = z.cpu().numpy()
            for s in range(0, S, max(1, S // 6)):
                a, b = int(sb.scene_ptr[s]), int(sb.scene_ptr[s + 1])
                obs = np.ascontiguousarray(inp[0][a:b].cpu().numpy().transpose(0, 2, 1))
                pred = np.ascontiguousarray(inp[1][a:b].cpu().numpy().transpose(0, 2, 1))
                assert_close(got[:, a:b], oracle_scene_inference(ora, obs, pred, zn[a * 20:b * 20]), what=f'{case} scene {s}: lagged form vs oracle')
        else:
            data = {k: v.cpu() for k, v in inp.items()}
            with torch.no_grad():
                ora.set_data_nba(data)
                want = ora.inference(data, z=z.cpu()).numpy()
            assert_close(got, want, what=f'{case}: lagged form vs oracle')
    finally:
        nat.set_chain(-1)
        m.reset_async()
        nat.set_lagged(3)
        m.async_depth = 6


@pytest.mark.parametrize('case', ['eth_61', 'eth_odd_Tf', 'nba', 'nba_long'])
def test_fused_metrics_of_the_lagged_form_are_bitwise_best_of_k(case):
    """inference_async(metrics_gt=...) in the lagged form: the call's trajectory groups compute its min-over-K ADE / FDE themselves
    (compute_ADE / compute_FDE, utils/metrics.py:7-26): per column the displacement norms summed in best_of_k_kernel's order, then an
    atomic minimum on the float bits per agent.  Against best_of_k on the call's own predictions: the same bits (agents that straddle two
    128-trajectory groups and two waves included), for Tf = 12, an odd Tf (2 Tf not a multiple of 4: the element-wise epilogue), the NBA
    shapes and the long horizon; with a scale factor; slots reused with different batches; against the NumPy oracle of the metric."""
    from oracle.metrics_ref import best_of_k_ade_fde
    from sttode_amd import scenes
    batches = []
    if case.startswith('eth'):
        Tp, Tf = (8, 11) if case == 'eth_odd_Tf' else (8, 12)
        m = hip_model('eth', Tp, Tf)
        for v in range(3):
            sb = scenes.make_scene_batch(range(8300 + 70 * v, 8361 + 70 * v), 'eth', obs_len=Tp, pred_len=Tf)
            batches.append(('scenes', (torch.from_numpy(sb.past).to(m.device), torch.from_numpy(sb.future).to(m.device), torch.from_numpy(sb.scene_ptr).to(m.device))))
    else:
        Tp, Tf, B, N = (5, 10, 64, 11) if case == 'nba' else (10, 40, 16, 10)
        m = hip_model('nba', Tp, Tf)
        for v in range(3):
            d = scenes.nba_batch(80 + v, B, N=N, obs_len=Tp, pred_len=Tf)
            batches.append(('nba', {'past_traj': torch.from_numpy(d['past_traj']).to(m.device), 'future_traj': torch.from_numpy(d['future_traj']).to(m.device)}))
    nat = m.native()
    try:
        nat.set_chain(1)
        m.reset_async()
        pend, got = [], []
        for i in range(9):
            kind, inp = batches[(2 * i + i // 4) % 3]
            if kind == 'scenes':
                m.set_scene_batch(*inp)
            else:
                m.set_data_nba(inp)
            scale = 1.0 if i % 3 else 2.5
            h = m.inference_async(metrics_gt=m._future, metrics_scale=scale)
            assert h['fused_metrics'] is not None
            pend.append((h, m._future, scale))
            if len(pend) > 2:
                hh, fut, sc = pend.pop(0)
                a, f = m.best_of_k_async(hh, scale=sc)            # no kernel: the groups' own values
                pred = m.wait(hh)
                got.append((a.clone(), f.clone(), pred.clone(), fut, sc))
        while pend:
            hh, fut, sc = pend.pop(0)
            a, f = m.best_of_k_async(hh, scale=sc)
            pred = m.wait(hh)
            got.append((a.clone(), f.clone(), pred.clone(), fut, sc))
        torch.cuda.synchronize()
        assert len(got) == 9
        for i, (a, f, pred, fut, sc) in enumerate(got):
            ra, rf = m.best_of_k(pred.permute(1, 0, 2, 3), gt=fut, scale=sc)
            assert torch.isfinite(a).all() and torch.isfinite(f).all()
            assert torch.equal(a, ra) and torch.equal(f, rf), f'{case} call {i}: fused metrics differ from best_of_k on the same predictions'
            oa, of = best_of_k_ade_fde(pred.permute(1, 0, 2, 3).cpu().numpy() * sc, fut.cpu().numpy() * sc)
            assert_close(a.cpu().numpy(), oa, rtol=1e-5, atol=1e-5, what=f'{case} call {i}: ADE vs the NumPy oracle')
            assert_close(f.cpu().numpy(), of, rtol=1e-5, atol=1e-5, what=f'{case} call {i}: FDE vs the NumPy oracle')
    finally:
        nat.set_chain(-1)
        m.reset_async()


def _philox_normals(key, first4, count4):

    """NumPy restatement of csrc/role32.hpp latents32: Philox4x32-10 (key = 64 bits, counter = float4 index) + two Box-Muller pairs per
    block -> float32 [count4 * 4]."""
    g4 = np.arange(first4, first4 + count4, dtype=np.uint64)
    c = [(g4 & np.uint64(0xffffffff)).astype(np.uint64), (g4 >> np.uint64(32)).astype(np.uint64), np.zeros(count4, np.uint64), np.zeros(count4, np.uint64)]
    k0, k1 = np.uint64(key & 0xffffffff), np.uint64((key >> 32) & 0xffffffff)
    M = np.uint64(0xffffffff)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        n0, n2 = ((p1 >> np.uint64(32)) ^ c[1] ^ k0) & M, ((p0 >> np.uint64(32)) ^ c[3] ^ k1) & M
        c = [n0, p1 & M, n2, p0 & M]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M, (k1 + np.uint64(0xBB67AE85)) & M
    out = np.empty((count4, 4), np.float32)
    for p in range(2):
        u1 = (c[2 * p] >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24) + np.float32(2.0 ** -25)
        u2 = (c[2 * p + 1] >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24) + np.float32(2.0 ** -25)
        rad = np.sqrt(np.float32(-2.0) * np.log(u1.astype(np.float64))).astype(np.float32)
        ang = np.float32(6.283185307179586) * u2
        out[:, 2 * p], out[:, 2 * p + 1] = rad * np.cos(ang.astype(np.float64)), rad * np.sin(ang.astype(np.float64))
    return out.reshape(-1)


def test_device_latents_of_the_lagged_form():
    """inference_async(z=None) in the lagged form: the call's own launch draws z ~ N(0, I) (Philox4x32-10 keyed from torch's generator,
    csrc/role32.hpp latents32; Normal.rsample, model/STTODE.py:89-93,609-616).  The latents are (a) the values of the NumPy restatement of
    the generator for the key torch's generator hands out, (b) standard normal by their moments, different from call to call, the same
    under the same torch seed; (c) exactly what the trajectory groups consumed: the serial form fed the SAME latents gives the call's
    predictions; (d) switched off (device_latents = False) the call draws torch.randn like the serial form."""
    from sttode_amd import scenes
    m = hip_model('eth', 8, 12)
    sb = scenes.make_scene_batch(range(8100, 8161), 'eth')
    n = sb.n_agents
    feed = lambda: m.set_scene_batch(sb.past, sb.future, sb.scene_ptr)
    nat = m.native()
    try:
        nat.set_chain(1)
        m.reset_async()
        runs = []
        for rep in range(2):
            torch.manual_seed(5)
            key = int(torch.empty((), dtype=torch.int64).random_()) & 0x7fffffffffffffff      # what inference_async will draw first
            torch.manual_seed(5)
            hs = []
            for _ in range(3):
                feed()
                hs.append(m.inference_async())
            outs = [(m.wait(h).clone(), h['z'].clone()) for h in hs]
            runs.append((key, outs))
        torch.cuda.synchronize()
        key, outs = runs[0]
        z0 = outs[0][1].cpu().numpy()
        assert z0.shape == (n * 20, 32)
        want = _philox_normals(key, 0, n * 20 * 8).reshape(n * 20, 32)
        assert_close(z0, want, rtol=1e-4, atol=1e-4, what='device latents vs the NumPy restatement of the generator')
        allz = np.concatenate([o[1].cpu().numpy().reshape(-1) for o in outs]).astype(np.float64)
        assert abs(allz.mean()) < 5e-3 and abs(allz.std() - 1.0) < 5e-3 and abs((allz ** 4).mean() - 3.0) < 0.05 and np.abs(allz).max() < 7.0
        assert not torch.equal(outs[0][1], outs[1][1]) and not torch.equal(outs[1][1], outs[2][1])
        for i in range(3):
            assert torch.equal(runs[0][1][i][1], runs[1][1][i][1]) and torch.equal(runs[0][1][i][0], runs[1][1][i][0]), 'same torch seed, different latents'
            feed()
            ser = m.inference(None, z=outs[i][1])
            assert_close(outs[i][0].cpu().numpy(), ser.cpu().numpy(), rtol=2e-5, atol=2e-5, what=f'call {i}: groups consumed other latents than the call reports')
        m.device_latents = False
        torch.manual_seed(9)
        feed()
        h = m.inference_async()
        m.wait(h)
        torch.manual_seed(9)
        assert torch.equal(h['z'], torch.randn(n * 20, 32, device=m.device))
    finally:
        m.device_latents = True
        nat.set_chain(-1)
        m.reset_async()


def test_lagged_form_with_mixed_batch_shapes_and_small_calls_in_between():
    """Robustness of the lagged rotation: consecutive pipelined calls of DIFFERENT shapes (two chain-sized scene batches with different
    agent counts: a call's trajectory groups ride in the launch of another shape's call) with calls BELOW the chain threshold in between
    (they take the round-3 unfused form on the same pipeline streams), a weight change in the middle (re-packed weights, new native
    model: outstanding groups are flushed first), all against serial calls."""
    from sttode_amd import scenes
    m = hip_model('eth', 8, 12)
    big = [scenes.make_scene_batch(range(9000, 9060), 'eth'), scenes.make_scene_batch(range(9100, 9175), 'eth')]   # ~20 k and ~26 k trajectories
    small = scenes.make_scene_batch(range(9200, 9212), 'eth')
    batches = [big[0], big[1], small, big[1], big[0], big[0], small, big[1]]
    zs = [torch.from_numpy(scenes.latents(500 + i, b.n_agents)).to(m.device) for i, b in enumerate(batches)]

    def serial_all():
        outs = []
        for b, z in zip(batches, zs):
            m.set_scene_batch(b.past, b.future, b.scene_ptr)
            outs.append(m.inference(None, z=z).clone())
        return outs
    try:
        ref = serial_all()
        m.reset_async()
        hs, outs = [], []
        for b, z in zip(batches, zs):
            m.set_scene_batch(b.past, b.future, b.scene_ptr)
            hs.append(m.inference_async(z=z))
            if len(hs) > 4:                                   # (at most async_depth = 6 calls may be in flight: a slot's buffers are reused)
                outs.append(m.wait(hs.pop(0)).clone())
        outs += [m.wait(h).clone() for h in hs]
        torch.cuda.synchronize()
        for i, (o, r) in enumerate(zip(outs, ref)):
            assert_close(o.cpu().numpy(), r.cpu().numpy(), rtol=2e-5, atol=2e-5, what=f'mixed shapes, call {i}')
        # weight change with calls in flight: the next packed() builds a new native model
        sd = {k: v.clone() for k, v in m.state_dict().items()}
        m.set_scene_batch(big[0].past, big[0].future, big[0].scene_ptr)
        h_old = m.inference_async(z=zs[0])
        with torch.no_grad():
            m.decoder.decompose[1].decoder_y.layers[2].bias.add_(0.25)
        m.set_scene_batch(big[0].past, big[0].future, big[0].scene_ptr)
        h_new = m.inference_async(z=zs[0])
        o_new = m.wait(h_new).clone()
        m.set_scene_batch(big[0].past, big[0].future, big[0].scene_ptr)
        s_new = m.inference(None, z=zs[0])
        assert_close(o_new.cpu().numpy(), s_new.cpu().numpy(), rtol=2e-5, atol=2e-5, what='call after a weight change')
        assert float((o_new - ref[0]).abs().max()) > 0.1      # the new bias really is in the result
    finally:
        m.load_state_dict(sd, strict=True) if 'sd' in dir() else None
        m.reset_async()


def test_zero_copy_futures_of_the_lagged_form():
    """inference_async(pred_host=True): the trajectory groups of a lagged call write the futures straight to PINNED HOST memory (the kernel
    only writes `pred`: block 0's y_hat0 waits in the workspace), what test.py:186-188 does with a .cpu() per call -- the same bits as the
    device-buffer call, fused metrics included, slots reused; refused for calls that do not take the lagged form."""
    from sttode_amd import capi, scenes
    m = hip_model('eth', 8, 12)
    sb = scenes.make_scene_batch(range(8600, 8661), 'eth')
    z = torch.from_numpy(scenes.latents(77, sb.n_agents)).to(m.device)
    fut = torch.from_numpy(sb.future).to(m.device)
    nat = m.native()
    try:
        nat.set_chain(1)
        m.reset_async()
        outs = {}
        for host in (False, True):
            hs = []
            for _ in range(7):                                    # more calls than slots
                m.set_scene_batch(sb.past, sb.future, sb.scene_ptr)
                h = m.inference_async(z=z, metrics_gt=m._future, pred_host=host)
                hs.append(h)
                if len(hs) > 3:
                    hh = hs.pop(0)
                    a, f = m.best_of_k_async(hh)
                    p = m.wait_host(hh) if host else m.wait(hh)
                    torch.cuda.synchronize()
                    outs.setdefault(host, []).append((torch.as_tensor(p).cpu().clone(), a.clone(), f.clone()))
            for hh in hs:
                a, f = m.best_of_k_async(hh)
                p = m.wait_host(hh) if host else m.wait(hh)
                torch.cuda.synchronize()
                outs[host].append((torch.as_tensor(p).cpu().clone(), a.clone(), f.clone()))
            assert (hs[-1]['pred'].is_pinned() and not hs[-1]['pred'].is_cuda) == host
        assert len(outs[True]) == len(outs[False]) == 7
        for (ph, ah, fh), (pd, ad, fd) in zip(outs[True], outs[False]):
            assert torch.isfinite(ph).all()
            assert torch.equal(ph, pd) and torch.equal(ah, ad) and torch.equal(fh, fd), 'futures written to pinned host memory differ from the device-buffer call'
        small = scenes.make_scene_batch(range(8700, 8704), 'eth')
        nat.set_chain(-1)
        m.set_scene_batch(small.past, small.future, small.scene_ptr)
        with pytest.raises(capi.SttodeError):
            m.inference_async(pred_host=True)
    finally:
        nat.set_chain(-1)
        m.reset_async()


def test_check_reports_a_given_up_hand_off():
    """sttode_check: the host-visible error path of the in-launch hand-off forms (round-3 fused launch): after a launch in which a group
    gave up waiting for its producer (fault injection) the check fails loudly; after a healthy launch it passes."""
    from sttode_amd import capi, scenes
    m = hip_model('eth', 8, 12)
    sb = scenes.make_scene_batch(range(4000, 4061), 'eth')
    z = torch.from_numpy(scenes.latents(9, sb.n_agents)).to(m.device)
    nat = m.native()
    try:
        nat.set_chain(1)
        m.set_scene_batch(sb.past, sb.future, sb.scene_ptr)
        m.inference(None, z=z)
        buf, _ = m._workspace(sb.n_agents, sb.n_scenes)
        nat.check(buf, sb.n_agents, sb.n_scenes)
        capi.call('sttode_debug_drop_role_flag', nat.h, 3)
        m.set_scene_batch(sb.past, sb.future, sb.scene_ptr)
        m.inference(None, z=z)
        with pytest.raises(capi.SttodeError):
            nat.check(buf, sb.n_agents, sb.n_scenes)
        assert nat.timeout_word.value == 1                       # ... and the model's host-visible word (read without any synchronisation)
        with pytest.raises(capi.SttodeError, match='gave up'):
            nat.raise_if_timed_out()
        assert nat.timeout_word.value == 0                       # reported once
    finally:
        capi.call('sttode_debug_drop_role_flag', nat.h, -1)
        nat.set_chain(-1)
    m.set_scene_batch(sb.past, sb.future, sb.scene_ptr)
    m.inference(None, z=z)


def test_async_latents_follow_the_same_generator_sequence_as_serial_calls():
    """inference_async(z=None) draws its latents from torch's generator at call time, like inference(None): the same seed gives the same
    predictions call by call, whether the calls are pipelined or serial."""
    from sttode_amd import scenes
    m = hip_model('eth', 8, 12)
    sb = scenes.make_scene_batch(range(5000, 5012), 'eth')
    feed = lambda: m.set_scene_batch(sb.past, sb.future, sb.scene_ptr)
    torch.manual_seed(11)
    serial = []
    for _ in range(4):
        feed()
        serial.append(m.inference(None).clone())
    torch.manual_seed(11)
    m.reset_async()
    hs = []
    for _ in range(4):
        feed()
        hs.append(m.inference_async())
    outs = [m.wait(h).clone() for h in hs]
    torch.cuda.synchronize()
    for i in range(4):
        assert torch.equal(outs[i], serial[i]), f'call {i}: async latents differ from the serial sequence'
    assert not torch.equal(outs[0], outs[1])
    m.reset_async()


def test_nba_group_spanning_two_ranks_matches_single_rank():
    """one attention group sharded over ranks, with an all-gather of q|k|v.  Two ranks are simulated in one
    process (the gather is injected); every rank's slice must equal the single-rank result."""
    from sttode_amd import scenes
    m = hip_model('nba', 5, 10)
    B, N, split = 24, 11, 10
    d = scenes.nba_batch(321, B, N=N)
    z = torch.from_numpy(scenes.latents(322, B * N)).to(m.device)
    full_data = {'past_traj': torch.from_numpy(d['past_traj']), 'future_traj': torch.from_numpy(d['future_traj'])}
    m.set_data_nba(full_data)
    full = m.inference(full_data, z=z).clone()
    qkv_full = m._view(*m._workspace(B * N, 0), 'qkv', B * N, 192).clone()
    parts = [(0, split), (split, B)]
    for (b0, b1) in parts:
        loc = {'past_traj': torch.from_numpy(d['past_traj'][b0:b1]), 'future_traj': torch.from_numpy(d['future_traj'][b0:b1])}
        out = m.inference_nba_sharded(loc, z=z[b0 * N * 20:b1 * N * 20], gather=lambda q: qkv_full)
        assert_close(out.cpu().numpy(), full[:, b0 * N:b1 * N].cpu().numpy(), rtol=1e-6, atol=1e-6, what=f'rank slice {b0}:{b1}')


def _chunked_oracle_mhgsa(query, key, value, num_heads, in_w, in_b, out_w, out_b, slots=2):
    """oracle.sttode_ref.mhgsa evaluated a few batch slots at a time: attention never mixes batch slots (dim 1), and at L = 4096 the
    un-chunked score tensor [Nb*H, S, L] is 5.4 GB in fp32.  Same function, same arithmetic; returns (out, None)."""
    import oracle.sttode_ref as R
    outs = []
    for b0 in range(0, query.shape[1], slots):
        sl = slice(b0, b0 + slots)
        outs.append(R._mhgsa_unchunked(query[:, sl], key[:, sl], value[:, sl], num_heads, in_w, in_b, out_w, out_b)[0])
    return torch.cat(outs, dim=1), None


def test_attention_at_config5_length_vs_oracle(monkeypatch):
    """BASELINE config 5 read literally: ONE attention group of 4096 scenes x 10 agents (obs 10 / pred 40).  The flash-style column
    tiling of mhgsa_attn (32 tiles of 128 columns, 4096-term un-normalised softmax sums, the acos polynomial) is compared with the
    CPU oracle at that length: (1) the stand-alone op; (2) the NBA branch of inference(): past_feature of all 40 960 agents against
    the oracle encoder, and the predictions of a sample of agents against the oracle decoder fed with the oracle's own
    past_feature; (3) the same group split over two simulated ranks (all-gather of q|k|v injected) equals the single-rank call."""
    import oracle.sttode_ref as R
    from sttode_amd import scenes
    from sttode_amd.ops import mhgsa
    dev = _gpu()
    if not hasattr(R, '_mhgsa_unchunked'):
        R._mhgsa_unchunked = R.mhgsa
    monkeypatch.setattr(R, 'mhgsa', _chunked_oracle_mhgsa)
    torch.set_num_threads(min(16, torch.get_num_threads()))
    L, N, Tp, Tf = 4096, 10, 10, 40
    m, ora = hip_model('nba', Tp, Tf), oracle_model('nba', Tp, Tf)
    # (1) op level, self-attention L = S = 4096 (the untransposed-score quirk applies)
    att = ora.past_encoder.ODE_Encoder.odeblock.odefunc.layers[0].self_attn.temporal_attention_before
    W = [att.in_proj_weight.detach(), att.in_proj_bias.detach(), att.out_proj.weight.detach(), att.out_proj.bias.detach()]
    x = torch.from_numpy(np.random.default_rng(4096).standard_normal((L, N, 64)).astype(np.float32))
    o, _ = mhgsa(x.to(dev), x.to(dev), x.to(dev), *[w.to(dev) for w in W])
    with torch.no_grad():
        ref, _ = _chunked_oracle_mhgsa(x, x, x, 8, *W)
    assert_close(o.cpu().numpy(), ref.numpy(), what='mhgsa self-attention L=4096')
    # (2) inference(), NBA branch
    d = scenes.nba_batch(4096, L, N=N, obs_len=Tp, pred_len=Tf)
    z = scenes.latents(4097, L * N)
    data = {'past_traj': torch.from_numpy(d['past_traj']), 'future_traj': torch.from_numpy(d['future_traj'])}
    m.set_data_nba(data)
    out = m.inference(data, z=torch.from_numpy(z))
    pf = m.past_feature.cpu().numpy()
    with torch.no_grad():
        past = data['past_traj'].reshape(L * N, Tp, 2)
        inputs = torch.cat((past, R.first_diff_dup(past)), dim=-1)
        pf_ref = ora.past_encoder(inputs, L, N)
        err = np.abs(pf - pf_ref.numpy())
        if (err > ATOL + RTOL * np.abs(pf_ref.numpy())).any():
            # The encoder output is 12 x the layer output (one Euler step of size 12) on values up to ~60, and every row of the layer
            # is a 4096-term softmax sum: two fp32 evaluations differ by a few 1e-4 on a handful of the 5.2 M entries.  Yardstick:
            # the same encoder in FLOAT64 (same oracle code, .double()); HIP must be no further from it than twice the fp32 oracle is.
            import copy
            enc64 = copy.deepcopy(ora.past_encoder).double()
            t64 = enc64(inputs.double(), L, N).numpy()
            e_hip = (np.abs(pf - t64) / (1.0 + np.abs(t64))).max()
            e_ref = (np.abs(pf_ref.numpy() - t64) / (1.0 + np.abs(t64))).max()
            assert e_hip <= max(2 * e_ref, 1e-4), f'past_feature at L=4096: HIP {e_hip:.3e} vs float64, fp32 oracle {e_ref:.3e}'
        idx = np.sort(np.random.default_rng(7).choice(L * N, 96, replace=False))
        ti = torch.from_numpy(idx)
        zs = torch.from_numpy(z).view(L * N, 20, 32)[ti].reshape(-1, 32)
        dec, _ = ora.decoder(pf_ref[ti].repeat_interleave(20, dim=0), zs, past[ti], past[ti][:, -1:], sample_num=20, mode='inference')
    assert_close(out[:, ti.to(dev)].cpu().numpy(), dec.permute(1, 0, 2, 3).numpy(), what='inference() at L=4096, sampled agents')
    # (3) two simulated ranks: 1500 + 2596 scenes
    qkv_full = m._view(*m._workspace(L * N, 0), 'qkv', L * N, 192).clone()
    full = out.clone()
    zt = torch.from_numpy(z).to(dev)
    for b0, b1 in ((0, 1500), (1500, L)):
        loc = {'past_traj': data['past_traj'][b0:b1], 'future_traj': data['future_traj'][b0:b1]}
        part = m.inference_nba_sharded(loc, z=zt[b0 * N * 20:b1 * N * 20], gather=lambda q: qkv_full)
        assert_close(part.cpu().numpy(), full[:, b0 * N:b1 * N].cpu().numpy(), rtol=2e-5, atol=2e-5, what=f'rank slice {b0}:{b1} of the 4096 group')


def _two_process_worker(rank, world, port, q):
    """One of two processes sharing cuda:0; collectives over gloo (host copies), compute on the GPU through the C ABI."""
    import os
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY='0')
    dist.init_process_group('gloo', rank=rank, world_size=world)
    from sttode_amd import parallel, scenes
    m = hip_model('nba', 5, 10)
    B, N, split = 24, 11, 10
    d = scenes.nba_batch(321, B, N=N)
    z = torch.from_numpy(scenes.latents(322, B * N)).to(m.device)
    b0, b1 = (0, split) if rank == 0 else (split, B)
    loc = {'past_traj': torch.from_numpy(d['past_traj'][b0:b1]), 'future_traj': torch.from_numpy(d['future_traj'][b0:b1])}
    part = m.inference_nba_sharded(loc, z=z[b0 * N * 20:b1 * N * 20])           # gather=None: the real parallel.gather_futures
    allp = parallel.gather_futures(part.permute(1, 0, 2, 3).contiguous())         # [B*N, K, Tf, 2] in rank order
    # ETH path: scenes sharded over the two processes through parallel.infer_sharded
    me = hip_model('eth', 8, 12)
    me.native().set_chain(0)        # one form of the per-trajectory stage on every shard size, so the comparison below can be bitwise
    sb = scenes.make_scene_batch(range(700, 745), 'eth')
    ze = scenes.latents(71, sb.n_agents)
    pe, metrics = parallel.infer_sharded(me, sb, rank, world, z=ze)
    if rank == 0:
        q.put((allp.cpu().numpy(), pe.cpu().numpy(), metrics))
    dist.barrier()
    dist.destroy_process_group()


def test_two_processes_real_collectives_match_single_process():
    """The non-injected multi-rank code paths: inference_nba_sharded's all-gather of q|k|v through parallel.gather_futures, the
    gather of the futures, and parallel.infer_sharded (scene sharding + gather + metric all-reduce), run by TWO processes (both on
    cuda:0, gloo collectives over host copies -- RCCL itself needs two GPUs) and compared with the single-process results."""
    import os
    import torch.multiprocessing as mp
    from sttode_amd import scenes
    _gpu()
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = 35500 + os.getpid() % 2000
    procs = [ctx.Process(target=_two_process_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    allp, pe, (ade, fde, cnt) = q.get(timeout=300)
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    m = hip_model('nba', 5, 10)
    d = scenes.nba_batch(321, 24, N=11)
    data = {'past_traj': torch.from_numpy(d['past_traj']), 'future_traj': torch.from_numpy(d['future_traj'])}
    m.set_data_nba(data)
    full = m.inference(data, z=torch.from_numpy(scenes.latents(322, 24 * 11))).permute(1, 0, 2, 3).cpu().numpy()
    assert_close(allp, full, rtol=1e-6, atol=1e-6, what='two-process NBA group vs single process')
    me = hip_model('eth', 8, 12)
    sb = scenes.make_scene_batch(range(700, 745), 'eth')
    me.set_scene_batch(sb.past, sb.future, sb.scene_ptr)
    me.native().set_chain(0)
    try:
        ref = me.inference(None, z=torch.from_numpy(scenes.latents(71, sb.n_agents)))
    finally:
        me.native().set_chain(-1)
    assert np.array_equal(pe, ref.cpu().numpy())                 # scene independence: bitwise
    a, f = me.best_of_k(ref.permute(1, 0, 2, 3))
    assert cnt == sb.n_agents and abs(ade - float(a.double().mean())) < 1e-5 and abs(fde - float(f.double().mean())) < 1e-5


def _rccl_worker(rank, world, port, q):
    """One rank per GPU, backend nccl (= RCCL over xGMI): the scene-sharded hot path with the REAL collectives of parallel.py."""
    import os
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY='0')
    torch.cuda.set_device(rank)
    dist.init_process_group('nccl', rank=rank, world_size=world, device_id=torch.device('cuda', rank))
    from sttode_amd import STTODENet, parallel, scenes
    from sttode_amd.weights import make_weights, to_torch_state_dict
    me = STTODENet(make_args('eth', 8, 12), torch.device('cuda', rank)).eval()
    me.load_state_dict(to_torch_state_dict(make_weights(1234)), strict=True)
    me.native().set_chain(0)        # one form of the per-trajectory stage on every shard size, so the comparison can be bitwise
    sb = scenes.make_scene_batch(range(700, 745), 'eth')
    ze = scenes.latents(71, sb.n_agents)
    pe, metrics = parallel.infer_sharded(me, sb, rank, world, z=ze)            # gather_futures + reduce_metrics under RCCL
    rows = parallel.gather_futures(torch.full((rank + 2, 3), float(rank), device=me.device))   # ragged row counts
    if rank == 0:
        q.put((pe.cpu().numpy(), metrics, rows.cpu().numpy()))
    dist.barrier()
    dist.destroy_process_group()


def test_rccl_gather_futures_and_reduce_metrics_on_two_gpus():
    """parallel.gather_futures (padded variable-size all-gather of the futures) and parallel.reduce_metrics (3-scalar all-reduce) on
    backend nccl = RCCL with two fresh child processes, one per GPU (the reference's only distributed code: core/utils.py:370-389; its
    metric path wants the futures on one rank: test.py:194,526), against the single-process result.  Needs two visible GPUs: skipped
    on the one-GPU box, run by whoever has a node."""
    import os
    import torch.multiprocessing as mp
    from sttode_amd import scenes
    if torch.cuda.device_count() < 2:
        pytest.skip('needs two GPUs (RCCL with one rank per GPU)')
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = 37500 + os.getpid() % 2000
    procs = [ctx.Process(target=_rccl_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    pe, (ade, fde, cnt), rows = q.get(timeout=300)
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    me = hip_model('eth', 8, 12)
    sb = scenes.make_scene_batch(range(700, 745), 'eth')
    me.set_scene_batch(sb.past, sb.future, sb.scene_ptr)
    me.native().set_chain(0)
    try:
        ref = me.inference(None, z=torch.from_numpy(scenes.latents(71, sb.n_agents)))
    finally:
        me.native().set_chain(-1)
    assert np.array_equal(pe, ref.cpu().numpy())                 # scene independence: bitwise, whichever GPU ran the scene
    a, f = me.best_of_k(ref.permute(1, 0, 2, 3))
    assert cnt == sb.n_agents and abs(ade - float(a.double().mean())) < 1e-5 and abs(fde - float(f.double().mean())) < 1e-5
    assert rows.shape == (5, 3) and np.array_equal(rows[:, 0], [0, 0, 1, 1, 1])


def test_stale_training_tape_is_refused(golden):
    """Eager training steps keep ONE tape per model (the most recent forward()).  backward() of an older loss, or a second backward()
    of the same loss, must raise instead of differentiating the wrong step (round-1 advisor finding)."""
    import os
    from sttode_amd import STTODENet, capi
    from sttode_amd.weights import make_weights, to_torch_state_dict
    g = golden('eth_forward_losses')
    try:
        m = STTODENet(make_args('eth', 8, 12), _gpu()).train()
        m.load_state_dict(to_torch_state_dict(make_weights(1234)), strict=True)
        m.rand_rot_scene = False
        m.train_graphs = False                     # eager steps (the hipGraph replay path keeps its gradients per call)
        m.set_data(None, torch.from_numpy(g['obs']), torch.from_numpy(g['pred']))
        first = m.forward()[0]
        second = m.forward()[0]
        with pytest.raises(capi.SttodeError, match='earlier forward'):
            first.backward()
        second.backward()
        assert all(p.grad is not None for p in m.decoder.parameters())
        with pytest.raises((capi.SttodeError, RuntimeError)):
            second.backward()
    finally:
        pass


def test_graph_replayed_step_refuses_a_second_backward_and_follows_replaced_parameters(golden):
    """Round-2 advisor findings on the hipGraph training path: (1) a second backward() of a graph-replayed step raises like the eager
    step's consumed tape does, instead of silently doubling .grad; (2) the cached (names, parameters) list is validated on every call:
    after a Parameter object is replaced the step computes with -- and hands its gradient to -- the live object, not the stale one
    (the hipGraph key changes with the parameters' storage)."""
    from sttode_amd import STTODENet, capi
    from sttode_amd.weights import make_weights, to_torch_state_dict
    g = golden('eth_forward_losses')
    m = STTODENet(make_args('eth', 8, 12), _gpu()).train()
    m.load_state_dict(to_torch_state_dict(make_weights(1234)), strict=True)
    m.rand_rot_scene = False
    eps = [torch.from_numpy(np.random.default_rng(5).standard_normal(s).astype(np.float32)) for s in ((g['obs'].shape[0], 32),) * 2 + ((g['obs'].shape[0] * 20, 32),)]
    dp = torch.ones(g['obs'].shape[0] * 8, 64, device=m.device)
    df = torch.ones(g['obs'].shape[0] * 12, 64, device=m.device)

    def step():
        m.set_data(None, torch.from_numpy(g['obs']), torch.from_numpy(g['pred']))
        return m.forward(eps[0], eps[1], eps[2], dp, df)[0]
    step().backward()                             # eager (first step of the shape)
    m.zero_grad()
    step().backward()                             # captured
    m.zero_grad()
    loss = step()                                 # replayed
    loss.backward()
    g1 = m.decoder.decompose[0].decoder_y.layers[2].weight.grad.clone()
    with pytest.raises((capi.SttodeError, RuntimeError)):
        loss.backward()
    assert torch.equal(m.decoder.decompose[0].decoder_y.layers[2].weight.grad, g1)      # not doubled
    # replace a Parameter object (same values): the next steps must hand the gradient to the NEW object
    lin = m.decoder.decompose[0].decoder_y.layers[2]
    old = lin.weight
    lin.weight = torch.nn.Parameter(old.detach().clone())
    m.zero_grad()
    old.grad = None
    for _ in range(3):                            # eager -> capture -> replay on the new key
        m.zero_grad()
        step().backward()
    assert lin.weight.grad is not None and old.grad is None
    assert torch.allclose(lin.weight.grad, g1, rtol=1e-5, atol=1e-6 * float(g1.abs().max()))


def test_evaluation_loops_vs_oracle_metrics(tmp_path):
    """test.py-style evaluation on top of the batched HIP path: ETH/UCY CSV dataset and NBA loader, checked against the
    CPU oracle run scene by scene / batch by batch with the same latents and the NumPy metric restatement."""
    from oracle.metrics_ref import best_of_k_ade_fde, nba_horizon_errors
    from sttode_amd import scenes
    from sttode_amd.datasets import NBADataset, TrajectoryDataset, seq_collate
    from sttode_amd.evaluate import eval_nba, eval_scenes
    rng = np.random.default_rng(4)
    # --- ETH/UCY-like CSV: 30 frames, 6 pedestrians present throughout
    rows = []
    for p in range(6):
        start, vel = rng.uniform(0, 10, 2), rng.normal(0, 0.3, 2)
        for t in range(30):
            x, y = start + vel * t + rng.normal(0, 0.02, 2)
            rows.append((10 * t, p + 1, x, y))
    rows.sort()
    np.savetxt(tmp_path / 'a.csv', np.asarray(rows).T, delimiter=',', fmt='%.6f')
    ds = TrajectoryDataset(str(tmp_path), obs_len=8, pred_len=12, skip=3, min_ped=1, files=['a.csv'])
    m = hip_model('eth', 8, 12)
    zall = scenes.latents(8, ds.obs_traj.shape[0])
    ade, fde, n = eval_scenes(m, ds, traj_scale=1.0, z_fn=lambda rows_: torch.from_numpy(zall[:rows_]))
    ora = oracle_model('eth', 8, 12)
    a_ref, f_ref = [], []
    for i in range(len(ds)):
        s, e = ds.seq_start_end[i]
        out = oracle_scene_inference(ora, ds.obs_traj[s:e].numpy(), ds.pred_traj[s:e].numpy(), zall[s * 20:e * 20])
        a, f = best_of_k_ade_fde(out.transpose(1, 0, 2, 3), ds.pred_traj[s:e].permute(0, 2, 1).numpy())
        a_ref.append(a); f_ref.append(f)
    assert n == ds.obs_traj.shape[0]
    assert abs(ade - np.concatenate(a_ref).mean()) < 1e-4 and abs(fde - np.concatenate(f_ref).mean()) < 1e-4
    # --- NBA loader, two batches of 3 scenes
    np.save(tmp_path / 'test.npy', rng.uniform(10, 80, (6, 15, 11, 2)))
    nds = NBADataset(obs_len=5, pred_len=10, training=False, data_root=str(tmp_path / 'test.npy'))
    batches = [seq_collate([nds[i] for i in range(b, b + 3)]) for b in (0, 3)]
    mn = hip_model('nba', 5, 10)
    zn = scenes.latents(9, 33)
    res = eval_nba(mn, batches, traj_scale=1.0, z_fn=lambda rows_: torch.from_numpy(zn[:rows_]))
    on = oracle_model('nba', 5, 10)
    acc = np.zeros((10, 2))
    for data in batches:
        with torch.no_grad():
            on.set_data_nba(data)
            out = on.inference(data, z=torch.from_numpy(zn)).numpy()
        e = nba_horizon_errors(out, data['future_traj'].reshape(33, 10, 2).numpy(), range(1, 11))
        acc += np.array([e[h] for h in range(1, 11)]) * 3
    acc /= 6
    for h in range(1, 11):
        assert abs(res[h][0] - acc[h - 1, 0]) < 1e-4 and abs(res[h][1] - acc[h - 1, 1]) < 1e-4


@pytest.mark.parametrize('kind,nsc', [('ucy', 48), ('sdd', 96)])
def test_other_baseline_configs_vs_oracle(kind, nsc):
    """BASELINE configs[2] (UCY-mixed: zara 2-20 / univ 20-60 pedestrians) and configs[3] (SDD: ragged, 1..40 agents,
    pixel coordinates / 50): batched HIP call vs the CPU oracle scene by scene."""
    from sttode_amd import scenes
    m = hip_model('eth', 8, 12)
    ora = oracle_model('eth', 8, 12)
    sb = scenes.make_scene_batch(range(nsc), kind)
    z = scenes.latents(500 + nsc, sb.n_agents)
    m.set_scene_batch(sb.past, sb.future, sb.scene_ptr)
    out = m.inference(None, z=torch.from_numpy(z)).cpu().numpy()
    sizes = np.diff(sb.scene_ptr)
    assert sizes.min() >= 1 and (sizes.max() > 32 if kind == 'ucy' else sizes.max() <= 40)
    for s in list(range(0, nsc, 7)) + [int(np.argmax(sizes)), int(np.argmin(sizes))]:
        a, b = int(sb.scene_ptr[s]), int(sb.scene_ptr[s + 1])
        obs, pred = sb.scene(s)
        ref = oracle_scene_inference(ora, obs, pred, z[a * 20:b * 20])
        assert_close(out[:, a:b], ref, what=f'{kind} scene {s} (N={b - a})')


def test_repeated_runs_are_bitwise_identical():
    """Race screen: the LDS-DMA / barrier protocol of the streaming kernels must give the same bits on every run."""
    from sttode_amd import scenes
    m = hip_model('eth', 8, 12)
    sb = scenes.make_scene_batch(range(300, 812), 'eth')
    z = torch.from_numpy(scenes.latents(77, sb.n_agents)).to(m.device)
    m.set_scene_batch(sb.past, sb.future, sb.scene_ptr)
    ref = m.inference(None, z=z).clone()
    for _ in range(6):
        assert torch.equal(m.inference(None, z=z), ref)


def test_linear_cols_tanh_and_long_k():
    """Q-net shapes of the stage-2 sampler: tanh epilogue (utils/mlp.py:26-29) and the K = 640 contraction of q_c (sampler.py:26)."""
    from sttode_amd.ops import linear_cols
    dev = _gpu()
    rng = np.random.default_rng(3)
    for ncols, K, N, act in ((11, 64, 512, 'tanh'), (70, 512, 256, 'tanh'), (66, 640, 32, None), (9, 256, 640, None)):
        W = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
        b = rng.standard_normal(N).astype(np.float32)
        X = rng.standard_normal((ncols, K)).astype(np.float32)
        out = linear_cols(torch.from_numpy(X).to(dev), torch.from_numpy(W).to(dev), torch.from_numpy(b).to(dev), act=act)
        ref = X.astype(np.float64) @ W.T.astype(np.float64) + b
        assert_close(out.cpu().numpy(), np.tanh(ref) if act else ref, rtol=1e-5, atol=2e-5, what=f'linear_cols {act} {ncols}x{K}->{N}')


@pytest.mark.parametrize('tag,dataset,Tp,Tf,modes', SAMPLER_CASES)
def test_sampler_vs_reference_golden(golden, tag, dataset, Tp, Tf, modes):
    """Stage-2 Sampler.forward + compute_sampler_loss (sampler.py:32-70, samplerloss.py:41-73) on the HIP path."""
    from sttode_amd import Sampler, samplerloss
    from sttode_amd.weights import make_sampler_weights, to_torch_state_dict
    dev = _gpu()
    g = golden('sampler')
    net = hip_model(dataset, Tp, Tf)
    smp = Sampler(sampler_args(dataset, Tp, Tf))
    smp.load_state_dict(to_torch_state_dict(make_sampler_weights()), strict=True)
    with pytest.raises(Exception):
        smp.forward(net)                    # still on CPU: must refuse, not fall back
    smp.set_device(dev)
    inp, fut = sampler_case_inputs(g, tag, dataset)
    for mode in modes:
        smp.share_eps = mode != 'peragent'
        if dataset == 'eth':
            n = inp['obs'].shape[0]
            net.set_data(None, torch.from_numpy(inp['obs']), torch.from_numpy(inp['pred']), torch.ones(n, Tp), torch.ones(n, Tf))
        else:
            net.set_data_nba({k: (torch.from_numpy(v) if isinstance(v, np.ndarray) else v) for k, v in inp['data'].items()})
        k = f'{tag}_{mode}_'
        with torch.no_grad():                                   # value path (fused inference kernels); the autograd path is
            dec, sd, vd, aw = smp.forward(net, mean=(mode == 'mean'), eps=torch.from_numpy(g[k + 'eps']))   # tested below
        assert_close(dec.cpu().numpy(), g[k + 'dec'], what=k + 'dec')
        assert_close(sd.mu.cpu().numpy(), g[k + 'mu'], what=k + 'mu')
        # logvar = log(A^2 + 1e-8) is ill-conditioned where A ~ 0; sigma = exp(logvar / 2) ~ |A| is what KL and rsample consume
        assert_close(sd.sigma.cpu().numpy(), np.exp(0.5 * g[k + 'logvar']), what=k + 'sigma')
        assert_close(aw.cpu().numpy(), g[k + 'pred_traj'], what=k + 'pred_traj')
        futd = torch.from_numpy(fut).to(dev)
        if dataset == 'nba':
            tot, ld, _ = samplerloss.compute_sampler_loss_nba(smp.args, futd, dec.reshape(-1, 20, Tf, 2), 1, vd, sd, {'weight': 1, 'scale': 1.0})
        else:
            tot, ld, _ = samplerloss.compute_sampler_loss(smp.args, futd, dec, 1, torch.ones(n, Tf), vd, sd, {'weight': 1, 'scale': 1})
        got = np.array([float(tot), float(ld['kld']), float(ld['diverse'])])
        np.testing.assert_allclose(got, g[k + 'loss'], rtol=1e-4)
        # and against the CPU oracle on the same inputs
        odec, omu, _, _, oloss = oracle_sampler_case(g, tag, dataset, Tp, Tf, mode)
        assert_close(dec.cpu().numpy(), odec, what=k + 'dec vs oracle')
        np.testing.assert_allclose(got, oloss, rtol=1e-4)


def test_sampler_loss_kernel_general_prior_and_scales():
    """sttode_sampler_loss with a non-standard prior and the per-dataset diversity scales (trainsampler.py:102-116) vs torch fp64."""
    from sttode_amd import samplerloss
    from sttode_amd.dist import Normal
    dev = _gpu()
    rng = np.random.default_rng(12)
    n, K, nz, Tf = 19, 20, 32, 12
    t = lambda a: torch.from_numpy(a.astype(np.float32)).to(dev)
    q = Normal(mu=t(rng.standard_normal((n * K, nz))), logvar=t(0.5 * rng.standard_normal((n * K, nz))))
    p = Normal(mu=t(0.3 * rng.standard_normal((n * K, nz))), logvar=t(0.3 * rng.standard_normal((n * K, nz))))
    motion = t(0.6 * rng.standard_normal((n, K, Tf, 2)))
    for ds in ('sdd', 'eth', 'univ', 'other'):
        cfg = samplerloss.get_diversity_config(ds)
        kld, div = samplerloss._per_agent(q, p, motion, cfg['scale'])
        qm, ql, pm, pl, mo = (x.double().cpu() for x in (q.mu, q.logvar, p.mu, p.logvar, motion))
        ps = torch.exp(0.5 * pl) + 1e-8
        t1, t2 = (qm - pm) / ps, torch.exp(0.5 * ql) / ps
        ref_k = (0.5 * (t1 * t1 + t2 * t2) - 0.5 - torch.log(t2)).view(n, -1).sum(1)
        ref_d = torch.stack([(-(torch.nn.functional.pdist(m.reshape(K, -1)) ** 2) / cfg['scale']).exp().mean() for m in mo])
        assert_close(kld.cpu().numpy(), ref_k.numpy(), rtol=1e-5, atol=1e-4, what='kld ' + ds)
        assert_close(div.cpu().numpy(), ref_d.numpy(), rtol=1e-4, atol=1e-6, what='div ' + ds)


def _twgrad_generic_split_case(capi, dev, rng, scratch, st, cols, N, K):
    """The one case in which the GENERIC weight gradient still splits its columns (sttode_twgrad's reduction launch; 3001 columns: 188
    chunks of 16, 6 splits): an abandoned group's split gradient keeps the whole deferral buffer reserved, nothing is pending or queued
    that a flush could free, and the next gradient finds no room there and splits over the call's scratch."""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
    S = ((cols + 15) // 16 + 31) // 32
    per = N * (K + 1)
    assert cols > 1024 and S > 1 and S * per < scratch.numel()
    dY, Xw = rng.standard_normal((cols, N)).astype(np.float32), rng.standard_normal((cols, K + 5)).astype(np.float32)
    gW0, gb0 = rng.standard_normal((N, K)).astype(np.float32), rng.standard_normal(N).astype(np.float32)
    X = t(Xw)[:, :K]
    buf = torch.zeros(2 * per, device=dev)
    gWa, gba, gW, gb = t(gW0), t(gb0), t(gW0), t(gb0)
    scratch.zero_()
    try:
        capi.call('sttode_twgrad_defer', 1, buf, buf.numel())
        capi.call('sttode_tgemm_group', 1)
        capi.call('sttode_twgrad', t(dY), N, X, X.stride(0), 1, gWa, K, gba, cols, N, K, scratch, scratch.numel(), st)   # queued, 2 splits reserved
        capi.call('sttode_tgemm_group', -1)
        capi.call('sttode_twgrad', t(dY), N, X, X.stride(0), 1, gW, K, gb, cols, N, K, scratch, scratch.numel(), st)
        capi.call('sttode_twgrad_defer', 0, None, 0)
        torch.cuda.synchronize()
    finally:
        capi.call('sttode_tgemm_group', -1)
        capi.call('sttode_twgrad_defer', -1, None, 0)
    assert (buf == 0).all() and (scratch[(S - 1) * per:S * per] != 0).any() and (scratch[S * per:] == 0).all(), \
        f'not the generic kernel with {S} column splits in the call\'s scratch'
    assert np.array_equal(gWa.cpu().numpy(), gW0) and np.array_equal(gba.cpu().numpy(), gb0), 'the abandoned gradient ran'
    tol = 1e-5 * max(1.0, np.sqrt(cols))
    assert_close(gW.cpu().numpy(), dY.astype(np.float64).T @ Xw[:, :K].astype(np.float64) + gW0, rtol=1e-5, atol=tol,
                 what='twgrad dW, generic kernel with split columns')
    assert_close(gb.cpu().numpy(), dY.astype(np.float64).sum(0) + gb0, rtol=1e-5, atol=tol, what='twgrad db, generic kernel with split columns')


def test_tlinear_and_twgrad_vs_torch():
    """Generic training kernels: forward / input-gradient / weight-gradient of nn.Linear at the model's awkward shapes
    (K = 4, 67; N = 24; ragged columns; broadcast rows; strided views; relu mask; accumulation; >1 column split)."""
    from sttode_amd import capi
    dev = _gpu()
    rng = np.random.default_rng(21)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
    scratch = torch.empty(1 << 20, device=dev)
    st = capi.stream_ptr()
    # (more than 2048 columns: the LDS-tiled kernel of round 4 -- ragged tiles in every dimension, k not a multiple of 32, unaligned rows,
    # broadcast rows, outputs narrower than a tile, the NBA step's shapes)
    for cols, J, I, xdiv, act in ((37, 67, 64, 1, 0), (7, 4, 64, 1, 0), (640, 256, 512, 20, 1), (33, 512, 24, 1, 0), (5000, 96, 288, 1, 3),
                                  (19, 1024, 64, 1, 2), (7392, 256, 512, 21, 1), (7392, 512, 256, 1, 1), (7040, 256, 20, 1, 0), (1100, 67, 70, 1, 2),
                                  (36960, 32, 288, 1, 0), (2049, 131, 33, 3, 3), (3001, 67, 70, 1, 2)):
        rows = (cols + xdiv - 1) // xdiv
        Xw = rng.standard_normal((rows, J + 5)).astype(np.float32)          # strided view: ld = J + 5 (unaligned unless J+5 % 4 == 0)
        W = (rng.standard_normal((I, J)) / np.sqrt(J)).astype(np.float32)
        b = rng.standard_normal(I).astype(np.float32)
        X = t(Xw)[:, :J]
        Y = torch.full((cols, I + 3), 7.0, device=dev)[:, :I]
        capi.call('sttode_tlinear', X, X.stride(0), xdiv, t(W), J, 0, t(b), None, 0, Y, Y.stride(0), cols, J, I, act, 0, st)
        xr = Xw[:, :J].astype(np.float64)[np.arange(cols) // xdiv]
        ref = xr @ W.T.astype(np.float64) + b
        ref = {0: ref, 1: np.maximum(ref, 0), 2: np.tanh(ref), 3: 1 / (1 + np.exp(-ref))}[act]
        assert_close(Y.cpu().numpy(), ref, rtol=1e-5, atol=2e-5, what=f'tlinear fwd {cols}x{J}->{I}')
        # input gradient with relu mask and accumulation
        dY = rng.standard_normal((cols, I)).astype(np.float32)
        mask = rng.standard_normal((cols, J)).astype(np.float32)
        base = rng.standard_normal((cols, J)).astype(np.float32)
        dX = t(base)
        capi.call('sttode_tlinear', t(dY), I, 1, t(W), J, 1, None, t(mask), J, dX, J, cols, I, J, 0, 1, st)
        ref = (dY.astype(np.float64) @ W.astype(np.float64) + base) * (mask > 0)
        assert_close(dX.cpu().numpy(), ref, rtol=1e-5, atol=2e-5, what=f'tlinear dX {cols}x{I}->{J}')
        # weight / bias gradient (accumulating), broadcast rows
        gW0, gb0 = rng.standard_normal((I, J)).astype(np.float32), rng.standard_normal(I).astype(np.float32)
        gW, gb = t(gW0), t(gb0)
        capi.call('sttode_twgrad', t(dY), I, X, X.stride(0), xdiv, gW, J, gb, cols, I, J, scratch, scratch.numel(), st)
        refW = dY.astype(np.float64).T @ xr + gW0
        refb = dY.astype(np.float64).sum(0) + gb0
        tol = 1e-5 * max(1.0, np.sqrt(cols))
        assert_close(gW.cpu().numpy(), refW, rtol=1e-5, atol=tol, what=f'twgrad dW {cols}')
        assert_close(gb.cpu().numpy(), refb, rtol=1e-5, atol=tol, what=f'twgrad db {cols}')
    _twgrad_generic_split_case(capi, dev, rng, scratch, st, cols=3001, N=70, K=67)


@pytest.mark.gpu
@pytest.mark.parametrize('defer', [False, True])
def test_layer_backward_at_batch_sizes_one_launch_and_deferred_reductions(defer):
    """sttode_tlinear_bwd above 2048 columns: dX tiles and dW tiles x splits in ONE launch (aligned operands: the branch-free panel loads,
    two tiles ahead; N = 10: the generic loads), the split sums added by a reduction per gradient or -- between sttode_twgrad_defer(1, buf)
    and sttode_twgrad_defer(0) -- by one launch for all of them, including a second gradient into a destination that is already pending
    (forces an early flush) and a buffer too small for everything (forces another)."""
    from sttode_amd import capi
    dev = _gpu()
    rng = np.random.default_rng(77)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
    scratch = torch.empty(1 << 20, device=dev)
    st = capi.stream_ptr()
    shapes = [(7392, 512, 256, 256), (4100, 20, 256, 256), (36960, 288, 32, 32), (2500, 64, 100, 64), (3000, 10, 256, 256), (2100, 256, 512, 512),
              (7392, 512, 256, 256)]
    cases = []
    for i, (cols, N, K, Kdx) in enumerate(shapes):
        dY = rng.standard_normal((cols, N)).astype(np.float32)
        X = rng.standard_normal((cols, K)).astype(np.float32)
        W = (rng.standard_normal((N, K)) / np.sqrt(N)).astype(np.float32)
        mask = rng.standard_normal((cols, Kdx)).astype(np.float32)
        gW0, gb0 = rng.standard_normal((N, K)).astype(np.float32), rng.standard_normal(N).astype(np.float32)
        cases.append(dict(cols=cols, N=N, K=K, Kdx=Kdx, dY=dY, X=X, W=W, mask=mask, gW0=gW0, gb0=gb0, d=(t(dY), t(X), t(W), t(mask)),
                          gW=t(gW0), gb=t(gb0), dX=torch.full((cols, Kdx), 3.0, device=dev)))
    cases[6]['gW'], cases[6]['gb'] = cases[0]['gW'], cases[0]['gb']          # the same destination twice (a shared weight)
    buf = torch.empty(3 << 20, device=dev)                                    # room for about two of the large gradients' split sums
    if defer:
        capi.call('sttode_twgrad_defer', 1, buf, buf.numel())
    try:
        for c in cases:
            dY, X, W, mask = c['d']
            capi.call('sttode_tlinear_bwd', dY, c['N'], W, c['K'], mask, c['Kdx'], c['dX'], c['Kdx'], c['Kdx'], 0, X, c['K'], 1, c['gW'], c['K'],
                      c['gb'], c['cols'], c['N'], c['K'], scratch, scratch.numel(), st)
    finally:
        capi.call('sttode_twgrad_defer', 0, None, 0)
    torch.cuda.synchronize()
    for i, c in enumerate(cases):
        ref = (c['dY'].astype(np.float64) @ c['W'].astype(np.float64)[:, :c['Kdx']]) * (c['mask'] > 0)
        assert_close(c['dX'].cpu().numpy(), ref, rtol=1e-5, atol=2e-5, what=f"layer backward dX {c['cols']}x{c['N']}->{c['Kdx']}")
        if i == 6:
            continue
        refW = c['dY'].astype(np.float64).T @ c['X'].astype(np.float64) + c['gW0']
        refb = c['dY'].astype(np.float64).sum(0) + c['gb0']
        if i == 0:                                                            # ... which received both gradients
            refW += cases[6]['dY'].astype(np.float64).T @ cases[6]['X'].astype(np.float64)
            refb += cases[6]['dY'].astype(np.float64).sum(0)
        tol = 1e-5 * max(1.0, np.sqrt(c['cols']))
        assert_close(c['gW'].cpu().numpy(), refW, rtol=1e-5, atol=tol, what=f"layer backward dW {c['cols']}x{c['N']}x{c['K']}")
        assert_close(c['gb'].cpu().numpy(), refb, rtol=1e-5, atol=tol, what=f"layer backward db {c['cols']}x{c['N']}")


@pytest.mark.gpu
def test_grouped_launch_of_independent_products_equals_the_separate_launches():
    """sttode_tgemm_group: two forward layers on the same input, a layer's backward (two products) and a fifth product that overflows the
    group leave as grouped launches; forward and input-gradient outputs carry the bits of the same calls made one by one, the weight gradient
    (split differently) the same sum."""
    from sttode_amd import capi
    dev = _gpu()
    g = torch.Generator(device='cpu').manual_seed(5)
    r = lambda *s: torch.randn(*s, generator=g).to(dev)
    cols = 5000
    X, Wa, ba, Wb, bb = r(cols, 256), r(512, 256) / 16, r(512), r(512, 256) / 16, r(512)
    dY, W2, X2, mask = r(cols, 256), r(256, 512) / 16, r(cols, 512), r(cols, 512)
    W3, b3 = r(24, 256), r(24)
    scratch = torch.empty(4 << 20, device=dev)
    st = capi.stream_ptr()

    def run(group):
        Ya, Yb, Yc = torch.empty(cols, 512, device=dev), torch.empty(cols, 512, device=dev), torch.empty(cols, 24, device=dev)
        dX, gW, gb = torch.empty(cols, 512, device=dev), torch.zeros(256, 512, device=dev), torch.zeros(256, device=dev)
        if group:
            capi.call('sttode_tgemm_group', 1)
        capi.call('sttode_tlinear', X, 256, 1, Wa, 256, 0, ba, None, 0, Ya, 512, cols, 256, 512, 1, 0, st)
        capi.call('sttode_tlinear', X, 256, 1, Wb, 256, 0, bb, None, 0, Yb, 512, cols, 256, 512, 2, 0, st)
        capi.call('sttode_tlinear_bwd', dY, 256, W2, 512, mask, 512, dX, 512, 512, 0, X2, 512, 1, gW, 512, gb, cols, 256, 512, scratch, scratch.numel(), st)
        capi.call('sttode_tlinear', X, 256, 1, W3, 256, 0, b3, None, 0, Yc, 24, cols, 256, 24, 0, 0, st)      # the fifth product: next launch
        if group:
            capi.call('sttode_tgemm_group', 0)
        torch.cuda.synchronize()
        return Ya, Yb, Yc, dX, gW, gb
    one, grp = run(False), run(True)
    for a, b, name in zip(one[:4], grp[:4], ('Ya', 'Yb', 'Yc', 'dX')):
        assert torch.equal(a, b), name
    # (the weight gradient's reduction is split differently inside a group -- fewer splits, the launch is full anyway: same sum, another order)
    refW, refb = dY.double().T @ X2.double(), dY.double().sum(0)
    for got in (one, grp):
        assert_close(got[4].cpu().numpy(), refW.cpu().numpy(), rtol=1e-5, atol=1e-5 * np.sqrt(cols), what='grouped / separate dW vs float64')
        assert_close(got[5].cpu().numpy(), refb.cpu().numpy(), rtol=1e-5, atol=1e-5 * np.sqrt(cols), what='grouped / separate db vs float64')
    ref = torch.relu(X.double() @ Wa.double().T + ba.double())
    assert_close(one[0].cpu().numpy(), ref.cpu().numpy(), rtol=1e-5, atol=2e-5, what='grouped forward vs float64')


def _hip_grads(tag, dataset, Tp, Tf, g, drop=None, train_mode=False):
    m = hip_model(dataset, Tp, Tf)
    m.zero_grad()
    eq, ep1, ep20 = grad_case_setup(g, tag, m)
    m.train(train_mode)
    try:
        out = m.forward(eq, ep1, ep20, *(drop if drop is not None else (None, None)))
        out[0].backward()
    finally:
        m.eval()
    grads = {k: (p.grad.detach().cpu().clone() if p.grad is not None else None) for k, p in m.named_parameters()}
    m.zero_grad()
    return grads, [float(out[0].detach())] + list(out[1:])


def _compare_grads(got, ref, rtol=2e-4):
    worst = ('', 0.0)
    for name, r in ref.items():
        gt = got[name]
        if r is None:
            assert gt is None, name
            continue
        assert gt is not None, name
        scale = float(r.abs().max()) + 1e-12
        err = float((gt.double() - r.double()).abs().max()) / scale
        if err > worst[1]:
            worst = (name, err)
    assert worst[1] <= rtol, f'gradient mismatch: {worst[0]} off by {worst[1]:.3e} of its max |g|'
    return worst


def _fp32_errs(g64, g32):
    """name -> distance of an fp32 gradient from the float64 one, in units of max |g| (one sample of what fp32 rounding does there)."""
    return {k: float((g32[k].double().cpu() - v.double().cpu()).abs().max()) / (float(v.double().abs().max()) + 1e-300)
            for k, v in g64.items() if v is not None}


def _grad_yardstick(got, g64, g32, what, digests=None, factor=2.0, floor=1e-4, more_ref_errs=None):
    """Per-parameter float64 yardstick (the rule of the pmath boundary rows and of the L = 4096 attention test): the HIP gradient's
    distance from the float64 evaluation of the same graph, in units of max |g|, may be at most `factor` x the distance of a CORRECT fp32
    evaluation (torch's own fp32 autograd of the oracle: `g32`; with `digests`, the reference's own backward() as recorded in the golden
    file: norm + first 48 entries) from that same float64 gradient, or `floor`, whichever is larger.  No flat band: a parameter whose
    fp32 evaluation is tight must be tight here too.  Returns the table rows (also written to profiles/ by the caller's `dump`)."""
    rows, bad = [], []
    for name, r64 in g64.items():
        gt = got[name]
        if r64 is None:
            assert gt is None, name
            continue
        assert gt is not None, name
        r64 = r64.double().cpu()
        scale = float(r64.abs().max()) + 1e-300
        e_hip = float((gt.double().cpu() - r64).abs().max()) / scale
        e_ref = float((g32[name].double().cpu() - r64).abs().max()) / scale
        if more_ref_errs is not None:                            # a second sample of the fp32 rounding error on this parameter
            e_ref = max(e_ref, more_ref_errs.get(name, 0.0))
        bound = max(factor * e_ref, floor)
        row = {'param': name, 'max_abs_g': scale, 'err_hip_vs_f64': e_hip, 'err_fp32_autograd_vs_f64': e_ref, 'bound': bound}
        if digests is not None and name in digests:
            dg = digests[name]                                   # [sum, norm, max|g|, first 48 entries] of the reference's fp32 gradient
            f64 = r64.flatten()
            n64 = float(f64.norm())
            k = min(48, f64.numel())
            hd = grad_digest(gt)
            e_ref_norm, e_hip_norm = abs(dg[1] - n64) / (n64 + 1e-300), abs(hd[1] - n64) / (n64 + 1e-300)
            e_ref_ent = float(np.abs(dg[3:3 + k] - f64[:k].numpy()).max()) / scale
            e_hip_ent = float(np.abs(hd[3:3 + k] - f64[:k].numpy()).max()) / scale
            row.update(err_hip_norm=e_hip_norm, err_reference_norm=e_ref_norm, err_hip_first48=e_hip_ent, err_reference_first48=e_ref_ent)
            if e_hip_norm > max(factor * e_ref_norm, floor) or e_hip_ent > max(factor * e_ref_ent, floor):
                bad.append((name, 'digest', e_hip_norm, e_ref_norm, e_hip_ent, e_ref_ent))
        if e_hip > bound:
            bad.append((name, 'entries', e_hip, e_ref, bound))
        rows.append(row)
    _dump_grad_table(what, rows)
    assert not bad, f'{what}: gradients beyond max({factor} x fp32-vs-f64 error, {floor}) of max |g|: {bad[:6]}'
    return rows


def _dump_grad_table(what, rows, text=None):
    """The per-parameter table of one gradient test, as text under gpurun_out/ (copied into profiles/ by the collection script)."""
    import os
    out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'gpurun_out', 'grad_tables')
    try:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, what.replace(' ', '_').replace('/', '_') + '.txt'), 'w') as f:
            if text is not None:                                   # (a table its caller formatted)
                f.write(text)
                return
            keys = [k for k in rows[0] if k != 'param']
            f.write('# ' + what + '\n# param ' + ' '.join(keys) + '\n')
            for r in rows:
                f.write(r['param'] + ' ' + ' '.join(f'{r[k]:.3e}' for k in keys) + '\n')
    except OSError:
        pass


@pytest.mark.parametrize('tag,dataset,Tp,Tf', [('eth', 'eth', 8, 12), ('nba', 'nba', 5, 10)])
def test_training_step_gradients_vs_reference_and_oracle(golden, tag, dataset, Tp, Tf):
    """forward() + total_loss.backward() on the HIP training kernels (train.py:81-85): losses and all 88 live parameter
    gradients vs the reference's own digests (tests/golden/forward_grads.npz) and, entry by entry, vs oracle autograd."""
    _gpu()
    g = golden('forward_grads')
    grads, losses = _hip_grads(tag, dataset, Tp, Tf, g)
    np.testing.assert_allclose(losses, g[f'{tag}_losses'], rtol=1e-4)
    for name, gr in grads.items():
        if f'{tag}_nograd::{name}' in g:
            assert gr is None, name
            continue
    digests = {name: g[f'{tag}_grad::{name}'] for name in grads if f'{tag}_grad::{name}' in g}
    # Entry by entry AND through the reference's own backward() digests, on the per-parameter float64 yardstick (_grad_yardstick): the
    # float64 evaluation of the same graph is the truth, torch's fp32 autograd of the oracle / the reference's recorded fp32 gradient are
    # the measure of what a correct fp32 evaluation can reach for THAT parameter
    g64, l64 = oracle_grads(tag, dataset, Tp, Tf, g, double=True)
    np.testing.assert_allclose(losses, l64, rtol=1e-4)
    ograds, olosses = oracle_grads(tag, dataset, Tp, Tf, g)
    np.testing.assert_allclose(losses, olosses, rtol=1e-4)
    _grad_yardstick(grads, g64, ograds, f'training step {tag}', digests=digests)


def test_training_step_with_dropout_masks_vs_oracle(golden):
    """train() mode: nn.Dropout(0.1) of both positional encoders as injected masks (model/STTODE.py:140,176)."""
    dev = _gpu()
    g = golden('forward_grads')
    rng = np.random.default_rng(4)
    n = g['eth_obs'].shape[0]
    dp = torch.from_numpy(((rng.random((n * 8, 64)) < 0.9) / 0.9).astype(np.float32))
    df = torch.from_numpy(((rng.random((n * 12, 64)) < 0.9) / 0.9).astype(np.float32))
    grads, losses = _hip_grads('eth', 'eth', 8, 12, g, drop=(dp.to(dev), df.to(dev)), train_mode=True)
    g64, olosses = oracle_grads('eth', 'eth', 8, 12, g, drop=(dp, df), double=True)
    np.testing.assert_allclose(losses, olosses, rtol=1e-4)
    g32, _ = oracle_grads('eth', 'eth', 8, 12, g, drop=(dp, df))
    # block 1's conv / W_ih gradients: torch's fp32 autograd lands 1.6e-5 of max |g| from float64 WITH these masks and 7.9e-5 without
    # them on the same scene (HIP: 1.26e-4 and 1.34e-4 with the MFMA GRU-sequence kernels, 1.61e-4 with round 5's vector-ALU form whose 96-term
    # sums run in index order) -- all of them samples of the same fp32 rounding on two ill-conditioned rows: the yardstick takes the larger
    # reference sample and three times it
    more = _fp32_errs(oracle_grads('eth', 'eth', 8, 12, g, double=True)[0], oracle_grads('eth', 'eth', 8, 12, g)[0])
    _grad_yardstick(grads, g64, g32, 'training step eth with dropout masks', more_ref_errs=more, factor=3.0)
    assert abs(losses[0] - float(g['eth_losses'][0])) > 1e-3      # the masks really changed the objective


def test_adam_steps_track_the_oracle(golden):
    """train.py:81-87 loop (zero_grad / backward / Adam step) for 5 iterations on the HIP model vs the oracle, same noises."""
    from sttode_amd import STTODENet
    from oracle.sttode_ref import STTODENetRef
    from sttode_amd.weights import make_weights, to_torch_state_dict
    dev = _gpu()
    g = golden('forward_grads')
    sd = to_torch_state_dict(make_weights(1234, past_length=8, future_length=12))
    hip = STTODENet(make_args('eth', 8, 12), dev)
    hip.load_state_dict(sd, strict=True)
    hip.eval()                                                     # deterministic data path (no rotation / dropout)
    ora = STTODENetRef(make_args('eth', 8, 12)).eval()
    ora.load_state_dict(sd, strict=True)
    oh, oo = torch.optim.Adam(hip.parameters(), lr=1e-3), torch.optim.Adam(ora.parameters(), lr=1e-3)
    lh, lo = [], []
    for it in range(5):
        eq, ep1, ep20 = grad_case_setup(g, 'eth', hip)
        grad_case_setup(g, 'eth', ora)
        tot = hip.forward(eq, ep1, ep20)[0]
        oh.zero_grad(); tot.backward(); oh.step()
        vo = ora.forward_loss_tensors(eq, ep1, ep20)[0]
        oo.zero_grad(); vo.backward(); oo.step()
        lh.append(float(tot.detach())); lo.append(float(vo.detach()))
    assert lh[-1] < lh[0]                                          # it learns
    np.testing.assert_allclose(lh, lo, rtol=2e-3)
    w_h = hip.state_dict()['decoder.decompose.0.decoder_y.layers.0.weight'].cpu()
    w_o = ora.state_dict()['decoder.decompose.0.decoder_y.layers.0.weight']
    assert float((w_h - w_o).abs().max()) < 5e-4


def test_train_mode_rotation_vs_oracle(golden):
    """set_data in train() mode (model/STTODE.py:419-426): scene rotated about scene_orig by an injected theta."""
    _gpu()
    g = golden('forward_grads')
    m, ora = hip_model('eth', 8, 12), oracle_model('eth', 8, 12)
    o, p = torch.from_numpy(g['eth_obs']), torch.from_numpy(g['eth_pred'])
    eq, ep1, ep20 = (torch.from_numpy(g[f'eth_eps_{k}']) for k in ('q', 'p1', 'p20'))
    m.train()
    try:
        m.set_data(None, o, p, torch.ones(7, 8), torch.ones(7, 12), theta=0.7)
        with torch.no_grad():
            vals = m.forward(eq, ep1, ep20)
    finally:
        m.eval()
    ora.set_data(None, o, p, theta=0.7)
    ref = ora.forward_losses(eq, ep1, ep20)
    np.testing.assert_allclose([float(vals[0])] + list(vals[1:]), ref, rtol=1e-4)
    assert abs(ref[0] - float(g['eth_losses'][0])) > 1e-3 * abs(ref[0])        # the rotation changed the objective


def test_train_mode_agent_subsampling_follows_numpy_generator():
    """set_data in train() mode with more agents than max_train_agent (model/STTODE.py:405-413): the scene is sub-sampled with
    np.random.choice(N, max_train_agent) -- with replacement, from NumPy's global generator.  With the generator seeded, the HIP
    path must pick the same agents: its objective equals the oracle's on the explicitly sub-sampled (and rotated) scene."""
    from sttode_amd import scenes
    _gpu()
    m, ora = hip_model('eth', 8, 12), oracle_model('eth', 8, 12)
    obs, pred = scenes.eth_scene(4242, n_min=40, n_max=40)                    # 40 > max_train_agent = 32
    rng = np.random.default_rng(3)
    eq, ep1, ep20 = (torch.from_numpy(rng.standard_normal(sh).astype(np.float32)) for sh in ((32, 32), (32, 32), (640, 32)))
    np.random.seed(1234)
    ind = np.random.choice(40, 32)                                             # what the reference would draw
    assert len(set(ind.tolist())) < 32                                         # (with replacement: duplicates occur)
    m.train()
    try:
        np.random.seed(1234)
        m.set_data(None, torch.from_numpy(obs), torch.from_numpy(pred), torch.ones(40, 8), torch.ones(40, 12), theta=-1.1)
        assert m.agent_num == 32
        with torch.no_grad():
            vals = m.forward(eq, ep1, ep20)
    finally:
        m.eval()
    ora.set_data(None, torch.from_numpy(obs[ind]), torch.from_numpy(pred[ind]), theta=-1.1)
    ref = ora.forward_losses(eq, ep1, ep20)
    np.testing.assert_allclose([float(vals[0])] + list(vals[1:]), ref, rtol=1e-4)


def test_train_epoch_loop_on_csv_dataset(tmp_path):
    """train.py:72-95 loop over TrajectoryDataset + DataLoader(batch_size=1): augmentation on, losses finite and decreasing
    over repeated epochs on a tiny synthetic file; checkpoint round-trips through the inference path."""
    from torch.utils.data import DataLoader
    from sttode_amd import STTODENet
    from sttode_amd.datasets import TrajectoryDataset
    from sttode_amd.trainer import save_checkpoint, train_epoch
    dev = _gpu()
    rng = np.random.default_rng(6)
    rows = []
    for p in range(5):
        start, vel = rng.uniform(0, 10, 2), rng.normal(0, 0.3, 2)
        for t in range(26):
            x, y = start + vel * t + rng.normal(0, 0.02, 2)
            rows.append((10 * t, p + 1, x, y))
    rows.sort()
    np.savetxt(tmp_path / 'a.csv', np.asarray(rows).T, delimiter=',', fmt='%.6f')
    ds = TrajectoryDataset(str(tmp_path), obs_len=8, pred_len=12, skip=2, min_ped=1, files=['a.csv'])
    loader = DataLoader(ds, batch_size=1, shuffle=False)
    args = make_args('eth', 8, 12)
    args.num_epochs, args.iternum_print = 6, 1000
    torch.manual_seed(0)
    model = STTODENet(args, dev)                        # default PyTorch-style init of the parameter tree
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=10, gamma=0.5)
    means = []
    for epoch in range(args.num_epochs):
        ls = train_epoch(args, epoch, model, opt, sched, loader, log=None)
        assert len(ls) == len(ds) and np.isfinite(ls).all()
        means.append(np.mean(ls))
    assert means[-1] < means[0]
    save_checkpoint(tmp_path / 'model_0006.p', args, model, opt, sched, 5)
    cp = torch.load(tmp_path / 'model_0006.p', weights_only=False)
    m2 = STTODENet(cp['model_cfg'], dev).eval()
    m2.load_state_dict(cp['model_dict'], strict=True)
    batch = ds[0]
    m2.set_data(None, batch[0], batch[1], batch[6], batch[7])
    out = m2.inference(None)
    assert out.shape == (20, batch[0].shape[0], 12, 2) and bool(torch.isfinite(out).all())


@pytest.mark.parametrize('tag,dataset,Tp,Tf', [('eth', 'eth', 8, 12), ('nba', 'nba', 5, 10)])
def test_sampler_training_step_vs_reference_and_oracle(golden, tag, dataset, Tp, Tf):
    """Stage-2 training step (trainsampler.py:134-150,171-185) on the HIP path: loss + gradients of the Sampler's parameters
    (through the K = 20 decode, the latent codes and the tanh Q-net) vs the reference's digests and vs oracle autograd."""
    from sttode_amd import Sampler, samplerloss
    from sttode_amd.weights import make_sampler_weights, to_torch_state_dict
    dev = _gpu()
    g, gg = golden('sampler'), golden('sampler_grads')
    mode = str(gg[f'{tag}_mode'])
    net = hip_model(dataset, Tp, Tf)
    smp = Sampler(sampler_args(dataset, Tp, Tf))
    smp.load_state_dict(to_torch_state_dict(make_sampler_weights()), strict=True)
    smp.set_device(dev)
    smp.train()
    smp.share_eps = mode != 'peragent'
    inp, fut = sampler_case_inputs(g, tag, dataset)
    if dataset == 'eth':
        n = inp['obs'].shape[0]
        net.set_data(None, torch.from_numpy(inp['obs']), torch.from_numpy(inp['pred']), torch.ones(n, Tp), torch.ones(n, Tf))
    else:
        net.set_data_nba({k: (torch.from_numpy(v) if isinstance(v, np.ndarray) else v) for k, v in inp['data'].items()})
    futd = torch.from_numpy(fut).to(dev)
    cfg = {'weight': 1, 'scale': 1.0}
    # Conditioning: logvar = log(A^2 + 1e-8) makes dKL/dA = A - A / (A^2 + 1e-8), which swings by several percent for a 1e-6
    # change of an A near 3e-5 (a handful of the n*K*nz codes are always there).  Two fp32 evaluations of A therefore agree on
    # the A-path gradients only to ~1e-2 of max |g| (torch-on-CPU vs torch-on-GPU would not do better); everything that does
    # not pass through that factor -- the diversity term end to end, and q_b -- is checked at 1e-3 / 1e-4.
    from oracle import sampler_ref as SR
    onet, osmp = oracle_model(dataset, Tp, Tf), oracle_sampler(dataset, Tp, Tf)
    osmp.share_eps = smp.share_eps
    if dataset == 'eth':
        onet.set_data(None, torch.from_numpy(inp['obs']), torch.from_numpy(inp['pred']))
    else:
        onet.set_data_nba({k: (torch.from_numpy(v) if isinstance(v, np.ndarray) else v) for k, v in inp['data'].items()})
    for which, tol_a, tol_b in (('diverse', 1e-3, 1e-3), ('kld', 2e-2, 1e-4), ('total', 2e-2, 1e-3)):
        smp.zero_grad()
        osmp.zero_grad()
        dec, sd, vd, _ = smp.forward(net, mean=(mode == 'mean'), eps=torch.from_numpy(g[f'{tag}_{mode}_eps']))
        assert dec.requires_grad and sd.mu.requires_grad
        assert_close(dec.detach().cpu().numpy(), g[f'{tag}_{mode}_dec'], what='dec (training kernels)')
        tot, ld, _ = samplerloss.compute_sampler_loss(smp.args, futd, dec.reshape(-1, 20, Tf, 2), 1, None, vd, sd, cfg)
        (tot if which == 'total' else ld[which]).backward()
        odec, osd, ovd, _ = osmp.forward(onet, mean=(mode == 'mean'), eps=torch.from_numpy(g[f'{tag}_{mode}_eps']))
        otot, old = SR.compute_sampler_loss(osmp.args, torch.from_numpy(fut), odec.reshape(-1, 20, Tf, 2), ovd, osd, cfg)
        (otot if which == 'total' else old[which]).backward()
        for (name, prm), (_, o) in zip(smp.named_parameters(), osmp.named_parameters()):
            if o.grad is None:                                      # unused by this loss term: ours reports None or exact zeros
                assert prm.grad is None or not bool(prm.grad.any()), name
                continue
            err = float((prm.grad.cpu().double() - o.grad.double()).abs().max()) / (float(o.grad.abs().max()) + 1e-20)
            assert err <= (tol_b if name.startswith('q_b.') else tol_a), (which, name, err)
    got_loss = [float(tot.detach()), float(ld['kld'].detach()), float(ld['diverse'].detach())]
    np.testing.assert_allclose(got_loss, gg[f'{tag}_loss'], rtol=1e-4)
    for name, prm in smp.named_parameters():                        # the reference's own gradients (total loss)
        if f'{tag}_nograd::{name}' in gg:
            assert prm.grad is None, name
            continue
        ref, got = gg[f'{tag}_grad::{name}'], grad_digest(prm.grad)
        tol = 1e-3 if name.startswith('q_b.') else 2e-2
        assert abs(got[1] - ref[1]) <= tol * ref[1] + 1e-9, (name, got[1], ref[1])
        assert np.abs(got[3:] - ref[3:]).max() <= tol * (ref[2] + 1e-12), (name, np.abs(got[3:] - ref[3:]).max(), ref[2])
    assert all(p.grad is None for p in net.parameters())           # the prediction net stays frozen


def test_sampler_backward_kernels_vs_torch_autograd():
    """sttode_sampler_loss_bwd and the latent backward op on IDENTICAL inputs vs float64 torch autograd (well-conditioned check of
    the pieces whose end-to-end comparison is limited by the log(A^2 + 1e-8) conditioning)."""
    from sttode_amd import capi, samplerloss
    from sttode_amd.dist import Normal
    dev = _gpu()
    rng = np.random.default_rng(33)
    n, K, nz, Tf = 9, 20, 32, 12
    t = lambda a: torch.from_numpy(a.astype(np.float32)).to(dev)
    mu, lv = t(rng.standard_normal((n * K, nz))), t(0.5 * rng.standard_normal((n * K, nz)))
    mo = t(0.7 * rng.standard_normal((n, K, Tf, 2)))
    mu.requires_grad_(True); lv.requires_grad_(True); mo.requires_grad_(True)
    kld, div = samplerloss._per_agent(Normal(mu=mu, logvar=lv), None, mo, 2.0)
    wk, wd = t(rng.standard_normal(n)), t(rng.standard_normal(n))
    ((kld * wk).sum() + (div * wd).sum()).backward()
    m64, l64, o64 = (x.detach().double().cpu().requires_grad_(True) for x in (mu, lv, mo))
    t2 = torch.exp(0.5 * l64) / (1 + 1e-8)
    kl = (0.5 * ((m64 / (1 + 1e-8)) ** 2 + t2 * t2) - 0.5 - torch.log(t2)).view(n, -1).sum(1)
    dv = torch.stack([(-(torch.nn.functional.pdist(m.reshape(K, -1)) ** 2) / 2.0).exp().mean() for m in o64])
    ((kl * wk.double().cpu()).sum() + (dv * wd.double().cpu()).sum()).backward()
    for got, ref, nm in ((mu.grad, m64.grad, 'dmu'), (lv.grad, l64.grad, 'dlogvar'), (mo.grad, o64.grad, 'dmotion')):
        assert_close(got.cpu().numpy(), ref.numpy(), rtol=1e-4, atol=1e-6 * float(ref.abs().max()), what=nm)
    # latent backward: dA = dz * eps + dlogvar * 2A / (A^2 + 1e-8), including A near zero
    A = rng.standard_normal((n, K * nz)).astype(np.float32)
    A[0, :8] = [0.0, 1e-6, -3e-5, 1e-4, -1e-4, 3e-4, 1e-3, -1e-2]
    dz, dl = rng.standard_normal((n * K, nz)).astype(np.float32), rng.standard_normal((n * K, nz)).astype(np.float32)
    for mode, eps in ((0, None), (1, rng.standard_normal((1, nz)).astype(np.float32)), (2, rng.standard_normal((n, nz)).astype(np.float32))):
        dA = torch.empty(n, K * nz, device=dev)
        capi.call('sttode_train_ewise', 11, t(dz), t(dl), t(A), t(eps) if eps is not None else None, dA, n * K * nz, nz * 4 + mode, float(K * nz),
                  capi.stream_ptr())
        a64 = A.astype(np.float64).reshape(n * K, nz)
        e = 0.0 if eps is None else (np.broadcast_to(eps, (n * K, nz)) if mode == 1 else np.repeat(eps, K, axis=0)).astype(np.float64)
        ref = dz * e + dl * 2 * a64 / (a64 * a64 + 1e-8)
        assert_close(dA.cpu().numpy().reshape(n * K, nz), ref, rtol=1e-5, atol=1e-5, what=f'latent bwd mode {mode}')


def test_decoder_stack_ops_vs_reference_golden(golden):
    """The unused decoder-side stack as op-level drop-ins (hypertransformer.py:156-236, ode_demo.py:195-213): self-attention
    over L = 6, cross-attention over a memory of S = 9 steps, FFN, LayerNorms, one Euler step + relu."""
    from sttode_amd.hypertransformer import ODEG, TransformerDecoderLayer
    from sttode_amd.weights import make_decoder_layer_weights, to_torch_state_dict
    dev = _gpu()
    g = golden('decoder_stack')
    layer = TransformerDecoderLayer(64, 8, 256, dropout=0.0)
    layer.load_state_dict(to_torch_state_dict(make_decoder_layer_weights(61, d=64, ff=256)), strict=True)
    with pytest.raises(Exception):
        layer(torch.from_numpy(g['tgt']), torch.from_numpy(g['mem']))          # CPU tensors: refuse
    layer.to(dev)
    tgt, mem = torch.from_numpy(g['tgt']).to(dev), torch.from_numpy(g['mem']).to(dev)
    y, ws, wc = layer(tgt, mem, seq_mask=True, need_weights=True)
    assert_close(y.cpu().numpy(), g['layer_out'], what='decoder layer')
    assert ws.shape == (10, 6, 6) and wc.shape == (10, 6, 9)
    np.testing.assert_allclose(wc.sum(-1).cpu().numpy(), 1.0, atol=1e-5)
    z, w = ODEG(layer, 2, 3).to(dev)(tgt, mem, seq_mask=True)
    assert_close(z.cpu().numpy(), g['odeg_out'], what='ODEG')


@pytest.mark.parametrize('N', [1, 2, 33])
def test_training_step_edge_scene_sizes_vs_oracle(N):
    """Smallest scenes (SDD has single-pedestrian scenes; N = 2 is the ETH minimum) and a scene just past 32 agents (two column
    tiles in the K = 1 decode, 42 in the K = 20 decode): losses and gradients vs float64 oracle autograd; eager and hipGraph steps agree."""
    from sttode_amd import scenes
    dev = _gpu()
    o, p = scenes.eth_scene(7100 + N, n_min=N, n_max=N)
    rng = np.random.default_rng(N)
    g = {'eth_obs': o, 'eth_pred': p, 'eth_eps_q': rng.standard_normal((N, 32)).astype(np.float32),
         'eth_eps_p1': rng.standard_normal((N, 32)).astype(np.float32), 'eth_eps_p20': rng.standard_normal((N * 20, 32)).astype(np.float32)}
    grads, losses = _hip_grads('eth', 'eth', 8, 12, g)             # first step of this shape: eager
    g64, l64 = oracle_grads('eth', 'eth', 8, 12, g, double=True)
    np.testing.assert_allclose(losses, l64, rtol=1e-4)
    g32, _ = oracle_grads('eth', 'eth', 8, 12, g)
    _grad_yardstick(grads, g64, g32, f'training step eth N={N}')
    grads2, losses2 = _hip_grads('eth', 'eth', 8, 12, g)           # second step: captured + replayed hipGraph
    np.testing.assert_allclose(losses2, losses, rtol=1e-6)
    _compare_grads(grads2, {k: v for k, v in grads.items()}, rtol=1e-6)


@pytest.mark.parametrize('B,N,Tp,Tf', [(16, 11, 5, 10), (3, 10, 10, 40), (32, 11, 5, 10)])
def test_training_step_nba_shapes_vs_oracle(B, N, Tp, Tf):
    """NBA training step at a longer attention group (L = 16: geodesic-attention backward over 16 x 16 score blocks) and at the
    BASELINE config-5 horizon (obs 10 / pred 40, N = 10); round 5: at the reference's batch (32 x 11: the live backward's 704 columns run on the
    LDS-tiled GEMMs): losses and all gradients vs float64 oracle autograd."""
    from sttode_amd import scenes
    _gpu()
    d = scenes.nba_batch(50 + B, B, N=N, obs_len=Tp, pred_len=Tf)
    n = B * N
    rng = np.random.default_rng(B)
    eps = [rng.standard_normal(s).astype(np.float32) for s in ((n, 32), (n, 32), (n * 20, 32))]
    data = {k: (torch.from_numpy(v) if isinstance(v, np.ndarray) else v) for k, v in d.items()}
    m = hip_model('nba', Tp, Tf)
    m.zero_grad()
    m.set_data_nba(data)
    out = m.forward(*[torch.from_numpy(e) for e in eps])
    out[0].backward()
    grads = {k: (p.grad.detach().cpu().clone() if p.grad is not None else None) for k, p in m.named_parameters()}
    m.zero_grad()
    from oracle.sttode_ref import STTODENetRef
    o = STTODENetRef(make_args('nba', Tp, Tf)).eval()
    o.load_state_dict(oracle_model('nba', Tp, Tf).state_dict(), strict=True)
    o = o.double()
    o.set_data_nba({k: (v.double() if isinstance(v, torch.Tensor) else v) for k, v in data.items()})
    prev = torch.get_default_dtype()
    try:
        torch.set_default_dtype(torch.float64)
        vals = o.forward_loss_tensors(*[torch.from_numpy(e).double() for e in eps])
        vals[0].backward()
    finally:
        torch.set_default_dtype(prev)
    np.testing.assert_allclose([float(out[0].detach())] + list(out[1:]), [float(v.detach()) for v in vals], rtol=1e-4)
    o32 = oracle_model('nba', Tp, Tf)                       # the same graph in fp32 (torch autograd): what a correct fp32 evaluation reaches
    o32.zero_grad()
    o32.set_data_nba(data)
    o32.forward_loss_tensors(*[torch.from_numpy(e) for e in eps])[0].backward()
    g32 = {k: (p.grad.clone() if p.grad is not None else None) for k, p in o32.named_parameters()}
    o32.zero_grad()
    _grad_yardstick(grads, {k: p.grad for k, p in o.named_parameters()}, g32, f'training step nba B={B} N={N} Tp={Tp} Tf={Tf}')
    # the same step again, twice: the second is the eager step's twin, the third the captured + replayed hipGraph (NBA batches replay too)
    for _ in range(2):
        m.zero_grad()
        m.set_data_nba(data)
        out2 = m.forward(*[torch.from_numpy(e) for e in eps])
        out2[0].backward()
        np.testing.assert_allclose([float(out2[0].detach())] + list(out2[1:]), [float(out[0].detach())] + list(out[1:]), rtol=1e-6)
        _compare_grads({k: (p.grad.detach().cpu() if p.grad is not None else None) for k, p in m.named_parameters()}, grads, rtol=1e-6)
    assert any(k[0] == 'nba' for k in m._graphs), 'the NBA-size step was not captured'


def test_pmath_autograd_functions_vs_reference_golden(golden):
    """Artanh / Arsinh / RiemannianGradient (hyptorch/pmath.py:16-60) as autograd functions over the HIP ops."""
    from sttode_amd import pmath
    dev = _gpu()
    g = golden('pmath_grads')
    gr = torch.from_numpy(g['g']).to(dev)
    x = torch.from_numpy(g['x']).to(dev).requires_grad_(True)
    pmath.artanh(x).backward(gr)
    assert_close(x.grad.cpu().numpy(), g['artanh_grad'], rtol=1e-4, atol=1e-5, what='artanh backward')
    x = torch.from_numpy(g['x']).to(dev).requires_grad_(True)
    pmath.arsinh(x * 20).backward(gr)
    assert_close(x.grad.cpu().numpy(), g['arsinh_grad'], rtol=1e-4, atol=1e-5, what='arsinh backward')
    for c in (1.0, 0.5):
        pmath.RiemannianGradient.c = c
        xr = torch.from_numpy(g['xr']).to(dev).requires_grad_(True)
        y = pmath.RiemannianGradient.apply(xr)
        assert torch.equal(y, xr)
        y.backward(torch.from_numpy(g['gr']).to(dev))
        assert_close(xr.grad.cpu().numpy(), g[f'riem_c{c}_grad'], rtol=1e-5, atol=1e-6, what='riemannian gradient')
    pmath.RiemannianGradient.c = 1


@pytest.mark.parametrize('method,steps', [('euler', 1), ('euler', 4), ('rk4', 3), ('rk4_classic', 2)])
def test_ode_encoder_integrators_vs_oracle(method, steps):
    """ODEG_Encoder as an op with multi-step Euler / RK4 right-hand-side evaluations on the HIP layer kernels vs the CPU oracle
    (the reference itself only ever takes one Euler step; these variants are oracle-checked only: no reference pin exists)."""
    from oracle.sttode_ref import EncoderLayer, ode_integrate_ref
    from sttode_amd.hypertransformer import ODEG_Encoder, TransformerEncoderLayer
    from sttode_amd.weights import make_decoder_layer_weights, to_torch_state_dict
    dev = _gpu()
    sd = {k: v for k, v in to_torch_state_dict(make_decoder_layer_weights(71, d=64, ff=256)).items()
          if not k.startswith('cross_attn') and not k.startswith('norm3')}
    sd = {k: (v * 0.3 if k.endswith('weight') and 'norm' not in k else v) for k, v in sd.items()}     # keep the RHS mild
    layer = TransformerEncoderLayer(64, 8, 256)
    layer.load_state_dict(sd, strict=True)
    ora = EncoderLayer(64, 8, 256).eval()
    ora.load_state_dict(sd, strict=True)
    rng = np.random.default_rng(5)
    x = torch.from_numpy(rng.standard_normal((5, 7, 1, 64)).astype(np.float32))
    enc = ODEG_Encoder(layer, 1, 0.9, method=method, steps=steps).to(dev)
    out = enc(x.to(dev))
    with torch.no_grad():
        ref = torch.relu(ode_integrate_ref(ora, x, 0.9, method, steps))
    assert_close(out.cpu().numpy(), ref.numpy(), what=f'ODEG_Encoder {method} x{steps}')


@pytest.mark.parametrize('method,steps', [('euler', 3), ('rk4', 1), ('rk4', 2), ('rk4_classic', 2)])
def test_model_path_ode_integrator_parameter_vs_oracle(method, steps):
    """method / n_steps as parameters of the fused encoder kernel (post_attn_kernel<true>, attention length 1): inference() and the
    staged encode_history() with multi-step Euler / RK4 against the oracle model whose ODE block is integrated by
    oracle.ode_integrate_ref.  The reference only ever takes one Euler step (ode_demo.py:186-190), so these variants have no
    reference pin (parity unpinned, like the op-level test above); the default ('euler', 1) stays on the reference-pinned kernel."""
    from oracle.sttode_ref import ode_integrate_ref
    from sttode_amd import STTODENet, capi, scenes
    from sttode_amd.weights import make_weights, to_torch_state_dict
    m = STTODENet(make_args('eth', 8, 12), _gpu()).eval()
    m.load_state_dict(to_torch_state_dict(make_weights(1234)), strict=True)
    m.ode_method, m.ode_steps = method, steps
    ora = oracle_model('eth', 8, 12)
    blk = ora.past_encoder.ODE_Encoder.odeblock
    orig = blk.forward
    blk.forward = lambda x: ode_integrate_ref(lambda y: blk.odefunc(0.0, y), x, blk.t1, method, steps)
    try:
        sb = scenes.make_scene_batch(range(60, 66), 'eth')
        z = scenes.latents(61, sb.n_agents)
        m.set_scene_batch(sb.past, sb.future, sb.scene_ptr)
        out = m.inference(None, z=torch.from_numpy(z)).cpu().numpy()
        pf = m.past_feature.cpu().numpy()
        m.set_scene_batch(sb.past, sb.future, sb.scene_ptr)
        pf_staged = m.encode_history().cpu().numpy()
        for s in range(sb.n_scenes):
            a, b = int(sb.scene_ptr[s]), int(sb.scene_ptr[s + 1])
            obs, pred = sb.scene(s)
            tr = {}
            ref = oracle_scene_inference(ora, obs, pred, z[a * 20:b * 20], trace=tr)
            assert_close(pf[a:b], tr['past_feature'].numpy(), what=f'{method} x{steps}: past_feature scene {s}')
            assert_close(out[:, a:b], ref, what=f'{method} x{steps}: inference scene {s}')
        # staged API: same integrator (its velocities come from the un-normalised track: equal up to rounding of a - b vs (a-o) - (b-o))
        np.testing.assert_allclose(pf_staged[:, 64:], pf[:, 64:], rtol=2e-3, atol=2e-3)
    finally:
        blk.forward = orig


@pytest.mark.parametrize('method,steps,B,Tp,Tf', [('euler', 3, 6, 5, 10), ('rk4', 2, 6, 5, 10), ('rk4_classic', 1, 12, 5, 10), ('rk4', 40, 4, 10, 40)])
def test_model_path_ode_integrator_with_attention_groups_vs_oracle(method, steps, B, Tp, Tf):
    """The same parameter on the NBA branch (attention groups > 1): every stage of the integrator is a pass over the whole group --
    in-projection of the state, geodesic attention over the batch, f(y), axpy combinations -- enqueued natively by ONE
    sttode_inference_nba call (csrc/pipeline.hip), here against the oracle model whose ODE block is integrated by
    oracle.ode_integrate_ref with its attention over the same group.  ('rk4', 40) on obs 10 / pred 40 is BASELINE config 5's
    "40 RK4 steps" read literally.  Parity unpinned like every non-default integrator (the reference takes one Euler step).
    inference(), its past_feature, the pipelined form and the staged encode_history() are checked."""
    from oracle.sttode_ref import ode_integrate_ref
    from sttode_amd import STTODENet, scenes
    from sttode_amd.weights import make_weights, to_torch_state_dict
    N = 11 if Tp == 5 else 10
    m = STTODENet(make_args('nba', Tp, Tf), _gpu()).eval()
    m.load_state_dict(to_torch_state_dict(make_weights(1234, past_length=Tp, future_length=Tf)), strict=True)
    m.ode_method, m.ode_steps = method, steps
    ora = oracle_model('nba', Tp, Tf)
    blk = ora.past_encoder.ODE_Encoder.odeblock
    orig = blk.forward
    blk.forward = lambda x: ode_integrate_ref(lambda y: blk.odefunc(0.0, y), x, blk.t1, method, steps)
    try:
        d = scenes.nba_batch(77, B, N=N, obs_len=Tp, pred_len=Tf)
        data = {'past_traj': torch.from_numpy(d['past_traj']), 'future_traj': torch.from_numpy(d['future_traj'])}
        z = scenes.latents(78, B * N)
        m.set_data_nba(data)
        out = m.inference(data, z=torch.from_numpy(z)).cpu().numpy()
        pf = m.past_feature.cpu().numpy()
        tr = {}
        with torch.no_grad():
            ora.set_data_nba(data)
            ref = ora.inference(data, z=torch.from_numpy(z), trace=tr).numpy()
        # the integrated state is amplified by the step count (40 RK4 steps of a 12-unit horizon): float64 yardstick for past_feature
        assert_close(pf[:, :64], tr['past_feature'].numpy()[:, :64], what=f'{method} x{steps}: ftraj_input')
        o64 = type(ora)(ora.args).eval()
        o64.load_state_dict(ora.state_dict(), strict=True)
        o64 = o64.double()
        b64 = o64.past_encoder.ODE_Encoder.odeblock
        b64.forward = lambda x: ode_integrate_ref(lambda y: b64.odefunc(0.0, y), x, b64.t1, method, steps)
        prev = torch.get_default_dtype()
        try:
            torch.set_default_dtype(torch.float64)
            t64 = {}
            with torch.no_grad():
                d64 = {k: v.double() for k, v in data.items()}
                o64.set_data_nba(d64)
                o64.inference(d64, z=torch.from_numpy(z).double(), trace=t64)
        finally:
            torch.set_default_dtype(prev)
        p64 = t64['past_feature'].numpy()
        e_ref = np.abs(tr['past_feature'].numpy() - p64).max() / (np.abs(p64).max() + 1e-30)
        e_hip = np.abs(pf - p64).max() / (np.abs(p64).max() + 1e-30)
        assert e_hip <= max(2 * e_ref, 1e-4), f'{method} x{steps}: past_feature {e_hip:.3e} of max |pf| from float64 (fp32 oracle: {e_ref:.3e})'
        if e_ref < 2e-5:                                   # predictions: plain tolerance where fp32 itself is tight
            assert_close(out, ref, what=f'{method} x{steps}: inference')
        # pipelined form == serial form, bitwise
        m.reset_async()
        m.set_data_nba(data)
        h = m.inference_async(z=torch.from_numpy(z).to(m.device))
        assert np.array_equal(m.wait(h).cpu().numpy(), out)
        m.reset_async()
        # staged API: the Python spelling of the same stages (hypertransformer.ode_integrate over the new entry points)
        m.set_data_nba(data)
        pf_staged = m.encode_history().cpu().numpy()
        e_st = np.abs(pf_staged - p64).max() / (np.abs(p64).max() + 1e-30)
        assert e_st <= max(2 * e_ref, 1e-4) * 1.5 + 2e-3   # (its velocities come from the un-normalised track: rounding of a - b vs (a-o) - (b-o))
    finally:
        blk.forward = orig


@pytest.mark.parametrize('N', [1, 3, 17])
def test_single_small_scene_inference_vs_oracle(N):
    """One scene on its own (the reference's call pattern, test.py:182-184) at sizes below one 16-column tile per agent stage and
    20 .. 340 trajectories in the decoder (partial 64-column work items everywhere)."""
    from sttode_amd import scenes
    _gpu()
    o, p = scenes.eth_scene(8200 + N, n_min=N, n_max=N)
    z = scenes.latents(300 + N, N)
    m = hip_model('eth', 8, 12)
    m.set_data(None, torch.from_numpy(o), torch.from_numpy(p), torch.ones(N, 8), torch.ones(N, 12))
    out = m.inference(None, z=torch.from_numpy(z)).cpu().numpy()
    ref = oracle_scene_inference(oracle_model('eth', 8, 12), o, p, z)
    assert out.shape == (20, N, 12, 2)
    assert_close(out, ref, what=f'single scene N={N}')


def test_sampler_training_loop_reduces_the_objective():
    """trainsampler.py:171-185 loop (frozen prediction net, Adam over sampler.parameters()) for a few iterations on one scene:
    the stage-2 objective goes down and only the sampler's parameters move."""
    from sttode_amd import Sampler, samplerloss, scenes
    dev = _gpu()
    net = hip_model('eth', 8, 12)
    before = {k: v.clone() for k, v in net.state_dict().items()}
    torch.manual_seed(3)
    smp = Sampler(sampler_args('eth', 8, 12))
    smp.set_device(dev)
    smp.train()
    opt = torch.optim.Adam(smp.parameters(), lr=1e-3)
    o, p = scenes.eth_scene(4242, n_min=9, n_max=9)
    fut = torch.from_numpy(np.ascontiguousarray(p.transpose(0, 2, 1))).to(dev)
    cfg = samplerloss.get_diversity_config('eth')
    losses = []
    for it in range(12):
        net.set_data(None, torch.from_numpy(o), torch.from_numpy(p), torch.ones(9, 8), torch.ones(9, 12))
        dec, sd, vd, _ = smp.forward(net, mean=False, eps=torch.zeros(1, 32))          # deterministic codes: z = b
        tot, ld, _ = samplerloss.compute_sampler_loss(smp.args, fut, dec, 1, None, vd, sd, cfg)
        opt.zero_grad()
        tot.backward()
        opt.step()
        losses.append(float(tot.detach()))
    assert np.isfinite(losses).all() and losses[-1] < losses[0]
    assert all(torch.equal(before[k], v) for k, v in net.state_dict().items())
    assert smp.q_c.weight.grad is None                                                  # never on the loss path (sampler.py:52)


def test_batched_scene_training_step_equals_sum_of_per_scene_steps():
    """set_scene_batch + forward() + backward() over several independent scenes in ONE step: the objective is the sum of the
    per-scene objectives (per-scene KL clamp, per-scene mean of the best-of-20 term), so loss and gradients must equal the sum
    over the reference-style one-scene-per-step runs (which are pinned against the reference / oracle above)."""
    from sttode_amd import scenes
    dev = _gpu()
    m = hip_model('eth', 8, 12)
    m.eval()
    sizes = (5, 9, 3, 17)
    rng = np.random.default_rng(44)
    sc = [scenes.eth_scene(660000 + i, n_min=n, n_max=n) for i, n in enumerate(sizes)]
    eps = [[rng.standard_normal(s).astype(np.float32) for s in ((n, 32), (n, 32), (n * 20, 32))] for n in sizes]
    tot_sum, parts_sum, grad_sum = 0.0, np.zeros(4), None
    for (o, p), e in zip(sc, eps):
        m.zero_grad()
        m.set_data(None, torch.from_numpy(o), torch.from_numpy(p), None, None)
        out = m.forward(*[torch.from_numpy(x) for x in e])
        out[0].backward()
        tot_sum += float(out[0].detach())
        parts_sum += np.array(out[1:])
        g = {k: (q.grad.detach().double().cpu() if q.grad is not None else None) for k, q in m.named_parameters()}
        grad_sum = g if grad_sum is None else {k: (None if v is None else v + g[k]) for k, v in grad_sum.items()}
    past = np.concatenate([o.transpose(0, 2, 1) for o, _ in sc])
    fut = np.concatenate([p.transpose(0, 2, 1) for _, p in sc])
    ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    m.zero_grad()
    m.set_scene_batch(torch.from_numpy(past), torch.from_numpy(fut), torch.from_numpy(ptr))
    cat = [torch.from_numpy(np.concatenate([e[i] for e in eps])) for i in range(3)]
    out = m.forward(*cat)
    out[0].backward()
    np.testing.assert_allclose(float(out[0].detach()), tot_sum, rtol=2e-5)
    np.testing.assert_allclose(np.array(out[1:]), parts_sum, rtol=2e-5)
    got = {k: (q.grad.detach().cpu() if q.grad is not None else None) for k, q in m.named_parameters()}
    _compare_grads(got, grad_sum, rtol=2e-4)
    m.zero_grad()
    with torch.no_grad():                                       # the value path agrees on the batched objective
        v = m.forward(*cat)
    np.testing.assert_allclose([float(v[0])] + list(v[1:]), [tot_sum] + list(parts_sum), rtol=1e-4)


@pytest.mark.parametrize('scenes_csr', [False, True])
def test_fused_objective_kernel_vs_the_three_loss_entry_points(scenes_csr):
    """sttode_loss_objective (all four terms of model/STTODE.py:372-395 + every gradient for ONE decoder pass over 1 + K samples per
    agent) against sttode_loss_sqerr / _kl / _diverse on the corresponding slices, with and without a scene CSR, and against a
    float64 numpy evaluation of the same formulas."""
    from sttode_amd import capi
    dev = _gpu()
    rng = np.random.default_rng(11)
    n, K, D, Dp, zd = 37, 20, 24, 16, 32
    K1 = K + 1
    pred = rng.standard_normal((n, K1, D)).astype(np.float32)
    rec = rng.standard_normal((n, K1, Dp)).astype(np.float32)
    fut = rng.standard_normal((n, D)).astype(np.float32)
    past = rng.standard_normal((n, Dp)).astype(np.float32)
    qzp = (0.3 * rng.standard_normal((n, 2 * zd))).astype(np.float32)
    ptr = np.array([0, 5, 6, 20, 37], np.int32)
    ags = np.repeat(np.arange(4), np.diff(ptr)).astype(np.int32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    P, R, F, PA, Q = t(pred), t(rec), t(fut), t(past), t(qzp)
    sp, ag, S = (t(ptr), t(ags), 4) if scenes_csr else (None, None, 0)
    out = torch.zeros(5, device=dev)
    dpred, drec, dq = torch.empty_like(P), torch.empty_like(R), torch.empty_like(Q)
    scratch = torch.empty(1 << 16, device=dev)
    sm, sr, min_clip = 1.0 / 12, 1.0 / 8, 2.0
    capi.call('sttode_loss_objective', P, R, F, PA, Q, sp, ag, S, n, K1, D, Dp, zd, sm, sr, float(n), min_clip, out, dpred, drec, dq,
              scratch, scratch.numel(), capi.stream_ptr())
    # the three stand-alone entry points on the slices
    ref = torch.zeros(4, device=dev)
    p0, r0, pk = P[:, 0].contiguous(), R[:, 0].contiguous(), P[:, 1:].contiguous()
    g0, g1, gq, gk = torch.empty_like(p0), torch.empty_like(r0), torch.empty_like(Q), torch.empty_like(pk)
    capi.call('sttode_loss_sqerr', p0, F, n * D, sm, ref[0:], g0, capi.stream_ptr())
    capi.call('sttode_loss_sqerr', r0, PA, n * Dp, sr, ref[1:], g1, capi.stream_ptr())
    capi.call('sttode_loss_kl', Q, sp, S, n, zd, float(n), min_clip, ref[2:], gq, scratch, capi.stream_ptr())
    capi.call('sttode_loss_diverse', pk, F, sp, ag, n, K, D, ref[3:], gk, scratch, capi.stream_ptr())
    o, r = out.cpu().numpy(), ref.cpu().numpy()
    np.testing.assert_allclose(o[:4], r, rtol=2e-6)
    np.testing.assert_allclose(o[4], r.sum(), rtol=2e-6)
    assert torch.equal(dpred[:, 0], g0) and torch.equal(drec[:, 0], g1) and torch.equal(dq, gq) and torch.equal(dpred[:, 1:], gk)
    assert float(drec[:, 1:].abs().max()) == 0.0
    # float64 yardstick of the best-of-K term
    d2 = ((fut[:, None, :].astype(np.float64) - pred[:, 1:].astype(np.float64)) ** 2).sum(-1).min(1)
    w = 1.0 / np.diff(ptr)[ags] if scenes_csr else np.full(n, 1.0 / n)
    np.testing.assert_allclose(o[3], (d2 * w).sum(), rtol=1e-5)
    np.testing.assert_allclose(o[0], ((pred[:, 0].astype(np.float64) - fut) ** 2).sum() * sm, rtol=1e-5)


def test_release_native_rebuilds_the_pipeline_with_identical_results():
    """STTODENet.release_native() drops the native pipeline handle, packed weights and workspaces; the next call rebuilds them and gives
    the same bits (bench.py releases a finished leg's buffers before the next leg)."""
    from sttode_amd import scenes
    m = hip_model('eth', 8, 12)
    sb = scenes.make_scene_batch(range(40, 52), 'eth')
    z = torch.from_numpy(scenes.latents(5, sb.n_agents))
    m.set_scene_batch(sb.past, sb.future, sb.scene_ptr)
    a = m.inference(None, z=z).cpu().numpy()
    m.release_native()
    assert m._native is None
    m.set_scene_batch(sb.past, sb.future, sb.scene_ptr)
    b = m.inference(None, z=z).cpu().numpy()
    assert np.array_equal(a, b)


def test_fused_trunk_forward_writes_the_layer_by_layer_tape(golden):
    """sttode_ttrunk_fwd (a trunk's forward with its tape in one launch, csrc/train_trunk.hip) against the layer-by-layer path
    (Engine.trunk_fwd: 21 launches): every tensor of both trunks' tapes, with dropout masks, to fp32 rounding."""
    from sttode_amd import training
    dev = _gpu()
    g = golden('forward_grads')
    m = hip_model('eth', 8, 12)
    rng = np.random.default_rng(9)
    n = g['eth_obs'].shape[0]
    drops = tuple(torch.from_numpy(((rng.random((n * T, 64)) < 0.9) / 0.9).astype(np.float32)).to(dev) for T in (8, 12))
    tapes = {}
    was = getattr(m, 'train_graphs', None)
    m.train_graphs = False
    try:
        for fused in (True, False):
            m.eval()                                              # no random rotation in set_data; the masks are passed explicitly
            eq, ep1, ep20 = grad_case_setup(g, 'eth', m, dev)
            eng = getattr(m, '_engine', None)
            if eng is not None:
                eng.fused_trunk = fused
            training.training_forward(m, eq, ep1, ep20, drop_past=drops[0], drop_future=drops[1])
            m._engine.fused_trunk = fused
            if eng is None:                                       # the engine is created by the first call: run it again with the flag set
                eq, ep1, ep20 = grad_case_setup(g, 'eth', m, dev)
                training.training_forward(m, eq, ep1, ep20, drop_past=drops[0], drop_future=drops[1])
            T = m._engine.tape
            tapes[fused] = {f'{tr}.{k}': v.detach().float().cpu().numpy().copy() for tr in ('tp', 'tf') for k, v in T[tr].items()
                            if isinstance(v, torch.Tensor) and k not in ('feat', 'X0', 'drop')}
            tapes[fused]['hcat'] = T['hcat'].cpu().numpy().copy()
    finally:
        m.eval()
        m._engine.fused_trunk = True
        if was is None:
            del m.train_graphs
        else:
            m.train_graphs = was
    assert set(tapes[True]) == set(tapes[False]) and len(tapes[True]) >= 30
    for k in sorted(tapes[True]):
        a, b = tapes[True][k], tapes[False][k]
        if k.endswith('h3in'):
            a, b = a[:, :67], b[:, :67]
        assert_close(a, b, rtol=2e-5, atol=2e-5, what='tape ' + k)


def test_one_scene_inference_captured_in_a_hip_graph_replays_with_new_inputs():
    """Round-4 advice: the one-launch scene form compared its hand-off flags with a host-side epoch, so a captured launch replayed with the
    epoch of its capture and its consumers did not wait.  Now the flag words are zero between launches (sttode_workspace_init once, the
    launch's last workgroup afterwards): inference() of one scene captured into a hipGraph replays correctly with changed inputs, many times."""
    from sttode_amd import scenes
    m = hip_model('eth', 8, 12)
    scs = [scenes.eth_scene(9100 + i, n_min=9, n_max=9) for i in range(4)]
    zs = [torch.from_numpy(scenes.latents(40 + i, 9)).to(m.device) for i in range(4)]
    want = []
    for (o, p), z in zip(scs, zs):
        m.set_data(None, torch.from_numpy(o), torch.from_numpy(p))
        want.append(m.inference(None, z=z).clone())
    past = torch.from_numpy(np.ascontiguousarray(scs[0][0].transpose(0, 2, 1))).to(m.device)
    fut = torch.from_numpy(np.ascontiguousarray(scs[0][1].transpose(0, 2, 1))).to(m.device)
    ptr = torch.tensor([0, 9], dtype=torch.int32, device=m.device)
    zst = zs[0].clone()
    m.set_scene_batch(past, fut, ptr)
    m.inference(None, z=zst)                                     # warm: workspace allocated and initialised, weights packed
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = m.inference(None, z=zst)
    for rep in range(3):
        for i in (1, 2, 3, 0):
            past.copy_(torch.from_numpy(np.ascontiguousarray(scs[i][0].transpose(0, 2, 1))))
            zst.copy_(zs[i])
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, want[i]), (rep, i)
    m.native().raise_if_timed_out()


def test_uninitialised_workspace_is_refused_by_the_scene_form():
    """C-ABI contract (include/sttode_hip.h sttode_workspace_init): the one-launch scene form on a workspace whose flag words were never
    initialised must not trust them -- NaN predictions, time-out word 2, sttode_check fails -- and is healthy once the workspace is initialised."""
    from sttode_amd import capi, scenes
    m = hip_model('eth', 8, 12)
    o, p = scenes.eth_scene(9200, n_min=5, n_max=5)
    m.set_data(None, torch.from_numpy(o), torch.from_numpy(p))
    z = torch.from_numpy(scenes.latents(3, 5)).to(m.device)
    good = m.inference(None, z=z).clone()
    nat = m.native()
    _, tot = nat.layout(5, 1)
    raw = torch.full((tot,), 1.0, dtype=torch.float32, device=m.device)          # every flag word "up" with arbitrary bits
    pred = torch.zeros(5, 20, 12, 2, device=m.device)
    capi.call('sttode_inference_scenes', nat.h, m._past, m._scene_ptr, 5, 1, z, raw, pred, capi.stream_ptr())
    torch.cuda.synchronize()
    assert torch.isnan(pred).all()
    with pytest.raises(capi.SttodeError, match='never initialised'):
        nat.check(raw, 5, 1)
    with pytest.raises(capi.SttodeError, match='never initialised'):
        nat.raise_if_timed_out()
    nat.init_workspace(raw, 5, 1)
    capi.call('sttode_inference_scenes', nat.h, m._past, m._scene_ptr, 5, 1, z, raw, pred, capi.stream_ptr())
    nat.check(raw, 5, 1)
    assert torch.equal(pred.permute(1, 0, 2, 3), good)


def test_refused_async_call_leaves_no_state_behind():
    """Round-4 advice: inference_async armed the native model (device latents) before its later argument checks; a check that failed left the
    request armed and the NEXT call overwrote the caller's z.  Options now travel with the call (SttodeAsyncOpts) and every check comes
    first: a refused call changes nothing."""
    from sttode_amd import capi, scenes
    m = hip_model('eth', 8, 12)
    sb = scenes.make_scene_batch(range(5200, 5261), 'eth')
    n = sb.n_agents
    nat = m.native()
    try:
        nat.set_chain(1)
        m.set_scene_batch(sb.past, sb.future, sb.scene_ptr)
        calls = m._async_calls
        with pytest.raises(ValueError):
            m.inference_async(metrics_gt=torch.zeros(3, 12, 2, device=m.device))     # z=None (device latents would be drawn) + a bad metrics_gt
        assert m._async_calls == calls                                                # no slot taken
        z = torch.from_numpy(scenes.latents(12, n)).to(m.device)
        z0 = z.clone()
        h = m.inference_async(z=z)
        out = m.wait(h).clone()
        torch.cuda.synchronize()
        assert torch.equal(z, z0)                                                     # the caller's latents were read, not overwritten
        ref = m.inference(None, z=z0)
        assert_close(out.cpu().numpy(), ref.cpu().numpy(), rtol=2e-5, atol=2e-5, what='async after a refused call vs serial')
        # the C entry point itself: options its form cannot honour -> refused before anything is enqueued
        nat.set_lagged(0)
        import ctypes
        o = capi.AsyncOpts()
        o.device_latents = 1
        buf, pred = m._async_bufs[(n, sb.n_scenes, h['slot'])][:2]
        with pytest.raises(capi.SttodeError, match='lagged'):
            capi.call('sttode_inference_scenes_async', nat.h, m._past, m._scene_ptr, n, sb.n_scenes, z, buf, pred, 0, ctypes.addressof(o), capi.stream_ptr())
        torch.cuda.synchronize()
        assert torch.equal(z, z0)
    finally:
        nat.set_lagged(3)
        nat.set_chain(-1)
        m.reset_async()


def test_horizon_metrics_kernel_vs_numpy_and_reference_golden(golden):
    """The NBA evaluation's per-horizon metric (test.py:530-551) as ONE HIP kernel: bitwise its NumPy restatement (helpers.horizon_metrics_np)
    on the same predictions, equal to the oracle's statement of the reference expression, and -- on the canned predictions the reference's
    own test_model_all was run on (tests/golden/nba_eval.npz) -- the eight figures the reference printed."""
    from helpers import horizon_metrics_np
    from oracle.metrics_ref import nba_horizon_errors
    m = hip_model('nba', 5, 10)
    g = golden('nba_eval')
    for scale in (1, 3):
        avg, dest, tot = np.zeros(11), np.zeros(11), 0
        for i in range(int(g['n_batches'])):
            pred_kn, fut = g[f'pred{i}'], g[f'fut{i}']
            B, N = fut.shape[:2]
            pred_nk = np.ascontiguousarray(pred_kn.transpose(1, 0, 2, 3))
            gt = fut.reshape(B * N, 10, 2)
            hm = m.horizon_metrics(torch.from_numpy(pred_nk).to(m.device), torch.from_numpy(gt).to(m.device), scale=float(scale)).cpu().numpy()
            assert np.array_equal(hm, horizon_metrics_np(pred_nk, gt, float(scale))), (scale, i)
            e = nba_horizon_errors(pred_kn * np.float32(scale), gt * np.float32(scale), range(1, 11))
            for h in range(1, 11):
                assert abs(hm[:, h - 1, 0].astype(np.float64).mean() - e[h][0]) < 1e-5 and abs(hm[:, h - 1, 1].astype(np.float64).mean() - e[h][1]) < 1e-5
                avg[h] += hm[:, h - 1, 0].astype(np.float64).mean() * B
                dest[h] += hm[:, h - 1, 1].astype(np.float64).mean() * B
            tot += B
        avg, dest = avg / tot, dest / tot
        printed = np.array([(avg[2] + avg[3]) / 2, avg[5], (avg[8] + avg[7]) / 2, avg[10], (dest[2] + dest[3]) / 2, dest[5], (dest[7] + dest[8]) / 2, dest[10]])
        np.testing.assert_allclose(printed, g[f'scale{scale}_printed'], rtol=5e-6)
    # long horizon, K Tf = 800 staged in LDS
    rng = np.random.default_rng(5)
    pr, gt = rng.standard_normal((37, 20, 40, 2)).astype(np.float32), rng.standard_normal((37, 40, 2)).astype(np.float32)
    hm = m.horizon_metrics(torch.from_numpy(pr).to(m.device), torch.from_numpy(gt).to(m.device), scale=2.0).cpu().numpy()
    assert np.array_equal(hm, horizon_metrics_np(pr, gt, 2.0))


@pytest.mark.parametrize('B,G', [(128, 3), (24, 5)])
def test_several_attention_groups_per_call_equal_separate_calls(B, G):
    """sttode_inference_nba_groups / SttodeAsyncOpts.nba_groups: G forward-call batches of the NBA branch in ONE call -- the attention
    stays within each batch (hyptransformerlib.py:261-265 attends over the batch dimension of one forward call) -- give, batch by batch,
    the bits of G separate inference() calls in the same form, serial and pipelined."""
    from sttode_amd import scenes
    m = hip_model('nba', 5, 10)
    N = 11
    ds = [scenes.nba_batch(8800 + g, B, N=N) for g in range(G)]
    zs = [scenes.latents(600 + g, B * N) for g in range(G)]
    nat = m.native()
    try:
        nat.set_chain(1)                                          # one form of the per-trajectory stage whatever the call's size
        sep = []
        for d, z in zip(ds, zs):
            m.set_data_nba({k: (torch.from_numpy(v) if isinstance(v, np.ndarray) else v) for k, v in d.items()})
            sep.append(m.inference(None, z=torch.from_numpy(z)).clone())
        want = torch.cat(sep, dim=1)
        data = {'past_traj': torch.from_numpy(np.stack([d['past_traj'] for d in ds])), 'future_traj': torch.from_numpy(np.stack([d['future_traj'] for d in ds]))}
        zall = torch.from_numpy(np.concatenate(zs)).to(m.device)
        m.set_data_nba(data)
        assert (m._G, m.batch_size, m.agent_num) == (G, B, N)
        got = m.inference(None, z=zall)
        assert torch.equal(got, want)
        # pipelined (lagged form when chain-sized): against separate pipelined calls, bitwise; against the serial form to fp32 rounding
        hs = []
        for d, z in zip(ds, zs):
            m.set_data_nba({k: (torch.from_numpy(v) if isinstance(v, np.ndarray) else v) for k, v in d.items()})
            hs.append(m.inference_async(z=torch.from_numpy(z)))
        sep_async = torch.cat([m.wait(h).clone() for h in hs], dim=1)
        m.set_data_nba(data)
        h = m.inference_async(z=zall)
        got_async = m.wait(h).clone()
        torch.cuda.synchronize()
        assert torch.equal(got_async, sep_async)
        assert_close(got_async.cpu().numpy(), want.cpu().numpy(), rtol=2e-5, atol=2e-5, what='groups, pipelined vs serial')
    finally:
        nat.set_chain(-1)
        m.reset_async()


def test_pipelined_nba_evaluation_equals_the_serial_loop_and_the_oracle():
    """evaluate.eval_nba (test.py:495-552): the pipelined flow -- several loader batches per call, inference_async, the horizon metric as a
    HIP kernel on the call's stream -- returns the serial loop's values (one inference() per batch, torch ops) and the oracle's on the same latents."""
    from oracle.metrics_ref import nba_horizon_errors
    from sttode_amd import evaluate, scenes
    m = hip_model('nba', 5, 10)
    N, K = 11, 20
    sizes = [128, 128, 128, 128, 128, 40]
    loader = []
    for i, B in enumerate(sizes):
        d = scenes.nba_batch(9900 + i, B, N=N)
        loader.append({'past_traj': torch.from_numpy(d['past_traj']), 'future_traj': torch.from_numpy(d['future_traj'])})
    zall = scenes.latents(77, sum(sizes) * N)

    def make_zfn():
        pos = [0]

        def z_fn(rows):
            z = torch.from_numpy(zall[pos[0]:pos[0] + rows]).to(m.device)
            pos[0] += rows
            return z
        return z_fn
    serial = evaluate.eval_nba(m, loader, traj_scale=2.0, z_fn=make_zfn(), pipelined=False)
    piped = evaluate.eval_nba(m, loader, traj_scale=2.0, z_fn=make_zfn(), groups_per_call=2)
    piped_all = evaluate.eval_nba(m, loader, traj_scale=2.0, z_fn=make_zfn(), groups_per_call=16)
    for h in range(1, 11):
        for a, b in ((serial[h], piped[h]), (serial[h], piped_all[h])):
            assert abs(a[0] - b[0]) < 2e-5 * (1 + abs(a[0])) and abs(a[1] - b[1]) < 2e-5 * (1 + abs(a[1])), (h, a, b)
    # the oracle on the first batch with the same latents: the metric of that batch alone
    ora = oracle_model('nba', 5, 10)
    with torch.no_grad():
        ora.set_data_nba(loader[0])
        ref = ora.inference(loader[0], z=torch.from_numpy(zall[:128 * N * K])).numpy()
    one = evaluate.eval_nba(m, loader[:1], traj_scale=2.0, z_fn=make_zfn())
    e = nba_horizon_errors(ref * 2.0, loader[0]['future_traj'].numpy().reshape(-1, 10, 2) * 2.0, range(1, 11))
    for h in range(1, 11):
        assert abs(one[h][0] - e[h][0]) < 1e-4 and abs(one[h][1] - e[h][1]) < 1e-4, (h, one[h], e[h])


def test_bench_default_line_rehearsed_at_world_two_on_one_gpu():
    """Every multi-rank branch of bench.py with HIP kernels, once: the WHOLE --full line at world size 2 -- headline, the four legs, `train`
    with parallel.average_gradients, the gather leg (futures all-gathered on a communication stream, counts exchanged once, `check: ok`) --
    as two ranks that share cuda:0 with the collectives under gloo (hidden flag --dist-backend gloo; the round-4 review: no N > 1 path of
    bench.py had ever executed with kernels).  A rehearsal of the code path, not a scaling measurement."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY='0')
    env.pop('WORLD_SIZE', None)
    p = subprocess.run([sys.executable, os.path.join(root, 'bench.py'), '--gpus', '2', '--dist-backend', 'gloo', '--full', '--steps', '6', '--warmup', '2',
                        '--scenes', '128', '--leg-steps', '6', '--train-steps', '12', '--train-scenes', '6', '--no-exploratory'],
                       capture_output=True, text=True, timeout=900, env=env)
    assert p.returncode == 0, p.stderr[-3000:]
    line = [l for l in p.stdout.splitlines() if l.startswith('{')][-1]
    d = json.loads(line)
    assert d['n_gpus'] == 2 and d['dist_backend'] == 'gloo' and d['rccl_ranks'] == 0 and d['scaling'] == 'weak'
    assert d['value'] > 0 and d['steps'] == 6 and d['ms_per_step'] > 0
    g = d['gather']
    assert g['check'] == 'ok' and g['ranks'] == 2 and len(g['agents_per_rank']) == 2 and g['gathered_rows'] == sum(g['agents_per_rank'])
    assert d['value_incl_gather'] > 0
    assert set(d['configs']) == {'ucy_2048', 'sdd_1024', 'nba_128', 'nba_long_4096'} and all(v['value'] > 0 for v in d['configs'].values())
    assert d['train']['steps_per_s'] > 0 and 'all-reduce' in d['train']['config']['parallelism']
    assert 'cpu_baseline' not in d                                # rank 0 at N = 1 only


def _dims_model(tag, dataset):
    from helpers import dims_case_inputs, dims_case_weights
    from sttode_amd import STTODENet
    from sttode_amd.weights import to_torch_state_dict
    a, inputs, z, eps = dims_case_inputs(tag, dataset)
    m = STTODENet(a, _gpu()).eval()
    m.load_state_dict(to_torch_state_dict(dims_case_weights(a)), strict=True)
    return m, a, inputs, z, eps


def _dims_set(m, dataset, inputs):
    if dataset == 'eth':
        m.set_data(None, torch.from_numpy(inputs[0]), torch.from_numpy(inputs[1]))
        return None
    data = {k: (torch.from_numpy(v) if isinstance(v, np.ndarray) else v) for k, v in inputs.items()}
    m.set_data_nba(data)
    return data


@pytest.mark.parametrize('tag', ['tf28', 'tf36_tp8', 'tp20', 'tf60', 'nd1', 'nd3', 'zd16', 'zd64', 'hd32', 'hd128', 'mix'])
def test_non_default_hyperparameters_vs_reference_golden(golden, tag):
    """What the reference's CLI accepts (train.py:25-26,37-40 --past_length / --future_length / --zdim / --hidden_dim / --num_decompose)
    through the DEFAULT path of STTODENet -- constructor, load_state_dict(strict=True) of a state_dict with the reference's names and
    shapes for those flags, set_data / set_data_nba, inference(): one ETH scene and one NBA batch per value against the imported
    reference (tests/golden/dims.npz) at rtol 1e-4 + atol 1e-4.  tf28 / tf36_tp8 run on the fused forms (the (TPX, NOY) pairs rounds 1-4
    did not instantiate), the others on the generic form (sttode_amd/generic.py)."""
    from sttode_amd import generic
    g = golden('dims')
    for dataset in ('eth', 'nba'):
        m, a, inputs, z, _ = _dims_model(tag, dataset)
        assert m._generic == (tag not in ('tf28', 'tf36_tp8')) and generic.unsupported_reason(a) is None
        data = _dims_set(m, dataset, inputs)
        out = m.inference(data, z=torch.from_numpy(z))
        k = f'{tag}_{dataset}_'
        assert_close(m.past_feature.cpu().numpy(), g[k + 'past_feature'], what=k + 'past_feature')
        assert_close(out.cpu().numpy(), g[k + 'out'], what=k + 'inference')
        if not m._generic:                                        # the fused forms of those shapes: chain launch (forced) and pipelined
            nat = m.native()
            try:
                nat.set_chain(1)
                _dims_set(m, dataset, inputs)
                assert_close(m.inference(data, z=torch.from_numpy(z)).cpu().numpy(), g[k + 'out'], what=k + 'chain launch')
                _dims_set(m, dataset, inputs)
                h = m.inference_async(z=torch.from_numpy(z))
                assert_close(m.wait(h).cpu().numpy(), g[k + 'out'], what=k + 'pipelined')
            finally:
                nat.set_chain(-1)
                m.reset_async()


def _dims_oracle_steps(a, dataset, inputs, eps):
    """The oracle's step on one dims case in fp32 and in float64 -> {double: (name -> gradient | None, the five values)}."""
    from test_oracle_golden import _oracle_step
    return {dbl: _oracle_step(a, dataset, inputs, eps, dbl) for dbl in (False, True)}


def _dims_grads_vs_float64(got, g32, g64, what):
    """Every parameter gradient of a step at non-default widths (``got``: name -> tensor | None) against the float64 autograd of the oracle
    (``g64``), measured by the fp32 autograd of the same graph (``g32``); the per-parameter table goes through _dump_grad_table.
    -> (the number of parameters compared: those the float64 oracle gives a gradient, the worst err_hip / max|g64|)."""
    checked, bad, rows = 0, [], []
    for name, gr in got.items():
        g64p = g64[name]
        if g64p is None:
            assert gr is None or not bool(gr.any()), name
            continue
        assert gr is not None, name
        g64n = g64p.numpy()
        err_hip = np.abs(gr.cpu().numpy().astype(np.float64) - g64n).max()
        err_f32 = np.abs(g32[name].numpy().astype(np.float64) - g64n).max()
        rows.append((name, err_hip, err_f32, float(np.abs(g64n).max()), err_hip / (float(np.abs(g64n).max()) + 1e-30)))
        # float64 yardstick as in the default-width tests, with 6x instead of 2x the fp32 autograd's own error: at these widths the random-recipe
        # weights give activations of 1e3 and block-1 inputs x_true - x_hat_0 that cancel, so the fp32 autograd itself is off by 2e-4 of
        # max|g| on the blocks' conv / GRU gradients (profiles/r05/grad_tables/dims_*.txt) and two summation orders differ by a few times that
        # (floor 5e-4 of max|g| for the same rows: they sit at 2e-4 .. 4.3e-4 whichever summation order the trunk takes)
        if not err_hip <= max(6 * err_f32, 5e-4 * np.abs(g64n).max()) + 1e-12:
            bad.append((name, err_hip, err_f32, float(np.abs(g64n).max())))
        checked += 1
    _dump_grad_table(what, None, text=''.join('%-80s err_hip %.3e  err_fp32_autograd %.3e  max|g| %.3e  rel %.2e\n' % row for row in rows))
    assert not bad, (what, bad[:6])
    assert checked == sum(v is not None for v in g64.values())
    return checked, max(row[4] for row in rows)


def _dims_training_step(m, dataset, inputs, eps, ref_losses, what, ora, no_grad_too=True):
    """One forward() + backward() of ``m`` on a dims case: the five values against ``ref_losses`` at rtol 1e-4, every parameter gradient
    against the oracle's float64 autograd (``ora`` = _dims_oracle_steps(...)), then the no-grad forward() against the same five values.
    -> (the five values, name -> gradient, the number of parameters compared, the worst err_hip / max|g64|)."""
    eq, ep, e20 = (torch.from_numpy(e) for e in eps)
    _dims_set(m, dataset, inputs)
    m.zero_grad()
    vals = m.forward(eps_q=eq, eps_p=ep, eps20=e20)
    losses = [float(vals[0].detach())] + list(vals[1:])
    np.testing.assert_allclose(losses, ref_losses, rtol=1e-4)
    vals[0].backward()
    got = {name: (p.grad.detach().clone() if p.grad is not None else None) for name, p in m.named_parameters()}
    checked, worst = _dims_grads_vs_float64(got, ora[False][0], ora[True][0], what)
    if no_grad_too:                                               # no-grad forward(): the same values
        with torch.no_grad():
            _dims_set(m, dataset, inputs)
            v2 = m.forward(eps_q=eq, eps_p=ep, eps20=e20)
        np.testing.assert_allclose([float(v2[0])] + list(v2[1:]), ref_losses, rtol=1e-4)
    return losses, got, checked, worst


@pytest.mark.parametrize('tag', ['nd3', 'zd16', 'hd32', 'hd128', 'tf28'])
def test_non_default_hyperparameters_training_step_vs_reference(golden, tag):
    """forward() + backward() with non-default --num_decompose / --zdim / --hidden_dim / --future_length: the five loss values against the
    imported reference's, every parameter gradient against the float64 autograd of the oracle (the yardstick of the default-width tests).
    (The other accepted widths: tests/test_generic_training_gpu.py, on the same comparison.)"""
    g = golden('dims')
    for dataset in ('eth', 'nba'):
        m, a, inputs, z, eps = _dims_model(tag, dataset)
        k = f'{tag}_{dataset}_'
        checked = _dims_training_step(m, dataset, inputs, eps, g[k + 'losses'], f'dims_{k}', _dims_oracle_steps(a, dataset, inputs, eps))[2]
        assert checked > 80


def test_generic_form_staged_api_and_evaluation_loops():
    """The staged API (encode_history / fu_encoder / decoder_future_0 / _1: what sampler.py:36-70 drives) and the evaluation loops on a model
    with non-default widths: against the oracle on the same noises."""
    from helpers import dims_case_inputs
    from test_oracle_golden import _dims_set_data, _oracle_for
    m, a, inputs, z, (eq, ep, e20) = _dims_model('mix', 'nba')
    ora = _oracle_for(a)
    data = _dims_set(m, 'nba', inputs)
    from oracle.sttode_ref import Normal
    with torch.no_grad():
        _dims_set_data(ora, 'nba', inputs)
        ora.encode_history()
        qzp = ora.future_encoder(ora.inputs_for_posterior, ora.batch_size, ora.agent_num, ora.past_feature)
        ora.decoder_future_0(Normal(params=qzp).rsample(torch.from_numpy(eq)), torch.from_numpy(e20))
        ora.decoder_future_1(torch.from_numpy(e20))
    m.encode_history()
    m.fu_encoder(eps_q=torch.from_numpy(eq), eps_p=torch.from_numpy(ep))
    m.decoder_future_0(m.qz_sampled, eps20=torch.from_numpy(e20))
    m.decoder_future_1(torch.from_numpy(e20))
    assert_close(m.past_feature.cpu().numpy(), ora.past_feature.numpy(), what='past_feature')
    assert_close(m.qz_param.cpu().numpy(), qzp.numpy(), what='qz_param')
    # (the posterior decode of this random-recipe model reaches |values| of 2e3: the absolute floor scales with the output's magnitude)
    for got, ref, what in ((m.pred_traj, ora.pred_traj, 'pred_traj'), (m.recover_traj, ora.recover_traj, 'recover_traj'),
                           (m.diverse_pred_traj, ora.diverse_pred_traj, 'diverse_pred_traj')):
        r = ref.numpy().reshape(got.shape)
        assert_close(got.cpu().numpy(), r, atol=1e-4 * max(1.0, float(np.abs(r).max())), what=what)
    # the pipelined API degrades to serial calls, the callers keep working
    h = m.inference_async(z=torch.from_numpy(z))
    ade, fde = m.best_of_k_async(h)
    with torch.no_grad():
        ref = ora.inference(data, z=torch.from_numpy(z)).numpy()
    assert_close(m.wait(h).cpu().numpy(), ref, what='generic inference_async')
    from oracle.metrics_ref import best_of_k_ade_fde
    ra, rf = best_of_k_ade_fde(ref.transpose(1, 0, 2, 3), inputs['future_traj'].reshape(-1, a.future_length, 2))
    assert_close(ade.cpu().numpy(), ra, what='ade')
    assert_close(fde.cpu().numpy(), rf, what='fde')


def test_unsupported_arguments_are_refused_in_one_place():
    from sttode_amd import STTODENet, generic
    for over, frag in ((dict(hidden_dim=48), 'hidden_dim'), (dict(zdim=30), 'zdim'), (dict(num_decompose=0), 'num_decompose'),
                       (dict(past_length=1), 'past_length'), (dict(hyper_scales=[5]), 'hyper_scales'), (dict(learn_prior=True), 'learn_prior')):
        a = make_args('eth', 8, 12)
        for k_, v in over.items():
            setattr(a, k_, v)
        assert frag in generic.unsupported_reason(a)
        with pytest.raises(NotImplementedError, match=frag):
            STTODENet(a, _gpu())


def test_hip_adam_is_torch_adam_in_one_launch():
    """sttode_amd.optim.Adam: torch.optim.Adam's update (train.py:122,66,87) for all parameters as ONE HIP launch.  Against torch's own
    single-tensor implementation on tensors of assorted sizes (odd lengths, one element, a 1 M-element matrix), with and without weight
    decay, a changing learning rate (StepLR) and gradients that arrive as views of one flat buffer: parameters and both moments agree to fp32
    rounding after 6 steps; the state_dicts are interchangeable with torch's class."""
    from sttode_amd.optim import Adam
    dev = _gpu()
    torch.manual_seed(5)
    shapes = [(7,), (1,), (33, 5), (1024, 1024), (3, 3, 3), (4096,), (1025,)]
    for wd in (0.0, 0.01):
        ps_a = [torch.nn.Parameter(torch.randn(s, device=dev)) for s in shapes]
        ps_b = [torch.nn.Parameter(p.detach().clone()) for p in ps_a]
        oa = Adam(ps_a, lr=3e-3, weight_decay=wd)
        ob = torch.optim.Adam(ps_b, lr=3e-3, weight_decay=wd, foreach=False)
        sa = torch.optim.lr_scheduler.StepLR(oa, step_size=2, gamma=0.5)
        sb = torch.optim.lr_scheduler.StepLR(ob, step_size=2, gamma=0.5)
        tot = sum(((p.numel() + 3) // 4) * 4 for p in ps_a)
        for it in range(6):
            flat = torch.randn(tot, device=dev)                   # this step's gradients: views of ONE fresh flat buffer (the engine's layout)
            off = 0
            for pa, pb in zip(ps_a, ps_b):
                g = flat[off: off + pa.numel()].view(pa.shape)
                pa.grad, pb.grad = g, g.clone()
                off += ((pa.numel() + 3) // 4) * 4
            oa.step(); ob.step(); sa.step(); sb.step()
        for pa, pb in zip(ps_a, ps_b):
            assert_close(pa.detach().cpu().numpy(), pb.detach().cpu().numpy(), rtol=2e-6, atol=2e-7, what='parameter')
            for k in ('exp_avg', 'exp_avg_sq'):
                assert_close(oa.state[pa][k].cpu().numpy(), ob.state[pb][k].cpu().numpy(), rtol=2e-6, atol=1e-7, what=k)
        oa.state_dict()                                           # (writes the per-parameter step tensors of torch's state layout)
        assert all(float(oa.state[pa]['step']) == float(ob.state[pb]['step']) == 6 for pa, pb in zip(ps_a, ps_b))
        ob2 = torch.optim.Adam(ps_b, lr=1.0, foreach=False)
        ob2.load_state_dict(oa.state_dict())                      # torch's class takes our state ...
        oa2 = Adam(ps_a, lr=1.0)
        oa2.load_state_dict(ob.state_dict())                      # ... and ours takes torch's
        assert oa2.param_groups[0]['lr'] == ob.param_groups[0]['lr']
    # options the kernel does not implement take torch's own step
    p = torch.nn.Parameter(torch.randn(10, device=dev))
    o = Adam([p], lr=1e-2, amsgrad=True)
    p.grad = torch.randn(10, device=dev)
    o.step()
    assert 'max_exp_avg_sq' in o.state[p]


def test_training_loop_with_hip_adam_equals_torch_fused_adam():
    """The train.py:72-95 loop (set_data, forward, zero_grad, backward, step) over a few scenes with sttode_amd.optim.Adam against the same
    loop with torch.optim.Adam(fused=True) from the same weights and noises: the loss trajectories agree to fp32 rounding."""
    from sttode_amd import STTODENet, scenes
    from sttode_amd.optim import Adam
    from sttode_amd.weights import make_weights, to_torch_state_dict
    dev = _gpu()
    data = [scenes.eth_scene(81000 + i, n_min=5, n_max=12) for i in range(4)]
    runs = []
    for kind in ('hip', 'torch'):
        m = STTODENet(make_args('eth', 8, 12), dev).eval()
        m.load_state_dict(to_torch_state_dict(make_weights(1234)), strict=True)
        opt = Adam(m.parameters(), lr=1e-3) if kind == 'hip' else torch.optim.Adam(m.parameters(), lr=1e-3, fused=True)
        g = torch.Generator(device='cpu').manual_seed(3)
        losses = []
        for it in range(8):
            o, p = data[it % 4]
            n = o.shape[0]
            m.set_data(None, torch.from_numpy(o), torch.from_numpy(p))
            eq, ep, e20 = torch.randn(n, 32, generator=g), torch.randn(n, 32, generator=g), torch.randn(n * 20, 32, generator=g)
            tot = m.forward(eps_q=eq, eps_p=ep, eps20=e20)[0]
            opt.zero_grad()
            tot.backward()
            opt.step()
            losses.append(float(tot.detach()))
        runs.append(losses)
    np.testing.assert_allclose(runs[0], runs[1], rtol=2e-4)
    assert abs(runs[0][-1] - runs[0][0]) > 1e-3 * abs(runs[0][0])   # (the parameters did move)


def test_replayed_steps_gradients_rotate_and_accumulate_correctly(golden):
    """Graph-replayed training steps hand their gradients over as views of two persistent buffers used in turn (round 5: no 88 view
    operations per step).  (a) a step's gradients are still intact after the NEXT step ran; (b) gradient accumulation over several replayed
    steps without zero_grad (p.grad += g) gives exactly k times one step's gradient and is not corrupted by later replays; (c) the values are
    those of an eager step."""
    from sttode_amd import STTODENet
    from sttode_amd.weights import make_weights, to_torch_state_dict
    g = golden('eth_forward_losses')
    m = STTODENet(make_args('eth', 8, 12), _gpu()).eval()
    m.load_state_dict(to_torch_state_dict(make_weights(1234)), strict=True)
    n = g['obs'].shape[0]
    eps = [torch.from_numpy(np.random.default_rng(5).standard_normal(s).astype(np.float32)) for s in ((n, 32), (n, 32), (n * 20, 32))]

    def step():
        m.set_data(None, torch.from_numpy(g['obs']), torch.from_numpy(g['pred']))
        return m.forward(eps[0], eps[1], eps[2])[0]
    w = m.decoder.decompose[1].decoder_x.layers[0].weight
    m.train_graphs = False
    step().backward()
    eager = w.grad.clone()
    m.train_graphs = True
    for _ in range(3):                            # eager -> capture -> replay
        m.zero_grad()
        step().backward()
    assert torch.allclose(w.grad, eager, rtol=1e-6, atol=1e-7 * float(eager.abs().max()))
    first = w.grad                                # a view of rotating buffer A
    keep = first.clone()
    m.zero_grad()
    step().backward()                             # buffer B
    assert torch.equal(first, keep)               # (a) the previous step's gradients are intact
    # (b) accumulate over 4 replayed steps
    m.zero_grad()
    for _ in range(4):
        step().backward()
    assert torch.allclose(w.grad, 4 * keep, rtol=1e-6, atol=1e-6 * float(keep.abs().max()))
    acc = w.grad.clone()
    for p in m.parameters():
        p.grad = None if p is not w else p.grad   # keep accumulating on one parameter only
    step().backward(); step().backward()
    assert torch.allclose(w.grad, acc + 2 * keep, rtol=1e-6, atol=1e-6 * float(keep.abs().max()))


@pytest.mark.gpu
def test_published_values_reach_the_host_while_the_stream_is_still_busy():
    """sttode_publish_values / sttode_wait_value (round 5): values written by one launch are read by the host WITHOUT any stream or event
    synchronisation -- with a long queue behind the publishing launch, the wait returns while that queue is still running; a count that never
    comes times out with an error instead of hanging."""
    from sttode_amd import capi
    dev = _gpu()
    L = capi.lib()
    vals = torch.arange(5, dtype=torch.float32, device=dev) * 1.5 + 0.25
    host_vals, host_seq = torch.zeros(8).pin_memory(), torch.zeros(2, dtype=torch.int32).pin_memory()
    dev_seq = torch.zeros(2, dtype=torch.int32, device=dev)
    a = torch.randn(4096, 4096, device=dev)
    torch.cuda.synchronize()
    for k in (1, 2, 3):
        vals.add_(1.0)
        capi.call('sttode_publish_values', vals, 5, host_vals, dev_seq, host_seq, capi.stream_ptr())
        for _ in range(40):                           # ~40 x 0.9 ms of matrix products queued BEHIND the publishing launch
            a = (a @ a).clamp_(-1, 1)
        assert L.sttode_wait_value(host_seq.data_ptr(), k, 20.0) == 0
        busy = not torch.cuda.current_stream().query()
        assert host_vals[:5].tolist() == [0.25 + 1.5 * i + k for i in range(5)]
        assert busy, 'the wait outlasted the queue behind the publishing launch: it did not return early'
        torch.cuda.synchronize()
    assert int(dev_seq[0]) == 3
    assert L.sttode_wait_value(host_seq.data_ptr(), 9, 0.05) != 0 and b'did not reach' in L.sttode_last_error()
    with pytest.raises(capi.SttodeError, match='null pointer'):
        capi.call('sttode_publish_values', None, 5, host_vals, dev_seq, host_seq, capi.stream_ptr())


@pytest.mark.gpu
def test_nba_batches_are_staged_without_waiting_for_the_stream():
    """set_data_nba with the loader's pageable host tensors (train.py:61): one asynchronous copy through the pinned ring
    (sttode_stage_rows) -- the bytes of `.to(device)`, for sizes whose first array ends off a 16-byte boundary too, over more calls than the
    ring has slots, and issued while the stream is busy."""
    from sttode_amd import STTODENet, scenes
    dev = _gpu()
    m = STTODENet(make_args('nba', 5, 10), dev).eval()
    a = torch.randn(2048, 2048, device=dev)
    for i, (B, N) in enumerate([(1, 11), (3, 11), (32, 11), (7, 3), (2, 1), (128, 11), (5, 11)]):
        d = scenes.nba_batch(300 + i, B, N=N)
        data = {k: (torch.from_numpy(v) if isinstance(v, np.ndarray) else v) for k, v in d.items()}
        for _ in range(10):
            a = (a @ a).clamp_(-1, 1)
        m.set_data_nba(data)
        assert torch.equal(m._past.cpu().view(B, N, 5, 2), data['past_traj']) and torch.equal(m._future.cpu().view(B, N, 10, 2), data['future_traj'])
        assert m._past.data_ptr() % 16 == 0 and m._future.data_ptr() % 16 == 0
        m.set_data_nba({'past_traj': data['past_traj']})                      # no future: inference-only callers
        assert m._future is None and torch.equal(m._past.cpu().view(B, N, 5, 2), data['past_traj'])
    z = torch.randn(5 * 11 * 20, 32, device=dev)
    m.load_state_dict(__import__('sttode_amd.weights', fromlist=['x']).to_torch_state_dict(__import__('sttode_amd.weights', fromlist=['x']).make_weights(1234, past_length=5, future_length=10)))
    m.set_data_nba(data)
    out = m.inference(data, z=z)
    m.set_data_nba({k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in data.items()})   # device-resident inputs: the old route
    assert torch.equal(out, m.inference(data, z=z))


@pytest.mark.gpu
def test_replayed_step_returns_its_losses_before_the_backward_half_has_run(golden):
    """A replayed training step publishes its four loss values from the middle of its graph (round 5): forward() returns the same floats
    as the eager step's `.tolist()`, the train.py:61-67 loop run back to back WITHOUT any synchronisation in between moves the parameters
    exactly like the same loop with a device synchronisation after every call, and total.item() still is the step's total."""
    from sttode_amd import STTODENet, scenes
    from sttode_amd.optim import Adam
    from sttode_amd.weights import make_weights, to_torch_state_dict
    dev = _gpu()
    d = scenes.nba_batch(11, 16)
    data = {k: (torch.from_numpy(v) if isinstance(v, np.ndarray) else v) for k, v in d.items()}
    n = 16 * 11
    gen = torch.Generator().manual_seed(9)
    eps = [(torch.randn(n, 32, generator=gen), torch.randn(n, 32, generator=gen), torch.randn(n * 20, 32, generator=gen)) for _ in range(6)]
    runs = []
    for sync in (True, False):
        m = STTODENet(make_args('nba', 5, 10), dev).eval()
        m.load_state_dict(to_torch_state_dict(make_weights(1234, past_length=5, future_length=10)), strict=True)
        opt = Adam(m.parameters(), lr=1e-3)
        vals = []
        for it in range(6):
            m.set_data_nba(data)
            out = m.forward(*eps[it])
            if sync:
                torch.cuda.synchronize()
            opt.zero_grad(); out[0].backward(); opt.step()
            if sync:
                torch.cuda.synchronize()
            vals.append((out[0], out[1:]))
        torch.cuda.synchronize()
        for tot, four in vals:
            assert all(isinstance(v, float) for v in four)
            assert abs(float(tot) - sum(four)) <= 1e-5 * abs(float(tot))
        runs.append(([four for _, four in vals], [float(t) for t, _ in vals], [p.detach().clone() for p in m.parameters()]))
    assert runs[0][0] == runs[1][0] and runs[0][1] == runs[1][1]                  # replayed steps are deterministic: the same floats
    assert all(torch.equal(a, b) for a, b in zip(runs[0][2], runs[1][2]))
    # ... and a replayed step's values are the eager step's (same weights: no optimizer in between)
    m = STTODENet(make_args('nba', 5, 10), dev).eval()
    m.load_state_dict(to_torch_state_dict(make_weights(1234, past_length=5, future_length=10)), strict=True)
    got = []
    for _ in range(3):                                                            # eager -> capture + replay -> replay
        m.set_data_nba(data)
        got.append(m.forward(*eps[0])[1:])
    assert got[1] == got[2]
    np.testing.assert_allclose(got[2], got[0], rtol=1e-5)


@pytest.mark.gpu
@pytest.mark.parametrize('mode', ['train', 'eval'])
def test_replayed_step_draws_its_own_noise_like_the_eager_step(mode):
    """The random inputs nobody passes in (posterior / prior noise, the two dropout masks in train mode) are drawn INSIDE the replayed graph
    (round 5; torch's generator is graph-safe) by the calls of the eager step in the same order: under one torch.manual_seed a run of
    replayed steps sees the numbers the eager run sees -- same loss values step by step -- and two replays never see the same noise."""
    from sttode_amd import STTODENet, scenes
    from sttode_amd.weights import make_weights, to_torch_state_dict
    dev = _gpu()
    o, p = scenes.eth_scene(4242, n_min=9, n_max=9)
    o, p = torch.from_numpy(o), torch.from_numpy(p)
    runs = []
    for graphs in (False, True):
        m = STTODENet(make_args('eth', 8, 12), dev)
        m.load_state_dict(to_torch_state_dict(make_weights(1234)), strict=True)
        m.train() if mode == 'train' else m.eval()
        m.train_graphs = graphs
        torch.manual_seed(77); np.random.seed(77)
        vals = []
        for it in range(5):
            m.set_data(None, o, p, theta=0.3 * it)
            vals.append(m.forward()[1:])
        runs.append(vals)
    for a, b in zip(*runs):
        np.testing.assert_allclose(b, a, rtol=2e-5)
    assert len({v[0] for v in runs[1]}) == 5                        # every replay drew fresh noise


@pytest.mark.gpu
@pytest.mark.parametrize('L,Nb,hd', [(3, 4, 8), (5, 11, 8), (16, 11, 8), (32, 11, 8), (32, 3, 4), (24, 5, 16), (64, 2, 8), (128, 1, 8)])
def test_attention_backward_kernels_vs_autograd(L, Nb, hd):
    """sttode_mhgsa_attn_bwd against torch autograd (float64) of the same op -- out_i = sum_j softmax_j(-acos(clamp(k^_i . q^_j))) v_j per
    (slot, head), scores untransposed (hyptransformerlib.py:261-265) -- for both of its forms: one thread per row (L < 4 or the L x L
    terms beyond the LDS) and the pair-parallel form of round 5 (4 <= L <= ~100)."""
    from sttode_amd import capi
    dev = _gpu()
    DM = 8 * hd
    g = torch.Generator().manual_seed(100 * L + hd)
    qkv = torch.randn(L * Nb, 3 * DM, generator=g)
    dO = torch.randn(L * Nb, DM, generator=g)
    x = qkv.double().requires_grad_(True)
    q, k, v = (x[:, i * DM:(i + 1) * DM].view(L, Nb, 8, hd) for i in range(3))
    qn, kn = q / q.norm(dim=-1, keepdim=True), k / k.norm(dim=-1, keepdim=True)
    dots = torch.einsum('inhd,jnhd->nhij', kn, qn).clamp(-1 + 1e-4, 1 - 1e-4)          # [slot, head, key row i, query column j]
    P = torch.softmax(-torch.acos(dots), dim=-1)
    out = torch.einsum('nhij,jnhd->inhd', P, v).reshape(L * Nb, DM)
    out.backward(dO.double())
    got = torch.empty(L * Nb, 3 * DM, device=dev)
    capi.call('sttode_mhgsa_attn_bwd', qkv.to(dev), dO.to(dev), got, L, Nb, hd, capi.stream_ptr())
    ref = x.grad
    err = (got.cpu().double() - ref).abs().max().item()
    assert err <= 2e-5 * (1 + ref.abs().max().item()), (err, ref.abs().max().item())


@pytest.mark.gpu
@pytest.mark.parametrize('ds', ['eth', 'nba', 'nba32'])
def test_live_column_backward_equals_the_dense_backward(ds):
    """Round 5: the decoder's backward pass runs over the two trajectory columns per agent that carry a gradient (sample 0 and the sample the
    min over K of loss_diverse selects, model/STTODE.py:390-395), and the first block's conv + GRU once per agent (x_hat = 0 there).  Both are
    the DENSE backward over all 21 columns per agent with the exact zeros left out: same loss values, every parameter gradient equal to
    summation-order rounding -- on the same step, same noise, with the two switches off and on."""
    from sttode_amd import STTODENet, scenes, training
    from sttode_amd.weights import make_weights, to_torch_state_dict
    dev = _gpu()
    if ds == 'eth':
        a, n = make_args('eth', 8, 12), 9
        o, p = scenes.eth_scene(977, n_min=n, n_max=n)
        w = make_weights(1234)
    else:
        B = 32 if ds == 'nba32' else 8                            # 32 x 11: the dense backward's 7 392 and the live one's 704 columns both on the LDS-tiled GEMMs
        a, n = make_args('nba', 5, 10), B * 11
        d = scenes.nba_batch(41, B)
        data = {k: (torch.from_numpy(v) if isinstance(v, np.ndarray) else v) for k, v in d.items()}
        w = make_weights(1234, past_length=5, future_length=10)
    gen = torch.Generator().manual_seed(5)
    eps = (torch.randn(n, 32, generator=gen), torch.randn(n, 32, generator=gen), torch.randn(n * 20, 32, generator=gen))
    res = {}
    saved = training._LIVE_COLUMNS, training._AGENT_GRU
    try:
        for live, agent in ((False, False), (True, False), (True, True)):
            training._LIVE_COLUMNS, training._AGENT_GRU = live, agent
            m = STTODENet(a, dev).eval()
            m.load_state_dict(to_torch_state_dict(w), strict=True)
            m.train_graphs = False
            if ds == 'eth':
                m.set_data(None, torch.from_numpy(o), torch.from_numpy(p))
            else:
                m.set_data_nba(data)
            out = m.forward(*eps)
            out[0].backward()
            res[(live, agent)] = (out[1:], {k: v.grad.clone() for k, v in m.named_parameters() if v.grad is not None})
    finally:
        training._LIVE_COLUMNS, training._AGENT_GRU = saved
    dense = res[(False, False)]
    for key in ((True, False), (True, True)):
        vals, grads = res[key]
        np.testing.assert_allclose(vals, dense[0], rtol=1e-6)
        assert set(grads) == set(dense[1]) and len(grads) > 80
        for k, g in grads.items():
            ref = dense[1][k]
            assert float((g - ref).abs().max()) <= 2e-5 * float(ref.abs().max()) + 1e-12, (key, k, float((g - ref).abs().max()), float(ref.abs().max()))
