"""Training through a non-default encoder integrator (net.ode_method / net.ode_steps): forward() with autograd and backward() run the
stage program of sttode_amd/odestages.py on the training kernels (Engine._ode_*, csrc/train_ode.hip) for BOTH encoder trunks.

Yardstick: the oracle model with both trunks' ODE block integrated by oracle.sttode_ref.ode_integrate_ref, evaluated by torch autograd in
fp32 and in float64.  The reference only ever takes one Euler step (ode_demo.py:186-190), so these integrators have no reference pin:
they are held to the oracle (parity unpinned by construction)."""
import numpy as np
import pytest
import torch

from helpers import grad_case_setup, make_args

pytestmark = pytest.mark.gpu

CASES = [('euler', 3), ('rk4', 1), ('rk4', 2), ('rk4_classic', 2)]
DATA = {'eth': ('eth', 8, 12), 'nba': ('nba', 5, 10)}


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    return torch.device('cuda:0')


def _hip(dataset, Tp, Tf, method, steps, seed=1234):
    from sttode_amd import STTODENet
    from sttode_amd.weights import make_weights, to_torch_state_dict
    m = STTODENet(make_args(dataset, Tp, Tf), _gpu()).eval()
    m.load_state_dict(to_torch_state_dict(make_weights(seed, past_length=Tp, future_length=Tf)), strict=True)
    m.ode_method, m.ode_steps = method, steps
    return m


def _oracle(dataset, Tp, Tf, method, steps, double, seed=1234):
    """The oracle with both encoders' ODE block integrated by ode_integrate_ref (fp32 or float64)."""
    from oracle.sttode_ref import STTODENetRef, ode_integrate_ref
    from sttode_amd.weights import make_weights, to_torch_state_dict
    m = STTODENetRef(make_args(dataset, Tp, Tf)).eval()
    m.load_state_dict(to_torch_state_dict(make_weights(seed, past_length=Tp, future_length=Tf)), strict=True)
    if double:
        m = m.double()
    for enc in (m.past_encoder, m.future_encoder):
        blk = enc.ODE_Encoder.odeblock
        blk.forward = (lambda b: lambda x: ode_integrate_ref(lambda y: b.odefunc(0.0, y), x, b.t1, method, steps))(blk)
    return m


def _oracle_run(m, setup, double, drop=None):
    """setup(model) feeds the data and returns (eps_q, eps_p1, eps_p20); -> (name -> gradient, 5 losses)."""
    m.zero_grad()
    eq, ep1, ep20 = setup(m)
    if double:
        for attr in ('inputs', 'inputs_for_posterior', 'past_traj', 'future_traj', 'cur_location', 'scene_orig'):
            setattr(m, attr, getattr(m, attr).double())
        eq, ep1, ep20 = eq.double(), ep1.double(), ep20.double()
        drop = tuple(d.double() for d in drop) if drop is not None else None
    m.past_encoder.pos_encoder.drop_mask, m.future_encoder.pos_encoder.drop_mask = drop if drop is not None else (None, None)
    prev = torch.get_default_dtype()
    try:
        torch.set_default_dtype(torch.float64 if double else torch.float32)
        vals = m.forward_loss_tensors(eq, ep1, ep20)
        vals[0].backward()
    finally:
        torch.set_default_dtype(prev)
    grads = {k: (p.grad.detach().clone() if p.grad is not None else None) for k, p in m.named_parameters()}
    return grads, [float(v.detach()) for v in vals]


def _hip_run(m, setup, drop=None, train_mode=False):
    m.zero_grad()
    eq, ep1, ep20 = setup(m)
    m.train(train_mode)
    try:
        out = m.forward(eq.to(m.device), ep1.to(m.device), ep20.to(m.device), *(drop if drop is not None else (None, None)))
        out[0].backward()
    finally:
        m.eval()
    grads = {k: (p.grad.detach().cpu().clone() if p.grad is not None else None) for k, p in m.named_parameters()}
    m.zero_grad()
    return grads, [float(out[0].detach())] + [float(v) for v in out[1:]]


def _yardstick(got, g64, g32, what, factor=4.0, floor=5e-4):
    """Per parameter, in units of its max |g| (float64): |hip - f64| <= max(factor * |fp32 autograd - f64|, floor).  The floor: the decoder's
    block-1 GRU input weights are ill-conditioned in fp32 whatever the integrator -- the default path's HIP gradient there sits 1.3e-4 ..
    2.2e-4 of max |g| from float64 where one torch fp32 sample sits at 4e-5 (test_gpu_parity.py's dropout-mask test notes the same rows)."""
    worst = []
    for name, r64 in g64.items():
        gt = got[name]
        if r64 is None:
            assert gt is None or float(gt.abs().max()) == 0.0, name
            continue
        assert gt is not None, name
        r64 = r64.double().cpu()
        scale = float(r64.abs().max()) + 1e-300
        e_hip = float((gt.double() - r64).abs().max()) / scale
        e_ref = float((g32[name].double().cpu() - r64).abs().max()) / scale
        assert np.isfinite(e_hip), (what, name)
        worst.append((e_hip / max(factor * e_ref, floor), name, e_hip, e_ref))
    worst.sort(reverse=True)
    r, name, e_hip, e_ref = worst[0]
    assert r <= 1.0, f'{what}: {name} off by {e_hip:.3e} of its max |g| (fp32 autograd: {e_ref:.3e})'
    return worst


def _golden_setup(golden, tag):
    g = golden('forward_grads')
    return lambda m: grad_case_setup(g, tag, m)


def _check_vs_oracle(m, setup, dataset, Tp, Tf, method, steps, what, drop=None, train_mode=False, factor=4.0):
    grads, losses = _hip_run(m, setup, drop=tuple(d.to(m.device) for d in drop) if drop is not None else None, train_mode=train_mode)
    g64, l64 = _oracle_run(_oracle(dataset, Tp, Tf, method, steps, True), setup, True, drop=drop)
    g32, _ = _oracle_run(_oracle(dataset, Tp, Tf, method, steps, False), setup, False, drop=drop)
    np.testing.assert_allclose(losses, l64, rtol=1e-4, err_msg=what)
    _yardstick(grads, g64, g32, what, factor=factor)
    return grads, losses


@pytest.mark.parametrize('tag', ['eth', 'nba'])
@pytest.mark.parametrize('method,steps', CASES)
def test_gradients_and_losses_vs_float64_oracle(golden, tag, method, steps):
    """Losses and every live parameter's gradient of forward() + backward() under the integrator, vs float64 oracle autograd.  ETH:
    attention length 1 (fused trunk front); NBA: attention over the forward-call batch."""
    dataset, Tp, Tf = DATA[tag]
    m = _hip(dataset, Tp, Tf, method, steps)
    grads, losses = _check_vs_oracle(m, _golden_setup(golden, tag), dataset, Tp, Tf, method, steps, f'{tag} {method} x{steps}')
    # the integrator reached the objective: the default one-Euler-step model gives other losses
    g = golden('forward_grads')
    assert abs(losses[0] - float(g[f'{tag}_losses'][0])) > 1e-4 * abs(losses[0])


def _scene_batch_setup(sb, seed):
    rng = torch.Generator().manual_seed(seed)
    n = sb.n_agents
    eps = (torch.randn(n, 32, generator=rng), torch.randn(n, 32, generator=rng), torch.randn(n * 20, 32, generator=rng))

    def setup(m):
        m.set_scene_batch(sb.past, sb.future, sb.scene_ptr)
        return eps
    return setup


@pytest.mark.parametrize('case', ['eth', 'eth_scenes', 'nba'])
def test_with_and_without_grad_agree(golden, case):
    """Under a non-default integrator forward() with autograd (training kernels) and under torch.no_grad() (inference kernels) return the
    same five losses."""
    from sttode_amd import scenes
    if case == 'eth_scenes':
        dataset, Tp, Tf = DATA['eth']
        setup = _scene_batch_setup(scenes.make_scene_batch(range(300, 305), 'eth'), 11)
    else:
        dataset, Tp, Tf = DATA[case]
        setup = _golden_setup(golden, case)
    m = _hip(dataset, Tp, Tf, 'rk4', 2)
    eq, ep1, ep20 = (t.to(m.device) for t in setup(m))
    with torch.no_grad():
        ref = m.forward(eq, ep1, ep20)
    ref = [float(ref[0])] + [float(v) for v in ref[1:]]
    eq, ep1, ep20 = (t.to(m.device) for t in setup(m))
    out = m.forward(eq, ep1, ep20)
    out[0].backward()
    got = [float(out[0].detach())] + [float(v) for v in out[1:]]
    np.testing.assert_allclose(got, ref, rtol=1e-4, atol=1e-6)


def test_graph_replay_switching_integrators(golden):
    """Steps on one model with hipGraph capture on, switching ode_method between euler and rk4 and back: each step equals the same step
    run eagerly on a second model, and the rk4 steps sit on the float64 yardstick.  A graph captured for one integrator is never
    replayed for the other."""
    setup = _golden_setup(golden, 'eth')
    mg, me = _hip('eth', 8, 12, 'euler', 1), _hip('eth', 8, 12, 'euler', 1)
    mg.train_graphs, me.train_graphs = True, False
    seq = [('euler', 1), ('rk4', 2), ('euler', 1), ('rk4', 2), ('euler', 1), ('rk4', 2)]   # eager, captured, replayed per key
    rk4 = None
    for i, (method, steps) in enumerate(seq):
        mg.ode_method, mg.ode_steps = me.ode_method, me.ode_steps = method, steps
        gg, lg = _hip_run(mg, setup)
        ge, le = _hip_run(me, setup)
        np.testing.assert_allclose(lg, le, rtol=1e-6, err_msg=f'step {i} {method}')
        for k, v in ge.items():
            if v is None:
                assert gg[k] is None or float(gg[k].abs().max()) == 0.0, k
                continue
            scale = float(v.abs().max()) + 1e-30
            assert float((gg[k] - v).abs().max()) <= 1e-5 * scale, (i, method, k)
        if method == 'rk4':
            rk4 = gg if rk4 is None else rk4
            g64, l64 = _oracle_run(_oracle('eth', 8, 12, 'rk4', 2, True), setup, True)
            g32, _ = _oracle_run(_oracle('eth', 8, 12, 'rk4', 2, False), setup, False)
            np.testing.assert_allclose(lg, l64, rtol=1e-4)
            _yardstick(gg, g64, g32, f'graph step {i} rk4')
    keys = list(mg._graphs)
    assert any(k[-1] == ('rk4', 2) for k in keys) and any(k[-1] != ('rk4', 2) for k in keys), keys


def test_dropout_masks_rk4_vs_oracle(golden):
    """train() mode: the positional encoders' dropout masks injected, ('rk4', 2), vs the oracle with the same masks."""
    _gpu()
    g = golden('forward_grads')
    rng = np.random.default_rng(4)
    n = g['eth_obs'].shape[0]
    dp = torch.from_numpy(((rng.random((n * 8, 64)) < 0.9) / 0.9).astype(np.float32))
    df = torch.from_numpy(((rng.random((n * 12, 64)) < 0.9) / 0.9).astype(np.float32))
    m = _hip('eth', 8, 12, 'rk4', 2)
    _, losses = _check_vs_oracle(m, _golden_setup(golden, 'eth'), 'eth', 8, 12, 'rk4', 2, 'eth rk4 x2 dropout', drop=(dp, df), train_mode=True)
    _, plain = _hip_run(m, _golden_setup(golden, 'eth'))
    assert abs(losses[0] - plain[0]) > 1e-4 * abs(plain[0])          # the masks really changed the objective


def test_config5_rk4_40_steps_at_training_size():
    """BASELINE config 5's integrator, ('rk4', 40) on obs 10 / pred 40, an NBA batch of 4 x 10: finite losses and gradients on the float64
    yardstick.  160 stages: the factor is looser than the two-step cases' (each stage adds fp32 rounding on the HIP side as on torch's, and
    the fp32 autograd sample is one draw of it).  The peak device memory the step adds over the forward() state is reported and stays
    under the deferred weight-gradient cap plus the stage-input tape."""
    from sttode_amd import scenes
    from sttode_amd.training import _ODE_DW_CAP
    d = scenes.nba_batch(91, 4, N=10, obs_len=10, pred_len=40)
    data = {'past_traj': torch.from_numpy(d['past_traj']), 'future_traj': torch.from_numpy(d['future_traj'])}
    rng = torch.Generator().manual_seed(5)
    eps = (torch.randn(40, 32, generator=rng), torch.randn(40, 32, generator=rng), torch.randn(800, 32, generator=rng))

    def setup(m):
        m.set_data_nba(data)
        return eps
    m = _hip('nba', 10, 40, 'euler', 1)
    m.train_graphs = False
    _hip_run(m, setup)                                                 # warm: buffers every step allocates whatever the integrator
    peak = {}
    for method, steps in (('euler', 1), ('rk4', 40)):
        m.ode_method, m.ode_steps = method, steps
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        if method == 'euler':
            _hip_run(m, setup)
        else:
            grads, losses = _check_vs_oracle(m, setup, 'nba', 10, 40, 'rk4', 40, 'nba config 5 rk4 x40', factor=8.0)
        torch.cuda.synchronize()
        peak[method] = torch.cuda.max_memory_allocated() - base
    assert all(np.isfinite(losses))
    assert all(v is None or bool(torch.isfinite(v).all()) for v in grads.values())
    extra = peak['rk4'] - peak['euler']
    tape = 2 * 160 * 40 * 64 * 4
    print(f'config 5 (rk4 x40, 40 agents): peak device memory of the step {peak["rk4"] / 2**20:.1f} MB, {extra / 2**20:.1f} MB over the '
          f'(euler, 1) step (deferred weight-gradient cap {_ODE_DW_CAP / 2**20:.0f} MB, stage-input tape {tape / 2**20:.2f} MB)')
    assert extra < _ODE_DW_CAP + tape + (64 << 20)


def test_generic_widths_refuse_non_default_integrators(golden):
    """hidden_dim 128 runs the generic form, which has no stage program: forward() with autograd raises instead of training Euler."""
    from sttode_amd import STTODENet
    a = make_args('eth', 8, 12)
    a.hidden_dim = 128
    m = STTODENet(a, _gpu()).eval()
    eq, ep1, ep20 = (t.to(m.device) for t in _golden_setup(golden, 'eth')(m))
    m.ode_method, m.ode_steps = 'rk4', 1
    with pytest.raises(NotImplementedError):
        m.forward(eq, ep1, ep20)


def test_default_integrator_path_is_untouched(golden, monkeypatch):
    """('euler', 1): the step never enters the stage program (no sttode_ode_combine launch, eager or captured) and its graph key has the
    shape it had before the integrator was part of the key."""
    from sttode_amd import capi
    setup = _golden_setup(golden, 'eth')
    m = _hip('eth', 8, 12, 'euler', 1)
    m.train_graphs = True
    seen = []
    orig = capi.call

    def spy(name, *args, **kw):
        seen.append(name)
        return orig(name, *args, **kw)
    monkeypatch.setattr(capi, 'call', spy)
    for _ in range(3):                                                 # eager, captured, replayed
        _hip_run(m, setup)
    assert 'sttode_ttrunk_fwd' in seen and not {'sttode_ode_combine', 'sttode_ttrunk_ode_fwd', 'sttode_ode_stage_bwd'} & set(seen)
    keys = list(m._graphs) + list(m._graph_seen)
    assert keys and all(k[-1] == float(m.ODE_TIME) for k in keys), keys
    m.ode_method, m.ode_steps = 'rk4', 1
    n0 = len(seen)
    _hip_run(m, setup)                                                 # eager: the stage program, attention length 1
    new = seen[n0:]
    # one integration-forward launch for both trunks, one dX-chain launch per stage (4), one masked combination for dy_T
    assert new.count('sttode_ttrunk_ode_fwd') == 1 and new.count('sttode_ode_stage_bwd') == 4 and new.count('sttode_ode_combine') == 1, new


@pytest.mark.parametrize('tag', ['eth', 'nba'])
def test_chunked_weight_gradient_pass_matches_one_chunk(golden, tag, monkeypatch):
    """The deferred weight-gradient pass flushed in chunks of 1 and of 3 stages (('rk4', 2): 8 stages, 3 does not divide them) gives the
    gradients of the one-chunk pass: the chunk boundaries, the buffers of each chunk and its flush are exercised at a size where every
    stage would otherwise fit in one chunk.  ETH: the per-stage dX-chain kernel; NBA: the layer-by-layer stage program."""
    from sttode_amd import training
    dataset, Tp, Tf = DATA[tag]
    setup = _golden_setup(golden, tag)
    m = _hip(dataset, Tp, Tf, 'rk4', 2)
    m.train_graphs = False
    ref, lref = _hip_run(m, setup)
    for chunk in (1, 3):
        monkeypatch.setattr(training, '_ode_chunk_stages', lambda nst, per_stage, c=chunk: c)
        got, lgot = _hip_run(m, setup)
        np.testing.assert_allclose(lgot, lref, rtol=1e-6)
        for k, v in ref.items():
            if v is None:
                continue
            scale = float(v.abs().max()) + 1e-30
            assert float((got[k] - v).abs().max()) <= 2e-5 * scale, (chunk, k)
