"""GPU tests of stage-2 sampler evaluation (test_sampler.py:117-212) on the HIP path: the Q-net kernel (sttode_sampler_qnet), the Q-net on the
pipelined (lagged) launch's stream (SttodeAsyncOpts.sampler), Sampler.inference / inference_async, evaluate.eval_sampler and
trainer.train_sampler_epoch."""
import copy
import ctypes

import numpy as np
import pytest
import torch

from helpers import SAMPLER_CASES, assert_close, make_args, sampler_args, sampler_case_inputs

pytestmark = pytest.mark.gpu

_MODELS = {}


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    return torch.device('cuda:0')


def _model(dataset='eth', Tp=8, Tf=12, fresh=False):
    from sttode_amd import STTODENet
    from sttode_amd.weights import make_weights, to_torch_state_dict
    key = (dataset, Tp, Tf)
    if fresh or key not in _MODELS:
        m = STTODENet(make_args(dataset, Tp, Tf), _gpu()).eval()
        m.load_state_dict(to_torch_state_dict(make_weights(1234, past_length=Tp, future_length=Tf)), strict=True)
        if fresh:
            return m
        _MODELS[key] = m
    return _MODELS[key]


def _sampler(dataset='eth', Tp=8, Tf=12):
    from sttode_amd import Sampler
    from sttode_amd.weights import make_sampler_weights, to_torch_state_dict
    s = Sampler(sampler_args(dataset, Tp, Tf))
    s.load_state_dict(to_torch_state_dict(make_sampler_weights()), strict=True)
    s.set_device(_gpu())
    return s.eval()


def _replicated(g, tag, dataset, mode, rows=1024):
    """The golden case replicated up to a lagged-size batch: (set-data function, eps for the whole batch, agents per replica, replicas)."""
    inp, _ = sampler_case_inputs(g, tag, dataset)
    eps = g[f'{tag}_{mode}_eps']
    if dataset == 'eth':
        obs, pred = inp['obs'].transpose(0, 2, 1), inp['pred'].transpose(0, 2, 1)
        n = obs.shape[0]
        R = -(-rows // n)
        past, fut = np.ascontiguousarray(np.tile(obs, (R, 1, 1))), np.ascontiguousarray(np.tile(pred, (R, 1, 1)))
        ptr = np.arange(R + 1, dtype=np.int32) * n

        def setd(net):
            net.set_scene_batch(torch.from_numpy(past), torch.from_numpy(fut), torch.from_numpy(ptr))
    else:
        d = inp['data']
        n = d['past_traj'].shape[0] * d['past_traj'].shape[1]
        R = -(-rows // n)
        rep = {k: torch.from_numpy(np.ascontiguousarray(np.stack([np.asarray(d[k], np.float32)] * R))) for k in ('past_traj', 'future_traj')}

        def setd(net):
            net.set_data_nba(rep)
    eps_all = np.tile(eps, (R, 1)) if mode == 'peragent' else eps
    return setd, torch.from_numpy(np.ascontiguousarray(eps_all, dtype=np.float32)), n, R


@pytest.mark.parametrize('tag,dataset,Tp,Tf,modes', SAMPLER_CASES)
def test_sampler_inference_vs_reference_golden(golden, tag, dataset, Tp, Tf, modes):
    """Every sampler.npz case through Sampler.inference (one call: the Q-net kernel, then net.inference) and through inference_async in the
    lagged form (the Q-net on the call's stream), every replica of the golden batch against the reference's dec_motion."""
    g = golden('sampler')
    net, smp = _model(dataset, Tp, Tf), _sampler(dataset, Tp, Tf)
    inp, _ = sampler_case_inputs(g, tag, dataset)
    for mode in modes:
        smp.share_eps = mode != 'peragent'
        k = f'{tag}_{mode}_'
        ref = g[k + 'dec']                                                      # [n, K, Tf, 2]
        if dataset == 'eth':
            n = inp['obs'].shape[0]
            net.set_data(None, torch.from_numpy(inp['obs']), torch.from_numpy(inp['pred']), torch.ones(n, Tp), torch.ones(n, Tf))
        else:
            net.set_data_nba({kk: (torch.from_numpy(v) if isinstance(v, np.ndarray) else v) for kk, v in inp['data'].items()})
        out = smp.inference(net, mean=(mode == 'mean'), eps=torch.from_numpy(g[k + 'eps']))
        assert_close(out.permute(1, 0, 2, 3).cpu().numpy(), ref, what=k + 'inference')
        setd, eps, n, R = _replicated(g, tag, dataset, mode)
        setd(net)
        assert smp.unsupported_reason(net, n * R) is None
        h = smp.inference_async(net, mean=(mode == 'mean'), eps=eps)
        outp = net.wait(h).permute(1, 0, 2, 3).cpu().numpy()
        for r in range(R):
            assert_close(outp[r * n:(r + 1) * n], ref, what=f'{k}inference_async replica {r}')
    net.reset_async()


def _composed(net, smp, mean, eps):
    with torch.no_grad():
        return smp.forward(net, mean=mean, eps=eps)[0]                          # [n, K, Tf, 2]


def test_fused_equals_composed_eth_512_scenes_and_nba_groups():
    """The pipelined sampler call against Sampler.forward (linear_cols Q-net + five-kernel decode) with the same injected eps: the
    lagged-versus-serial band (2e-5)."""
    from sttode_amd import scenes
    net, smp = _model('eth'), _sampler('eth')
    sb = scenes.make_scene_batch(range(7000, 7512), 'eth')
    n = sb.n_agents
    rng = np.random.default_rng(5)
    for share in (True, False):
        for mean in (True, False):
            if mean and not share:
                continue
            smp.share_eps = share
            eps = torch.from_numpy(rng.standard_normal((1 if share else n, 32)).astype(np.float32))
            net.set_scene_batch(sb.past, sb.future, sb.scene_ptr)
            ref = _composed(net, smp, mean, eps).cpu().numpy()
            net.set_scene_batch(sb.past, sb.future, sb.scene_ptr)
            h = smp.inference_async(net, mean=mean, eps=eps)
            got = net.wait(h).permute(1, 0, 2, 3).cpu().numpy()
            d = np.abs(got - ref).max()
            assert d <= 2e-5, (share, mean, d)
    net.reset_async()
    netn, smpn = _model('nba', 5, 10), _sampler('nba', 5, 10)
    G = 4
    batches = [scenes.nba_batch(900 + i, 32) for i in range(G)]
    smpn.share_eps = False
    eps = torch.from_numpy(rng.standard_normal((G * 32 * 11, 32)).astype(np.float32))
    refs = []
    for i, d in enumerate(batches):
        netn.set_data_nba(d)
        refs.append(_composed(netn, smpn, False, eps[i * 352:(i + 1) * 352]).cpu().numpy())
    netn.set_data_nba({k: torch.from_numpy(np.stack([np.asarray(d[k], np.float32) for d in batches])) for k in ('past_traj', 'future_traj')})
    assert smpn.unsupported_reason(netn, G * 352) is None
    h = smpn.inference_async(netn, mean=False, eps=eps)
    got = netn.wait(h).permute(1, 0, 2, 3).cpu().numpy()
    d = np.abs(got - np.concatenate(refs)).max()
    assert d <= 2e-5, d
    netn.reset_async()


def test_fused_metrics_of_a_sampler_call_equal_best_of_k_bitwise():
    from sttode_amd import scenes
    net, smp = _model('eth'), _sampler('eth')
    sb = scenes.make_scene_batch(range(7600, 7700), 'eth')
    net.set_scene_batch(sb.past, sb.future, sb.scene_ptr)
    h = smp.inference_async(net, metrics_gt=net._future, metrics_scale=1.7)
    assert h['fused_metrics'] is not None
    ade, fde = net.best_of_k_async(h, scale=1.7)
    pred = net.wait(h)
    a2, f2 = net.best_of_k(pred.permute(1, 0, 2, 3), scale=1.7)
    assert torch.equal(ade, a2) and torch.equal(fde, f2)
    net.reset_async()


def test_eval_sampler_pipelined_serial_and_per_scene_loop_agree():
    """evaluate.eval_sampler, pipelined and not, against a test_sampler.py:124-212-style loop (one set_data + Sampler.forward per scene,
    best-of-K by the CPU oracle, weighted by agent count) on a small synthetic dataset of mixed scene sizes."""
    from oracle import metrics_ref
    from sttode_amd import datasets, scenes
    from sttode_amd.evaluate import eval_sampler

    class DS(datasets._SceneDataset):
        def __init__(self):
            sb = scenes.make_scene_batch(range(8000, 8180), 'eth')
            cnt = np.diff(sb.scene_ptr)
            ends = np.cumsum(cnt)
            self.seq_start_end = list(zip((ends - cnt).tolist(), ends.tolist()))
            self.num_seq = len(cnt)
            self.obs_traj = torch.from_numpy(np.ascontiguousarray(sb.past.transpose(0, 2, 1)))
            self.pred_traj = torch.from_numpy(np.ascontiguousarray(sb.future.transpose(0, 2, 1)))
    ds = DS()
    net, smp = _model('eth'), _sampler('eth')
    a_p, f_p, n_p = eval_sampler(net, smp, ds, traj_scale=1.0, scenes_per_call=60, pipelined=True)
    a_s, f_s, n_s = eval_sampler(net, smp, ds, traj_scale=1.0, scenes_per_call=60, pipelined=False)
    sa = sf = 0.0
    tot = 0
    for s0, s1 in ds.seq_start_end:
        obs, pred = ds.obs_traj[s0:s1], ds.pred_traj[s0:s1]
        n = s1 - s0
        net.set_data(None, obs, pred, torch.ones(n, 8), torch.ones(n, 12))
        dec = _composed(net, smp, True, None).cpu().numpy()
        gt = pred.numpy().transpose(0, 2, 1)
        sa += metrics_ref.compute_ade(dec, gt) * n
        sf += metrics_ref.compute_fde(dec, gt) * n
        tot += n
    assert n_p == n_s == tot
    for a, f in ((a_p, f_p), (a_s, f_s)):
        assert abs(a - sa / tot) <= 1e-5 * sa / tot and abs(f - sf / tot) <= 1e-5 * sf / tot, (a, f, sa / tot, sf / tot)


def test_sampler_and_plain_calls_interleave_and_a_weight_step_is_honoured():
    from sttode_amd import scenes
    net, smp = _model('eth'), _sampler('eth')
    batches = [scenes.make_scene_batch(range(9000 + 100 * i, 9100 + 100 * i), 'eth') for i in range(4)]
    zs = [torch.from_numpy(scenes.latents(40 + i, b.n_agents)) for i, b in enumerate(batches)]
    # references: serial forms on the weights each call must see
    refs = []
    for i, b in enumerate(batches):
        net.set_scene_batch(b.past, b.future, b.scene_ptr)
        refs.append(net.inference(None, z=zs[i]).cpu().numpy().copy())
    samp_ref = []
    for b in batches[:2]:
        net.set_scene_batch(b.past, b.future, b.scene_ptr)
        samp_ref.append(_composed(net, smp, True, None).permute(1, 0, 2, 3).cpu().numpy())
    hs = []
    for i, b in enumerate(batches):                       # plain, sampler, plain, sampler: four calls in flight
        net.set_scene_batch(b.past, b.future, b.scene_ptr)
        hs.append(net.inference_async(z=zs[i]))
        net.set_scene_batch(b.past, b.future, b.scene_ptr)
        if i < 2:
            hs.append(smp.inference_async(net))
    out0 = net.wait(hs[0]).cpu().numpy()                  # (its slot is the one the next call takes)
    with torch.no_grad():                                 # an optimizer-style step between two in-flight sampler calls
        smp.q_b.bias.add_(0.05)
    b = batches[0]
    net.set_scene_batch(b.past, b.future, b.scene_ptr)
    h_after = smp.inference_async(net)
    outs = [out0] + [net.wait(h).cpu().numpy() for h in hs[1:]]
    late = net.wait(h_after).cpu().numpy()
    net.set_scene_batch(b.past, b.future, b.scene_ptr)
    ref_after = _composed(net, smp, True, None).permute(1, 0, 2, 3).cpu().numpy()
    plain = [outs[0], outs[2], outs[4], outs[5]]
    for o, r in zip(plain, refs):
        assert np.abs(o - r).max() <= 2e-5
    assert np.abs(outs[1] - samp_ref[0]).max() <= 2e-5 and np.abs(outs[3] - samp_ref[1]).max() <= 2e-5
    assert np.abs(late - ref_after).max() <= 2e-5
    assert np.abs(late - samp_ref[0]).max() > 1e-3                  # the step did change the predictions
    net.reset_async()


def test_sampler_plan_refusals_leave_the_model_working():
    """A plan together with device latents, and a plan on a call outside the lagged form, fail before anything is enqueued."""
    from sttode_amd import capi, scenes
    net, smp = _model('eth', fresh=True), _sampler('eth')
    sb = scenes.make_scene_batch(range(9500, 9600), 'eth')
    net.set_scene_batch(sb.past, sb.future, sb.scene_ptr)
    ref = _composed(net, smp, True, None).permute(1, 0, 2, 3).cpu().numpy()
    net.set_scene_batch(sb.past, sb.future, sb.scene_ptr)
    nat = net.native()
    n, S = sb.n_agents, int(len(sb.scene_ptr) - 1)
    _, tot = nat.layout(n, S)
    ws = torch.empty(tot, device=net.device)
    nat.init_workspace(ws, n, S)
    z = torch.empty(n * 20, 32, device=net.device)
    pred = torch.empty(n, 20, 12, 2, device=net.device)
    plan, keep = smp._plan(0, None)
    opts = capi.AsyncOpts()
    opts.sampler, opts.device_latents, opts.zkey = ctypes.addressof(plan), 1, 7
    with pytest.raises(capi.SttodeError, match='device_latents'):
        capi.call('sttode_inference_scenes_async', nat.h, net._past, net._scene_ptr, n, S, z, ws, pred, 0, ctypes.addressof(opts), capi.stream_ptr())
    nat.set_lagged(0)
    opts.device_latents = 0
    with pytest.raises(capi.SttodeError, match='lagged'):
        capi.call('sttode_inference_scenes_async', nat.h, net._past, net._scene_ptr, n, S, z, ws, pred, 0, ctypes.addressof(opts), capi.stream_ptr())
    with pytest.raises(capi.SttodeError, match='lagged'):
        net.inference_async(sampler_plan=plan)
    assert smp.unsupported_reason(net, n) is not None
    h = smp.inference_async(net)                                  # not lagged: encoder + Q-net kernel, then inference_async(z=z)
    assert np.abs(net.wait(h).cpu().numpy() - ref).max() <= 2e-5
    net.reset_async()
    nat.set_lagged(3)
    net.set_scene_batch(sb.past, sb.future, sb.scene_ptr)
    h = smp.inference_async(net)
    assert np.abs(net.wait(h).cpu().numpy() - ref).max() <= 2e-5
    net.reset_async()


@pytest.mark.parametrize('dataset,Tp,Tf', [('eth', 8, 12), ('nba', 5, 10)])
def test_train_sampler_epoch_equals_the_hand_written_loop(dataset, Tp, Tf):
    from sttode_amd import samplerloss, scenes
    from sttode_amd.trainer import train_sampler_epoch
    net = _model(dataset, Tp, Tf)
    if dataset == 'eth':
        loader = []
        for s in (4242, 4243):
            o, p = scenes.eth_scene(s, n_min=9, n_max=9)
            o, p = torch.from_numpy(o), torch.from_numpy(p)
            N = o.shape[0]
            loader.append([o[None], p[None], o[None], p[None], torch.zeros(1, N), torch.ones(1, N), torch.ones(1, N, Tp), torch.ones(1, N, Tf),
                           torch.tensor([[10]]), ['seq']])
    else:
        loader = [scenes.nba_batch(70 + i, 4) for i in range(2)]
    cfg = samplerloss.get_diversity_config(dataset)
    s0 = _sampler(dataset, Tp, Tf).train()
    s1 = copy.deepcopy(s0)
    o0 = torch.optim.Adam(s0.parameters(), lr=1e-3)
    o1 = torch.optim.Adam(s1.parameters(), lr=1e-3)
    losses = train_sampler_epoch(s0.args, 0, net, s0, o0, torch.optim.lr_scheduler.StepLR(o0, 10), [copy.copy(b) for b in loader], cfg, log=None)
    hand = []
    for batch in loader:                                   # trainsampler.py:131-185
        if dataset == 'nba':
            net.set_data_nba(batch)
            dec, sd, vd, _ = s1.forward(net)
            fut = torch.as_tensor(batch['future_traj']).to(s1.device).reshape(-1, Tf, 2)
            tot, _, _ = samplerloss.compute_sampler_loss_nba(s1.args, fut, dec.reshape(-1, 20, Tf, 2), 1, vd, sd, cfg)
        else:
            obs, pred = batch[0][0], batch[1][0]
            net.set_data(batch, obs, pred, batch[6][0], batch[7][0])
            dec, sd, vd, _ = s1.forward(net)
            tot, _, _ = samplerloss.compute_sampler_loss(s1.args, pred.to(s1.device).transpose(1, 2), dec, 1, batch[7][0], vd, sd, cfg)
        o1.zero_grad()
        tot.backward()
        o1.step()
        hand.append(float(tot.detach()))
    assert len(losses) == 2 and np.allclose(losses, hand, rtol=1e-6, atol=0), (losses, hand)
    for (k, a), (_, b) in zip(s0.named_parameters(), s1.named_parameters()):
        assert torch.allclose(a, b, rtol=1e-6, atol=1e-7), k
