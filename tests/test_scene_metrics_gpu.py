"""GPU tests of the scene-level metrics: the kernels (sttode_joint_select, sttode_kde_nll) against
tests/golden/scene_metrics.npz and the NumPy restatement of tests/test_scene_metrics.py, one-agent segments against the best-of-K selection,
the pipelined forms against the serial ones, the report loops' new fields against a per-scene loop, refusals and repeatability."""
import numpy as np
import pytest
import torch

from test_scene_metrics import joint_np, kde_nll_np
from test_selection_gpu import _dataset, _gpu, _model, _z_fn

pytestmark = pytest.mark.gpu

JFIELDS = ('seg_jade', 'seg_jfde', 'seg_jade_idx', 'seg_jfde_idx', 'seg_col', 'seg_gt_col')
OLD_FIELDS = ('ade', 'fde', 'n_agents', 'miss_count', 'miss_rate', 'miss_threshold', 'scene_ade', 'scene_fde', 'scene_miss', 'scene_agents',
              'best_idx', 'best_fde_idx', 'best')
NEW_FIELDS = ('joint_ade', 'joint_fde', 'scene_joint_ade', 'scene_joint_fde', 'scene_joint_idx', 'collision_radius', 'collision_rate',
              'gt_collision_rate', 'scene_collision', 'kde_nll', 'kde_nll_agents', 'kde_invalid')


def _same_joint(a, b, what):
    for f in JFIELDS:
        x, y = getattr(a, f), getattr(b, f)
        assert (x is None) == (y is None), (what, f)
        if x is not None:
            assert torch.equal(x, y), (what, f)


def _same_kde(a, b, what):
    assert torch.equal(torch.isnan(a), torch.isnan(b)), what
    assert torch.equal(torch.nan_to_num(a, nan=0.0), torch.nan_to_num(b, nan=0.0)), what


def test_kernels_against_the_golden(golden):
    from sttode_amd import metrics
    dev = _gpu()
    g = golden('scene_metrics')
    for tag in map(str, g['cases']):
        pred_np, gt_np, sp = g[tag + '/pred'], g[tag + '/gt'], g[tag + '/seg_ptr']
        scale, r = float(g[tag + '/scale']), float(g[tag + '/radius'])
        pred, gt = torch.from_numpy(pred_np).to(dev), torch.from_numpy(gt_np).to(dev)
        js = metrics.joint_select(pred, gt, sp, scale=scale, collision_radius=r)
        torch.cuda.synchronize()
        for f in ('seg_jade', 'seg_jfde'):
            np.testing.assert_allclose(getattr(js, f).cpu().numpy(), g[tag + '/' + f], rtol=1e-5, atol=1e-6, err_msg=f'{tag} {f}')
        for f in ('seg_jade_idx', 'seg_jfde_idx', 'seg_col', 'seg_gt_col'):
            np.testing.assert_array_equal(getattr(js, f).cpu().numpy(), g[tag + '/' + f], err_msg=f'{tag} {f}')
        ref = joint_np(pred_np, gt_np, sp, scale, r)                   # the restatement: the same values to the last bit but rarely
        for f in ('seg_jade', 'seg_jfde'):
            np.testing.assert_allclose(getattr(js, f).cpu().numpy(), ref[f], rtol=1e-6, atol=0, err_msg=f'{tag} {f}')
        nll = metrics.kde_nll(pred, gt, scale=scale).cpu().numpy()
        want = g[tag + '/kde_nll']
        np.testing.assert_array_equal(np.isnan(nll), np.isnan(want), err_msg=tag)
        np.testing.assert_allclose(nll[~np.isnan(want)], want[~np.isnan(want)], rtol=0, atol=1e-8, err_msg=tag)
        np.testing.assert_allclose(nll[~np.isnan(want)], kde_nll_np(pred_np, gt_np, scale)[~np.isnan(want)], rtol=0, atol=1e-9, err_msg=tag)
        # without a radius: no collision outputs, the joint values unchanged
        js0 = metrics.joint_select(pred, gt, torch.from_numpy(sp).to(dev), scale=scale)
        assert js0.seg_col is None and js0.seg_gt_col is None
        assert torch.equal(js0.seg_jade, js.seg_jade) and torch.equal(js0.seg_jfde_idx, js.seg_jfde_idx)


def test_one_agent_segments_reproduce_the_selection_bitwise(golden):
    from sttode_amd import metrics, scenes
    dev = _gpu()
    g = golden('scene_metrics')
    inputs = [(g[t + '/pred'], g[t + '/gt']) for t in ('k20_t12', 'k64_t40', 'ties_k20_t12', 'k2_t12', 'k20_t1')]
    sb = scenes.make_scene_batch(range(9400, 9460), 'sdd')
    rng = np.random.default_rng(11)
    inputs.append(((sb.future[:, None] + rng.normal(0, 1.0, (sb.n_agents, 20, 12, 2))).astype(np.float32), sb.future))
    for pred_np, gt_np in inputs:
        pred, gt = torch.from_numpy(pred_np).to(dev), torch.from_numpy(gt_np).to(dev)
        n = pred.shape[0]
        for scale in (1.0, 1.7):
            sel = metrics.select(pred, gt, scale=scale)
            js = metrics.joint_select(pred, gt, np.arange(n + 1), scale=scale, collision_radius=5.0)
            torch.cuda.synchronize()
            assert torch.equal(js.seg_jade, sel.ade) and torch.equal(js.seg_jfde, sel.fde)
            assert torch.equal(js.seg_jade_idx, sel.best_ade_idx) and torch.equal(js.seg_jfde_idx, sel.best_fde_idx)
            assert int(js.seg_col.abs().sum()) == 0 and int(js.seg_gt_col.abs().sum()) == 0


def test_serial_and_pipelined_agree_on_scene_batches():
    """select_joint_async / kde_nll_async on lagged inference_async calls (three in flight; fused metrics on and off; the round-3 forms with
    set_lagged(0)) give the bits of select_joint / kde_nll on the same predictions."""
    from sttode_amd import scenes
    m = _model('eth')
    nat = m.native()
    sb = scenes.make_scene_batch(range(4100, 4180), 'eth')
    z = torch.from_numpy(scenes.latents(31, sb.n_agents)).to(m.device)
    try:
        for lagged, fused in ((3, True), (3, False), (0, False)):
            nat.set_lagged(lagged)
            m.set_scene_batch(sb.past, sb.future, sb.scene_ptr)
            hs = []
            for _ in range(3):
                h = m.inference_async(z=z, metrics_gt=m._future if fused else None)
                hs.append((h, m.select_joint_async(h, scale=1.3, collision_radius=0.4), m.kde_nll_async(h, scale=1.3),
                           m.select_best_of_k_async(h, scale=1.3, seg_ptr='scenes')))
            for h, js, kd, sel in hs:
                pred = m.wait(h).permute(1, 0, 2, 3)
                ser = m.select_joint(pred, scale=1.3, collision_radius=0.4)
                kser = m.kde_nll(pred, scale=1.3)
                ssel = m.select_best_of_k(pred, scale=1.3, seg_ptr=m._scene_ptr)
                torch.cuda.synchronize()
                _same_joint(js, ser, f'joint async vs serial (lagged {lagged}, fused {fused})')
                _same_kde(kd, kser, f'kde async vs serial (lagged {lagged}, fused {fused})')
                assert torch.equal(sel.seg_ade, ssel.seg_ade)
            m.reset_async()
    finally:
        nat.set_lagged(3)
        m.reset_async()


def test_serial_and_pipelined_agree_on_nba_groups():
    from sttode_amd import scenes
    m = _model('nba', 5, 10)
    N, K = 11, 20
    G, B = 3, 8
    past = np.stack([scenes.nba_batch(7800 + i, B, N=N)['past_traj'] for i in range(G)])
    fut = np.stack([scenes.nba_batch(7800 + i, B, N=N)['future_traj'] for i in range(G)])
    n = G * B * N
    games = torch.arange(0, n + 1, N, dtype=torch.int32, device=m.device)
    torch.cuda.synchronize()
    zall = torch.from_numpy(scenes.latents(5, n)).to(m.device)
    try:
        hs = []
        for _ in range(3):
            m.set_data_nba({'past_traj': torch.from_numpy(past), 'future_traj': torch.from_numpy(fut)})
            h = m.inference_async(z=zall)
            hs.append((h, m.select_joint_async(h, gt=m._future, seg_ptr=games, scale=2.0, collision_radius=0.3),
                       m.kde_nll_async(h, gt=m._future, scale=2.0), m._future))
        for h, js, kd, gt in hs:
            pred = m.wait(h).permute(1, 0, 2, 3)
            ser = m.select_joint(pred, gt=gt, seg_ptr=games, scale=2.0, collision_radius=0.3)
            kser = m.kde_nll(pred, gt=gt, scale=2.0)
            torch.cuda.synchronize()
            _same_joint(js, ser, 'nba joint async vs serial')
            _same_kde(kd, kser, 'nba kde async vs serial')
            assert js.seg_jade.numel() == G * B
    finally:
        m.reset_async()


def _per_scene_metrics(m, ds, zall, K, r, scale=1.0):
    """One set_data + inference per scene (test.py:171-205), the scene metrics of that scene alone through sttode_amd.metrics and the
    NumPy restatement."""
    from sttode_amd import metrics
    out = {'jade': [], 'jfde': [], 'jidx': [], 'col': [], 'gcol': [], 'nll': [], 'np_jade': [], 'np_col': [], 'np_nll': []}
    for s0, s1 in ds.seq_start_end:
        m.set_data(None, ds.obs_traj[s0:s1], ds.pred_traj[s0:s1])
        pred = m.inference(None, z=torch.from_numpy(zall[s0 * K:s1 * K])).permute(1, 0, 2, 3).contiguous()
        gt = m._future
        js = metrics.joint_select(pred, gt, [0, s1 - s0], scale=scale, collision_radius=r)
        out['jade'].append(float(js.seg_jade[0])); out['jfde'].append(float(js.seg_jfde[0])); out['jidx'].append(int(js.seg_jade_idx[0]))
        out['col'].append(int(js.seg_col[0])); out['gcol'].append(int(js.seg_gt_col[0]))
        out['nll'].append(metrics.kde_nll(pred, gt, scale=scale).cpu().numpy())
        p_np, g_np = pred.cpu().numpy(), gt.cpu().numpy()
        ref = joint_np(p_np, g_np, [0, s1 - s0], scale, r)
        out['np_jade'].append(float(ref['seg_jade'][0])); out['np_col'].append(int(ref['seg_col'][0]))
        out['np_nll'].append(kde_nll_np(p_np, g_np, scale))
    return out


def _check_new_fields(rep, ref, K, r):
    S = len(ref['jade'])
    assert rep.scene_joint_ade.shape == (S,) and rep.scene_collision.shape == (S, 2)
    np.testing.assert_allclose(rep.scene_joint_ade, ref['jade'], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(rep.scene_joint_ade, ref['np_jade'], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(rep.scene_joint_fde, ref['jfde'], rtol=1e-4, atol=1e-5)
    assert (np.asarray(ref['jidx']) == rep.scene_joint_idx).mean() > 0.9
    assert abs(rep.joint_ade - float(np.mean(np.asarray(rep.scene_joint_ade, np.float64)))) == 0.0
    assert (rep.scene_joint_ade >= rep.scene_ade - 1e-5).all()                      # one k for the scene is never better than each agent's
    assert (rep.scene_joint_fde >= rep.scene_fde - 1e-5).all()
    col = np.asarray(ref['col'])
    assert abs(int(rep.scene_collision[:, 0].sum()) - int(col.sum())) <= max(2, int(0.01 * col.sum()))
    assert abs(int(col.sum()) - int(np.sum(ref['np_col']))) <= max(2, int(0.01 * col.sum()))
    np.testing.assert_array_equal(rep.scene_collision[:, 1], ref['gcol'])
    assert rep.collision_radius == r
    assert rep.collision_rate == rep.scene_collision[:, 0].sum() / (K * rep.n_agents)
    assert rep.gt_collision_rate == rep.scene_collision[:, 1].sum() / rep.n_agents
    nll = np.concatenate(ref['nll'])
    np.testing.assert_array_equal(np.isnan(rep.kde_nll_agents), np.isnan(nll))
    ok = ~np.isnan(nll)
    np.testing.assert_allclose(rep.kde_nll_agents[ok], nll[ok], rtol=1e-3, atol=1e-3)
    np.testing.assert_allclose(rep.kde_nll_agents[ok], np.concatenate(ref['np_nll'])[ok], rtol=1e-3, atol=1e-3)
    assert rep.kde_invalid == int((~ok).sum()) and rep.kde_nll == float(rep.kde_nll_agents[ok].mean())


def _old_fields_equal(a, b):
    for f in OLD_FIELDS:
        x, y = getattr(a, f), getattr(b, f)
        if isinstance(x, np.ndarray) or isinstance(y, np.ndarray):
            assert (x is None) == (y is None) and (x is None or (x.dtype == y.dtype and np.array_equal(x, y))), f
        else:
            assert x == y, f


@pytest.mark.parametrize('kind,ids,per_call', [('eth', range(5200, 5330), 48), ('sdd', range(6100, 6190), 40)])
def test_scene_reports_with_the_new_options(kind, ids, per_call):
    from sttode_amd import scenes
    from sttode_amd.evaluate import eval_scenes_report
    m = _model('eth')
    ds = _dataset(ids, kind)
    K = m.args.sample_k
    zall = scenes.latents(57, int(ds.obs_traj.shape[0]))
    r = 0.3
    for pipelined in (True, False):
        off = eval_scenes_report(m, ds, scenes_per_call=per_call, z_fn=_z_fn(zall), pipelined=pipelined, gather=True)
        on = eval_scenes_report(m, ds, scenes_per_call=per_call, z_fn=_z_fn(zall), pipelined=pipelined, gather=True, joint=True, kde=True,
                                collision_radius=r)
        assert all(getattr(off, f) is None for f in NEW_FIELDS)
        _old_fields_equal(on, off)                                     # every pre-existing field: the same bits
        ref = _per_scene_metrics(m, ds, zall, K, r)
        _check_new_fields(on, ref, K, r)
        if pipelined:
            first = on
        else:
            np.testing.assert_array_equal(on.scene_joint_idx, first.scene_joint_idx)
            np.testing.assert_allclose(on.scene_joint_ade, first.scene_joint_ade, rtol=1e-5, atol=1e-6)
    again = eval_scenes_report(m, ds, scenes_per_call=per_call, z_fn=_z_fn(zall), gather=True, joint=True, kde=True, collision_radius=r)
    for f in NEW_FIELDS + OLD_FIELDS:                                  # two runs: bitwise the same report
        x, y = getattr(first, f), getattr(again, f)
        if isinstance(x, np.ndarray):
            assert np.array_equal(x, y, equal_nan=x.dtype.kind == 'f'), f
        elif isinstance(x, float) and np.isnan(x):
            assert np.isnan(y), f
        else:
            assert x == y, f


def test_sampler_report_with_the_new_options():
    from sttode_amd import Sampler
    from sttode_amd.evaluate import eval_sampler_report
    from sttode_amd.weights import make_sampler_weights, to_torch_state_dict
    from helpers import sampler_args
    m = _model('eth')
    smp = Sampler(sampler_args('eth', 8, 12))
    smp.load_state_dict(to_torch_state_dict(make_sampler_weights()), strict=True)
    smp.set_device(m.device)
    smp.eval()
    ds = _dataset(range(8300, 8420), 'eth')
    off = eval_sampler_report(m, smp, ds, scenes_per_call=50)
    on = eval_sampler_report(m, smp, ds, scenes_per_call=50, joint=True, kde=True, collision_radius=0.3)
    _old_fields_equal(on, off)
    assert len(on.scene_joint_ade) == len(ds) and on.kde_nll_agents.shape == (on.n_agents,)
    assert (on.scene_joint_ade >= on.scene_ade - 1e-5).all() and 0.0 <= on.collision_rate <= 1.0 and 0.0 <= on.gt_collision_rate <= 1.0
    only_col = eval_sampler_report(m, smp, ds, scenes_per_call=50, collision_radius=0.3)
    assert only_col.joint_ade is None and only_col.kde_nll is None
    np.testing.assert_array_equal(only_col.scene_collision, on.scene_collision)


def test_nba_report_segments_are_games():
    from sttode_amd import metrics, scenes
    from sttode_amd.evaluate import eval_nba_report
    m = _model('nba', 5, 10)
    N, K, Tf = 11, 20, 10
    sizes = [32, 32, 32, 20]
    loader = []
    for i, B in enumerate(sizes):
        d = scenes.nba_batch(7700 + i, B, N=N)
        loader.append({'past_traj': torch.from_numpy(d['past_traj']), 'future_traj': torch.from_numpy(d['future_traj'])})
    zall = scenes.latents(78, sum(sizes) * N)
    r = 0.5
    for pipelined in (True, False):
        off = eval_nba_report(m, loader, traj_scale=2.0, z_fn=_z_fn(zall), groups_per_call=2, pipelined=pipelined)
        on = eval_nba_report(m, loader, traj_scale=2.0, z_fn=_z_fn(zall), groups_per_call=2, pipelined=pipelined, joint=True, kde=True,
                             collision_radius=r)
        _old_fields_equal(on, off)
        assert on.scene_joint_ade.shape == (sum(sizes),) and on.scene_collision.shape == (sum(sizes), 2)
        # the per-game values of one loader batch at a time, through sttode_amd.metrics
        ref_j, ref_c, ref_n, pos = [], [], [], 0
        for data in loader:
            B = data['past_traj'].shape[0]
            m.set_data_nba(data)
            pred = m.inference(data, z=torch.from_numpy(zall[pos:pos + B * N * K])).permute(1, 0, 2, 3).contiguous()
            pos += B * N * K
            js = metrics.joint_select(pred, m._future, np.arange(0, B * N + 1, N), scale=2.0, collision_radius=r)
            ref_j.append(js.seg_jade.cpu().numpy()); ref_c.append(js.seg_gt_col.cpu().numpy())
            ref_n.append(metrics.kde_nll(pred, m._future, scale=2.0).cpu().numpy())
        np.testing.assert_allclose(on.scene_joint_ade, np.concatenate(ref_j), rtol=1e-4, atol=1e-5)
        np.testing.assert_array_equal(on.scene_collision[:, 1], np.concatenate(ref_c))
        nll = np.concatenate(ref_n)
        np.testing.assert_array_equal(np.isnan(on.kde_nll_agents), np.isnan(nll))
        np.testing.assert_allclose(on.kde_nll_agents[~np.isnan(nll)], nll[~np.isnan(nll)], rtol=1e-3, atol=1e-3)


def test_refusals_write_nothing():
    from sttode_amd import capi, metrics
    dev = _gpu()
    n, Tf = 5, 12
    sp = torch.tensor([0, 2, 5], dtype=torch.int32, device=dev)
    for K in (65, 1):
        pred, gt = torch.randn(n, K, Tf, 2, device=dev), torch.randn(n, Tf, 2, device=dev)
        jo = [torch.full((2,), -7.0, device=dev), torch.full((2,), -7.0, device=dev)] + [torch.full((2,), -7, dtype=torch.int32, device=dev)
                                                                                         for _ in range(4)]
        nll = torch.full((n,), -7.0, dtype=torch.float64, device=dev)
        if K > 64:
            with pytest.raises(capi.SttodeError, match='K > 64'):
                capi.call('sttode_joint_select', pred, gt, n, K, Tf, 1.0, sp, 2, 0.5, *jo, capi.stream_ptr())
            with pytest.raises(ValueError, match='K <= 64'):
                metrics.joint_select(pred, gt, sp)
        with pytest.raises(capi.SttodeError, match='2 <= K <= 64'):
            capi.call('sttode_kde_nll', pred, gt, n, K, Tf, 1.0, nll, capi.stream_ptr())
        with pytest.raises(ValueError, match='2 <= K <= 64'):
            metrics.kde_nll(pred, gt)
        torch.cuda.synchronize()
        assert all((o == -7).all() for o in jo) and (nll == -7).all()
    pred, gt = torch.randn(n, 20, Tf, 2, device=dev), torch.randn(n, Tf, 2, device=dev)
    with pytest.raises(ValueError):
        metrics.joint_select(pred, gt[:, :-1], sp)                     # gt of the wrong shape
    with pytest.raises(ValueError):
        metrics.kde_nll(pred[..., :1], gt)                             # not [n, K, Tf, 2]
    with pytest.raises(ValueError):
        metrics.joint_select(pred, gt, [0, 2, 4])                      # CSR does not end at n
    with pytest.raises(ValueError):
        metrics.joint_select(pred, gt, sp, collision_radius=0.0)
    with pytest.raises(ValueError, match='2 <= K <= 64'):             # the pipelined forms refuse before anything is enqueued
        m = _model('eth')
        from sttode_amd import scenes
        sb = scenes.make_scene_batch(range(4100, 4104), 'eth')
        m.set_scene_batch(sb.past, sb.future, sb.scene_ptr)
        h = m.inference_async(z=torch.from_numpy(scenes.latents(3, sb.n_agents)).to(m.device))
        try:
            h['pred'] = h['pred'][:, :1].contiguous()
            m.kde_nll_async(h)
        finally:
            m.reset_async()


def test_repeated_runs_are_bitwise_identical():
    from sttode_amd import metrics, scenes
    dev = _gpu()
    sb = scenes.make_scene_batch(range(9400, 9700), 'sdd')
    n = sb.n_agents
    rng = np.random.default_rng(3)
    gt = torch.from_numpy(sb.future).to(dev)
    pred = (gt[:, None] + torch.from_numpy(rng.normal(0, 1.0, (n, 20, 12, 2)).astype(np.float32)).to(dev)).contiguous()
    sp = torch.from_numpy(sb.scene_ptr).to(dev)
    first = metrics.joint_select(pred, gt, sp, scale=1.3, collision_radius=0.5)
    k0 = metrics.kde_nll(pred, gt, scale=1.3)
    for _ in range(3):
        _same_joint(metrics.joint_select(pred, gt, sp, scale=1.3, collision_radius=0.5), first, 'repeat')
        _same_kde(metrics.kde_nll(pred, gt, scale=1.3), k0, 'repeat')
    assert int(first.seg_col.sum()) > 0
