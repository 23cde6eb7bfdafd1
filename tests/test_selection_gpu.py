"""GPU tests of best-of-K selection (utils/metrics.py:7-48): the kernel (sttode_best_of_k_select) against the reference's outputs in
tests/golden/selection.npz and against sttode_best_of_k, its pipelined form (sttode_async_best_of_k_select) against the serial one, the
drop-in module sttode_amd.metrics, and the report forms of the evaluation loops against a per-scene loop written like test.py:171-205."""
import numpy as np
import pytest
import torch

from helpers import make_args
from test_selection import select_np

pytestmark = pytest.mark.gpu

_MODELS = {}
FIELDS = ('ade', 'fde', 'best_ade_idx', 'best_fde_idx', 'miss', 'best', 'seg_ade', 'seg_fde', 'seg_miss')


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    return torch.device('cuda:0')


def _model(dataset='eth', Tp=8, Tf=12):
    from sttode_amd import STTODENet
    from sttode_amd.weights import make_weights, to_torch_state_dict
    key = (dataset, Tp, Tf)
    if key not in _MODELS:
        m = STTODENet(make_args(dataset, Tp, Tf), _gpu()).eval()
        m.load_state_dict(to_torch_state_dict(make_weights(1234, past_length=Tp, future_length=Tf)), strict=True)
        _MODELS[key] = m
    return _MODELS[key]


def _dataset(ids, kind):
    from sttode_amd import datasets, scenes

    class DS(datasets._SceneDataset):
        def __init__(self):
            sb = scenes.make_scene_batch(ids, kind)
            cnt = np.diff(sb.scene_ptr)
            ends = np.cumsum(cnt)
            self.seq_start_end = list(zip((ends - cnt).tolist(), ends.tolist()))
            self.num_seq = len(cnt)
            self.obs_traj = torch.from_numpy(np.ascontiguousarray(sb.past.transpose(0, 2, 1)))
            self.pred_traj = torch.from_numpy(np.ascontiguousarray(sb.future.transpose(0, 2, 1)))
    return DS()


def _z_fn(zall):
    pos = [0]

    def z_fn(rows):
        z = torch.from_numpy(zall[pos[0]:pos[0] + rows])
        pos[0] += rows
        return z
    return z_fn


def _same(a, b, what):
    for f in FIELDS:
        x, y = getattr(a, f), getattr(b, f)
        assert (x is None) == (y is None), (what, f)
        if x is not None:
            assert torch.equal(x, y), (what, f)


def _clear_gap(values, rel):
    """Agents whose best and second-best value differ by more than `rel` relative (their index does not hinge on rounding)."""
    d = np.sort(values, axis=1)
    return np.ones(len(d), bool) if d.shape[1] < 2 else (d[:, 1] - d[:, 0]) > rel * np.maximum(d[:, 1], 1e-30)


def test_kernel_against_the_reference_fixture(golden):
    from sttode_amd import capi, metrics
    dev = _gpu()
    g = golden('selection')
    for tag in map(str, g['cases']):
        pred_np, gt_np, sp = g[tag + '/pred'], g[tag + '/gt'], g[tag + '/scene_ptr']
        pred, gt = torch.from_numpy(pred_np).to(dev), torch.from_numpy(gt_np).to(dev)
        n, K, Tf = pred_np.shape[:3]
        r = select_np(pred_np, gt_np, seg_ptr=sp)
        for scale in (1.0, 1.7):
            sel = metrics.select(pred, gt, scale=scale, seg_ptr=sp, gather=True)
            ade, fde = torch.empty(n, device=dev), torch.empty(n, device=dev)
            capi.call('sttode_best_of_k', pred, gt, n, K, Tf, scale, ade, fde, capi.stream_ptr())
            torch.cuda.synchronize()
            assert torch.equal(sel.ade, ade) and torch.equal(sel.fde, fde), (tag, scale)          # the bits of sttode_best_of_k
            idx = sel.best_ade_idx.cpu().numpy()
            assert ((idx >= 0) & (idx < K)).all()
            assert torch.equal(sel.best, pred[torch.arange(n, device=dev), sel.best_ade_idx.long()]), tag   # the gather, bit for bit
        sel = metrics.select(pred, gt, seg_ptr=sp)
        idx, fidx = sel.best_ade_idx.cpu().numpy(), sel.best_fde_idx.cpu().numpy()
        va = np.linalg.norm(pred_np - gt_np[:, None], axis=-1).astype(np.float32)
        ade_k, fde_k = va.mean(axis=-1), va[..., -1]
        clear = _clear_gap(ade_k, 1e-6)
        assert clear.mean() > 0.5 or tag.startswith('ties'), tag       # (the tie cases are checked exactly below)
        np.testing.assert_array_equal(idx[clear], g[tag + '/best_idx'][clear], err_msg=tag)         # get_best_idx
        fclear = _clear_gap(fde_k, 1e-6)
        np.testing.assert_array_equal(fidx[fclear], r['best_fde_idx'][fclear], err_msg=tag)
        np.testing.assert_allclose(sel.seg_ade.cpu().numpy(), g[tag + '/scene_ade'], rtol=2e-5, atol=2e-5, err_msg=tag)
        np.testing.assert_allclose(sel.seg_fde.cpu().numpy(), g[tag + '/scene_fde'], rtol=2e-5, atol=2e-5, err_msg=tag)
        for j, thr in enumerate(g['thresholds']):
            s2 = metrics.select(pred, gt, miss_threshold=float(thr), seg_ptr=torch.from_numpy(sp).to(dev))
            np.testing.assert_array_equal(s2.seg_miss.cpu().numpy(), g[tag + '/scene_miss'][j], err_msg=f'{tag} {thr}')
            assert int(s2.miss.sum()) == int(g[tag + '/scene_miss'][j].sum())
        # the drop-ins: the reference's arguments (a list of [K, Tf, 2] per agent) and return types
        agents = [pred_np[a] for a in range(n)]
        best = metrics.get_best_idx(agents, gt_np)
        assert isinstance(best, list) and all(type(i) is int for i in best)
        assert best == idx.tolist()
        a0, a1 = int(sp[0]), int(sp[1])
        assert abs(metrics.compute_ADE(agents[a0:a1], gt_np[a0:a1]) - g[tag + '/scene_ade'][0]) <= 2e-5 * (1 + g[tag + '/scene_ade'][0])
        assert abs(metrics.compute_FDE(pred_np[a0:a1], gt_np[a0:a1]) - g[tag + '/scene_fde'][0]) <= 2e-5 * (1 + g[tag + '/scene_fde'][0])
        for j, thr in enumerate(g['thresholds']):
            assert metrics.count_miss_samples(agents, gt_np, mr_threshold=thr) == int(g[tag + '/scene_miss'][j].sum())
    for tag in ('ties_k20_t12', 'ties_k64_t12'):                        # exact ties: the lowest k, everywhere
        pred = torch.from_numpy(g[tag + '/pred']).to(dev)
        sel = metrics.select(pred, torch.from_numpy(g[tag + '/gt']).to(dev))
        np.testing.assert_array_equal(sel.best_ade_idx.cpu().numpy(), g[tag + '/best_idx'], err_msg=tag)


def test_serial_async_and_generic_handles_agree():
    """The same predictions through select_best_of_k (caller's stream), select_best_of_k_async on the pipelined call (lagged launches with
    the fused metrics on and off, and the round-3 forms with set_lagged(0)) and a generic-form handle: the same bits."""
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
            for _ in range(3):                                           # three calls in flight: the first one's groups run behind later launches
                h = m.inference_async(z=z, metrics_gt=m._future if fused else None)
                hs.append((h, m.select_best_of_k_async(h, miss_threshold=1.5, seg_ptr='scenes', gather=True)))
            for h, sel in hs:
                pred = m.wait(h).permute(1, 0, 2, 3)
                ser = m.select_best_of_k(pred, miss_threshold=1.5, seg_ptr=m._scene_ptr, gather=True)
                gen = m.select_best_of_k_async({'generic': True, 'pred': pred.contiguous(), 'gt_default': m._future,
                                                'inputs': (m._past, m._scene_ptr)}, miss_threshold=1.5, seg_ptr='scenes', gather=True)
                torch.cuda.synchronize()
                _same(sel, ser, f'async vs serial (lagged {lagged}, fused {fused})')
                _same(gen, ser, 'generic handle vs serial')
                if fused:
                    ade, fde = m.best_of_k_async(h)
                    torch.cuda.synchronize()
                    assert torch.equal(ade, sel.ade) and torch.equal(fde, sel.fde)
            m.reset_async()
    finally:
        nat.set_lagged(3)
        m.reset_async()


def _per_scene_loop(m, ds, zall, K, thr, scale=1.0):
    """test.py:171-205: one set_data + inference per scene, the metrics in NumPy on the host (the reference's arithmetic)."""
    out = {'ade': [], 'fde': [], 'miss': [], 'idx': [], 'ade_k': []}
    for s0, s1 in ds.seq_start_end:
        m.set_data(None, ds.obs_traj[s0:s1], ds.pred_traj[s0:s1])
        dec = m.inference(None, z=torch.from_numpy(zall[s0 * K:s1 * K])).permute(1, 0, 2, 3).cpu().numpy() * scale
        gt = ds.pred_traj[s0:s1].numpy().transpose(0, 2, 1) * scale
        dist = np.linalg.norm(dec - gt[:, None], axis=-1)
        ade_k = dist.mean(axis=-1)
        fde = dist[..., -1].min(axis=1)
        out['ade'].append(ade_k.min(axis=1).mean())
        out['fde'].append(fde.mean())
        out['miss'].append(fde)
        out['idx'].append(np.argmin(ade_k, axis=1))
        out['ade_k'].append(ade_k)
    return out


def _check_report(rep, ref, thr, n_scenes):
    assert len(rep.scene_ade) == n_scenes and rep.n_agents == len(rep.best_idx)
    np.testing.assert_allclose(rep.scene_ade, ref['ade'], rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(rep.scene_fde, ref['fde'], rtol=1e-4, atol=1e-4)
    fde = np.concatenate(ref['miss'])
    sure = np.abs(fde - thr) > 1e-4 * (1 + thr)                          # agents whose miss does not hinge on rounding
    miss_ref = np.array([int((f > thr).sum()) for f in ref['miss']])
    assert abs(rep.miss_count - int((fde > thr).sum())) <= int((~sure).sum())
    assert sure.mean() > 0.9
    if sure.all():
        np.testing.assert_array_equal(rep.scene_miss, miss_ref)
    ade_k = np.concatenate(ref['ade_k'])
    clear = _clear_gap(ade_k, 1e-4)
    assert clear.mean() > 0.9
    np.testing.assert_array_equal(rep.best_idx[clear], np.concatenate(ref['idx'])[clear])
    assert rep.miss_rate == rep.miss_count / rep.n_agents and int(rep.scene_agents.sum()) == rep.n_agents


@pytest.mark.parametrize('kind,ids,per_call', [('eth', range(5200, 5330), 48), ('sdd', range(6100, 6190), 40)])
def test_scene_reports_against_a_per_scene_loop_and_eval_scenes(kind, ids, per_call):
    from sttode_amd import scenes
    from sttode_amd.evaluate import eval_scenes, eval_scenes_report
    m = _model('eth')
    ds = _dataset(ids, kind)
    K = m.args.sample_k
    n = int(ds.obs_traj.shape[0])
    zall = scenes.latents(57, n)
    thr = 1.0
    rep = eval_scenes_report(m, ds, scenes_per_call=per_call, z_fn=_z_fn(zall), miss_threshold=thr, gather=True)
    rep_s = eval_scenes_report(m, ds, scenes_per_call=per_call, z_fn=_z_fn(zall), miss_threshold=thr, pipelined=False)
    a, f, na = eval_scenes(m, ds, scenes_per_call=per_call, z_fn=_z_fn(zall))
    assert (rep.ade, rep.fde, rep.n_agents) == (a, f, na)                 # the existing loop's values, bit for bit
    a_s, f_s, _ = eval_scenes(m, ds, scenes_per_call=per_call, z_fn=_z_fn(zall), pipelined=False)
    assert (rep_s.ade, rep_s.fde) == (a_s, f_s)
    ref = _per_scene_loop(m, ds, zall, K, thr)
    for r in (rep, rep_s):
        _check_report(r, ref, thr, len(ds))
    assert rep.best.shape == (n, 12, 2) and rep_s.best is None
    np.testing.assert_array_equal(rep.best_idx, rep_s.best_idx)
    np.testing.assert_array_equal(rep.scene_miss, rep_s.scene_miss)
    np.testing.assert_allclose(rep.scene_ade, rep_s.scene_ade, rtol=1e-5, atol=1e-6)
    # repeated runs: bitwise the same report
    rep2 = eval_scenes_report(m, ds, scenes_per_call=per_call, z_fn=_z_fn(zall), miss_threshold=thr, gather=True)
    for f_ in ('scene_ade', 'scene_fde', 'scene_miss', 'best_idx', 'best_fde_idx', 'best'):
        np.testing.assert_array_equal(getattr(rep, f_), getattr(rep2, f_), err_msg=f_)
    assert (rep.ade, rep.fde, rep.miss_count) == (rep2.ade, rep2.fde, rep2.miss_count)


def test_sampler_report_matches_eval_sampler():
    from sttode_amd import Sampler
    from sttode_amd.evaluate import eval_sampler, eval_sampler_report
    from sttode_amd.weights import make_sampler_weights, to_torch_state_dict
    from helpers import sampler_args
    m = _model('eth')
    smp = Sampler(sampler_args('eth', 8, 12))
    smp.load_state_dict(to_torch_state_dict(make_sampler_weights()), strict=True)
    smp.set_device(m.device)
    smp.eval()
    ds = _dataset(range(8300, 8420), 'eth')
    rep = eval_sampler_report(m, smp, ds, scenes_per_call=50, miss_threshold=0.8)
    a, f, n = eval_sampler(m, smp, ds, scenes_per_call=50)
    assert (rep.ade, rep.fde, rep.n_agents) == (a, f, n)
    rep_s = eval_sampler_report(m, smp, ds, scenes_per_call=50, miss_threshold=0.8, pipelined=False)
    np.testing.assert_allclose(rep_s.scene_ade, rep.scene_ade, rtol=2e-5, atol=2e-5)
    assert abs(rep_s.miss_count - rep.miss_count) <= 1 and len(rep.scene_ade) == len(ds)


def test_nba_report_against_a_per_batch_loop():
    from sttode_amd import scenes
    from sttode_amd.evaluate import eval_nba, eval_nba_report
    m = _model('nba', 5, 10)
    N, K, Tf = 11, 20, 10
    sizes = [32, 32, 32, 20]
    loader = []
    for i, B in enumerate(sizes):
        d = scenes.nba_batch(7700 + i, B, N=N)
        loader.append({'past_traj': torch.from_numpy(d['past_traj']), 'future_traj': torch.from_numpy(d['future_traj'])})
    zall = scenes.latents(78, sum(sizes) * N)
    thr = 2.0
    rep = eval_nba_report(m, loader, traj_scale=2.0, z_fn=_z_fn(zall), groups_per_call=2, miss_threshold=thr, gather=True)
    rep_s = eval_nba_report(m, loader, traj_scale=2.0, z_fn=_z_fn(zall), pipelined=False, miss_threshold=thr)
    hm = eval_nba(m, loader, traj_scale=2.0, z_fn=_z_fn(zall), groups_per_call=2)
    assert abs(rep.ade - hm[Tf][0]) < 2e-5 * (1 + hm[Tf][0]) and abs(rep.fde - hm[Tf][1]) < 2e-5 * (1 + hm[Tf][1])
    ref = {'ade': [], 'fde': [], 'miss': [], 'idx': [], 'ade_k': []}
    pos = 0
    for data in loader:                                                  # test.py:495-552: one inference per loader batch
        B = data['past_traj'].shape[0]
        m.set_data_nba(data)
        dec = m.inference(data, z=torch.from_numpy(zall[pos:pos + B * N * K])).permute(1, 0, 2, 3).cpu().numpy() * 2.0
        pos += B * N * K
        gt = data['future_traj'].numpy().reshape(B * N, Tf, 2) * 2.0
        dist = np.linalg.norm(dec - gt[:, None], axis=-1)
        ade_k = dist.mean(axis=-1)
        fde = dist[..., -1].min(axis=1)
        ref['ade'].append(ade_k.min(axis=1).mean()); ref['fde'].append(fde.mean()); ref['miss'].append(fde)
        ref['idx'].append(np.argmin(ade_k, axis=1)); ref['ade_k'].append(ade_k)
    for r in (rep, rep_s):
        _check_report(r, ref, thr, len(loader))
    np.testing.assert_array_equal(rep.scene_agents, np.array(sizes) * N)
    assert rep.best.shape == (sum(sizes) * N, Tf, 2)


def test_k_over_64_is_refused_and_nothing_written():
    from sttode_amd import capi, metrics
    dev = _gpu()
    n, K, Tf = 5, 65, 12
    pred, gt = torch.randn(n, K, Tf, 2, device=dev), torch.randn(n, Tf, 2, device=dev)
    outs = [torch.full((n,), -7.0, device=dev), torch.full((n,), -7.0, device=dev), torch.full((n,), -7, dtype=torch.int32, device=dev)]
    with pytest.raises(capi.SttodeError, match='K > 64'):
        capi.call('sttode_best_of_k_select', pred, gt, n, K, Tf, 1.0, 1.0, None, 0, outs[0], outs[1], outs[2], None, None, None, None,
                  None, None, capi.stream_ptr())
    torch.cuda.synchronize()
    assert all((o == -7).all() for o in outs)
    with pytest.raises(ValueError, match='K <= 64'):
        metrics.select(pred, gt)


def test_repeated_runs_are_bitwise_identical():
    from sttode_amd import metrics, scenes
    dev = _gpu()
    sb = scenes.make_scene_batch(range(9400, 9700), 'sdd')
    n = sb.n_agents
    rng = np.random.default_rng(3)
    gt = torch.from_numpy(sb.future).to(dev)
    pred = (gt[:, None] + torch.from_numpy(rng.normal(0, 1.0, (n, 20, 12, 2)).astype(np.float32)).to(dev)).contiguous()
    sp = torch.from_numpy(sb.scene_ptr).to(dev)
    first = metrics.select(pred, gt, scale=1.3, seg_ptr=sp, gather=True)
    for _ in range(3):
        _same(metrics.select(pred, gt, scale=1.3, seg_ptr=sp, gather=True), first, 'repeat')
