"""GPU tests of the sample-spread metrics: sttode_sample_spread against tests/golden/sample_spread.npz and the stored value of
the reference's diversity_loss, the best-of-k columns against the best-of-K selection bit for bit, repeatability, the pipelined form against
the serial one, the report loops' new fields, refusals.

Tolerance of the float64 outputs: |got - ref| <= 1e-10 * (sum of the magnitudes of the terms combined) -- the worst-case N u bound of
N <= 2016 * 200 float64 additions, u = 2^-53, is 4.5e-11.  Every term of apd / fpd / pade / dlow is positive, so that sum is the value
itself; for the energy scores it is A + B of the difference A - B (the fixture's es_*_mag).  Measured on an MI355X (worst ratio
|got - ref| / magnitude over all cases): apd 7.2e-16, fpd 8.4e-16, pade 2.8e-15, dlow 2.6e-15, es_ade 1.2e-15, es_fde 3.6e-16;
dlow.sum() / n against the stored value of the reference's diversity_loss 3.3e-16."""
import numpy as np
import pytest
import torch

from test_sample_spread import F64, cases, close
from test_scene_metrics_gpu import NEW_FIELDS as SCENE_FIELDS, _old_fields_equal
from test_selection_gpu import _dataset, _gpu, _model, _z_fn

pytestmark = pytest.mark.gpu

OUTS = ('apd', 'fpd', 'pade', 'dlow', 'es_ade', 'es_fde', 'ade_at_k', 'fde_at_k')
SPREAD_FIELDS = ('apd', 'fpd', 'pade', 'dlow', 'energy_ade', 'energy_fde', 'spread_agents', 'ade_at_k', 'fde_at_k')
U32 = 2.0 ** -24


def _same(a, b, what):
    for f in OUTS:
        x, y = getattr(a, f), getattr(b, f)
        assert (x is None) == (y is None), (what, f)
        if x is not None:
            assert torch.equal(torch.isnan(x), torch.isnan(y)) and torch.equal(torch.nan_to_num(x, nan=0.0), torch.nan_to_num(y, nan=0.0)), (what, f)


def test_kernel_against_the_fixture(golden):
    from sttode_amd import metrics
    dev = _gpu()
    worst = {k: 0.0 for k in F64 + ('es_ade', 'es_fde', 'dlow_ref')}
    failures = []
    for tag, pred_np, gt_np, scale, ds, g in cases(golden):
        n, K, Tf = pred_np.shape[:3]
        pred, gt = torch.from_numpy(pred_np).to(dev), torch.from_numpy(gt_np).to(dev)
        ss = metrics.sample_spread(pred, gt, scale=scale, div_scale=ds)
        s0 = metrics.sample_spread(pred, scale=scale, div_scale=ds)   # without a ground truth: the pair outputs alone, the same bits
        torch.cuda.synchronize()
        assert s0.es_ade is None and s0.es_fde is None and s0.ade_at_k is None and s0.fde_at_k is None
        with pytest.raises(ValueError, match='ground truth'):
            s0.at(1)
        for k in F64:
            assert getattr(ss, k).dtype == torch.float64 and getattr(ss, k).shape == (n,)
            a, b = getattr(ss, k), getattr(s0, k)
            assert torch.equal(torch.nan_to_num(a, nan=-1.0), torch.nan_to_num(b, nan=-1.0)), (tag, k)
        for k, mag in [(k, k) for k in F64] + [('es_ade', 'es_ade_mag'), ('es_fde', 'es_fde_mag')]:
            try:
                worst[k] = max(worst[k], close(getattr(ss, k).cpu().numpy(), g[tag + '/' + k], g[tag + '/' + mag], f'{tag} {k}'))
            except AssertionError as e:
                failures.append(str(e))
        got, ref = float(ss.dlow.sum().item() / n), float(g[tag + '/dlow_ref'])   # diversity_loss's loss_unweighted
        if np.isnan(ref):
            assert np.isnan(got), tag
        else:
            worst['dlow_ref'] = max(worst['dlow_ref'], abs(got - ref) / abs(ref))
            if not abs(got - ref) <= 1e-10 * abs(ref):
                failures.append(f'{tag} dlow.sum() / n = {got!r}, the reference gives {ref!r}')
        # the float32 best-of-k columns against the float64 restatement: the products x * scale are rounded to float32 before the difference
        # there and after it here (<= 2^-24 |x scale| per coordinate of pred and of gt), then Tf + 4 float32 roundings of the distance sum
        big = float(np.nanmax(np.abs(np.concatenate([pred_np.ravel(), gt_np.ravel()])))) * abs(scale)
        for k in ('ade_at_k', 'fde_at_k'):
            v, want = getattr(ss, k).cpu().numpy(), g[tag + '/' + k]
            assert v.dtype == np.float32 and v.shape == (n, K)
            np.testing.assert_array_equal(np.isinf(v), np.isinf(want), err_msg=f'{tag} {k}')
            fin = np.isfinite(want)
            assert (np.abs(v[fin] - want[fin]) <= 2 * U32 * (2 * big + (Tf + 4) * want[fin])).all(), (tag, k)
            a5, f5 = ss.at(min(5, K))
            assert torch.equal(a5, ss.ade_at_k[:, min(5, K) - 1]) and torch.equal(f5, ss.fde_at_k[:, min(5, K) - 1])
    print('worst |got - ref| / magnitude per output:', {k: '%.2e' % v for k, v in worst.items()})
    assert not failures, failures


def test_best_of_k_columns_are_the_selection_bit_for_bit(golden):
    from sttode_amd import metrics
    dev = _gpu()
    for tag, pred_np, gt_np, scale, ds, g in cases(golden):
        n, K, Tf = pred_np.shape[:3]
        pred, gt = torch.from_numpy(pred_np).to(dev), torch.from_numpy(gt_np).to(dev)
        ss = metrics.sample_spread(pred, gt, scale=scale, div_scale=ds)
        sel = metrics.select(pred, gt, scale=scale)
        torch.cuda.synchronize()
        for at, full in ((ss.ade_at_k, sel.ade), (ss.fde_at_k, sel.fde)):
            a, b = at[:, K - 1], full
            assert torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a), torch.nan_to_num(b)), tag
        # column k - 1: what the selection gives for the first k samples
        pre_a = torch.stack([metrics.select(pred[:, :k].contiguous(), gt, scale=scale).ade for k in range(1, K + 1)], dim=1)
        pre_f = torch.stack([metrics.select(pred[:, :k].contiguous(), gt, scale=scale).fde for k in range(1, K + 1)], dim=1)
        assert torch.equal(ss.ade_at_k, pre_a) and torch.equal(ss.fde_at_k, pre_f), tag
        if not np.isnan(pred_np).any():                                # ... and the running minimum of the per-sample values
            one = [metrics.select(pred[:, k:k + 1].contiguous(), gt, scale=scale) for k in range(K)]
            va = np.stack([s.ade.cpu().numpy() for s in one], axis=1)
            vf = np.stack([s.fde.cpu().numpy() for s in one], axis=1)
            np.testing.assert_array_equal(ss.ade_at_k.cpu().numpy(), np.minimum.accumulate(va, axis=1), err_msg=tag)
            np.testing.assert_array_equal(ss.fde_at_k.cpu().numpy(), np.minimum.accumulate(vf, axis=1), err_msg=tag)


def test_two_runs_give_equal_bits(golden):
    from sttode_amd import metrics
    dev = _gpu()
    g = golden('sample_spread')
    for tag in ('k7_t3_n70', 'k64_t40', 'nan_k20_t12'):
        pred, gt = torch.from_numpy(g[tag + '/pred']).to(dev), torch.from_numpy(g[tag + '/gt']).to(dev)
        first = metrics.sample_spread(pred, gt, scale=1.3, div_scale=2.0)
        for _ in range(2):
            _same(metrics.sample_spread(pred, gt, scale=1.3, div_scale=2.0), first, tag)


def test_serial_and_pipelined_agree_on_an_eth_golden_batch(golden):
    """sample_spread_async on lagged inference_async calls (three in flight, fused metrics on; the round-3 form with set_lagged(0)) gives the
    bits of sample_spread on the same samples (the scene of tests/golden/eth_N32.npz)."""
    g = golden('eth_N32')
    m = _model('eth')
    nat = m.native()
    z = torch.from_numpy(g['z']).to(m.device)
    try:
        for lagged, fused in ((3, True), (0, False)):
            nat.set_lagged(lagged)
            m.set_data(None, torch.from_numpy(g['obs']), torch.from_numpy(g['pred']))
            hs = []
            for _ in range(3):
                h = m.inference_async(z=z, metrics_gt=m._future if fused else None)
                hs.append((h, m.sample_spread_async(h, scale=1.3, div_scale=2.0), m.select_best_of_k_async(h, scale=1.3)))
            for h, ss, sel in hs:
                pred = m.wait(h).permute(1, 0, 2, 3)
                ser = m.sample_spread(pred, scale=1.3, div_scale=2.0)
                torch.cuda.synchronize()
                _same(ss, ser, f'async vs serial (lagged {lagged}, fused {fused})')
                assert h['spread'] is ss and torch.equal(ss.ade_at_k[:, -1], sel.ade) and torch.equal(ss.fde_at_k[:, -1], sel.fde)
                assert ss.apd.shape == (32,) and bool((ss.apd > 0).all()) and bool(((ss.dlow >= 0) & (ss.dlow < 1)).all())
            m.reset_async()
    finally:
        nat.set_lagged(3)
        m.reset_async()


def test_serial_and_pipelined_agree_on_an_nba_golden_batch(golden):
    from sttode_amd import scenes
    g = golden('nba_B32')
    m = _model('nba', 5, 10)
    B, N = 32, 11
    d = scenes.nba_batch(int(g['nba_seed']), B)
    z = torch.from_numpy(scenes.latents(int(g['z_seed']), B * N)).to(m.device)
    try:
        hs = []
        for _ in range(2):
            m.set_data_nba({'past_traj': torch.from_numpy(d['past_traj']), 'future_traj': torch.from_numpy(d['future_traj'])})
            h = m.inference_async(z=z)
            hs.append((h, m.sample_spread_async(h, gt=m._future, scale=2.0, div_scale=1.0), m._future))
        for h, ss, gt in hs:
            pred = m.wait(h).permute(1, 0, 2, 3)
            ser = m.sample_spread(pred, gt=gt, scale=2.0, div_scale=1.0)
            torch.cuda.synchronize()
            _same(ss, ser, 'nba async vs serial')
            assert ss.apd.shape == (B * N,) and ss.ade_at_k.shape == (B * N, 20)
    finally:
        m.reset_async()


def _check_spread_fields(rep, K, ks):
    n = rep.n_agents
    assert rep.spread_agents.shape == (n, 6) and rep.spread_agents.dtype == np.float64 and np.isfinite(rep.spread_agents).all()
    for i, f in enumerate(SPREAD_FIELDS[:6]):
        assert abs(getattr(rep, f) - float(rep.spread_agents[:, i].sum() / n)) <= 1e-12 * abs(getattr(rep, f)), f   # (the order of the sum)
    assert rep.apd > 0 and rep.fpd > 0 and rep.pade > 0 and 0 < rep.dlow < 1 and rep.energy_ade > 0 and rep.energy_fde > 0
    want = [k for k in ks if k <= K]
    assert list(rep.ade_at_k) == want and list(rep.fde_at_k) == want
    vals = [rep.ade_at_k[k] for k in want]
    assert all(a >= b for a, b in zip(vals, vals[1:]))                 # more samples never hurt
    if K in want:                                                      # best-of-K over all samples is the report's own ADE / FDE
        assert abs(rep.ade_at_k[K] - rep.ade) <= 1e-12 * rep.ade and abs(rep.fde_at_k[K] - rep.fde) <= 1e-12 * rep.fde


def test_scene_report_with_spread():
    from sttode_amd import scenes
    from sttode_amd.evaluate import eval_scenes_report
    m = _model('eth')
    ds = _dataset(range(5200, 5290), 'eth')
    K = m.args.sample_k
    zall = scenes.latents(57, int(ds.obs_traj.shape[0]))
    ks = (1, 5, 10, 20, 40)
    reps = {}
    for pipelined in (True, False):
        off = eval_scenes_report(m, ds, scenes_per_call=48, z_fn=_z_fn(zall), pipelined=pipelined, gather=True)
        on = eval_scenes_report(m, ds, scenes_per_call=48, z_fn=_z_fn(zall), pipelined=pipelined, gather=True, spread=True, ks=ks)
        assert all(getattr(off, f) is None for f in SPREAD_FIELDS + SCENE_FIELDS)
        assert all(getattr(on, f) is None for f in SCENE_FIELDS)
        _old_fields_equal(on, off)                                     # every pre-existing field: the same bits
        _check_spread_fields(on, K, ks)
        reps[pipelined] = on
    # the two forms' samples differ by float32 rounding; the metrics follow
    np.testing.assert_allclose(reps[True].spread_agents, reps[False].spread_agents, rtol=1e-3, atol=1e-4)
    # div_scale: default the DLow scale of the model's dataset (eth: 1); a larger scale gives a larger kernel value, nothing else moves
    wide = eval_scenes_report(m, ds, scenes_per_call=48, z_fn=_z_fn(zall), gather=True, spread=True, div_scale=10.0, ks=ks)
    one = eval_scenes_report(m, ds, scenes_per_call=48, z_fn=_z_fn(zall), gather=True, spread=True, div_scale=1.0, ks=ks)
    np.testing.assert_array_equal(one.spread_agents, reps[True].spread_agents)
    np.testing.assert_array_equal(wide.spread_agents[:, [0, 1, 2, 4, 5]], one.spread_agents[:, [0, 1, 2, 4, 5]])
    assert (wide.spread_agents[:, 3] > one.spread_agents[:, 3]).all() and wide.ade_at_k == one.ade_at_k


def test_nba_and_reduced_reports_with_spread():
    from sttode_amd import scenes
    from sttode_amd.evaluate import eval_nba_report, eval_scenes_reduced
    m = _model('nba', 5, 10)
    N = 11
    loader = []
    for i, B in enumerate((16, 16, 8)):
        d = scenes.nba_batch(7700 + i, B, N=N)
        loader.append({'past_traj': torch.from_numpy(d['past_traj']), 'future_traj': torch.from_numpy(d['future_traj'])})
    zall = scenes.latents(78, 40 * N)
    for pipelined in (True, False):
        off = eval_nba_report(m, loader, traj_scale=2.0, z_fn=_z_fn(zall), groups_per_call=2, pipelined=pipelined)
        on = eval_nba_report(m, loader, traj_scale=2.0, z_fn=_z_fn(zall), groups_per_call=2, pipelined=pipelined, spread=True)
        _old_fields_equal(on, off)
        _check_spread_fields(on, 20, (1, 5, 10))
    e = _model('eth')
    ds = _dataset(range(5200, 5230), 'eth')
    z2 = scenes.latents(9, 2 * int(ds.obs_traj.shape[0]))
    off = eval_scenes_reduced(e, ds, rounds=2, K=10, z_fn=_z_fn(z2), pipelined=False)
    on = eval_scenes_reduced(e, ds, rounds=2, K=10, z_fn=_z_fn(z2), pipelined=False, spread=True, ks=(1, 5, 10, 20))
    _old_fields_equal(on, off)
    assert all(getattr(off, f) is None for f in SPREAD_FIELDS)
    _check_spread_fields(on, 10, (1, 5, 10, 20))


def test_refusals_write_nothing():
    from sttode_amd import capi, metrics
    dev = _gpu()
    n, Tf = 5, 12

    def outs(K):
        return [torch.full((n,), -7.0, dtype=torch.float64, device=dev) for _ in range(6)] + [torch.full((n, K), -7.0, device=dev) for _ in range(2)]
    for K, ds, what in ((65, 1.0, '2 <= K <= 64'), (1, 1.0, '2 <= K <= 64'), (20, 0.0, 'div_scale'), (20, float('inf'), 'div_scale'),
                        (20, float('nan'), 'div_scale')):
        pred, gt = torch.randn(n, K, Tf, 2, device=dev), torch.randn(n, Tf, 2, device=dev)
        o = outs(K)
        with pytest.raises(capi.SttodeError, match='sttode_sample_spread.*' + what):
            capi.call('sttode_sample_spread', pred, gt, n, K, Tf, 1.0, ds, *o, capi.stream_ptr())
        with pytest.raises(ValueError, match=what):
            metrics.sample_spread(pred, gt, div_scale=ds)
        torch.cuda.synchronize()
        assert all(bool((t == -7).all()) for t in o)
    pred, gt = torch.randn(n, 20, Tf, 2, device=dev), torch.randn(n, Tf, 2, device=dev)
    o = outs(20)
    with pytest.raises(capi.SttodeError, match='need gt'):             # an output that needs gt, without gt
        capi.call('sttode_sample_spread', pred, None, n, 20, Tf, 1.0, 1.0, *o, capi.stream_ptr())
    with pytest.raises(capi.SttodeError, match='null pointer'):
        capi.call('sttode_sample_spread', pred, gt, n, 20, Tf, 1.0, 1.0, o[0], None, *o[2:], capi.stream_ptr())
    torch.cuda.synchronize()
    assert all(bool((t == -7).all()) for t in o)
    with pytest.raises(ValueError):
        metrics.sample_spread(pred, gt[:, :-1])                        # gt of the wrong shape
    with pytest.raises(ValueError):
        metrics.sample_spread(pred[..., :1], gt)                       # not [n, K, Tf, 2]
    with pytest.raises(ValueError):
        metrics.sample_spread(pred, gt).at(21)
    with pytest.raises(ValueError, match='2 <= K <= 64'):             # the pipelined form refuses before anything is enqueued
        m = _model('eth')
        from sttode_amd import scenes
        sb = scenes.make_scene_batch(range(4100, 4104), 'eth')
        m.set_scene_batch(sb.past, sb.future, sb.scene_ptr)
        h = m.inference_async(z=torch.from_numpy(scenes.latents(3, sb.n_agents)).to(m.device))
        try:
            h['pred'] = h['pred'][:, :1].contiguous()
            m.sample_spread_async(h)
        finally:
            m.reset_async()
