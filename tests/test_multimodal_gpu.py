"""GPU tests of the multi-modal ground truth metrics: sttode_multimodal against tests/golden/multimodal.npz, repeatability,
independence of an agent's values from the other segments of the batch, refusals, and eval_scenes_multimodal against the same pass on
predictions reassembled by hand.

Tolerance of mmade / mmfde: |got - ref| <= 1e-10 * (|ref| + cmag), cmag the largest |coordinate| of the case.  A coordinate difference built
in another order carries at most a few u * cmag of absolute error (u = 2^-53), and the sums add at most (2^20 + 200) u * value: 1.2e-10 at
the limit of n, 3e-14 at the fixture's sizes.  count is exact: no pair of the fixture lies within 1e-9 eps of the threshold
(tests/test_multimodal.py checks that condition on the stored inputs).  Measured on an MI355X (worst |got - ref| / (|ref| + cmag) over all
cases): mmade 1.8e-16, mmfde 2.8e-16."""
import numpy as np
import pytest
import torch

from test_multimodal import cases, close
from test_selection_gpu import _dataset, _gpu, _model, _z_fn

pytestmark = pytest.mark.gpu


def _run(case, dev, seg_ptr='own', **kw):
    from sttode_amd import metrics
    tag, pred, past, gt, scale, eps, h, sp, g = case
    return metrics.multimodal(torch.from_numpy(pred).to(dev), torch.from_numpy(past).to(dev), torch.from_numpy(gt).to(dev), eps, hist_frames=h,
                              scale=scale, seg_ptr=sp if isinstance(seg_ptr, str) else seg_ptr, **kw)


def _bits(a, b, what, rows=slice(None)):
    for f in ('count', 'mmade', 'mmfde'):
        assert torch.equal(getattr(a, f)[rows], getattr(b, f)[rows]), (what, f)   # (no NaN among the outputs: +inf compares equal)


def test_kernel_against_the_fixture(golden):
    dev = _gpu()
    worst = {'mmade': 0.0, 'mmfde': 0.0}
    failures = []
    for case in cases(golden):
        tag, pred, g = case[0], case[1], case[-1]
        mm = _run(case, dev)
        torch.cuda.synchronize()
        n = pred.shape[0]
        assert mm.count.dtype == torch.int32 and mm.count.shape == (n,)
        np.testing.assert_array_equal(mm.count.cpu().numpy(), g[tag + '/count'], err_msg=tag)
        for k in worst:
            v = getattr(mm, k)
            assert v.dtype == torch.float64 and v.shape == (n,)
            try:
                worst[k] = max(worst[k], close(v.cpu().numpy(), g[tag + '/' + k], float(g[tag + '/cmag']), f'{tag} {k}'))
            except AssertionError as e:
                failures.append(str(e))
        if case[6] == case[2].shape[1] - 1:                              # hist_frames defaults to Tp - 1
            _bits(_run(case[:6] + (None,) + case[7:], dev), mm, tag)
    print('worst |got - ref| / (|ref| + cmag) per output:', {k: '%.2e' % v for k, v in worst.items()})
    assert not failures, failures


def test_two_runs_give_equal_bits_and_other_segments_do_not_matter(golden):
    dev = _gpu()
    by_tag = {c[0]: c for c in cases(golden)}
    for tag in ('seg', 'n257_k3', 'nan_k5'):
        first = _run(by_tag[tag], dev)
        for _ in range(2):
            _bits(_run(by_tag[tag], dev), first, tag)
    # another segment appended to the batch (the first 70 agents of another case with the same K, Tp and Tf): the agents' own values keep their bits
    more = by_tag['n257_k3']
    for tag in ('seg', 'far'):
        c = by_tag[tag]
        n = c[1].shape[0]
        sp = np.array([0, n], np.int32) if c[7] is None else c[7]
        both = (tag,) + tuple(np.concatenate([a, b[:70]]) for a, b in zip(c[1:4], more[1:4])) + c[4:7] + (np.append(sp, n + 70).astype(np.int32), c[8])
        got = _run(both, dev)
        assert got.count.shape == (n + 70,)
        _bits(got, _run(c, dev), tag + ' with a segment appended', slice(0, n))
        assert int(got.count[n:].max()) <= 70
    # p agents of another segment in FRONT of the batch: every agent moves to another wave of another workgroup, its tiles start at another
    # address, and it keeps its bits
    for tag in ('n257_k3', 'seg'):
        c = by_tag[tag]
        n = c[1].shape[0]
        alone = _run(c, dev)
        sp = np.array([0, n], np.int32) if c[7] is None else c[7]
        for p in (1, 2, 3):
            both = (tag,) + tuple(np.concatenate([b[:p], a]) for a, b in zip(c[1:4], by_tag['far'][1:4])) + c[4:7] + (np.concatenate([[0], sp + p]).astype(np.int32), c[8])
            got = _run(both, dev)
            for f in ('count', 'mmade', 'mmfde'):
                assert torch.equal(getattr(got, f)[p:], getattr(alone, f)), (tag, p, f)


def test_refusals_write_nothing():
    from sttode_amd import capi, metrics
    dev = _gpu()
    n, K, Tp, Tf = 6, 20, 8, 12
    pred, past, gt = torch.randn(n, K, Tf, 2, device=dev), torch.randn(n, Tp, 2, device=dev), torch.randn(n, Tf, 2, device=dev)
    ok = dict(seg=None, n_seg=0, n=n, K=K, Tp=Tp, Tf=Tf, h=7, scale=1.0, eps=0.3, ws_doubles=16 * n)
    for bad, what in ((dict(n=0), '2\\^20'), (dict(K=65), '1 <= K <= 64'), (dict(K=0), '1 <= K <= 64'), (dict(Tf=0), 'Tf'), (dict(Tp=1, h=1), 'Tp >= 2'),
                      (dict(h=0), 'hist_frames'), (dict(h=8), 'hist_frames'), (dict(eps=-0.1), 'eps'), (dict(eps=float('nan')), 'eps'),
                      (dict(eps=float('inf')), 'eps'), (dict(scale=float('inf')), 'scale'), (dict(ws_doubles=16 * n - 1), 'workspace'),
                      (dict(seg=torch.tensor([0, n], dtype=torch.int32, device=dev)), 'seg_ptr'), (dict(n_seg=1), 'seg_ptr')):
        a = {**ok, **bad}
        ws = torch.full((16 * n,), -7.0, dtype=torch.float64, device=dev)
        count = torch.full((n,), -7, dtype=torch.int32, device=dev)
        mmade, mmfde = (torch.full((n,), -7.0, dtype=torch.float64, device=dev) for _ in range(2))
        with pytest.raises(capi.SttodeError, match='sttode_multimodal.*' + what):
            capi.call('sttode_multimodal', pred, past, gt, a['seg'], a['n_seg'], a['n'], a['K'], a['Tp'], a['Tf'], a['h'], a['scale'], a['eps'], ws,
                      a['ws_doubles'], count, mmade, mmfde, capi.stream_ptr())
        with pytest.raises(capi.SttodeError, match='null pointer'):
            capi.call('sttode_multimodal', pred, past, gt, None, 0, n, K, Tp, Tf, 7, 1.0, 0.3, ws, 16 * n, count, None, mmfde, capi.stream_ptr())
        torch.cuda.synchronize()
        assert all(bool((t == -7).all()) for t in (ws, count, mmade, mmfde)), bad
    for kw, what in ((dict(eps=-1.0), 'eps'), (dict(eps=float('inf')), 'eps'), (dict(hist_frames=8), 'hist_frames'), (dict(hist_frames=0), 'hist_frames'),
                     (dict(scale=float('nan')), 'scale'), (dict(seg_ptr=np.array([0, 3, 5])), 'seg_ptr'), (dict(seg_ptr=np.array([0, 4, 3, n])), 'seg_ptr')):
        with pytest.raises(ValueError, match=what):
            metrics.multimodal(pred, past, gt, **{**dict(eps=0.3), **kw})
    with pytest.raises(ValueError, match='1 <= K <= 64'):
        metrics.multimodal(torch.randn(n, 65, Tf, 2, device=dev), past, gt, 0.3)
    with pytest.raises(ValueError, match='Tp >= 2'):
        metrics.multimodal(pred, past[:, :1], gt, 0.3)
    with pytest.raises(ValueError):
        metrics.multimodal(pred, past[:-1], gt, 0.3)                    # past of another agent count
    with pytest.raises(ValueError):
        metrics.multimodal(pred, past, gt[:, :-1], 0.3)                 # gt of the wrong shape
    with pytest.raises(ValueError, match='within'):
        from sttode_amd.evaluate import eval_scenes_multimodal
        eval_scenes_multimodal(_model('eth'), _dataset(range(5200, 5204), 'eth'), 0.3, within='recording')


def _by_hand(m, ds, zall, scenes_per_call, eps, seg_ptr=None, scale=1.0):
    """metrics.multimodal on the predictions of serial model.inference calls over the same batches, put together by hand."""
    from sttode_amd import metrics
    z_fn, parts = _z_fn(zall), []
    for s0 in range(0, len(ds), scenes_per_call):
        sb = ds.scene_batch(range(s0, min(s0 + scenes_per_call, len(ds))))
        m.set_scene_batch(sb.past, sb.future, sb.scene_ptr)
        parts.append(m.inference(None, z=z_fn(sb.n_agents * m.args.sample_k)).permute(1, 0, 2, 3).clone())
    whole = ds.scene_batch(range(len(ds)))
    return metrics.multimodal(torch.cat(parts).contiguous(), whole.past, whole.future, eps, scale=scale, seg_ptr=seg_ptr), whole


def _some_eps(whole, q):
    """The q-quantile of the pairwise distances of the dataset's anchored histories: an eps at which some agents have neighbours."""
    H = (whole.past[:, :-1] - whole.past[:, -1:]).reshape(whole.past.shape[0], -1).astype(np.float64)
    D = np.sqrt(((H[:, None] - H[None]) ** 2).sum(axis=-1))
    return float(np.quantile(D[~np.eye(len(D), dtype=bool)], q))


def test_scene_loop_gives_the_pass_on_predictions_reassembled_by_hand():
    from sttode_amd import scenes
    from sttode_amd.evaluate import eval_scenes_multimodal
    m = _model('eth')
    ds = _dataset(range(5200, 5290), 'eth')
    n = int(ds.obs_traj.shape[0])
    zall = scenes.latents(57, n)
    whole = ds.scene_batch(range(len(ds)))
    eps = _some_eps(whole, 0.03)
    ds.seq_name = ['a'] * 40 + ['b'] * 50
    file_ptr = np.array([0, whole.scene_ptr[40], n], np.int32)
    for within, sp in (('dataset', None), ('file', file_ptr), ('scene', whole.scene_ptr)):
        rep = eval_scenes_multimodal(m, ds, eps, within=within, scenes_per_call=48, z_fn=_z_fn(zall), pipelined=False)
        mm, _ = _by_hand(m, ds, zall, 48, eps, seg_ptr=sp)
        np.testing.assert_array_equal(rep.count, mm.count.cpu().numpy(), err_msg=within)
        np.testing.assert_array_equal(rep.mmade_agents, mm.mmade.cpu().numpy(), err_msg=within)
        np.testing.assert_array_equal(rep.mmfde_agents, mm.mmfde.cpu().numpy(), err_msg=within)
        assert rep.n_agents == n and rep.within == within and rep.hist_frames == 7 and rep.eps == eps
        assert rep.count.dtype == np.int32 and rep.mmade_agents.dtype == np.float64 and np.isfinite(rep.mmade_agents).all()
        assert rep.mmade == float(rep.mmade_agents.sum() / n) and rep.mmfde == float(rep.mmfde_agents.sum() / n)
        assert rep.mean_count == float(rep.count.sum() / n) and rep.frac_multi == float((rep.count > 1).sum() / n)
        multi = rep.count > 1
        if multi.any():
            assert rep.mmade_multi == float(rep.mmade_agents[multi].sum() / multi.sum())
            assert rep.mmfde_multi == float(rep.mmfde_agents[multi].sum() / multi.sum())
        else:
            assert np.isnan(rep.mmade_multi) and np.isnan(rep.mmfde_multi)
        if sp is not None:
            size = np.repeat(np.diff(sp), np.diff(sp))
            assert (rep.count <= size).all()
        if within == 'dataset':
            assert 0 < rep.frac_multi and rep.mean_count > 1 and rep.mmade_multi > 0
            whole_count = rep.count
        else:
            assert (rep.count <= whole_count).all()
    # the pipelined loop: the same neighbours (they depend on the observed tracks alone); its samples differ by float32 rounding
    pip = eval_scenes_multimodal(m, ds, eps, scenes_per_call=48, z_fn=_z_fn(zall))
    np.testing.assert_array_equal(pip.count, whole_count)
    np.testing.assert_allclose(pip.mmade_agents, eval_scenes_multimodal(m, ds, eps, scenes_per_call=48, z_fn=_z_fn(zall), pipelined=False).mmade_agents,
                               rtol=1e-3, atol=1e-4)


def test_at_eps_zero_the_report_is_best_of_k():
    from sttode_amd import scenes
    from sttode_amd.evaluate import eval_scenes_multimodal, eval_scenes_report
    m = _model('eth')
    ds = _dataset(range(5200, 5290), 'eth')
    zall = scenes.latents(57, int(ds.obs_traj.shape[0]))
    Tf = m.args.future_length
    for pipelined in (False, True):
        rep = eval_scenes_multimodal(m, ds, 0.0, scenes_per_call=48, z_fn=_z_fn(zall), pipelined=pipelined)
        assert (rep.count == 1).all()                                  # pairwise distinct histories: every agent alone
        assert rep.frac_multi == 0.0 and rep.mean_count == 1.0 and np.isnan(rep.mmade_multi) and np.isnan(rep.mmfde_multi)
        sel = eval_scenes_report(m, ds, scenes_per_call=48, z_fn=_z_fn(zall), pipelined=pipelined)
        # the selection sums the frames' float32 distances in float32 (bok_dist): (Tf + 8) roundings of 2^-24 each way
        bound = (Tf + 8) * 2.0 ** -23
        print('eps 0, pipelined %s: mmade %.9g ade %.9g  mmfde %.9g fde %.9g' % (pipelined, rep.mmade, sel.ade, rep.mmfde, sel.fde))
        assert abs(rep.mmade - sel.ade) <= bound * sel.ade and abs(rep.mmfde - sel.fde) <= bound * sel.fde
