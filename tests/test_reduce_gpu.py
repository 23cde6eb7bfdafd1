"""GPU tests of oversample-and-reduce (sttode_reduce_samples, csrc/reduce.hip) against the float64 yardstick of
tests/test_reduce.py.  What is compared, and why not more, is that module's near-tie rule: full runs on the stored seeds whose every margin
holds (labels and counts exactly equal, no sample left out); one Lloyd step from a caller's init on large shapes (labels equal wherever the
float64 margin is >= 1e-3, at most 1 % left out); the centroids always against float64 means over the DEVICE's labels within
M * 2^-24 * max |coordinate| (the bound of a sequential fp32 sum); many iterations at large M through the bitwise chain property.  Then
the layers above: metrics.reduce_samples, STTODENet.inference_reduced, evaluate.eval_scenes_reduced."""
import dataclasses

import numpy as np
import pytest
import torch

from helpers import make_args
from test_reduce import CASES, MARGIN, ONE_STEP_CAP, SHAPES, centroid_atol, kmeans_f64, make_samples, means_over_labels, shape_case

pytestmark = pytest.mark.gpu

_MODELS = {}


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


def _reduce(x, K, **kw):
    """metrics.reduce_samples of a NumPy / torch input -> (centroids, labels, counts) as NumPy arrays and the Reduction."""
    from sttode_amd import metrics
    t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.array(x))              # (a copy: the shared cases are read-only)
    if 'init' in kw and isinstance(kw['init'], np.ndarray):
        kw['init'] = torch.from_numpy(np.array(kw['init'])).to(_gpu())
    red = metrics.reduce_samples(t.to(_gpu()), K, **kw)
    torch.cuda.synchronize()
    return red.centroids.cpu().numpy(), red.labels.cpu().numpy(), red.counts.cpu().numpy(), red


def _same_bits(a, b, what):
    for u, v, f in zip(a[:3], b[:3], ('centroids', 'labels', 'counts')):
        assert u.dtype == v.dtype and u.shape == v.shape and u.tobytes() == v.tobytes(), (what, f)


def _check_centroids(x, prev, cent, lab, cnt, what):
    """Per agent: counts are the label histogram; a non-empty cluster's centroid is the float64 mean over the device's own labels within
    M * 2^-24 * max |coordinate|; an empty cluster has the bits of `prev`, the centroids one iteration earlier (None: not known here)."""
    n, K = cnt.shape
    for a in range(n):
        assert lab[a].min() >= 0 and lab[a].max() < K, what
        np.testing.assert_array_equal(cnt[a], np.bincount(lab[a], minlength=K), err_msg=what)
        ref = means_over_labels(x[a], lab[a], K, np.zeros_like(cent[a]) if prev is None else prev[a])
        full = cnt[a] > 0
        np.testing.assert_allclose(cent[a][full], ref[full], rtol=0, atol=centroid_atol(x[a]), err_msg=what)
        if prev is not None:
            assert cent[a][~full].tobytes() == np.ascontiguousarray(prev[a][~full]).tobytes(), what


@pytest.mark.parametrize('tag', sorted(t for t in CASES if CASES[t][0] == 'full'))
def test_full_runs_on_the_stored_seeds(golden, tag):
    """iters = 10 from 'first' / 'maximin': every label and count equals the yardstick's (every sample's margin holds at every iteration,
    tests/test_reduce.py re-asserts it), the centroids agree with the yardstick's and with float64 means over the device's labels."""
    g = golden('reduce')
    _, _, n, M, K, Tf, t0, init = CASES[tag]
    x = g[tag + '/x']
    out = _reduce(x, K, iters=10, from_frame=t0, init=init)
    np.testing.assert_array_equal(out[1], g[tag + '/labels'], err_msg=tag)
    np.testing.assert_array_equal(out[2], g[tag + '/counts'], err_msg=tag)
    _check_centroids(x, g[tag + '/init'], out[0], out[1], out[2], tag)
    for a in range(n):
        np.testing.assert_allclose(out[0][a], g[tag + '/centroids'][a], rtol=0, atol=centroid_atol(x[a]), err_msg=tag)
    # the same run from the stored initial centroids as a caller's init: for maximin this pins the picks (the yardstick's, all of them)
    _same_bits(out, _reduce(x, K, iters=10, from_frame=t0, init=g[tag + '/init']), tag + ': init as a tensor')
    if t0 == Tf - 1:
        _same_bits(out, _reduce(x, K, iters=10, from_frame=-1, init=init), tag + ': from_frame = -1')


def _check_one_step(tag, x, init, c, lab, cnt, sure, K, t0, **kw):
    out = _reduce(x, K, iters=1, from_frame=t0, init=init, **kw)
    assert 1.0 - sure.mean() <= ONE_STEP_CAP, tag
    np.testing.assert_array_equal(out[1][sure], lab[sure], err_msg=tag)
    _check_centroids(x, init, out[0], out[1], out[2], tag)
    for a in range(x.shape[0]):
        if (out[1][a] == lab[a]).all():
            np.testing.assert_allclose(out[0][a], c[a], rtol=0, atol=centroid_atol(x[a]), err_msg=tag)
    return out


@pytest.mark.parametrize('tag', sorted(t for t in CASES if CASES[t][0] == 'step'))
def test_one_step_on_the_stored_seeds(golden, tag):
    g = golden('reduce')
    _, _, n, M, K, Tf, t0, _ = CASES[tag]
    _check_one_step(tag, g[tag + '/x'], g[tag + '/init'], g[tag + '/centroids'], g[tag + '/labels'], g[tag + '/counts'], g[tag + '/sure'], K, t0)


@pytest.mark.parametrize('tag', sorted(SHAPES))
def test_shapes_one_step_chain_batch_and_layout(tag):
    """Per shape: one step against the yardstick; two runs give the same bits; iters = 3 equals three chained iters = 1 calls that pass the
    centroids on as init, bitwise (an empty cluster therefore keeps its centroid's bits); an agent alone equals the agent inside the batch,
    bitwise; the round-major [R, n, K_in, Tf, 2] layout equals the same samples given as [n, M, Tf, 2], bitwise."""
    seed, n, R, K_in, K, Tf, t0 = SHAPES[tag]
    M = R * K_in
    x, init, c, lab, cnt, sure = shape_case(tag)
    x5 = np.ascontiguousarray(x.reshape(n, R, K_in, Tf, 2).transpose(1, 0, 2, 3, 4))     # sample m = r K_in + k
    out = _check_one_step(tag, x, init, c, lab, cnt, sure, K, t0)
    _same_bits(out, _reduce(x, K, iters=1, from_frame=t0, init=init), tag + ': second run')
    _same_bits(out, _reduce(x5, K, iters=1, from_frame=t0, init=init), tag + ': round-major layout')
    if t0 == Tf - 1:
        _same_bits(out, _reduce(x, K, iters=1, from_frame=-1, init=init), tag + ': from_frame = -1')
    # chain
    whole = _reduce(x5, K, iters=3, from_frame=t0, init=init)
    second = _reduce(x5, K, iters=1, from_frame=t0, init=out[0])
    third = _reduce(x5, K, iters=1, from_frame=t0, init=second[0])
    _same_bits(whole, third, tag + ': iters = 3 against three chained calls')
    _check_centroids(x, second[0], *whole[:3], tag + ': after three iterations')
    # an agent alone; its own 'first' and 'maximin' runs inside the batch too (ten iterations, early stop or not)
    a = n // 2
    for kw in ({'iters': 3, 'init': init}, {'iters': 10, 'init': 'first'}, {'iters': 10, 'init': 'maximin'}):
        batch = _reduce(x5, K, from_frame=t0, **kw)
        kw1 = {**kw, 'init': kw['init'][a:a + 1]} if isinstance(kw['init'], np.ndarray) else kw
        alone = _reduce(x5[:, a:a + 1], K, from_frame=t0, **kw1)
        _same_bits([v[a:a + 1] for v in batch[:3]], alone, f'{tag}: agent {a} alone, {kw["iters"]} iterations')
        _check_centroids(x, None, *batch[:3], f'{tag}: {kw["init"] if isinstance(kw["init"], str) else "init"}, {kw["iters"]} iterations')


def test_identity_single_cluster_duplicates_and_empty_clusters():
    x = make_samples(31, 5, 64, 12)
    x[0, 3, 2, 0] = x[4, 63, 11, 1] = -0.0                             # a lone -0.0 must come back as -0.0
    # K = M with 'first': the centroids are the samples bit for bit, every count is 1
    for M in (20, 64):
        out = _reduce(x[:, :M], M, iters=4, init='first')
        assert out[0].tobytes() == np.ascontiguousarray(x[:, :M]).tobytes() and (out[2] == 1).all()
        assert (out[1] == np.arange(M)[None]).all()
    # K = 1: every label 0, the centroid is the mean
    for t0 in (0, 5, -1):
        out = _reduce(x, 1, iters=3, from_frame=t0, init='maximin')
        assert (out[1] == 0).all() and (out[2] == 64).all()
        _check_centroids(x, None, *out[:3], 'K = 1')
    # duplicate centroids in init: the higher index stays empty and keeps its bits; -0.0 included
    init = np.ascontiguousarray(x[:, :6]).copy()
    init[:, 4] = init[:, 1]
    init[:, 5] = init[:, 1]
    out = _reduce(x, 6, iters=1, init=init)
    assert (out[2][:, 4:] == 0).all() and out[0][:, 4:].tobytes() == init[:, 4:].tobytes()
    _check_centroids(x, init, *out[:3], 'duplicate centroids')
    for a in range(5):                                                  # (margins among the four distinct centroids: the copies tie exactly)
        _, lab, _, marg = kmeans_f64(x[a], init[a, :4], 1)
        sure = marg[0] >= MARGIN
        np.testing.assert_array_equal(out[1][a][sure], lab[sure])
    # exactly duplicated samples take the same label, whatever else happens
    y = x.copy()
    y[:, 40:50] = y[:, 7:8]
    for init in ('first', 'maximin'):
        out = _reduce(y, 5, iters=6, init=init)
        assert (out[1][:, 40:50] == out[1][:, 7:8]).all()
        _check_centroids(y, None, *out[:3], 'duplicated samples')
    # ... and a far-away sample with its ten copies is a cluster of eleven around that sample
    far = y.copy()
    far[:, 7] += 1000.0
    far[:, 40:50] += 1000.0
    out = _reduce(far, 5, iters=2, init=np.ascontiguousarray(far[:, [7, 0, 1, 2, 3]]))
    assert (out[2][:, 0] == 11).all() and (out[1][:, 7] == 0).all() and (out[1][:, 40:50] == 0).all()
    _check_centroids(far, None, *out[:3], 'a repeated far sample')


def test_outputs_beyond_the_extent_are_untouched_and_limits_write_nothing():
    from sttode_amd import capi
    dev = _gpu()
    n, R, K_in, K, Tf = 5, 3, 20, 7, 12
    M = R * K_in
    x = torch.from_numpy(make_samples(41, n, M, Tf).reshape(n, R, K_in, Tf, 2).transpose(1, 0, 2, 3, 4).copy()).to(dev)
    pad = 64
    cent = torch.full((pad + n * K * Tf * 2 + pad,), -7.0, device=dev)
    lab = torch.full((pad + n * M + pad,), -7, dtype=torch.int32, device=dev)
    cnt = torch.full((pad + n * K + pad,), -7, dtype=torch.int32, device=dev)
    args = lambda **kw: (x, kw.get('n', n), R, K_in, Tf, kw.get('K', K), kw.get('iters', 10), kw.get('t0', 0), kw.get('mode', 1), None,
                         cent[pad:], lab[pad:], cnt[pad:], capi.stream_ptr())
    for bad, match in (({'K': 65}, 'K must be'), ({'K': 61}, 'M = R K_in'), ({'iters': 0}, 'iters'), ({'t0': 12}, 'from_frame'),
                       ({'mode': 2}, 'init must be'), ({'n': 0}, 'n must be')):
        with pytest.raises(capi.SttodeError, match='sttode_reduce_samples.*' + match):
            capi.call('sttode_reduce_samples', *args(**bad))
    torch.cuda.synchronize()
    assert (cent == -7).all() and (lab == -7).all() and (cnt == -7).all()
    capi.call('sttode_reduce_samples', *args())
    torch.cuda.synchronize()
    for t, size in ((cent, n * K * Tf * 2), (lab, n * M), (cnt, n * K)):
        assert (t[:pad] == -7).all() and (t[pad + size:] == -7).all()
    l = lab[pad:pad + n * M]
    assert l.min() >= 0 and l.max() < K and int(cnt[pad:pad + n * K].sum()) == n * M and torch.isfinite(cent[pad:pad + n * K * Tf * 2]).all()


def test_non_finite_inputs_keep_the_labels_in_range():
    x = make_samples(43, 3, 70, 12)
    x[0, 5] = np.nan
    x[1, :, 3] = np.inf
    x[2, 0] = -np.inf
    x[2, 1] = np.nan
    for init in ('first', 'maximin'):
        out = _reduce(x, 7, iters=5, init=init)
        assert out[1].min() >= 0 and out[1].max() < 7 and (out[2] >= 0).all() and (out[2].sum(axis=1) == 70).all()


def test_python_layer_arguments():
    from sttode_amd import metrics
    dev = _gpu()
    x = torch.from_numpy(make_samples(47, 4, 40, 12)).to(dev)
    red = metrics.reduce_samples(x, 5, from_frame=-12)
    assert red.centroids.shape == (4, 5, 12, 2) and red.labels.shape == (4, 40) and red.labels.dtype == torch.int32
    assert red.counts.shape == (4, 5) and red.weights.dtype == torch.float32
    assert torch.equal(red.weights, red.counts.float() / 40) and torch.allclose(red.weights.sum(dim=1), torch.ones(4, device=dev))
    assert torch.equal(red.centroids, metrics.reduce_samples(x, 5, from_frame=0).centroids)
    assert torch.equal(red.centroids, metrics.reduce_samples(x.double(), 5).centroids)            # converted to float32
    for bad in (dict(K=0), dict(K=65), dict(K=41), dict(K=5, from_frame=12), dict(K=5, from_frame=-13), dict(K=5, init='kmeans++'),
                dict(K=5, init=torch.zeros(4, 6, 12, 2, device=dev))):
        with pytest.raises(ValueError):
            metrics.reduce_samples(x, **bad)
    with pytest.raises(ValueError):
        metrics.reduce_samples(x[0], 5)


# ----- the layers above ------------------------------------------------------------------------------------------------------------------

def _set(m, mode):
    """Put data on model `m` in one of its three modes; returns the number of agents."""
    from sttode_amd import scenes
    if mode == 'scenes':
        sb = scenes.make_scene_batch(range(5400, 5430), 'eth')
        m.set_scene_batch(sb.past, sb.future, sb.scene_ptr)
        return sb.n_agents
    if mode == 'one_scene':
        obs, fut = scenes.eth_scene(5007, n_min=7, n_max=7)
        m.set_data(None, torch.from_numpy(obs), torch.from_numpy(fut))
        return 7
    d = scenes.nba_batch(7700, 6, N=11)
    m.set_data_nba({'past_traj': torch.from_numpy(d['past_traj']), 'future_traj': torch.from_numpy(d['future_traj'])})
    return 66


@pytest.mark.parametrize('mode', ['scenes', 'one_scene', 'nba'])
def test_inference_reduced_is_the_composition(mode):
    from sttode_amd import metrics, scenes
    m = _model('nba', 5, 10) if mode == 'nba' else _model('eth')
    n = _set(m, mode)
    Ks, rounds = m.args.sample_k, 3
    z = torch.from_numpy(scenes.latents(61, n * rounds).reshape(rounds, n * Ks, -1)).to(m.device)
    for kw in (dict(K=None, iters=10, from_frame=0, init='first'), dict(K=7, iters=4, from_frame=-1, init='maximin')):
        out = m.inference_reduced(rounds, z=z, **kw)
        red = m.reduction
        K = Ks if kw['K'] is None else kw['K']
        assert out.shape == (K, n, m.args.future_length, 2) and m.diverse_pred is red.centroids
        assert torch.equal(out, red.centroids.permute(1, 0, 2, 3))
        stack = torch.stack([m.inference(None, z=z[r]).permute(1, 0, 2, 3).contiguous() for r in range(rounds)])
        ref = metrics.reduce_samples(stack, K, **{k: v for k, v in kw.items() if k != 'K'})
        assert torch.equal(red.centroids, ref.centroids) and torch.equal(red.labels, ref.labels) and torch.equal(red.counts, ref.counts)
        assert torch.equal(red.weights, ref.counts.float() / (rounds * Ks)) and int(red.counts.sum()) == n * rounds * Ks
    _set(m, mode)
    with pytest.raises(ValueError):
        m.inference_reduced(2, z=z)
    with pytest.raises(ValueError):
        m.inference_reduced(0)


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


def _z_fn(zall, log=None):
    pos = [0]

    def z_fn(rows):
        z = torch.from_numpy(zall[pos[0]:pos[0] + rows])
        if log is not None:
            log.append((pos[0], rows))
        pos[0] += rows
        return z
    return z_fn


def _reports_equal(a, b, what):
    for f in dataclasses.fields(a):
        u, v = getattr(a, f.name), getattr(b, f.name)
        if isinstance(u, np.ndarray):
            assert u.dtype == v.dtype and u.shape == v.shape and u.tobytes() == v.tobytes(), (what, f.name)
        else:
            assert u == v or (u is None and v is None), (what, f.name, u, v)


def test_eval_scenes_reduced_against_a_hand_written_composition():
    from sttode_amd import metrics, scenes
    from sttode_amd.evaluate import _ReportAcc, eval_scenes_reduced
    m = _model('eth')
    ds = _dataset(range(5200, 5290), 'eth')
    n, Ks = int(ds.obs_traj.shape[0]), m.args.sample_k
    rounds, K, per_call, thr = 3, 7, 40, 0.8
    zall = scenes.latents(71, n * rounds)
    log = []
    kw = dict(K=K, iters=5, from_frame=-1, init='maximin')
    rep = eval_scenes_reduced(m, ds, rounds, traj_scale=1.3, scenes_per_call=per_call, z_fn=_z_fn(zall, log), pipelined=False,
                              miss_threshold=thr, **kw)
    # z_fn: once per round, in round order, per scene batch
    sizes = [ds.scene_batch(range(s, min(s + per_call, len(ds)))).n_agents * Ks for s in range(0, len(ds), per_call)]
    assert [r for _, r in log] == [s for s in sizes for _ in range(rounds)]
    acc, z_fn = _ReportAcc(thr, K=K), _z_fn(zall)
    for s0 in range(0, len(ds), per_call):
        sb = ds.scene_batch(range(s0, min(s0 + per_call, len(ds))))
        m.set_scene_batch(sb.past, sb.future, sb.scene_ptr)
        stack = torch.stack([m.inference(None, z=z_fn(sb.n_agents * Ks)).permute(1, 0, 2, 3).contiguous() for _ in range(rounds)])
        red = metrics.reduce_samples(stack, K, iters=5, from_frame=-1, init='maximin')
        acc.add(m.select_best_of_k(red.centroids, scale=1.3, miss_threshold=thr, seg_ptr=m._scene_ptr), sb.scene_ptr)
    _reports_equal(rep, acc.report(False), 'serial loop against the composition')
    assert rep.n_agents == n and len(rep.scene_ade) == len(ds) and rep.best_idx.max() < K
    # the pipelined loop: the same calls to z_fn, a report of the same shape (its samples differ by fp32 rounding: no comparison at rounds > 1)
    # (seven rounds: more than the pipeline keeps in flight, so slots are waited for, copied out and taken again)
    log2 = []
    rep_p = eval_scenes_reduced(m, ds, 7, traj_scale=1.3, scenes_per_call=per_call, z_fn=_z_fn(scenes.latents(72, n * 7), log2),
                                miss_threshold=thr, **kw)
    assert [r for _, r in log2] == [s for s in sizes for _ in range(7)]
    assert rep_p.n_agents == n and np.isfinite(rep_p.scene_ade).all() and rep_p.best_idx.max() < K


def test_one_round_first_init_is_eval_scenes_report():
    """rounds = 1, K = sample_k, init 'first': the reduction is the identity, so the loop is eval_scenes_report."""
    from sttode_amd import scenes
    from sttode_amd.evaluate import eval_scenes_reduced, eval_scenes_report
    m = _model('eth')
    ds = _dataset(range(5200, 5290), 'eth')
    n = int(ds.obs_traj.shape[0])
    zall = scenes.latents(73, n)
    kw = dict(traj_scale=1.3, scenes_per_call=40, miss_threshold=0.8)
    ser = eval_scenes_reduced(m, ds, 1, z_fn=_z_fn(zall), pipelined=False, **kw)
    _reports_equal(ser, eval_scenes_report(m, ds, z_fn=_z_fn(zall), pipelined=False, **kw), 'serial, one round')
    pip = eval_scenes_reduced(m, ds, 1, z_fn=_z_fn(zall), pipelined=True, **kw)
    ref = eval_scenes_report(m, ds, z_fn=_z_fn(zall), pipelined=True, **kw)
    np.testing.assert_allclose(pip.scene_ade, ref.scene_ade, rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(pip.scene_fde, ref.scene_fde, rtol=1e-5, atol=1e-6)
    assert abs(pip.ade - ref.ade) <= 1e-5 * (1 + ref.ade) and abs(pip.fde - ref.fde) <= 1e-5 * (1 + ref.fde)
    assert pip.n_agents == ref.n_agents == n and (pip.scene_agents == ref.scene_agents).all()
