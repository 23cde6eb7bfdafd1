"""GPU tests of the scene-level oversample-and-reduce (sttode_reduce_scenes, csrc/reduce_scenes.hip) against the float64
yardstick of tests/test_reduce.py applied to scene futures (tests/test_reduce_scenes.py).  What is compared, and why not more, is that
module's near-tie rule: full runs on the stored seeds whose every margin holds (labels and counts exactly equal, no sample left out); one
Lloyd step from a caller's init on the shapes the kernel branches on (labels equal wherever the float64 margin is >= 1e-3, at most 1 % of a
segment left out); the centroids always against float64 means over the DEVICE's labels within M * 2^-24 * max |coordinate| (the bound of a
sequential fp32 sum, tests/test_reduce.py centroid_atol).  Then the identities the contract promises, bit for bit, and the layers above:
metrics.reduce_scenes, STTODENet.inference_reduced(level='scene'), evaluate.eval_scenes_reduced(level=, joint=, collision_radius=, kde=)."""
import numpy as np
import pytest
import torch

from test_reduce import ONE_STEP_CAP, centroid_atol, make_samples, means_over_labels
from test_reduce_gpu import _dataset, _gpu, _model, _reports_equal, _set, _z_fn
from test_reduce_scenes import CASES, SHAPES, seg_ptr_of, shape_case

pytestmark = pytest.mark.gpu


def _rs(x, sp, K, **kw):
    """metrics.reduce_scenes of a NumPy / torch input -> (centroids, labels, counts) as NumPy arrays and the SceneReduction."""
    from sttode_amd import metrics
    t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.array(x))              # (a copy: the shared cases are read-only)
    if 'init' in kw and isinstance(kw['init'], np.ndarray):
        kw['init'] = torch.from_numpy(np.array(kw['init'])).to(_gpu())
    red = metrics.reduce_scenes(t.to(_gpu()), sp, K, **kw)
    torch.cuda.synchronize()
    return red.centroids.cpu().numpy(), red.labels.cpu().numpy(), red.counts.cpu().numpy(), red


def _ra(x, K, **kw):
    from sttode_amd import metrics
    if 'init' in kw and isinstance(kw['init'], np.ndarray):
        kw['init'] = torch.from_numpy(np.array(kw['init'])).to(_gpu())
    red = metrics.reduce_samples(torch.from_numpy(np.array(x)).to(_gpu()), K, **kw)
    torch.cuda.synchronize()
    return red.centroids.cpu().numpy(), red.labels.cpu().numpy(), red.counts.cpu().numpy(), red


def _same_bits(a, b, what):
    for u, v, f in zip(a[:3], b[:3], ('centroids', 'labels', 'counts')):
        assert u.dtype == v.dtype and u.shape == v.shape and u.tobytes() == v.tobytes(), (what, f)


def _check_centroids(x, sp, prev, cent, lab, cnt, what):
    """Per segment: counts are the label histogram; per agent of it a non-empty cluster's centroid is the float64 mean over the device's own
    labels within M * 2^-24 * max |coordinate|; an empty cluster has the bits of `prev`, the centroids one iteration earlier (None: not
    known here)."""
    S, K = cnt.shape
    for s in range(S):
        if sp[s + 1] == sp[s]:
            continue
        assert lab[s].min() >= 0 and lab[s].max() < K, what
        np.testing.assert_array_equal(cnt[s], np.bincount(lab[s], minlength=K), err_msg=what)
        full = cnt[s] > 0
        for a in range(sp[s], sp[s + 1]):
            ref = means_over_labels(x[a], lab[s], K, np.zeros_like(cent[a]) if prev is None else prev[a])
            np.testing.assert_allclose(cent[a][full], ref[full], rtol=0, atol=centroid_atol(x[a]), err_msg=what)
            if prev is not None:
                assert cent[a][~full].tobytes() == np.ascontiguousarray(prev[a][~full]).tobytes(), what


# ----- against the yardstick -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('tag', sorted(CASES))
def test_full_runs_on_the_stored_seeds(golden, tag):
    """iters = 10 from 'first' / 'maximin': every label and count equals the yardstick's (every sample's margin holds at every iteration,
    tests/test_reduce_scenes.py re-asserts it), the centroids agree with the yardstick's and with float64 means over the device's labels."""
    g = golden('reduce_scenes')
    _, sizes, M, K, Tf, t0, init = CASES[tag]
    sp = g[tag + '/seg_ptr']
    x = np.concatenate([make_samples(int(seed), A, M, Tf) for seed, A in zip(g[tag + '/seeds'], sizes)])
    out = _rs(x, sp, K, iters=10, from_frame=t0, init=init)
    np.testing.assert_array_equal(out[1], g[tag + '/labels'], err_msg=tag)
    np.testing.assert_array_equal(out[2], g[tag + '/counts'], err_msg=tag)
    _check_centroids(x, sp, g[tag + '/init'], out[0], out[1], out[2], tag)
    for a in range(x.shape[0]):
        np.testing.assert_allclose(out[0][a], g[tag + '/centroids'][a], rtol=0, atol=centroid_atol(x[a]), err_msg=tag)
    # the same run from the stored initial centroids as a caller's init: for maximin this pins the picks (the yardstick's, all of them)
    _same_bits(out, _rs(x, sp, K, iters=10, from_frame=t0, init=g[tag + '/init']), tag + ': init as a tensor')
    if t0 == Tf - 1:
        _same_bits(out, _rs(x, sp, K, iters=10, from_frame=-1, init=init), tag + ': from_frame = -1')
    _same_bits(out, _rs(x, torch.from_numpy(sp).to(_gpu()), K, iters=10, from_frame=t0, init=init), tag + ': seg_ptr on the device')


@pytest.mark.parametrize('tag', sorted(SHAPES))
def test_shapes_one_step_chain_and_layout(golden, tag):
    """Per shape: one step from a caller's init against the yardstick (labels equal on the samples that hold the margin; centroids against
    float64 means over the device's own labels); two runs give the same bits; the round-major [R, n, K_in, Tf, 2] layout equals the same
    samples given as [n, M, Tf, 2]; iters = 3 equals three chained iters = 1 calls that pass the centroids on as init (an empty cluster
    therefore keeps its bits); ten iterations from 'first' and 'maximin' end with valid labels and centroids that are their means."""
    _, sizes, R, K_in, K, Tf, t0 = SHAPES[tag]
    M, n, sp = R * K_in, sum(sizes), seg_ptr_of(sizes)
    x, init, c, lab, cnt, sure = shape_case(tag, golden('reduce_scenes')[tag + '/seeds'])
    x5 = np.ascontiguousarray(x.reshape(n, R, K_in, Tf, 2).transpose(1, 0, 2, 3, 4))     # sample m = r K_in + k
    out = _rs(x5, sp, K, iters=1, from_frame=t0, init=init)
    assert (1.0 - sure.mean(axis=1)).max() <= ONE_STEP_CAP, tag
    np.testing.assert_array_equal(out[1][sure], lab[sure], err_msg=tag)
    _check_centroids(x, sp, init, out[0], out[1], out[2], tag)
    for s in range(len(sizes)):
        if (out[1][s] == lab[s]).all():
            for a in range(sp[s], sp[s + 1]):
                np.testing.assert_allclose(out[0][a], c[a], rtol=0, atol=centroid_atol(x[a]), err_msg=tag)
    _same_bits(out, _rs(x5, sp, K, iters=1, from_frame=t0, init=init), tag + ': second run')
    _same_bits(out, _rs(x, sp, K, iters=1, from_frame=t0, init=init), tag + ': [n, M, Tf, 2] layout')
    if t0 == Tf - 1:
        _same_bits(out, _rs(x5, sp, K, iters=1, from_frame=-1, init=init), tag + ': from_frame = -1')
    whole = _rs(x5, sp, K, iters=3, from_frame=t0, init=init)
    second = _rs(x5, sp, K, iters=1, from_frame=t0, init=out[0])
    third = _rs(x5, sp, K, iters=1, from_frame=t0, init=second[0])
    _same_bits(whole, third, tag + ': iters = 3 against three chained calls')
    _check_centroids(x, sp, second[0], *whole[:3], tag + ': after three iterations')
    for kw in ({'iters': 10, 'init': 'first'}, {'iters': 10, 'init': 'maximin'}):
        _check_centroids(x, sp, None, *_rs(x5, sp, K, from_frame=t0, **kw)[:3], f'{tag}: {kw["init"]}, ten iterations')


# ----- exact identities ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('n,R,K_in,K,Tf,t0', [(7, 1, 70, 7, 12, 0), (5, 3, 20, 20, 12, 5), (3, 27, 19, 20, 13, 12), (2, 1, 1024, 64, 12, 0)])
def test_one_agent_segments_have_the_bits_of_reduce_samples(n, R, K_in, K, Tf, t0):
    M = R * K_in
    x = make_samples(51, n, M, Tf)
    x5 = np.ascontiguousarray(x.reshape(n, R, K_in, Tf, 2).transpose(1, 0, 2, 3, 4))
    sp = np.arange(n + 1, dtype=np.int32)
    for init in ('first', 'maximin', np.ascontiguousarray(x[:, M - K:])):
        for iters in (1, 10):
            a = _ra(x5, K, iters=iters, from_frame=t0, init=init)
            b = _rs(x5, sp, K, iters=iters, from_frame=t0, init=init)
            assert torch.equal(a[3].centroids, b[3].centroids) and torch.equal(a[3].labels, b[3].labels), (init if isinstance(init, str) else 'init', iters)
            assert torch.equal(a[3].counts, b[3].counts) and torch.equal(a[3].weights, b[3].weights) and torch.equal(a[3].weights, b[3].agent_weights)


@pytest.mark.parametrize('A', [2, 4])
def test_a_segment_of_copies_is_its_agent(A):
    """A copies of one agent: every distance is A times the agent's, exactly (a float64 holds A fp32 values' sum), so the labels are the
    per-agent labels and every copy has the agent's centroids, bit for bit."""
    M, K, Tf = 70, 7, 12
    x = make_samples(53, 3, M, Tf)
    xc = np.repeat(x, A, axis=0)                                        # segments (a, a, ..), (b, b, ..), (c, c, ..)
    sp = np.arange(0, 3 * A + 1, A, dtype=np.int32)
    for init in ('first', 'maximin', np.ascontiguousarray(x[:, 20:20 + K])):
        ref = _ra(x, K, iters=10, from_frame=3, init=init)
        out = _rs(xc, sp, K, iters=10, from_frame=3, init=np.repeat(init, A, axis=0) if isinstance(init, np.ndarray) else init)
        assert out[1].tobytes() == ref[1].tobytes() and out[2].tobytes() == ref[2].tobytes()
        for j in range(A):
            assert np.ascontiguousarray(out[0][j::A]).tobytes() == ref[0].tobytes(), (A, j)


def test_a_segment_alone_appended_to_prefixed_and_beside_an_empty_one():
    """A segment's outputs are the same bits alone, with segments appended behind it, with one to three agents in front of it, and next to
    an empty segment; the empty segment gets labels 0 and counts (M, 0, ..) and touches no centroid."""
    M, K, Tf, A = 70, 7, 12, 18
    x = make_samples(57, A + 9, M, Tf)
    seg, rest = x[:A], x[A:]
    for init in ('first', 'maximin', np.ascontiguousarray(x[:, 10:10 + K])):
        def kw(sl):
            return dict(iters=10, from_frame=2, init=init if isinstance(init, str) else np.ascontiguousarray(init[sl]))
        alone = _rs(seg, [0, A], K, **kw(slice(0, A)))
        tail = _rs(x, [0, A, A + 4, A + 9], K, **kw(slice(None)))
        _same_bits(alone, (tail[0][:A], tail[1][:1], tail[2][:1]), 'segments appended')
        for f in (1, 2, 3):
            order = np.r_[A:A + f, 0:A]
            pre = _rs(x[order], [0, f, f + A], K, **kw(order))
            _same_bits(alone, (pre[0][f:], pre[1][1:], pre[2][1:]), f'{f} agents in front')
        empty = _rs(x, [0, A, A, A + 9], K, **kw(slice(None)))
        both = _rs(x, [0, A, A + 9], K, **kw(slice(None)))
        _same_bits(alone, (empty[0][:A], empty[1][:1], empty[2][:1]), 'in front of an empty segment')
        _same_bits((both[0][A:], both[1][1:], both[2][1:]), (empty[0][A:], empty[1][2:], empty[2][2:]), 'behind an empty segment')
        assert (empty[1][1] == 0).all() and empty[2][1].tolist() == [M] + [0] * (K - 1)
        assert empty[3].agent_weights.shape == (A + 9, K) and torch.equal(empty[3].agent_weights[A:], empty[3].weights[2].expand(9, K))
    # an empty segment touches no centroid: every segment empty but one, sentinels elsewhere
    from sttode_amd import capi
    dev = _gpu()
    cent = torch.full((A + 9, K, Tf, 2), -7.0, device=dev)
    lab = torch.full((3, M), -7, dtype=torch.int32, device=dev)
    cnt = torch.full((3, K), -7, dtype=torch.int32, device=dev)
    sp = torch.tensor([0, 0, A, A], dtype=torch.int32, device=dev)
    capi.call('sttode_reduce_scenes', torch.from_numpy(x).to(dev), A + 9, 1, M, Tf, K, 10, 2, 0, None, sp, 3, cent, lab, cnt, capi.stream_ptr())
    torch.cuda.synchronize()
    assert (cent[A:] == -7).all() and torch.isfinite(cent[:A]).all() and (cent[:A] != -7).any()
    assert (lab[0] == 0).all() and (lab[2] == 0).all() and cnt[0].tolist() == cnt[2].tolist() == [M] + [0] * (K - 1)
    first = _rs(seg, [0, A], K, iters=10, from_frame=2, init='first')
    assert cent[:A].cpu().numpy().tobytes() == first[0].tobytes() and lab[1].cpu().numpy().tobytes() == first[1][0].tobytes()


def test_labels_are_joint():
    """A two-agent segment: agent 0's samples are all equal, agent 1's form K separated groups.  The segment's labels are agent 1's groups
    -- for both agents -- where the per-agent reduction gives agent 0 one cluster (all its distances tie: the lowest k)."""
    M, K, Tf = 40, 4, 12
    rng = np.random.default_rng(3)
    x = np.empty((2, M, Tf, 2), np.float32)
    x[0] = (np.arange(Tf, dtype=np.float32) * 0.5)[None, :, None]
    grp = np.arange(M) % K
    x[1] = (10.0 * grp[:, None, None] + rng.normal(0, 0.1, (M, Tf, 2))).astype(np.float32)
    for init in ('first', 'maximin'):
        out = _rs(x, [0, 2], K, iters=10, init=init)
        per = _ra(x, K, iters=10, init=init)
        same_group = out[1][0][:, None] == out[1][0][None, :]
        assert (same_group == (grp[:, None] == grp[None, :])).all() and out[2][0].tolist() == [M // K] * K, init
        assert (per[1][0] == 0).all() and (per[1][0] != out[1][0]).any()
        assert (out[1][0] == per[1][1]).all()                                        # agent 1 alone finds its groups as well
        np.testing.assert_allclose(out[0][0], np.broadcast_to(x[0, :1], (K, Tf, 2)), rtol=0, atol=centroid_atol(x[0]))
        _check_centroids(x, [0, 2], None, *out[:3], 'joint labels')


# ----- robustness ------------------------------------------------------------------------------------------------------------------------

def test_outputs_beyond_the_extent_are_untouched_and_limits_write_nothing():
    from sttode_amd import capi
    dev = _gpu()
    n, R, K_in, K, Tf, S = 9, 3, 20, 7, 12, 3
    M = R * K_in
    x = torch.from_numpy(make_samples(41, n, M, Tf).reshape(n, R, K_in, Tf, 2).transpose(1, 0, 2, 3, 4).copy()).to(dev)
    sp = torch.tensor([0, 2, 3, 9], dtype=torch.int32, device=dev)
    pad = 64
    cent = torch.full((pad + n * K * Tf * 2 + pad,), -7.0, device=dev)
    lab = torch.full((pad + S * M + pad,), -7, dtype=torch.int32, device=dev)
    cnt = torch.full((pad + S * K + pad,), -7, dtype=torch.int32, device=dev)
    args = lambda **kw: (x, kw.get('n', n), R, K_in, Tf, kw.get('K', K), kw.get('iters', 10), kw.get('t0', 0), kw.get('mode', 1), None,
                         sp, kw.get('S', S), cent[pad:], lab[pad:], cnt[pad:], capi.stream_ptr())
    for bad, match in (({'K': 65}, 'K must be'), ({'K': 61}, 'M = R K_in'), ({'iters': 0}, 'iters'), ({'t0': 12}, 'from_frame'),
                       ({'mode': 2}, 'init must be'), ({'n': 0}, 'n must be'), ({'S': 0}, 'S must be')):
        with pytest.raises(capi.SttodeError, match='sttode_reduce_scenes.*' + match):
            capi.call('sttode_reduce_scenes', *args(**bad))
    torch.cuda.synchronize()
    assert (cent == -7).all() and (lab == -7).all() and (cnt == -7).all()
    for mode in (1, 0):
        capi.call('sttode_reduce_scenes', *args(mode=mode))
        torch.cuda.synchronize()
        for t, size in ((cent, n * K * Tf * 2), (lab, S * M), (cnt, S * K)):
            assert (t[:pad] == -7).all() and (t[pad + size:] == -7).all()
        l = lab[pad:pad + S * M]
        assert l.min() >= 0 and l.max() < K and int(cnt[pad:pad + S * K].sum()) == S * M and torch.isfinite(cent[pad:pad + n * K * Tf * 2]).all()


def test_non_finite_inputs_keep_the_labels_in_range():
    x = make_samples(43, 9, 70, 12)
    x[0, 5] = np.nan
    x[1, :, 3] = np.inf
    x[4, 0] = -np.inf
    x[4, 1] = np.nan
    x[8] = np.nan
    for init in ('first', 'maximin'):
        out = _rs(x, [0, 3, 4, 6, 9], 7, iters=5, init=init)
        assert out[1].min() >= 0 and out[1].max() < 7 and (out[2] >= 0).all() and (out[2].sum(axis=1) == 70).all()


def test_python_layer_arguments():
    from sttode_amd import metrics
    dev = _gpu()
    x = torch.from_numpy(make_samples(47, 6, 40, 12)).to(dev)
    red = metrics.reduce_scenes(x, [0, 2, 6], 5, from_frame=-12)
    assert red.centroids.shape == (6, 5, 12, 2) and red.labels.shape == (2, 40) and red.labels.dtype == torch.int32
    assert red.counts.shape == (2, 5) and red.weights.dtype == torch.float32 and red.agent_weights.shape == (6, 5)
    assert torch.equal(red.weights, red.counts.float() / 40) and torch.allclose(red.weights.sum(dim=1), torch.ones(2, device=dev))
    assert torch.equal(red.agent_weights, red.weights[torch.tensor([0, 0, 1, 1, 1, 1], device=dev)])
    assert torch.equal(red.centroids, metrics.reduce_scenes(x, [0, 2, 6], 5, from_frame=0).centroids)
    assert torch.equal(red.centroids, metrics.reduce_scenes(x.double(), np.array([0, 2, 6]), 5).centroids)            # converted to float32
    uni = metrics.reduce_scenes(x, K=5, seg_len=3)
    assert torch.equal(uni.centroids, metrics.reduce_scenes(x, [0, 3, 6], 5).centroids) and uni.seg_ptr.tolist() == [0, 3, 6]
    for bad in (dict(seg_ptr=[0, 2, 6], K=0), dict(seg_ptr=[0, 2, 6], K=65), dict(seg_ptr=[0, 2, 6], K=41), dict(seg_ptr=[0, 2, 6], K=5, from_frame=12),
                dict(seg_ptr=[0, 2, 6], K=5, from_frame=-13), dict(seg_ptr=[0, 2, 6], K=5, init='kmeans++'), dict(seg_ptr=[0, 2, 6], K=5, iters=0),
                dict(seg_ptr=[0, 2, 6], K=5, init=torch.zeros(6, 6, 12, 2, device=dev)), dict(seg_ptr=[1, 2, 6], K=5), dict(seg_ptr=[0, 2, 5], K=5),
                dict(seg_ptr=[0, 4, 2, 6], K=5), dict(seg_ptr=[0], K=5), dict(K=5), dict(seg_ptr=[0, 6], K=5, seg_len=3), dict(K=5, seg_len=4),
                dict(K=5, seg_len=0), dict(seg_ptr=[0, 6])):
        with pytest.raises(ValueError):
            metrics.reduce_scenes(x, **bad)
    with pytest.raises(ValueError):
        metrics.reduce_scenes(x[0], [0, 6], 5)


# ----- the layers above ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('mode', ['scenes', 'one_scene', 'nba'])
def test_inference_reduced_at_scene_level_is_the_composition(mode):
    from sttode_amd import metrics, scenes
    m = _model('nba', 5, 10) if mode == 'nba' else _model('eth')
    n = _set(m, mode)
    Ks, rounds = m.args.sample_k, 3
    z = torch.from_numpy(scenes.latents(61, n * rounds).reshape(rounds, n * Ks, -1)).to(m.device)
    seg = dict(seg_len=11) if mode == 'nba' else dict(seg_ptr=m._scene_ptr.clone())
    S = n // 11 if mode == 'nba' else int(seg['seg_ptr'].numel()) - 1
    for kw in (dict(K=None, iters=10, from_frame=0, init='first'), dict(K=7, iters=4, from_frame=-1, init='maximin')):
        out = m.inference_reduced(rounds, z=z, level='scene', **kw)
        red = m.reduction
        K = Ks if kw['K'] is None else kw['K']
        assert isinstance(red, metrics.SceneReduction) and out.shape == (K, n, m.args.future_length, 2) and m.diverse_pred is red.centroids
        assert torch.equal(out, red.centroids.permute(1, 0, 2, 3)) and red.labels.shape == (S, rounds * Ks)
        stack = torch.stack([m.inference(None, z=z[r]).permute(1, 0, 2, 3).contiguous() for r in range(rounds)])
        ref = metrics.reduce_scenes(stack, K=K, **seg, **{k: v for k, v in kw.items() if k != 'K'})
        assert torch.equal(red.centroids, ref.centroids) and torch.equal(red.labels, ref.labels) and torch.equal(red.counts, ref.counts)
        assert torch.equal(red.agent_weights, ref.agent_weights) and int(red.counts.sum()) == S * rounds * Ks
        _set(m, mode)
        m.inference_reduced(rounds, z=z, **kw)                                            # the default level is the per-agent reduction
        assert isinstance(m.reduction, metrics.Reduction) and m.reduction.labels.shape == (n, rounds * Ks)
        _set(m, mode)
    with pytest.raises(ValueError, match='level'):
        m.inference_reduced(rounds, z=z, level='game')


def test_eval_scenes_reduced_scene_level_against_a_hand_written_loop():
    from sttode_amd import metrics, scenes
    from sttode_amd.evaluate import _ReportAcc, eval_scenes_reduced
    m = _model('eth')
    ds = _dataset(range(5200, 5290), 'eth')
    n, Ks = int(ds.obs_traj.shape[0]), m.args.sample_k
    rounds, K, per_call, thr, rad = 3, 7, 40, 0.8, 0.3
    zall = scenes.latents(71, n * rounds)
    kw = dict(K=K, iters=5, from_frame=-1, init='maximin')
    rep = eval_scenes_reduced(m, ds, rounds, traj_scale=1.3, scenes_per_call=per_call, z_fn=_z_fn(zall), pipelined=False, miss_threshold=thr,
                              weighted=True, ks=(1, 5), level='scene', joint=True, collision_radius=rad, kde=True, **kw)
    acc, z_fn = _ReportAcc(thr, joint=True, kde=True, collision_radius=rad, K=K, ks=(1, 5), weighted=True), _z_fn(zall)
    agent = _ReportAcc(thr, joint=True, kde=True, collision_radius=rad, K=K, ks=(1, 5), weighted=True)
    plain = _ReportAcc(thr, K=K)
    for s0 in range(0, len(ds), per_call):
        sb = ds.scene_batch(range(s0, min(s0 + per_call, len(ds))))
        m.set_scene_batch(sb.past, sb.future, sb.scene_ptr)
        stack = torch.stack([m.inference(None, z=z_fn(sb.n_agents * Ks)).permute(1, 0, 2, 3).contiguous() for _ in range(rounds)])
        red = metrics.reduce_scenes(stack, sb.scene_ptr, K, iters=5, from_frame=-1, init='maximin')
        per = metrics.reduce_samples(stack, K, iters=5, from_frame=-1, init='maximin')
        for a, r, w in ((acc, red, red.agent_weights), (agent, per, per.weights)):
            a.add(m.select_best_of_k(r.centroids, scale=1.3, miss_threshold=thr, seg_ptr=m._scene_ptr), sb.scene_ptr)
            a.add_scene_metrics(m.select_joint(r.centroids, seg_ptr=m._scene_ptr, scale=1.3, collision_radius=rad), m.kde_nll(r.centroids, scale=1.3))
            a.add_weighted(m.weighted_set(r.centroids, w, scale=1.3))
        plain.add(m.select_best_of_k(per.centroids, scale=1.3, miss_threshold=thr, seg_ptr=m._scene_ptr), sb.scene_ptr)
    _reports_equal(rep, acc.report(False), 'scene level against the loop')
    assert rep.n_agents == n and len(rep.scene_joint_ade) == len(ds) and rep.scene_joint_idx.max() < K and rep.scene_collision.shape == (len(ds), 2)
    assert (rep.scene_joint_ade >= rep.scene_ade * (1 - 1e-6)).all() and 0.0 <= rep.collision_rate <= 1.0   # per scene: min of a mean >= mean of minima
    # the same keywords on the per-agent reduction: the joint numbers of per-agent representatives, beside the scene-level ones
    rep_a = eval_scenes_reduced(m, ds, rounds, traj_scale=1.3, scenes_per_call=per_call, z_fn=_z_fn(zall), pipelined=False, miss_threshold=thr,
                                weighted=True, ks=(1, 5), joint=True, collision_radius=rad, kde=True, **kw)
    _reports_equal(rep_a, agent.report(False), 'agent level with the scene metrics against the loop')
    # every new keyword at its default, and spelled out: the report the loop gave before
    for extra in ({}, dict(level='agent', joint=False, collision_radius=None, kde=False)):
        rep_d = eval_scenes_reduced(m, ds, rounds, traj_scale=1.3, scenes_per_call=per_call, z_fn=_z_fn(zall), pipelined=False,
                                    miss_threshold=thr, **kw, **extra)
        _reports_equal(rep_d, plain.report(False), 'defaults against the loop as it was')
        assert rep_d.joint_ade is None and rep_d.collision_rate is None and rep_d.kde_nll is None
    # the pipelined loop at scene level: a report of the same shape
    rep_p = eval_scenes_reduced(m, ds, 7, traj_scale=1.3, scenes_per_call=per_call, z_fn=_z_fn(scenes.latents(72, n * 7)), miss_threshold=thr,
                                level='scene', joint=True, **kw)
    assert rep_p.n_agents == n and np.isfinite(rep_p.scene_joint_ade).all() and rep_p.collision_rate is None


def test_one_round_first_init_at_scene_level_is_eval_scenes_report():
    """rounds = 1, K = sample_k, init 'first', level='scene': each cluster is one scene future, so the centroids are the samples and every
    field, the joint ones included, is eval_scenes_report's."""
    from sttode_amd import scenes
    from sttode_amd.evaluate import eval_scenes_reduced, eval_scenes_report
    m = _model('eth')
    ds = _dataset(range(5200, 5290), 'eth')
    zall = scenes.latents(73, int(ds.obs_traj.shape[0]))
    kw = dict(traj_scale=1.3, scenes_per_call=40, miss_threshold=0.8, joint=True, collision_radius=0.3, kde=True)
    red = eval_scenes_reduced(m, ds, 1, z_fn=_z_fn(zall), pipelined=False, level='scene', **kw)
    ref = eval_scenes_report(m, ds, z_fn=_z_fn(zall), pipelined=False, **kw)
    _reports_equal(red, ref, 'scene level, one round')
    assert red.joint_ade == ref.joint_ade and red.scene_joint_idx.tobytes() == ref.scene_joint_idx.tobytes()
