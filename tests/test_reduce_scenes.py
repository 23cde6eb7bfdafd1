"""CPU tests of the scene-level oversample-and-reduce (sttode_reduce_scenes, csrc/reduce_scenes.hip).

The yardstick is tests/test_reduce.py's own float64 ``kmeans_f64`` / ``maximin_f64`` / ``margins`` (pinned there to
scipy.cluster.vq.kmeans2), imported, applied to a segment's samples laid out as scene futures: x_seg [A, M, Tf, 2] becomes
``np.moveaxis(x_seg, 0, 2).reshape(M, Tf, 2 A)`` -- a sample is a point of R^(A 2 Tf), the frame slice stays on axis 1.

Near-ties: that module's rule carries over with its reason.  A per-agent fp32 squared distance carries a relative error of about
(2 Tf) 2^-24; the float64 sum of positive terms over the agents does not raise it, so MARGIN = 1e-3 stays two orders above what fp32 can
flip.  The stored full-run cases are seeds on which EVERY sample holds the margin at EVERY iteration (and every maximin pick does); a
one-step case may leave out at most ONE_STEP_CAP = 1 % of a segment's samples.  Both are conditions on the inputs:
tests/golden/make_reduce_scenes_golden.py searches the seeds, the tests here assert them on the yardstick alone."""
import ctypes
import inspect

import numpy as np
import pytest

from test_reduce import MARGIN, ONE_STEP_CAP, kmeans_f64, make_samples, maximin_f64

ENTRY = 'sttode_reduce_scenes'


# ----- a segment as scene futures ----------------------------------------------------------------------------------------------------------

def scene_points(x_seg):
    """x_seg [A, M, Tf, 2] -> [M, Tf, 2 A]: sample m of the segment as one point per frame."""
    A, M, Tf = x_seg.shape[:3]
    return np.moveaxis(x_seg, 0, 2).reshape(M, Tf, 2 * A)


def agent_form(c, A):
    """[K, Tf, 2 A] -> [A, K, Tf, 2]: the inverse of scene_points for centroids."""
    K, Tf = c.shape[:2]
    return np.ascontiguousarray(np.moveaxis(c.reshape(K, Tf, A, 2), 2, 0))


def scene_kmeans_f64(x_seg, init, iters, t0=0):
    """The contract for ONE segment in float64: x_seg [A, M, Tf, 2], init [A, K, Tf, 2] -> (centroids [A, K, Tf, 2] f64, labels [M],
    counts [K], margin [iters, M])."""
    c, lab, cnt, marg = kmeans_f64(scene_points(np.asarray(x_seg)), scene_points(np.asarray(init)), iters, t0)
    return agent_form(c, x_seg.shape[0]), lab, cnt, marg


def segment_case(seed, A, M, K, Tf, t0, init, kind):
    """One segment of a case from its seed, as tests/test_reduce.py's case_agent: (x_seg, init [A,K,Tf,2] f32, iters, yardstick outputs, ok)."""
    x = make_samples(seed, A, M, Tf)
    if kind == 'step':
        c0 = scene_kmeans_f64(x, x[:, :K], 3, t0)[0].astype(np.float32)
        out = scene_kmeans_f64(x, c0, 1, t0)
        return x, c0, 1, out, (out[3] < MARGIN).mean() <= ONE_STEP_CAP
    ok = True
    if init == 'maximin':
        chosen, mm = maximin_f64(scene_points(x), K, t0)
        c0, ok = np.ascontiguousarray(x[:, chosen]), mm >= MARGIN
    else:
        c0 = np.ascontiguousarray(x[:, :K])
    out = scene_kmeans_f64(x, c0, 10, t0)
    return x, c0, 10, out, bool(ok and out[3].min() >= MARGIN)


# the stored full-run cases (iters = 10, every margin held): tag -> (seed-search start, segment sizes, M, K, Tf, from_frame, init)
CASES = {
    'sizes_1_2_3_7_m40_k5': (100, (1, 2, 3, 7), 40, 5, 12, 0, 'first'),
    'size_17_m64_k20_mid': (200, (17,), 64, 20, 12, 5, 'first'),
    'sizes_65_1_4_m40_k5_end': (300, (65, 1, 4), 40, 5, 12, 11, 'first'),
    'sizes_1_2_3_7_m64_k5_maximin': (400, (1, 2, 3, 7), 64, 5, 12, 0, 'maximin'),
    'sizes_17_2_m40_k20_maximin_end': (500, (17, 2), 40, 20, 12, 11, 'maximin'),
}

# one-step cases, regenerated at test time from the seeds the maker found (one per segment): tag -> (seed-search start, segment sizes, R,
# K_in, K, Tf, from_frame); M = R K_in.  The shapes are the smallest on either side of what the kernel branches on: 64-sample chunks
# (64 / 70), samples per lane and blocks of samples (256 / 257, 512 / 513, 1024), the centroids held per pass (K = 4 / 5, 12 / 13, 20 / 21,
# 64: four passes), the 24-float chunks of a row (Tf = 1, 12, 13, 20, 80), the batches of 16 agents (4 at Tf = 80) whose centroids are staged
# together (segments of 1, 4, 5, 16, 17, 64, 65, 300; 13 at Tf = 80), one workgroup and a few hundred.
SHAPES = {
    'a1_m64_k5_tf1': (1000, (1,), 1, 64, 5, 1, 0),
    'a3_m64_k4': (1050, (3,), 1, 64, 4, 12, 0),
    'a2_a3_m70_k12': (1060, (2, 3), 1, 70, 12, 12, 0),
    'a3_a2_m70_k13': (1070, (3, 2), 1, 70, 13, 12, 4),
    'a3_m64_k21': (1080, (3,), 1, 64, 21, 12, 0),
    'a4_a5_a16_m70_k7_tf13_mid': (1100, (4, 5, 16), 1, 70, 7, 13, 6),
    'a13_m64_k5_tf80': (1200, (13,), 2, 32, 5, 80, 0),
    'a64_a65_m256_k20': (1300, (64, 65), 4, 64, 20, 12, 0),
    'a65_m257_k7_tf20_end': (1400, (65,), 1, 257, 7, 20, 19),
    'a17_m512_k20': (1500, (17,), 2, 256, 20, 12, 3),
    'a65_m513_k20': (1600, (65,), 27, 19, 20, 12, 0),
    'a17_m1024_k64': (1700, (17,), 1, 1024, 64, 12, 0),
    'a300_m257_k7': (1800, (300,), 1, 257, 7, 12, 0),
    's300_small_m64_k5': (2000, tuple(1 + i % 3 for i in range(300)), 1, 64, 5, 12, 0),
}
_SHAPE_CACHE = {}


def seg_ptr_of(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)


def shape_case(tag, seeds):
    """(x [n,M,Tf,2] f32, init [n,K,Tf,2] f32 -- per segment the yardstick's centroids after 3 float64 iterations from 'first' --, and the
    yardstick's ONE step from there: centroids [n,K,Tf,2] f64, labels [S,M], counts [S,K], sure [S,M] = margin >= 1e-3).  Once per process."""
    if tag not in _SHAPE_CACHE:
        _, sizes, R, K_in, K, Tf, t0 = SHAPES[tag]
        res = [segment_case(int(seed), A, R * K_in, K, Tf, t0, None, 'step') for seed, A in zip(seeds, sizes)]
        out = (np.concatenate([r[0] for r in res]), np.concatenate([r[1] for r in res]), np.concatenate([r[3][0] for r in res]),
               np.stack([r[3][1] for r in res]), np.stack([r[3][2] for r in res]), np.stack([r[3][3][0] >= MARGIN for r in res]))
        for v in out:
            v.setflags(write=False)
        _SHAPE_CACHE[tag] = out
    return _SHAPE_CACHE[tag]


# ----- the yardstick and the stored cases ------------------------------------------------------------------------------------------------

def test_scene_restatement_is_scipy_kmeans2(golden):
    """The [M, Tf, 2 A] restatement against scipy.cluster.vq.kmeans2 directly on one stored case: labels equal, the sliced code book to
    1e-12, and the centroids come back in agent form."""
    vq = pytest.importorskip('scipy.cluster.vq')
    g = golden('reduce_scenes')
    tag = 'sizes_1_2_3_7_m40_k5'
    _, sizes, M, K, Tf, t0, init = CASES[tag]
    A, seed = sizes[3], int(g[tag + '/seeds'][3])
    x, c0, iters, (c, lab, cnt, marg), ok = segment_case(seed, A, M, K, Tf, t0, init, 'full')
    pts = scene_points(x).astype(np.float64)
    assert pts.shape == (M, Tf, 2 * A) and (pts[5, 3, 2 * 4:2 * 4 + 2] == x[4, 5, 3]).all()
    book, code = vq.kmeans2(pts[:, t0:].reshape(M, -1), scene_points(c0).astype(np.float64)[:, t0:].reshape(K, -1), iter=iters, minit='matrix')
    np.testing.assert_array_equal(lab, code)
    np.testing.assert_allclose(scene_points(c)[:, t0:].reshape(K, -1), book, rtol=0, atol=1e-12 * np.abs(x).max())
    assert (agent_form(scene_points(c0), A) == c0).all() and cnt.sum() == M


def test_stored_cases_match_the_yardstick_and_hold_their_margins(golden):
    """reduce_scenes.npz is what make_reduce_scenes_golden.py writes from CASES and SHAPES: the inputs regenerate from the stored seeds, the
    stored outputs are the yardstick's, every full-run sample holds the margin at every iteration (every maximin pick too)."""
    g = golden('reduce_scenes')
    assert sorted(map(str, g['cases'])) == sorted(CASES) and sorted(map(str, g['shapes'])) == sorted(SHAPES)
    for tag, (_, sizes, M, K, Tf, t0, init) in CASES.items():
        sp = seg_ptr_of(sizes)
        np.testing.assert_array_equal(g[tag + '/seg_ptr'], sp)
        assert len(g[tag + '/seeds']) == len(sizes) and g[tag + '/centroids'].shape == (sp[-1], K, Tf, 2)
        for s, (seed, A) in enumerate(zip(g[tag + '/seeds'], sizes)):
            x, c0, iters, (c, lab, cnt, marg), ok = segment_case(int(seed), A, M, K, Tf, t0, init, 'full')
            assert ok and marg.min() >= MARGIN, (tag, s, marg.min())
            np.testing.assert_array_equal(g[tag + '/init'][sp[s]:sp[s + 1]], c0, err_msg=tag)
            np.testing.assert_array_equal(g[tag + '/labels'][s], lab, err_msg=tag)
            np.testing.assert_array_equal(g[tag + '/counts'][s], cnt, err_msg=tag)
            np.testing.assert_allclose(g[tag + '/centroids'][sp[s]:sp[s + 1]], c, rtol=0, atol=1e-12 * np.abs(x).max(), err_msg=tag)


@pytest.mark.parametrize('tag', sorted(SHAPES))
def test_regenerated_shapes_hold_the_one_step_cap(golden, tag):
    """On the yardstick alone: per segment, the share of samples a one-step comparison leaves out (margin < 1e-3) is at most 1 %."""
    g = golden('reduce_scenes')
    _, sizes, R, K_in, K, Tf, t0 = SHAPES[tag]
    seeds = g[tag + '/seeds']
    assert len(seeds) == len(sizes)
    x, init, c, lab, cnt, sure = shape_case(tag, seeds)
    n, M = sum(sizes), R * K_in
    assert x.shape == (n, M, Tf, 2) and init.shape == c.shape == (n, K, Tf, 2) and lab.shape == sure.shape == (len(sizes), M)
    assert (1.0 - sure.mean(axis=1)).max() <= ONE_STEP_CAP, (tag, (1.0 - sure.mean(axis=1)).max())
    assert (cnt.sum(axis=1) == M).all() and lab.min() >= 0 and lab.max() < K


def test_one_agent_segments_are_the_per_agent_yardstick():
    """The restatement of a one-agent segment is tests/test_reduce.py's yardstick of that agent, value for value."""
    x = make_samples(3, 1, 50, 12)
    for t0 in (0, 7):
        a = kmeans_f64(x[0], x[0, :6], 5, t0)
        b = scene_kmeans_f64(x, x[:, :6], 5, t0)
        assert (a[0] == b[0][0]).all() and (a[1] == b[1]).all() and (a[2] == b[2]).all() and (a[3] == b[3]).all()


# ----- the entry point -----------------------------------------------------------------------------------------------------------------

def test_entry_point_exported_declared_and_abi_version():
    from sttode_amd import capi
    from test_capi_symbols import header_functions
    fns = header_functions()
    L = capi.lib()
    assert capi.ABI_VERSION == 15 and L.sttode_abi_version() == 15
    assert ENTRY in fns and ENTRY in capi.SIGNATURES and hasattr(L, ENTRY)
    assert len(fns[ENTRY]) == len(capi.SIGNATURES[ENTRY]) == 16
    assert ENTRY + '_ws' not in fns and ENTRY not in capi.RESTYPES          # no workspace: the centroids live in the output array


def test_argument_checks_before_launch():
    """Every limit is refused with a message naming the entry point (host logic only: no pointer is dereferenced, nothing launches)."""
    from sttode_amd import capi
    L = capi.lib()
    p = ctypes.c_void_p(0x1000)          # never dereferenced: every call below fails its checks first
    good = dict(pred=p, n=5, R=3, K_in=20, Tf=12, K=20, iters=10, from_frame=0, init_mode=0, init=None, seg_ptr=p, S=2, centroids=p,
                labels=p, counts=p)

    def refused(match, **kw):
        a = {**good, **kw}
        rc = L.sttode_reduce_scenes(a['pred'], a['n'], a['R'], a['K_in'], a['Tf'], a['K'], a['iters'], a['from_frame'], a['init_mode'],
                                    a['init'], a['seg_ptr'], a['S'], a['centroids'], a['labels'], a['counts'], None)
        assert rc != 0, kw
        msg = L.sttode_last_error().decode()
        assert ENTRY in msg and match in msg, (kw, msg)
    refused('n must be', n=0)
    refused('n must be', n=-3)
    refused('S must be', S=0)
    refused('S must be', S=-1)
    refused('K must be', K=0)
    refused('K must be', K=65, R=4)
    refused('M = R K_in', K=61)                       # K > M = 60
    refused('M = R K_in', R=205)                      # M = 4100 > 4096
    refused('M = R K_in', R=0)
    refused('M = R K_in', K_in=0)
    refused('M = R K_in', R=1 << 20, K_in=1 << 20)    # the product does not wrap
    refused('Tf must be', Tf=0)
    refused('Tf must be', Tf=201)
    refused('from_frame', from_frame=-1)
    refused('from_frame', from_frame=12)
    refused('iters', iters=0)
    refused('iters', iters=1001)
    refused('init_mode', init_mode=3)
    refused('init_mode', init_mode=-1)
    refused('init must be', init_mode=2)              # mode 2 without init
    refused('init must be', init_mode=0, init=p)      # init outside mode 2
    refused('init must be', init_mode=1, init=p)
    for name in ('pred', 'seg_ptr', 'centroids', 'labels', 'counts'):
        refused('null', **{name: None})


# ----- the Python layers -----------------------------------------------------------------------------------------------------------------

def test_python_layers_refuse_bad_input():
    import torch
    from helpers import make_args
    from sttode_amd import STTODENet, capi, metrics
    from sttode_amd.evaluate import eval_scenes_reduced
    with pytest.raises(capi.SttodeError, match='HIP'):
        metrics.reduce_scenes(torch.zeros(3, 40, 12, 2), [0, 1, 3], 5)              # CPU tensor: no fallback
    with pytest.raises(capi.SttodeError, match='HIP'):
        metrics.reduce_scenes(torch.zeros(2, 4, 20, 12, 2), K=5, seg_len=2, init='maximin')
    with pytest.raises(capi.SttodeError, match='HIP'):
        metrics.reduce_scenes(np.zeros((3, 40, 12, 2), np.float32), [0, 3], 5)
    m = STTODENet(make_args(), 'cpu')
    m.set_data(None, torch.zeros(3, 2, 8), torch.zeros(3, 2, 12))
    with pytest.raises(capi.SttodeError):
        m.inference_reduced(3, level='scene')
    with pytest.raises(ValueError, match='rounds'):
        eval_scenes_reduced(m, [], 0, level='scene')
    with pytest.raises(ValueError, match='level'):
        eval_scenes_reduced(m, [], 2, level='game')


def test_agent_weights_are_a_gather_of_the_segment_rows():
    """SceneReduction.agent_weights [n, K] against a NumPy gather, empty segments included (the class is plain tensor code: the CPU runs it)."""
    import torch
    from sttode_amd import metrics
    rng = np.random.default_rng(5)
    for sizes in ((3,), (1, 2, 3, 7), (2, 0, 4, 0, 0, 1), (0, 5), (5, 0)):
        sp = seg_ptr_of(sizes)
        n, S, M, K = int(sp[-1]), len(sizes), 40, 5
        red = metrics.SceneReduction(n, S, M, K, 12, torch.device('cpu'), torch.from_numpy(sp))
        cnt = rng.multinomial(M, np.ones(K) / K, size=S).astype(np.int32)
        red.counts.copy_(torch.from_numpy(cnt))
        w = cnt.astype(np.float32) / np.float32(M)
        assert red.weights.dtype == torch.float32 and (red.weights.numpy() == w).all()
        ref = w[np.repeat(np.arange(S), sizes)]
        got = red.agent_weights
        assert got.dtype == torch.float32 and tuple(got.shape) == (n, K) and (got.numpy() == ref).all(), sizes
        assert red.labels.shape == (S, M) and red.centroids.shape == (n, K, 12, 2) and red.seg_ptr.dtype == torch.int32


def test_signatures_keep_their_parameters_and_defaults():
    """The new keywords trail: everything in front of them is what it was, defaults included."""
    from sttode_amd import STTODENet, metrics
    from sttode_amd.evaluate import eval_scenes_reduced

    def params(f):
        return [(p.name, p.default) for p in inspect.signature(f).parameters.values()]
    E = inspect.Parameter.empty
    assert params(eval_scenes_reduced) == [
        ('model', E), ('dataset', E), ('rounds', E), ('K', None), ('iters', 10), ('from_frame', 0), ('init', 'first'), ('traj_scale', 1.0),
        ('scenes_per_call', 512), ('z_fn', None), ('pipelined', True), ('miss_threshold', 1.0), ('spread', False), ('div_scale', None),
        ('ks', (1, 5, 10)), ('weighted', False), ('level', 'agent'), ('joint', False), ('collision_radius', None), ('kde', False)]
    assert params(STTODENet.inference_reduced) == [('self', E), ('rounds', E), ('K', None), ('iters', 10), ('from_frame', 0), ('init', 'first'),
                                                   ('z', None), ('level', 'agent')]
    assert params(metrics.reduce_samples) == [('pred', E), ('K', E), ('iters', 10), ('from_frame', 0), ('init', 'first')]
    p = params(metrics.reduce_scenes)
    assert [n for n, _ in p] == ['pred', 'seg_ptr', 'K', 'iters', 'from_frame', 'init', 'seg_len'] and p[3:] == [
        ('iters', 10), ('from_frame', 0), ('init', 'first'), ('seg_len', None)]
    assert inspect.signature(metrics.reduce_scenes).parameters['seg_len'].kind is inspect.Parameter.KEYWORD_ONLY
