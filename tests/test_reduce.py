"""CPU tests of oversample-and-reduce (sttode_reduce_samples, csrc/reduce.hip): the float64 NumPy restatement of the contract
that the GPU tests compare the kernel with (``kmeans_f64`` / ``maximin_f64``), pinned here against scipy.cluster.vq.kmeans2; the stored
cases of tests/golden/reduce.npz re-checked against it, near-tie margins included; the entry point's argument checks (host logic only).

Near-ties.  Lloyd iterations are chaotic in floating point: a label that flips on a near-tie moves a centroid, which moves later labels.
For a sample let d1 <= d2 be its two smallest squared distances in float64; its margin is (d2 - d1) / (d2 + d1).  An fp32 squared distance
over <= 96 terms carries a relative error of about 100 * 2^-24 ~ 6e-6, so a margin of 1e-3 is two orders above what fp32 can flip.  The
stored full-run cases are seeds whose EVERY sample at EVERY iteration holds that margin on the float64 path (so the fp32 labels must be
equal, all of them); the one-step cases compare only the samples that hold it, at most 1 % left out.  The same rule applies to maximin's
argmax (its top two candidates)."""
import ctypes

import numpy as np
import pytest

ENTRY = 'sttode_reduce_samples'
MARGIN = 1e-3
ONE_STEP_CAP = 0.01


# ----- inputs: multi-modal random walks in world coordinates --------------------------------------------------------------------------

def make_samples(seed, n, M, Tf):
    """[n, M, Tf, 2] float32: per agent 2-5 velocity modes (spread ~1 m per frame), every sample follows one mode with per-step noise of a
    third of the spread, summed over the frames from an origin several metres out (coordinates look like world coordinates)."""
    rng = np.random.default_rng(seed)
    out = np.empty((n, M, Tf, 2), np.float64)
    for a in range(n):
        modes = rng.normal(0.0, 1.0, (int(rng.integers(2, 6)), 2))
        pick = rng.integers(0, len(modes), M)
        vel = modes[pick][:, None, :] + rng.normal(0.0, 1.0 / 3.0, (M, Tf, 2))
        out[a] = rng.uniform(-15.0, 15.0, 2) + np.cumsum(vel, axis=1)
    return out.astype(np.float32)


# ----- the yardstick -----------------------------------------------------------------------------------------------------------------

def sq_dists(x, c, t0):
    """[M, K] float64: sum over frames t >= t0 of |x[m, t] - c[k, t]|^2."""
    d = x[:, None, t0:, :].astype(np.float64) - c[None, :, t0:, :].astype(np.float64)
    return (d * d).sum(axis=(2, 3))


def margins(d):
    """Per row of d [M, K]: (d2 - d1) / (d2 + d1) of its two smallest entries (1 for K = 1; 0 for an exact tie, 0 / 0 included)."""
    if d.shape[1] < 2:
        return np.ones(d.shape[0])
    s = np.sort(d, axis=1)
    den = s[:, 1] + s[:, 0]
    return np.where(den > 0, (s[:, 1] - s[:, 0]) / np.where(den > 0, den, 1.0), 0.0)


def kmeans_f64(x, init, iters, t0=0):
    """The contract of include/sttode_hip.h in float64 for ONE agent: x [M, Tf, 2], init [K, Tf, 2] -> (centroids [K, Tf, 2], labels [M],
    counts [K], margin): labels by the frames t >= t0 (np.argmin: the lowest k on exact ties), centroids the means over ALL frames, an
    empty cluster keeps its centroid; margin [iters, M] is every sample's near-tie margin at every iteration."""
    x = np.asarray(x, np.float64)
    c = np.array(init, np.float64)
    K = c.shape[0]
    marg = np.empty((iters, x.shape[0]))
    for i in range(iters):
        d = sq_dists(x, c, t0)
        marg[i] = margins(d)
        lab = np.argmin(d, axis=1)
        for k in range(K):
            if (lab == k).any():
                c[k] = x[lab == k].mean(axis=0)
    return c, lab.astype(np.int32), np.bincount(lab, minlength=K).astype(np.int32), marg


def maximin_f64(x, K, t0=0):
    """Farthest-point initialisation in float64: sample 0, then K - 1 times the sample whose squared distance (frames t >= t0) to its
    nearest chosen sample is largest (np.argmax: the lowest index on ties).  Returns (chosen [K], margin): margin is the smallest
    (v1 - v2) / (v1 + v2) over the picks, v1 >= v2 the top two candidates."""
    x = np.asarray(x, np.float64)
    chosen, marg = [0], 1.0
    mind = sq_dists(x, x[[0]], t0)[:, 0]
    for _ in range(K - 1):
        j = int(np.argmax(mind))
        if len(mind) > 1:
            top = np.sort(mind)[-2:]
            marg = min(marg, (top[1] - top[0]) / (top[1] + top[0]) if top[1] + top[0] > 0 else 0.0)
        chosen.append(j)
        mind = np.minimum(mind, sq_dists(x, x[[j]], t0)[:, 0])
    return np.array(chosen), marg


def means_over_labels(x, labels, K, prev):
    """float64 means of x [M, Tf, 2] over the clusters of `labels`; an empty cluster takes prev[k]."""
    c = np.array(prev, np.float64)
    for k in range(K):
        if (labels == k).any():
            c[k] = np.asarray(x, np.float64)[labels == k].mean(axis=0)
    return c


def centroid_atol(x):
    """M * 2^-24 * max |coordinate|: the bound on a sequential fp32 sum of M terms (relative to the mean after the division)."""
    return x.shape[-3] * 2.0 ** -24 * float(np.abs(x).max())


# the stored cases: tag -> (kind, seed-search start, n, M, K, Tf, from_frame, init); kind 'full': iters = 10, every margin held;
# 'step': iters = 1 from a caller's init (the yardstick's centroids after 3 float64 iterations from 'first'), left-out share <= 1 %
CASES = {
    'full_m20_k5': ('full', 100, 5, 20, 5, 12, 0, 'first'),
    'full_m40_k20': ('full', 200, 5, 40, 20, 12, 0, 'first'),
    'full_m64_k20_mid': ('full', 300, 5, 64, 20, 12, 5, 'first'),
    'full_m64_k6_tf1': ('full', 400, 5, 64, 6, 1, 0, 'first'),
    'full_m70_k7_tf13_end': ('full', 500, 5, 70, 7, 13, 12, 'first'),
    'full_m200_k20': ('full', 600, 2, 200, 20, 12, 0, 'first'),
    'full_m60_k5_tf20': ('full', 700, 5, 60, 5, 20, 0, 'first'),
    'maximin_m40_k5': ('full', 800, 5, 40, 5, 12, 0, 'maximin'),
    'maximin_m64_k20_end': ('full', 900, 3, 64, 20, 12, 11, 'maximin'),
    'step_m1000_k20': ('step', 1000, 2, 1000, 20, 12, 0, None),
    'step_m1024_k64_end': ('step', 1100, 1, 1024, 64, 12, 11, None),
}


def case_agent(seed, M, K, Tf, t0, init, kind):
    """One agent of a case from its seed: (x, init centroids, iters, yardstick outputs, ok): ok says whether the seed qualifies."""
    x = make_samples(seed, 1, M, Tf)[0]
    if kind == 'step':
        c0 = kmeans_f64(x, x[:K], 3, t0)[0].astype(np.float32)
        c, lab, cnt, marg = kmeans_f64(x, c0, 1, t0)
        return x, c0, 1, (c, lab, cnt, marg), (marg < MARGIN).mean() <= ONE_STEP_CAP
    ok = True
    if init == 'maximin':
        chosen, mm = maximin_f64(x, K, t0)
        c0, ok = x[chosen], mm >= MARGIN
    else:
        c0 = x[:K]
    c, lab, cnt, marg = kmeans_f64(x, c0, 10, t0)
    return x, c0, 10, (c, lab, cnt, marg), ok and marg.min() >= MARGIN


# one-step cases regenerated from a seed at test time (too large to store, or many agents): (seed, n, R, K_in, K, Tf, from_frame); M = R K_in.
# The shapes are the smallest on either side of what the kernel branches on: 64-sample chunks (64 / 70), samples per lane (256 / 257,
# 512 / 513), centroid quads (K = 5, 7, 20, 64), LDS staging (M 900 x Tf 20 fits, M 1000 x Tf 20 and M 2048 x Tf 20 do not), one / a few /
# many workgroups.
SHAPES = {
    'n700_m20_k5': (11, 700, 1, 20, 5, 12, 0),
    'n5_m60_r3_k7_mid': (12, 5, 3, 20, 7, 12, 6),
    'n5_m64_k20_tf13': (13, 5, 1, 64, 20, 13, 0),
    'n5_m70_k5_tf1': (14, 5, 1, 70, 5, 1, 0),
    'n5_m200_k20_end': (15, 5, 10, 20, 20, 12, 11),
    'n5_m256_k7': (16, 5, 1, 256, 7, 12, 0),
    'n5_m257_k7_tf20': (17, 5, 1, 257, 7, 20, 19),
    'n2_m512_k20': (18, 2, 2, 256, 20, 12, 3),
    'n2_m513_k20': (19, 2, 27, 19, 20, 12, 0),
    'n5_m1000_r50_k20': (20, 5, 50, 20, 20, 12, 0),
    'n1_m1024_k64': (21, 1, 1, 1024, 64, 12, 0),
    'n2_m900_k20_tf20': (22, 2, 45, 20, 20, 20, 0),
    'n2_m1000_k20_tf20': (23, 2, 50, 20, 20, 20, 0),
    'n2_m2048_k20_tf20': (24, 2, 1, 2048, 20, 20, 10),
}
_SHAPE_CACHE = {}


def shape_case(tag):
    """(x [n,M,Tf,2] f32, init [n,K,Tf,2] f32 -- the yardstick's centroids after 3 float64 iterations from 'first' --, and the yardstick's
    ONE step from there: centroids [n,K,Tf,2] f64, labels [n,M], counts [n,K], sure [n,M] = margin >= 1e-3).  Computed once per process."""
    if tag not in _SHAPE_CACHE:
        seed, n, R, K_in, K, Tf, t0 = SHAPES[tag]
        M = R * K_in
        x = make_samples(seed, n, M, Tf)
        init = np.stack([kmeans_f64(x[a], x[a, :K], 3, t0)[0] for a in range(n)]).astype(np.float32)
        res = [kmeans_f64(x[a], init[a], 1, t0) for a in range(n)]
        out = (x, init, np.stack([r[0] for r in res]), np.stack([r[1] for r in res]), np.stack([r[2] for r in res]),
               np.stack([r[3][0] >= MARGIN for r in res]))
        for v in out:
            v.setflags(write=False)
        _SHAPE_CACHE[tag] = out
    return _SHAPE_CACHE[tag]


# ----- tests ---------------------------------------------------------------------------------------------------------------------------

def test_yardstick_is_scipy_kmeans2():
    """Labels equal and the sliced code book to 1e-12 against scipy.cluster.vq.kmeans2(minit='matrix') over random shapes, empty clusters
    (duplicate centroids in the initial code book) included."""
    vq = pytest.importorskip('scipy.cluster.vq')
    import warnings
    rng = np.random.default_rng(11)
    for trial in range(40):
        M, K, Tf = int(rng.integers(20, 300)), int(rng.integers(1, 21)), int(rng.integers(1, 21))
        K = min(K, M)
        t0 = int(rng.integers(0, Tf))
        iters = int(rng.integers(1, 12))
        x = make_samples(1000 + trial, 1, M, Tf)[0].astype(np.float64)
        init = x[:K].copy()
        if trial % 4 == 0 and K > 2:
            init[K - 1] = init[0]                                       # a duplicate: the higher index stays empty and keeps its value
        c, lab, cnt, _ = kmeans_f64(x, init, iters, t0)
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')                             # (kmeans2 warns about the empty cluster)
            book, code = vq.kmeans2(x[:, t0:].reshape(M, -1), init[:, t0:].reshape(K, -1), iter=iters, minit='matrix')
        np.testing.assert_array_equal(lab, code, err_msg=str(trial))
        np.testing.assert_allclose(c[:, t0:].reshape(K, -1), book, rtol=0, atol=1e-12 * np.abs(x).max(), err_msg=str(trial))
        assert cnt.sum() == M and (cnt == np.bincount(code, minlength=K)).all()
        if trial % 4 == 0 and K > 2:                                    # (one step: later the moved centroid 0 no longer shadows it)
            c1, _, cnt1, _ = kmeans_f64(x, init, 1, t0)
            assert cnt1[K - 1] == 0 and (c1[K - 1] == init[K - 1]).all()


def test_stored_cases_match_the_yardstick_and_hold_their_margins(golden):
    """reduce.npz is what make_reduce_golden.py writes from CASES: inputs regenerate from the stored seeds, the stored outputs are the
    yardstick's, every full-run sample holds the margin at every iteration, every one-step case leaves out at most 1 %."""
    g = golden('reduce')
    assert sorted(map(str, g['cases'])) == sorted(CASES)
    for tag, (kind, _, n, M, K, Tf, t0, init) in CASES.items():
        seeds = g[tag + '/seeds']
        assert len(seeds) == n and g[tag + '/x'].shape == (n, M, Tf, 2) and g[tag + '/x'].dtype == np.float32
        for a, seed in enumerate(seeds):
            x, c0, iters, (c, lab, cnt, marg), ok = case_agent(int(seed), M, K, Tf, t0, init, kind)
            assert ok, (tag, a)
            np.testing.assert_array_equal(g[tag + '/x'][a], x, err_msg=tag)
            np.testing.assert_array_equal(g[tag + '/init'][a], c0, err_msg=tag)
            np.testing.assert_array_equal(g[tag + '/labels'][a], lab, err_msg=tag)
            np.testing.assert_array_equal(g[tag + '/counts'][a], cnt, err_msg=tag)
            np.testing.assert_allclose(g[tag + '/centroids'][a], c, rtol=0, atol=1e-12 * np.abs(x).max(), err_msg=tag)
            if kind == 'full':
                assert marg.min() >= MARGIN, (tag, a, marg.min())
            else:
                assert (marg < MARGIN).mean() <= ONE_STEP_CAP, (tag, a)
                np.testing.assert_array_equal(g[tag + '/sure'][a], marg[0] >= MARGIN, err_msg=tag)


@pytest.mark.parametrize('tag', sorted(SHAPES))
def test_regenerated_shapes_hold_the_one_step_cap(tag):
    """On the yardstick alone: the share of samples a one-step comparison leaves out (margin < 1e-3) is at most 1 % per case."""
    x, init, c, lab, cnt, sure = shape_case(tag)
    seed, n, R, K_in, K, Tf, t0 = SHAPES[tag]
    assert x.shape == (n, R * K_in, Tf, 2) and init.shape == (n, K, Tf, 2) and lab.shape == sure.shape == (n, R * K_in)
    assert 1.0 - sure.mean() <= ONE_STEP_CAP, (tag, 1.0 - sure.mean())
    assert (cnt.sum(axis=1) == R * K_in).all() and lab.min() >= 0 and lab.max() < K


def test_yardstick_edge_rules():
    x = make_samples(5, 1, 30, 4)[0]
    # K = 1: all labels 0, the centroid is the mean
    c, lab, cnt, marg = kmeans_f64(x, x[:1], 3)
    assert (lab == 0).all() and cnt.tolist() == [30] and np.allclose(c[0], x.astype(np.float64).mean(axis=0)) and (marg == 1).all()
    # K = M from the samples themselves: the identity
    c, lab, cnt, _ = kmeans_f64(x, x, 2)
    assert (lab == np.arange(30)).all() and (cnt == 1).all() and (c == x).all()
    # exact ties go to the lowest k; the duplicate stays empty and keeps its value
    init = np.stack([x[0], x[1], x[0]])
    c, lab, cnt, marg = kmeans_f64(x, init, 1)
    assert cnt[2] == 0 and (c[2] == x[0]).all() and (marg >= 0).all()
    # the labels look at frames >= t0 only, the centroids are means over all frames
    y = x.copy()
    y[:, :3] += np.random.default_rng(0).normal(0, 50, (30, 3, 2)).astype(np.float32)
    la = kmeans_f64(x, x[:4], 5, 3)[1]
    cb, lb = kmeans_f64(y, y[:4], 5, 3)[:2]
    assert (la == lb).all() and np.allclose(cb, means_over_labels(y, lb, 4, y[:4]))
    # maximin: sample 0 first, distinct picks on distinct data, ties to the lowest index
    ch, _ = maximin_f64(x, 6)
    assert ch[0] == 0 and len(set(ch.tolist())) == 6
    assert maximin_f64(np.zeros((5, 2, 2)), 3)[0].tolist() == [0, 0, 0]


def test_entry_point_exported_declared_and_abi_version():
    from sttode_amd import capi, evaluate, metrics
    from test_capi_symbols import header_functions
    fns = header_functions()
    L = capi.lib()
    assert capi.ABI_VERSION == 15 and L.sttode_abi_version() == 15
    assert ENTRY in fns and ENTRY in capi.SIGNATURES and hasattr(L, ENTRY)
    assert len(fns[ENTRY]) == len(capi.SIGNATURES[ENTRY]) == 14
    assert callable(metrics.reduce_samples) and callable(evaluate.eval_scenes_reduced)
    from sttode_amd import STTODENet
    assert callable(STTODENet.inference_reduced)


def test_argument_checks_before_launch():
    """Every limit is refused with a message naming the entry point (host logic only: no pointer is dereferenced, nothing launches)."""
    from sttode_amd import capi
    L = capi.lib()
    p = ctypes.c_void_p(0x1000)          # never dereferenced: every call below fails its checks first
    good = dict(pred=p, n=5, R=3, K_in=20, Tf=12, K=20, iters=10, from_frame=0, init_mode=0, init=None, centroids=p, labels=p, counts=p)

    def refused(match, **kw):
        a = {**good, **kw}
        rc = L.sttode_reduce_samples(a['pred'], a['n'], a['R'], a['K_in'], a['Tf'], a['K'], a['iters'], a['from_frame'], a['init_mode'],
                                     a['init'], a['centroids'], a['labels'], a['counts'], None)
        assert rc != 0, kw
        msg = L.sttode_last_error().decode()
        assert ENTRY in msg and match in msg, (kw, msg)
    refused('n must be', n=0)
    refused('n must be', n=-3)
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
    for name in ('pred', 'centroids', 'labels', 'counts'):
        refused('null', **{name: None})


def test_python_layers_refuse_bad_input():
    import torch
    from helpers import make_args
    from sttode_amd import STTODENet, capi, metrics
    from sttode_amd.evaluate import eval_scenes_reduced
    with pytest.raises(capi.SttodeError, match='HIP'):
        metrics.reduce_samples(torch.zeros(3, 40, 12, 2), 5)              # CPU tensor: no fallback
    with pytest.raises(capi.SttodeError, match='HIP'):
        metrics.reduce_samples(torch.zeros(2, 3, 20, 12, 2), 5, init='maximin')
    with pytest.raises(capi.SttodeError, match='HIP'):
        metrics.reduce_samples(np.zeros((3, 40, 12, 2), np.float32), 5)
    m = STTODENet(make_args(), 'cpu')
    m.set_data(None, torch.zeros(3, 2, 8), torch.zeros(3, 2, 12))
    with pytest.raises(capi.SttodeError):
        m.inference_reduced(3)
    with pytest.raises(ValueError, match='rounds'):
        eval_scenes_reduced(m, [], 0)
