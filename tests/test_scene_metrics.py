"""CPU tests of the scene-level metrics (sttode_joint_select, sttode_kde_nll): a NumPy restatement of the kernels' contract
held to tests/golden/scene_metrics.npz (and, where SciPy imports, to scipy.stats.gaussian_kde directly), and the new entry points in
header, ctypes table and library."""
import ctypes
import os

import numpy as np
import pytest

from test_selection import select_np


def joint_np(pred, gt, seg_ptr, scale=1.0, radius=None):
    """What sttode_joint_select computes: ADE(a, k) / FDE(a, k) in fp32 as select_np (the selection kernel's order), per segment their sum
    over the agents in increasing agent order in float64 divided by the agent count, the minimum as float32 and its first index; with a
    radius, per segment the colliding agents summed over the samples and those of the ground truth (float32 differences of the scaled
    coordinates, squared distance strictly below radius^2, another agent of the segment, some frame)."""
    pred, gt = np.asarray(pred, np.float32), np.asarray(gt, np.float32)
    n, K, Tf = pred.shape[:3]
    d = (pred - gt[:, None]) * np.float32(scale)
    dist = np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1])
    s = np.zeros((n, K), np.float32)
    for t in range(Tf):
        s += dist[..., t]
    per = {'jade': s / np.float32(Tf), 'jfde': dist[..., -1]}
    sp = np.asarray(seg_ptr)
    out = {}
    for name, v in per.items():
        vals, idx = [], []
        for a0, a1 in zip(sp[:-1], sp[1:]):
            acc = np.zeros(K, np.float64)
            for a in range(a0, a1):
                acc += v[a].astype(np.float64)
            m = acc / (a1 - a0)
            idx.append(int(np.argmin(m)))
            vals.append(np.float32(m.min()))
        out['seg_' + name], out['seg_' + name + '_idx'] = np.array(vals, np.float32), np.array(idx, np.int32)
    if radius is not None:
        P, G = pred * np.float32(scale), gt * np.float32(scale)
        r2 = np.float32(radius) * np.float32(radius)

        def colliding(pos, a0, a1):                                     # pos [n, Tf, 2] -> colliding agents of the segment
            q = pos[a0:a1]
            dd = q[:, None] - q[None]
            hit = ((dd[..., 0] * dd[..., 0] + dd[..., 1] * dd[..., 1]) < r2).any(axis=-1)
            np.fill_diagonal(hit, False)
            return int(hit.any(axis=1).sum())
        out['seg_col'] = np.array([sum(colliding(P[:, k], a0, a1) for k in range(K)) for a0, a1 in zip(sp[:-1], sp[1:])], np.int32)
        out['seg_gt_col'] = np.array([colliding(G, a0, a1) for a0, a1 in zip(sp[:-1], sp[1:])], np.int32)
    return out


def kde_nll_np(pred, gt, scale=1.0):
    """What sttode_kde_nll computes, in float64 on (double)(x * scale): per frame the unbiased covariance C of the K samples, Scott's factor
    f = K^(-1/6), Sigma = f^2 C, logsumexp over k of the Gaussian exponent, minus log K and log det(2 pi Sigma) / 2, clipped below at -20;
    minus the mean over frames; NaN where C00 <= 0 or det C <= 0 at some frame."""
    X = (np.asarray(pred, np.float32) * np.float32(scale)).astype(np.float64)
    G = (np.asarray(gt, np.float32) * np.float32(scale)).astype(np.float64)
    K = X.shape[1]
    m = X.sum(axis=1) / K                                              # [n, Tf, 2]
    dx = X - m[:, None]
    c00 = (dx[..., 0] * dx[..., 0]).sum(axis=1) / (K - 1)
    c01 = (dx[..., 0] * dx[..., 1]).sum(axis=1) / (K - 1)
    c11 = (dx[..., 1] * dx[..., 1]).sum(axis=1) / (K - 1)
    det = c00 * c11 - c01 * c01
    bad = ~(c00 > 0) | ~(det > 0)                                      # [n, Tf]
    f2 = (K ** (-1.0 / 6.0)) ** 2
    with np.errstate(divide='ignore', invalid='ignore'):
        e = G[:, None] - X                                             # [n, K, Tf, 2]
        q = (c11[:, None] * e[..., 0] ** 2 - 2 * c01[:, None] * e[..., 0] * e[..., 1] + c00[:, None] * e[..., 1] ** 2) / (f2 * det[:, None])
        ex = -0.5 * q
        mx = ex.max(axis=1)
        lse = np.log(np.exp(ex - mx[:, None]).sum(axis=1)) + mx
        lp = lse - np.log(K) - 0.5 * np.log((2 * np.pi * f2) ** 2 * det)
    lp = np.where(lp < -20.0, -20.0, lp)
    nll = -lp.mean(axis=1)
    nll[bad.any(axis=1)] = np.nan
    return nll


def cases(golden):
    g = golden('scene_metrics')
    for tag in map(str, g['cases']):
        yield tag, g[tag + '/pred'], g[tag + '/gt'], g[tag + '/seg_ptr'], float(g[tag + '/scale']), float(g[tag + '/radius']), g


def test_restatement_matches_the_golden(golden):
    seen_k, seen_tf, big, single = set(), set(), 0, 0
    for tag, pred, gt, sp, scale, r, g in cases(golden):
        seen_k.add(pred.shape[1])
        seen_tf.add(pred.shape[2])
        big = max(big, int(np.diff(sp).max()))
        single += int((np.diff(sp) == 1).sum())
        j = joint_np(pred, gt, sp, scale, r)
        for f in ('seg_jade', 'seg_jfde'):
            np.testing.assert_allclose(j[f], g[tag + '/' + f], rtol=1e-5, atol=1e-6, err_msg=f'{tag} {f}')
        for f in ('seg_jade_idx', 'seg_jfde_idx', 'seg_col', 'seg_gt_col'):
            np.testing.assert_array_equal(j[f], g[tag + '/' + f], err_msg=f'{tag} {f}')
        nll = kde_nll_np(pred, gt, scale)
        ref = g[tag + '/kde_nll']
        np.testing.assert_array_equal(np.isnan(nll), np.isnan(ref), err_msg=tag)
        np.testing.assert_allclose(nll[~np.isnan(ref)], ref[~np.isnan(ref)], rtol=0, atol=1e-9, err_msg=tag)
    assert {2, 6, 20, 64} <= seen_k and {1, 12, 40} <= seen_tf and big >= 700 and single >= 5


def test_golden_exercises_ties_clip_and_degenerate_frames(golden):
    g = golden('scene_metrics')
    pred, gt, sp = g['ties_k20_t12/pred'], g['ties_k20_t12/gt'], g['ties_k20_t12/seg_ptr']
    j = joint_np(pred, gt, sp)
    ade = select_np(pred, gt)
    for s, (a0, a1) in enumerate(zip(sp[:-1], sp[1:])):
        k = int(g['ties_k20_t12/seg_jade_idx'][s])
        dup = [q for q in range(pred.shape[1]) if (pred[a0:a1, q] == pred[a0:a1, k]).all()]
        assert len(dup) >= 3 and dup[0] == k == j['seg_jade_idx'][s], (s, dup, k)   # exact ties: the lowest k
    assert g['ties_k20_t12/seg_jade_idx'][2] == 0 and ade['best_ade_idx'][sp[2]] == 0
    # the -20 clip engages: some finite agent's NLL is at least 20 * 2 / Tf (two frames 60 m away)
    nll = g['k20_t12/kde_nll']
    assert np.nanmax(nll) >= 20 * 2 / 12 and np.isnan(nll).sum() >= 5
    assert np.isnan(g['k2_t12/kde_nll']).all()                         # two points always lie on a line


def test_one_agent_segments_reproduce_the_selection():
    rng = np.random.default_rng(5)
    pred = rng.normal(0, 2, (9, 20, 12, 2)).astype(np.float32)
    gt = rng.normal(0, 2, (9, 12, 2)).astype(np.float32)
    sel = select_np(pred, gt, scale=1.3)
    j = joint_np(pred, gt, np.arange(10), scale=1.3)
    np.testing.assert_array_equal(j['seg_jade'], sel['ade'])
    np.testing.assert_array_equal(j['seg_jfde'], sel['fde'])
    np.testing.assert_array_equal(j['seg_jade_idx'], sel['best_ade_idx'])
    np.testing.assert_array_equal(j['seg_jfde_idx'], sel['best_fde_idx'])


def test_restatement_matches_gaussian_kde(golden):
    pytest.importorskip('scipy.stats')
    import importlib.util
    spec = importlib.util.spec_from_file_location('make_scene_metrics_golden', os.path.join(os.path.dirname(__file__), 'golden',
                                                                                            'make_scene_metrics_golden.py'))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    compute_kde_nll = gen.compute_kde_nll                              # Trajectron++'s loop over scipy.stats.gaussian_kde
    for tag, pred, gt, sp, scale, r, g in cases(golden):
        n = min(pred.shape[0], 40)
        X = (pred[:n] * np.float32(scale)).astype(np.float64)
        G = (gt[:n] * np.float32(scale)).astype(np.float64)
        nll = kde_nll_np(pred[:n], gt[:n], scale)
        for a in range(n):
            v = compute_kde_nll(X[a][None], G[a])
            if pred.shape[1] == 2:                                     # (singular by construction; scipy's Cholesky passes or fails on rounding)
                assert np.isnan(nll[a])
            elif np.isnan(v):
                assert np.isnan(nll[a]), (tag, a)
            else:
                assert abs(nll[a] - v) <= 1e-9, (tag, a, nll[a], v)


def test_collisions_are_strict_and_need_another_agent():
    pred = np.zeros((3, 1, 2, 2), np.float32)
    pred[1, 0, :, 0] = 1.0                                             # agent 1 exactly 1 m from agent 0; agent 2 2 m away
    pred[2, 0, :, 0] = 3.0
    gt = pred[:, 0].copy()
    assert joint_np(pred, gt, [0, 3], radius=1.0)['seg_col'].tolist() == [0]
    assert joint_np(pred, gt, [0, 3], radius=1.001)['seg_col'].tolist() == [2]
    assert joint_np(pred, gt, [0, 1, 2, 3], radius=5.0)['seg_gt_col'].tolist() == [0, 0, 0]


def test_scene_metric_entry_points_in_header_table_and_library():
    from sttode_amd import capi
    from test_capi_symbols import header_functions
    fns = header_functions()
    for name, nargs in (('sttode_joint_select', 16), ('sttode_kde_nll', 8), ('sttode_async_joint_select', 17),
                        ('sttode_async_kde_nll', 9)):
        assert name in fns and len(fns[name]) == nargs, name
        assert name in capi.SIGNATURES and len(capi.SIGNATURES[name]) == nargs, name
    assert fns['sttode_joint_select'][8] == 'float radius' and fns['sttode_kde_nll'][6] == 'double* nll'
    assert capi.ABI_VERSION >= 13
    if not os.path.exists(capi.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    L = ctypes.CDLL(capi.LIB_PATH)
    for name in ('sttode_joint_select', 'sttode_kde_nll', 'sttode_async_joint_select', 'sttode_async_kde_nll'):
        assert hasattr(L, name), name
    assert L.sttode_abi_version() == capi.ABI_VERSION


def test_refusals_name_the_entry_point_without_a_device():
    from sttode_amd import capi
    L = capi.lib()
    P = ctypes.c_void_p(16)                                            # (never dereferenced: every call below is refused first)
    rc = L.sttode_joint_select(P, P, 4, 65, 12, ctypes.c_float(1.0), P, 1, ctypes.c_float(0.0), P, P, P, P, None, None, None)
    assert rc != 0 and b'sttode_joint_select' in L.sttode_last_error() and b'K > 64' in L.sttode_last_error()
    rc = L.sttode_joint_select(P, P, 4, 20, 12, ctypes.c_float(1.0), P, 1, ctypes.c_float(0.5), P, P, P, P, None, None, None)
    assert rc != 0 and b'radius > 0' in L.sttode_last_error()
    for K in (1, 65):
        rc = L.sttode_kde_nll(P, P, 4, K, 12, ctypes.c_float(1.0), P, None)
        assert rc != 0 and b'sttode_kde_nll' in L.sttode_last_error() and b'2 <= K <= 64' in L.sttode_last_error()
    rc = L.sttode_async_kde_nll(None, 0, P, P, 4, 20, 12, ctypes.c_float(1.0), P)
    assert rc != 0 and b'sttode_async_kde_nll' in L.sttode_last_error()


def test_python_surface_exists():
    import inspect
    from sttode_amd import STTODENet, evaluate, metrics
    for name in ('select_joint', 'select_joint_async', 'kde_nll', 'kde_nll_async'):
        assert callable(getattr(STTODENet, name))
    assert callable(metrics.joint_select) and callable(metrics.kde_nll)
    for name in ('eval_scenes_report', 'eval_sampler_report', 'eval_nba_report'):
        ps = inspect.signature(getattr(evaluate, name)).parameters
        assert ps['joint'].default is False and ps['kde'].default is False and ps['collision_radius'].default is None
    f = {x.name: x.default for x in __import__('dataclasses').fields(evaluate.EvalReport)}
    for name in ('joint_ade', 'joint_fde', 'scene_joint_ade', 'scene_joint_fde', 'scene_joint_idx', 'collision_radius', 'collision_rate',
                 'gt_collision_rate', 'scene_collision', 'kde_nll', 'kde_nll_agents', 'kde_invalid'):
        assert name in f and f[name] is None, name
