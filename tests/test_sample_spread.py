"""CPU tests of the sample-spread metrics (sttode_sample_spread): tests/golden/sample_spread.npz checked against itself -- a
loop restatement in the kernel's order (pairs in F.pdist order, frames in frame order) against the stored array-form values and the stored
value of the reference's diversity_loss, the identities at Tf = 1, the energy scores against the explicit 1/K^2 double sum -- and the new
entry points in header, ctypes table and library, their refusals, and the Python surface."""
import ctypes
import os

import numpy as np
import pytest

F64 = ('apd', 'fpd', 'pade', 'dlow')


def coords(x, scale):
    return (np.asarray(x, np.float32) * np.float32(scale)).astype(np.float64)


def spread_np(pred, gt, scale, div_scale):
    """What sttode_sample_spread computes for its float64 outputs, pair by pair in F.pdist order with the frames added in frame order."""
    X, Y = coords(pred, scale), coords(gt, scale)
    n, K, Tf = X.shape[:3]
    P = K * (K - 1) // 2
    out = {k: np.zeros(n) for k in F64 + ('es_ade', 'es_fde')}
    for a in range(n):
        for i in range(K):
            for j in range(i + 1, K):
                s2 = s1 = last = 0.0
                for t in range(Tf):
                    dx, dy = X[a, i, t] - X[a, j, t]
                    last = np.sqrt(dx * dx + dy * dy)
                    s2 += dx * dx + dy * dy
                    s1 += last
                out['apd'][a] += np.sqrt(s2)
                out['fpd'][a] += last
                out['pade'][a] += s1 / Tf
                out['dlow'][a] += np.exp(-s2 / div_scale)
        for k in F64:
            out[k][a] /= P
        G = np.sqrt(((X[a] - Y[a][None]) ** 2).sum(axis=-1))          # [K, Tf]
        c = (K - 1) / (2.0 * K)
        out['es_ade'][a] = G.mean(axis=1).sum() / K - c * out['pade'][a]
        out['es_fde'][a] = G[:, -1].sum() / K - c * out['fpd'][a]
    return out


def cases(golden):
    g = golden('sample_spread')
    for tag in map(str, g['cases']):
        yield tag, g[tag + '/pred'], g[tag + '/gt'], float(g[tag + '/scale']), float(g[tag + '/div_scale']), g


def close(got, ref, mag, what, bound=1e-10):
    """|got - ref| <= bound * (sum of the magnitudes of the terms combined), NaN where the reference is NaN; returns the worst ratio."""
    got, ref, mag = np.asarray(got, np.float64), np.asarray(ref, np.float64), np.asarray(mag, np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), what
    ok = ~np.isnan(ref)
    err = np.abs(got[ok] - ref[ok])
    assert (err <= bound * np.abs(mag[ok])).all(), (what, float(err.max()), float(np.abs(mag[ok]).min()))
    nz = np.abs(mag[ok]) > 0
    return float((err[nz] / np.abs(mag[ok])[nz]).max()) if nz.any() else 0.0


def test_fixture_covers_the_kernel_edges(golden):
    g = golden('sample_spread')
    tile = int(g['tile'])
    shapes = [g[t + '/pred'].shape for t in map(str, g['cases'])]
    assert {2, 3, 23, 24, 64} <= {s[1] for s in shapes}
    assert {1, tile - 1, tile, tile + 1, 40} <= {s[2] for s in shapes}
    assert {1, 5, 70} <= {s[0] for s in shapes} and (2, 64, 40, 2) in shapes
    assert {1.0, 0.5, 50.0} <= {float(g[t + '/scale']) for t in map(str, g['cases'])}
    assert os.path.getsize(os.path.join(os.path.dirname(__file__), 'golden', 'sample_spread.npz')) < 1 << 20
    assert g['dup_k20_t12/apd'][0] == 0.0 and g['dup_k20_t12/dlow'][0] == 1.0        # every sample the same
    assert np.isnan(g['nan_k20_t12/apd'][:4]).all() and np.isfinite(g['nan_k20_t12/apd'][4])
    assert np.isinf(g['nan_k20_t12/ade_at_k'][1, 0]) and np.isfinite(g['nan_k20_t12/ade_at_k'][1, 1])
    assert np.isinf(g['nan_k20_t12/ade_at_k'][3]).all()
    assert g['far_k20_t12/es_ade'][0] > 50.0


def test_restatement_matches_the_fixture_and_the_reference_value(golden):
    for tag, pred, gt, scale, ds, g in cases(golden):
        r = spread_np(pred, gt, scale, ds)
        for k in F64:
            close(r[k], g[tag + '/' + k], g[tag + '/' + k], f'{tag} {k}', 1e-12)
        for k in ('es_ade', 'es_fde'):
            close(r[k], g[tag + '/' + k], g[tag + '/' + k + '_mag'], f'{tag} {k}', 1e-12)
        ref = float(g[tag + '/dlow_ref'])                              # the reference's diversity_loss(..., weight=1)[1]
        mine = r['dlow'].sum() / pred.shape[0]
        assert (np.isnan(ref) and np.isnan(mine)) or abs(mine - ref) <= 1e-12 * abs(ref), (tag, mine, ref)


def test_identities_at_one_frame_and_the_double_sum(golden):
    for tag, pred, gt, scale, ds, g in cases(golden):
        if pred.shape[2] == 1:                                         # d_traj == d_fde == Tf d_ade
            np.testing.assert_allclose(g[tag + '/apd'], g[tag + '/fpd'], rtol=1e-14, atol=0)
            np.testing.assert_allclose(g[tag + '/apd'], g[tag + '/pade'], rtol=1e-14, atol=0)
            np.testing.assert_array_equal(g[tag + '/ade_k'], g[tag + '/fde_k'])
        for k in ('es_ade', 'es_fde'):                                 # the pair-mean form == the 1/K^2 double sum
            close(g[tag + '/' + k], g[tag + '/' + k + '_double'], g[tag + '/' + k + '_mag'], f'{tag} {k}', 1e-13)
        ok = ~np.isnan(g[tag + '/es_ade'])
        assert (g[tag + '/es_ade'][ok] > 0).all()                      # an energy score with a proper distance is positive
        K = pred.shape[1]
        for k in ('ade', 'fde'):
            at, per = g[tag + '/' + k + '_at_k'], g[tag + '/' + k + '_k']
            assert (at[:, 1:] <= at[:, :-1]).all() and at.shape == (pred.shape[0], K)
            if not np.isnan(per).any():
                np.testing.assert_array_equal(at, np.minimum.accumulate(per, axis=1))


def test_entry_points_in_header_table_and_library():
    from sttode_amd import capi
    from test_capi_symbols import header_functions
    fns = header_functions()
    for name, nargs in (('sttode_sample_spread', 16), ('sttode_async_sample_spread', 17)):
        assert name in fns and len(fns[name]) == nargs, name
        assert name in capi.SIGNATURES and len(capi.SIGNATURES[name]) == nargs, name
    assert fns['sttode_sample_spread'][5] == 'float scale' and fns['sttode_sample_spread'][6] == 'double div_scale'
    assert fns['sttode_sample_spread'][7] == 'double* apd' and fns['sttode_sample_spread'][14] == 'float* fde_at_k'
    assert capi.ABI_VERSION == 15
    if not os.path.exists(capi.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    L = ctypes.CDLL(capi.LIB_PATH)
    for name in ('sttode_sample_spread', 'sttode_async_sample_spread'):
        assert hasattr(L, name), name
    assert L.sttode_abi_version() == 15


def test_refusals_name_the_entry_point_without_a_device():
    from sttode_amd import capi
    L = capi.lib()
    P = ctypes.c_void_p(16)                                            # (never dereferenced: every call below is refused first)
    one, d = ctypes.c_float(1.0), ctypes.c_double

    def refused(what, *args):
        rc = L.sttode_sample_spread(*args)
        err = L.sttode_last_error()
        assert rc != 0 and b'sttode_sample_spread' in err and what in err, (what, err)
    for K in (1, 65):
        refused(b'2 <= K <= 64', P, P, 4, K, 12, one, d(1.0), P, P, P, P, P, P, P, P, None)
    for ds in (0.0, -1.0, float('inf'), float('nan')):
        refused(b'div_scale', P, P, 4, 20, 12, one, d(ds), P, P, P, P, P, P, P, P, None)
    refused(b'n and Tf', P, P, 0, 20, 12, one, d(1.0), P, P, P, P, P, P, P, P, None)
    refused(b'n and Tf', P, P, 4, 20, 0, one, d(1.0), P, P, P, P, P, P, P, P, None)
    refused(b'null pointer', P, P, 4, 20, 12, one, d(1.0), P, P, None, P, P, P, P, P, None)
    refused(b'null pointer', None, P, 4, 20, 12, one, d(1.0), P, P, P, P, P, P, P, P, None)
    for i in range(4):                                                 # an output that needs gt, without gt
        outs = [None] * 4
        outs[i] = P
        refused(b'need gt', P, None, 4, 20, 12, one, d(1.0), P, P, P, P, *outs, None)
    rc = L.sttode_async_sample_spread(None, 0, P, P, 4, 20, 12, one, d(1.0), P, P, P, P, P, P, P, P)
    assert rc != 0 and b'sttode_async_sample_spread' in L.sttode_last_error()


def test_python_surface_and_host_side_refusals():
    import dataclasses
    import inspect
    import torch
    from sttode_amd import STTODENet, capi, evaluate, metrics
    for name in ('sample_spread', 'sample_spread_async'):
        ps = inspect.signature(getattr(STTODENet, name)).parameters
        assert ps['gt'].default is None and ps['scale'].default == 1.0 and ps['div_scale'].default == 1.0
    ps = inspect.signature(metrics.sample_spread).parameters
    assert list(ps) == ['pred_nk', 'gt', 'scale', 'div_scale'] and ps['gt'].default is None
    assert set(metrics.SampleSpread.__slots__) >= {'apd', 'fpd', 'pade', 'dlow', 'es_ade', 'es_fde', 'ade_at_k', 'fde_at_k'}
    assert callable(metrics.SampleSpread.at) and callable(metrics.SampleSpread.record_stream)
    with pytest.raises(capi.SttodeError, match='HIP device only'):     # device-only: no CPU fallback
        metrics.sample_spread(torch.zeros(3, 20, 12, 2))
    for K in (1, 65):
        with pytest.raises(ValueError, match='2 <= K <= 64'):
            metrics.check_spread(K, 1.0)
    for ds in (0.0, -2.0, float('inf'), float('nan')):
        with pytest.raises(ValueError, match='div_scale'):
            metrics.check_spread(20, ds)
    assert metrics.check_spread(20, 2) == 2.0
    for name in ('eval_scenes_report', 'eval_sampler_report', 'eval_nba_report', 'eval_scenes_reduced'):
        ps = inspect.signature(getattr(evaluate, name)).parameters
        assert ps['spread'].default is False and ps['div_scale'].default is None and tuple(ps['ks'].default) == (1, 5, 10), name
    fields = dataclasses.fields(evaluate.EvalReport)
    new = ('apd', 'fpd', 'pade', 'dlow', 'energy_ade', 'energy_fde', 'spread_agents', 'ade_at_k', 'fde_at_k')
    assert tuple(f.name for f in fields[-len(new):]) == new            # trailing
    assert all(f.default is None for f in fields[-len(new):])
