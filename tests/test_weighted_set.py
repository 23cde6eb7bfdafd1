"""CPU tests of the weighted sample set (sttode_weighted_set): tests/golden/weighted_set.npz checked against its own
conditions and against the loop restatement of tests/weighted_ref.py; the identities at equal weights against a restatement of 4s's
formulas; the entry point in header, ctypes table and library; its refusals by name without a launch; the Python surface."""
import ctypes
import inspect
import os

import numpy as np
import pytest

from weighted_ref import F64, bok_f32, coords, uniform_spread_np, weighted_set_np

ENTRY = 'sttode_weighted_set'
NARGS = 20
_REF = {}


def cases(golden):
    g = golden('weighted_set')
    for tag in map(str, g['cases']):
        yield tag, g[tag + '/pred'], g[tag + '/weights'], g[tag + '/gt'], float(g[tag + '/scale']), g


def restated(golden, tag):
    """The restatement of a stored case, computed once per process and shared (read-only) among the tests."""
    if tag not in _REF:
        g = golden('weighted_set')
        r = weighted_set_np(g[tag + '/pred'], g[tag + '/weights'], g[tag + '/gt'], float(g[tag + '/scale']))
        for v in r.values():
            v.setflags(write=False)
        _REF[tag] = r
    return _REF[tag]


def close(got, ref, mag, what, bound=1e-10):
    """|got - ref| <= bound * (sum of the magnitudes of the terms combined), NaN exactly where the reference is NaN; the worst ratio."""
    got, ref, mag = np.asarray(got, np.float64), np.asarray(ref, np.float64), np.asarray(mag, np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), (what, got, ref)
    ok = ~np.isnan(ref)
    err = np.abs(got[ok] - ref[ok])
    assert (err <= bound * np.abs(mag[ok])).all(), (what, float(err.max()))
    nz = np.abs(mag[ok]) > 0
    return float((err[nz] / np.abs(mag[ok])[nz]).max()) if nz.any() else 0.0


def magnitude(ref, k):
    """What the 1e-10 bound of output k is relative to: A + B of the energy scores' A - B, the brier terms' sum, else the value itself."""
    return ref[k + '_mag'] if k in ('es_ade', 'es_fde') else ref[k]


def f32_bound(pred, gt, scale, v):
    """Bound on |float32 ADE / FDE - float64 value v| (tests/test_sample_spread_gpu.py's): the products x * scale are rounded to float32
    before the difference in float64 and after it in bok_dist (<= 2^-24 |x scale| per coordinate of pred and of gt), then Tf + 4 float32
    roundings of the distance sum."""
    big = float(np.nanmax(np.abs(np.concatenate([pred.ravel(), gt.ravel()])))) * abs(scale)
    return 2 * 2.0 ** -24 * (2 * big + (pred.shape[2] + 4) * np.asarray(v, np.float64))


def bad_rows(w):
    return (w < 0).any(axis=1) | ~np.isfinite(w).all(axis=1) | ~(w.astype(np.float64).sum(axis=1) > 0)


def test_fixture_covers_the_kernel_edges(golden):
    g = golden('weighted_set')
    tile = int(g['tile'])
    shapes = [g[t + '/pred'].shape for t in map(str, g['cases'])]
    assert {1, 3, 6, 20, 23, 24, 64} <= {s[1] for s in shapes}
    assert {1, 12, tile + 1, 40} <= {s[2] for s in shapes}
    assert {1, 5, 37} <= {s[0] for s in shapes}
    here = os.path.join(os.path.dirname(__file__), 'golden')
    assert os.path.getsize(os.path.join(here, 'weighted_set.npz')) < os.path.getsize(os.path.join(here, 'scene_metrics.npz'))
    w = g['counts_k20_t12/weights']
    assert (w == np.round(w)).all() and ((w == 0).sum(axis=1) >= 2).any()                      # integer counts with several zeros
    assert len(np.unique(g['equal_k20_t12/weights'])) == 1
    w = g['dominant_k6_t12/weights']
    assert (np.sort(w, axis=1)[:, -1] >= 9 * np.sort(w, axis=1)[:, -2]).all()
    w = g['ties_k23_t33/weights']
    assert (w[:, 2] == w[:, 9]).all() and (w[:, 9] == w[:, 17]).all() and (w[:, 0] == w[:, 22]).all() and (w[:, 3] != w[:, 2]).any()
    for tag in ('special_k6_t12', 'special_k24_t33'):
        w = g[tag + '/weights']
        assert [(w[r] > 0).sum() for r in (0, 1, 2, 6)] == [1, 2, 0, 3]
        assert (w[3] < 0).any() and np.isnan(w[4]).any() and np.isinf(w[5]).any() and bad_rows(w).tolist() == [False, False] + [True] * 4 + [False] * 4
        for k in F64:
            assert np.isnan(g[tag + '/' + k][2:6]).all(), (tag, k)                              # bad rows: NaN everywhere
        assert np.isnan(g[tag + '/ade_top'][2:6]).all() and np.isnan(g[tag + '/fde_top'][2:6]).all()
        assert np.isnan(g[tag + '/kde_nll'][[0, 1]]).all() and np.isfinite(g[tag + '/kde_nll'][6:]).all()   # P = 1, 2: NaN by contract
        assert np.isnan(g[tag + '/apd'][0]) and np.isfinite(g[tag + '/apd'][1]) and g[tag + '/neff'][0] == 1.0
        assert np.isfinite(g[tag + '/eade'][[0, 1]]).all() and np.isfinite(g[tag + '/brier_ade'][[0, 1]]).all()
    assert np.isnan(g['k1_t12/apd']).all() and np.isnan(g['k1_t12/kde_nll']).all() and (g['k1_t12/neff'] == 1.0).all()
    np.testing.assert_array_equal(g['k1_t12/es_ade'], g['k1_t12/eade'])                         # K = 1: no pair term
    np.testing.assert_array_equal(g['k1_t12/brier_ade'], g['k1_t12/ade_top'][:, 0])             # ... and (1 - 1)^2
    for tag in ('counts_k20_t12', 'ties_k23_t33', 'counts_k64_t40'):                            # the clip and the built-singular frames
        deg = g[tag + '/degenerate']
        assert deg.any() and np.array_equal(np.isnan(g[tag + '/kde_nll']), deg.any(axis=1)), tag
        far = np.abs(coords(g[tag + '/gt'], 1.0)[:, None] - coords(g[tag + '/pred'], 1.0)).max(axis=-1).min(axis=1)   # [n, Tf]
        assert ((far > 40).sum(axis=1) >= 2).any(), tag


def test_fixture_conditions_on_the_stored_data(golden):
    """Outside the built-degenerate frames det C >= 1e-3 C00 C11; outside the deliberate duplicates the best and the second-best ADE_k / FDE_k
    differ by more than 1e-5 relative; top rows are non-increasing and repeat beyond the P positive weights."""
    for tag, pred, w, gt, scale, g in cases(golden):
        X = coords(pred, scale)
        n, K, Tf = pred.shape[:3]
        bad = bad_rows(w)
        for a in np.nonzero(~bad)[0]:
            pos = w[a] > 0
            p = w[a].astype(np.float64) / w[a].astype(np.float64).sum()
            if pos.sum() >= 3:
                for t in range(Tf):
                    C = np.cov(X[a, pos, t].T, aweights=p[pos], bias=False)
                    det = C[0, 0] * C[1, 1] - C[0, 1] ** 2
                    if g[tag + '/degenerate'][a, t]:
                        assert not C[0, 0] * C[1, 1] > 0 or abs(det) <= 1e-12 * C[0, 0] * C[1, 1], (tag, a, t)
                    else:
                        assert det >= 1e-3 * C[0, 0] * C[1, 1] > 0, (tag, a, t)
            for k in ('ade', 'fde'):
                v = np.sort(g[tag + '/' + k + '_k'][a][pos])
                if len(v) > 1 and not tag.startswith('dup_'):
                    assert v[1] - v[0] > 1e-5 * v[1], (tag, a, k)
                top = g[tag + '/' + k + '_top'][a]
                assert (top[1:] <= top[:-1]).all() and (top[pos.sum() - 1:] == top[pos.sum() - 1]).all(), (tag, a, k)
                assert top[-1] == g[tag + '/' + k + '_k'][a][pos].min()


def test_restatement_matches_the_fixture(golden):
    """tests/weighted_ref.py (the kernel's order) against the stored array-form values and the stored scipy KDE values."""
    for tag, pred, w, gt, scale, g in cases(golden):
        r = restated(golden, tag)
        for k in F64:
            if k == 'kde_nll':
                assert np.array_equal(np.isnan(r[k]), np.isnan(g[tag + '/' + k])), tag
                ok = ~np.isnan(r[k])
                assert (np.abs(r[k][ok] - g[tag + '/' + k][ok]) <= 1e-8).all(), tag           # test_scene_metrics_gpu.py's bound
            elif k.startswith('brier_'):                               # (double) of the float32 minimum: bok_dist's rounding, as ade_top
                assert np.array_equal(np.isnan(r[k]), np.isnan(g[tag + '/' + k])), (tag, k)
                ok = ~np.isnan(r[k])
                assert (np.abs(r[k][ok] - g[tag + '/' + k][ok]) <= f32_bound(pred, gt, scale, g[tag + '/' + k][ok])).all(), (tag, k)
            else:
                close(r[k], g[tag + '/' + k], magnitude({**{q: g[tag + '/' + q] for q in F64}, 'es_ade_mag': g[tag + '/es_ade_mag'],
                                                         'es_fde_mag': g[tag + '/es_fde_mag']}, k), f'{tag} {k}', 1e-12)
        for k in ('ade_top', 'fde_top'):                              # float32 rows against the float64 ones
            assert r[k].dtype == np.float32 and np.array_equal(np.isnan(r[k]), np.isnan(g[tag + '/' + k])), (tag, k)
            ok = ~np.isnan(r[k])
            assert (np.abs(r[k][ok] - g[tag + '/' + k][ok]) <= f32_bound(pred, gt, scale, g[tag + '/' + k][ok])).all(), (tag, k)


def test_uniform_weights_are_the_sample_spread_formulas(golden):
    """p = 1/K: es_*, apd, fpd are 4s's pair-mean forms, kde_nll is sttode_kde_nll's, the top rows are the running minimum in sample order;
    and a power-of-two multiple of the weights changes no bit of the restatement."""
    for tag in ('equal_k20_t12', 'counts_k24_t12', 'k3_t1', 'counts_k64_t40'):
        g = golden('weighted_set')
        pred, gt, scale = g[tag + '/pred'][:3], g[tag + '/gt'][:3], float(g[tag + '/scale'])
        K = pred.shape[1]
        u = uniform_spread_np(pred, gt, scale)
        for wv in (1.0, 3.0):
            r = weighted_set_np(pred, np.full(pred.shape[:2], wv, np.float32), gt, scale)
            for k in ('apd', 'fpd'):
                close(r[k], u[k], u[k], f'{tag} {k}', 1e-12)
            for k in ('es_ade', 'es_fde'):
                close(r[k], u[k], r[k + '_mag'], f'{tag} {k}', 1e-12)
            assert np.array_equal(np.isnan(r['kde_nll']), np.isnan(u['kde_nll'])), tag
            ok = ~np.isnan(u['kde_nll'])
            assert (np.abs(r['kde_nll'][ok] - u['kde_nll'][ok]) <= 1e-9).all(), tag
            np.testing.assert_allclose(r['neff'], K, rtol=1e-14)
            for a in range(pred.shape[0]):
                ade, fde = bok_f32(pred[a], gt[a], scale)
                np.testing.assert_array_equal(r['ade_top'][a], np.minimum.accumulate(ade))
                np.testing.assert_array_equal(r['fde_top'][a], np.minimum.accumulate(fde))
    g = golden('weighted_set')
    tag = 'special_k6_t12'
    a = restated(golden, tag)
    for f in (2.0 ** 5, 2.0 ** -7):
        b = weighted_set_np(g[tag + '/pred'], g[tag + '/weights'] * np.float32(f), g[tag + '/gt'], 1.0)
        for k in F64 + ('ade_top', 'fde_top'):
            assert a[k].tobytes() == b[k].tobytes() or np.array_equal(np.isnan(a[k]), np.isnan(b[k])) and np.array_equal(
                np.nan_to_num(a[k]), np.nan_to_num(b[k])), (f, k)


def test_entry_point_in_header_table_and_library():
    """Fails without the feature: the entry is exported with equal arity in header, capi.SIGNATURES and the library; the ABI stays 15."""
    from sttode_amd import capi
    from test_capi_symbols import header_functions
    fns = header_functions()
    assert ENTRY in fns and len(fns[ENTRY]) == NARGS
    assert ENTRY in capi.SIGNATURES and len(capi.SIGNATURES[ENTRY]) == NARGS
    assert fns[ENTRY][1] == 'const float* weights' and fns[ENTRY][6] == 'float scale' and fns[ENTRY][7] == 'double* eade'
    assert fns[ENTRY][17] == 'float* ade_top' and fns[ENTRY][19] == 'void* stream'
    assert capi.ABI_VERSION == 15
    if not os.path.exists(capi.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    L = ctypes.CDLL(capi.LIB_PATH)
    assert hasattr(L, ENTRY) and L.sttode_abi_version() == 15
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert '#define STTODE_ABI_VERSION 15' in open(os.path.join(root, 'include', 'sttode_hip.h')).read()


def test_refusals_name_the_entry_point_without_a_device():
    from sttode_amd import capi
    L = capi.lib()
    P = ctypes.c_void_p(16)                                            # (never dereferenced: every call below is refused first)
    one = ctypes.c_float(1.0)
    outs = [P] * 12

    def refused(what, *args):
        rc = getattr(L, ENTRY)(*args)
        err = L.sttode_last_error()
        assert rc != 0 and ENTRY.encode() in err and what in err, (what, err)
    for K in (0, -1, 65):
        refused(b'1 <= K <= 64', P, P, P, 4, K, 12, one, *outs, None)
    refused(b'n and Tf', P, P, P, 0, 20, 12, one, *outs, None)
    refused(b'n and Tf', P, P, P, -2, 20, 12, one, *outs, None)
    refused(b'n and Tf', P, P, P, 4, 20, 0, one, *outs, None)
    for i in range(3):                                                 # pred / weights / gt
        ins = [P, P, P]
        ins[i] = None
        refused(b'null pointer (pred, weights and gt', *ins, 4, 20, 12, one, *outs, None)
    for i in (0, 1, 2, 3, 4, 5, 9):                                    # the required outputs: eade efde es_ade es_fde apd fpd | neff
        o = list(outs)
        o[i] = None
        refused(b'null pointer (eade', P, P, P, 4, 20, 12, one, *o, None)


def test_python_surface_and_host_side_refusals():
    import dataclasses
    import torch
    from sttode_amd import STTODENet, capi, evaluate, metrics
    ps = inspect.signature(metrics.weighted_set).parameters
    assert list(ps) == ['pred_nk', 'weights', 'gt', 'scale'] and ps['scale'].default == 1.0
    ps = inspect.signature(STTODENet.weighted_set).parameters
    assert list(ps)[1:] == ['pred_nk', 'weights', 'gt', 'scale'] and ps['gt'].default is None and ps['scale'].default == 1.0
    assert set(metrics.WeightedSet.__slots__) >= set(F64) | {'ade_top', 'fde_top'}
    assert callable(metrics.WeightedSet.at) and callable(metrics.WeightedSet.record_stream)
    with pytest.raises(capi.SttodeError, match='HIP device only'):     # device-only: no CPU fallback
        metrics.weighted_set(torch.zeros(3, 20, 12, 2), torch.ones(3, 20), torch.zeros(3, 12, 2))
    with pytest.raises(capi.SttodeError, match='HIP device only'):
        metrics.weighted_set(np.zeros((3, 20, 12, 2), np.float32), torch.ones(3, 20), torch.zeros(3, 12, 2))
    for K in (0, 65):
        with pytest.raises(ValueError, match='1 <= K <= 64'):
            metrics.check_weighted_k(K)
    metrics.check_weighted_k(1)
    ps = inspect.signature(evaluate.eval_scenes_reduced).parameters
    assert ps['weighted'].default is False and tuple(ps['ks'].default) == (1, 5, 10)
    f = {x.name: x.default for x in dataclasses.fields(evaluate.EvalReport)}
    for name in ('w_kde_nll', 'w_kde_invalid', 'w_es_ade', 'w_es_fde', 'w_apd', 'w_fpd', 'eade', 'efde', 'brier_ade', 'brier_fde', 'ade_top_k',
                 'fde_top_k', 'mean_neff', 'weighted_agents'):
        assert name in f and f[name] is None, name
    acc = evaluate._ReportAcc(1.0, K=10, weighted=True, ks=(5, 10, 20))
    assert acc.wks == [1, 5, 10] and not evaluate._ReportAcc(1.0, K=10).weighted
