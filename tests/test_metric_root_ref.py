"""CPU tests of the float64 yardstick of the per-agent displacement kernels (tests/metric_root_ref.py) and of its cases
(tests/metric_root_cases.py): the yardstick reproduces the reference project's stored outputs within the bands the suite already uses for
them and agrees with oracle.metrics_ref; a float32 evaluation in the kernels' order stays inside the derived bounds on every case; the two
older restatements (test_selection.select_np, helpers.horizon_metrics_np) are that evaluation bit for bit; every case meets its
conditions.  The device side is tests/test_metric_root_gpu.py."""
import numpy as np
import pytest

import metric_root_cases as C
import metric_root_ref as R
from helpers import horizon_metrics_np
from test_selection import select_np

ALL = C.all_cases()


def test_reproduces_the_reference_metrics_fixture(golden):
    g = golden('metrics')
    b = R.best64(g['pred'], g['gt'], 1.0)
    assert abs(b['ade'].mean() - float(g['ade'])) < 1e-6 and abs(b['fde'].mean() - float(g['fde'])) < 1e-6


def test_reproduces_the_reference_selection_fixture(golden):
    g = golden('selection')
    assert tuple(g['thresholds']) == C.THRESHOLDS
    for tag in map(str, g['cases']):
        pred, gt, sp = g[tag + '/pred'], g[tag + '/gt'], g[tag + '/scene_ptr']
        b = R.best64(pred, gt, 1.0)
        np.testing.assert_array_equal(b['ade_idx'], g[tag + '/best_idx'], err_msg=tag)
        for j, thr in enumerate(g['thresholds']):
            sa, sf, sm = R.segments64(b['ade'], b['fde'], sp, thr)
            np.testing.assert_array_equal(sm, g[tag + '/scene_miss'][j], err_msg=f'{tag} {thr}')
        np.testing.assert_allclose(sa, g[tag + '/scene_ade'], rtol=2e-5, atol=2e-5, err_msg=tag)
        np.testing.assert_allclose(sf, g[tag + '/scene_fde'], rtol=2e-5, atol=2e-5, err_msg=tag)


def test_reproduces_the_printed_figures_of_the_nba_fixture(golden):
    g = golden('nba_eval')
    for scale in (1, 3):
        avg, dest, tot = np.zeros(11), np.zeros(11), 0
        for i in range(int(g['n_batches'])):
            pred_kn, fut = g[f'pred{i}'], g[f'fut{i}']
            B, N = fut.shape[:2]
            hm = R.horizon64(np.ascontiguousarray(pred_kn.transpose(1, 0, 2, 3)), fut.reshape(B * N, 10, 2), float(scale))
            avg[1:] += hm[:, :, 0].mean(axis=0) * B
            dest[1:] += hm[:, :, 1].mean(axis=0) * B
            tot += B
        avg, dest = avg / tot, dest / tot
        printed = np.array([(avg[2] + avg[3]) / 2, avg[5], (avg[8] + avg[7]) / 2, avg[10],
                            (dest[2] + dest[3]) / 2, dest[5], (dest[7] + dest[8]) / 2, dest[10]])
        np.testing.assert_allclose(printed, g[f'scale{scale}_printed'], rtol=2e-6)


@pytest.mark.parametrize('case', [(5, 20, 12), (3, 130, 8), (4, 20, 100)], ids=C.case_id)
def test_agrees_with_the_oracle(case):
    """oracle.metrics_ref on the same inputs taken to float64 (it scales the coordinates, the yardstick the difference: a few 1e-16)."""
    from oracle.metrics_ref import best_of_k_ade_fde, nba_horizon_errors
    pred, gt = C.inputs(*case)
    for scale in C.SCALES:
        s = np.float64(np.float32(scale))
        p64, g64 = pred.astype(np.float64) * s, gt.astype(np.float64) * s
        ref = C.reference(*case, scale)
        ade, fde = best_of_k_ade_fde(p64, g64)
        np.testing.assert_allclose(ref['ade'], ade, rtol=1e-12)
        np.testing.assert_allclose(ref['fde'], fde, rtol=1e-12)
        e = nba_horizon_errors(p64.transpose(1, 0, 2, 3), g64, range(1, case[2] + 1))
        for h in range(1, case[2] + 1):
            np.testing.assert_allclose(ref['horizon'][:, h - 1].mean(axis=0), e[h], rtol=1e-12)


def test_first_min_skips_nan_and_takes_the_first_index():
    v = np.array([[np.nan, 2.0, 1.0, 1.0], [np.nan] * 4, [3.0, np.nan, 3.0, 4.0]])
    m, i = R.first_min(v)
    assert m.tolist() == [1.0, np.inf, 3.0] and i.tolist() == [2, 0, 0]


def test_segment_rule():
    """Bounds clamped to [0, n] with a1 >= a0; an empty segment gives NaN means and a zero count."""
    assert R.clamp_csr(C.SEG_CSRS['empty_and_clamped'], 200) == [(0, 10), (10, 10), (10, 150), (150, 200), (200, 200)]
    assert [b - a for a, b in R.clamp_csr(C.SEG_CSRS['sizes_1_63_64_65_7'], 200)] == [1, 63, 64, 65, 7]
    ade, fde = np.arange(200, dtype=np.float32), np.arange(200, dtype=np.float32) / 100
    for fn in (R.segments64, R.segments32):
        sa, sf, sm = fn(ade, fde, C.SEG_CSRS['empty_and_clamped'], 1.0)
        assert np.isnan(sa[[1, 4]]).all() and np.isnan(sf[[1, 4]]).all() and sm.tolist() == [0, 0, 49, 50, 0]
        assert sa[[0, 2, 3]].tolist() == [4.5, 79.5, 174.5]


@pytest.mark.parametrize('case', ALL, ids=C.case_id)
def test_conditions_hold_on_every_agent(case):
    """C.reference asserts them; here the margins are also held to what the draws were chosen for."""
    for scale in C.SCALES:
        ga, gf, away = C.reference(*case, scale)['margins']
        assert ga > 4 * R.bound_ade(case[2]) and gf > 4 * R.bound_fde and away > 4 * R.bound_fde


@pytest.mark.parametrize('case', ALL, ids=C.case_id)
def test_fp32_restatement_within_the_derived_bounds(case):
    n, K, Tf = case
    pred, gt = C.inputs(*case)
    for scale in C.SCALES:
        ref, b = C.reference(*case, scale), R.best32(pred, gt, scale)
        assert R.units(b['ade_k'], ref['ade_k']).max() <= R.bound_ade(Tf) / R.U
        assert R.units(b['fde_k'], ref['fde_k']).max() <= R.bound_fde / R.U
        assert R.units(b['ade'], ref['ade']).max() <= R.bound_ade(Tf) / R.U and R.units(b['fde'], ref['fde']).max() <= R.bound_fde / R.U
        np.testing.assert_array_equal(b['ade_idx'], ref['ade_idx'])
        np.testing.assert_array_equal(b['fde_idx'], ref['fde_idx'])
        hm = horizon_metrics_np(pred, gt, scale)
        assert (R.units(hm, ref['horizon']) <= R.bound_horizon(Tf)[None] / R.U).all()


@pytest.mark.parametrize('name', list(C.SEG_CSRS))
def test_fp32_segment_sums_within_the_derived_bound(name):
    pred, gt = C.inputs(*C.SEG_CASE)
    sp = C.SEG_CSRS[name]
    sizes = [b - a for a, b in R.clamp_csr(sp, C.SEG_CASE[0])]
    for scale in C.SCALES:
        ref, b = C.reference(*C.SEG_CASE, scale), R.best32(pred, gt, scale)
        for thr in C.THRESHOLDS:
            s32, own, full = (fn(x['ade'], x['fde'], sp, thr) for fn, x in ((R.segments32, b), (R.segments64, b), (R.segments64, ref)))
            np.testing.assert_array_equal(s32[2], full[2])
            for j in (0, 1):
                assert np.array_equal(np.isnan(s32[j]), [na == 0 for na in sizes])
                for s, na in enumerate(sizes):
                    if na:
                        assert R.units(s32[j][s], own[j][s]) <= R.bound_seg(na) / R.U
                        assert R.units(s32[j][s], full[j][s]) <= (R.bound_seg(na) + (R.bound_ade(C.SEG_CASE[2]), R.bound_fde)[j]) / R.U


@pytest.mark.parametrize('case', ALL, ids=C.case_id)
def test_older_restatements_are_the_same_fp32_evaluation(case):
    """select_np and horizon_metrics_np against per_sample32, bit for bit."""
    pred, gt = C.inputs(*case)
    for scale in C.SCALES:
        b, r = R.best32(pred, gt, scale), select_np(pred, gt, scale=scale)
        for f in ('ade', 'fde'):
            assert np.array_equal(r[f], b[f]), f
        assert np.array_equal(r['best_ade_idx'], b['ade_idx']) and np.array_equal(r['best_fde_idx'], b['fde_idx'])
        d = np.stack([b['ade_k'], b['fde_k']], axis=-1)
        hm = horizon_metrics_np(pred, gt, scale)
        assert np.array_equal(hm[:, -1], d.min(axis=1))                           # the last horizon is the ADE / FDE
    sp = C.SEG_CSRS['sizes_1_63_64_65_7']
    if case == C.SEG_CASE:                                                        # select_np's segments: a plain in-order float32 sum
        r = select_np(pred, gt, thr=1.0, seg_ptr=np.array(sp))
        np.testing.assert_array_equal(r['seg_miss'], R.segments64(r['ade'], r['fde'], sp, 1.0)[2])
