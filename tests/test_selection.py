"""CPU tests of best-of-K selection (utils/metrics.py:7-48 on the device: sttode_best_of_k_select): a NumPy restatement of the kernel's
contract held to the reference's outputs in tests/golden/selection.npz, and the new entry points in header, ctypes table and library."""
import ctypes
import os

import numpy as np
import pytest

from helpers import bok_dist_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def select_np(pred, gt, scale=1.0, thr=1.0, seg_ptr=None):
    """What sttode_best_of_k_select computes, in fp32 and in the kernel's order: per frame |scale (pred - gt)|, the frames summed in order
    and divided by Tf, the minimum over k and its first index (np.argmin), miss = fde > thr; per segment the mean of the agents' values
    and the miss count.  Returns a dict of the kernel's outputs."""
    pred, gt = np.asarray(pred, np.float32), np.asarray(gt, np.float32)
    n, K, Tf = pred.shape[:3]
    dist = bok_dist_np(pred, gt, scale)                                   # [n, K, Tf], with bok_dist's fused multiply-add
    s = np.zeros((n, K), np.float32)
    for t in range(Tf):
        s += dist[..., t]
    va, vf = s / np.float32(Tf), dist[..., -1]
    ia, i_f = np.argmin(va, axis=1), np.argmin(vf, axis=1)
    out = {'ade': va[np.arange(n), ia], 'fde': vf[np.arange(n), i_f], 'best_ade_idx': ia, 'best_fde_idx': i_f}
    out['miss'] = out['fde'] > np.float32(thr)
    out['best'] = pred[np.arange(n), ia]
    if seg_ptr is not None:
        sp = np.asarray(seg_ptr)
        cnt = np.diff(sp).astype(np.float32)
        out['seg_ade'] = np.array([out['ade'][a:b].sum(dtype=np.float32) for a, b in zip(sp[:-1], sp[1:])], np.float32) / cnt
        out['seg_fde'] = np.array([out['fde'][a:b].sum(dtype=np.float32) for a, b in zip(sp[:-1], sp[1:])], np.float32) / cnt
        out['seg_miss'] = np.array([out['miss'][a:b].sum() for a, b in zip(sp[:-1], sp[1:])])
    return out


def cases(golden):
    g = golden('selection')
    for tag in g['cases']:
        tag = str(tag)
        yield tag, g[tag + '/pred'], g[tag + '/gt'], g[tag + '/scene_ptr'], g


def test_restatement_matches_the_reference_metrics(golden):
    seen_k, seen_tf = set(), set()
    for tag, pred, gt, sp, g in cases(golden):
        seen_k.add(pred.shape[1])
        seen_tf.add(pred.shape[2])
        r = select_np(pred, gt, seg_ptr=sp)
        np.testing.assert_array_equal(r['best_ade_idx'], g[tag + '/best_idx'], err_msg=tag)          # get_best_idx
        np.testing.assert_allclose(r['seg_ade'], g[tag + '/scene_ade'], rtol=2e-5, atol=2e-5, err_msg=tag)   # compute_ADE per scene
        np.testing.assert_allclose(r['seg_fde'], g[tag + '/scene_fde'], rtol=2e-5, atol=2e-5, err_msg=tag)   # compute_FDE per scene
        for j, thr in enumerate(g['thresholds']):                                                   # count_miss_samples
            np.testing.assert_array_equal(select_np(pred, gt, thr=thr, seg_ptr=sp)['seg_miss'], g[tag + '/scene_miss'][j],
                                          err_msg=f'{tag} threshold {thr}')
    assert {1, 64} <= seen_k and {1, 12} <= seen_tf


def test_fixture_pins_the_first_index_rule(golden):
    g = golden('selection')
    for tag in ('ties_k20_t12', 'ties_k64_t12'):
        pred, gt, idx = g[tag + '/pred'], g[tag + '/gt'], g[tag + '/best_idx']
        va = select_np(pred, gt)
        ties = 0
        for a in range(pred.shape[0]):
            dup = [k for k in range(pred.shape[1]) if (pred[a, k] == pred[a, idx[a]]).all()]
            assert dup[0] == idx[a], (tag, a, dup, idx[a])            # the reference takes the first of equal samples
            ties += len(dup) > 1
            assert va['best_ade_idx'][a] == idx[a]
        assert ties >= pred.shape[0] // 2, tag
    assert (g['ties_k20_t12/best_idx'][0] == 0)                       # (agent 0: every sample the same)


def test_miss_is_strict():
    pred = np.zeros((2, 3, 4, 2), np.float32)
    gt = np.zeros((2, 4, 2), np.float32)
    pred[0, :, -1, 0] = [1.0, 2.0, 3.0]                              # best fde exactly 1: not a miss at threshold 1
    pred[1, :, -1, 0] = [1.5, 2.0, 1.25]
    r = select_np(pred, gt, thr=1.0)
    assert r['miss'].tolist() == [False, True] and r['best_fde_idx'].tolist() == [0, 2]


def test_selection_entry_points_in_header_table_and_library():
    from sttode_amd import capi
    from test_capi_symbols import header_functions
    fns = header_functions()
    for name, nargs in (('sttode_best_of_k_select', 19), ('sttode_async_best_of_k_select', 20)):
        assert name in fns and len(fns[name]) == nargs, name
        assert name in capi.SIGNATURES and len(capi.SIGNATURES[name]) == nargs, name
    assert fns['sttode_best_of_k_select'][7] == 'const int* seg_ptr' and fns['sttode_best_of_k_select'][13] == 'unsigned char* miss'
    assert capi.ABI_VERSION >= 11
    if not os.path.exists(capi.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    L = ctypes.CDLL(capi.LIB_PATH)
    assert hasattr(L, 'sttode_best_of_k_select') and hasattr(L, 'sttode_async_best_of_k_select')
    assert L.sttode_abi_version() == capi.ABI_VERSION


def test_python_surface_exists():
    from sttode_amd import STTODENet, evaluate, metrics
    for name in ('select_best_of_k', 'select_best_of_k_async'):
        assert callable(getattr(STTODENet, name))
    for name in ('compute_ADE', 'compute_FDE', 'get_best_idx', 'count_miss_samples', 'select'):
        assert callable(getattr(metrics, name))
    for name in ('eval_scenes_report', 'eval_sampler_report', 'eval_nba_report'):
        assert callable(getattr(evaluate, name))


def test_drop_ins_need_a_device():
    """No CPU fallback: without a device the drop-ins raise; with one they answer."""
    import torch
    from sttode_amd import capi, metrics
    args = ([np.zeros((2, 3, 2), np.float32)], np.ones((1, 3, 2), np.float32))
    if torch.cuda.is_available():
        assert metrics.count_miss_samples(*args) == 1 and metrics.get_best_idx(*args) == [0]
        return
    with pytest.raises(capi.SttodeError):
        metrics.compute_ADE(*args)
