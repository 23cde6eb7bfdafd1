"""CPU tests of the multi-modal ground truth metrics (sttode_multimodal): tests/golden/multimodal.npz checked against itself --
a loop restatement in the kernel's order (j in tiles of 64 lanes, history components in order, neighbours in ascending j, frames in frame
order) against the stored array-form values, the identities at eps = 0 and at a huge eps, the symmetry of the neighbour relation, the maker's
margin condition -- and the new entry point in header, ctypes table and library, its refusals, and the Python surface."""
import ctypes
import os

import numpy as np
import pytest

MM_CASES = ('n1', 'n63_k1_t1', 'n64_k3_h3', 'n65_k20_h19', 'n8_k64_t33', 'n257_k3', 'eps0_twins', 'huge_h4', 'seg', 'seg_huge', 'nan_k5',
            'scale50', 'far')


def coords(x, scale):
    return (np.asarray(x, np.float32) * np.float32(scale)).astype(np.float64)


def segment_of(n, seg_ptr):
    """(a0, a1) [n]: the bounds of every agent's segment."""
    if seg_ptr is None:
        return np.zeros(n, np.int64), np.full(n, n, np.int64)
    s = np.repeat(np.arange(len(seg_ptr) - 1), np.diff(seg_ptr))
    return np.asarray(seg_ptr, np.int64)[s], np.asarray(seg_ptr, np.int64)[s + 1]


def multimodal_np(pred, past, gt, scale, eps, h, seg_ptr=None):
    """What sttode_multimodal computes, in its order: per agent i the lanes j = j0 .. j0 + 63 of a tile add (H_i[c] - H_j[c])^2 over the
    components c in order; the matches are taken in ascending j; per match the lanes k add the frames' distances in frame order, the minimum
    over k (NaN counted as +inf) is added to the running sums.  Returns count, mmade, mmfde and the neighbour matrix."""
    X, P, Y = coords(pred, scale), coords(past, scale), coords(gt, scale)
    n, K, Tf = X.shape[:3]
    Tp = P.shape[1]
    A = P[:, Tp - 1]
    H = (P[:, Tp - 1 - h:Tp - 1] - A[:, None]).reshape(n, 2 * h)
    a0, a1 = segment_of(n, seg_ptr)
    count, mmade, mmfde = np.zeros(n, np.int32), np.zeros(n), np.zeros(n)
    M = np.zeros((n, n), bool)
    with np.errstate(invalid='ignore'):
        for i in range(n):
            sa = sf = 0.0
            for j0 in range(a0[i], a1[i], 64):
                js = np.arange(j0, min(j0 + 64, a1[i]))
                s = np.zeros(len(js))
                for c in range(2 * h):
                    d = H[i, c] - H[js, c]
                    s = s + d * d
                for j in js[(js == i) | (np.sqrt(s) <= eps)]:
                    M[i, j] = True
                    tot, last = np.zeros(K), np.zeros(K)
                    for t in range(Tf):
                        g = (Y[j, t] - A[j]) + A[i]
                        dx, dy = X[i, :, t, 0] - g[0], X[i, :, t, 1] - g[1]
                        last = np.sqrt(dx * dx + dy * dy)
                        tot = tot + last
                    va, vf = tot / Tf, last
                    sa += np.where(np.isnan(va), np.inf, va).min()
                    sf += np.where(np.isnan(vf), np.inf, vf).min()
                    count[i] += 1
            mmade[i], mmfde[i] = sa / count[i], sf / count[i]
    return count, mmade, mmfde, M


def cases(golden):
    g = golden('multimodal')
    for tag in map(str, g['cases']):
        sp = g[tag + '/seg_ptr'] if tag + '/seg_ptr' in g else None
        yield tag, g[tag + '/pred'], g[tag + '/past'], g[tag + '/gt'], float(g[tag + '/scale']), float(g[tag + '/eps']), int(g[tag + '/h']), sp, g


def close(got, ref, cmag, what, bound=1e-10):
    """|got - ref| <= bound * (|ref| + cmag), +inf where the reference is +inf; returns the worst ratio."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert not np.isnan(ref).any() and np.array_equal(np.isinf(got), np.isinf(ref)) and not np.isnan(got).any(), what
    ok = np.isfinite(ref)
    ratio = np.abs(got[ok] - ref[ok]) / (np.abs(ref[ok]) + cmag)
    assert (ratio <= bound).all(), (what, float(ratio.max()))
    return float(ratio.max()) if ok.any() else 0.0


def best_of_k_np(pred, gt, scale):
    """float64 best-of-K ADE / FDE per agent, NaN samples skipped."""
    D = np.linalg.norm(coords(pred, scale) - coords(gt, scale)[:, None], axis=-1)     # [n, K, Tf]
    ade, fde = D.mean(axis=-1), D[..., -1]
    return np.where(np.isnan(ade), np.inf, ade).min(axis=1), np.where(np.isnan(fde), np.inf, fde).min(axis=1)


def test_fixture_covers_the_kernel_edges(golden):
    g = golden('multimodal')
    assert tuple(map(str, g['cases'])) == MM_CASES
    tile, chunk = int(g['tile']), int(g['chunk'])
    shapes = {t: (g[t + '/pred'].shape, g[t + '/past'].shape[1], int(g[t + '/h'])) for t in MM_CASES}
    assert {1, tile - 1, tile, tile + 1, 4 * tile + 1} <= {s[0][0] for s in shapes.values()}
    assert {1, 3, 20, 64} <= {s[0][1] for s in shapes.values()} and {1, 12, 33} <= {s[0][2] for s in shapes.values()}
    assert {(2, 1), (8, 3), (8, 7), (20, 19)} <= {(s[1], s[2]) for s in shapes.values()}
    assert {2 * s[2] for s in shapes.values()} >= {2, chunk, chunk + 6, 4 * chunk + 6}   # short, one whole chunk, a chunk and a short one
    assert {0.5, 1.0, 50.0} <= {float(g[t + '/scale']) for t in MM_CASES}
    assert os.path.getsize(os.path.join(os.path.dirname(__file__), 'golden', 'multimodal.npz')) < 1 << 20
    sp = g['seg/seg_ptr']
    assert np.diff(sp).tolist() == [1, 64, 65, 64] and sp[2] % 4 != 0 and np.array_equal(sp, g['seg_huge/seg_ptr'])
    assert max(int(g[t + '/count'].max()) for t in MM_CASES if float(g[t + '/eps']) < 100) >= 20       # non-trivial neighbour sets
    assert all(g[t + '/count'].dtype == np.int32 and (g[t + '/count'] >= 1).all() for t in MM_CASES)
    # the NaN case: one NaN sample and one NaN coordinate are skipped, an agent without a finite sample gets +inf, a NaN history keeps only itself
    c, a = g['nan_k5/count'], g['nan_k5/mmade']
    assert np.isfinite(a[0]) and np.isfinite(a[4]) and np.isinf(a[1]) and np.isinf(g['nan_k5/mmfde'][1]) and np.isfinite(np.delete(a, 1)).all()
    assert c[2] == 1 and np.isnan(g['nan_k5/past'][2]).any()
    assert g['far/mmade'].max() > 50.0


def test_restatement_in_the_kernels_order_matches_the_fixture(golden):
    for tag, pred, past, gt, scale, eps, h, sp, g in cases(golden):
        count, mmade, mmfde, M = multimodal_np(pred, past, gt, scale, eps, h, sp)
        np.testing.assert_array_equal(count, g[tag + '/count'], err_msg=tag)
        cmag = float(g[tag + '/cmag'])
        close(mmade, g[tag + '/mmade'], cmag, f'{tag} mmade', 1e-13)
        close(mmfde, g[tag + '/mmfde'], cmag, f'{tag} mmfde', 1e-13)
        assert np.array_equal(M, M.T), tag                              # j in S_i <=> i in S_j
        assert M.diagonal().all() and np.array_equal(M.sum(axis=1), count), tag
        if tag == 'nan_k5':
            assert M[2].sum() == 1 and M[:, 2].sum() == 1                # the agent with a NaN history enters nobody else's set


def test_identities_at_eps_zero_and_at_a_huge_eps(golden):
    g = golden('multimodal')
    t = 'eps0_twins'
    count = g[t + '/count']
    assert float(g[t + '/eps']) == 0.0 and np.array_equal(g[t + '/past'][3], g[t + '/past'][40])
    assert count[3] == 2 and count[40] == 2 and (np.delete(count, [3, 40]) == 1).all()     # the twins find each other, nobody else does
    ade, fde = best_of_k_np(g[t + '/pred'], g[t + '/gt'], float(g[t + '/scale']))
    one = count == 1
    close(g[t + '/mmade'][one], ade[one], float(g[t + '/cmag']), 'eps 0: mmade is best-of-K ADE', 1e-13)
    close(g[t + '/mmfde'][one], fde[one], float(g[t + '/cmag']), 'eps 0: mmfde is best-of-K FDE', 1e-13)
    assert g[t + '/mmade'][3] != ade[3]
    assert (g['huge_h4/count'] == 65).all()
    a0, a1 = segment_of(194, g['seg_huge/seg_ptr'])
    np.testing.assert_array_equal(g['seg_huge/count'], a1 - a0)
    a0, a1 = segment_of(194, g['seg/seg_ptr'])
    assert (g['seg/count'] <= a1 - a0).all() and g['seg/count'][0] == 1


def test_no_pair_of_the_fixture_lies_on_the_threshold(golden):
    """The maker's condition, from the stored arrays: no pair of a segment has |d_hist - eps| < 1e-9 eps (eps = 0: d_hist is exactly 0 or
    clearly positive)."""
    g = golden('multimodal')
    assert float(g['margin_required']) == 1e-9
    for tag, pred, past, gt, scale, eps, h, sp, _ in cases(golden):
        P = coords(past, scale)
        H = (P[:, P.shape[1] - 1 - h:P.shape[1] - 1] - P[:, -1][:, None]).reshape(len(P), 2 * h)
        with np.errstate(invalid='ignore'):
            D = np.sqrt(((H[:, None] - H[None]) ** 2).sum(axis=-1))
        a0, _a1 = segment_of(len(P), sp)
        pair = (a0[:, None] == a0[None]) & ~np.eye(len(P), dtype=bool) & ~np.isnan(D)
        if not pair.any():
            continue
        if eps == 0.0:
            assert ((D[pair] == 0.0) | (D[pair] > 1e-3)).all(), tag
        else:
            m = float((np.abs(D[pair] - eps) / eps).min())
            assert m >= 1e-9 and abs(m - float(g[tag + '/margin'])) <= 1e-6 * m, (tag, m)


def test_entry_point_in_header_table_and_library():
    from sttode_amd import capi
    from test_capi_symbols import header_functions
    fns = header_functions()
    assert 'sttode_multimodal' in fns and len(fns['sttode_multimodal']) == 18 == len(capi.SIGNATURES['sttode_multimodal'])
    f = fns['sttode_multimodal']
    assert f[3] == 'const int* seg_ptr_or_NULL' and f[10] == 'float scale' and f[11] == 'double eps' and f[13] == 'long ws_doubles'
    assert f[14] == 'int* count' and f[16] == 'double* mmfde' and f[17] == 'void* stream'
    assert capi.ABI_VERSION == 15
    if not os.path.exists(capi.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    L = ctypes.CDLL(capi.LIB_PATH)
    assert hasattr(L, 'sttode_multimodal') and L.sttode_abi_version() == 15


def test_refusals_name_the_entry_point_without_a_device():
    from sttode_amd import capi
    L = capi.lib()
    P = ctypes.c_void_p(16)                                            # (never dereferenced: every call below is refused first)
    ok = dict(pred=P, past=P, gt=P, seg=None, n_seg=0, n=4, K=20, Tp=8, Tf=12, h=7, scale=1.0, eps=0.3, ws=P, ws_doubles=64, count=P, mmade=P,
              mmfde=P)

    def refused(what, **kw):
        a = {**ok, **kw}
        rc = L.sttode_multimodal(a['pred'], a['past'], a['gt'], a['seg'], a['n_seg'], a['n'], a['K'], a['Tp'], a['Tf'], a['h'],
                                 ctypes.c_float(a['scale']), ctypes.c_double(a['eps']), a['ws'], a['ws_doubles'], a['count'], a['mmade'],
                                 a['mmfde'], None)
        err = L.sttode_last_error()
        assert rc != 0 and b'sttode_multimodal' in err and what in err, (kw, err)
    for name in ('pred', 'past', 'gt', 'ws', 'count', 'mmade', 'mmfde'):
        refused(b'null pointer', **{name: None})
    for n in (0, -1, (1 << 20) + 1):
        refused(b'n <= 2^20', n=n, ws_doubles=1 << 40)
    for K in (0, 65):
        refused(b'1 <= K <= 64', K=K)
    refused(b'Tf must be positive', Tf=0)
    refused(b'Tp >= 2', Tp=1, h=1)
    for h in (0, 8, -3):
        refused(b'hist_frames <= Tp - 1', h=h)
    for eps in (-1e-9, float('inf'), float('nan')):
        refused(b'eps must be', eps=eps)
    for scale in (float('inf'), float('nan')):
        refused(b'scale must be finite', scale=scale)
    refused(b'workspace too small', ws_doubles=63)
    refused(b'workspace too small', ws_doubles=0)
    refused(b'seg_ptr', seg=P, n_seg=0)
    refused(b'seg_ptr', seg=None, n_seg=2)


def test_python_surface_and_host_side_refusals():
    import dataclasses
    import inspect
    import torch
    from sttode_amd import capi, evaluate, metrics
    ps = inspect.signature(metrics.multimodal).parameters
    assert list(ps) == ['pred_nk', 'past', 'gt', 'eps', 'hist_frames', 'scale', 'seg_ptr']
    assert ps['hist_frames'].default is None and ps['scale'].default == 1.0 and ps['seg_ptr'].default is None
    assert set(metrics.MultiModal.__slots__) >= {'count', 'mmade', 'mmfde'} and callable(metrics.MultiModal.record_stream)
    with pytest.raises(capi.SttodeError, match='HIP device only'):     # device-only: no CPU fallback
        metrics.multimodal(torch.zeros(3, 20, 12, 2), torch.zeros(3, 8, 2), torch.zeros(3, 12, 2), 0.3)
    assert metrics.check_multimodal(5, 20, 8, 12, 1, None, 1.0) == (1.0, 7) and metrics.check_multimodal(5, 20, 8, 12, 0, 3, 2.0) == (0.0, 3)
    for bad, what in ((dict(n=0), '2\\^20'), (dict(n=(1 << 20) + 1), '2\\^20'), (dict(K=0), '1 <= K <= 64'), (dict(K=65), '1 <= K <= 64'),
                      (dict(Tp=1), 'Tp >= 2'), (dict(hist_frames=0), 'hist_frames'), (dict(hist_frames=8), 'hist_frames'),
                      (dict(eps=-1.0), 'eps'), (dict(eps=float('inf')), 'eps'), (dict(eps=float('nan')), 'eps'),
                      (dict(scale=float('inf')), 'scale'), (dict(scale=float('nan')), 'scale')):
        kw = {**dict(n=5, K=20, Tp=8, Tf=12, eps=0.3, hist_frames=None, scale=1.0), **bad}
        with pytest.raises(ValueError, match=what):
            metrics.check_multimodal(**kw)
    ps = inspect.signature(evaluate.eval_scenes_multimodal).parameters
    assert list(ps) == ['model', 'dataset', 'eps', 'hist_frames', 'within', 'traj_scale', 'scenes_per_call', 'z_fn', 'pipelined', 'sampler',
                        'mean', 'eps_fn']
    assert ps['within'].default == 'dataset' and ps['scenes_per_call'].default == 512 and ps['pipelined'].default is True
    names = [f.name for f in dataclasses.fields(evaluate.MultiModalReport)]
    assert names[:7] == ['mmade', 'mmfde', 'n_agents', 'mean_count', 'frac_multi', 'mmade_multi', 'mmfde_multi']
    assert {'count', 'mmade_agents', 'mmfde_agents'} <= set(names)


def test_segments_within_a_file_follow_the_sequence_names():
    from sttode_amd.evaluate import multimodal_segments

    class Stub:
        seq_name = ['eth', 'eth', 'hotel', 'hotel', 'hotel', 'eth', 'zara']
    ptr = np.array([0, 3, 4, 9, 10, 12, 20, 21])
    assert multimodal_segments(Stub(), ptr, 'dataset') is None
    sp = multimodal_segments(Stub(), ptr, 'file')
    assert sp.dtype == np.int32 and sp.tolist() == [0, 4, 12, 20, 21]   # a name that comes back later is a new segment: only neighbours join
    sp = multimodal_segments(Stub(), ptr, 'scene')
    assert sp.dtype == np.int32 and sp.tolist() == ptr.tolist()
    one = multimodal_segments(type('One', (), {'seq_name': ['a', 'a']})(), np.array([0, 2, 5]), 'file')
    assert one.tolist() == [0, 5]
    with pytest.raises(ValueError, match='within'):
        multimodal_segments(Stub(), ptr, 'recording')
    with pytest.raises(ValueError, match='seq_name'):
        multimodal_segments(object(), ptr, 'file')
    with pytest.raises(ValueError, match='seq_name'):
        multimodal_segments(type('Short', (), {'seq_name': ['a']})(), ptr, 'file')
