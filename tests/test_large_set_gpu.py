"""GPU tests of the large-set scores (sttode_large_select / _kde_nll / _spread, csrc/large_set.hip) and the layers above them:
metrics.large_*, STTODENet.score_samples / inference_reduced_samples, evaluate.eval_scenes_reduced_raw.

Bounds.  Selection: ade / fde / *_at are the BITS of tests/weighted_ref.py's float32 walk in bok_dist order.  Beside that they are held to
the stored float64 values of the same formula within (Tf + 3) 2^-23 relative: in units of 2^-24, a displacement carries 2 (the difference,
the scale), its square 4, dy dy and the fused add one each, the root halves that and adds one -- 3.5 per distance -- and a sum of Tf
distances adds Tf - 1; (Tf + 3) 2^-23 is above that worst case at every Tf, and a quarter of the fixture's gaps at most.  Indices, miss flags and
joint indices equal the stored ones (the fixture's gaps are sixteen times what a float32 sum of Tf terms can move); seg_jade / seg_jfde within 1 float32 ulp of the double sum, in agent order, of the walk's values.  KDE NLL: the stored NaN
pattern and atol = 1e-8 on the rest, the bound tests/test_scene_metrics_gpu.py holds kde_nll_kernel to against gaussian_kde.  Pair
statistics: |got - ref| <= 1e-10 x the sum of the magnitudes of the terms combined (4s's rule).  The kernel's longest chain of additions
at M = 4096, Tf = 2 is 33 tiles x 16 pairs per thread + 6 + 2 (xor tree, waves) + 64 workgroups < 700 additions, a worst case of
700 x 2^-53 = 8e-14 relative: the 1e-10 holds at every M without widening.

No input here is beyond the entries' limits except in the refusal test, whose calls launch nothing."""
import ctypes
import dataclasses

import numpy as np
import pytest
import torch

import large_set_ref as ref
from test_large_set import case
from test_reduce_gpu import _dataset, _gpu, _model, _z_fn

pytestmark = pytest.mark.gpu
EPS32 = 2.0 ** -23
SEL = [t for t, c in ref.CASES.items() if 's' in c['parts']]
KDE = [t for t, c in ref.CASES.items() if 'k' in c['parts']]
SPR = [t for t, c in ref.CASES.items() if 'p' in c['parts']]
_EXPECT = {}


def _dev(a):
    return torch.from_numpy(np.array(a)).to(_gpu())                       # (a copy: the shared cases are read-only)


def _np(t):
    return None if t is None else t.cpu().numpy()


def _sel_np(ls):
    torch.cuda.synchronize()
    return {k: _np(getattr(ls, k)) for k in ls.__slots__ if k not in ('M', 'ks')}


def _spr_np(sp):
    torch.cuda.synchronize()
    return {k: _np(getattr(sp, k)) for k in ('apd', 'fpd', 'pade', 'dlow', 'es_ade', 'es_fde')}


def _bits(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), what


def _same(d0, d1, what):
    for k in d0:
        assert (d0[k] is None) == (d1[k] is None), (what, k)
        if d0[k] is not None:
            _bits(d0[k], d1[k], (what, k))


def _expected_f32(golden, tag):
    """The selection's outputs from the float32 walk, once per case."""
    if tag not in _EXPECT:
        c, g, pred5, x, gt, info = case(golden, tag)
        va, vf = ref.select_f32(x, gt, c['scale'])
        _EXPECT[tag] = ref.select_from(va, vf, c['thr'], list(g[tag + '/ks']), g[tag + '/seg_ptr'])
    return _EXPECT[tag]


def _ulp32(got, want64, what, ulps=1):
    w = want64.astype(np.float32)
    fin = np.isfinite(want64)
    assert (np.isnan(got) == np.isnan(want64)).all() and (got[~fin & ~np.isnan(want64)] == w[~fin & ~np.isnan(want64)]).all(), what
    assert (np.abs(got[fin].astype(np.float64) - want64[fin]) <= ulps * np.spacing(np.abs(w[fin])).astype(np.float64)).all(), what


# ----- against the fixture -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('tag', SEL)
def test_select_against_the_fixture(golden, tag):
    from sttode_amd import metrics
    c, g, pred5, x, gt, info = case(golden, tag)
    ks, sp = list(g[tag + '/ks']), g[tag + '/seg_ptr']
    got = _sel_np(metrics.large_select(_dev(pred5), _dev(gt), scale=c['scale'], miss_threshold=c['thr'], ks=ks, seg_ptr=sp))
    e32 = _expected_f32(golden, tag)
    for name in ('ade', 'fde'):
        _bits(got[name], e32[name], (tag, name))
        _bits(got[name + '_at'], e32[name + '_at'], (tag, name + '_at'))
        for k, want in ((name, g[f'{tag}/{name}']), (name + '_at', g[f'{tag}/{name}_at'])):
            fin = np.isfinite(want)
            assert (got[k][~fin] == want[~fin]).all(), (tag, k)
            assert (np.abs(got[k][fin] - want[fin]) <= (c['Tf'] + 3) * EPS32 * np.abs(want[fin])).all(), (tag, k)
        np.testing.assert_array_equal(got[f'best_{name}_idx'], g[f'{tag}/{name}_idx'], err_msg=tag)
        np.testing.assert_array_equal(got[f'best_{name}_idx'], e32[name + '_idx'], err_msg=tag)
        np.testing.assert_array_equal(got[f'seg_j{name}_idx'], g[f'{tag}/seg_j{name}_idx'], err_msg=tag)
        _ulp32(got['seg_j' + name], e32['seg_j' + name], (tag, 'seg_j' + name))
        want = g[f'{tag}/seg_j{name}']
        fin = np.isfinite(want)
        assert (np.abs(got['seg_j' + name][fin] - want[fin]) <= (c['Tf'] + 3) * EPS32 * np.abs(want[fin])).all(), (tag, 'seg_j' + name)
    np.testing.assert_array_equal(got['miss'], g[tag + '/miss'], err_msg=tag)
    n, M = x.shape[:2]
    one = np.nonzero(np.diff(sp) == 1)[0]                                 # one-agent segments reproduce the agent's values bitwise
    for name in ('ade', 'fde'):
        _bits(got['seg_j' + name][one], got[name][sp[one]], (tag, 'one-agent segments'))
        _bits(got[f'seg_j{name}_idx'][one], got[f'best_{name}_idx'][sp[one]], (tag, 'one-agent segments'))
        assert ((got[f'best_{name}_idx'] >= 0) & (got[f'best_{name}_idx'] < M)).all()


@pytest.mark.parametrize('tag', KDE)
def test_kde_against_the_fixture(golden, tag):
    from sttode_amd import metrics
    c, g, pred5, x, gt, info = case(golden, tag)
    got = metrics.large_kde_nll(_dev(pred5), _dev(gt), scale=c['scale']).cpu().numpy()
    want = g[tag + '/kde']
    ok = ~np.isnan(want)
    assert got.dtype == np.float64 and (np.isnan(got) == ~ok).all(), (tag, got, want)
    print(tag, 'max |kde - scipy| = %.3e' % (np.abs(got[ok] - want[ok]).max() if ok.any() else 0.0))
    np.testing.assert_allclose(got[ok], want[ok], rtol=0, atol=1e-8, err_msg=tag)


@pytest.mark.parametrize('tag', SPR)
def test_spread_against_the_fixture(golden, tag):
    from sttode_amd import metrics
    c, g, pred5, x, gt, info = case(golden, tag)
    got = _spr_np(metrics.large_spread(_dev(pred5), _dev(gt), scale=c['scale'], div_scale=c['div']))
    for name in ('apd', 'fpd', 'pade', 'dlow', 'es_ade', 'es_fde'):
        want = g[f'{tag}/{name}']
        mag = g[f'{tag}/{name}_mag'] if name.startswith('es_') else np.abs(want)          # (the pair means add positive terms)
        print(tag, name, 'max |got - ref| / mag = %.3e' % (np.abs(got[name] - want) / mag).max())
        assert (np.abs(got[name] - want) <= 1e-10 * mag).all(), (tag, name)
    nogt = _spr_np(metrics.large_spread(_dev(pred5), scale=c['scale'], div_scale=c['div']))
    assert nogt['es_ade'] is None and nogt['es_fde'] is None
    for name in ('apd', 'fpd', 'pade', 'dlow'):
        _bits(nogt[name], got[name], (tag, name, 'without gt'))


# ----- ties to the one-lane-per-sample kernels at M <= 64 ------------------------------------------------------------------------------

@pytest.mark.parametrize('tag', ['m3_t1', 'm64_t12'])
def test_small_sets_tie_to_the_existing_kernels(golden, tag):
    from sttode_amd import metrics
    c, g, pred5, x, gt, info = case(golden, tag)
    xd, gd, sp = _dev(x), _dev(gt), g[tag + '/seg_ptr']                     # R = 1: the plain [n, M, Tf, 2]
    M = x.shape[1]
    ks = [k for k in g[tag + '/ks'] if k <= 64]
    got = _sel_np(metrics.large_select(xd, gd, scale=c['scale'], miss_threshold=c['thr'], ks=ks, seg_ptr=sp))
    old = metrics.select(xd, gd, scale=c['scale'], miss_threshold=c['thr'])
    torch.cuda.synchronize()
    for a, b in (('ade', old.ade), ('fde', old.fde), ('best_ade_idx', old.best_ade_idx), ('best_fde_idx', old.best_fde_idx), ('miss', old.miss)):
        _bits(got[a], _np(b), (tag, a, 'against metrics.select'))
    for i, k in enumerate(ks):
        first = metrics.select(xd[:, :k].contiguous(), gd, scale=c['scale'])
        _bits(got['ade_at'][:, i], _np(first.ade), (tag, 'ade_at', k))
        _bits(got['fde_at'][:, i], _np(first.fde), (tag, 'fde_at', k))
    js = metrics.joint_select(xd, gd, sp, scale=c['scale'])
    full = np.diff(sp) > 0                                                # (an empty segment: NaN / 0 there, NaN / -1 here, as documented)
    for name in ('jade', 'jfde'):
        np.testing.assert_array_equal(got[f'seg_{name}_idx'][full], _np(getattr(js, f'seg_{name}_idx'))[full])
        _ulp32(got['seg_' + name][full], _np(getattr(js, 'seg_' + name))[full].astype(np.float64), (tag, name))
        assert np.isnan(got['seg_' + name][~full]).all() and (got[f'seg_{name}_idx'][~full] == -1).all()
    kd, kd_old = metrics.large_kde_nll(xd, gd, scale=c['scale']).cpu().numpy(), metrics.kde_nll(xd, gd, scale=c['scale']).cpu().numpy()
    np.testing.assert_allclose(kd, kd_old, rtol=0, atol=1e-9)
    sp_new = _spr_np(metrics.large_spread(xd, gd, scale=c['scale'], div_scale=c['div']))
    sp_old = metrics.sample_spread(xd, gd, scale=c['scale'], div_scale=c['div'])
    for name in ('apd', 'fpd', 'pade', 'dlow', 'es_ade', 'es_fde'):
        mag = g[f'{tag}/{name}_mag'] if name.startswith('es_') else np.abs(g[f'{tag}/{name}'])
        assert (np.abs(sp_new[name] - _np(getattr(sp_old, name))) <= 1e-10 * mag).all(), (tag, name)


# ----- layout and properties -----------------------------------------------------------------------------------------------------------

def _all_outputs(pred, gt, c, ks, sp):
    from sttode_amd import metrics
    out = _sel_np(metrics.large_select(pred, gt, scale=c['scale'], miss_threshold=c['thr'], ks=ks, seg_ptr=sp))
    out['kde'] = metrics.large_kde_nll(pred, gt, scale=c['scale']).cpu().numpy()
    out.update(_spr_np(metrics.large_spread(pred, gt, scale=c['scale'], div_scale=c['div'])))
    return out


@pytest.mark.parametrize('tag', ['m64_t12', 'm256_t12', 'm400_r20_dup'])
def test_round_major_layout_gives_the_bits_of_the_flat_one_and_two_runs_agree(golden, tag):
    c, g, pred5, x, gt, info = case(golden, tag)
    ks, sp = list(g[tag + '/ks']), g[tag + '/seg_ptr']
    a = _all_outputs(_dev(pred5), _dev(gt), c, ks, sp)
    b = _all_outputs(_dev(x), _dev(gt), c, ks, sp)
    a2 = _all_outputs(_dev(pred5), _dev(gt), c, ks, sp)
    for k in a:
        _bits(a[k], b[k], (tag, k, 'round-major against flat'))
        _bits(a[k], a2[k], (tag, k, 'two runs'))


@pytest.mark.parametrize('tag,front', [('m257_t33', 1), ('m400_r20_dup', 3), ('m4096_t2', 2)])
def test_outputs_do_not_depend_on_the_rest_of_the_batch(golden, tag, front):
    """`front` agents put in front of the batch (a segment of their own) and a segment of two agents appended behind it: the batch's own
    agents and segments keep every bit."""
    c, g, pred5, x, gt, info = case(golden, tag)
    ks, sp = list(g[tag + '/ks']), g[tag + '/seg_ptr']
    n = x.shape[0]
    rng = np.random.default_rng(5)
    extra = lambda k: (rng.normal(0, 1, (pred5.shape[0], k) + pred5.shape[2:]).astype(np.float32),   # noqa: E731
                       rng.normal(0, 1, (k,) + gt.shape[1:]).astype(np.float32))
    (pf, gf), (pb, gb) = extra(front), extra(2)
    big_p, big_g = np.concatenate([pf, pred5, pb], axis=1), np.concatenate([gf, gt, gb])
    big_sp = np.concatenate([[0], sp + front, [n + front + 2]]).astype(np.int32)
    alone = _all_outputs(_dev(pred5), _dev(gt), c, ks, sp)
    inside = _all_outputs(_dev(big_p), _dev(big_g), c, ks, big_sp)
    for k in alone:
        cut = inside[k][1:-1] if k.startswith('seg_') else inside[k][front:front + n]
        _bits(alone[k], cut, (tag, k))


def test_refused_calls_write_nothing():
    """Calls beyond the limits, straight at the C ABI with live device buffers: non-zero status, the entry named, and every output and the
    workspace still hold their sentinel."""
    from sttode_amd import capi
    L, dev = capi.lib(), _gpu()
    n, Tf = 3, 4
    pred, gt = torch.zeros(n * 70 * Tf * 2, device=dev), torch.zeros(n, Tf, 2, device=dev)
    f32 = torch.full((16 * n,), -7.0, device=dev)
    i32 = torch.full((16 * n,), -7, dtype=torch.int32, device=dev)
    f64 = torch.full((16 * n,), -7.0, dtype=torch.float64, device=dev)
    u8 = torch.full((n,), 9, dtype=torch.uint8, device=dev)
    ws = torch.full((1 << 16,), 5, dtype=torch.uint8, device=dev)
    sp = torch.tensor([0, 1, 3], dtype=torch.int32, device=dev)
    ks = (ctypes.c_int * 2)(1, 9)
    P = lambda t, o=0: t.data_ptr() + o * t.element_size()   # noqa: E731
    sel_out = [P(f32), P(f32, n), P(i32), P(i32, n), P(u8), P(f32, 2 * n), P(f32, 4 * n), P(f32, 6 * n), P(f32, 7 * n), P(i32, 2 * n), P(i32, 3 * n)]
    for R, K_in, tf, kk in ((4097, 1, Tf, ks), (1, 4097, Tf, ks), (1, 70, 201, ks), (1, 70, Tf, (ctypes.c_int * 2)(9, 9))):
        rc = L.sttode_large_select(P(pred), P(gt), n, R, K_in, tf, 1.0, 1.0, ctypes.cast(kk, ctypes.c_void_p), 2, P(sp), 2, P(ws), ws.numel(),
                                   *sel_out, None)
        assert rc != 0 and b'sttode_large_select' in L.sttode_last_error()
    rc = L.sttode_large_select(P(pred), P(gt), n, 1, 70, Tf, 1.0, 1.0, ctypes.cast(ks, ctypes.c_void_p), 2, P(sp), 2, P(ws), 2 * n * 70 * 4 - 1,
                               *sel_out, None)
    assert rc != 0 and b'workspace' in L.sttode_last_error()
    for R, K_in, tf in ((1, 2, Tf), (4097, 1, Tf), (1, 70, 0)):
        assert L.sttode_large_kde_nll(P(pred), P(gt), n, R, K_in, tf, 1.0, P(f64), None) != 0 and b'sttode_large_kde_nll' in L.sttode_last_error()
    spr_out = [P(f64, q * n) for q in range(6)]
    for R, K_in, tf, div, wsb in ((1, 1, Tf, 1.0, ws.numel()), (2, 2049, Tf, 1.0, ws.numel()), (1, 70, Tf, 0.0, ws.numel()), (1, 70, Tf, 1.0, 8)):
        assert L.sttode_large_spread(P(pred), P(gt), n, R, K_in, tf, 1.0, div, P(ws), wsb, *spr_out, None) != 0
        assert b'sttode_large_spread' in L.sttode_last_error()
    torch.cuda.synchronize()
    assert (f32 == -7.0).all() and (i32 == -7).all() and (f64 == -7.0).all() and (u8 == 9).all() and (ws == 5).all()


def test_non_finite_inputs_keep_every_index_in_range():
    from sttode_amd import metrics
    rng = np.random.default_rng(11)
    n, M, Tf = 9, 130, 5
    x = rng.normal(0, 1, (n, M, Tf, 2)).astype(np.float32)
    x[rng.random((n, M, Tf, 2)) < 0.3] = np.nan
    x[rng.random((n, M, Tf, 2)) < 0.1] = np.inf
    x[rng.random((n, M, Tf, 2)) < 0.1] = -np.inf
    x[4] = np.nan
    x[5] = np.inf
    gt = rng.normal(0, 1, (n, Tf, 2)).astype(np.float32)
    gt[7, 2, 0] = np.nan
    sp = np.array([0, 2, 2, 5, 6, 9], np.int32)
    got = _sel_np(metrics.large_select(_dev(x), _dev(gt), ks=(1, 64, 65, 130), seg_ptr=sp))
    for k in ('best_ade_idx', 'best_fde_idx'):
        assert ((got[k] >= 0) & (got[k] < M)).all(), k
    for k in ('seg_jade_idx', 'seg_jfde_idx'):
        assert got[k][1] == -1 and ((np.delete(got[k], 1) >= 0) & (np.delete(got[k], 1) < M)).all(), k
    for k in ('ade', 'fde', 'ade_at', 'fde_at'):
        assert not np.isnan(got[k]).any(), k                                   # a NaN never wins
    assert got['ade'][4] == np.inf and got['best_ade_idx'][4] == 0 and got['ade'][5] == np.inf and got['best_fde_idx'][5] == 0
    assert got['ade'][7] == np.inf and got['seg_jade'][4] == np.inf and np.isnan(got['seg_jade'][1])
    kd = metrics.large_kde_nll(_dev(x), _dev(gt)).cpu().numpy()
    assert np.isnan(kd[4]) and np.isnan(kd[5])
    metrics.large_spread(_dev(x), _dev(gt))
    torch.cuda.synchronize()


# ----- the loops -----------------------------------------------------------------------------------------------------------------------

def test_score_samples_and_inference_reduced_samples_against_direct_calls():
    from sttode_amd import metrics, scenes
    m = _model('eth')
    sb = scenes.make_scene_batch(range(5400, 5412), 'eth')
    m.set_scene_batch(sb.past, sb.future, sb.scene_ptr)
    n, Ks, rounds = sb.n_agents, m.args.sample_k, 4
    z = torch.from_numpy(scenes.latents(61, n * rounds).reshape(rounds, n * Ks, -1)).to(m.device)
    red, samples = m.inference_reduced_samples(rounds, z=z)
    assert tuple(samples.shape) == (rounds, n, Ks, 12, 2) and samples is m.reduced_samples and red is m.reduction
    again = metrics.reduce_samples(samples, Ks)
    torch.cuda.synchronize()
    _bits(_np(again.centroids), _np(red.centroids), 'the returned buffer is what was reduced')
    sc = m.score_samples(samples, scale=1.3, miss_threshold=0.4, ks=(1, Ks, 65), kde=True, spread=True, div_scale=3.0)
    gt = torch.from_numpy(sb.future).to(m.device)
    ls = metrics.large_select(samples, gt, scale=1.3, miss_threshold=0.4, ks=(1, Ks, 65), seg_ptr=sb.scene_ptr)
    _same(_sel_np(sc.select), _sel_np(ls), 'score_samples: selection')
    _bits(_np(sc.kde_nll), _np(metrics.large_kde_nll(samples, gt, scale=1.3)), 'score_samples: kde')
    _same(_spr_np(sc.spread), _spr_np(metrics.large_spread(samples, gt, scale=1.3, div_scale=3.0)), 'score_samples: spread')
    plain = m.score_samples(samples, seg_ptr=False)
    assert plain.kde_nll is None and plain.spread is None and plain.select.seg_jade is None and plain.select.ade_at is None
    # best-of-M bounds best-of-K of the representatives' source set from below
    first = metrics.select(samples[0].contiguous(), gt)
    torch.cuda.synchronize()
    assert (_np(plain.select.ade) <= _np(first.ade)).all()


def test_eval_scenes_reduced_raw_against_a_hand_written_loop():
    from sttode_amd import metrics, scenes
    from sttode_amd.evaluate import eval_scenes_reduced, eval_scenes_reduced_raw
    m = _model('eth')
    ds = _dataset(range(5200, 5260), 'eth')
    n, Ks = int(ds.obs_traj.shape[0]), m.args.sample_k
    rounds, per_call, thr, scale, div = 4, 25, 0.6, 1.3, 2.0
    zall = scenes.latents(75, n * rounds)
    kw = dict(K=7, iters=4, traj_scale=scale, scenes_per_call=per_call, pipelined=False, miss_threshold=thr, spread=True, div_scale=div, ks=(1, 5, 70),
              joint=True, kde=True)
    rep = eval_scenes_reduced_raw(m, ds, rounds, z_fn=_z_fn(zall), **kw)
    base = eval_scenes_reduced(m, ds, rounds, z_fn=_z_fn(zall), **kw)
    for f in dataclasses.fields(rep):                                     # every field that existed: the bits of the loop without the raw pass
        u, v = getattr(rep, f.name), getattr(base, f.name)
        if f.name.startswith('raw_'):
            assert v is None and u is not None, f.name
        elif isinstance(u, np.ndarray):
            assert u.dtype == v.dtype and u.tobytes() == v.tobytes(), f.name
        else:
            assert u == v or (u != u and v != v), f.name
    z_fn = _z_fn(zall)
    sel, at_a, at_f, joint, kde, spr, miss = [], [], [], [], [], [], 0
    ks = [1, 5, Ks, 70]
    for s0 in range(0, len(ds), per_call):
        sb = ds.scene_batch(range(s0, min(s0 + per_call, len(ds))))
        m.set_scene_batch(sb.past, sb.future, sb.scene_ptr)
        stack = torch.stack([m.inference(None, z=z_fn(sb.n_agents * Ks)).permute(1, 0, 2, 3).contiguous() for _ in range(rounds)])
        gt = torch.from_numpy(sb.future).to(m.device)
        ls = metrics.large_select(stack, gt, scale=scale, miss_threshold=thr, ks=ks, seg_ptr=sb.scene_ptr)
        sp = metrics.large_spread(stack, gt, scale=scale, div_scale=div)
        kde.append(_np(metrics.large_kde_nll(stack, gt, scale=scale)))
        sel.append(np.stack([_np(ls.ade), _np(ls.fde)], axis=1).astype(np.float64))
        at_a.append(_np(ls.ade_at).astype(np.float64))
        at_f.append(_np(ls.fde_at).astype(np.float64))
        joint.append(np.stack([_np(ls.seg_jade), _np(ls.seg_jfde)], axis=1).astype(np.float64))
        spr.append(np.stack([_np(t) for t in (sp.apd, sp.fpd, sp.pade, sp.dlow, sp.es_ade, sp.es_fde)], axis=1))
        miss += int(_np(ls.miss).sum())
    sel, at_a, at_f, joint, kde, spr = (np.concatenate(v) for v in (sel, at_a, at_f, joint, kde, spr))
    assert rep.raw_m == rounds * Ks == 80 and rep.n_agents == n
    assert (rep.raw_ade, rep.raw_fde) == tuple(float(v) for v in sel.sum(axis=0) / n) and rep.raw_miss_rate == miss / n
    assert rep.raw_ade_at_k == {k: float(at_a[:, i].sum() / n) for i, k in enumerate(ks)}
    assert rep.raw_fde_at_k == {k: float(at_f[:, i].sum() / n) for i, k in enumerate(ks)}
    assert (rep.raw_joint_ade, rep.raw_joint_fde) == tuple(float(v) for v in joint.mean(axis=0))
    ok = np.isfinite(kde)
    assert rep.raw_kde_invalid == int((~ok).sum()) and rep.raw_kde_nll == float(kde[ok].mean())
    assert (rep.raw_apd, rep.raw_fpd, rep.raw_pade, rep.raw_dlow, rep.raw_energy_ade, rep.raw_energy_fde) == tuple(
        float(v) for v in spr.sum(axis=0) / n)
    # what the numbers are for: the raw set bounds its own prefix and the representatives cut from it
    assert rep.raw_ade <= rep.raw_ade_at_k[Ks] and rep.raw_ade <= rep.ade and rep.raw_ade_at_k[70] <= rep.raw_ade_at_k[5]
    # the pipelined form fills the same fields
    rep_p = eval_scenes_reduced_raw(m, ds, rounds, z_fn=_z_fn(zall), **{**kw, 'pipelined': True})
    assert rep_p.raw_m == 80 and np.isfinite([rep_p.raw_ade, rep_p.raw_joint_ade, rep_p.raw_apd]).all()
