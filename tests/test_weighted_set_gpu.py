"""GPU tests of the weighted sample set: sttode_weighted_set against tests/golden/weighted_set.npz and the loop restatement
of tests/weighted_ref.py, the identities at equal weights against the device's own sample_spread / kde_nll / selection, the invariances
(power-of-two multiples of the weights, NaN coordinates at zero weight, joint permutations, the rest of the batch, repeats), refusals that
leave their outputs untouched, and eval_scenes_reduced(weighted=True) against a hand-written composition.

Tolerances.  float64 outputs: |got - ref| <= 1e-10 * (sum of the magnitudes of the terms combined) against the restatement -- the worst-case
N u bound of N <= 2016 * 200 float64 additions is 4.5e-11 (tests/test_sample_spread_gpu.py's bound); for the energy scores that sum is A + B
of the difference A - B, else the value itself.  kde_nll: 1e-9 absolute against the restatement, 1e-8 against the stored scipy values
(tests/test_scene_metrics_gpu.py's bounds).  ade_top / fde_top: bit for bit against the float32 restatement of bok_dist, and within
bok_dist's rounding of the stored float64 rows.  Measured on an MI355X (worst over all cases): es_ade 9.0e-17, es_fde 6.9e-17, apd 1.1e-14,
fpd 1.1e-14, brier_* 2.1e-16, neff 4.6e-16, eade / efde 0; kde_nll 1.7e-14 against the restatement, 7.7e-14 against scipy; no float32
value differs in any bit."""
import dataclasses

import numpy as np
import pytest
import torch

from test_selection_gpu import _dataset, _gpu, _model, _z_fn
from test_weighted_set import bad_rows, cases, close, f32_bound, magnitude, restated
from weighted_ref import F64

pytestmark = pytest.mark.gpu

OUTS = F64 + ('ade_top', 'fde_top')
NEW_FIELDS = ('w_kde_nll', 'w_kde_invalid', 'w_es_ade', 'w_es_fde', 'w_apd', 'w_fpd', 'eade', 'efde', 'brier_ade', 'brier_fde', 'ade_top_k',
              'fde_top_k', 'mean_neff', 'weighted_agents')


def _dev(g, tag, dev):
    return (torch.from_numpy(g[tag + '/pred']).to(dev), torch.from_numpy(g[tag + '/weights']).to(dev), torch.from_numpy(g[tag + '/gt']).to(dev),
            float(g[tag + '/scale']))


def _eq(x, y):
    return torch.equal(torch.isnan(x), torch.isnan(y)) and torch.equal(torch.nan_to_num(x, nan=0.0), torch.nan_to_num(y, nan=0.0))


def _same(a, b, what, rows=None, rows_b=None, outs=OUTS):
    for f in outs:
        x, y = getattr(a, f), getattr(b, f)
        x, y = (x if rows is None else x[rows]), (y if rows_b is None else y[rows_b])
        assert _eq(x, y), (what, f)


def test_kernel_against_the_fixture_and_the_restatement(golden):
    from sttode_amd import metrics
    dev = _gpu()
    worst = {k: 0.0 for k in F64 + ('kde_scipy',)}
    bits = {'ade_top': 0, 'fde_top': 0}
    failures = []
    for tag, pred_np, w_np, gt_np, scale, g in cases(golden):
        n, K, Tf = pred_np.shape[:3]
        pred, w, gt, _ = _dev(g, tag, dev)
        ws = metrics.weighted_set(pred, w, gt, scale=scale)
        torch.cuda.synchronize()
        ref = restated(golden, tag)
        for k in F64:
            v = getattr(ws, k)
            assert v.dtype == torch.float64 and v.shape == (n,)
            got = v.cpu().numpy()
            try:
                if k == 'kde_nll':
                    assert np.array_equal(np.isnan(got), np.isnan(ref[k])), f'{tag} kde_nll NaN pattern'
                    ok = ~np.isnan(got)
                    e1 = float(np.abs(got[ok] - ref[k][ok]).max()) if ok.any() else 0.0
                    e2 = float(np.abs(got[ok] - g[tag + '/kde_nll'][ok]).max()) if ok.any() else 0.0
                    worst[k], worst['kde_scipy'] = max(worst[k], e1), max(worst['kde_scipy'], e2)
                    assert e1 <= 1e-9 and e2 <= 1e-8, f'{tag} kde_nll: {e1:.2e} against the restatement, {e2:.2e} against scipy'
                else:
                    worst[k] = max(worst[k], close(got, ref[k], magnitude(ref, k), f'{tag} {k}'))
            except AssertionError as e:
                failures.append(str(e))
        assert np.array_equal(np.isnan(ws.eade.cpu().numpy()), bad_rows(w_np)), tag              # NaN exactly on the bad rows
        for k in ('ade_top', 'fde_top'):
            v, want = getattr(ws, k).cpu().numpy(), g[tag + '/' + k]
            assert v.dtype == np.float32 and v.shape == (n, K)
            diff = int(((v.view(np.uint32) != ref[k].view(np.uint32)) & ~(np.isnan(v) & np.isnan(ref[k]))).sum())
            bits[k] += diff
            if diff:
                failures.append(f'{tag} {k}: {diff} of {v.size} values differ in bits from the float32 restatement')
            if not np.array_equal(np.isnan(v), np.isnan(want)):
                failures.append(f'{tag} {k}: NaN pattern')
            fin = ~np.isnan(want)
            if not (np.abs(v[fin] - want[fin]) <= f32_bound(pred_np, gt_np, scale, want[fin])).all():
                failures.append(f'{tag} {k}: outside the float32 bound of the stored float64 rows')
        k5 = min(5, K)
        a5, f5 = ws.at(k5)
        assert torch.equal(a5, ws.ade_top[:, k5 - 1]) and torch.equal(f5, ws.fde_top[:, k5 - 1])
        with pytest.raises(ValueError):
            ws.at(K + 1)
    print('worst |got - ref| / magnitude per output (kde_nll, kde_scipy: absolute):', {k: '%.2e' % v for k, v in worst.items()})
    print('float32 rows, values whose bits differ from the restatement:', bits)
    assert not failures, failures


def test_uniform_weights_are_the_unweighted_passes(golden):
    from sttode_amd import metrics
    dev = _gpu()
    g = golden('weighted_set')
    for tag in map(str, g['cases']):
        pred, _, gt, scale = _dev(g, tag, dev)
        n, K, Tf = pred.shape[:3]
        ws = metrics.weighted_set(pred, torch.full((n, K), 3.0, device=dev), gt, scale=scale)
        sel = metrics.select(pred, gt, scale=scale)
        assert torch.equal(ws.ade_top[:, K - 1], sel.ade) and torch.equal(ws.fde_top[:, K - 1], sel.fde), tag
        np.testing.assert_allclose(ws.neff.cpu().numpy(), K, rtol=1e-14)
        if K < 2:
            continue
        ss = metrics.sample_spread(pred, gt, scale=scale)
        nll = metrics.kde_nll(pred, gt, scale=scale)
        torch.cuda.synchronize()
        assert torch.equal(ws.ade_top, ss.ade_at_k) and torch.equal(ws.fde_top, ss.fde_at_k), tag
        got = {k: getattr(ws, k).cpu().numpy() for k in F64}
        es_mag = {'es_ade': got['eade'] + (got['eade'] - got['es_ade']), 'es_fde': got['efde'] + (got['efde'] - got['es_fde'])}
        for k in ('apd', 'fpd', 'es_ade', 'es_fde'):
            want = getattr(ss, k).cpu().numpy()
            close(got[k], want, es_mag.get(k, want), f'{tag} {k}')
        want = nll.cpu().numpy()
        assert np.array_equal(np.isnan(got['kde_nll']), np.isnan(want)), tag
        ok = ~np.isnan(want)
        assert (np.abs(got['kde_nll'][ok] - want[ok]) <= 1e-9).all(), (tag, float(np.abs(got['kde_nll'][ok] - want[ok]).max()))


def test_power_of_two_multiples_of_the_weights_give_equal_bits(golden):
    from sttode_amd import metrics
    dev = _gpu()
    g = golden('weighted_set')
    for tag in ('counts_k20_t12', 'ties_k23_t33', 'special_k24_t33', 'counts_k64_t40', 'k1_t12'):
        pred, w, gt, scale = _dev(g, tag, dev)
        first = metrics.weighted_set(pred, w, gt, scale=scale)
        for f in (2.0 ** 5, 2.0 ** -7):
            _same(metrics.weighted_set(pred, w * f, gt, scale=scale), first, (tag, f))
        _same(metrics.weighted_set(pred, w, gt, scale=scale), first, (tag, 'a second run'))   # two runs give equal bits


def test_zero_weight_samples_are_never_read(golden):
    from sttode_amd import metrics
    dev = _gpu()
    g = golden('weighted_set')
    for tag in ('counts_k20_t12', 'special_k6_t12', 'special_k24_t33', 'counts_k64_t40'):
        pred, w, gt, scale = _dev(g, tag, dev)
        assert bool((w == 0).any())
        poisoned = pred.clone()
        poisoned[w == 0] = float('nan')
        _same(metrics.weighted_set(poisoned, w, gt, scale=scale), metrics.weighted_set(pred, w, gt, scale=scale), tag)


def test_joint_permutation_of_samples_and_weights(golden):
    from sttode_amd import metrics
    dev = _gpu()
    g = golden('weighted_set')
    rng = np.random.default_rng(5)
    for tag in ('one_k20_t12', 'counts_k24_t12', 'counts_k64_t40'):
        pred, _, gt, scale = _dev(g, tag, dev)
        n, K, Tf = pred.shape[:3]
        keep = ~torch.from_numpy(g[tag + '/degenerate'].any(axis=1)).to(dev)
        pred, gt = pred[keep].contiguous(), gt[keep].contiguous()
        n = pred.shape[0]
        w = torch.from_numpy(np.stack([rng.permutation(K) for _ in range(n)]).astype(np.float32)).to(dev)   # distinct, one of them zero
        perm = torch.from_numpy(rng.permutation(K)).to(dev)
        a = metrics.weighted_set(pred, w, gt, scale=scale)
        b = metrics.weighted_set(pred[:, perm].contiguous(), w[:, perm].contiguous(), gt, scale=scale)
        torch.cuda.synchronize()
        _same(a, b, tag, outs=('ade_top', 'fde_top', 'brier_ade', 'brier_fde'))
        x = {k: getattr(a, k).cpu().numpy() for k in F64}
        y = {k: getattr(b, k).cpu().numpy() for k in F64}
        x['es_ade_mag'], x['es_fde_mag'] = 2 * x['eade'] - x['es_ade'], 2 * x['efde'] - x['es_fde']
        for k in F64:
            if k == 'kde_nll':
                assert np.isfinite(x[k]).all() and (np.abs(x[k] - y[k]) <= 1e-9).all(), (tag, k)
            else:
                close(y[k], x[k], magnitude(x, k), f'{tag} {k}')


def test_an_agent_does_not_depend_on_the_rest_of_the_batch(golden):
    from sttode_amd import metrics
    dev = _gpu()
    g = golden('weighted_set')
    for tag, other in (('special_k6_t12', 'dominant_k6_t12'), ('counts_k20_t12', 'dup_k20_t12')):
        pred, w, gt, scale = _dev(g, tag, dev)
        po, wo, go, _ = _dev(g, other, dev)
        n = pred.shape[0]
        alone = metrics.weighted_set(pred, w, gt, scale=scale)
        behind = metrics.weighted_set(torch.cat([pred, po]), torch.cat([w, wo]), torch.cat([gt, go]), scale=scale)
        _same(behind, alone, (tag, 'agents appended behind'), rows=slice(0, n))
        for front in (1, 2, 3):
            b = metrics.weighted_set(torch.cat([po[:front], pred]), torch.cat([wo[:front], w]), torch.cat([go[:front], gt]), scale=scale)
            _same(b, alone, (tag, front, 'agents in front'), rows=slice(front, front + n))


def test_refused_calls_leave_their_outputs_untouched():
    from sttode_amd import capi, metrics
    dev = _gpu()
    n, K, Tf = 4, 20, 12
    pred, w, gt = torch.zeros(n, K, Tf, 2, device=dev), torch.ones(n, K, device=dev), torch.zeros(n, Tf, 2, device=dev)
    d = [torch.full((n,), -7.0, dtype=torch.float64, device=dev) for _ in range(10)]
    f = [torch.full((n, 64), -7.0, device=dev) for _ in range(2)]
    o = d + f
    for what, args in (('1 <= K <= 64', (pred, w, gt, n, 65, Tf, 1.0, *o)), ('1 <= K <= 64', (pred, w, gt, n, 0, Tf, 1.0, *o)),
                       ('n and Tf', (pred, w, gt, 0, K, Tf, 1.0, *o)), ('n and Tf', (pred, w, gt, n, K, 0, 1.0, *o)),
                       ('null pointer', (pred, None, gt, n, K, Tf, 1.0, *o)), ('null pointer', (None, w, gt, n, K, Tf, 1.0, *o)),
                       ('null pointer', (pred, w, None, n, K, Tf, 1.0, *o)),
                       ('null pointer', (pred, w, gt, n, K, Tf, 1.0, *o[:9], None, *o[10:])),
                       ('null pointer', (pred, w, gt, n, K, Tf, 1.0, None, *o[1:]))):
        with pytest.raises(capi.SttodeError, match='sttode_weighted_set.*' + what):
            capi.call('sttode_weighted_set', *args, capi.stream_ptr())
    torch.cuda.synchronize()
    assert all(bool((t == -7.0).all()) for t in o)
    # the optional outputs may be NULL: the required ones keep their bits
    full = metrics.weighted_set(pred + 1.0, w, gt)
    capi.call('sttode_weighted_set', pred + 1.0, w, gt, n, K, Tf, 1.0, *d[:6], None, None, None, d[9], None, None, capi.stream_ptr())
    torch.cuda.synchronize()
    for t, k in zip(d[:6] + [d[9]], F64[:6] + ('neff',)):
        assert _eq(t, getattr(full, k)), k
    assert all(bool((t == -7.0).all()) for t in d[6:9] + f)
    # the Python layer
    with pytest.raises(ValueError, match='1 <= K <= 64'):
        metrics.weighted_set(torch.zeros(n, 65, Tf, 2, device=dev), torch.ones(n, 65, device=dev), gt)
    with pytest.raises(ValueError, match='weights must be'):
        metrics.weighted_set(pred, w[:, :-1], gt)                      # weights of the wrong shape
    with pytest.raises(ValueError, match='float32'):
        metrics.weighted_set(pred, w.to(torch.int32), gt)              # Reduction.counts without .float()
    with pytest.raises(capi.SttodeError, match='HIP device only'):
        metrics.weighted_set(pred, w.cpu(), gt)
    with pytest.raises(ValueError, match='gt must be'):
        metrics.weighted_set(pred, w, gt[:, :-1])
    with pytest.raises(ValueError, match='pred_nk must be'):
        metrics.weighted_set(pred[..., :1], w, gt)


def test_eval_scenes_reduced_weighted_against_a_hand_written_composition(monkeypatch):
    from sttode_amd import capi, metrics, scenes
    from sttode_amd.evaluate import eval_scenes_reduced
    m = _model('eth')
    ds = _dataset(range(5200, 5230), 'eth')
    n, Ks = int(ds.obs_traj.shape[0]), m.args.sample_k
    rounds, K, per_call, ks = 2, 10, 16, (1, 5, 10, 20)
    zall = scenes.latents(83, n * rounds)
    kw = dict(K=K, iters=5, traj_scale=1.3, scenes_per_call=per_call, pipelined=False, ks=ks)
    eval_scenes_reduced(m, ds, rounds, z_fn=_z_fn(zall), **kw)        # (the model's one-time calls -- workspaces of these shapes -- are made here)
    calls = []
    real = capi.call
    monkeypatch.setattr(capi, 'call', lambda name, *a, **k: (calls.append(name), real(name, *a, **k))[1])
    off = eval_scenes_reduced(m, ds, rounds, z_fn=_z_fn(zall), **kw)
    calls_off, calls[:] = list(calls), []
    on = eval_scenes_reduced(m, ds, rounds, z_fn=_z_fn(zall), weighted=True, **kw)
    calls_on = list(calls)
    monkeypatch.undo()
    # weighted=False: the calls it made before (none of the new entry), and every old field of the two reports is the same
    assert 'sttode_weighted_set' not in calls_off and calls_on.count('sttode_weighted_set') == -(-len(ds) // per_call)
    assert [c for c in calls_on if c != 'sttode_weighted_set'] == calls_off
    for f in dataclasses.fields(off):
        u, v = getattr(off, f.name), getattr(on, f.name)
        if f.name in NEW_FIELDS:
            assert u is None and v is not None, f.name
        elif isinstance(u, np.ndarray):
            assert u.dtype == v.dtype and u.tobytes() == v.tobytes(), f.name
        else:
            assert u == v or (u is None and v is None), f.name
    # weighted=True: reduce_samples -> metrics.weighted_set -> means
    z_fn, rows, tops = _z_fn(zall), [], []
    for s0 in range(0, len(ds), per_call):
        sb = ds.scene_batch(range(s0, min(s0 + per_call, len(ds))))
        m.set_scene_batch(sb.past, sb.future, sb.scene_ptr)
        stack = torch.stack([m.inference(None, z=z_fn(sb.n_agents * Ks)).permute(1, 0, 2, 3).contiguous() for _ in range(rounds)])
        red = metrics.reduce_samples(stack, K, iters=5)
        assert _eq(red.weights, red.counts.float() / (rounds * Ks))
        ws = metrics.weighted_set(red.centroids, red.weights, m._future, scale=1.3)
        rows.append(torch.stack([getattr(ws, k) for k in F64], dim=1).cpu().numpy())
        tops.append((ws.ade_top.cpu().numpy(), ws.fde_top.cpu().numpy()))
    v = np.concatenate(rows)
    assert on.weighted_agents.shape == (n, 10) and on.weighted_agents.tobytes() == v.tobytes()

    def mean(x):
        x = x.astype(np.float64)
        return float(x[np.isfinite(x)].mean())
    for i, name in enumerate(('eade', 'efde', 'w_es_ade', 'w_es_fde', 'w_apd', 'w_fpd', 'w_kde_nll', 'brier_ade', 'brier_fde', 'mean_neff')):
        assert getattr(on, name) == mean(v[:, i]), name
    assert on.w_kde_invalid == int((~np.isfinite(v[:, 6])).sum())
    assert sorted(on.ade_top_k) == sorted(on.fde_top_k) == [1, 5, 10]
    for k in (1, 5, 10):
        assert on.ade_top_k[k] == mean(np.concatenate([t[0][:, k - 1] for t in tops]))
        assert on.fde_top_k[k] == mean(np.concatenate([t[1][:, k - 1] for t in tops]))
    # the last column is the minimum over the non-empty clusters: never below the selection over all K centroids
    assert on.ade_top_k[10] >= on.ade * (1 - 1e-6) and on.ade_top_k[1] >= on.ade_top_k[5] >= on.ade_top_k[10] and 1.0 <= on.mean_neff <= K
    assert on.eade >= on.ade_top_k[10] and on.brier_ade >= on.ade_top_k[10]
