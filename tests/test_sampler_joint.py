"""CPU tests of the scene-level forms of the stage-2 sampler's terms: the restatement tests/sampler_joint_ref.py against
NumPy loops, np.argmin and central differences; the fixture against the restatement; the properties that tie the joint terms to the
marginal ones; the three entry points in header, ctypes table and library; every refusal by name before anything is launched; and the
defaults, which leave compute_sampler_loss what it was."""
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch

import sampler_joint_ref as JR
import sampler_objective_ref as SR
from test_capi_symbols import header_functions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WS, FWD, BWD = 'sttode_sampler_objective_joint_ws', 'sttode_sampler_objective_joint', 'sttode_sampler_objective_joint_bwd'


def _loops(motion, gt, w, sp, scale):
    """div, rec, best, es per segment and J [S,K] by plain double loops over float64 arrays."""
    n, K, Tf, _ = motion.shape
    S = len(sp) - 1
    div, rec, best, es, Js = np.zeros(S), np.zeros(S), np.zeros(S, int), np.zeros(S), np.zeros((S, K))
    for g in range(S):
        ag = range(sp[g], sp[g + 1])
        ng = len(ag)
        acc, pairs, rp = 0.0, 0, 0.0
        for i in range(K):
            for j in range(i + 1, K):
                d2 = sum(((motion[a, i] - motion[a, j]) ** 2).sum() for a in ag) / ng
                acc += np.exp(-d2 / scale)
                pairs += 1
                rp += np.sqrt(sum(((w[a][:, None] * (motion[a, i] - motion[a, j])) ** 2).sum() for a in ag) / (ng * Tf))
        div[g] = acc / pairs
        for k in range(K):
            Js[g, k] = sum(((w[a][:, None] * (motion[a, k] - gt[a])) ** 2).sum() for a in ag)
        best[g] = np.argmin(Js[g])
        rec[g] = Js[g, best[g]]
        es[g] = np.sqrt(Js[g] / (ng * Tf)).sum() / K - rp / K ** 2
    return div, rec, best, es, Js


def _small(seed=3, segs=(1, 2, 3), K=4, nz=3, Tf=3, masked=True):
    rng = np.random.default_rng(seed)
    n = sum(segs)
    f = lambda *s: torch.from_numpy(rng.standard_normal(s))
    mask = torch.from_numpy((rng.random((n, Tf)) < 0.7).astype(np.float64)) if masked else None
    return [f(n * K, nz), 0.5 * f(n * K, nz), 0.5 * f(n * K, nz), 0.5 * f(n * K, nz), f(n, K, Tf, 2), f(n, Tf, 2), mask, JR.seg_ptr_of(segs)]


def test_restatement_vs_numpy_loops_and_central_differences():
    a = _small()
    mo, gt, mask, sp = a[4], a[5], a[6], a[7]
    S = len(sp) - 1
    g = {k: torch.from_numpy(np.random.default_rng(5).standard_normal(S)) for k in ('div', 'rec', 'es')}
    r = JR.objective(*a, 1.5, g=g)
    div, rec, best, es, Js = _loops(mo.numpy(), gt.numpy(), mask.numpy(), sp, 1.5)
    for k, v in (('div', div), ('rec', rec), ('es', es), ('J', Js)):
        np.testing.assert_allclose(r[k].numpy(), v, rtol=1e-12, atol=1e-14, err_msg=k)
    assert np.array_equal(r['best'].numpy(), best)

    def total(x):
        d, rc, _, e, _ = _loops(x, gt.numpy(), mask.numpy(), sp, 1.5)
        return float((d * g['div'].numpy()).sum() + (rc * g['rec'].numpy()).sum() + (e * g['es'].numpy()).sum())
    x0 = mo.numpy().copy()
    rng = np.random.default_rng(9)
    h = 1e-6
    for _ in range(24):                                                                     # central differences at random coordinates
        idx = tuple(int(rng.integers(s)) for s in x0.shape)
        xp, xm = x0.copy(), x0.copy()
        xp[idx] += h
        xm[idx] -= h
        fd = (total(xp) - total(xm)) / (2 * h)
        assert abs(fd - float(r['dmotion'][idx])) <= 1e-6 * max(1.0, abs(fd)), (idx, fd, float(r['dmotion'][idx]))
    # the kld half is the marginal restatement's
    m = SR.objective(*a[:6], mask, 1.5, g={'kld': torch.ones(mo.shape[0], dtype=torch.float64)})
    j = JR.objective(*a, 1.5, g={'kld': torch.ones(mo.shape[0], dtype=torch.float64)})
    for k in ('kld', 'dmu', 'dlogvar'):
        assert torch.equal(m[k], j[k]), k
    assert (j['dmotion'] == 0).all()
    # an empty segment: NaN values, index 0, the others untouched
    sp2 = np.array([0, 1, 1, 3, 6], np.int32)
    e = JR.objective(*a[:7], sp2, 1.5)
    assert all(np.isnan(float(e[k][1])) for k in ('div', 'rec', 'es')) and int(e['best'][1]) == 0
    assert torch.equal(e['div'][[0, 2, 3]], r['div']) and torch.equal(e['es'][[0, 2, 3]], r['es'])


def test_fixture_vs_restatement_and_input_conditions():
    z = np.load(os.path.join(ROOT, 'tests', 'golden', 'sampler_joint.npz'))
    assert list(z['cases']) == [JR.tag(s, m) for s in JR.SHAPES for m in JR.GOLDEN_MASKS[s]]
    for si, shape in enumerate(JR.SHAPES):
        segs = JR.GOLDEN_SEGS[shape]
        for mk in JR.GOLDEN_MASKS[shape]:
            t = JR.tag(shape, mk)
            inp = JR.draw(int(z[t + '/seed']), shape, segs, mk)
            assert np.array_equal(inp['motion'], z[t + '/motion']) and np.array_equal(inp['gt'], z[t + '/gt']), t
            assert np.array_equal(inp['seg_ptr'], z[t + '/seg_ptr']) and (mk == 'none' or np.array_equal(inp['mask'], z[t + '/mask'])), t
            inp.update(motion=z[t + '/motion'], gt=z[t + '/gt'], mask=z[t + '/mask'] if mk == 'ragged' else None)
            g = {k: torch.from_numpy(z[t + '/g_' + k]) for k in ('div', 'rec', 'es')}
            r = JR.objective(*JR.as_torch(inp, torch.float64), 2.0, g=g)
            for k in ('div', 'rec', 'es', 'J', 'dmotion'):
                np.testing.assert_allclose(r[k].numpy(), z[t + '/' + k], rtol=1e-12, atol=1e-15, err_msg=f'{t} {k}')
            assert np.array_equal(r['best'].numpy(), z[t + '/best'])
            assert JR.conditions(inp, shape, segs, r) is None, (t, JR.conditions(inp, shape, segs, r))
            tie, eq = JR.roles(segs, shape[0])
            sp = inp['seg_ptr']
            if tie is not None:
                assert r['best'][tie] == 1 and np.array_equal(inp['motion'][sp[tie]:sp[tie + 1], 1], inp['motion'][sp[tie]:sp[tie + 1], -1])
            assert r['best'][eq] == 0 and r['rec'][eq] == 0
            if mk == 'ragged':
                m = inp['mask']
                free = [i for i, c in enumerate(segs) if c > 1 and i not in (tie, eq)][0]
                assert set(np.unique(m)) <= {0.0, 1.0} and not m[sp[free]].any() and not m[sp[free]:sp[free + 1], -1].any()
    assert os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'sampler_joint.npz')) <= os.path.getsize(
        os.path.join(ROOT, 'tests', 'golden', 'sampler_objective.npz'))


def test_properties_of_the_joint_terms():
    a = _small(seed=11, segs=(2, 3, 1), K=5, Tf=4)
    mu, lv, pmu, plv, mo, gt, mask, sp = a
    n, K, Tf = mo.shape[:3]
    marg = SR.objective(mu, lv, pmu, plv, mo, gt, mask, 2.0)
    # one-agent segments: the marginal div and rec (and best)
    one = JR.objective(mu, lv, pmu, plv, mo, gt, mask, np.arange(n + 1), 2.0)
    np.testing.assert_allclose(one['div'].numpy(), marg['div'].numpy(), rtol=1e-13)
    np.testing.assert_allclose(one['rec'].numpy(), marg['rec'].numpy(), rtol=1e-13)
    assert torch.equal(one['best'], marg['best'])
    # sum_g rec_g / n >= mean_a rec_a, with equality when the agents' own minima coincide
    r = JR.objective(*a, 2.0)
    assert float(r['rec'].sum() / n) >= float(marg['rec'].mean())
    mo2 = mo.clone()
    mo2[:, 2] = gt + 1e-3 * (mo[:, 2] - gt)                                                 # sample 2 is every agent's own best
    r2, m2 = JR.objective(mu, lv, pmu, plv, mo2, gt, mask, sp, 2.0), SR.objective(mu, lv, pmu, plv, mo2, gt, mask, 2.0)
    assert (m2['best'] == 2).all() and (r2['best'] == 2).all()
    np.testing.assert_allclose(float(r2['rec'].sum() / n), float(m2['rec'].mean()), rtol=1e-13)
    # n_g = 1, Tf = 1: es_fde of the marginal restatement
    b = _small(seed=12, segs=(1, 1, 1), K=6, Tf=1)
    j1, s1 = JR.objective(*b, 2.0), SR.objective(*b[:7], 2.0)
    np.testing.assert_allclose(j1['es'].numpy(), s1['es_fde'].numpy(), rtol=1e-12)
    # ... and in general not es_ade
    assert not np.allclose(one['es'].numpy(), marg['es_ade'].numpy(), rtol=1e-3)
    # permuting the agents inside a segment leaves the values unchanged
    perm = np.array([1, 0, 4, 2, 3, 5])
    f = lambda t, per: t.reshape(n, -1)[perm].reshape(t.shape) if per else t
    pa = [mu.reshape(n, K, -1)[perm].reshape(mu.shape), lv.reshape(n, K, -1)[perm].reshape(lv.shape), pmu.reshape(n, K, -1)[perm].reshape(mu.shape),
          plv.reshape(n, K, -1)[perm].reshape(mu.shape), mo[perm], gt[perm], mask[perm], sp]
    rp = JR.objective(*pa, 2.0)
    for k in ('div', 'rec', 'es'):
        np.testing.assert_allclose(rp[k].numpy(), r[k].numpy(), rtol=1e-13, err_msg=k)
    assert torch.equal(rp['best'], r['best'])
    # the joint score sees dependence between agents: a sum-over-agents distance would make it the mean of the per-agent scores
    assert not np.allclose(r['es'][1].item(), one['es'][2:5].mean().item(), rtol=1e-3)


def test_three_exports_with_equal_arity_in_header_table_and_library():
    from sttode_amd import capi
    fns = header_functions()
    L = ctypes.CDLL(capi.LIB_PATH)
    for name, arity in ((WS, 3), (FWD, 22), (BWD, 24)):
        assert name in fns and name in capi.SIGNATURES, name
        assert len(fns[name]) == len(capi.SIGNATURES[name]) == arity, name
        assert hasattr(L, name), f'{name} is not exported'
    assert capi.RESTYPES[WS] is ctypes.c_longlong and capi.lib().sttode_sampler_objective_joint_ws.restype is ctypes.c_longlong
    src = open(os.path.join(ROOT, 'include', 'sttode_hip.h')).read()
    assert 'long long int ' + WS + '(' in src


def test_abi_version_stays_15():
    from sttode_amd import capi
    assert capi.ABI_VERSION == 15 and capi.lib().sttode_abi_version() == 15
    assert '#define STTODE_ABI_VERSION 15' in open(os.path.join(ROOT, 'include', 'sttode_hip.h')).read()


def test_workspace_query_values():
    """Per agent K float64 sums against the ground truth and np float64 + np float32 pair sums; per segment 2 np + K float64 table
    entries and one int32 index."""
    from sttode_amd import capi
    for n, K, S in ((1, 2, 1), (19, 20, 3), (8729, 20, 512), (3, 64, 3), (2 ** 20, 20, 2 ** 16)):
        npair = K * (K - 1) // 2
        want = n * (8 * K + 12 * npair) + S * (8 * (2 * npair + K) + 4)
        assert capi.sampler_joint_ws(n, K, S) == want, (n, K, S)
    L = capi.lib()
    for bad in ((0, 20, 1), (-1, 20, 1), (4, 1, 1), (4, 0, 1), (4, 20, 0), (4, 20, -3), (4, 2049, 1)):
        assert L.sttode_sampler_objective_joint_ws(*bad) < 0 and L.sttode_last_error().decode().startswith(WS + ':'), bad
        with pytest.raises(capi.SttodeError, match=WS):
            capi.sampler_joint_ws(*bad)


def _args(name, n=2, K=3, nz=4, D=8, S=1, scale=2.0, ws=64, ws_bytes=1 << 20, null=()):
    """Argument list of one entry point with non-null dummy addresses (nothing is dereferenced: every refusal comes before the launch)."""
    p = lambda k: None if k in null else 64
    head = [p('mu'), p('logvar'), None, None, p('motion'), p('gt'), None, p('seg_ptr'), S]
    if name == FWD:
        return head + [n, K, nz, D, scale, None if 'workspace' in null else ws, ws_bytes] + [p(k) for k in ('kld', 'div', 'rec', 'best', 'es')] + [None]
    return head + [None] * 4 + [n, K, nz, D, scale, None if 'workspace' in null else ws, ws_bytes] + [p(k) for k in ('dmu', 'dlogvar', 'dmotion')] + [None]


@pytest.mark.parametrize('name', (FWD, BWD))
def test_every_refusal_names_its_entry_point(name):
    """A NULL required pointer; K <= 1; K D > 4096; an odd D; scale <= 0; n, nz, S < 1; a misaligned or short workspace -- refused on the
    host, without a GPU."""
    from sttode_amd import capi
    L = capi.lib()
    outs = ('kld', 'div', 'rec', 'best', 'es') if name == FWD else ('dmu', 'dlogvar', 'dmotion')
    bad = [dict(null=(k,)) for k in ('mu', 'logvar', 'motion', 'gt', 'seg_ptr', 'workspace') + outs]
    bad += [dict(K=1), dict(K=0), dict(K=17, D=242), dict(K=2, D=2050), dict(D=7), dict(scale=0.0), dict(scale=-1.0), dict(n=0), dict(nz=0),
            dict(S=0), dict(S=-1), dict(ws=68), dict(ws_bytes=capi.sampler_joint_ws(2, 3, 1) - 1), dict(ws_bytes=0), dict(ws_bytes=-8)]
    for kw in bad:
        rc = getattr(L, name)(*_args(name, **kw))
        msg = L.sttode_last_error().decode()
        assert rc != 0 and msg.startswith(name + ':'), (kw, rc, msg)
        with pytest.raises(capi.SttodeError, match=name + ':'):
            capi.call(name, *_args(name, **kw))


def test_python_surface_and_refusals():
    from helpers import sampler_args
    from sttode_amd import capi, samplerloss
    from sttode_amd.dist import Normal
    from sttode_amd.trainer import train_sampler_epoch
    p = inspect.signature(samplerloss.compute_sampler_loss).parameters
    assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ('joint', 'seg_ptr')) and (p['joint'].default, p['seg_ptr'].default) == (False, None)
    p = inspect.signature(samplerloss.compute_sampler_loss_nba).parameters
    assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ('joint', 'seg_len')) and (p['joint'].default, p['seg_len'].default) == (False, None)
    assert inspect.signature(train_sampler_epoch).parameters['joint'].default is False
    assert list(inspect.signature(samplerloss.diversity_loss_joint).parameters)[:4] == ['infer_dec_motion', 'seg_ptr', 'weight', 'scale']
    assert list(inspect.signature(samplerloss.recon_loss_joint).parameters)[:5] == ['fut_motion_orig', 'infer_dec_motion', 'fut_mask', 'seg_ptr', 'weight']
    assert list(inspect.signature(samplerloss.energy_loss_joint).parameters)[:5] == ['fut_motion_orig', 'infer_dec_motion', 'fut_mask', 'seg_ptr', 'weight']
    n, K, Tf, nz = 6, 4, 5, 6
    mo, gt = torch.zeros(n, K, Tf, 2), torch.zeros(n, Tf, 2)
    q = Normal(mu=torch.zeros(n * K, nz), logvar=torch.zeros(n * K, nz))
    a, cfg = sampler_args(), {'weight': 1, 'scale': 1}
    # CPU tensors: no fallback
    for call in (lambda: samplerloss.diversity_loss_joint(mo, [0, 2, 6], 1.0, 2.0), lambda: samplerloss.recon_loss_joint(gt, mo, None, [0, 6], 1.0),
                 lambda: samplerloss.energy_loss_joint(gt, mo, torch.ones(n, Tf), None, 1.0),
                 lambda: samplerloss.compute_sampler_loss(a, gt, mo, 1, None, None, q, cfg, joint=True),
                 lambda: samplerloss.compute_sampler_loss(a, gt, mo, 1, None, None, q, cfg, joint=True, recon=True, energy_weight=0.5, seg_ptr=[0, 3, 6]),
                 lambda: samplerloss.compute_sampler_loss_nba(a, gt, mo, 1, None, q, cfg, joint=True, seg_len=3)):
        with pytest.raises(capi.SttodeError):
            call()
    # the joint energy score has one kind
    with pytest.raises(ValueError, match='one kind'):
        samplerloss.compute_sampler_loss(a, gt, mo, 1, None, None, q, cfg, joint=True, energy_weight=1.0, energy_kind='fde')
    with pytest.raises(ValueError, match='one kind'):
        samplerloss.compute_sampler_loss_nba(a, gt, mo, 1, None, q, cfg, joint=True, seg_len=3, energy_kind='fde')
    # a seg_len that is missing or does not divide n
    for sl in (None, 4, 0):
        with pytest.raises(ValueError, match='seg_len'):
            samplerloss.compute_sampler_loss_nba(a, gt, mo, 1, None, q, cfg, joint=True, seg_len=sl)
    # a bad seg_ptr is refused on the host before any call (device tensors faked by a cuda-typed check being skipped: the CSR check is first)
    calls = []
    import unittest.mock as um
    with um.patch.object(capi, 'call', lambda *a_, **k_: calls.append(a_[0])):
        for sp in ([0, 3], [1, 6], [0, 4, 3, 6], [6], [[0, 6]]):
            with pytest.raises(ValueError, match='seg_ptr'):
                samplerloss._segments(sp, n, torch.device('cpu'))
    assert calls == []
    assert samplerloss._segments(None, n, torch.device('cpu')).tolist() == [0, n]
    with pytest.raises(ValueError, match='seg_ptr'):
        samplerloss.compute_sampler_loss(a, gt, mo, 1, None, None, q, cfg, seg_ptr=[0, 6])   # read only with joint=True


def test_joint_false_makes_the_calls_and_keys_of_today(monkeypatch):
    """joint=False (the default, and spelled out): the recorded capi.call names and the loss_dict keys are the parent's for every
    combination of the opt-in terms, for both front ends."""
    from helpers import sampler_args
    from sttode_amd import capi, samplerloss
    from sttode_amd.dist import Normal
    calls = []

    def fake_call(name, *a, **k):
        calls.append(name)
        for t in a:
            if torch.is_tensor(t) and t.dtype == torch.float32 and t.shape == (3,):
                t.fill_(1.5)

    monkeypatch.setattr(capi, 'call', fake_call)
    monkeypatch.setattr(capi, 'stream_ptr', lambda: None)
    n, K, Tf, nz = 3, 4, 5, 6
    gt = torch.zeros(n, Tf, 2)
    q = Normal(mu=torch.zeros(n * K, nz), logvar=torch.zeros(n * K, nz))
    monkeypatch.setattr(samplerloss, '_per_agent', lambda q_, p_, m_, s_: samplerloss._PerAgentLoss.apply(q_.mu, q_.logvar, m_, None, None, s_))
    monkeypatch.setattr(samplerloss, '_objective', lambda q_, p_, m_, g_, fm, s_: samplerloss._Objective.apply(q_.mu, q_.logvar, m_, None, None, g_, None, s_))
    a, cfg = sampler_args(), {'weight': 1, 'scale': 1}
    for kw, fwd, bwd, keys in ((dict(), 'sttode_sampler_loss', 'sttode_sampler_loss_bwd', ['kld', 'diverse', 'recon']),
                               (dict(recon=True), 'sttode_sampler_objective', 'sttode_sampler_objective_bwd', ['kld', 'diverse', 'recon']),
                               (dict(recon=True, energy_weight=0.5, energy_kind='fde'), 'sttode_sampler_objective', 'sttode_sampler_objective_bwd',
                                ['kld', 'diverse', 'recon', 'energy'])):
        for extra in (dict(), dict(joint=False)):
            for nba in (False, True):
                del calls[:]
                mo = torch.zeros(n, K, Tf, 2, requires_grad=True)
                if nba:
                    tot, ld, uw = samplerloss.compute_sampler_loss_nba(a, gt, mo, 1, None, q, cfg, **kw, **extra)
                else:
                    tot, ld, uw = samplerloss.compute_sampler_loss(a, gt, mo, 1, torch.ones(n, Tf), None, q, cfg, **kw, **extra)
                assert calls == [fwd], (kw, extra, nba, calls)
                assert list(ld) == keys and list(uw) == keys
                tot.backward()
                assert calls == [fwd, bwd], (kw, extra, nba, calls)
