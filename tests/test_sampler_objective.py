"""CPU tests of the stage-2 objective's ground-truth terms: the fixture checks itself, the public surface exists, the two
entry points are declared alike in the header and the ctypes table, every refusal names its entry point before anything is launched, and
the defaults leave compute_sampler_loss what it was."""
import inspect
import os

import numpy as np
import pytest
import torch

import sampler_objective_ref as SR
from test_capi_symbols import header_functions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ('sttode_sampler_objective', 'sttode_sampler_objective_bwd')


@pytest.fixture(scope='module')
def fixture():
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'sampler_objective.npz'))


def test_fixture_checks_itself(fixture):
    """The stored float64 values are what the restatement gives on the stored float32 inputs; the reference's recon_loss value is the mean
    of rec and its gradient the restatement's; Tf = 1 has es_ade == es_fde; the constructed branches are there."""
    z = fixture
    assert list(z['cases']) == [SR.tag(c, m) for c in SR.CASES for m in SR.MASKS]
    for case in SR.CASES:
        n, K, nz, Tf = case
        for mk in SR.MASKS:
            inp, st = SR.load_case(z, case, mk)
            a64 = [inp[k].double() for k in ('mu', 'logvar', 'pmu', 'plogvar', 'motion', 'gt')]
            w = None if inp['mask'] is None else inp['mask'].double()
            r = SR.objective(*a64, w, 2.0)
            for k in ('rec', 'es_ade', 'es_fde'):
                np.testing.assert_allclose(r[k].numpy(), st[k], rtol=1e-12, atol=1e-15, err_msg=f'{SR.tag(case, mk)} {k}')
            assert np.array_equal(r['best'].numpy(), st['best'])
            assert abs(float(st['ref_recon']) - st['rec'].mean()) <= 1e-12 * abs(float(st['ref_recon']))
            jac = SR.stored_jacobians(st, (n, K, Tf, 2))
            for k in ('rec', 'es_ade', 'es_fde'):
                d = SR.objective(*a64, w, 2.0, g={k: torch.ones(n, dtype=torch.float64)})['dmotion'].numpy()
                np.testing.assert_allclose(d, jac[k], rtol=1e-12, atol=1e-15, err_msg=f'{SR.tag(case, mk)} d {k}')
            tied = [int(a) for a in st['ties'][:, 0]] if not bool(st['tie_grad_on_lowest']) else []
            keep = np.setdiff1d(np.arange(n), tied)
            np.testing.assert_allclose(st['ref_recon_grad_best'][keep], st['d_rec_best'][keep], rtol=1e-12, atol=1e-15)
            if Tf == 1:
                assert np.array_equal(st['es_ade'], st['es_fde'])
            live = np.ones(n, bool) if w is None else w.numpy().any(1)
            for a, lo, hi in st['ties']:
                assert np.array_equal(inp['motion'][a, lo].numpy(), inp['motion'][a, hi].numpy())
                if live[a]:
                    assert st['best'][a] == min(lo, hi)
            assert (st['rec'][~live] == 0).all() and (st['best'][~live] == 0).all() and (jac['rec'][~live] == 0).all()
            if mk == 'ragged':
                m = inp['mask'].numpy()
                assert set(np.unique(m)) <= {0.0, 1.0} and m[0, -1] == 0 and (n < 2 or not m[n - 1].any())
                assert (np.asarray(jac['es_ade']).transpose(0, 2, 1, 3)[m == 0] == 0).all()  # a masked frame: no gradient
            assert np.array_equal(inp['motion'][n // 2, 0, 0].numpy(), inp['gt'][n // 2, 0].numpy())
    assert os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'sampler_objective.npz')) < 1 << 20


def test_recon_loss_and_energy_loss_exist_with_the_reference_signature():
    from sttode_amd import samplerloss
    assert list(inspect.signature(samplerloss.recon_loss).parameters)[:4] == ['fut_motion_orig', 'infer_dec_motion', 'fut_mask', 'weight']
    p = inspect.signature(samplerloss.energy_loss).parameters
    assert list(p)[:5] == ['fut_motion_orig', 'infer_dec_motion', 'fut_mask', 'weight', 'kind'] and p['kind'].default == 'ade'
    for fn in (samplerloss.compute_sampler_loss, samplerloss.compute_sampler_loss_nba):
        p = inspect.signature(fn).parameters
        for k, d in (('recon', False), ('energy_weight', 0.0), ('energy_kind', 'ade')):
            assert p[k].kind is inspect.Parameter.KEYWORD_ONLY and p[k].default == d, (fn.__name__, k)
    from sttode_amd.trainer import train_sampler_epoch
    p = inspect.signature(train_sampler_epoch).parameters
    assert (p['recon'].default, p['energy_weight'].default, p['energy_kind'].default) == (False, 0.0, 'ade')
    with pytest.raises(ValueError):
        samplerloss.energy_loss(torch.zeros(1, 2, 2), torch.zeros(1, 2, 2, 2), None, 1.0, kind='mde')


def test_entry_points_in_header_and_ctypes_table():
    from sttode_amd import capi
    fns = header_functions()
    for name in ENTRIES:
        assert name in fns and name in capi.SIGNATURES and len(fns[name]) == len(capi.SIGNATURES[name]), name
    assert len(fns[ENTRIES[0]]) == 19 and len(fns[ENTRIES[1]]) == 21
    assert capi.ABI_VERSION == 15 and capi.lib().sttode_abi_version() == 15
    src = open(os.path.join(ROOT, 'include', 'sttode_hip.h')).read()
    assert '#define STTODE_ABI_VERSION 15' in src


def _args(name, n=2, K=3, nz=4, D=8, scale=2.0, null=()):
    """Argument list of one entry point with non-null dummy addresses (nothing is dereferenced: every refusal comes before the launch)."""
    p = lambda k: None if k in null else 64
    head = [p('mu'), p('logvar'), None, None, p('motion'), p('gt'), None]
    if name == ENTRIES[0]:
        return head + [n, K, nz, D, scale] + [p(k) for k in ('kld', 'div', 'rec', 'best', 'es_ade', 'es_fde')] + [None]
    return head + [None] * 5 + [n, K, nz, D, scale] + [p(k) for k in ('dmu', 'dlogvar', 'dmotion')] + [None]


@pytest.mark.parametrize('name', ENTRIES)
def test_every_refusal_names_its_entry_point(name):
    """NULL motion, gt or outputs; K <= 1; K D > 4096; an odd D; scale <= 0 -- refused on the host, without a GPU."""
    from sttode_amd import capi
    L = capi.lib()
    outs = ('kld', 'div', 'rec', 'best', 'es_ade', 'es_fde') if name == ENTRIES[0] else ('dmu', 'dlogvar', 'dmotion')
    bad = [dict(null=(k,)) for k in ('mu', 'logvar', 'motion', 'gt') + outs]
    bad += [dict(K=1), dict(K=0), dict(K=17, D=242), dict(K=2, D=2050), dict(D=7), dict(scale=0.0), dict(scale=-1.0), dict(n=0), dict(nz=0)]
    for kw in bad:
        rc = getattr(L, name)(*_args(name, **kw))
        msg = L.sttode_last_error().decode()
        assert rc != 0 and msg.startswith(name + ':'), (kw, rc, msg)
        with pytest.raises(capi.SttodeError, match=name + ':'):
            capi.call(name, *_args(name, **kw))


def test_cpu_tensors_are_refused():
    from helpers import sampler_args
    from sttode_amd import capi, samplerloss
    from sttode_amd.dist import Normal
    n, K, Tf, nz = 3, 4, 5, 6
    mo, gt = torch.zeros(n, K, Tf, 2), torch.zeros(n, Tf, 2)
    q = Normal(mu=torch.zeros(n * K, nz), logvar=torch.zeros(n * K, nz))
    with pytest.raises(capi.SttodeError):
        samplerloss.recon_loss(gt, mo, torch.ones(n, Tf), 1.0)
    with pytest.raises(capi.SttodeError):
        samplerloss.energy_loss(gt, mo, None, 1.0, kind='fde')
    for kw in (dict(recon=True), dict(energy_weight=1.0), dict(recon=True, energy_weight=0.5, energy_kind='fde')):
        with pytest.raises(capi.SttodeError):
            samplerloss.compute_sampler_loss(sampler_args(), gt, mo, 1, torch.ones(n, Tf), None, q, {'weight': 1, 'scale': 1}, **kw)
        with pytest.raises(capi.SttodeError):
            samplerloss.compute_sampler_loss_nba(sampler_args(), gt, mo, 1, None, q, {'weight': 1, 'scale': 1}, **kw)


def test_defaults_return_the_keys_of_the_two_term_objective(monkeypatch):
    """With both terms off: one sttode_sampler_loss call and nothing else, the dict {'kld', 'diverse', 'recon': 0}, total = kld + diverse --
    although helpers.sampler_args() carries recon_weight = 5 and the caller passes a mask."""
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
    mo, gt = torch.zeros(n, K, Tf, 2), torch.zeros(n, Tf, 2)
    q = Normal(mu=torch.zeros(n * K, nz), logvar=torch.zeros(n * K, nz))
    # (the device check of _per_agent is stepped over: the tensors are on the CPU and capi.call is the recorder above)
    monkeypatch.setattr(samplerloss, '_per_agent', lambda q_, p_, m_, s_: samplerloss._PerAgentLoss.apply(q_.mu, q_.logvar, m_, None, None, s_))
    a = sampler_args()
    assert a.recon_weight == 5.0
    tot, ld, uw = samplerloss.compute_sampler_loss(a, gt, mo, 1, torch.ones(n, Tf), None, q, {'weight': 1, 'scale': 1})
    assert calls == ['sttode_sampler_loss']
    assert list(ld) == ['kld', 'diverse', 'recon'] and ld['recon'] == 0 and list(uw) == list(ld)
    assert float(tot) == float(ld['kld'] + ld['diverse'])
