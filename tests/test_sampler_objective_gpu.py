"""GPU tests of sttode_sampler_objective / _bwd (csrc/sampler_objective.hip) and of what samplerloss and the trainer build
on them, against tests/golden/sampler_objective.npz.  The yardstick is tests/train_ref.py's, through _close:
|hip - f64| <= max(4 |torch_fp32 - f64|, atol + rtol |f64|), f64 and torch-fp32 the same restatement (tests/sampler_objective_ref.py) on the
very float32 inputs the kernel got; the float64 restatement is first held to the fixture's stored values (1e-12).  Integer outputs and
everything sampler.hip already computes are bitwise.  Every output sits inside a sentinel-margined buffer.

The constructed tie (agent 0, samples 1 and K-1 identical bit for bit and nearest the ground truth): `best` must be 1 always; the
comparison of rec's gradient with the REFERENCE's autograd keeps the tied agent only if the fixture's maker found that torch puts the
gradient on the lowest index (tie_grad_on_lowest; true for the torch build the fixture was made with)."""
import copy
import functools
import os

import numpy as np
import pytest
import torch

import sampler_objective_ref as SR
from helpers import sampler_args, sampler_case_inputs
from test_train_kernels_gpu import SENT, _capi, _close, _gpu, _worst
from test_train_loss_kernels_gpu import ISENT, _dev, _Out

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FWD, BWD = 'sttode_sampler_objective', 'sttode_sampler_objective_bwd'
LAT = ('mu', 'logvar', 'pmu', 'plogvar')


@functools.lru_cache(maxsize=None)
def _fixture():
    return dict(np.load(os.path.join(ROOT, 'tests', 'golden', 'sampler_objective.npz')))


@functools.lru_cache(maxsize=None)
def _case(case, mk, prior, scale):
    """The fixture's inputs and the two references with every upstream gradient on (computed once, shared, never written); the float64 one
    is held to the fixture's stored values and per-agent gradients."""
    inp, st = SR.load_case(_fixture(), case, mk)
    if not prior:
        inp['pmu'] = inp['plogvar'] = None
    n, K, nz, Tf = case
    arg = lambda cast: [None if inp[k] is None else cast(inp[k]) for k in LAT + ('motion', 'gt', 'mask')]
    r64 = SR.objective(*arg(torch.Tensor.double), scale, g=inp['g'])
    r32 = SR.objective(*arg(lambda t: t), scale, g=inp['g'], best=r64['best'])
    for k in ('rec', 'es_ade', 'es_fde'):
        np.testing.assert_allclose(r64[k].numpy(), st[k], rtol=1e-12, atol=1e-15)
    assert np.array_equal(r64['best'].numpy(), st['best'])
    new = SR.objective(*arg(torch.Tensor.double), scale, g={k: inp['g'][k] for k in ('rec', 'es_ade', 'es_fde')})['dmotion'].numpy()
    jac = SR.stored_jacobians(st, (n, K, Tf, 2))
    want = sum(inp['g'][k].double().numpy()[:, None, None, None] * jac[k] for k in ('rec', 'es_ade', 'es_fde'))
    np.testing.assert_allclose(new, want, rtol=1e-11, atol=1e-14)
    return inp, st, r64, r32


def _run(capi, dev, inp, case, scale, mask='own', g=SR.TERMS, fill=float('nan')):
    """One forward and one backward call.  mask: 'own' (the case's) | a tensor; g: the upstream gradients that are passed (the others NULL)."""
    n, K, nz, Tf = case
    D = 2 * Tf
    st = capi.stream_ptr()
    lat = [_dev(dev, None if inp[k] is None else inp[k].numpy()) for k in LAT]
    mo, gt = inp['motion'].to(dev), inp['gt'].to(dev)
    mk = (None if inp['mask'] is None else inp['mask'].to(dev)) if isinstance(mask, str) else mask
    o = dict(kld=_Out(dev, (n,), fill), div=_Out(dev, (n,), fill), rec=_Out(dev, (n,), fill), best=_Out(dev, (n,), ISENT, torch.int32),
             es_ade=_Out(dev, (n,), fill), es_fde=_Out(dev, (n,), fill), dmu=_Out(dev, (n * K, nz), fill), dlogvar=_Out(dev, (n * K, nz), fill),
             dmotion=_Out(dev, (n, K, Tf, 2), fill))
    gs = [inp['g'][k].to(dev) if k in g else None for k in SR.TERMS]
    capi.call(FWD, *lat, mo, gt, mk, n, K, nz, D, scale, *(o[k].v for k in ('kld', 'div', 'rec', 'best', 'es_ade', 'es_fde')), st)
    capi.call(BWD, *lat, mo, gt, mk, *gs, n, K, nz, D, scale, o['dmu'].v, o['dlogvar'].v, o['dmotion'].v, st)
    torch.cuda.synchronize()
    return o


PARAMS = [(c, m, p, s) for c in SR.CASES for m in SR.MASKS for p in (False, True) for s in SR.SCALES]
_id = lambda p: '%s-%s-scale%s' % (SR.tag(p[0], p[1]), 'prior' if p[2] else 'std', p[3])


@pytest.mark.parametrize('param', PARAMS, ids=_id)
def test_objective_forward_and_backward_vs_fixture(param):
    """Both entry points under the yardstick with margins intact; kld, div, dmu, dlogvar and (new upstream gradients NULL or zero) dmotion
    == sttode_sampler_loss(_bwd); two runs and mask None / all ones give equal bits; an agent masked entirely gets nothing from the new terms."""
    capi, dev = _capi(), _gpu()
    case, mk, prior, scale = param
    n, K, nz, Tf = case
    inp, st, r64, r32 = _case(*param)
    what = 'objective ' + _id(param)
    o = _run(capi, dev, inp, case, scale)
    worst = {}
    for k in SR.TERMS + ('dmu', 'dlogvar', 'dmotion'):
        worst[k] = _close(o[k].v, r64[k], r32[k], f'{what} {k}')
    assert torch.equal(o['best'].v.cpu(), r64['best'].int()), f'{what}: best {o["best"].v.tolist()} != {r64["best"].tolist()}'
    for k, v in o.items():
        assert v.margins_ok(), f'{what}: wrote outside {k}'
    # what sampler.hip computes: the same bits
    s = capi.stream_ptr()
    lat = [_dev(dev, None if inp[k] is None else inp[k].numpy()) for k in LAT]
    mo, g = inp['motion'].to(dev).view(n, K, 2 * Tf), {k: v.to(dev) for k, v in inp['g'].items()}
    p = dict(kld=_Out(dev, (n,)), div=_Out(dev, (n,)), dmu=_Out(dev, (n * K, nz)), dlogvar=_Out(dev, (n * K, nz)), dmotion=_Out(dev, (n, K, Tf, 2)))
    capi.call('sttode_sampler_loss', *lat, mo, n, K, nz, 2 * Tf, scale, p['kld'].v, p['div'].v, s)
    capi.call('sttode_sampler_loss_bwd', *lat, mo, g['kld'], g['div'], n, K, nz, 2 * Tf, scale, p['dmu'].v, p['dlogvar'].v, p['dmotion'].v, s)
    torch.cuda.synchronize()
    for k in ('kld', 'div', 'dmu', 'dlogvar'):
        assert torch.equal(o[k].v, p[k].v), f'{what}: {k} differs from sttode_sampler_loss'
    old = _run(capi, dev, inp, case, scale, g=('kld', 'div'))
    assert torch.equal(old['dmotion'].v, p['dmotion'].v), f'{what}: dmotion with NULL g_rec, g_es_* differs from sttode_sampler_loss_bwd'
    zero = dict(inp, g={k: (v if k in ('kld', 'div') else torch.zeros_like(v)) for k, v in inp['g'].items()})
    assert torch.equal(_run(capi, dev, zero, case, scale)['dmotion'].v, p['dmotion'].v), f'{what}: dmotion with zero g_rec, g_es_*'
    # determinism; mask None == all ones
    again = _run(capi, dev, inp, case, scale)
    for k in o:
        assert torch.equal(o[k].v, again[k].v), f'{what}: two runs differ in {k}'
    if mk == 'none':
        ones = _run(capi, dev, inp, case, scale, mask=torch.ones(n, Tf, device=dev))
        for k in o:
            assert torch.equal(o[k].v, ones[k].v), f'{what}: mask None and all ones differ in {k}'
    # the new terms alone
    new = _run(capi, dev, inp, case, scale, g=('rec', 'es_ade', 'es_fde'))
    assert (new['dmu'].v == 0).all() and (new['dlogvar'].v == 0).all()
    live = np.ones(n, bool) if inp['mask'] is None else inp['mask'].numpy().any(1)
    dead = torch.from_numpy(~live).to(dev)
    assert (o['rec'].v[dead] == 0).all() and (o['best'].v[dead] == 0).all() and (new['dmotion'].v[dead] == 0).all()
    assert (o['es_ade'].v[dead] == 0).all() and (o['es_fde'].v[dead] == 0).all()
    if inp['mask'] is not None:
        gone = (inp['mask'] == 0).to(dev)                                                   # [n,Tf]: no gradient at a masked frame
        assert (new['dmotion'].v.transpose(1, 2)[gone] == 0).all()
        last = (inp['mask'][:, -1] == 0).to(dev)
        only = _run(capi, dev, inp, case, scale, g=('es_fde',))
        assert (only['dmotion'].v[last] == 0).all() and (only['dmotion'].v[:, :, :-1] == 0).all()
    if Tf == 1:
        assert torch.equal(o['es_ade'].v, o['es_fde'].v)
    k = max(worst, key=worst.get)
    _worst(f'sampler objective {_id(param)} (at {k})', worst[k])


def test_objective_refusals_write_nothing():
    """K = 1, K D = 4097 + (one float more than the LDS holds), an odd D, scale 0, NULL gt, NULL motion, a NULL output: forward and backward
    refuse, naming themselves, and every output keeps its sentinel."""
    capi, dev = _capi(), _gpu()
    st = capi.stream_ptr()
    z = lambda *s: torch.zeros(*s, device=dev)
    for label, (n, K, nz, D, scale), null in (('K = 1', (2, 1, 4, 8, 2.0), ()), ('K D = 4114', (2, 17, 4, 242, 2.0), ()), ('D odd', (2, 3, 4, 7, 2.0), ()),
                                              ('scale 0', (2, 3, 4, 8, 0.0), ()), ('null gt', (2, 3, 4, 8, 2.0), ('gt',)),
                                              ('null motion', (2, 3, 4, 8, 2.0), ('motion',)), ('null es_fde / dmotion', (2, 3, 4, 8, 2.0), ('out',))):
        mu, lv, g = z(n * K, nz), z(n * K, nz), z(n)
        mo = None if 'motion' in null else z(n, K, D)
        gt = None if 'gt' in null else z(n, D)
        o = dict(kld=_Out(dev, (n,), SENT), div=_Out(dev, (n,), SENT), rec=_Out(dev, (n,), SENT), best=_Out(dev, (n,), ISENT, torch.int32),
                 es_ade=_Out(dev, (n,), SENT), es_fde=_Out(dev, (n,), SENT), dmu=_Out(dev, (n * K, nz), SENT), dlogvar=_Out(dev, (n * K, nz), SENT),
                 dmotion=_Out(dev, (n, K, D), SENT))
        with pytest.raises(capi.SttodeError, match=FWD + ':'):
            capi.call(FWD, mu, lv, None, None, mo, gt, None, n, K, nz, D, scale, o['kld'].v, o['div'].v, o['rec'].v, o['best'].v, o['es_ade'].v,
                      None if 'out' in null else o['es_fde'].v, st)
        with pytest.raises(capi.SttodeError, match=BWD + ':'):
            capi.call(BWD, mu, lv, None, None, mo, gt, None, g, g, g, g, g, n, K, nz, D, scale, o['dmu'].v, o['dlogvar'].v,
                      None if 'out' in null else o['dmotion'].v, st)
        torch.cuda.synchronize()
        for k, v in o.items():
            assert v.untouched(), f'{label}: refused, but wrote {k}'


@pytest.mark.parametrize('case', SR.CASES, ids=lambda c: SR.tag(c, 'x')[:-2])
@pytest.mark.parametrize('mk', SR.MASKS)
def test_energy_scores_vs_sample_spread(case, mk):
    """metrics.sample_spread (float64) at coordinate scale 1 on the masked coordinates gives the same energy scores."""
    from sttode_amd import metrics
    capi, dev = _capi(), _gpu()
    inp, st, r64, r32 = _case(case, mk, False, 2.0)
    o = _run(capi, dev, inp, case, 2.0)
    w = torch.ones(case[0], case[3]) if inp['mask'] is None else inp['mask']
    sp = metrics.sample_spread((inp['motion'] * w[:, None, :, None]).to(dev), (inp['gt'] * w[:, :, None]).to(dev), scale=1.0)
    torch.cuda.synchronize()
    worst = max(_close(o[k].v, getattr(sp, k), r32[k], f'{SR.tag(case, mk)} {k} vs sample_spread') for k in ('es_ade', 'es_fde'))
    _worst(f'sampler objective {SR.tag(case, mk)} energy scores vs sample_spread', worst)


@pytest.mark.parametrize('case', SR.CASES, ids=lambda c: SR.tag(c, 'x')[:-2])
@pytest.mark.parametrize('mk', SR.MASKS)
def test_recon_loss_and_energy_loss_vs_reference_value_and_gradient(case, mk):
    """samplerloss.recon_loss against the REFERENCE's own recon_loss value and autograd gradient (stored in float64); energy_loss against the
    stored restatement.  fut_mask as a CPU tensor (what the existing callers pass) and as a device tensor give equal bits."""
    from sttode_amd import samplerloss
    dev = _gpu()
    n, K, nz, Tf = case
    inp, st, r64, r32 = _case(case, mk, False, 2.0)
    gt = inp['gt'].to(dev)
    jac = SR.stored_jacobians(st, (n, K, Tf, 2))
    j32 = {k: SR.objective(*[inp[a] for a in LAT[:2]], None, None, inp['motion'], inp['gt'], inp['mask'], 2.0, g={k: torch.ones(n)},
                           best=r64['best'])['dmotion'] for k in ('rec', 'es_ade', 'es_fde')}
    keep = torch.ones(n, dtype=torch.bool)
    if not bool(st['tie_grad_on_lowest']):
        keep[[int(a) for a in st['ties'][:, 0]]] = False
    worst = {}
    for name, fn, key, val in (('recon_loss', samplerloss.recon_loss, 'rec', float(st['ref_recon'])),
                               ('energy_loss ade', functools.partial(samplerloss.energy_loss, kind='ade'), 'es_ade', st['es_ade'].mean()),
                               ('energy_loss fde', functools.partial(samplerloss.energy_loss, kind='fde'), 'es_fde', st['es_fde'].mean())):
        res = []
        for mask in ((None,) if inp['mask'] is None else (inp['mask'], inp['mask'].to(dev))):
            x = inp['motion'].to(dev).requires_grad_(True)
            loss, uw = fn(gt, x, mask, 3.0)
            loss.backward()
            res.append((loss.detach(), uw.detach(), x.grad))
        if len(res) == 2:
            assert all(torch.equal(a, b) for a, b in zip(*res)), f'{name}: a CPU mask and a device mask differ'
        loss, uw, grad = res[0]
        assert float(loss) == float(uw * 3.0)
        what = f'{name} {SR.tag(case, mk)}'
        worst[name] = _close(uw.reshape(1), torch.tensor([val], dtype=torch.float64), r32[key].mean().reshape(1), what)
        ref_grad = torch.from_numpy(jac[key]) * (3.0 / n)
        if key == 'rec':                                            # the reference's autograd, where the fixture stores it
            full = np.zeros((n, K, Tf, 2))
            full[np.arange(n), st['best']] = st['ref_recon_grad_best']
            ref_grad = torch.from_numpy(full) * (3.0 / n)
        worst[name + ' grad'] = _close(grad[keep.to(dev)], ref_grad[keep], j32[key][keep] * (3.0 / n), what + ' gradient')
    k = max(worst, key=worst.get)
    _worst(f'samplerloss {SR.tag(case, mk)} (at {k})', worst[k])


def _eth(dev):
    from sttode_amd import Sampler
    from sttode_amd.weights import make_sampler_weights, to_torch_state_dict
    from test_gpu_parity import hip_model
    g = dict(np.load(os.path.join(ROOT, 'tests', 'golden', 'sampler.npz')))
    net = hip_model('eth', 8, 12)
    smp = Sampler(sampler_args('eth', 8, 12))
    smp.load_state_dict(to_torch_state_dict(make_sampler_weights()), strict=True)
    smp.set_device(dev)
    inp, fut = sampler_case_inputs(g, 'eth', 'eth')
    n = inp['obs'].shape[0]

    def forward():
        net.set_data(None, torch.from_numpy(inp['obs']), torch.from_numpy(inp['pred']), torch.ones(n, 8), torch.ones(n, 12))
        return smp.forward(net, mean=False, eps=torch.from_numpy(g['eth_shared_eps']))
    mask = torch.ones(n, 12)
    mask[0, 7:] = 0
    mask[n - 1, ::2] = 0
    return g, smp, forward, torch.from_numpy(fut).to(dev), mask, n


def _grads(smp):
    out = {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in smp.named_parameters()}
    smp.zero_grad(set_to_none=True)
    return out


def test_compute_sampler_loss_sum_of_parts_and_defaults_at_the_eth_golden_case():
    """recon=True, energy_weight=w: total == kld + diverse + recon + energy with each part what recon_loss / energy_loss / the two-term
    objective give on their own.  Both off: bitwise the two-term objective (its statements, spelled out here), values and gradients, and the
    golden losses of tests/golden/sampler.npz."""
    from sttode_amd import samplerloss
    dev = _gpu()
    g, smp, forward, fut, mask, n = _eth(dev)
    a, cfg = smp.args, {'weight': 1, 'scale': 1}
    assert a.recon_weight == 5.0
    dec, sd, vd, _ = forward()
    tot0, ld0, uw0 = samplerloss.compute_sampler_loss(a, fut, dec, 1, torch.ones(n, 12), vd, sd, cfg)
    assert list(ld0) == ['kld', 'diverse', 'recon'] and ld0['recon'] == 0 and list(uw0) == list(ld0)
    np.testing.assert_allclose([float(v.detach()) for v in (tot0, ld0['kld'], ld0['diverse'])], g['eth_shared_loss'], rtol=1e-4)
    tot0.backward()
    g0 = _grads(smp)
    dec, sd, vd, _ = forward()                                                              # the two-term objective, statement by statement
    kld_a, div_a = samplerloss._per_agent(sd, vd, dec, cfg['scale'])
    kl = (kld_a.sum() / n).clamp_min(a.kld_min_clamp) * a.kld_weight
    dv = div_a.sum() / n * cfg['weight']
    assert torch.equal(tot0.detach(), (kl + dv).detach()) and torch.equal(ld0['kld'].detach(), kl.detach()) and torch.equal(ld0['diverse'].detach(), dv.detach())
    (kl + dv).backward()
    g1 = _grads(smp)
    assert all((g0[k] is None and g1[k] is None) or torch.equal(g0[k], g1[k]) for k in g0), 'defaults: gradients differ from the two-term objective'
    for kind, w in (('ade', 0.7), ('fde', 2.0)):
        dec, sd, vd, _ = forward()
        tot, ld, _ = samplerloss.compute_sampler_loss(a, fut, dec, 1, mask, vd, sd, cfg, recon=True, energy_weight=w, energy_kind=kind)
        assert list(ld) == ['kld', 'diverse', 'recon', 'energy']
        with torch.no_grad():
            rec, rec_uw = samplerloss.recon_loss(fut, dec, mask, a.recon_weight)
            en, en_uw = samplerloss.energy_loss(fut, dec, mask, w, kind)
        assert torch.equal(ld['kld'].detach(), ld0['kld'].detach()) and torch.equal(ld['diverse'].detach(), ld0['diverse'].detach())
        assert torch.equal(ld['recon'].detach(), rec) and torch.equal(ld['energy'].detach(), en) and float(rec) == float(rec_uw * 5.0)
        assert float(tot.detach()) == float((((ld['kld'] + ld['diverse']) + ld['recon']) + ld['energy']).detach())
        only_rec, ld_r, _ = samplerloss.compute_sampler_loss(a, fut, dec, 1, mask, vd, sd, cfg, recon=True)
        assert list(ld_r) == ['kld', 'diverse', 'recon'] and float(only_rec.detach()) == float(((ld['kld'] + ld['diverse']) + ld['recon']).detach())


def test_end_to_end_gradients_and_one_training_epoch():
    """Sampler.forward -> compute_sampler_loss(recon=True, energy_weight=1) -> backward: finite gradients on every parameter but q_c.*, equal
    (under the yardstick, the hand-fed gradients as both references) to feeding the entry points' own dmotion, dmu, dlogvar back through the
    sampler's graph by hand -- _SamplerFn.backward is linear in them.  Then one train_sampler_epoch with the term on, which logs it."""
    from sttode_amd import samplerloss, scenes
    from sttode_amd.trainer import train_sampler_epoch
    capi, dev = _capi(), _gpu()
    g, smp, forward, fut, mask, n = _eth(dev)
    a, cfg = smp.args, {'weight': 1, 'scale': 1}
    K, nz, Tf = 20, 32, 12
    dec, sd, vd, _ = forward()
    tot, ld, _ = samplerloss.compute_sampler_loss(a, fut, dec, 1, mask, vd, sd, cfg, recon=True, energy_weight=1.0)
    tot.backward()
    got = _grads(smp)
    for k, v in got.items():
        assert (v is None) == k.startswith('q_c.'), k
        assert v is None or bool(torch.isfinite(v).all()), k
    # by hand: the upstream gradients of the per-agent terms, one backward call, and the sampler's own graph
    dec, sd, vd, _ = forward()
    mu, lv, mo = sd.mu.detach().contiguous(), sd.logvar.detach().contiguous(), dec.detach().contiguous()
    pmu, plv = vd.mu.detach().float().contiguous(), vd.logvar.detach().float().contiguous()
    md = mask.to(dev)
    o = [torch.empty(n, device=dev) for _ in range(3)] + [torch.empty(n, dtype=torch.int32, device=dev)] + [torch.empty(n, device=dev) for _ in range(2)]
    capi.call(FWD, mu, lv, pmu, plv, mo, fut, md, n, K, nz, 2 * Tf, float(cfg['scale']), *o, capi.stream_ptr())
    live = float(o[0].sum() / n) > a.kld_min_clamp
    full = lambda v: torch.full((n,), v / n, device=dev)
    gs = [full(a.kld_weight if live else 0.0), full(float(cfg['weight'])), full(a.recon_weight), full(1.0), None]
    dmu, dlv, dmo = torch.empty_like(mu), torch.empty_like(lv), torch.empty_like(mo)
    capi.call(BWD, mu, lv, pmu, plv, mo, fut, md, *gs, n, K, nz, 2 * Tf, float(cfg['scale']), dmu, dlv, dmo, capi.stream_ptr())
    torch.autograd.backward([dec, sd.mu, sd.logvar], [dmo, dmu, dlv])
    hand = _grads(smp)
    worst = max(_close(got[k], hand[k], hand[k], f'end to end {k}') for k in got if got[k] is not None)
    _worst('sampler objective end to end', worst)
    # one epoch of two scenes with the reconstruction term on
    loader = []
    for s in (4242, 4243):
        ob, pr = scenes.eth_scene(s, n_min=9, n_max=9)
        ob, pr = torch.from_numpy(ob), torch.from_numpy(pr)
        N = ob.shape[0]
        pm = torch.ones(1, N, Tf)
        pm[0, 0, 9:] = 0
        loader.append([ob[None], pr[None], ob[None], pr[None], torch.zeros(1, N), torch.ones(1, N), torch.ones(1, N, 8), pm, torch.tensor([[10]]), ['seq']])
    s0 = copy.deepcopy(smp).train()
    opt = torch.optim.Adam(s0.parameters(), lr=1e-3)
    lines = []
    from test_gpu_parity import hip_model
    losses = train_sampler_epoch(s0.args, 0, hip_model('eth', 8, 12), s0, opt, None, loader, samplerloss.get_diversity_config('eth'), log=lines.append,
                                 max_iters=2, recon=True)
    assert len(losses) == 2 and all(np.isfinite(losses)) and len(lines) == 1 and '| recon: ' in lines[0] and 'energy' not in lines[0], lines
