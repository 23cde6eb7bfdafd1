"""GPU tests of sttode_sampler_objective_joint / _bwd (csrc/sampler_joint.hip) and of what samplerloss and the trainer build
on them.  The yardstick is tests/train_ref.py's, through _close: |hip - f64| <= max(4 |torch_fp32 - f64|, atol + rtol |f64|), f64 and
torch-fp32 the same restatement (tests/sampler_joint_ref.py) on the very float32 inputs the kernel got.  Integer outputs and everything
sampler.hip already computes are bitwise.  Every output sits inside a sentinel-margined buffer.

Shapes: sampler_joint_ref.SHAPES with the segment sizes of GPU_SEGS (1, 2, 11, 64, 65, at the training shape 257, and two equal
segments of 3) in one batch; the inputs are drawn from a fixed seed and meet sampler_joint_ref.conditions (asserted)."""
import copy
import functools
import os

import numpy as np
import pytest
import torch

import sampler_joint_ref as JR
import sampler_objective_ref as SR
from helpers import sampler_args
from test_train_kernels_gpu import SENT, _capi, _close, _gpu, _worst
from test_train_loss_kernels_gpu import ISENT, _dev, _Out

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FWD, BWD = 'sttode_sampler_objective_joint', 'sttode_sampler_objective_joint_bwd'
LAT = ('mu', 'logvar', 'pmu', 'plogvar')
TRAIN = (20, 32, 12)


@functools.lru_cache(maxsize=None)
def _inputs(shape, mk):
    """The seeded inputs of one (shape, mask) with the GPU tests' segments; the input conditions hold (make_case asserts them)."""
    inp, _ = JR.make_case(shape, JR.GPU_SEGS[shape], mk, 7000 + 100 * JR.SHAPES.index(shape))
    return inp


@functools.lru_cache(maxsize=None)
def _refs(shape, mk, prior, scale):
    """The two references with every upstream gradient on (computed once, shared, never written)."""
    inp = _inputs(shape, mk)
    g = JR.upstream(inp)
    r64 = JR.objective(*JR.as_torch(inp, torch.float64, prior), scale, g=g)
    r32 = JR.objective(*JR.as_torch(inp, torch.float32, prior), scale, g=g, best=r64['best'])
    return r64, r32


class _Run:
    """One forward and one backward call on sentinel-margined outputs.  inp: numpy inputs (JR.draw); g: the upstream gradients that are
    passed (the others NULL); mask: 'own' | a device tensor | None."""

    def __init__(self, capi, dev, inp, shape, scale, prior=True, g=JR.TERMS, mask='own', seg_ptr=None, fwd=True, bwd=True):
        K, nz, Tf = shape
        n = inp['motion'].shape[0]
        sp = np.asarray(inp['seg_ptr'] if seg_ptr is None else seg_ptr, np.int32)
        S = len(sp) - 1
        st = capi.stream_ptr()
        lat = [_dev(dev, inp[k]) if (prior or k in LAT[:2]) else None for k in LAT]
        mo, gt, spd = _dev(dev, inp['motion']), _dev(dev, inp['gt']), _dev(dev, sp)
        mkd = _dev(dev, inp['mask']) if isinstance(mask, str) else mask
        nan = float('nan')
        self.o = dict(kld=_Out(dev, (n,), nan), div=_Out(dev, (S,), nan), rec=_Out(dev, (S,), nan), best=_Out(dev, (S,), ISENT, torch.int32),
                      es=_Out(dev, (S,), nan), dmu=_Out(dev, (n * K, nz), nan), dlogvar=_Out(dev, (n * K, nz), nan),
                      dmotion=_Out(dev, (n, K, Tf, 2), nan))
        nb = capi.sampler_joint_ws(n, K, S)
        self.ws = _Out(dev, (nb // 4,), nan, margin=64)                                     # (nb is a multiple of 4; 8-aligned: margin 64 floats)
        assert self.ws.v.data_ptr() % 8 == 0
        gs = [_dev(dev, inp['g'][k]) if k in g else None for k in JR.TERMS]
        o = self.o
        if fwd:
            capi.call(FWD, *lat, mo, gt, mkd, spd, S, n, K, nz, 2 * Tf, scale, self.ws.v, nb, o['kld'].v, o['div'].v, o['rec'].v, o['best'].v,
                      o['es'].v, st)
        if bwd:
            self.ws.v.fill_(nan)                                                            # the backward relies on nothing the forward left
            capi.call(BWD, *lat, mo, gt, mkd, spd, S, *gs, n, K, nz, 2 * Tf, scale, self.ws.v, nb, o['dmu'].v, o['dlogvar'].v, o['dmotion'].v, st)
        torch.cuda.synchronize()

    def __getitem__(self, k):
        return self.o[k].v

    def margins_ok(self):
        return all(v.margins_ok() for v in self.o.values()) and self.ws.margins_ok()


PARAMS = [(s, m, p, sc) for s in JR.SHAPES for m in JR.MASKS for p, sc in ((False, 2.0), (True, 0.5))]
_id = lambda p: '%s-%s-scale%s' % (JR.tag(p[0], p[1]), 'prior' if p[2] else 'std', p[3])
OUTS = JR.TERMS + ('dmu', 'dlogvar', 'dmotion')


@pytest.mark.parametrize('param', PARAMS, ids=_id)
def test_joint_forward_and_backward_vs_float64(param):
    """Both entry points under the yardstick with margins intact; best exact (the constructed tie: the lower index; the sample equal to
    the ground truth); kld, dmu, dlogvar == sttode_sampler_loss(_bwd); with only g_kld, dmotion is exactly zero; two runs and mask None /
    all ones give equal bits."""
    capi, dev = _capi(), _gpu()
    shape, mk, prior, scale = param
    K, nz, Tf = shape
    inp = _inputs(shape, mk)
    segs = JR.GPU_SEGS[shape]
    n = inp['motion'].shape[0]
    r64, r32 = _refs(*param)
    what = 'joint ' + _id(param)
    o = _Run(capi, dev, inp, shape, scale, prior)
    worst = {k: _close(o[k], r64[k], r32[k], f'{what} {k}') for k in OUTS}
    assert torch.equal(o['best'].cpu(), r64['best'].int()), f'{what}: best {o["best"].tolist()} != {r64["best"].tolist()}'
    tie, eq = JR.roles(segs, K)
    assert (tie is None or int(o['best'][tie]) == 1) and int(o['best'][eq]) == 0 and float(o['rec'][eq]) == 0.0
    assert o.margins_ok(), f'{what}: wrote outside an output or the workspace'
    # what sampler.hip computes: the same bits
    s = capi.stream_ptr()
    lat = [_dev(dev, inp[k]) if (prior or k in LAT[:2]) else None for k in LAT]
    mo, gk = _dev(dev, inp['motion']).view(n, K, 2 * Tf), _dev(dev, inp['g']['kld'])
    p = dict(kld=_Out(dev, (n,)), div=_Out(dev, (n,)), dmu=_Out(dev, (n * K, nz)), dlogvar=_Out(dev, (n * K, nz)), dmotion=_Out(dev, (n, K, Tf, 2)))
    capi.call('sttode_sampler_loss', *lat, mo, n, K, nz, 2 * Tf, scale, p['kld'].v, p['div'].v, s)
    capi.call('sttode_sampler_loss_bwd', *lat, mo, gk, torch.zeros(n, device=dev), n, K, nz, 2 * Tf, scale, p['dmu'].v, p['dlogvar'].v,
              p['dmotion'].v, s)
    torch.cuda.synchronize()
    for k in ('kld', 'dmu', 'dlogvar'):
        assert torch.equal(o[k], p[k].v), f'{what}: {k} differs from sttode_sampler_loss'
    only = _Run(capi, dev, inp, shape, scale, prior, g=('kld',))
    assert (only['dmotion'] == 0).all() and torch.equal(only['dmu'], p['dmu'].v) and torch.equal(only['dlogvar'], p['dlogvar'].v)
    new = _Run(capi, dev, inp, shape, scale, prior, g=('div', 'rec', 'es'))
    assert (new['dmu'] == 0).all() and (new['dlogvar'] == 0).all()
    # determinism; mask None == all ones
    again = _Run(capi, dev, inp, shape, scale, prior)
    for k in o.o:
        assert torch.equal(o[k], again[k]), f'{what}: two runs differ in {k}'
    if mk == 'none':
        ones = _Run(capi, dev, inp, shape, scale, prior, mask=torch.ones(n, Tf, device=dev))
        for k in o.o:
            assert torch.equal(o[k], ones[k]), f'{what}: mask None and all ones differ in {k}'
    else:
        # a masked frame takes no gradient from rec and es (DLow is unmasked)
        ge = _Run(capi, dev, inp, shape, scale, prior, g=('rec', 'es'))
        gone = torch.from_numpy(inp['mask'] == 0).to(dev)
        assert (ge['dmotion'].transpose(1, 2)[gone] == 0).all()
    k = max(worst, key=worst.get)
    _worst(f'sampler joint {_id(param)} (at {k})', worst[k])
    for fam in (('div', 'rec', 'es'), ('dmotion',), ('kld', 'dmu', 'dlogvar')):
        _worst(f'sampler joint family {"/".join(fam)} {_id(param)}', max(worst[f] for f in fam))


def test_fixture_cases_vs_stored_float64():
    """tests/golden/sampler_joint.npz: the stored float64 values and gradients of the small cases (scale 2, no prior), under the yardstick
    with torch's own float32 evaluation computed on the spot."""
    capi, dev = _capi(), _gpu()
    z = np.load(os.path.join(ROOT, 'tests', 'golden', 'sampler_joint.npz'))
    worst = 0.0
    for shape in JR.SHAPES:
        for mk in JR.GOLDEN_MASKS[shape]:
            t = JR.tag(shape, mk)
            inp = JR.draw(int(z[t + '/seed']), shape, JR.GOLDEN_SEGS[shape], mk)
            assert np.array_equal(inp['motion'], z[t + '/motion'])
            g = {k: torch.from_numpy(z[t + '/g_' + k]) for k in ('div', 'rec', 'es')}
            r32 = JR.objective(*JR.as_torch(inp, torch.float32, False), 2.0, g=g, best=torch.from_numpy(z[t + '/best']))
            o = _Run(capi, dev, inp, shape, 2.0, prior=False, g=('div', 'rec', 'es'))
            for k in ('div', 'rec', 'es', 'dmotion'):
                worst = max(worst, _close(o[k], torch.from_numpy(z[t + '/' + k]), r32[k], f'fixture {t} {k}'))
            assert np.array_equal(o['best'].cpu().numpy(), z[t + '/best']) and o.margins_ok(), t
    _worst('sampler joint fixture cases', worst)


def _sub(inp, shape, a0, a1, sp):
    """The agents [a0, a1) of a case as a case of their own with the CSR sp (upstream gradients per segment: the caller's)."""
    K = shape[0]
    rows = slice(a0 * K, a1 * K)
    out = {k: inp[k][rows] for k in LAT}
    out.update(motion=inp['motion'][a0:a1], gt=inp['gt'][a0:a1], mask=None if inp['mask'] is None else inp['mask'][a0:a1],
               seg_ptr=np.asarray(sp, np.int32))
    return out


@pytest.mark.parametrize('mk', JR.MASKS)
def test_segments_do_not_depend_on_the_batch(mk):
    """Appending a segment to the batch, or putting one to three agents in front as a segment of their own, leaves the other segments'
    outputs and gradients bitwise unchanged (training shape; the 257-agent segment among them)."""
    capi, dev = _capi(), _gpu()
    shape = TRAIN
    K, nz, Tf = shape
    inp = _inputs(shape, mk)
    sp = inp['seg_ptr']
    S, n = len(sp) - 1, int(sp[-1])
    full = _Run(capi, dev, inp, shape, 2.0)
    # without the last segment (= the full batch is this one with a segment appended)
    cut = _sub(inp, shape, 0, int(sp[-2]), sp[:-1])
    cut['g'] = {k: (v[:sp[-2]] if k == 'kld' else v[:-1]) for k, v in inp['g'].items()}
    a = _Run(capi, dev, cut, shape, 2.0)
    for k in ('div', 'rec', 'best', 'es'):
        assert torch.equal(a[k], full[k][:-1]), f'appending a segment changed {k}'
    for k, per in (('kld', 1), ('dmu', K), ('dlogvar', K), ('dmotion', 1)):
        assert torch.equal(a[k], full[k][:int(sp[-2]) * per]), f'appending a segment changed {k}'
    # without the first one, two or three agents: segments 0 (1 agent), 0-1 (3 agents) cut away, and the front moved by them
    for first in (1, 2):
        a0 = int(sp[first])
        tail = _sub(inp, shape, a0, n, sp[first:] - a0)
        tail['g'] = {k: (v[a0:] if k == 'kld' else v[first:]) for k, v in inp['g'].items()}
        b = _Run(capi, dev, tail, shape, 2.0)
        for k in ('div', 'rec', 'best', 'es'):
            assert torch.equal(b[k], full[k][first:]), f'{a0} agents in front changed {k}'
        for k, per in (('kld', 1), ('dmu', K), ('dlogvar', K), ('dmotion', 1)):
            assert torch.equal(b[k], full[k][a0 * per:]), f'{a0} agents in front changed {k}'
    # two agents in front as a segment of their own: the batch's agents 1.. behind agents 0, 0 (a copy) -- the tail again, moved by 2
    a0 = int(sp[1])
    two = {k: np.concatenate([inp[k][:K], inp[k][:K], inp[k][a0 * K:]]) for k in LAT}
    cat = lambda v: np.concatenate([v[:1], v[:1], v[a0:]])
    two.update(motion=cat(inp['motion']), gt=cat(inp['gt']), mask=None if inp['mask'] is None else cat(inp['mask']),
               seg_ptr=np.concatenate([[0], sp[1:] - a0 + 2]).astype(np.int32), g={k: (cat(v) if k == 'kld' else v) for k, v in inp['g'].items()})
    c = _Run(capi, dev, two, shape, 2.0)
    for k in ('div', 'rec', 'best', 'es'):
        assert torch.equal(c[k][1:], full[k][1:]), f'two agents in front changed {k}'
    assert torch.equal(c['dmotion'][2:], full['dmotion'][a0:]), 'two agents in front changed dmotion'


def test_nan_stays_in_its_segment_and_best_stays_valid():
    """A NaN coordinate in one sample of one agent: that segment's best is a valid column (the NaN sample never wins), its div and es are
    NaN; a segment whose every J is NaN gets best 0 and rec NaN; every other segment keeps its bits."""
    capi, dev = _capi(), _gpu()
    shape = TRAIN
    K, nz, Tf = shape
    inp = dict(_inputs(shape, 'none'))
    sp = inp['seg_ptr']
    clean = _Run(capi, dev, inp, shape, 2.0)
    mo = inp['motion'].copy()
    s1, s2 = 3, 4                                                                           # the 64- and the 65-agent segment
    k_bad = int(clean['best'][s1])
    mo[sp[s1] + 5, k_bad, 3, 1] = np.nan                                                    # the sample that would have won
    mo[sp[s2] + 7, :, 0, 0] = np.nan                                                        # every sample of one agent
    inp['motion'] = mo
    o = _Run(capi, dev, inp, shape, 2.0)
    best = o['best'].cpu().numpy()
    assert ((best >= 0) & (best < K)).all()
    assert best[s1] != k_bad and np.isfinite(float(o['rec'][s1])) and np.isnan(float(o['div'][s1])) and np.isnan(float(o['es'][s1]))
    J = JR.objective(*JR.as_torch(inp, torch.float64), 2.0)['J'][s1].numpy()
    assert best[s1] == int(np.nanargmin(J))
    assert best[s2] == 0 and all(np.isnan(float(o[k][s2])) for k in ('div', 'rec', 'es'))
    keep = [s for s in range(len(sp) - 1) if s not in (s1, s2)]
    for k in ('div', 'rec', 'best', 'es'):
        assert torch.equal(o[k][keep], clean[k][keep]), f'a NaN left its segment in {k}'
    rows = np.concatenate([np.arange(sp[s], sp[s + 1]) for s in keep])
    assert torch.equal(o['dmotion'][rows], clean['dmotion'][rows]) and torch.equal(o['kld'], clean['kld'])
    assert o.margins_ok()


def test_empty_segment_writes_nan_and_index_zero():
    capi, dev = _capi(), _gpu()
    shape = (3, 5, 10)
    inp = dict(_inputs(shape, 'none'))
    sp = inp['seg_ptr']
    full = _Run(capi, dev, inp, shape, 2.0)
    sp2 = np.concatenate([sp[:3], sp[2:]]).astype(np.int32)                                 # an empty segment in the middle
    inp['g'] = {k: (v if k == 'kld' else np.concatenate([v[:2], v[:1], v[2:]])) for k, v in inp['g'].items()}
    inp['seg_ptr'] = sp2
    o = _Run(capi, dev, inp, shape, 2.0)
    assert all(np.isnan(float(o[k][2])) for k in ('div', 'rec', 'es')) and int(o['best'][2]) == 0
    keep = [0, 1] + list(range(3, len(sp2) - 1))
    for k in ('div', 'rec', 'best', 'es'):
        assert torch.equal(o[k][keep], full[k])
    assert torch.equal(o['dmotion'], full['dmotion']) and o.margins_ok()


def test_joint_refusals_write_nothing():
    """K = 1, K D > 4096, an odd D, scale 0, S = 0, a NULL gt / motion / seg_ptr / workspace / output, a short workspace: forward and
    backward refuse, naming themselves, and every output and the workspace keep their sentinels."""
    capi, dev = _capi(), _gpu()
    st = capi.stream_ptr()
    z = lambda *s: torch.zeros(*s, device=dev)
    ok = (2, 3, 4, 8, 1, 2.0)
    for label, (n, K, nz, D, S, scale), null in (('K = 1', (2, 1, 4, 8, 1, 2.0), ()), ('K D = 4114', (2, 17, 4, 242, 1, 2.0), ()),
                                                 ('D odd', (2, 3, 4, 7, 1, 2.0), ()), ('scale 0', (2, 3, 4, 8, 1, 0.0), ()), ('S = 0', (2, 3, 4, 8, 0, 2.0), ()),
                                                 ('null gt', ok, ('gt',)), ('null motion', ok, ('motion',)), ('null seg_ptr', ok, ('seg_ptr',)),
                                                 ('null workspace', ok, ('ws',)), ('null es / dmotion', ok, ('out',)), ('short workspace', ok, ('short',))):
        mu, lv, g, gs = z(n * K, nz), z(n * K, nz), z(n), z(max(S, 1))
        mo = None if 'motion' in null else z(n, K, D)
        gt = None if 'gt' in null else z(n, D)
        sp = None if 'seg_ptr' in null else torch.tensor([0, n], dtype=torch.int32, device=dev)
        S1 = max(S, 1)
        o = dict(kld=_Out(dev, (n,), SENT), div=_Out(dev, (S1,), SENT), rec=_Out(dev, (S1,), SENT), best=_Out(dev, (S1,), ISENT, torch.int32),
                 es=_Out(dev, (S1,), SENT), dmu=_Out(dev, (n * K, nz), SENT), dlogvar=_Out(dev, (n * K, nz), SENT), dmotion=_Out(dev, (n, K, D), SENT),
                 ws=_Out(dev, (1 << 14,), SENT, margin=64))
        nb = capi.sampler_joint_ws(2, 3, 1) - 4 if 'short' in null else 4 << 14
        ws = None if 'ws' in null else o['ws'].v
        with pytest.raises(capi.SttodeError, match=FWD + ':'):
            capi.call(FWD, mu, lv, None, None, mo, gt, None, sp, S, n, K, nz, D, scale, ws, nb, o['kld'].v, o['div'].v, o['rec'].v, o['best'].v,
                      None if 'out' in null else o['es'].v, st)
        with pytest.raises(capi.SttodeError, match=BWD + ':'):
            capi.call(BWD, mu, lv, None, None, mo, gt, None, sp, S, g, gs, gs, gs, n, K, nz, D, scale, ws, nb, o['dmu'].v, o['dlogvar'].v,
                      None if 'out' in null else o['dmotion'].v, st)
        torch.cuda.synchronize()
        for k, v in o.items():
            assert v.untouched(), f'{label}: refused, but wrote {k}'


@pytest.mark.parametrize('shape', JR.SHAPES, ids=lambda s: JR.tag(s, 'x')[:-2])
@pytest.mark.parametrize('mk', JR.MASKS)
def test_one_agent_segments_vs_the_marginal_objective(shape, mk):
    """Every agent a segment of its own: div, rec under the yardstick against sttode_sampler_objective's (the float64 marginal
    restatement as the yardstick), best equal, and at Tf = 1 es against its es_fde."""
    capi, dev = _capi(), _gpu()
    K, nz, Tf = shape
    inp = dict(_inputs(shape, mk))
    n = min(inp['motion'].shape[0], 40)
    one = _sub(inp, shape, 0, n, np.arange(n + 1))
    one['g'] = {k: inp['g'][k][:n] if k == 'kld' else inp['g']['kld'][:n] for k in JR.TERMS}
    o = _Run(capi, dev, one, shape, 2.0, bwd=False)
    t = JR.as_torch(one, torch.float64)[:7]
    m64, m32 = SR.objective(*t, 2.0), SR.objective(*JR.as_torch(one, torch.float32)[:7], 2.0)
    st = capi.stream_ptr()
    q = {k: _Out(dev, (n,)) for k in ('kld', 'div', 'rec', 'es_ade', 'es_fde')}
    qb = _Out(dev, (n,), ISENT, torch.int32)
    capi.call('sttode_sampler_objective', *[_dev(dev, one[k]) for k in LAT], _dev(dev, one['motion']), _dev(dev, one['gt']), _dev(dev, one['mask']),
              n, K, nz, 2 * Tf, 2.0, q['kld'].v, q['div'].v, q['rec'].v, qb.v, q['es_ade'].v, q['es_fde'].v, st)
    torch.cuda.synchronize()
    worst = max(_close(o['div'], m64['div'], m32['div'], f'one-agent div {JR.tag(shape, mk)}'),
                _close(o['rec'], m64['rec'], m32['rec'], f'one-agent rec {JR.tag(shape, mk)}'),
                _close(o['div'], q['div'].v, m32['div'], f'one-agent div vs the marginal kernel {JR.tag(shape, mk)}'),
                _close(o['rec'], q['rec'].v, m32['rec'], f'one-agent rec vs the marginal kernel {JR.tag(shape, mk)}'))
    assert torch.equal(o['kld'], q['kld'].v)
    # (a tie of an agent's own minimum -- the tie segment's agents, an agent masked entirely -- resolves to the lowest index in both)
    assert torch.equal(o['best'], qb.v), (o['best'].tolist(), qb.v.tolist())
    if Tf == 1:
        worst = max(worst, _close(o['es'], m64['es_fde'], m32['es_fde'], f'one-agent es vs es_fde {JR.tag(shape, mk)}'))
    _worst(f'sampler joint one-agent segments {JR.tag(shape, mk)}', worst)


def _eth(dev):
    from test_sampler_objective_gpu import _eth as eth
    return eth(dev)


def _grads(smp):
    out = {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in smp.named_parameters()}
    smp.zero_grad(set_to_none=True)
    return out


def test_compute_sampler_loss_joint_is_the_sum_of_the_stand_alone_terms():
    """joint=True, recon=True, energy_weight=w: total == kld + diverse + recon + energy, each part what diversity_loss_joint /
    recon_loss_joint / energy_loss_joint / the marginal KL give on their own; seg_ptr None is one segment; a CSR as list, array, host and
    device tensor gives equal bits; the stand-alone terms are differentiable."""
    from sttode_amd import samplerloss
    dev = _gpu()
    g, smp, forward, fut, mask, n = _eth(dev)
    a, cfg = smp.args, {'weight': 3, 'scale': 2}
    dec, sd, vd, _ = forward()
    tot0, ld0, _ = samplerloss.compute_sampler_loss(a, fut, dec, 1, mask, vd, sd, cfg)
    for sp in (None, [0, 2, n - 1, n]):
        tot, ld, uw = samplerloss.compute_sampler_loss(a, fut, dec, 1, mask, vd, sd, cfg, recon=True, energy_weight=0.7, joint=True, seg_ptr=sp)
        assert list(ld) == ['kld', 'diverse', 'recon', 'energy'] and list(uw) == list(ld)
        spx = [0, n] if sp is None else sp
        with torch.no_grad():
            dv, dv_uw = samplerloss.diversity_loss_joint(dec, spx, cfg['weight'], cfg['scale'])
            rc, rc_uw = samplerloss.recon_loss_joint(fut, dec, mask, spx, a.recon_weight)
            en, en_uw = samplerloss.energy_loss_joint(fut, dec, mask, spx, 0.7)
        assert torch.equal(ld['kld'].detach(), ld0['kld'].detach())
        assert torch.equal(ld['diverse'].detach(), dv) and torch.equal(ld['recon'].detach(), rc) and torch.equal(ld['energy'].detach(), en)
        assert float(dv) == float(dv_uw * 3) and float(rc) == float(rc_uw * 5.0)
        assert float(tot.detach()) == float((((ld['kld'] + ld['diverse']) + ld['recon']) + ld['energy']).detach())
        only, ld_r, _ = samplerloss.compute_sampler_loss(a, fut, dec, 1, mask, vd, sd, cfg, joint=True, seg_ptr=sp)
        assert list(ld_r) == ['kld', 'diverse', 'recon'] and ld_r['recon'] == 0
        assert float(only.detach()) == float((ld['kld'] + ld['diverse']).detach())
        # recon: sum_g rec_g / n >= the marginal mean
        with torch.no_grad():
            assert float(rc_uw) >= float(samplerloss.recon_loss(fut, dec, mask, 1.0)[1]) * (1 - 1e-6)
    sp = [0, 2, n - 1, n]
    forms = (sp, np.asarray(sp), torch.tensor(sp), torch.tensor(sp, dtype=torch.int32, device=dev))
    vals = [samplerloss.compute_sampler_loss(a, fut, dec, 1, mask, vd, sd, cfg, recon=True, energy_weight=0.7, joint=True, seg_ptr=f)[0].detach() for f in forms]
    assert all(torch.equal(vals[0], v) for v in vals[1:])
    x = dec.detach().clone().requires_grad_(True)
    total = (samplerloss.diversity_loss_joint(x, sp, 1.0, 2.0)[0] + samplerloss.recon_loss_joint(fut, x, mask, sp, 1.0)[0]
             + samplerloss.energy_loss_joint(fut, x, mask, sp, 1.0)[0])
    total.backward()
    assert bool(torch.isfinite(x.grad).all()) and bool((x.grad != 0).any())
    with pytest.raises(ValueError, match='seg_ptr'):
        samplerloss.compute_sampler_loss(a, fut, dec, 1, mask, vd, sd, cfg, joint=True, seg_ptr=[0, 3, n - 1])


def test_joint_false_is_bitwise_the_current_objective_at_the_eth_golden_case():
    """joint=False spelled out == the default == the parent's statements (spelled out here): the two-term objective and the
    sttode_sampler_objective form, values and parameter gradients, and the golden losses of tests/golden/sampler.npz."""
    from sttode_amd import samplerloss
    dev = _gpu()
    g, smp, forward, fut, mask, n = _eth(dev)
    a, cfg = smp.args, {'weight': 1, 'scale': 1}
    res = []
    for kw in (dict(), dict(joint=False)):
        dec, sd, vd, _ = forward()
        tot, ld, _ = samplerloss.compute_sampler_loss(a, fut, dec, 1, torch.ones(n, 12), vd, sd, cfg, **kw)
        tot.backward()
        res.append((tot.detach(), ld, _grads(smp)))
    np.testing.assert_allclose([float(v.detach()) for v in (res[0][0], res[0][1]['kld'], res[0][1]['diverse'])], g['eth_shared_loss'], rtol=1e-4)
    dec, sd, vd, _ = forward()
    kld_a, div_a = samplerloss._per_agent(sd, vd, dec, cfg['scale'])
    kl = (kld_a.sum() / n).clamp_min(a.kld_min_clamp) * a.kld_weight
    dv = div_a.sum() / n * cfg['weight']
    (kl + dv).backward()
    hand = _grads(smp)
    for tot, ld, gr in res:
        assert torch.equal(tot, (kl + dv).detach()) and list(ld) == ['kld', 'diverse', 'recon'] and ld['recon'] == 0
        assert all((gr[k] is None and hand[k] is None) or torch.equal(gr[k], hand[k]) for k in gr)
    # the four-term form
    res = []
    for kw in (dict(), dict(joint=False)):
        dec, sd, vd, _ = forward()
        tot, ld, _ = samplerloss.compute_sampler_loss(a, fut, dec, 1, mask, vd, sd, cfg, recon=True, energy_weight=0.7, energy_kind='fde', **kw)
        tot.backward()
        res.append((tot.detach(), _grads(smp)))
    dec, sd, vd, _ = forward()
    kld_a, div_a, rec_a, _, fde_a = samplerloss._objective(sd, vd, dec, fut, mask, cfg['scale'])
    hand_tot = (((kld_a.sum() / n).clamp_min(a.kld_min_clamp) * a.kld_weight + div_a.sum() / n * cfg['weight']) + rec_a.mean() * a.recon_weight) + fde_a.mean() * 0.7
    hand_tot.backward()
    hand = _grads(smp)
    for tot, gr in res:
        assert torch.equal(tot, hand_tot.detach())
        assert all((gr[k] is None and hand[k] is None) or torch.equal(gr[k], hand[k]) for k in gr)


def test_end_to_end_gradients_through_the_sampler():
    """Sampler.forward -> compute_sampler_loss(joint=True, recon=True, energy_weight=1) -> backward: finite gradients on every parameter
    but q_c.*, equal (under the yardstick, the hand-fed gradients as both references) to feeding the entry's own dmotion, dmu, dlogvar back
    through the sampler's graph by hand."""
    from sttode_amd import samplerloss
    capi, dev = _capi(), _gpu()
    g, smp, forward, fut, mask, n = _eth(dev)
    a, cfg = smp.args, {'weight': 1, 'scale': 1}
    K, nz, Tf = 20, 32, 12
    sp = [0, 3, n]
    dec, sd, vd, _ = forward()
    tot, ld, _ = samplerloss.compute_sampler_loss(a, fut, dec, 1, mask, vd, sd, cfg, recon=True, energy_weight=1.0, joint=True, seg_ptr=sp)
    tot.backward()
    got = _grads(smp)
    for k, v in got.items():
        assert (v is None) == k.startswith('q_c.'), k
        assert v is None or bool(torch.isfinite(v).all()), k
    dec, sd, vd, _ = forward()
    mu, lv, mo = sd.mu.detach().contiguous(), sd.logvar.detach().contiguous(), dec.detach().contiguous()
    pmu, plv = vd.mu.detach().float().contiguous(), vd.logvar.detach().float().contiguous()
    md, spd, S = mask.to(dev), torch.tensor(sp, dtype=torch.int32, device=dev), len(sp) - 1
    nb = capi.sampler_joint_ws(n, K, S)
    ws = torch.empty(nb // 8 + 1, dtype=torch.float64, device=dev)
    kld = torch.empty(n, device=dev)
    o = [torch.empty(S, device=dev) for _ in range(2)] + [torch.empty(S, dtype=torch.int32, device=dev), torch.empty(S, device=dev)]
    capi.call(FWD, mu, lv, pmu, plv, mo, fut, md, spd, S, n, K, nz, 2 * Tf, float(cfg['scale']), ws, nb, kld, *o, capi.stream_ptr())
    live = float(kld.sum() / n) > a.kld_min_clamp
    gs = [torch.full((n,), (a.kld_weight if live else 0.0) / n, device=dev), torch.full((S,), float(cfg['weight']) / S, device=dev),
          torch.full((S,), a.recon_weight / n, device=dev), torch.full((S,), 1.0 / S, device=dev)]
    dmu, dlv, dmo = torch.empty_like(mu), torch.empty_like(lv), torch.empty_like(mo)
    capi.call(BWD, mu, lv, pmu, plv, mo, fut, md, spd, S, *gs, n, K, nz, 2 * Tf, float(cfg['scale']), ws, nb, dmu, dlv, dmo, capi.stream_ptr())
    torch.autograd.backward([dec, sd.mu, sd.logvar], [dmo, dmu, dlv])
    hand = _grads(smp)
    worst = max(_close(got[k], hand[k], hand[k], f'end to end {k}') for k in got if got[k] is not None)
    _worst('sampler joint end to end', worst)


@pytest.mark.parametrize('dataset,Tp,Tf', [('eth', 8, 12), ('nba', 5, 10)])
def test_one_joint_training_epoch(dataset, Tp, Tf):
    """train_sampler_epoch(joint=True, recon=True, energy_weight=0.5) on the scene branch (one segment per step) and on the NBA branch
    (one segment per game): finite losses, the terms in the printed line, and the parameters move."""
    from sttode_amd import samplerloss, scenes
    from sttode_amd.trainer import train_sampler_epoch
    from test_sampler_fused import _model, _sampler
    net = _model(dataset, Tp, Tf)
    if dataset == 'eth':
        loader = []
        for s in (4242, 4243):
            ob, pr = scenes.eth_scene(s, n_min=9, n_max=9)
            ob, pr = torch.from_numpy(ob), torch.from_numpy(pr)
            N = ob.shape[0]
            pm = torch.ones(1, N, Tf)
            pm[0, 0, 9:] = 0
            loader.append([ob[None], pr[None], ob[None], pr[None], torch.zeros(1, N), torch.ones(1, N), torch.ones(1, N, Tp), pm, torch.tensor([[10]]), ['seq']])
    else:
        loader = [scenes.nba_batch(70 + i, 4) for i in range(2)]
    s0 = copy.deepcopy(_sampler(dataset, Tp, Tf)).train()
    before = {k: p.detach().clone() for k, p in s0.named_parameters()}
    opt = torch.optim.Adam(s0.parameters(), lr=1e-3)
    lines = []
    calls = []
    capi = _capi()
    real = capi.call
    try:
        capi.call = lambda name, *a, **k: (calls.append(name), real(name, *a, **k))[1]
        losses = train_sampler_epoch(s0.args, 0, net, s0, opt, None, loader, samplerloss.get_diversity_config(dataset), log=lines.append, max_iters=2,
                                     recon=True, energy_weight=0.5, joint=True)
    finally:
        capi.call = real
    assert len(losses) == 2 and all(np.isfinite(losses)) and len(lines) == 1 and '| recon: ' in lines[0] and '| energy: ' in lines[0], lines
    assert calls.count(FWD) == 2 and calls.count(BWD) == 2 and not any(c in ('sttode_sampler_loss', 'sttode_sampler_objective') for c in calls)
    moved = [k for k, p in s0.named_parameters() if not k.startswith('q_c.') and not torch.equal(p.detach(), before[k])]
    assert moved and all(bool(torch.isfinite(p).all()) for p in s0.parameters()), 'no parameter moved'


def test_graph_capture_and_replay_of_forward_plus_backward():
    """Forward plus backward at the training shape captured into one graph and replayed: bitwise the eager results (the entries allocate
    nothing and read nothing back)."""
    capi, dev = _capi(), _gpu()
    shape = TRAIN
    K, nz, Tf = shape
    inp = _inputs(shape, 'ragged')
    eager = _Run(capi, dev, inp, shape, 2.0)
    n, sp = inp['motion'].shape[0], inp['seg_ptr']
    S = len(sp) - 1
    lat = [_dev(dev, inp[k]) for k in LAT]
    mo, gt, mk, spd = _dev(dev, inp['motion']), _dev(dev, inp['gt']), _dev(dev, inp['mask']), _dev(dev, sp)
    gs = [_dev(dev, inp['g'][k]) for k in JR.TERMS]
    nb = capi.sampler_joint_ws(n, K, S)
    ws = torch.empty(nb // 8 + 1, dtype=torch.float64, device=dev)
    out = dict(kld=torch.empty(n, device=dev), div=torch.empty(S, device=dev), rec=torch.empty(S, device=dev),
               best=torch.empty(S, dtype=torch.int32, device=dev), es=torch.empty(S, device=dev), dmu=torch.empty(n * K, nz, device=dev),
               dlogvar=torch.empty(n * K, nz, device=dev), dmotion=torch.empty(n, K, Tf, 2, device=dev))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        st = capi.stream_ptr()
        capi.call(FWD, *lat, mo, gt, mk, spd, S, n, K, nz, 2 * Tf, 2.0, ws, nb, out['kld'], out['div'], out['rec'], out['best'], out['es'], st)
        capi.call(BWD, *lat, mo, gt, mk, spd, S, *gs, n, K, nz, 2 * Tf, 2.0, ws, nb, out['dmu'], out['dlogvar'], out['dmotion'], st)
    for _ in range(2):
        for v in out.values():
            v.fill_(-7) if v.dtype == torch.int32 else v.fill_(float('nan'))
        graph.replay()
        torch.cuda.synchronize()
        for k, v in out.items():
            assert torch.equal(v, eager[k]), f'replay differs from eager in {k}'
    del graph
