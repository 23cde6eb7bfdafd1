"""GPU tests of the scene-level (joint) best-of-K objective.  Kernel level: sttode_loss_objective_joint and
sttode_loss_diverse_joint through capi.call, every output NaN-prefilled inside sentinel margins (tests/test_train_loss_kernels_gpu.py),
against tests/joint_ref.py in float64 on the same fp32 inputs with torch's fp32 evaluation as the measure (train_ref.assert_f64_close at its
default factor); `best` / `seg_best`, the relation to the live form, independence of the segments and repeatability to the bit.  Model
level: forward() + backward() in joint mode against oracle autograd of joint_ref.oracle_joint_loss on the per-parameter float64 yardstick
of tests/test_gpu_parity.py, a CSR batch, graph replay, mode switching, the values-only path, one generic width and a short training run.

Input condition, asserted while the inputs are built (no case is skipped): the two lowest J_g(k) of every segment differ by at least 1e-4
relative, apart from the constructed bit-for-bit ties -- which sample a segment selects is never an accident of rounding."""
import functools

import numpy as np
import pytest
import torch

import joint_ref as JR
import train_ref as R

from helpers import grad_case_setup, make_args, oracle_model
from test_train_kernels_gpu import SENT, _capi, _close, _gpu, _worst
from test_train_loss_kernels_gpu import ISENT, MIN_CLIP, _dev, _Out

pytestmark = pytest.mark.gpu

# ---------------------------------------------------------------------------------------------------------------------------------------
# kernel level
# ---------------------------------------------------------------------------------------------------------------------------------------
# segment sizes 1, 2, 11, 64, 65 (a wave's share of the agents uneven), 257 (more than a workgroup's threads), ragged, as scenes of a CSR
RAGGED = (1, 64, 65, 2, 11, 257)
K1S = (2, 21, 34, 65)                       # one sample | the default | more than half a wave | the full wave
DIMS = ((2, 4), (24, 16), (80, 20))
# (segment sizes of a CSR or None, seg_len, n, K1, D, Dp, zd)
JOINT_CASES = ([(RAGGED, 0, sum(RAGGED), K1, D, Dp, 32) for K1 in K1S for D, Dp in DIMS]
               + [((1, 64, 65, 2), 0, 132, 21, 24, 16, 32), ((7,), 0, 7, 21, 24, 16, 32)]
               + [(None, 1, 7, 21, 24, 16, 32), (None, 11, 33, 21, 20, 10, 32), (None, 65, 65, 21, 24, 16, 32), (None, 257, 257, 34, 2, 4, 16),
                  (None, 2, 8, 65, 80, 20, 16), (None, 64, 128, 2, 24, 16, 32), (None, 1, 1, 2, 2, 4, 16)])
_case_id = lambda c: '%s-n%d-K1_%d-D%d-Dp%d-zd%d' % ('csr' + 'x'.join(map(str, c[0])) if c[0] else 'seg%d' % c[1], *c[2:])


def _ptr(sizes):
    return tuple(int(v) for v in np.concatenate([[0], np.cumsum(sizes)]))


def _gap_ok(J, tied=()):
    """The input condition on J [G, K] (float64): per segment the two lowest values differ by >= 1e-4 relative; for a segment in ``tied``
    the two lowest are equal to the bit and the third is that far away."""
    for g in range(J.shape[0]):
        s = np.sort(J[g])
        if g in tied:
            assert s[0] == s[1], (g, s[:3])
            s = s[1:]
        assert s.size < 2 or s[1] - s[0] >= 1e-4 * s[1], (g, s[:3])


def _references(arrs, csr, seg_len, K1, n, D, Dp, tied=()):
    t32 = [torch.from_numpy(v) for v in arrs]
    sm, sr = 2.0 / D, 2.0 / Dp
    r64 = JR.objective_joint(*[v.double() for v in t32], csr, seg_len, K1, sm, sr, float(n), MIN_CLIP)
    r32 = JR.objective_joint(*t32, csr, seg_len, K1, sm, sr, float(n), MIN_CLIP)
    _gap_ok(r64['J'].numpy(), tied)
    kls = R.scene_kl(t32[4].double(), csr, float(n)).numpy()
    assert (kls >= 1.1 * MIN_CLIP).all(), kls                          # every scene's KL clear of the clamp
    return r64, r32, sm, sr


@functools.lru_cache(maxsize=None)
def _joint_inputs(case):
    sizes, seg_len, n, K1, D, Dp, zd = case
    csr = _ptr(sizes) if sizes else None
    seed = 5000 + 97 * n + 13 * K1 + D
    for _ in range(8):                    # the seed rule, moved on while a segment's two lowest sums lie within 1e-4 (under 1 % of draws)
        rng = np.random.default_rng(seed)
        f = lambda *s: rng.standard_normal(s).astype(np.float32)
        arrs = (f(n, K1, D), f(n, K1, Dp), f(n, D), f(n, Dp), np.float32(0.6) * f(n, 2 * zd))
        d2 = ((arrs[2].astype(np.float64)[:, None] - arrs[0].astype(np.float64)[:, 1:]) ** 2).sum(-1)
        s = np.sort(np.stack([d2[a:b].sum(0) for a, b in JR.segments_of(n, csr, seg_len)]), axis=1)
        if K1 == 2 or (s[:, 1] - s[:, 0] >= 2e-4 * s[:, 1]).all():
            break
        seed += 1000003
    r64, r32, sm, sr = _references(arrs, csr, seg_len, K1, n, D, Dp)
    assert torch.equal(r64['best'], r32['best'])
    return dict(np=arrs, csr=csr, seg_len=seg_len, dims=(n, K1, D, Dp, zd), r64=r64, r32=r32, sm=sm, sr=sr)


def _call(capi, dev, arrs, csr, seg_len, dims, entry='joint', with_seg_best=True):
    """One sttode_loss_objective_joint (or _live) call with the documented minimum of scratch -> dict of _Out."""
    n, K1, D, Dp, zd = dims
    P, Rc, F_, PA, Q = (_dev(dev, v) for v in arrs)
    S = len(csr) - 1 if csr is not None else 0
    G = S if csr is not None else n // seg_len
    sp = _dev(dev, np.asarray(csr, np.int32)) if csr is not None else None
    ag = _dev(dev, R.scene_of(csr, n).astype(np.int32)) if csr is not None else None
    need = 3 * n + (S if csr is not None else n)
    o = dict(out=_Out(dev, (5,)), dpred=_Out(dev, (n, 2, D)), drec=_Out(dev, (n, 2, Dp)), dqzp=_Out(dev, (n, 2 * zd)),
             best=_Out(dev, (n,), ISENT, torch.int32), seg_best=_Out(dev, (G,), ISENT, torch.int32), scratch=_Out(dev, (need,), SENT))
    head = (P, Rc, F_, PA, Q, sp, ag, S, n, K1, D, Dp, zd, 2.0 / D, 2.0 / Dp, float(n), MIN_CLIP, o['out'].v, o['dpred'].v, o['drec'].v, o['dqzp'].v,
            o['best'].v)
    tail = (o['scratch'].v, need, capi.stream_ptr())
    if entry == 'joint':
        capi.call('sttode_loss_objective_joint', *head, seg_len, o['seg_best'].v if with_seg_best else None, *tail)
    else:
        capi.call('sttode_loss_objective_live', *head, *tail)
    torch.cuda.synchronize()
    return o


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32)) if a.dtype == torch.float32 else torch.equal(a, b)


@pytest.mark.parametrize('case', JOINT_CASES, ids=_case_id)
def test_joint_objective_vs_float64(case):
    """Five values, three gradients, best and seg_best; nothing outside the outputs; a second run to the bit; seg_best optional."""
    capi, dev = _capi(), _gpu()
    inp = _joint_inputs(case)
    n, K1, D, Dp, zd = inp['dims']
    r64, r32 = inp['r64'], inp['r32']
    what = 'joint objective ' + _case_id(case)
    o = _call(capi, dev, inp['np'], inp['csr'], inp['seg_len'], inp['dims'])
    best = o['best'].v.cpu()
    assert torch.equal(best, r64['best']), f'{what}: best {best.tolist()} != {r64["best"].tolist()}'
    assert torch.equal(o['seg_best'].v.cpu(), r64['seg_best']), f'{what}: seg_best'
    worst = {}
    vals = o['out'].v.cpu()
    for i, k in enumerate(('mse', 'rec', 'kl', 'diverse', 'total')):
        worst['value ' + k] = _close(vals[i:i + 1], r64[k].reshape(1), r32[k].reshape(1), f'{what} {k}')
    ar, bl = torch.arange(n), best.long()
    two = lambda d: torch.stack([d[:, 0], d[ar, bl]], dim=1)             # the dense reference gradient's two live rows
    worst['dpred2'] = _close(o['dpred'].v, two(r64['dpred']), two(r32['dpred']), f'{what} dpred2')
    worst['drec2'] = _close(o['drec'].v, two(r64['drec']), two(r32['drec']), f'{what} drec2')
    worst['dqzp'] = _close(o['dqzp'].v, r64['dqzp'], r32['dqzp'], f'{what} dqzp')
    assert (o['drec'].v[:, 1] == 0).all()
    others = torch.ones(n, K1, dtype=torch.bool)
    others[:, 0] = False
    others[ar, bl] = False
    assert (r64['dpred'][others] == 0).all()                             # (the reference agrees that no other column carries a gradient)
    for k, v in o.items():
        assert v.margins_ok(), f'{what}: wrote outside {k}'
    again = _call(capi, dev, inp['np'], inp['csr'], inp['seg_len'], inp['dims'], with_seg_best=False)
    for k in ('out', 'dpred', 'drec', 'dqzp', 'best'):
        assert _same_bits(o[k].v, again[k].v), f'{what}: {k} differs between two runs'
    assert again['seg_best'].untouched()
    k = max(worst, key=worst.get)
    _worst(f'joint objective {_case_id(case)} (at {k})', worst[k])


@pytest.mark.parametrize('case', JOINT_CASES, ids=_case_id)
def test_joint_objective_is_the_live_form_outside_the_diverse_term(case):
    """out[0..2], dqzp and row 0 of dpred2 / drec2 bitwise the live form's; one-agent segments: every output; the joint term is never below
    the marginal one."""
    capi, dev = _capi(), _gpu()
    inp = _joint_inputs(case)
    what = 'joint vs live ' + _case_id(case)
    j = _call(capi, dev, inp['np'], inp['csr'], inp['seg_len'], inp['dims'])
    l = _call(capi, dev, inp['np'], inp['csr'], inp['seg_len'], inp['dims'], entry='live')
    assert _same_bits(j['out'].v[:3], l['out'].v[:3]) and _same_bits(j['dqzp'].v, l['dqzp'].v), what
    assert _same_bits(j['dpred'].v[:, 0], l['dpred'].v[:, 0]) and _same_bits(j['drec'].v, l['drec'].v), what
    sizes = case[0] if case[0] else (case[1],)
    if max(sizes) == 1:
        for k in ('out', 'dpred', 'best'):
            assert _same_bits(j[k].v, l[k].v), f'{what}: one-agent segments, {k}'
    else:                       # (K1 = 2: the two terms are one number summed in two orders; fp32 sums of <= 400 positive terms agree to ~1e-6)
        assert float(j['out'].v[3]) >= float(l['out'].v[3]) * (1 - 1e-5)


def test_one_agent_segments_are_the_live_form_to_the_bit():
    """... at every K1 and width, as scenes of a CSR and as seg_len = 1 (more than 256 agents: the sum kernel's stride loop)."""
    capi, dev = _capi(), _gpu()
    for K1 in K1S:
        for D, Dp in DIMS:
            for n, csr in ((300, None), (5, _ptr((1,) * 5))):
                rng = np.random.default_rng(K1 + D)
                f = lambda *s: rng.standard_normal(s).astype(np.float32)
                arrs = (f(n, K1, D), f(n, K1, Dp), f(n, D), f(n, Dp), np.float32(0.6) * f(n, 32))
                dims = (n, K1, D, Dp, 16)
                j = _call(capi, dev, arrs, csr, 0 if csr else 1, dims)
                l = _call(capi, dev, arrs, csr, 0 if csr else 1, dims, entry='live')
                for k in ('out', 'dpred', 'drec', 'dqzp', 'best'):
                    assert _same_bits(j[k].v, l[k].v), (K1, D, n, k)
                assert torch.equal(j['seg_best'].v, j['best'].v)


@pytest.mark.parametrize('case', JOINT_CASES, ids=_case_id)
@pytest.mark.parametrize('with_dpred', [True, False])
def test_stand_alone_joint_term_is_the_objectives_to_the_bit(case, with_dpred):
    capi, dev = _capi(), _gpu()
    inp = _joint_inputs(case)
    n, K1, D, Dp, zd = inp['dims']
    K, csr = K1 - 1, inp['csr']
    what = 'stand-alone joint term ' + _case_id(case)
    o = _call(capi, dev, inp['np'], csr, inp['seg_len'], inp['dims'])
    pk = _dev(dev, np.ascontiguousarray(inp['np'][0][:, 1:]))
    F_ = _dev(dev, inp['np'][2])
    sp = _dev(dev, np.asarray(csr, np.int32)) if csr is not None else None
    ag = _dev(dev, R.scene_of(csr, n).astype(np.int32)) if csr is not None else None
    val, g, best, scr = _Out(dev, (1,)), _Out(dev, (n, K, D)), _Out(dev, (n,), ISENT, torch.int32), _Out(dev, (n,), SENT)
    capi.call('sttode_loss_diverse_joint', pk, F_, sp, ag, n, K, D, inp['seg_len'], val.v, g.v if with_dpred else None,
              best.v if with_dpred else None, scr.v, capi.stream_ptr())
    torch.cuda.synchronize()
    assert _same_bits(val.v, o['out'].v[3:4]), f'{what}: {float(val.v)} != {float(o["out"].v[3])}'
    if with_dpred:
        assert torch.equal(best.v, o['best'].v)
        dense = torch.zeros(n, K, D, device=dev)
        dense[torch.arange(n), o['best'].v.long() - 1] = o['dpred'].v[:, 1]
        assert _same_bits(g.v, dense), what
    else:
        assert torch.isnan(g.v).all() and best.untouched()
    for k, v in dict(val=val, g=g, best=best, scr=scr).items():
        assert v.margins_ok(), f'{what}: wrote outside {k}'


# (segment sizes, K1, [(segment, 0-based winner among the K prior samples = lane, its bit-for-bit duplicate)]); K = 64: pairs across lane 32 in
# both orders, both above it, the two lanes next to it
TIE_CASES = [((3, 65, 2, 11, 257), 65, [(0, 5, 50), (1, 50, 5), (2, 33, 60), (3, 32, 31), (4, 63, 0)]),
             ((11, 11, 11), 21, [(0, 0, 19), (1, 19, 0), (2, 3, 4)])]


# (the equal segments also as a seg_len)
@pytest.mark.parametrize('tie_case,as_csr', [(0, True), (1, True), (1, False)])
def test_two_identical_sample_columns_across_a_segment_select_the_lower_k(tie_case, as_csr):
    sizes, K1, ties = TIE_CASES[tie_case]
    capi, dev = _capi(), _gpu()
    n, D, Dp, zd = sum(sizes), 24, 16, 32
    rng = np.random.default_rng(77 + K1)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    pred, rec, fut, past, qzp = f(n, K1, D), f(n, K1, Dp), f(n, D), f(n, Dp), np.float32(0.6) * f(n, 2 * zd)
    ptr = _ptr(sizes)
    for g, w, dup in ties:
        a, b = ptr[g], ptr[g + 1]
        pred[a:b, 1 + w] = fut[a:b] + np.float32(1e-3) * f(b - a, D)    # the winner of the whole segment: the targets plus small noise
        pred[a:b, 1 + dup] = pred[a:b, 1 + w]                           # ... and its duplicate, bit for bit
    csr, seg_len = (ptr, 0) if as_csr else (None, sizes[0])
    arrs = (pred, rec, fut, past, qzp)
    r64, r32, _, _ = _references(arrs, csr, seg_len, K1, n, D, Dp, tied={g for g, _, _ in ties})
    for g, w, dup in ties:
        assert int(r64['seg_best'][g]) == 1 + min(w, dup)
    o = _call(capi, dev, arrs, csr, seg_len, (n, K1, D, Dp, zd))
    assert torch.equal(o['seg_best'].v.cpu(), r64['seg_best']) and torch.equal(o['best'].v.cpu(), r64['best'])
    _close(o['out'].v[3:4], r64['diverse'].reshape(1), r32['diverse'].reshape(1), f'tied segments {sizes} diverse')


def _segment_rows(o, a, b):
    return [o['best'].v[a:b].clone(), o['dpred'].v[a:b].clone(), o['drec'].v[a:b].clone(), o['dqzp'].v[a:b].clone()]


@pytest.mark.parametrize('nx', [11, 65])
def test_a_segments_outputs_do_not_depend_on_its_neighbours_or_its_place(nx):
    """Scene X alone, with a scene appended, and with one, two and three agents of another scene in front: X's best, gradient rows and
    dqzp rows to the bit."""
    capi, dev = _capi(), _gpu()
    K1, D, Dp, zd = 21, 24, 16, 32
    rng = np.random.default_rng(91 + nx)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    mk = lambda n: (f(n, K1, D), f(n, K1, Dp), f(n, D), f(n, Dp), np.float32(0.6) * f(n, 2 * zd))
    X, Y = mk(nx), mk(7)
    cat = lambda u, v: tuple(np.concatenate([p, q]) for p, q in zip(u, v))
    cut = lambda u, m: tuple(p[:m] for p in u)
    for arrs, sizes in ((X, (nx,)), (cat(X, Y), (nx, 7))) + tuple((cat(cut(Y, m), X), (m, nx)) for m in (1, 2, 3)):
        _references(arrs, _ptr(sizes), 0, K1, sum(sizes), D, Dp)        # (the input condition)
    base = _segment_rows(_call(capi, dev, X, _ptr((nx,)), 0, (nx, K1, D, Dp, zd)), 0, nx)
    o = _call(capi, dev, cat(X, Y), _ptr((nx, 7)), 0, (nx + 7, K1, D, Dp, zd))
    assert all(_same_bits(u, v) for u, v in zip(base, _segment_rows(o, 0, nx))), 'a scene appended'
    for m in (1, 2, 3):
        o = _call(capi, dev, cat(cut(Y, m), X), _ptr((m, nx)), 0, (m + nx, K1, D, Dp, zd))
        assert all(_same_bits(u, v) for u, v in zip(base, _segment_rows(o, m, m + nx))), f'{m} agents in front'
        assert int(o['seg_best'].v[1]) == int(base[0][0])


def test_nan_in_one_segment_leaves_the_other_segments_alone():
    capi, dev = _capi(), _gpu()
    sizes, K1, D, Dp, zd = (11, 5, 65), 21, 24, 16, 32
    n, ptr = sum(sizes), _ptr(sizes)
    inp = _joint_inputs((sizes, 0, n, K1, D, Dp, zd))
    clean = _call(capi, dev, inp['np'], ptr, 0, inp['dims'])
    pred = inp['np'][0].copy()
    pred[ptr[1] + 2, 1:] = np.nan                                     # every prior sample of one agent of scene 1: all its J_g(k) are NaN
    o = _call(capi, dev, (pred,) + inp['np'][1:], ptr, 0, inp['dims'])
    for a, b in ((ptr[0], ptr[1]), (ptr[2], ptr[3])):
        assert all(_same_bits(u, v) for u, v in zip(_segment_rows(clean, a, b), _segment_rows(o, a, b)))
    assert torch.equal(o['seg_best'].v[[0, 2]], clean['seg_best'].v[[0, 2]])
    assert _same_bits(o['out'].v[:3], clean['out'].v[:3])
    assert torch.isnan(o['out'].v[3]) and torch.isnan(o['out'].v[4])
    bad = o['best'].v[ptr[1]:ptr[2]].cpu()
    assert ((bad >= 1) & (bad <= K1 - 1)).all() and (bad == bad[0]).all()
    for k, v in o.items():
        assert v.margins_ok(), k


def test_joint_refusals_write_nothing():
    capi, dev = _capi(), _gpu()
    n, K1, D, Dp, zd = 12, 21, 24, 16, 32
    z = lambda *s: torch.zeros(*s, device=dev)
    P, Rc, F_, PA, Q = z(n, K1, D), z(n, K1, Dp), z(n, D), z(n, Dp), z(n, 2 * zd)
    sp, ag = _dev(dev, np.array([0, 5, 12], np.int32)), _dev(dev, np.repeat([0, 1], [5, 7]).astype(np.int32))
    base = dict(sp=None, ag=None, S=0, K1=K1, seg_len=n, best=True, scratch_floats=4 * n)
    for label, over in (('K1 = 1', dict(K1=1)), ('K1 = 66', dict(K1=66)), ('seg_len 5 of 12', dict(seg_len=5)), ('seg_len 0', dict(seg_len=0)),
                        ('seg_len with a CSR', dict(sp=sp, ag=ag, S=2, seg_len=6)), ('null best', dict(best=False)),
                        ('scratch one float short', dict(scratch_floats=4 * n - 1)),
                        ('scratch one float short, CSR', dict(sp=sp, ag=ag, S=2, seg_len=0, scratch_floats=3 * n + 2 - 1))):
        a = dict(base, **over)
        o = dict(out=_Out(dev, (5,), SENT), dpred=_Out(dev, (n, 2, D), SENT), drec=_Out(dev, (n, 2, Dp), SENT), dqzp=_Out(dev, (n, 2 * zd), SENT),
                 best=_Out(dev, (n,), ISENT, torch.int32), seg_best=_Out(dev, (n,), ISENT, torch.int32), scratch=_Out(dev, (4 * n,), SENT))
        with pytest.raises(capi.SttodeError, match='sttode_loss_objective_joint'):
            capi.call('sttode_loss_objective_joint', P, Rc, F_, PA, Q, a['sp'], a['ag'], a['S'], n, a['K1'], D, Dp, zd, 0.1, 0.1, float(n), MIN_CLIP,
                      o['out'].v, o['dpred'].v, o['drec'].v, o['dqzp'].v, o['best'].v if a['best'] else None, a['seg_len'], o['seg_best'].v,
                      o['scratch'].v, a['scratch_floats'], capi.stream_ptr())
        torch.cuda.synchronize()
        for k, v in o.items():
            assert v.untouched(), f'{label}: refused, but wrote {k}'


# ---------------------------------------------------------------------------------------------------------------------------------------
# model level
# ---------------------------------------------------------------------------------------------------------------------------------------
def _fresh_model(dataset='eth', Tp=8, Tf=12, mode='joint'):
    from sttode_amd import STTODENet
    from sttode_amd.weights import make_weights, to_torch_state_dict
    m = STTODENet(make_args(dataset, Tp, Tf), _gpu()).eval()
    m.load_state_dict(to_torch_state_dict(make_weights(1234, past_length=Tp, future_length=Tf)), strict=True)
    m.diverse_mode = mode
    return m


def _grads_of(m):
    return {k: (p.grad.detach().cpu().clone() if p.grad is not None else None) for k, p in m.named_parameters()}


def _step(m, feed, eps):
    m.zero_grad()
    feed(m)
    out = m.forward(*eps)
    out[0].backward()
    return _grads_of(m), [float(out[0].detach())] + list(out[1:])


def _oracle_joint(ref, feed, eps, double):
    """Gradients (name -> tensor or None) and the five values of joint_ref.oracle_joint_loss on ``ref`` (an fp32 STTODENetRef; ``double``:
    a float64 copy of it), segments: the one scene, or the NBA games."""
    from oracle.sttode_ref import STTODENetRef
    m = ref
    if double:
        m = STTODENetRef(ref.args).eval()
        m.load_state_dict(ref.state_dict(), strict=True)
        m = m.double()
    m.zero_grad()
    prev = torch.get_default_dtype()
    try:
        torch.set_default_dtype(torch.float64 if double else torch.float32)
        feed(m)
        if double:
            for attr in ('inputs', 'inputs_for_posterior', 'past_traj', 'future_traj', 'cur_location', 'scene_orig'):
                if isinstance(getattr(m, attr, None), torch.Tensor):
                    setattr(m, attr, getattr(m, attr).double())
        e = [torch.as_tensor(v).double() if double else torch.as_tensor(v) for v in eps]
        n = m.past_traj.shape[0]
        B, N = (m.batch_size, m.agent_num) if m.args.dataset == 'nba' else (1, n)
        vals = JR.oracle_joint_loss(m, *e, [(b * N, b * N + N) for b in range(B)])
        vals[0].backward()
    finally:
        torch.set_default_dtype(prev)
    grads = {k: (p.grad.clone() if p.grad is not None else None) for k, p in m.named_parameters()}
    m.zero_grad()
    return grads, [float(v.detach()) for v in vals]


@pytest.mark.parametrize('tag,dataset,Tp,Tf', [('eth', 'eth', 8, 12), ('nba', 'nba', 5, 10)])
def test_joint_training_step_gradients_vs_oracle(golden, tag, dataset, Tp, Tf):
    """forward() in joint mode + backward() on the inputs and noises of tests/golden/forward_grads.npz (eth: one scene; nba: B x 11): the
    values within 1e-4, every parameter gradient on the per-parameter float64 yardstick (factor 2, floor 1e-4)."""
    from test_gpu_parity import _grad_yardstick
    g = golden('forward_grads')
    m = _fresh_model(dataset, Tp, Tf)
    feed = lambda mm: grad_case_setup(g, tag, mm)
    eps = list(feed(m))
    grads, losses = _step(m, feed, eps)
    ref = oracle_model(dataset, Tp, Tf)
    g64, l64 = _oracle_joint(ref, feed, eps, True)
    g32, l32 = _oracle_joint(ref, feed, eps, False)
    print(f'[joint step {tag}] hip {losses} f64 {l64} marginal (golden) {g[tag + "_losses"].tolist()}')
    np.testing.assert_allclose(losses, l64, rtol=1e-4)
    np.testing.assert_allclose(losses, l32, rtol=1e-4)
    np.testing.assert_allclose(losses[1:4], g[f'{tag}_losses'][1:4], rtol=1e-4)     # the other three terms are the marginal step's
    assert losses[4] >= float(g[f'{tag}_losses'][4]) * (1 - 1e-4)
    _grad_yardstick(grads, g64, g32, f'joint training step {tag}')


def _three_scenes():
    from sttode_amd import scenes
    sizes = (5, 9, 3)
    rng = np.random.default_rng(45)
    sc = [scenes.eth_scene(670000 + i, n_min=n, n_max=n) for i, n in enumerate(sizes)]
    eps = [[rng.standard_normal(s).astype(np.float32) for s in ((n, 32), (n, 32), (n * 20, 32))] for n in sizes]
    return sizes, sc, eps


def test_joint_training_step_on_a_csr_batch_vs_oracle_per_scene():
    """set_scene_batch over three scenes in joint mode: values and gradients against the oracle's per-scene joint steps accumulated."""
    from test_gpu_parity import _grad_yardstick
    sizes, sc, eps = _three_scenes()
    ref = oracle_model('eth', 8, 12)
    acc = {}
    for dbl in (True, False):
        gsum, lsum = None, np.zeros(5)
        for (o, p), e in zip(sc, eps):
            gr, ls = _oracle_joint(ref, lambda mm: mm.set_data(None, torch.from_numpy(o), torch.from_numpy(p)), e, dbl)
            lsum += np.array(ls)
            gsum = gr if gsum is None else {k: (None if v is None else v + gr[k]) for k, v in gsum.items()}
        acc[dbl] = (gsum, lsum)
    m = _fresh_model()
    past = np.concatenate([o.transpose(0, 2, 1) for o, _ in sc])
    fut = np.concatenate([p.transpose(0, 2, 1) for _, p in sc])
    ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    cat = [torch.from_numpy(np.concatenate([e[i] for e in eps])) for i in range(3)]
    feed = lambda mm: mm.set_scene_batch(torch.from_numpy(past), torch.from_numpy(fut), torch.from_numpy(ptr))
    grads, losses = _step(m, feed, cat)
    np.testing.assert_allclose(losses, acc[True][1], rtol=1e-4)
    _grad_yardstick(grads, acc[True][0], acc[False][0], 'joint training step csr batch')
    with torch.no_grad():                                               # the values-only path on the batched joint objective
        feed(m)
        v = m.forward(*cat)
    np.testing.assert_allclose([float(v[0])] + list(v[1:]), losses, rtol=1e-4)


def _close_grads(got, ref, what):
    """The standard of the replay tests of the marginal step (test_replayed_steps_gradients_rotate_and_accumulate_correctly)."""
    for k, r in ref.items():
        if r is None:
            assert got[k] is None, k
            continue
        assert torch.allclose(got[k], r, rtol=1e-6, atol=1e-7 * float(r.abs().max())), f'{what}: {k}'


def test_joint_step_replayed_from_a_graph_equals_the_eager_step(golden):
    g = golden('forward_grads')
    for tag, dataset, Tp, Tf in (('eth', 'eth', 8, 12), ('nba', 'nba', 5, 10)):
        m = _fresh_model(dataset, Tp, Tf)
        eps = list(grad_case_setup(g, tag, m))
        feed = lambda mm: grad_case_setup(g, tag, mm)
        m.train_graphs = False
        eager, le = _step(m, feed, eps)
        m.train_graphs = True
        for _ in range(3):                                             # eager -> capture -> replay
            got, lg = _step(m, feed, eps)
        assert any('diverse_joint' in k for k in m._graphs), 'the step was not captured under the joint key'
        np.testing.assert_allclose(lg, le, rtol=1e-6)
        _close_grads(got, eager, f'joint replay {tag}')


def test_switching_modes_between_steps_reproduces_fresh_models(golden):
    """marginal -> joint -> marginal -> joint on ONE model (the second visit of each mode replays that mode's graph): every step's values
    and gradients are those of a fresh model in that mode."""
    g = golden('forward_grads')
    fresh = {}
    for mode in ('marginal', 'joint'):
        f = _fresh_model('nba', 5, 10, mode)
        fresh[mode] = _step(f, lambda mm: grad_case_setup(g, 'nba', mm), list(grad_case_setup(g, 'nba', f)))
    assert fresh['joint'][1][4] > fresh['marginal'][1][4] * (1 + 1e-3)  # (the two objectives differ on this batch)
    m = _fresh_model('nba', 5, 10, 'marginal')
    eps = list(grad_case_setup(g, 'nba', m))
    for i, mode in enumerate(('marginal', 'joint', 'marginal', 'joint', 'marginal', 'joint')):
        m.diverse_mode = mode
        got, ls = _step(m, lambda mm: grad_case_setup(g, 'nba', mm), eps)
        np.testing.assert_allclose(ls, fresh[mode][1], rtol=1e-6, err_msg=f'step {i} ({mode})')
        _close_grads(got, fresh[mode][0], f'step {i} ({mode})')
    assert len(m._graphs) == 2
    m.diverse_mode = 'neither'
    with pytest.raises(ValueError, match='diverse_mode'):
        m.forward(*eps)


def test_joint_values_only_path_equals_the_autograd_path(golden):
    g = golden('forward_grads')
    for tag, dataset, Tp, Tf in (('eth', 'eth', 8, 12), ('nba', 'nba', 5, 10)):
        m = _fresh_model(dataset, Tp, Tf)
        eps = list(grad_case_setup(g, tag, m))
        out = m.forward(*eps)
        want = [float(out[0].detach())] + list(out[1:])
        with torch.no_grad():
            grad_case_setup(g, tag, m)
            v = m.forward(*eps)
        np.testing.assert_allclose([float(v[0])] + list(v[1:]), want, rtol=1e-4)
        m.diverse_mode = 'marginal'
        with torch.no_grad():
            grad_case_setup(g, tag, m)
            v = m.forward(*eps)
        np.testing.assert_allclose([float(v[0])] + list(v[1:]), g[f'{tag}_losses'], rtol=1e-4)


def test_joint_step_at_a_generic_width():
    """hidden_dim 32 (the generic form runs the same Engine): a joint step's values against the oracle, finite gradients for every parameter
    the oracle gives one."""
    from test_gpu_parity import _dims_model, _dims_set
    from test_oracle_golden import _dims_set_data, _oracle_for
    for dataset in ('eth', 'nba'):
        m, a, inputs, z, (eq, ep, e20) = _dims_model('hd32', dataset)
        assert m._generic
        m.diverse_mode = 'joint'
        eps = [torch.from_numpy(v) for v in (eq, ep, e20)]
        grads, losses = _step(m, lambda mm: _dims_set(mm, dataset, inputs), eps)
        og, ol = _oracle_joint(_oracle_for(a), lambda mm: _dims_set_data(mm, dataset, inputs), eps, False)
        np.testing.assert_allclose(losses, ol, rtol=1e-4)
        m.diverse_mode = 'marginal'
        _, lm = _step(m, lambda mm: _dims_set(mm, dataset, inputs), eps)
        assert losses[4] >= lm[4] * (1 - 1e-5) and np.allclose(losses[1:4], lm[1:4], rtol=1e-5)
        for k, r in og.items():
            if r is not None:
                assert grads[k] is not None and bool(torch.isfinite(grads[k]).all()), k
        assert sum(r is not None for r in og.values()) > 80


def test_twenty_adam_steps_in_joint_mode_reduce_the_joint_term(golden):
    """20 Adam steps (lr 1e-3) on one fixed NBA batch with fixed noises, in joint and in marginal mode from the same initial weights: the
    joint-mode run ends with its joint term below the value at step 0.  Both curves are printed and written beside the gradient tables
    (profiles/joint_objective/record.txt is a copy)."""
    from test_gpu_parity import _dump_grad_table
    g = golden('forward_grads')
    curves = {}
    for mode in ('joint', 'marginal'):
        m = _fresh_model('nba', 5, 10, mode)
        eps = list(grad_case_setup(g, 'nba', m))
        opt = torch.optim.Adam(m.parameters(), lr=1e-3)
        rows = []
        for step in range(21):                                         # 20 updates; row i = the objective before update i
            m.zero_grad()
            grad_case_setup(g, 'nba', m)
            out = m.forward(*eps)
            rows.append([float(out[0].detach())] + list(out[1:]))
            if step < 20:
                out[0].backward()
                opt.step()
        curves[mode] = np.array(rows)
    text = ['# 20 Adam steps (lr 1e-3), one fixed NBA batch (tests/golden/forward_grads.npz), fixed noises, same initial weights',
            '# step | joint mode: total mse recover kl diverse_joint | marginal mode: total mse recover kl diverse_marginal']
    for i in range(21):
        text.append('%2d | %s | %s' % (i, ' '.join('%.6f' % v for v in curves['joint'][i]), ' '.join('%.6f' % v for v in curves['marginal'][i])))
    print('\n'.join(text))
    _dump_grad_table('joint_objective_record', None, text='\n'.join(text) + '\n')
    assert np.isfinite(curves['joint']).all() and np.isfinite(curves['marginal']).all()
    assert curves['joint'][20, 4] < curves['joint'][0, 4], (curves['joint'][0], curves['joint'][20])
