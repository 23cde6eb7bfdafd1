"""GPU tests of global-norm gradient clipping and the non-finite guard in the one-launch Adam (csrc/train_optim.hip, sttode_amd/optim.py):
the norm against float64, the guarded step bit for bit against the plain one when nothing clips, the clipped step and the step after a
skipped one against a float64 yardstick, the stand-alone clip_grad_norm_, and a training loop against torch's clip + fused Adam.

Shapes: one element, fewer than four, an odd length, a matrix, one short of / exactly / one over a 1024-element chunk, several chunks.
Gradients arrive as separate tensors, or as views of one flat buffer at offsets that are no multiple of four floats (the scalar path)."""
import math

import numpy as np
import pytest
import torch

from helpers import make_args

pytestmark = pytest.mark.gpu

SHAPES = [(1,), (3,), (37,), (5, 3), (1023,), (1024,), (1025,), (2500,)]
MODES = ('separate', 'flat')
B1, B2, EPS = 0.9, 0.999, 1e-8


def _gpu():
    return torch.device('cuda:0')


def _params(shapes=SHAPES, seed=41):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(s, generator=g).to(_gpu())) for s in shapes]


def _clones(ps, dtype=torch.float32):
    return [torch.nn.Parameter(p.detach().clone().to(dtype)) for p in ps]


def _grads(shapes=SHAPES, seed=42, steps=4):
    g = torch.Generator().manual_seed(seed)
    return [[torch.randn(s, generator=g) for s in shapes] for _ in range(steps)]


def _set_grads(ps, grads, mode):
    """separate: one tensor each.  flat: views of ONE buffer, every offset NOT a multiple of 4 floats."""
    if mode == 'separate':
        for p, g in zip(ps, grads):
            p.grad = g.to(p.device, p.dtype)
        return
    offs, off = [], 1
    for g in grads:
        while off % 4 == 0:
            off += 1
        offs.append(off)
        off += g.numel()
    flat = torch.zeros(off + 4, dtype=ps[0].dtype, device=ps[0].device)
    assert flat.data_ptr() % 16 == 0
    for p, g, o in zip(ps, grads, offs):
        flat[o: o + g.numel()] = g.flatten().to(p.device, p.dtype)
        p.grad = flat[o: o + g.numel()].view(g.shape)


def _norm64(grads):
    return math.sqrt(sum(float((g.double() ** 2).sum()) for g in grads))


class Yardstick:
    """torch's clip formula and Adam's update written out in float64 on double copies of the tensors."""

    def __init__(self, ps, lr):
        self.p = [p.detach().double().cpu() for p in ps]
        self.m = [torch.zeros_like(p) for p in self.p]
        self.v = [torch.zeros_like(p) for p in self.p]
        self.t, self.lr = 0, lr

    def step(self, grads, max_norm, norm=None):
        """norm: the global norm when `grads` are only some of the gradients it is taken over."""
        self.t += 1
        coef = min(1.0, max_norm / ((_norm64(grads) if norm is None else norm) + 1e-6)) if max_norm is not None else 1.0
        for p, m, v, g in zip(self.p, self.m, self.v, grads):
            g = g.double() * coef
            m += (1 - B1) * (g - m)
            v.mul_(B2).add_((1 - B2) * g * g)
            p -= self.lr / (1 - B1 ** self.t) * m / (v.sqrt() / math.sqrt(1 - B2 ** self.t) + EPS)


def _errors(opt, ps, yard):
    """max |x - f64| over all tensors, for the parameters and both moments."""
    out = {}
    for k, ref in (('p', yard.p), ('exp_avg', yard.m), ('exp_avg_sq', yard.v)):
        got = [p.detach() if k == 'p' else opt.state[p][k] for p in ps]
        out[k] = max(float((x.double().cpu() - r).abs().max()) for x, r in zip(got, ref))
    return out


ATOL = {'p': 2e-7, 'exp_avg': 1e-7, 'exp_avg_sq': 1e-7}       # the Adam drop-in's own figures against torch (parameters / moments)


def _assert_tracks_yardstick(oa, ps_a, ob, ps_b, yard, what):
    ea, eb = _errors(oa, ps_a, yard), _errors(ob, ps_b, yard)
    for k in ea:
        print(f'{what} {k}: max|hip - f64| = {ea[k]:.3e}, max|torch32 - f64| = {eb[k]:.3e}')
        assert ea[k] <= 4 * eb[k] + ATOL[k], f'{what} {k}: max|hip - f64| = {ea[k]:.3e}, max|torch32 - f64| = {eb[k]:.3e}'


def _state_equal(oa, ps_a, ob, ps_b):
    return all(torch.equal(pa, pb) and torch.equal(oa.state[pa]['exp_avg'], ob.state[pb]['exp_avg'])
               and torch.equal(oa.state[pa]['exp_avg_sq'], ob.state[pb]['exp_avg_sq']) for pa, pb in zip(ps_a, ps_b))


# 1. the norm --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', MODES)
def test_norm_matches_float64_and_repeats_bitwise(mode):
    """rtol 2e-6: every term is non-negative, so a chunk's fp32 tree sum is off by at most ~12 roundings x 2^-24 = 7e-7 relative; the finish
    is in double, the square root halves the error and the rounding to float adds 6e-8: under 5e-7, times 4."""
    from sttode_amd import optim
    grads = _grads(steps=1)[0]
    ref = _norm64(grads)
    ps = _params()
    opt = optim.Adam(ps, lr=1e-3, max_grad_norm=1e30)
    seen = []
    for _ in range(2):
        _set_grads(ps, grads, mode)
        opt.step()
        seen.append(opt.last_grad_norm.clone())
        assert opt.last_grad_norm.dim() == 0 and opt.last_grad_norm.device.type == 'cuda'
    _set_grads(ps, grads, mode)
    for _ in range(2):
        seen.append(optim.clip_grad_norm_(ps, 1e30))
    for x in seen:
        assert abs(float(x) - ref) <= 2e-6 * ref, (float(x), ref)
        assert torch.equal(x, seen[0])


def _model_params():
    from sttode_amd import STTODENet
    from sttode_amd.weights import make_weights, to_torch_state_dict
    m = STTODENet(make_args('eth', 8, 12), _gpu()).eval()
    m.load_state_dict(to_torch_state_dict(make_weights(1234)), strict=True)
    return [p for p in m.parameters()]


def test_model_parameters_norm_and_bitwise_step():
    """Every parameter of the real model with random gradients: the norm against float64, and the guarded step with nothing to clip against the
    plain step, bit for bit."""
    from sttode_amd import optim
    base = _model_params()
    assert len(base) >= 88                                       # (88 of them get a gradient in a training step)
    shapes = [tuple(p.shape) for p in base]
    grads = _grads(shapes, seed=43, steps=2)
    ps_a, ps_b = _clones(base), _clones(base)
    oa, ob = optim.Adam(ps_a, lr=1e-3, max_grad_norm=1e30, skip_nonfinite=True), optim.Adam(ps_b, lr=1e-3)
    for gs in grads:
        _set_grads(ps_a, gs, 'separate')
        _set_grads(ps_b, gs, 'separate')
        oa.step()
        ob.step()
        ref = _norm64(gs)
        assert abs(float(oa.last_grad_norm) - ref) <= 2e-6 * ref
        assert abs(float(optim.clip_grad_norm_(ps_b, 1e30)) - ref) <= 2e-6 * ref
    assert _state_equal(oa, ps_a, ob, ps_b)
    assert oa.skipped_steps == 0


# 2. no clipping active: bitwise --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', MODES)
def test_guarded_step_with_nothing_to_clip_is_the_plain_step_bitwise(mode):
    from sttode_amd.optim import Adam
    base = _params()
    ps_a, ps_b = _clones(base), _clones(base)
    oa, ob = Adam(ps_a, lr=3e-3, max_grad_norm=1e30, skip_nonfinite=True), Adam(ps_b, lr=3e-3)
    sa = torch.optim.lr_scheduler.StepLR(oa, step_size=2, gamma=0.5)
    sb = torch.optim.lr_scheduler.StepLR(ob, step_size=2, gamma=0.5)
    for gs in _grads(steps=4):
        _set_grads(ps_a, gs, mode)
        _set_grads(ps_b, gs, mode)
        oa.step(); ob.step(); sa.step(); sb.step()
    assert oa.param_groups[0]['lr'] == 3e-3 * 0.25
    assert _state_equal(oa, ps_a, ob, ps_b)
    assert oa.skipped_steps == 0 and oa.steps_taken == ob.steps_taken == {0: 4}


# 3. clipping active --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', MODES)
def test_clipped_steps_track_the_float64_yardstick(mode):
    from sttode_amd.optim import Adam
    base, grads = _params(), _grads(steps=4)
    c = 0.1 * _norm64(grads[0])
    ps_a, ps_b = _clones(base), _clones(base)
    oa, ob, yard = Adam(ps_a, lr=1e-2, max_grad_norm=c), torch.optim.Adam(ps_b, lr=1e-2, foreach=False), Yardstick(base, 1e-2)
    for gs in grads:
        _set_grads(ps_a, gs, mode)
        _set_grads(ps_b, gs, mode)
        oa.step()
        torch.nn.utils.clip_grad_norm_(ps_b, c)
        ob.step()
        yard.step(gs, c)
        assert abs(float(oa.last_grad_norm) - _norm64(gs)) <= 2e-6 * _norm64(gs)
    _assert_tracks_yardstick(oa, ps_a, ob, ps_b, yard, 'clipped, ' + mode)
    assert all(float(st['step']) == 4 for st in oa.state_dict()['state'].values())


def test_two_param_groups_share_one_norm():
    """torch's clip is over all parameters: with two groups (their own lr) the partial sums of both go into one norm."""
    from sttode_amd.optim import Adam
    base, grads = _params(), _grads(steps=3)
    c = 0.1 * _norm64(grads[0])
    ps_a, ps_b = _clones(base), _clones(base)

    def groups(ps):
        return [{'params': ps[:3], 'lr': 1e-2}, {'params': ps[3:], 'lr': 1e-3}]
    oa, ob = Adam(groups(ps_a), max_grad_norm=c), torch.optim.Adam(groups(ps_b), foreach=False)
    ya, yb = Yardstick(base[:3], 1e-2), Yardstick(base[3:], 1e-3)
    for gs in grads:
        _set_grads(ps_a, gs, 'separate')
        _set_grads(ps_b, gs, 'separate')
        oa.step()
        torch.nn.utils.clip_grad_norm_(ps_b, c)
        ob.step()
        ya.step(gs[:3], c, norm=_norm64(gs))
        yb.step(gs[3:], c, norm=_norm64(gs))
        assert abs(float(oa.last_grad_norm) - _norm64(gs)) <= 2e-6 * _norm64(gs)
    _assert_tracks_yardstick(oa, ps_a[:3], ob, ps_b[:3], ya, 'two groups, first')
    _assert_tracks_yardstick(oa, ps_a[3:], ob, ps_b[3:], yb, 'two groups, second')


# 4. the guard --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('bad', [((1025,), 1024, math.nan), ((3,), 0, math.inf)])
def test_nonfinite_step_is_skipped_and_does_not_count(bad, mode):
    from sttode_amd.optim import Adam
    shape, index, value = bad
    base, grads = _params(), _grads(steps=3)
    poisoned = [g.clone() for g in grads[1]]
    poisoned[SHAPES.index(shape)].view(-1)[index] = value
    c = 0.1 * _norm64(grads[0])
    ps_a, ps_b = _clones(base), _clones(base)
    oa = Adam(ps_a, lr=1e-2, max_grad_norm=c, skip_nonfinite=True)
    ob, yard = torch.optim.Adam(ps_b, lr=1e-2, foreach=False), Yardstick(base, 1e-2)

    def finite_step(gs):
        _set_grads(ps_a, gs, mode)
        _set_grads(ps_b, gs, mode)
        oa.step()
        torch.nn.utils.clip_grad_norm_(ps_b, c)
        ob.step()
        yard.step(gs, c)
    finite_step(grads[0])
    before = [(p.detach().clone(), oa.state[p]['exp_avg'].clone(), oa.state[p]['exp_avg_sq'].clone()) for p in ps_a]
    _set_grads(ps_a, poisoned, mode)
    oa.step()
    assert not math.isfinite(float(oa.last_grad_norm))
    for p, (p0, m0, v0) in zip(ps_a, before):                    # ALL tensors are what they were
        assert torch.equal(p.detach(), p0) and torch.equal(oa.state[p]['exp_avg'], m0) and torch.equal(oa.state[p]['exp_avg_sq'], v0)
    assert oa.skipped_steps == 1
    finite_step(grads[2])                                         # t = applied = 2, not 3
    _assert_tracks_yardstick(oa, ps_a, ob, ps_b, yard, 'after a skipped step, ' + mode)
    assert all(float(st['step']) == 2 for st in oa.state_dict()['state'].values())
    assert oa.skipped_steps == 1 and oa.steps_taken == {0: 2}
    finite_step(grads[1])                                         # and on from the folded count: t = 3
    _assert_tracks_yardstick(oa, ps_a, ob, ps_b, yard, 'second step after a skipped step, ' + mode)
    assert all(float(st['step']) == 3 for st in oa.state_dict()['state'].values()) and oa.skipped_steps == 1


def test_default_path_lets_a_nan_gradient_through_as_before():
    from sttode_amd.optim import Adam
    ps, grads = _params(), _grads(steps=1)[0]
    grads[SHAPES.index((1025,))][1024] = math.nan
    opt = Adam(ps, lr=1e-2)
    _set_grads(ps, grads, 'separate')
    opt.step()
    big = ps[SHAPES.index((1025,))]
    assert math.isnan(float(big[1024])) and bool(torch.isfinite(big[:1024]).all())
    assert opt.last_grad_norm is None and opt.skipped_steps == 0 and opt._gstate is None      # nothing new was allocated


# 5. stand-alone clip_grad_norm_ --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', MODES)
def test_clip_grad_norm_scales_like_float64(mode):
    from sttode_amd import optim
    ps, grads = _params(), _grads(steps=1)[0]
    n64 = _norm64(grads)
    _set_grads(ps, grads, mode)
    kept = [p.grad.clone() for p in ps]
    r = optim.clip_grad_norm_(ps, 10 * n64)                      # above the norm: bitwise unchanged
    assert abs(float(r) - n64) <= 2e-6 * n64 and r.device.type == 'cuda'
    assert all(torch.equal(p.grad, k) for p, k in zip(ps, kept))
    r = optim.clip_grad_norm_(ps, 0.25 * n64)
    assert abs(float(r) - n64) <= 2e-6 * n64
    coef = min(1.0, 0.25 * n64 / (n64 + 1e-6))
    for p, g in zip(ps, grads):
        np.testing.assert_allclose(p.grad.double().cpu().numpy(), (g.double() * coef).numpy(), rtol=2e-6, atol=0)
    # a NaN norm: raises when asked to, else the gradients turn NaN as torch's do
    ps[SHAPES.index((1025,))].grad.view(-1)[1024] = math.nan
    with pytest.raises(RuntimeError):
        optim.clip_grad_norm_(ps, 1.0, error_if_nonfinite=True)
    assert math.isnan(float(optim.clip_grad_norm_(ps, 1.0)))
    assert all(bool(torch.isnan(p.grad).all()) for p in ps)


# 6. the training loop ------------------------------------------------------------------------------------------------------------------------
def test_training_loop_with_clipping_equals_torch_clip_and_fused_adam():
    """The loop of test_training_loop_with_hip_adam_equals_torch_fused_adam (train.py:72-95) with clipping active: Adam(max_grad_norm=c)
    against torch's clip + torch.optim.Adam(fused=True); c is half the first step's norm, read here."""
    from sttode_amd import STTODENet, scenes
    from sttode_amd.optim import Adam
    from sttode_amd.weights import make_weights, to_torch_state_dict
    dev = _gpu()
    data = [scenes.eth_scene(81000 + i, n_min=5, n_max=12) for i in range(4)]
    runs, c = {}, None
    for kind in ('plain', 'hip', 'torch'):
        m = STTODENet(make_args('eth', 8, 12), dev).eval()
        m.load_state_dict(to_torch_state_dict(make_weights(1234)), strict=True)
        params = list(m.parameters())
        opt = torch.optim.Adam(params, lr=1e-3, fused=True) if kind == 'torch' else Adam(params, lr=1e-3, max_grad_norm=c if kind == 'hip' else None)
        g = torch.Generator(device='cpu').manual_seed(3)
        losses = []
        for it in range(8):
            o, p = data[it % 4]
            n = o.shape[0]
            m.set_data(None, torch.from_numpy(o), torch.from_numpy(p))
            eq, ep, e20 = torch.randn(n, 32, generator=g), torch.randn(n, 32, generator=g), torch.randn(n * 20, 32, generator=g)
            tot = m.forward(eps_q=eq, eps_p=ep, eps20=e20)[0]
            opt.zero_grad()
            tot.backward()
            if c is None:
                c = 0.5 * math.sqrt(sum(float((q.grad.double() ** 2).sum()) for q in params if q.grad is not None))
            if kind == 'torch':
                torch.nn.utils.clip_grad_norm_(params, c)
            opt.step()
            if kind == 'hip' and it == 0:
                assert float(opt.last_grad_norm) > c            # clipping is active
            losses.append(float(tot.detach()))
        runs[kind] = losses
    np.testing.assert_allclose(runs['hip'], runs['torch'], rtol=2e-4)
    assert runs['hip'][-1] != runs['plain'][-1]
