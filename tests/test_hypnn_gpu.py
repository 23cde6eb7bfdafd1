"""GPU tests of the hyperbolic layers (sttode_amd/hypnn.py) and of the kernels they add (csrc/pmath_grad.hip: _hyperbolic_softmax's backward,
the feature clip; _mobius_addition_batch through mobius_add's row kernel) against the float64 yardstick of tests/golden/hypnn.npz: the
reference's own functions and modules differentiated by torch autograd in float64 on the stored float32 inputs.  Metric
max |got - ref| / (1 + |ref|), bound 1e-4 (pmath_vjp_cases.BOUND), for every case.

Measured on the MI355X (worst per op; the reference's own fp32 run on the same inputs beside it): DESIGN.md 4r.
"""
import numpy as np
import pytest
import torch

from hypnn_cases import (BOUND, CLIP_R, MODULES, TRAIN_LR, TRAIN_STEPS, case_arrays, case_forward, case_grads, err, function_cases,
                         shape_tag, train_model)

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available(), 'these tests need the GPU'
    return torch.device('cuda:0')


def _fn(pm, op, c):
    if op == 'hsoftmax':
        return lambda X, A, P: pm._hyperbolic_softmax(X, A, P, c)
    if op == 'mobius_addition_batch':
        return lambda x, y: pm._mobius_addition_batch(x, y, c)
    return lambda x: pm.feature_clip(x, CLIP_R)


def _module(hn, name, params, dev):
    m = MODULES[name](hn)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=True)
    return m.to(dev)


@pytest.fixture(scope='module')
def results(golden):
    """Every gradient case of the fixture run once: {case: (family, forward value, {key: gradient}, rerun without grad)}."""
    import sttode_amd.hypnn as hn
    import sttode_amd.pmath as pm
    dev = _dev()
    z = golden('hypnn')
    res = {}
    try:
        todo = [(name, op, _fn(pm, op, c), None) for name, op, c in function_cases()]
        for name in MODULES:
            case = 'mod.' + name
            todo.append((case, 'mod.' + name.split('.')[0], _module(hn, name, case_arrays(z, case)[1], dev), True))
        for case, family, fn, is_module in todo:
            ins, _, g = case_arrays(z, case)
            ts = [torch.from_numpy(a).to(dev).requires_grad_() for a in ins]
            out = fn(*ts)
            assert out.requires_grad, case + ': the result is cut off from the graph'
            out.backward(torch.from_numpy(g).to(dev).reshape(out.shape))
            grads = {'gin.%d' % k: t.grad.cpu().numpy() for k, t in enumerate(ts)}
            if is_module:
                grads.update({'gp.' + n: p.grad.cpu().numpy() for n, p in fn.named_parameters()})
            with torch.no_grad():
                plain = fn(*[t.detach() for t in ts])
            res[case] = (family, out.detach(), grads, plain)
        torch.cuda.synchronize()
    finally:
        pm.RiemannianGradient.c = 1
    return z, res


def test_every_case_against_the_float64_yardstick(results):
    z, res = results
    worst, ref32, bad = {}, {}, []
    for case, (family, _, grads, _) in res.items():
        stored = case_grads(z, case)
        assert sorted(k for k, _, _ in stored) == sorted(grads), case
        for k, ref, r32 in stored:
            got = grads[k]
            assert got.shape == ref.shape and np.isfinite(got).all(), (case, k)
            e = err(got, ref)
            worst[family] = max(worst.get(family, 0.0), e)
            ref32[family] = max(ref32.get(family, 0.0), err(r32, ref))
            if not e <= BOUND:
                bad.append((case, k, e))
    for family in sorted(worst):
        print('%-30s worst error %.2e   (reference fp32: %.2e)' % (family, worst[family], ref32[family]))
    assert {'hsoftmax', 'mobius_addition_batch', 'clip', 'mod.mlr', 'mod.hyplinear', 'mod.hyplinear_nobias', 'mod.concat', 'mod.distlayer',
            'mod.topoincare', 'mod.topoincare_euclidean_grad', 'mod.topoincare_train_x', 'mod.frompoincare',
            'mod.frompoincare_train_x'} == set(worst)
    assert not bad, bad


def test_forward_values_of_the_two_paths_are_bitwise_equal(results):
    import sttode_amd.pmath as pm
    dev = _dev()
    z, res = results
    for case, (_, out, _, plain) in res.items():
        assert not plain.requires_grad and plain.shape == out.shape and torch.equal(plain, out), case
    for name, op, c in function_cases():                               # no input asks for a gradient: today's call
        ts = [torch.from_numpy(a).to(dev) for a in case_arrays(z, name)[0]]
        plain = _fn(pm, op, c)(*ts)
        assert not plain.requires_grad and torch.equal(plain, res[name][1]), name
        with torch.no_grad():                                          # grad mode off, whatever the inputs ask
            ng = _fn(pm, op, c)(*[t.clone().requires_grad_() for t in ts])
        assert not ng.requires_grad and torch.equal(ng, res[name][1]), name


def test_forward_values_against_the_reference_formulas(results):
    """The clip op's forward against its formula in float64, and the forward value of every module against the reference module's own
    float64 run on the same float32 inputs and parameters (<case>.out64 of the fixture; its rounding to float32, 6e-8 relative, is inside the
    1e-6 floor).  Two bounds per module family: the project's 1e-4, and eight times the error of the reference's own fp32 run (or 1e-6),
    which a dropped tail element or a swapped index does not pass.  The forward values of the raw pair functions at these shapes, and of
    every pmath function at the wave and block edges: test_pmath_forward_gpu.py."""
    z, res = results
    for kind in ('clipped', 'unclipped', 'mixed'):
        x = case_arrays(z, 'clip.' + kind)[0][0].astype(np.float64)
        n = np.linalg.norm(x, axis=-1, keepdims=True) + np.float64(np.float32(1e-5))
        e = err(res['clip.' + kind][1].cpu().numpy(), x * np.minimum(1.0, CLIP_R / n))
        print('clip.%s forward: error %.2e' % (kind, e))
        assert e <= 1e-6, (kind, e)       # one rounding of a float64 product to float32: 6e-8 relative
    worst, ref32 = {}, {}
    for case, (family, out, _, _) in res.items():
        if not case.startswith('mod.'):
            continue
        ref, r32 = case_forward(z, case)
        got = out.cpu().numpy()
        assert got.shape == ref.shape and np.isfinite(got).all(), case
        worst[family] = max(worst.get(family, 0.0), err(got, ref))
        ref32[family] = max(ref32.get(family, 0.0), err(r32, ref))
    for family in sorted(worst):
        print('%-30s forward: worst error %.2e   (reference fp32: %.2e)' % (family, worst[family], ref32[family]))
    assert len(worst) == 10 and sum(c.startswith('mod.') for c in res) == len(MODULES)
    bad = [(f, worst[f], ref32[f]) for f in sorted(worst) if not (worst[f] <= BOUND and worst[f] <= max(8 * ref32[f], 1e-6))]
    assert not bad, bad


def test_hyperbolic_softmax_backward_is_bitwise_repeatable(golden):
    from sttode_amd import capi
    dev = _dev()
    z = golden('hypnn')
    for B, C, d, c in ((3, 67, 65, 0.5), (70, 3, 130, 1.0)):
        (X, A, P), _, g = case_arrays(z, 'hs.' + shape_tag(B, C, d, c))
        X, A, P, g = (torch.from_numpy(a).to(dev) for a in (X, A, P, g))
        runs = []
        for _ in range(2):
            outs = [torch.full_like(t, float('nan')) for t in (X, A, P)]
            ws = torch.full((6, B, C), float('nan'), dtype=torch.float64, device=dev)
            capi.call('sttode_pmath_hsoftmax_bwd', X, A, P, g, ws, *outs, B, C, d, c, capi.stream_ptr())
            runs.append(outs + [ws])
        for a, b in zip(*runs):
            assert torch.isfinite(a).all() and torch.equal(a, b)


def test_training_record(golden):
    """ToPoincare(clip_r) -> HypLinear -> HyperbolicMLR: the reference's initial state_dict loads strictly, and 5 Adam steps on the device
    follow the reference's float64 losses."""
    import sttode_amd.hypnn as hn
    import sttode_amd.pmath as pm
    dev = _dev()
    z = golden('hypnn')
    try:
        model = train_model(hn)
        model.load_state_dict({k[len('train.sd.'):]: torch.from_numpy(v) for k, v in z.items() if k.startswith('train.sd.')}, strict=True)
        model.to(dev)
        x, labels = torch.from_numpy(z['train.x']).to(dev), torch.from_numpy(z['train.labels']).to(dev)
        opt = torch.optim.Adam(model.parameters(), lr=TRAIN_LR)
        losses = []
        for _ in range(TRAIN_STEPS):
            opt.zero_grad()
            loss = torch.nn.functional.cross_entropy(model(x), labels)
            loss.backward()
            opt.step()
            losses.append(loss.item())
    finally:
        pm.RiemannianGradient.c = 1
    for i, (got, ref, r32) in enumerate(zip(losses, z['train.loss64'], z['train.loss32'])):
        print('step %d: loss %.7f   float64 reference %.7f   error %.2e   (reference fp32: %.2e)' % (i, got, ref, err(got, ref), err(r32, ref)))
    assert all(err(got, ref) <= BOUND for got, ref in zip(losses, z['train.loss64'])), losses
    assert losses[-1] < losses[0]


def test_refusals():
    import sttode_amd.hypnn as hn
    from sttode_amd import capi
    dev = _dev()
    with pytest.raises(capi.SttodeError, match='HIP tensors'):
        hn.HyperbolicMLR(8, 5, c=1.0).to(dev)(torch.zeros(3, 8))
    with pytest.raises(capi.SttodeError, match='HIP tensors'):
        hn.HypLinear(8, 4, c=1.0)(torch.zeros(3, 8, device=dev))          # the module's parameters are still on the CPU
    X, A, P = (torch.full((4, 8), 0.1, device=dev) for _ in range(3))
    g = torch.ones(4, 4, device=dev)
    outs = [torch.full((4, 8), 7.0, device=dev) for _ in range(3)]
    ws = torch.full((6, 4, 4), 7.0, dtype=torch.float64, device=dev)
    for args, word in (((X, A, P, g, ws, *outs, 4, 4, 8, 0.0), 'curvature'), ((X, A, P, g, ws, *outs, 4, 0, 8, 1.0), 'positive'),
                       ((X, A, P, g, None, *outs, 4, 4, 8, 1.0), 'null pointer')):
        with pytest.raises(capi.SttodeError, match='sttode_pmath_hsoftmax_bwd.*' + word):
            capi.call('sttode_pmath_hsoftmax_bwd', *args, capi.stream_ptr())
    with pytest.raises(capi.SttodeError, match='sttode_pmath_clip: .*radius'):
        capi.call('sttode_pmath_clip', X, outs[0], 4, 8, 0.0, capi.stream_ptr())
    with pytest.raises(capi.SttodeError, match='sttode_pmath_clip_bwd: .*radius'):
        capi.call('sttode_pmath_clip_bwd', X, A, outs[0], 4, 8, -1.0, capi.stream_ptr())
    torch.cuda.synchronize()
    assert all((o == 7.0).all() for o in outs) and (ws == 7.0).all(), 'a refused call wrote its outputs'
