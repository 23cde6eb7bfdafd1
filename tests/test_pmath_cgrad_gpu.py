"""GPU tests of the trainable curvature (csrc/pmath.hip, csrc/pmath_grad.hip): c as a 1-element tensor on the device
through sttode_amd.pmath and sttode_amd.hypnn.  The c gradients are held to the float64 yardstick of tests/golden/pmath_cgrad.npz -- the
reference's own functions and modules differentiated by torch autograd in float64 on the stored float32 inputs -- on
|got - ref| / (1 + |ref|) <= 1e-4; everything else on the tensor-c path is held BITWISE to the float-c path at the same value.

Measured on the MI355X (worst over the fixture's cases per op, the reference's own fp32 run beside it): DESIGN.md 4w.
"""
from collections import OrderedDict

import numpy as np
import pytest
import torch
from torch import nn

from pmath_cgrad_cases import BOUND, CLIP_R, MODULE_C, MODULES, cases, err

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available(), 'these tests need the GPU'
    return torch.device('cuda:0')


def _call(pm, op, c, *a):
    if op in ('p2k', 'k2p', '_hyperbolic_softmax', '_mobius_addition_batch'):
        return getattr(pm, op)(*a, c)
    return getattr(pm, 'lorenz_factor' if op == 'lorenz' else op)(*a, c=c)


def _ctensor(c, dev, grad):
    return torch.tensor([c], dtype=torch.float32, device=dev, requires_grad=grad)


def _run(pm, case, dev, c, tensors_grad):
    """One forward and backward pass: (forward value, [input gradients or None], c.grad or None)."""
    ts = [torch.from_numpy(np.ascontiguousarray(a)).to(dev).requires_grad_(tensors_grad) for a in case['inputs']]
    out = _call(pm, case['op'], c, *ts)
    if out.requires_grad:
        out.backward(torch.from_numpy(np.ascontiguousarray(case['g'])).to(dev).reshape(out.shape))
    cg = c.grad if isinstance(c, torch.Tensor) else None
    return out.detach(), [t.grad for t in ts], cg


@pytest.fixture(scope='module')
def results(golden):
    """Every fixture case run four ways, once: tensor c with everything requiring grad, float c, c alone requiring grad, a tensor c
    that does not require grad."""
    import sttode_amd.pmath as pm
    dev = _dev()
    res = []
    for case in cases(golden('pmath_cgrad'), golden('pmath_vjp'), golden('pmath_vjp_rows')):
        cv = float(np.float32(case['c']))
        res.append((case, _run(pm, case, dev, _ctensor(cv, dev, True), True), _run(pm, case, dev, cv, True),
                    _run(pm, case, dev, _ctensor(cv, dev, True), False), _run(pm, case, dev, _ctensor(cv, dev, False), True)))
    torch.cuda.synchronize()
    return res


def test_c_gradient_of_every_case_against_the_float64_yardstick(results):
    worst, ref32, bad = {}, {}, []
    for case, (_, _, gc), _, _, _ in results:
        assert gc is not None and gc.shape == (1,) and torch.isfinite(gc).all(), case['name']
        e = err(gc.item(), case['gc64'])
        worst[case['op']] = max(worst.get(case['op'], 0.0), e)
        ref32[case['op']] = max(ref32.get(case['op'], 0.0), err(case['gc32'], case['gc64']))
        if not e <= BOUND:
            bad.append((case['name'], e, gc.item(), case['gc64']))
    for op in sorted(worst):
        print('%-22s dL/dc worst error %.2e   (reference fp32: %.2e)' % (op, worst[op], ref32[op]))
    assert len(worst) == 12 + 4
    assert not bad, bad


def test_forward_values_and_tensor_gradients_are_bitwise_those_of_the_float_path(results):
    for case, (out, grads, _), (fout, fgrads, _), _, _ in results:
        assert torch.equal(out, fout), case['name'] + ': forward value'
        for i, (a, b) in enumerate(zip(grads, fgrads)):
            assert a is not None and a.shape == b.shape and torch.equal(a, b), '%s: gradient of input %d' % (case['name'], i)


def test_partial_requirements(results):
    for case, (out, grads, gc), _, (cout, cgrads, cgc), (nout, ngrads, ngc) in results:
        assert all(g is None for g in cgrads) and torch.equal(cout, out), case['name']
        assert torch.equal(cgc, gc), case['name'] + ': c alone requiring grad gives another c.grad'
        assert ngc is None and torch.equal(nout, out), case['name']
        assert all(torch.equal(a, b) for a, b in zip(ngrads, grads)), case['name'] + ': a c that does not require grad changes the tensor gradients'


def test_c_gradient_is_bitwise_repeatable(golden):
    """Two runs of the entry points into buffers prefilled with different values: gc is written, not accumulated, and has equal bits."""
    from sttode_amd import capi
    dev = _dev()
    zc, z = golden('pmath_cgrad'), golden('pmath_vjp')
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    c, c1, c07 = (_ctensor(v, dev, False) for v in (2.0, 1.0, MODULE_C))      # each case at the curvature its inputs were drawn for
    x, y, _ = (t(a) for a in zc['edge.in'])
    gs = t(zc['edge.gs'])
    dx, dy, dg = (t(z['dm.P67R3d65.' + k]) for k in ('x', 'y', 'g'))
    X, A, P, hg = (t(zc['pair.B67C3d65.' + k]) for k in ('X', 'A', 'P', 'g'))
    runs = []
    for fill in (7.0, -3.0):
        gc = [torch.full((1,), fill, device=dev) for _ in range(3)]
        ws = [torch.full((n,), fill, dtype=torch.float64, device=dev) for n in (1030, 67, 67)]
        capi.call('sttode_pmath_rowop_bwd_c', 3, x, y, gs, None, None, 1030, 5, c, ws[0], gc[0], capi.stream_ptr())
        capi.call('sttode_pmath_dist_matrix_bwd_c', dx, dy, dg, None, None, 67, 3, 65, c1, ws[1], gc[1], capi.stream_ptr())
        capi.call('sttode_pmath_hsoftmax_bwd_c', X, A, P, hg, torch.empty(7, 67, 3, dtype=torch.float64, device=dev), None, None, None, 67, 3, 65,
                  c07, ws[2], gc[2], capi.stream_ptr())
        runs.append(torch.cat(gc))
    assert torch.isfinite(runs[0]).all() and torch.equal(runs[0], runs[1]), runs
    for got, k in zip(runs[0].tolist(), ('edge.dist.n1030', 'dm.P67R3d65', 'hs.B67C3d65')):
        assert err(got, zc[k + '.gc'][0]) <= BOUND, k


def test_no_host_read_a_captured_forward_follows_the_curvature_on_the_device(golden):
    import sttode_amd.pmath as pm
    from sttode_amd import hypnn
    dev = _dev()
    z = golden('pmath_vjp')
    t = lambda k: torch.from_numpy(z[k]).to(dev)
    x, m, dx, dy = t('mv.d16O16.x'), t('mv.d16O16.m'), t('dm.P5R9d16.x'), t('dm.P5R9d16.y')
    torch.manual_seed(3)
    mlr = hypnn.HyperbolicMLR(16, 5, c=1.0).to(dev)
    c = _ctensor(1.0, dev, False)

    def forward(cc):
        return pm.expmap0(x, c=cc), pm.mobius_matvec(m, x, c=cc), pm.dist_matrix(dx, dy, c=cc), mlr(x, c=cc)
    with torch.no_grad():
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            forward(c)                                   # warm-up: the library and the allocator, outside the capture
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            outs = forward(c)
        c.fill_(0.5)
        graph.replay()
        torch.cuda.synchronize()
        want = forward(0.5)
    for a, b in zip(outs, want):
        assert torch.isfinite(a).all() and torch.equal(a, b)


def _build(hypnn, name, c, zc, dev):
    t = lambda k: torch.from_numpy(zc['%s.%s' % (name, k)]).to(dev)
    if name == 'mod.net':
        net = nn.ModuleDict(dict(tp=hypnn.ToPoincare(c=c), lin=hypnn.HypLinear(16, 8, c=1.0), mlr=hypnn.HyperbolicMLR(8, 5, c=1.0))).to(dev)
        with torch.no_grad():
            for p, k in ((net['lin'].weight, 'w'), (net['lin'].bias, 'b'), (net['mlr'].a_vals, 'a'), (net['mlr'].p_vals, 'p')):
                p.copy_(t(k))
        cc = net['tp'].c
        return net, lambda xx, cc=cc: net['mlr'](net['lin'](net['tp'](xx), c=cc), c=cc), dict(w=net['lin'].weight, b=net['lin'].bias,
                                                                                         a=net['mlr'].a_vals, p=net['mlr'].p_vals, c=cc)
    mod = {'mod.to': lambda: hypnn.ToPoincare(c=c), 'mod.to_xp_clip': lambda: hypnn.ToPoincare(c=c, train_x=True, ball_dim=16, clip_r=CLIP_R),
           'mod.from': lambda: hypnn.FromPoincare(c=c), 'mod.from_xp': lambda: hypnn.FromPoincare(c=c, train_x=True, ball_dim=16)}[name]().to(dev)
    if mod.xp is not None:
        with torch.no_grad():
            mod.xp.copy_(t('xp'))
    return mod, mod, {**({'xp': mod.xp} if mod.xp is not None else {}), 'c': mod.c}


def test_modules_give_every_parameter_gradient_of_the_reference(golden):
    import sttode_amd.pmath as pm
    from sttode_amd import hypnn
    dev = _dev()
    zc = golden('pmath_cgrad')
    try:
        for name in MODULES:
            mod, run, params = _build(hypnn, name, nn.Parameter(torch.tensor([MODULE_C])), zc, dev)
            assert isinstance(params['c'], nn.Parameter) and 'c' in dict(mod.named_parameters()) or name == 'mod.net'
            x = torch.from_numpy(zc[name + '.x']).to(dev).requires_grad_()
            out = run(x)
            out.backward(torch.from_numpy(zc[name + '.g']).to(dev).reshape(out.shape))
            for k, p in {**params, 'x': x}.items():
                ref = zc['%s.g%s' % (name, k)]
                assert p.grad is not None and p.grad.shape == ref[0].shape, (name, k)
                e = err(p.grad.cpu().numpy(), ref[0])
                print('%-15s d/d%-2s error %.2e   (reference fp32: %.2e)' % (name, k, e, err(ref[1], ref[0])))
                assert e <= BOUND, (name, k, e)
    finally:
        pm.RiemannianGradient.c = 1


def test_a_training_step_moves_the_shared_curvature(golden):
    import sttode_amd.pmath as pm
    from sttode_amd import hypnn
    dev = _dev()
    zc = golden('pmath_cgrad')
    try:
        net, run, params = _build(hypnn, 'mod.net', nn.Parameter(torch.tensor([MODULE_C])), zc, dev)
        c = params['c']
        assert sum(p is c for p in net.parameters()) == 1 and len(list(net.parameters())) == 5
        x = torch.from_numpy(zc['mod.net.x']).to(dev)
        opt = torch.optim.Adam(net.parameters(), lr=1e-2)
        before = c.detach().clone()
        nn.functional.cross_entropy(run(x), torch.arange(9, device=dev) % 5).backward()
        opt.step()
        assert torch.isfinite(c).all() and not torch.equal(c.detach(), before), 'the optimiser step left c where it was'
        with torch.no_grad():
            got = run(x)
            cf = float(c.item())
            want = net['mlr'](net['lin'](hypnn.ToPoincare(c=cf)(x), c=cf), c=cf)
        assert torch.isfinite(got).all() and torch.equal(got, want)
    finally:
        pm.RiemannianGradient.c = 1


def test_checkpoints_of_the_reference_with_train_c_load_strictly():
    import sttode_amd.pmath as pm
    from sttode_amd import hypnn
    dev = _dev()
    try:
        for cls in (hypnn.ToPoincare, hypnn.FromPoincare):
            # the reference's state dicts: train_c=True -> 'c' [1]; with train_x 'xp' [ball_dim] first
            for sd in (OrderedDict(c=torch.tensor([0.9])), OrderedDict(xp=torch.full((6,), 0.1), c=torch.tensor([0.9]))):
                mod = cls(c=nn.Parameter(torch.tensor([0.7])), train_x='xp' in sd, ball_dim=6).to(dev)
                assert list(mod.state_dict().keys()) == list(sd.keys()) and mod.state_dict()['c'].shape == (1,)
                mod.load_state_dict(sd, strict=True)
                assert mod.c.item() == pytest.approx(0.9) and mod.c.requires_grad and mod.c.is_cuda
                out = mod(torch.full((2, 6), 0.05, device=dev))
                assert out.requires_grad and torch.isfinite(out).all()
        with pytest.raises(NotImplementedError, match='train_c.*nn.Parameter'):
            hypnn.ToPoincare(0.7, train_c=True)
    finally:
        pm.RiemannianGradient.c = 1


def test_refusals():
    import sttode_amd.pmath as pm
    from sttode_amd import capi, manifolds
    dev = _dev()
    x = torch.full((3, 4), 0.1, device=dev)
    bad = (torch.tensor([1.0], dtype=torch.float64, device=dev), torch.tensor([1.0, 1.0], device=dev), torch.tensor([1.0]))
    for c in bad:
        for call in (lambda: pm.expmap0(x, c=c), lambda: pm.mobius_add(x, x, c=c), lambda: pm.mobius_matvec(x[:, :4], x, c=c),
                     lambda: pm.dist_matrix(x, x, c=c), lambda: pm._hyperbolic_softmax(x, x, x, c), lambda: pm._mobius_addition_batch(x, x, c)):
            with pytest.raises(capi.SttodeError, match='1-element float32 tensor on the inputs'):
                call()
    with pytest.raises(capi.SttodeError, match='poincare_mean.*forward-only'):
        pm.poincare_mean(x, c=torch.tensor([1.0], device=dev))
    with pytest.raises(ValueError, match='PoincareBall.*not a tensor'):
        manifolds.PoincareBall(c=torch.tensor([1.0], device=dev))
