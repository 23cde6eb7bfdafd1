"""GPU tests of the pmath backward passes (csrc/pmath_grad.hip) against the float64 yardstick of tests/golden/pmath_vjp.npz and
pmath_vjp_rows.npz: the reference's own functions differentiated by torch autograd in float64 on the stored float32 inputs.  Metric max |got - ref| / (1 + |ref|), bound 1e-4
(pmath_vjp_cases.BOUND), for every case.

Measured on the MI355X (worst over the fixture's cases per op; the reference's own fp32 run on the same inputs beside it): DESIGN.md 4q.
"""
import numpy as np
import pytest
import torch

from pmath_vjp_cases import BOUND, COMPOSITIONS, ROW_OPS, cases, err

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available(), 'these tests need the GPU'
    return torch.device('cuda:0')


def _call(pm, op, c, *a):
    if op in ('p2k', 'k2p'):
        return getattr(pm, op)(*a, c)
    if op == 'dist_matrix':
        return pm.dist_matrix(*a, c=c)
    return getattr(pm, 'lorenz_factor' if op == 'lorenz' else op)(*a, c=c)


def _vjp(pm, op, c, inputs, g, dev):
    ts = [torch.from_numpy(np.ascontiguousarray(a)).to(dev).requires_grad_() for a in inputs]
    out = _call(pm, op, c, *ts)
    assert out.requires_grad, op + ': the result is cut off from the graph'
    out.backward(torch.from_numpy(g).to(dev).reshape(out.shape))
    return out.detach(), [t.grad.cpu().numpy() for t in ts]


@pytest.fixture(scope='module')
def results(golden):
    """Every fixture case run once: [(case, forward value, gradients)]."""
    import sttode_amd.pmath as pm
    dev = _dev()
    z = golden('pmath_vjp')
    res = [(case,) + _vjp(pm, case['op'], case['c'], case['inputs'], case['g'], dev) for case in cases(z, golden('pmath_vjp_rows'))]
    torch.cuda.synchronize()
    return z, res


def test_every_case_against_the_float64_yardstick(results):
    z, res = results
    worst, ref32, bad = {}, {}, []
    for case, _, grads in res:
        for (k, ref, r32), got in zip(case['grads'], grads):
            if case['zero_row'] is not None and k.endswith('gx'):      # the deviation: zero gradient where the reference gives NaN
                assert not got[case['zero_row']].any(), 'mobius_matvec: the gradient of a zero x row must be zero'
            assert got.shape == ref.shape and np.isfinite(got).all(), k
            e = err(got, ref)
            worst[case['op']] = max(worst.get(case['op'], 0.0), e)
            ref32[case['op']] = max(ref32.get(case['op'], 0.0), err(r32, ref))
            if not e <= BOUND:
                bad.append((k, e))
    for op in sorted(worst):
        print('%-14s worst error %.2e   (reference fp32: %.2e)' % (op, worst[op], ref32[op]))
    assert set(ROW_OPS) | {'mobius_matvec', 'dist_matrix'} == set(worst)
    assert not bad, bad


def test_forward_values_of_the_two_paths_are_bitwise_equal(results):
    import sttode_amd.pmath as pm
    dev = _dev()
    seen = set()
    for case, out, _ in results[1]:
        ts = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in case['inputs']]
        plain = _call(pm, case['op'], case['c'], *ts)
        assert not plain.requires_grad and plain.shape == out.shape
        assert torch.equal(plain, out), case['name']
        with torch.no_grad():                                             # grad mode off: the forward-only calls, whatever the inputs ask
            ng = _call(pm, case['op'], case['c'], *[t.clone().requires_grad_() for t in ts])
        assert not ng.requires_grad and torch.equal(ng, out), case['name']
        seen.add(case['op'])
    assert set(ROW_OPS) | {'mobius_matvec', 'dist_matrix'} == seen


def test_gradients_are_finite_on_the_clipped_boundary(golden):
    """Points that project() produced from radius 1.2: finite gradients of dist0, logmap0, dist, lambda_x (no parity is claimed there)."""
    import sttode_amd.pmath as pm
    dev = _dev()
    z = golden('pmath_vjp')
    for c in (1.0, 0.5):
        xb = pm.project(torch.from_numpy(z['clip.project.c%s.x' % c]).to(dev), c=c)
        yb = xb.flip(0).contiguous()
        for op, two in (('dist0', False), ('logmap0', False), ('lambda_x', False), ('dist', True)):
            x, y = xb.clone().requires_grad_(), yb.clone().requires_grad_()
            out = _call(pm, op, c, *((x, y) if two else (x,)))
            out.backward(torch.ones_like(out))
            assert torch.isfinite(out).all() and torch.isfinite(x.grad).all() and (not two or torch.isfinite(y.grad).all()), (op, c)


def test_layers_of_the_reference_are_compositions_of_pmath_calls(golden):
    """hyptorch/nn.py's ToPoincare, HypLinear and HyperbolicDistanceLayer rebuilt from pmath calls only, held to the gradients of the
    reference's own modules (float64) at the same bound."""
    import sttode_amd.pmath as pm
    dev = _dev()
    z = golden('pmath_vjp')

    def topoincare(x):
        pm.RiemannianGradient.c = 1.0
        return pm.RiemannianGradient.apply(pm.project(pm.expmap0(x, c=1.0), c=1.0))

    def hyplinear(w, b, x):   # hyptorch/nn.py:66-74 passes c to every call but mobius_add, which runs at its default c = 1
        return pm.project(pm.mobius_add(pm.mobius_matvec(w, x, c=0.5), pm.expmap0(b, c=0.5)), c=0.5)

    def distlayer(x, y):
        return pm.dist(x, y, c=1.0, keepdim=True)
    try:
        for name, fn in (('comp.topoincare', topoincare), ('comp.hyplinear', hyplinear), ('comp.distlayer', distlayer)):
            ts = [torch.from_numpy(z['%s.%s' % (name, i)]).to(dev).requires_grad_() for i in COMPOSITIONS[name]]
            out = fn(*ts)
            out.backward(torch.from_numpy(z[name + '.g']).to(dev).reshape(out.shape))
            for i, t in zip(COMPOSITIONS[name], ts):
                e = err(t.grad.cpu().numpy(), z['%s.g%s64' % (name, i)])
                print('%s d/d%s: error %.2e   (reference fp32: %.2e)' % (name, i, e, err(z['%s.g%s32' % (name, i)], z['%s.g%s64' % (name, i)])))
                assert e <= BOUND, (name, i, e)
    finally:
        pm.RiemannianGradient.c = 1


def test_dist_matrix_backward_is_bitwise_repeatable(golden):
    from sttode_amd import capi
    dev = _dev()
    z = golden('pmath_vjp')
    x, y, g = (torch.from_numpy(z['dm.P67R3d65.' + k]).to(dev) for k in ('x', 'y', 'g'))
    runs = []
    for _ in range(2):
        gx, gy = torch.full_like(x, float('nan')), torch.full_like(y, float('nan'))
        capi.call('sttode_pmath_dist_matrix_bwd', x, y, g, gx, gy, 67, 3, 65, 1.0, capi.stream_ptr())
        runs.append((gx, gy))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert torch.isfinite(runs[0][0]).all() and torch.isfinite(runs[0][1]).all()


def test_refusals_name_the_entry_point_and_launch_nothing():
    from sttode_amd import capi
    dev = _dev()
    x, y, g = (torch.zeros(4, 8, device=dev) for _ in range(3))
    gx, gy = torch.full_like(x, 7.0), torch.full_like(x, 7.0)
    for args, word in (((2, x, y, g, gx, None, 4, 8, 1.0), 'gy'), ((99, x, y, g, gx, gy, 4, 8, 1.0), 'unknown op'),
                       ((12, x, None, g, gx, None, 4, 8, 1.0), 'Oblique'), ((2, x, y, g, gx, gy, 4, 8, 0.0), 'curvature'),
                       ((2, x, y, g, gx, gy, 4, 8, -1.0), 'curvature')):
        with pytest.raises(capi.SttodeError, match='sttode_pmath_rowop_bwd.*' + word):
            capi.call('sttode_pmath_rowop_bwd', *args, capi.stream_ptr())
    m, ws, v = torch.zeros(8, 8, device=dev), torch.zeros(4, 8, device=dev), torch.zeros(4, device=dev)
    with pytest.raises(capi.SttodeError, match='sttode_pmath_matvec_bwd.*curvature'):
        capi.call('sttode_pmath_matvec_bwd', m, x, g, ws, ws.clone(), v, gx, m.clone(), 4, 8, 8, 0.0, capi.stream_ptr())
    with pytest.raises(capi.SttodeError, match='sttode_pmath_dist_matrix_bwd.*curvature'):
        capi.call('sttode_pmath_dist_matrix_bwd', x, y, g, gx, gy, 4, 4, 8, -2.0, capi.stream_ptr())
    torch.cuda.synchronize()
    assert (gx == 7.0).all() and (gy == 7.0).all(), 'a refused call wrote its outputs'


def test_forward_only_functions_say_so():
    """_mobius_addition_batch, _hyperbolic_softmax, poincare_mean and the Oblique ops stay forward-only (documented in the module docstring)."""
    import sttode_amd.pmath as pm
    dev = _dev()
    x = (0.1 * torch.ones(3, 4, device=dev)).requires_grad_()
    assert not pm.poincare_mean(x, c=1.0).requires_grad and not pm.oblique_proj(x).requires_grad
    assert 'FORWARD-ONLY' in pm.__doc__ and 'forward values only' not in pm.__doc__
