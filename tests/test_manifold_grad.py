"""CPU tests of the opt-in gradients through poincare_mean and the manifold operations: the fixture
tests/golden/manifold_grad.npz checks itself, tests/riemannian_ref.py and the restated poincare_mean are held to it, and the new entry
points are exported, declared and refuse by name without a GPU.  The kernels are held to the same arrays in test_manifold_grad_gpu.py."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import manifold_grad_cases as mc
import riemannian_ref as rr
from pmath_vjp_cases import BOUND

NEW_EXPORTS = ('sttode_pmath_mean_seg', 'sttode_pmath_mean_bwd', 'sttode_pmath_mean_bwd_c', 'sttode_oblique_proj_bwd', 'sttode_oblique_dist_bwd',
               'sttode_manifold_rowop_bwd')


@pytest.fixture(scope='module')
def fx(golden):
    return rr.Fixture(golden('manifold_grad'), golden('riemannian_ops'))


def test_fixture_float32_run_is_within_the_bound_of_its_float64_run(fx):
    """Every stored float32 result of the reference within 1e-4 of its float64 run, in the project's metric; nothing stored is masked."""
    n = 0
    for k in fx.keys():
        if k.endswith('32'):
            a64, a32 = fx[k[:-2] + '64'], fx[k]
            assert np.isfinite(a64).all() and np.isfinite(a32).all(), k
            assert rr.err(a32, a64) <= BOUND, (k, rr.err(a32, a64))
            n += 1
    assert n >= 40
    mean = mc.MeanFixture(fx)
    assert len(mean.case) == len(mc.mean_cases()) == 122
    x = mean['mean.R2.W5.d16.c1.0.dim0']['x']
    assert np.array_equal(x[1, 1], -x[0, 1]) and not x[0, 3].any() and x[0, 1].any()
    for name, shape, dim, c in mc.mean_cases():
        assert (np.sqrt(c) * np.linalg.norm(mean[name]['x'].astype(np.float64), axis=-1) <= 0.95 + 1e-6).all()


def test_restated_poincare_mean_reproduces_the_reference(fx):
    """The few-line float64 restatement (the closed forms the kernels use) against the reference's values, dL/dx and dL/dc."""
    mean = mc.MeanFixture(fx)
    worst = 0.0
    for name, shape, dim, c in mc.mean_cases():
        rec = mean[name]
        x = torch.from_numpy(rec['x']).double().requires_grad_()
        ct = torch.tensor([c], dtype=torch.float64, requires_grad=True)
        out = mc.pmean(x, dim, ct)
        gx, gc = torch.autograd.grad((out * torch.from_numpy(rec['g']).double()).sum(), (x, ct))
        for got, key in ((out.detach(), 'out64'), (gx, 'gx64'), (gc, 'gc64')):
            worst = max(worst, rr.err(got.numpy(), rec[key]))
    assert worst <= 2e-7, worst      # the yardstick is stored as float32: 6e-8 relative


def test_riemannian_ref_gradients_equal_the_references(fx):
    """riemannian_ref.ObliqueRef (no reference plugged in) differentiated by autograd in float64 against the stored gradients of the
    reference's own Oblique; the zero-u row through the branch as taken."""
    man = mc.TakenOblique()
    worst = 0.0
    cases = [(name, fx[key], mc.OBL_OPS) for name, key, d in mc.obl_cases()] + [('obl.edge', fx['obl.edge.in'], ('expmap', 'retr_transp'))]
    for name, ins, ops in cases:
        for op in ops:
            _, grads = mc.vjp(lambda *t: mc.obl_run(man, op, *t), list(ins), list(fx[name + '.g']), torch.float64)
            worst = max(worst, rr.err(np.stack(grads), fx['%s.%s.grads64' % (name, op)]))
    assert worst <= 2e-7, worst
    assert not fx['obl.edge.in'][2, mc.EDGE_ZERO_ROW].any()
    # Oblique.inner of the reference is the matrix u w^T: its gradients are the matrix products, and say why the drop-in refuses it
    p, _, u, w = fx['op.obl.d16.in']
    g = fx['obl.inner.g'].astype(np.float64)
    assert rr.err(g @ w.astype(np.float64), fx['obl.inner.gu64']) <= 2e-7 and rr.err(g.T @ u.astype(np.float64), fx['obl.inner.gv64']) <= 2e-7


def test_oblique_dist_fixture_has_both_sides_of_the_clamp(fx):
    for nb, n1, n2, d in mc.OBL_DIST:
        name = 'dist.%d.%d.%d.%d' % (nb, n1, n2, d)
        s = np.einsum('bid,bjd->bij', fx[name + '.p2'].astype(np.float64), fx[name + '.p1'].astype(np.float64))
        assert (np.abs(np.abs(s) - (1 - 1e-4)) > 1e-5).all()
        coef = np.where(np.abs(s) <= 1 - 1e-4, -fx[name + '.g'] / np.sqrt(np.maximum(1 - s * s, 1e-300)), 0.0)
        assert rr.err(np.einsum('bij,bjd->bid', coef, fx[name + '.p1'].astype(np.float64)), fx[name + '.g264']) <= 2e-7
        assert rr.err(np.einsum('bij,bid->bjd', coef, fx[name + '.p2'].astype(np.float64)), fx[name + '.g164']) <= 2e-7
        if (nb, n1, n2, d) == mc.OBL_DIST_SPECIAL:
            assert coef[0, 0, 0] == 0 and coef[0, 1, 1] == 0 and np.count_nonzero(coef) == coef.size - 2


def test_ball_clip_case_has_both_sides_of_the_clip():
    for c in mc.CS:
        ins = mc.ball_clip_case(c)
        assert ins.shape == (4, 9, 16) and ins.dtype == np.float32


def test_new_exports_are_declared_bound_and_refuse_by_name():
    from sttode_amd import capi
    from test_capi_symbols import header_functions
    fns = header_functions()
    L = capi.lib()
    for name in NEW_EXPORTS:
        assert name in fns and name in capi.SIGNATURES and hasattr(L, name), name
        args = [0 if t in (ctypes.c_int, ctypes.c_long) else 0.0 if t in (ctypes.c_float, ctypes.c_double) else None for t in capi.SIGNATURES[name]]
        with pytest.raises(capi.SttodeError, match=name + ':'):
            capi.call(name, *args)
    one = 1     # a non-NULL pointer that no refused call may touch
    for name, args, needle in (
            ('sttode_manifold_rowop_bwd', (9, 2, one, one, one, one, None, one, one, one, 4, 4, 1.0, None), 'unknown op'),
            ('sttode_manifold_rowop_bwd', (0, 3, one, one, one, one, None, one, one, one, 4, 4, 1.0, None), 'unknown manifold'),
            ('sttode_manifold_rowop_bwd', (0, 2, one, one, one, one, None, one, one, one, 4, 4, -1.0, None), 'positive and finite'),
            ('sttode_manifold_rowop_bwd', (0, 2, one, one, one, one, None, one, one, one, 4, 4, float('nan'), None), 'positive and finite'),
            ('sttode_manifold_rowop_bwd', (2, 2, one, one, None, one, None, one, one, one, 4, 4, 1.0, None), 'third operand'),
            ('sttode_manifold_rowop_bwd', (0, 2, one, one, one, one, one, one, one, one, 4, 4, 1.0, None), 'g2 is retr_transp'),
            ('sttode_manifold_rowop_bwd', (5, 2, one, one, one, None, None, one, one, one, 4, 4, 1.0, None), 'upstream gradient'),
            ('sttode_manifold_rowop_bwd', (0, 2, one, one, one, one, None, None, None, None, 4, 4, 1.0, None), 'no gradient buffer'),
            ('sttode_manifold_rowop_bwd', (0, 2, one, one, one, one, None, one, one, one, 0, 4, 1.0, None), 'empty shape'),
            ('sttode_pmath_mean_seg', (one, one, one, one, None, None, 1, 2, 1, 4, 0.0, None, None), 'positive and finite'),
            ('sttode_pmath_mean_seg', (one, one, one, one, None, None, 1, 0, 1, 4, 1.0, None, None), 'empty shape'),
            ('sttode_pmath_mean_bwd', (one, one, one, one, one, 1, 2, 1, 4, float('inf'), None), 'positive and finite'),
            ('sttode_pmath_mean_bwd', (one, one, one, one, None, 1, 2, 1, 4, 1.0, None), 'null pointer'),
            ('sttode_pmath_mean_bwd_c', (one, one, one, one, one, 1, 2, 1, 4, None, one, one, None), 'c_dev is NULL'),
            ('sttode_pmath_mean_bwd_c', (one, one, one, one, one, 1, 2, 1, 4, one, None, one, None), 'gc_ws'),
            ('sttode_oblique_proj_bwd', (one, one, one, 4, 0, None), 'empty shape'),
            ('sttode_oblique_dist_bwd', (one, one, one, None, None, 1, 2, 2, 4, None), 'null pointer')):
        with pytest.raises(capi.SttodeError, match=name + ': .*' + needle):
            capi.call(name, *args)


def test_public_interface_and_defaults():
    from sttode_amd import capi, manifolds as mf, pmath
    for fn in (pmath.poincare_mean, pmath.oblique_proj, pmath.oblique_dist):
        par = inspect.signature(fn).parameters['differentiable']
        assert par.kind is inspect.Parameter.KEYWORD_ONLY and par.default is False
    assert list(inspect.signature(pmath.poincare_mean).parameters) == ['x', 'dim', 'c', 'differentiable']
    assert mf.Manifold.differentiable is False and mf.Oblique().differentiable is False and mf.PoincareBall(0.5).differentiable is False
    ball = mf.PoincareBall(0.5)
    assert mf.differentiable(ball) is ball and ball.differentiable is True and mf.PoincareBall(0.5).differentiable is False
    assert ball.c == 0.5 and isinstance(ball.c, float)
    z = torch.zeros(2, 4, requires_grad=True)
    for man in (mf.differentiable(mf.Oblique()), ball):       # no CPU fallback on the differentiable path either
        for call in (lambda: man.proj(z), lambda: man.egrad2rgrad(z, z), lambda: man.expmap(z, z), lambda: man.ptransp(z, z, z),
                     lambda: man.retr(z, z), lambda: man.retr_transp(z, z, z), lambda: man.dist(z, z)):
            with pytest.raises(capi.SttodeError):
                call()
    for call in (lambda: pmath.poincare_mean(z, differentiable=True), lambda: pmath.oblique_proj(z, differentiable=True),
                 lambda: pmath.oblique_dist(z, z, differentiable=True)):
        with pytest.raises(capi.SttodeError):
            call()
    for name in ('logmap', 'inner'):
        with pytest.raises(NotImplementedError):
            getattr(mf.differentiable(mf.Oblique()), name)(z, z)
    assert 'FORWARD-ONLY' in pmath.__doc__ and 'forward values only' not in pmath.__doc__ and 'differentiable=True' in pmath.__doc__
    assert 'FORWARD-ONLY' in mf.__doc__ and 'differentiable(manifold)' in mf.__doc__
