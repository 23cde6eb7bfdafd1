"""CPU tests of the Riemannian optimisers' surface (sttode_amd.manifolds, sttode_amd.optim.RiemannianAdam / RiemannianSGD, the two C
entry points of csrc/manifold.hip) and of their fixture.  The kernels themselves are held to the fixture in test_riemannian_gpu.py.

Yardstick: tests/golden/riemannian.npz and riemannian_ops.npz, written by tests/golden/make_riemannian_golden.py from the reference's own
Oblique and hyptorch.pmath functions plus the loops of riemannian_ref.py; `*64` is the float64 run on the float32 inputs, `*32` the
float32 run of the same code.  Bound: pmath_vjp_cases.BOUND = 1e-4 on max |got - ref| / (1 + |ref|).
"""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import riemannian_ref as rr
from pmath_vjp_cases import BOUND

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def fx(golden):
    return rr.Fixture(golden('riemannian'), golden('riemannian_ops'))


def _t(a, dt=torch.float64):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dt)


# --------------------------------------------------------------------------------------------------- the fixture checks itself
@pytest.mark.parametrize('group', ['op.'] + ['opt.%s.' % case for case in rr.OPT_CASES])
def test_fixture_float32_run_is_within_the_bound_of_the_float64_run(fx, group):
    """Every stored float32 array against its float64 partner: the reference's own arithmetic holds the bound the kernels are held to
    (the worst figure of each group is printed).  Measured: op. 1.9e-07, opt.obl. 6.1e-07, opt.ball.c0.5. 1.5e-07, opt.ball.c1.0. 3.2e-07,
    opt.three. 6.6e-07, opt.clip. 4.6e-07.

    The clip case is why riemannian_ref.ball_ptransp regroups the gyration over d = y - x: on project's sphere x and y = retr(x, u) are
    nearly the same point at |x|^2 = 0.998 / c, the denominator 1 - 2 c <x,y> + c^2 |x|^2 |y|^2 is 4e-6, and formed from terms of size 1
    in float32 it put the transported SGD momentum buffer 4.1e-04 from the float64 run (on values of 2.7e-03)."""
    worst, n = ('', 0.0), 0
    bad = []
    for k in fx.keys():
        if not (k.endswith('32') and k.startswith(group)):
            continue
        a32, a64 = fx[k], fx[k[:-2] + '64']
        assert a32.dtype == a64.dtype == np.float32 and a32.shape == a64.shape, k
        assert np.isfinite(a64).all() and np.isfinite(a32).all(), k
        e = rr.err(a32, a64)
        n += 1
        worst = max(worst, (k, e), key=lambda t: t[1])
        if not e <= BOUND:
            bad.append((k, e))
    print('float32 run vs float64 run, worst of %d arrays of %s: %s %.2e' % (n, group, *worst))
    n_ball = sum(man == 'poincare' for _, man, _, _ in rr.op_shapes())
    # vector results of every shape, edge and bcast, inner of the ball's; per optimiser parameter x, s1, s2 (adam), x, s1 (sgdm), x (sgd0)
    assert n == (len(rr.op_shapes()) + 2 + n_ball + 1 if group == 'op.' else 6 * len(rr.OPT_CASES[group[4:-1]][0]))
    assert not bad, bad


def test_fixture_has_every_case_and_the_stated_edge_rows(fx):
    for name, man, c, d in rr.op_shapes():
        assert fx[name + '.in'].shape == (4, rr.MAX_ROWS, d) and fx[name + '.out64'].shape == (len(rr.OP_NAMES), rr.MAX_ROWS, d), name
        p = fx[name + '.in'][0].astype(np.float64)
        r = np.sqrt(c) * np.linalg.norm(p, axis=-1)
        assert (np.abs(r - 1) < 1e-6).all() if man == 'oblique' else ((r > 0.049) & (r < 0.901)).all(), name
    assert len(rr.op_cases()) == 3 * (len(rr.DIMS) * 3 - 1)
    n = np.linalg.norm(fx['op.obl.edge.in'][2].astype(np.float64), axis=-1)
    assert n[4] == 0 and abs(n[6] - 5e-5) < 1e-9 and (np.delete(n, (4, 6)) > 2e-4).all()       # no row within a factor 2 of the 1e-4 branch
    p = fx['op.obl.edge.in'][0]
    np.testing.assert_allclose(fx['op.obl.edge.out64'][1][4], p[4], atol=1e-6)                   # a zero u returns p, not NaN
    assert fx['op.ball.bcast.out64'].shape == (len(rr.OP_NAMES), 2, 3, 16)
    for case, (params, lr) in rr.OPT_CASES.items():
        for k, (man, c, shape) in enumerate(params):
            assert fx['opt.%s.p%d.g' % (case, k)].shape == (rr.STEPS,) + shape
            assert fx[rr.opt_key(case, k, 'adam', 's2', 64)].shape == (rr.STEPS,) + shape[:-1] + (1,)
            assert rr.opt_key(case, k, 'sgd0', 's1', 64) not in fx and rr.opt_key(case, k, 'sgdm', 's1', 64) in fx
    # the clip case: every SGD step ends on project's sphere; Adam's steps are a geodesic distance below 1 whatever the gradient: its first
    # three approach the sphere, the other five are clipped
    for k, (man, c, shape) in enumerate(rr.OPT_CASES['clip'][0]):
        x0 = fx['opt.clip.p%d.x0' % k].astype(np.float64)
        np.testing.assert_allclose(np.sqrt(c) * np.linalg.norm(x0, axis=-1), 0.99, atol=1e-6)
        assert ((fx['opt.clip.p%d.g' % k].astype(np.float64) * x0).sum(-1) < 0).all()
        for rule in rr.RULES:
            r = np.sqrt(c) * np.linalg.norm(fx[rr.opt_key('clip', k, rule, 'x', 64)].astype(np.float64), axis=-1)
            np.testing.assert_allclose(r[3 if rule == 'adam' else 0:], 1 - 1e-3, atol=1e-6)


def test_restatement_reproduces_the_fixture(fx):
    """riemannian_ref.py on its own functions (no reference plugged in) gives the stored float64 arrays: what the GPU tests and the
    documents call the yardstick is what the reference's functions gave."""
    for name, man, c, d in rr.op_shapes()[::5] + [('op.obl.edge', 'oblique', 1.0, 16)]:
        vec, inner = rr.run_ops(rr.make_manifold(man, c), *[_t(a) for a in fx[name + '.in']])
        assert rr.err(vec.numpy(), fx[name + '.out64']) <= 1e-6, name
        if man == 'poincare':
            assert rr.err(inner.numpy(), fx[name + '.inner64']) <= 1e-6, name
    for case in ('obl', 'ball.c0.5', 'clip'):
        params, lr = rr.OPT_CASES[case]
        for k, (man, c, shape) in enumerate(params):
            for rule in rr.RULES:
                steps = rr.run_rule(rule, rr.make_manifold(man, c), _t(fx['opt.%s.p%d.x0' % (case, k)]), list(_t(fx['opt.%s.p%d.g' % (case, k)])), lr)
                for i, what in enumerate(('x', 's1', 's2')):
                    if steps[0][i] is not None:
                        got = torch.stack([s[i] for s in steps]).numpy()
                        assert rr.err(got, fx[rr.opt_key(case, k, rule, what, 64)]) <= 1e-6, (case, k, rule, what)


def test_ptransp_is_the_gyration_and_preserves_the_norm(fx):
    """The closed-form gyration equals its definition -(a (+) b) (+) (a (+) (b (+) w)) with exact Moebius addition, and the stored
    ptransp keeps lambda |.|, the Riemannian norm (Oblique: the transported vector is tangent at y)."""
    rng = np.random.default_rng(5)
    for c in rr.CS:
        for d in (1, 2, 16):
            a, b, w = (_t(rng.standard_normal((7, d)) * 0.4 / np.sqrt(c) / np.sqrt(d)) for _ in range(3))
            add = lambda x, y: rr.mobius_add_exact(x, y, c)
            want = add(-add(a, b), add(a, add(b, w)))
            assert rr.err(rr.gyration(a, b, w, c).numpy(), want.numpy()) <= 1e-10, (c, d)
            # the regrouped form the ball's ptransp uses is the same function: gyr[y, -x] w lambda_x / lambda_y
            lam = lambda x: 2 / (1 - c * (x * x).sum(-1, keepdim=True))
            assert rr.err(rr.ball_ptransp(a, b, w, c).numpy(), (rr.gyration(b, -a, w, c) * lam(a) / lam(b)).numpy()) <= 1e-12, (c, d)
    for name, man, c, d in rr.op_shapes():
        p, y, u, w = (a.astype(np.float64) for a in fx[name + '.in'])
        got = fx[name + '.out64'][2].astype(np.float64)
        if man == 'oblique':
            assert np.abs((got * y).sum(-1)).max() <= 1e-6, name
        else:
            lam = lambda x: 2 / (1 - c * (x * x).sum(-1))
            np.testing.assert_allclose(lam(y) * np.linalg.norm(got, axis=-1), lam(p) * np.linalg.norm(w, axis=-1), rtol=2e-6, err_msg=name)


# --------------------------------------------------------------------------------------------------- the C ABI
def _header():
    src = open(os.path.join(ROOT, 'include', 'sttode_hip.h')).read()
    return re.sub(r'/\*.*?\*/', '', src, flags=re.S)


def test_exports_exist_in_library_header_and_table_with_equal_arity():
    from sttode_amd import capi
    L, src = capi.lib(), _header()
    assert capi.ABI_VERSION == 15 and L.sttode_abi_version() == 15 and re.search(r'#define STTODE_ABI_VERSION 15\b', src)
    for name in ('sttode_manifold_rowop', 'sttode_riemannian_step'):
        m = re.search(r'\bint\s+%s\s*\(([^;]*?)\)\s*;' % name, src, flags=re.S)
        assert m, name + ' is not declared in include/sttode_hip.h'
        assert len([a for a in m.group(1).split(',') if a.strip()]) == len(capi.SIGNATURES[name]), name
        assert hasattr(L, name), name
    for enum, table in (('SttodeManifold', capi.MANIFOLDS), ('SttodeManifoldOp', capi.MANIFOLD_OPS), ('SttodeRiemannianRule', capi.RIEMANNIAN_RULES)):
        names = [t.strip().split('=')[0].strip() for t in re.search(r'enum %s \{(.*?)\};' % enum, src, flags=re.S).group(1).split(',')]
        assert names[-1].endswith('_COUNT') and len(names) - 1 == len(table) and sorted(table.values()) == list(range(len(table))), enum
        assert [n.split('_', 2)[2].lower() for n in names[:-1]] == list(table), enum
    assert re.search(r'#define STTODE_RIEMANNIAN_ITEM_WORDS %d\b' % capi.RIEMANNIAN_ITEM_WORDS, src)


ROWOP_OK = dict(op=0, manifold=2, a=64, b=64, w=64, out=64, out2=64, rows=1, d=1, c=1.0)
STEP_OK = dict(rule=0, table=64, n=1, total=1, lr=0.1, b1=0.9, b2=0.999, eps=1e-8, wd=0.0, mom=0.0, t=1, tstate=None)


@pytest.mark.parametrize('change, needle', [
    (dict(op=6), 'unknown op'), (dict(op=-1), 'unknown op'), (dict(manifold=3), 'unknown manifold'), (dict(manifold=-1), 'unknown manifold'),
    (dict(a=None), 'null pointer'), (dict(b=None), 'null pointer'), (dict(out=None), 'null pointer'), (dict(rows=0), 'empty shape'),
    (dict(d=0), 'empty shape'), (dict(rows=-3), 'empty shape'), (dict(op=2, w=None), 'third operand'), (dict(op=5, w=None), 'third operand'),
    (dict(op=5, out2=None), 'out2'), (dict(c=0.0), 'curvature'), (dict(c=-1.0), 'curvature'), (dict(c=float('inf')), 'curvature'),
    (dict(c=float('nan')), 'curvature')])
def test_rowop_refuses_by_name_without_a_launch(change, needle):
    """No GPU here and the pointers are not addresses: a call that got as far as a launch would fail differently or crash."""
    from sttode_amd import capi
    a = {**ROWOP_OK, **change}
    with pytest.raises(capi.SttodeError, match='sttode_manifold_rowop: .*' + needle):
        capi.call('sttode_manifold_rowop', *a.values(), None)


@pytest.mark.parametrize('change, needle', [
    (dict(rule=2), 'unknown rule'), (dict(rule=-1), 'unknown rule'), (dict(table=None), 'null table'), (dict(n=0), 'no rows'), (dict(total=0), 'no rows'),
    (dict(lr=float('nan')), 'bad lr'), (dict(lr=float('inf')), 'bad lr'), (dict(lr=-1.0), 'bad lr'), (dict(wd=float('nan')), 'weight_decay'),
    (dict(b1=1.0), 'bad beta'), (dict(b2=float('nan')), 'bad beta'), (dict(eps=float('inf')), 'bad beta or eps'), (dict(t=0), 'step count'),
    (dict(t=-1), 'step count'), (dict(rule=1, mom=float('nan')), 'bad momentum'), (dict(rule=1, mom=-0.5), 'bad momentum')])
def test_step_refuses_by_name_without_a_launch(change, needle):
    from sttode_amd import capi
    a = {**STEP_OK, **change}
    with pytest.raises(capi.SttodeError, match='sttode_riemannian_step: .*' + needle):
        capi.call('sttode_riemannian_step', *a.values(), None)


# --------------------------------------------------------------------------------------------------- the module surface
def test_module_surface_follows_the_reference():
    from sttode_amd import capi, manifolds as mf
    base = ('sqdist', 'egrad2rgrad', 'proj', 'proj_tan', 'proj_tan0', 'expmap', 'logmap', 'init_weights', 'inner', 'ptransp', 'ptransp0', 'retr',
            'retr_transp')
    assert mf.Manifold().eps == 10e-8
    for name in base:
        with pytest.raises(NotImplementedError):
            getattr(mf.Manifold(), name)(*[None] * (len(inspect.signature(getattr(mf.Manifold, name)).parameters) - 1))
    order = dict(expmap=['u', 'p'], proj_tan=['u', 'p'], ptransp=['x', 'y', 'u'], retr_transp=['x', 'u', 'v'], retr=['x', 'u'],
                 egrad2rgrad=['p', 'dp'], inner=['p', 'u', 'v', 'keepdim'], logmap=['p1', 'p2'], proj=['p'])
    for cls in (mf.Manifold, mf.Oblique, mf.PoincareBall):
        for name, args in order.items():
            assert list(inspect.signature(getattr(cls, name)).parameters)[1:] == args, (cls, name)
    assert list(inspect.signature(mf.Euclidean.ptransp).parameters)[1:] == ['x', 'y', 'v']
    assert mf.Oblique().name == 'Oblique' and mf.Euclidean().name == 'Euclidean' and mf.EPS[torch.float32] == 1e-4
    assert list(inspect.signature(mf.ManifoldParameter.__init__).parameters)[1:] == ['data', 'requires_grad', 'manifold']
    p = mf.ManifoldParameter(torch.zeros(2, 3), True, mf.Oblique())
    assert isinstance(p, torch.nn.Parameter) and p.requires_grad and isinstance(p.manifold, mf.Oblique)
    assert repr(p) == 'Oblique Parameter containing:\n' + torch.Tensor.__repr__(p) and '[0., 0., 0.]' in repr(p)
    assert repr(mf.ManifoldParameter(torch.zeros(2), False, mf.PoincareBall(0.5))).startswith('PoincareBall Parameter containing:\n')
    with pytest.raises(NotImplementedError, match=r'\[n, n\]'):
        mf.Oblique().logmap(torch.zeros(9, 16), torch.zeros(9, 16))
    with pytest.raises(NotImplementedError, match='ignores p'):
        mf.Oblique().inner(torch.zeros(9, 16), torch.zeros(9, 16))
    for bad in (0, -1.0, float('inf'), float('nan'), torch.tensor(1.0), True):
        with pytest.raises(ValueError, match='PoincareBall'):
            mf.PoincareBall(bad)
    assert mf.PoincareBall(0.5).c == 0.5 and mf.PoincareBall().c == 1.0
    # Euclidean: identities and adds, on any tensor
    e, a, b = mf.Euclidean(), torch.arange(6.).view(2, 3), torch.ones(2, 3)
    assert e.egrad2rgrad(a, b) is b and e.proj(a) is a and e.proj_tan(b, a) is b and e.ptransp(a, b, b) is b
    assert torch.equal(e.expmap(b, a), a + b) and torch.equal(e.retr(a, b), a + b) and torch.equal(e.logmap(a, b), b - a)
    assert torch.equal(e.inner(a, a, b), a.sum(-1)) and torch.equal(e.sqdist(a, b), (a - b).pow(2).sum(-1))
    y, v = e.retr_transp(a, b, a)
    assert torch.equal(y, a + b) and v is a
    # no CPU fallback, fp32 only
    z = torch.zeros(2, 4)
    for man in (mf.Oblique(), mf.PoincareBall()):
        for call in (lambda: man.proj(z), lambda: man.proj_tan(z, z) if isinstance(man, mf.Oblique) else man.egrad2rgrad(z, z),
                     lambda: man.expmap(z, z), lambda: man.ptransp(z, z, z), lambda: man.retr(z, z), lambda: man.retr_transp(z, z, z),
                     lambda: man.dist(z, z)):
            with pytest.raises(capi.SttodeError):
                call()
    with pytest.raises(capi.SttodeError):
        mf.PoincareBall().inner(z, z)
    src = open(os.path.join(ROOT, 'sttode_amd', 'manifolds.py')).read()
    assert not re.search(r'^\s*(from|import)\s+oracle', src, flags=re.M) and 'FORWARD-ONLY' in src


def test_optimisers_refuse_unknown_manifolds_and_unsupported_tensors():
    from sttode_amd import manifolds as mf, optim

    class Lorentz(mf.Manifold):
        def __init__(self):
            super().__init__()
            self.name = 'Lorentz'
    p = mf.ManifoldParameter(torch.zeros(3, 4), True, Lorentz())
    for make in (lambda ps: optim.RiemannianAdam(ps), lambda ps: optim.RiemannianSGD(ps, lr=0.1)):
        with pytest.raises(ValueError, match='Lorentz'):
            make([p])
        opt = make([torch.nn.Parameter(torch.zeros(2))])
        with pytest.raises(ValueError, match='Lorentz'):
            opt.add_param_group(dict(params=[p]))
        # CPU tensors, float64 tensors: refused at the first step, not stepped by a slow path
        for q in (mf.ManifoldParameter(torch.ones(3, 4), True, mf.Oblique()), torch.nn.Parameter(torch.ones(3, 4))):
            q.grad = torch.ones_like(q)
            with pytest.raises(ValueError, match='cpu'):
                make([q]).step()
            assert torch.equal(q.detach(), torch.ones(3, 4))
    for kw in (dict(amsgrad=True), dict(max_grad_norm=1.0), dict(skip_nonfinite=True)):
        with pytest.raises(TypeError):
            optim.RiemannianAdam([torch.nn.Parameter(torch.zeros(2))], **kw)
    for kw in (dict(nesterov=True), dict(dampening=0.1)):
        with pytest.raises(TypeError):
            optim.RiemannianSGD([torch.nn.Parameter(torch.zeros(2))], lr=0.1, **kw)
    assert list(inspect.signature(optim.RiemannianAdam.__init__).parameters)[1:] == ['params', 'lr', 'betas', 'eps', 'weight_decay']
    assert list(inspect.signature(optim.RiemannianSGD.__init__).parameters)[1:] == ['params', 'lr', 'momentum', 'weight_decay']
    d = optim.RiemannianAdam([torch.nn.Parameter(torch.zeros(2))]).defaults
    assert d == dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0)
    # a ManifoldParameter on the Euclidean manifold is a plain parameter
    optim.RiemannianAdam([mf.ManifoldParameter(torch.zeros(2), True, mf.Euclidean())])


def test_state_dict_of_a_fresh_optimiser_and_a_loaded_state():
    """Without a GPU: the state layout (keys and shapes) that load_state_dict takes and state_dict gives back."""
    from sttode_amd import manifolds as mf, optim
    p = mf.ManifoldParameter(torch.zeros(2, 3, 5), True, mf.PoincareBall(0.5))
    q = torch.nn.Parameter(torch.zeros(7))
    opt = optim.RiemannianAdam([p, q], lr=0.01)
    sd = opt.state_dict()
    assert sd['state'] == {} and sd['param_groups'][0]['params'] == [0, 1] and sd['param_groups'][0]['lr'] == 0.01
    state = {0: dict(step=torch.tensor(3.0), exp_avg=torch.ones(2, 3, 5), exp_avg_sq=torch.ones(2, 3, 1)),
             1: dict(step=torch.tensor(3.0), exp_avg=torch.ones(7), exp_avg_sq=torch.ones(7))}
    opt.load_state_dict(dict(state=state, param_groups=sd['param_groups']))
    back = opt.state_dict()['state']
    assert set(back[0]) == set(back[1]) == {'step', 'exp_avg', 'exp_avg_sq'}
    assert back[0]['exp_avg'].shape == (2, 3, 5) and back[0]['exp_avg_sq'].shape == (2, 3, 1) and float(back[0]['step']) == 3.0
    sgd = optim.RiemannianSGD([p, q], lr=0.1, momentum=0.9)
    sd = sgd.state_dict()
    sgd.load_state_dict(dict(state={0: dict(momentum_buffer=torch.ones(2, 3, 5))}, param_groups=sd['param_groups']))
    assert sgd.state_dict()['state'][0]['momentum_buffer'].shape == (2, 3, 5) and sgd.state_dict()['param_groups'][0]['momentum'] == 0.9
