"""GPU tests of the opt-in gradients through poincare_mean, the Oblique entry points and the manifold operations (DESIGN.md 4y;
csrc/pmath_grad.hip, csrc/manifold.hip through sttode_amd.pmath and sttode_amd.manifolds).

Yardstick: tests/golden/manifold_grad.npz -- the reference's own functions differentiated by torch autograd in float64 on the float32
inputs -- and, for the ball's egrad2rgrad / inner / ptransp / retr, which the reference does not have, tests/riemannian_ref.py
differentiated by CPU autograd in float64 here.  Metric: max |got - ref| / (1 + |ref|).  Two bounds, as test_riemannian_gpu.py: hard
<= 1e-4 (pmath_vjp_cases.BOUND), tight <= max(8 x the yardstick's own float32 error, 1e-6).

Measured on the MI355X: DESIGN.md 4y, profiles/manifold_grad/gputests.txt.
"""
import numpy as np
import pytest
import torch

import manifold_grad_cases as mc
import riemannian_ref as rr
from pmath_vjp_cases import BOUND

pytestmark = pytest.mark.gpu

FACTOR, FLOOR = 8.0, 1e-6


@pytest.fixture(scope='module')
def fx(golden):
    return rr.Fixture(golden('manifold_grad'), golden('riemannian_ops'))


@pytest.fixture(scope='module')
def mean(fx):
    return mc.MeanFixture(fx)


def _dev():
    assert torch.cuda.is_available(), 'these tests need the GPU'
    return torch.device('cuda:0')


def _d(a, grad=False):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev()).requires_grad_(grad)


def _man(name, c, diff=True):
    from sttode_amd import manifolds as mf
    man = mf.Oblique() if name == 'oblique' else mf.PoincareBall(c)
    return mf.differentiable(man) if diff else man


class Tally:
    """Worst error per key of the kernel and of the yardstick's float32 run, both against the float64 run."""

    def __init__(self):
        self.hip, self.ora, self.bad = {}, {}, []

    def add(self, key, got, r64, r32, what):
        got, r64, r32 = got.detach().cpu().numpy(), np.asarray(r64), np.asarray(r32)
        assert got.dtype == np.float32 and got.shape == r64.shape == r32.shape, (what, got.dtype, got.shape, r64.shape, r32.shape)
        assert np.isfinite(r64).all(), what
        assert np.isfinite(got).all(), what + ': not finite where the yardstick is'
        e = rr.err(got, r64)
        self.hip[key] = max(self.hip.get(key, 0.0), e)
        self.ora[key] = max(self.ora.get(key, 0.0), rr.err(r32, r64))
        if not e <= BOUND:
            self.bad.append((what, e))

    def check(self):
        for key in sorted(self.hip):
            print('%-34s worst error %.2e   (yardstick fp32: %.2e)' % (key, self.hip[key], self.ora[key]))
        assert not self.bad, ('outside the hard bound', self.bad)
        loose = [(k, self.hip[k], self.ora[k]) for k in sorted(self.hip) if not self.hip[k] <= max(FACTOR * self.ora[k], FLOOR)]
        assert not loose, ('outside the tight bound max(8 x yardstick fp32, 1e-6): (op, kernel, yardstick fp32)', loose)


def _grads(outs, operands, gs):
    """The gradients of sum_k <g_k, out_k> with respect to the operands; an operand the graph does not reach gets zeros."""
    gr = torch.autograd.grad(list(outs), operands, grad_outputs=[g.reshape(o.shape) for o, g in zip(outs, gs)], allow_unused=True)
    return [torch.zeros_like(t) if g is None else g for g, t in zip(gr, operands)]


def _obl_run(man, op, p, y, u, w):
    t = dict(p=p, y=y, u=u, w=w)
    res = {'proj': lambda: (man.proj(w),), 'proj_tan': lambda: (man.proj_tan(u, p),), 'expmap': lambda: (man.expmap(u, p),),
           'ptransp': lambda: (man.ptransp(p, y, w),), 'retr_transp': lambda: man.retr_transp(p, u, w)}[op]()
    return res, [t[k] for k in mc.OBL_OPERANDS[op]]


# --------------------------------------------------------------------------------------------------- 1. gradients against the yardstick
def test_oblique_row_op_gradients(fx):
    """d in {2, 16, 63, 64, 65, 130, 300} x rows in {1, 5, 9}; the zero-u row of expmap (the proj(p + u) branch as taken)."""
    tally, man = Tally(), _man('oblique', 1.0)
    cases = [(name, fx[key], mc.OBL_OPS) for name, key, d in mc.obl_cases()] + [('obl.edge', fx['obl.edge.in'], ('expmap', 'retr_transp'))]
    for name, ins, ops in cases:
        for rows in rr.ROWS:
            for op in ops:
                outs, operands = _obl_run(man, op, *[_d(a[:rows], True) for a in ins])
                assert all(o.requires_grad for o in outs)
                gs = [_d(g[:rows]) for g in fx[name + '.g']]
                for k, got in zip(mc.OBL_OPERANDS[op], _grads(outs, operands, gs)):
                    i = mc.OBL_OPERANDS[op].index(k)
                    tally.add('oblique %s d/d%s' % (op, k), got, fx['%s.%s.grads64' % (name, op)][i, :rows], fx['%s.%s.grads32' % (name, op)][i, :rows],
                              '%s rows %d %s d/d%s' % (name, rows, op, k))
    # egrad2rgrad is proj_tan; retr is the first result of retr_transp (its second upstream gradient NULL: zero)
    p, y, u, w = [_d(a, True) for a in fx['op.obl.d65.in']]
    g = _d(fx['obl.d65.g'][0])
    a = _grads([man.egrad2rgrad(p, u)], [u, p], [g])
    b = _grads([man.proj_tan(u, p)], [u, p], [g])
    assert all(torch.equal(s, t) for s, t in zip(a, b))
    ry, rv = man.retr_transp(p, u, w)
    a = _grads([ry], [p, u], [g])
    b = _grads([man.retr(p, u)], [p, u], [g])
    assert all(torch.equal(s, t) for s, t in zip(a, b)) and torch.equal(man.retr(p, u), ry)
    tally.check()


def test_ball_row_op_gradients(fx):
    """d in {1, 2, 16, 63, 64, 65, 130, 300} x rows in {1, 5, 9} x c in {1, 0.5}, and a case on both sides of project's clip; the yardstick
    is riemannian_ref.BallRef under CPU autograd, float64 and float32."""
    tally = Tally()
    cases = [(name, c, fx[name + '.in']) for name, mname, c, d in rr.op_shapes() if mname == 'poincare']
    cases += [('clip.c%s' % c, c, mc.ball_clip_case(c)) for c in mc.CS]
    for name, c, ins in cases:
        man, ref = _man('poincare', c), rr.BallRef(c)
        with torch.no_grad():       # no retraction within 1e-4 (relative) of project's clip radius: the branch is unambiguous
            e = ref.expmap(torch.from_numpy(ins[2]).double(), torch.from_numpy(ins[0]).double()).norm(dim=-1).numpy()
        assert (np.abs(e * np.sqrt(c) / (1 - 1e-3) - 1) > 1e-4).all(), name
        for rows in rr.ROWS if not name.startswith('clip') else (9,):
            sub = [a[:rows] for a in ins]
            for op in mc.BALL_OPS:
                two = op == 'retr_transp'
                shape = (rows,) if op == 'inner' else sub[0].shape
                gs = [mc.upstream('%s.%s.%d' % (name, op, k), shape) for k in range(2 if two else 1)]
                r64, r32 = [mc.vjp(lambda *t: mc.ball_run(ref, op, *t), sub, gs, dt) for dt in (torch.float64, torch.float32)]
                outs, operands = mc.ball_run(man, op, *[_d(a, True) for a in sub])
                for o, o64, o32 in zip(outs, r64[0], r32[0]):
                    tally.add('poincare %s value' % op, o, o64, o32, '%s rows %d %s value' % (name, rows, op))
                for k, got, g64, g32 in zip(mc.BALL_OPERANDS[op], _grads(outs, operands, [_d(g) for g in gs]), r64[1], r32[1]):
                    key = 'poincare %s d/d%s%s' % (op, k, ' (clip)' if name.startswith('clip') else '')
                    tally.add(key, got, g64, g32, '%s rows %d %s d/d%s' % (name, rows, op, k))
    tally.check()


def test_ball_routed_ops_only_stop_detaching(fx):
    """proj / expmap / logmap / dist / sqdist of a differentiable ball are pmath's differentiable functions; proj_tan is the identity."""
    from sttode_amd import pmath
    c = 0.5
    ins = fx['op.ball.d16.c0.5.in']
    man = _man('poincare', c)
    g, gs = _d(mc.upstream('routed', (9, 16))), _d(mc.upstream('routed.s', (9,)))
    for got, want, up in (
            (lambda p, y, u: man.proj(p * 3), lambda p, y, u: pmath.project(p * 3, c=c), g),
            (lambda p, y, u: man.expmap(u, p), lambda p, y, u: pmath.expmap(p, u, c=c), g),
            (lambda p, y, u: man.logmap(p, y), lambda p, y, u: pmath.logmap(y, p, c=c), g),
            (lambda p, y, u: man.dist(p, y), lambda p, y, u: pmath.dist(p, y, c=c), gs),
            (lambda p, y, u: man.sqdist(p, y), lambda p, y, u: pmath.dist(p, y, c=c).pow(2), gs),
            (lambda p, y, u: man.proj_tan(u, p) * 2, lambda p, y, u: u * 2, g),
            (lambda p, y, u: man.proj_tan0(u) * 2, lambda p, y, u: u * 2, g)):
        res = []
        for fn in (got, want):
            p, y, u = [_d(a, True) for a in ins[:3]]
            out = fn(p, y, u)
            res.append([out] + _grads([out], [p, y, u], [up]))
        assert res[0][0].requires_grad and all(torch.equal(a, b) for a, b in zip(*res))


def test_oblique_proj_and_dist_gradients(fx):
    from sttode_amd import pmath
    tally = Tally()
    for nb, n1, n2, d in mc.OBL_DIST:
        name = 'dist.%d.%d.%d.%d' % (nb, n1, n2, d)
        p1, p2 = _d(fx[name + '.p1'], True), _d(fx[name + '.p2'], True)
        out = pmath.oblique_dist(p1, p2, differentiable=True)
        assert out.shape == (nb, n2, n1) and out.requires_grad and torch.equal(out, pmath.oblique_dist(p1, p2))
        tally.add('oblique_dist value', out, fx[name + '.out64'], fx[name + '.out32'], name)
        g1, g2 = _grads([out], [p1, p2], [_d(fx[name + '.g'])])
        tally.add('oblique_dist d/dp1', g1, fx[name + '.g164'], fx[name + '.g132'], name)
        tally.add('oblique_dist d/dp2', g2, fx[name + '.g264'], fx[name + '.g232'], name)
        man = _man('oblique', 1.0)
        assert all(torch.equal(a, b) for a, b in zip(_grads([man.dist(p1, p2)], [p1, p2], [_d(fx[name + '.g'])]), (g1, g2)))
        (only2,) = torch.autograd.grad(pmath.oblique_dist(p1.detach(), p2, differentiable=True), [p2], _d(fx[name + '.g']))
        assert torch.equal(only2, g2)
        if (nb, n1, n2, d) == mc.OBL_DIST_SPECIAL:
            # the identical and the antipodal pair are clamped: their contribution is exactly zero, so the gradient is the sum without them
            g = fx[name + '.g'].copy()
            g[0, 0, 0] = g[0, 1, 1] = 0
            h1, h2 = _grads([pmath.oblique_dist(p1, p2, differentiable=True)], [p1, p2], [_d(g)])
            assert torch.equal(h1, g1) and torch.equal(h2, g2)
    # oblique_proj: the rows of the fixture's Oblique cases (w, off the sphere), through pmath and through the manifold
    for name, key, d in mc.obl_cases():
        w = _d(fx[key][3], True)
        out = pmath.oblique_proj(w, differentiable=True)
        assert torch.equal(out, pmath.oblique_proj(w)) and out.requires_grad
        (gw,) = _grads([out], [w], [_d(fx[name + '.g'][0])])
        tally.add('oblique_proj d/dp', gw, fx[name + '.proj.grads64'][0], fx[name + '.proj.grads32'][0], name)
    z = torch.zeros(3, 16, device=_dev())
    z[1] = 1.0
    z.requires_grad_()
    (gz,) = _grads([pmath.oblique_proj(z, differentiable=True)], [z], [torch.ones_like(z)])
    assert torch.isnan(gz[0]).all() and torch.isnan(gz[2]).all() and torch.isfinite(gz[1]).all()      # a zero row: NaN, as the forward
    tally.check()


# --------------------------------------------------------------------------------------------------- 2. poincare_mean: values, gradients
def test_poincare_mean_values_and_gradients(mean):
    """[R, W, d] over R in {1, 2, 9}, W in {1, 5}, d in {1, 2, 16, 65, 130}, dim in {0, 1}, c in {1, 0.5}; [2, 3, 2, 16] over dim 1; the
    group x, -x and the zero row.  Forward bits with the flag equal those without; a group is bitwise the 2-D call on its rows."""
    from sttode_amd import pmath
    tally = Tally()
    for name, shape, dim, c in mc.mean_cases():
        rec = mean[name]
        x = _d(rec['x'], True)
        out = pmath.poincare_mean(x, dim=dim, c=c, differentiable=True)
        plain = pmath.poincare_mean(x, dim=dim, c=c)
        assert out.requires_grad and not plain.requires_grad and torch.equal(out, plain) and out.shape == rec['out64'].shape, name
        assert torch.equal(pmath.poincare_mean(x, dim=dim - len(shape), c=c), plain), name
        tally.add('poincare_mean value', out, rec['out64'], rec['out32'], name)
        (gx,) = _grads([out], [x], [_d(rec['g'])])
        tally.add('poincare_mean d/dx', gx, rec['gx64'], rec['gx32'], name)
        # a tensor c: the same bits, and its gradient
        ct = torch.tensor([c], device=_dev(), requires_grad=True)
        out_c = pmath.poincare_mean(x, dim=dim, c=ct, differentiable=True)
        assert torch.equal(out_c, plain), name
        gx_c, gc = _grads([out_c], [x, ct], [_d(rec['g'])])
        assert torch.equal(gx_c, gx) and gc.shape == (1,), name
        tally.add('poincare_mean d/dc c%s' % c, gc, rec['gc64'], rec['gc32'], name)
        (gc_only,) = torch.autograd.grad(pmath.poincare_mean(x.detach(), dim=dim, c=ct, differentiable=True), [ct], _d(rec['g']))
        assert torch.equal(gc_only, gc), name
        if len(shape) == 3:
            xs = x.detach().movedim(dim, 0)
            for w in range(xs.shape[1]):
                assert torch.equal(plain[w], pmath.poincare_mean(xs[:, w].contiguous(), dim=0, c=c)), (name, w)
    tally.check()
    from sttode_amd import capi
    for dim in (-1, 3):
        with pytest.raises(capi.SttodeError, match='last .feature. dimension'):
            pmath.poincare_mean(_d(mean['mean.r4.c1.0.dim1']['x']), dim=dim)


def test_shared_curvature_gets_the_sum_of_both_contributions(mean):
    from sttode_amd import pmath
    rec = mean['mean.R9.W5.d16.c0.5.dim0']
    x, g = _d(rec['x']), _d(rec['g'])
    q = _d(mc.upstream('queries', (7, 16)) * np.float32(0.1))
    gd = _d(mc.upstream('queries.g', (7, 5)))

    def run(c_mean, c_dist):
        protos = pmath.poincare_mean(x, dim=0, c=c_mean, differentiable=True)
        return (protos * g).sum() + (pmath.dist_matrix(q, protos.detach(), c=c_dist) * gd).sum()
    c = torch.nn.Parameter(torch.tensor([0.5], device=_dev()))
    run(c, c).backward()
    a, b = [torch.tensor([0.5], device=_dev(), requires_grad=True) for _ in range(2)]
    run(a, b).backward()
    assert a.grad.abs().item() > 0 and b.grad.abs().item() > 0 and torch.equal(c.grad, a.grad + b.grad)
    assert rr.err(a.grad.cpu().numpy(), rec['gc64']) <= BOUND


# --------------------------------------------------------------------------------------------------- 3. the default is untouched
def test_defaults_are_untouched(fx, mean):
    from sttode_amd import capi, pmath
    x = _d(mean['mean.R9.W5.d16.c1.0.dim0']['x'], True)
    assert not pmath.poincare_mean(x, dim=0, c=1.0).requires_grad and not pmath.oblique_proj(x).requires_grad
    assert not pmath.oblique_dist(x, x).requires_grad
    with torch.no_grad():
        assert not pmath.poincare_mean(x, dim=0, c=1.0, differentiable=True).requires_grad
    with pytest.raises(capi.SttodeError, match='poincare_mean.*forward-only'):
        pmath.poincare_mean(x, c=torch.tensor([1.0], device=_dev()))
    for bad in (torch.tensor([1.0], dtype=torch.float64, device=_dev()), torch.tensor([1.0, 1.0], device=_dev()), torch.tensor([1.0])):
        with pytest.raises(capi.SttodeError, match='1-element float32 tensor on the inputs'):
            pmath.poincare_mean(x, c=bad, differentiable=True)
    for mname, c, key in (('oblique', 1.0, 'op.obl.d16.in'), ('poincare', 0.5, 'op.ball.d16.c0.5.in')):
        plain, diff = _man(mname, c, False), _man(mname, c)
        ins = [_d(a, True) for a in fx[key]]
        p, y, u, w = ins
        calls = [lambda m: m.proj(w), lambda m: m.egrad2rgrad(p, u), lambda m: m.expmap(u, p), lambda m: m.dist(p, y), lambda m: m.ptransp(p, y, w),
                 lambda m: m.retr(p, u), lambda m: m.retr_transp(p, u, w)[1], lambda m: m.proj_tan(u, p)]
        if mname == 'poincare':
            calls += [lambda m: m.inner(p, u, w), lambda m: m.logmap(p, y), lambda m: m.sqdist(p, y), lambda m: m.proj_tan0(u)]
        for call in calls:
            base = call(plain)
            assert not base.requires_grad                                       # the plain manifold: forward-only, whatever the operands ask
            assert call(diff).requires_grad and torch.equal(call(diff), base)  # the flag: a graph, the same bits
            with torch.no_grad():
                out = call(diff)
            assert not out.requires_grad and torch.equal(out, base)
        detached = [t.detach() for t in ins]
        assert not diff.retr(detached[0], detached[2]).requires_grad           # no operand asks: the forward-only call


# --------------------------------------------------------------------------------------------------- 4. repeatability
def test_backward_passes_repeat_bit_for_bit_and_rows_are_independent(fx, mean):
    from sttode_amd import pmath

    def twice(fn):
        a, b = fn(), fn()
        assert all(torch.equal(s, t) for s, t in zip(a, b))
        return a
    # poincare_mean: appending a group leaves the other groups' gradients unchanged
    rec = mean['mean.R9.W5.d65.c0.5.dim0']
    for c in (0.5, torch.tensor([0.5], device=_dev(), requires_grad=True)):
        def run(W):
            x = _d(rec['x'][:, :W], True)
            out = pmath.poincare_mean(x, dim=0, c=c, differentiable=True)
            return _grads([out], [x] + ([c] if isinstance(c, torch.Tensor) else []), [_d(rec['g'][:W])])
        full, part = twice(lambda: run(5)), twice(lambda: run(4))
        assert torch.equal(full[0][:, :4], part[0])
    # the manifold row ops: appending rows leaves the other rows' gradients unchanged
    for mname, c, key in (('oblique', 1.0, 'op.obl.d130.in'), ('poincare', 0.5, 'op.ball.d130.c0.5.in')):
        man = _man(mname, c)
        g = [mc.upstream('rep.%d' % k, (9, 130)) for k in range(2)]

        def run(rows, op):
            p, y, u, w = [_d(a[:rows], True) for a in fx[key]]
            outs = {'egrad2rgrad': lambda: (man.egrad2rgrad(p, u),), 'expmap': lambda: (man.expmap(u, p),), 'ptransp': lambda: (man.ptransp(p, y, w),),
                    'retr': lambda: (man.retr(p, u),), 'retr_transp': lambda: man.retr_transp(p, u, w)}[op]()
            return _grads(outs, [p, y, u, w], [_d(a[:rows]) for a in g])
        for op in ('egrad2rgrad', 'expmap', 'ptransp', 'retr', 'retr_transp'):
            full, part = twice(lambda: run(9, op)), twice(lambda: run(5, op))
            assert all(torch.equal(a[:5], b) for a, b in zip(full, part)), (mname, op)
    # oblique_dist: appending a batch
    p1, p2, g = fx['dist.2.3.7.65.p1'], fx['dist.2.3.7.65.p2'], fx['dist.2.3.7.65.g']

    def run(nb):
        a, b = _d(p1[:nb], True), _d(p2[:nb], True)
        return _grads([pmath.oblique_dist(a, b, differentiable=True)], [a, b], [_d(g[:nb])])
    full, part = twice(lambda: run(2)), twice(lambda: run(1))
    assert all(torch.equal(a[:1], b) for a, b in zip(full, part))

    def run_proj():
        w = _d(fx['op.obl.d65.in'][3], True)
        return _grads([pmath.oblique_proj(w, differentiable=True)], [w], [_d(fx['obl.d65.g'][0])])
    twice(run_proj)


# --------------------------------------------------------------------------------------------------- 5. refusals
def test_a_refused_call_leaves_its_outputs_untouched(fx):
    from sttode_amd import capi
    p, y, u, w = [_d(a) for a in fx['op.ball.d16.c1.0.in']]
    st = capi.stream_ptr()
    outs = [torch.full_like(p, 7.0) for _ in range(4)]
    ga, gb, gw, out = outs
    wsd = torch.full((9 * 16 + 64,), 7.0, dtype=torch.float64, device=p.device)
    gc = torch.full((1,), 7.0, device=p.device)
    c_dev = torch.tensor([1.0], device=p.device)
    refused = (
        ('sttode_manifold_rowop_bwd', (5, 2, p, u, w, y, y, ga, gb, gw, 9, 16, -1.0)),
        ('sttode_manifold_rowop_bwd', (5, 2, p, u, None, y, y, ga, gb, gw, 9, 16, 1.0)),
        ('sttode_manifold_rowop_bwd', (9, 2, p, u, w, y, None, ga, gb, gw, 9, 16, 1.0)),
        ('sttode_manifold_rowop_bwd', (5, 3, p, u, w, y, y, ga, gb, gw, 9, 16, 1.0)),
        ('sttode_manifold_rowop_bwd', (5, 2, p, u, w, None, None, ga, gb, gw, 9, 16, 1.0)),
        ('sttode_manifold_rowop_bwd', (1, 2, p, u, w, y, y, ga, gb, gw, 9, 16, 1.0)),
        ('sttode_manifold_rowop_bwd', (1, 2, p, u, w, y, None, ga, gb, gw, 0, 16, 1.0)),
        ('sttode_manifold_rowop_bwd', (1, 2, p, u, w, y, None, ga, gb, gw, 9, 16, float('inf'))),
        ('sttode_pmath_mean_seg', (p, ga, gb, out, None, None, 1, 9, 1, 16, 0.0, None)),
        ('sttode_pmath_mean_seg', (p, ga, gb, out, None, None, 1, 9, 0, 16, 1.0, None)),
        ('sttode_pmath_mean_seg', (None, ga, gb, out, None, None, 1, 9, 1, 16, 1.0, None)),
        ('sttode_pmath_mean_bwd', (p, y, wsd, wsd, ga, 1, 9, 1, 16, -1.0)),
        ('sttode_pmath_mean_bwd', (p, y, wsd, wsd, ga, 1, 9, 1, 0, 1.0)),
        ('sttode_pmath_mean_bwd', (p, None, wsd, wsd, ga, 1, 9, 1, 16, 1.0)),
        ('sttode_pmath_mean_bwd_c', (p, y, wsd, wsd, ga, 1, 9, 1, 16, None, wsd, gc)),
        ('sttode_pmath_mean_bwd_c', (p, y, wsd, wsd, ga, 1, 9, 1, 16, c_dev, None, gc)),
        ('sttode_pmath_mean_bwd_c', (p, y, wsd, wsd, ga, 0, 9, 1, 16, c_dev, wsd, gc)),
        ('sttode_oblique_proj_bwd', (p, None, ga, 9, 16)),
        ('sttode_oblique_proj_bwd', (p, y, ga, 9, 0)),
        ('sttode_oblique_dist_bwd', (p, y, None, ga, gb, 1, 9, 9, 16)),
        ('sttode_oblique_dist_bwd', (p, y, u, ga, gb, 1, 9, 0, 16)),
    )
    for name, args in refused:
        with pytest.raises(capi.SttodeError, match=name + ':'):
            capi.call(name, *args, st)
    torch.cuda.synchronize()
    assert all(bool((t == 7.0).all()) for t in outs + [wsd, gc])


# --------------------------------------------------------------------------------------------------- 6. it trains
def _prototype_head(dev):
    """Embeddings [shot 5, way 4, d 16] -> ToPoincare -> poincare_mean over the shots -> -dist_matrix to fixed queries -> cross-entropy."""
    from sttode_amd import hypnn, pmath
    rng = np.random.default_rng(mc.SEED)
    centres = rng.standard_normal((4, 16))
    centres *= 1.5 / np.linalg.norm(centres, axis=-1, keepdims=True)
    emb = torch.nn.Parameter(_d((0.1 * rng.standard_normal((5, 4, 16))).astype(np.float32)))
    labels = torch.arange(12, device=dev) % 4
    tp = hypnn.ToPoincare(c=1.0).to(dev)
    with torch.no_grad():
        queries = tp(_d((centres[np.arange(12) % 4] + 0.1 * rng.standard_normal((12, 16))).astype(np.float32)))

    def loss_fn():
        protos = pmath.poincare_mean(tp(emb), dim=0, c=1.0, differentiable=True)
        return torch.nn.functional.cross_entropy(-pmath.dist_matrix(queries, protos, c=1.0), labels), protos
    return emb, loss_fn


def test_a_prototype_head_trains():
    import sttode_amd.pmath as pm
    dev = _dev()
    try:
        emb, loss_fn = _prototype_head(dev)
        opt = torch.optim.Adam([emb], lr=0.05)
        losses = []
        for _ in range(30):
            opt.zero_grad()
            loss, protos = loss_fn()
            loss.backward()
            assert emb.grad is not None and torch.isfinite(emb.grad).all() and emb.grad.abs().max() > 0
            opt.step()
            losses.append(loss.item())
        loss, protos = loss_fn()
        print('prototype head: loss %.4f -> %.4f' % (losses[0], loss.item()))
        assert loss.item() < 0.5 * losses[0], losses
        assert float(protos.detach().norm(dim=-1).max()) <= 1 - 1e-3 + 1e-6      # inside project's radius at c = 1
    finally:
        pm.RiemannianGradient.c = 1


def test_an_oblique_parameter_trains_through_the_manifolds_own_dist():
    from sttode_amd import manifolds as mf, optim
    rng = np.random.default_rng(mc.SEED + 1)
    unit = lambda: (lambda v: (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(np.float32))(rng.standard_normal((9, 16)))   # noqa: E731
    man = mf.differentiable(mf.Oblique())
    p = mf.ManifoldParameter(_d(unit()), True, man)
    target = _d(unit())
    opt = optim.RiemannianAdam([p], lr=0.05)
    losses = []
    for _ in range(30):
        opt.zero_grad()
        loss = man.dist(p, target).mean()
        loss.backward()
        opt.step()
        losses.append(loss.item())
    final = man.dist(p, target).mean().item()
    print('oblique parameter: loss %.4f -> %.4f' % (losses[0], final))
    assert final < losses[0] and torch.isfinite(p).all()
    assert float((p.detach().double().norm(dim=-1) - 1).abs().max()) <= 1e-6


def test_a_captured_backward_replays_with_equal_bits():
    """No host read on the path: forward + backward of the prototype head captured in a HIP graph; the replay's gradient is the eager one."""
    import sttode_amd.pmath as pm
    dev = _dev()
    try:
        emb, loss_fn = _prototype_head(dev)
        (eager,) = torch.autograd.grad(loss_fn()[0], [emb])
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            torch.autograd.grad(loss_fn()[0], [emb])          # warm-up outside the capture
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            (captured,) = torch.autograd.grad(loss_fn()[0], [emb])
        captured.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.isfinite(captured).all() and torch.equal(captured, eager)
    finally:
        pm.RiemannianGradient.c = 1
