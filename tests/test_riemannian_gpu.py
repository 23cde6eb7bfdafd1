"""GPU tests of the manifold row operations and the Riemannian optimisers (csrc/manifold.hip through sttode_amd.manifolds and
sttode_amd.optim.RiemannianAdam / RiemannianSGD).

Yardstick: tests/golden/riemannian.npz / riemannian_ops.npz -- the float64 run, on the float32 inputs, of the reference's own Oblique and
hyptorch.pmath functions under the loops of riemannian_ref.py.  Metric: max |got - ref| / (1 + |ref|).  Ops carry the two bounds of
test_pmath_forward_gpu.py: hard <= 1e-4 (pmath_vjp_cases.BOUND), tight <= max(8 x the yardstick's own float32 error, 1e-6); NaN positions the
yardstick's, finite wherever it is.  Optimiser trajectories: parameters and both state buffers after each of the 8 steps <= 1e-4.

Measured on the MI355X: DESIGN.md 4u, profiles/riemannian/gputests.txt.
"""
import numpy as np
import pytest
import torch

import riemannian_ref as rr
from pmath_vjp_cases import BOUND

pytestmark = pytest.mark.gpu

FACTOR, FLOOR = 8.0, 1e-6


@pytest.fixture(scope='module')
def fx(golden):
    return rr.Fixture(golden('riemannian'), golden('riemannian_ops'))


def _dev():
    assert torch.cuda.is_available(), 'these tests need the GPU'
    return torch.device('cuda:0')


def _d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _man(name, c):
    from sttode_amd import manifolds as mf
    return mf.Oblique() if name == 'oblique' else mf.PoincareBall(c)


class Tally:
    """Worst error per (manifold, op) of the kernel and of the yardstick's float32 run, both against the float64 run."""

    def __init__(self):
        self.hip, self.ora, self.bad = {}, {}, []

    def add(self, key, got, r64, r32, what):
        got, r64, r32 = got.cpu().numpy(), np.asarray(r64), np.asarray(r32)
        assert got.dtype == np.float32 and got.shape == r64.shape == r32.shape, (what, got.dtype, got.shape, r64.shape)
        assert np.isfinite(r64).all(), what
        assert np.isfinite(got).all(), what + ': not finite where the yardstick is'
        e = rr.err(got, r64)
        self.hip[key] = max(self.hip.get(key, 0.0), e)
        self.ora[key] = max(self.ora.get(key, 0.0), rr.err(r32, r64))
        if not e <= BOUND:
            self.bad.append((what, e))

    def check(self):
        for key in sorted(self.hip):
            print('%-28s worst error %.2e   (yardstick fp32: %.2e)' % ('%s %s' % key, self.hip[key], self.ora[key]))
        assert not self.bad, ('outside the hard bound', self.bad)
        loose = [(k, self.hip[k], self.ora[k]) for k in sorted(self.hip) if not self.hip[k] <= max(FACTOR * self.ora[k], FLOOR)]
        assert not loose, ('outside the tight bound max(8 x yardstick fp32, 1e-6): (op, kernel, yardstick fp32)', loose)


def _ops(tally, man, mname, ins, out64, out32, inner64, inner32, what):
    """Every operation of one case through the public module."""
    p, y, u, w = ins
    results = dict(zip(rr.OP_NAMES, range(len(rr.OP_NAMES))))
    ry, rv = man.retr_transp(p, u, w)
    got = {'proj_tan': man.egrad2rgrad(p, u), 'expmap': man.expmap(u, p), 'ptransp': man.ptransp(p, y, w), 'retr_transp.y': ry,
           'retr_transp.v': rv}
    for op, i in results.items():
        assert not got[op].requires_grad
        tally.add((mname, op), got[op], out64[i], out32[i], what + ' ' + op)
    assert torch.equal(man.retr(p, u), ry), what + ': retr and the point of retr_transp differ'
    if mname == 'oblique':
        assert torch.equal(man.proj_tan(u, p), got['proj_tan']), what
    else:
        tally.add((mname, 'inner'), man.inner(p, u, w), inner64, inner32, what + ' inner')
        assert torch.equal(man.proj_tan(u, p), u), what


# --------------------------------------------------------------------------------------------------- 1. row ops
def test_row_ops_at_every_fixture_case(fx):
    """d in {1, 2, 16, 63, 64, 65, 130, 300} (one, two and five trips of the lane loop, +-1) x rows in {1, 5, 9} (every remainder of the
    four-rows-per-block grid) x c in {1, 0.5}; the two branches of Oblique.expmap (a zero u gives p); broadcast operands."""
    tally, n = Tally(), 0
    for name, mname, c, d in rr.op_shapes():
        ins = _d(fx[name + '.in'])
        for rows in rr.ROWS:
            ball = mname == 'poincare'
            _ops(tally, _man(mname, c), mname, [t[:rows] for t in ins], fx[name + '.out64'][:, :rows], fx[name + '.out32'][:, :rows],
                 fx[name + '.inner64'][:rows] if ball else None, fx[name + '.inner32'][:rows] if ball else None, '%s rows %d' % (name, rows))
            n += 1
    assert n == len(rr.op_cases()) == 69
    from sttode_amd import manifolds as mf
    ins = _d(fx['op.obl.edge.in'])
    _ops(tally, mf.Oblique(), 'oblique', ins, fx['op.obl.edge.out64'], fx['op.obl.edge.out32'], None, None, 'op.obl.edge')
    got = mf.Oblique().expmap(ins[2], ins[0]).cpu().numpy()
    assert not ins[2][4].any() and np.abs(got[4] - fx['op.obl.edge.in'][0][4]).max() <= 1e-6, 'a zero u must return p'
    ins = [_d(fx['op.ball.bcast.' + k]) for k in 'pyuw']
    _ops(tally, mf.PoincareBall(1.0), 'poincare', ins, fx['op.ball.bcast.out64'], fx['op.ball.bcast.out32'], fx['op.ball.bcast.inner64'],
         fx['op.ball.bcast.inner32'], 'op.ball.bcast')
    assert mf.PoincareBall(1.0).inner(ins[0], ins[2], keepdim=True).shape == (2, 3, 1)
    tally.check()
    assert set(tally.hip) == {('oblique', op) for op in rr.OP_NAMES} | {('poincare', op) for op in rr.OP_NAMES + ('inner',)}


def test_routed_ops_and_operand_checks(fx):
    """proj / dist / logmap route to pmath; operands that require grad give results that do not; CPU and float64 tensors are refused."""
    from sttode_amd import capi, manifolds as mf, pmath
    p, y, u, w = _d(fx['op.ball.d16.c0.5.in'])
    ball = mf.PoincareBall(0.5)
    assert torch.equal(ball.proj(p * 3), pmath.project(p * 3, c=0.5)) and torch.equal(ball.dist(p, y), pmath.dist(p, y, c=0.5))
    assert torch.equal(ball.logmap(p, y), pmath.logmap(y, p, c=0.5)) and torch.equal(ball.expmap(u, p), pmath.expmap(p, u, c=0.5))
    q = _d(fx['op.obl.d16.in'])[0]
    assert torch.equal(mf.Oblique().proj(q * 3), pmath.oblique_proj(q * 3)) and mf.Oblique().dist(q, q).shape == (9, 9)
    pg = p.clone().requires_grad_()
    for out in (ball.retr(pg, u), ball.expmap(u, pg), ball.dist(pg, y), ball.proj(pg), ball.egrad2rgrad(pg, u), mf.Oblique().proj(pg)):
        assert not out.requires_grad
    for bad in (p.cpu(), p.double()):
        for call in (lambda: ball.retr(bad, bad), lambda: ball.ptransp(bad, bad, bad), lambda: mf.Oblique().proj_tan(bad, bad)):
            with pytest.raises(capi.SttodeError):
                call()


def test_a_refused_call_leaves_its_outputs_untouched(fx):
    from sttode_amd import capi
    p, y, u, w = _d(fx['op.ball.d16.c1.0.in'])
    out, out2 = torch.full_like(p, 7.0), torch.full_like(p, 7.0)
    st = capi.stream_ptr()
    for args in ((5, 2, p, u, w, out, out2, 9, 16, -1.0), (5, 2, p, u, None, out, out2, 9, 16, 1.0), (9, 2, p, u, w, out, out2, 9, 16, 1.0),
                 (5, 3, p, u, w, out, out2, 9, 16, 1.0), (5, 2, p, u, w, out, None, 9, 16, 1.0), (5, 2, p, u, w, out, out2, 0, 16, 1.0)):
        with pytest.raises(capi.SttodeError, match='sttode_manifold_rowop'):
            capi.call('sttode_manifold_rowop', *args, st)
    x, m, v = p.clone(), torch.full_like(p, 7.0), torch.full((9,), 7.0, device=p.device)
    table = torch.tensor([[x.data_ptr(), m.data_ptr(), v.data_ptr(), u.data_ptr(), 16, 9, 0, 2, 0x3FF0000000000000, 144]], dtype=torch.int64).to(p.device)
    for args in ((0, table, 1, 3, 0.1, 0.9, 0.999, 1e-8, 0.0, 0.0, 0, None), (0, table, 1, 3, float('nan'), 0.9, 0.999, 1e-8, 0.0, 0.0, 1, None),
                 (2, table, 1, 3, 0.1, 0.9, 0.999, 1e-8, 0.0, 0.0, 1, None), (0, table, 1, 3, 0.1, 1.0, 0.999, 1e-8, 0.0, 0.0, 1, None)):
        with pytest.raises(capi.SttodeError, match='sttode_riemannian_step'):
            capi.call('sttode_riemannian_step', *args, st)
    torch.cuda.synchronize()
    assert (out == 7).all() and (out2 == 7).all() and (m == 7).all() and (v == 7).all() and torch.equal(x, p)
    # ... and the same table is taken once the arguments are right (the host's step count, no device count; 9 rows of 16: 3 wave slots)
    capi.call('sttode_riemannian_step', 0, table, 1, 3, 0.1, 0.9, 0.999, 1e-8, 0.0, 0.0, 1, None, st)
    torch.cuda.synchronize()
    assert not torch.equal(x, p) and not (m == 7).any() and not (v == 7).any()


# --------------------------------------------------------------------------------------------------- 2. the optimisers against the fixture
def _params(fx, case):
    from sttode_amd import manifolds as mf
    ps = []
    for k, (mname, c, shape) in enumerate(rr.OPT_CASES[case][0]):
        p = mf.ManifoldParameter(_d(fx['opt.%s.p%d.x0' % (case, k)]), True, _man(mname, c))
        p.grad = torch.zeros_like(p)
        ps.append(p)
    return ps


def _optimizer(rule, ps, lr):
    from sttode_amd import optim
    if rule == 'adam':
        return optim.RiemannianAdam(ps, lr=lr, betas=rr.BETAS, eps=rr.ADAM_EPS, weight_decay=rr.WD)
    return optim.RiemannianSGD(ps, lr=lr, momentum=rr.RULES[rule], weight_decay=rr.WD)


STATE_KEYS = dict(adam=('exp_avg', 'exp_avg_sq'), sgdm=('momentum_buffer',), sgd0=())


def _run(fx, case, rule, worst=None):
    """The case's 8 steps; every step's parameters and state buffers against the float64 run when `worst` is a dict.  Returns the final
    tensors (parameters, then state buffers)."""
    ps = _params(fx, case)
    opt = _optimizer(rule, ps, rr.OPT_CASES[case][1])
    grads = [_d(fx['opt.%s.p%d.g' % (case, k)]) for k in range(len(ps))]
    for step in range(rr.STEPS):
        for p, g in zip(ps, grads):
            p.grad.copy_(g[step])
        opt.step()
        if worst is None:
            continue
        for k, p in enumerate(ps):
            mname = rr.OPT_CASES[case][0][k][0]
            got = [('x', p.detach())] + [(w, opt.state[p][key]) for w, key in zip(('s1', 's2'), STATE_KEYS[rule])]
            for what, t in got:
                ref = fx[rr.opt_key(case, k, rule, what, 64)][step]
                assert t.shape == ref.shape, (case, k, rule, what, t.shape, ref.shape)
                a = t.cpu().numpy()
                assert np.isfinite(a).all(), (case, k, rule, what, step)
                e = rr.err(a, ref)
                key = (rule, mname + (' (clipped)' if case == 'clip' else ''))
                worst[key] = max(worst.get(key, 0.0), e)
                assert e <= BOUND, (case, k, rule, what, 'step %d' % (step + 1), e)
    return [p.detach().clone() for p in ps] + [opt.state[p][key].clone() for p in ps for key in STATE_KEYS[rule]], opt


@pytest.mark.parametrize('rule', list(rr.RULES))
def test_optimiser_trajectories_against_the_float64_run(fx, rule):
    """Every optimiser case, 8 steps: Oblique, the ball at both c, the three-parameter table ([9,16] Oblique in wave slots 0-2, four rows a wave and the last slot with one, [2,3,65]
    ball in the next 6 wave slots, [2100,8] ball in 525 more, four rows each: the lookup at its boundaries, 134 blocks) and the clip case."""
    worst = {}
    for case in rr.OPT_CASES:
        _, opt = _run(fx, case, rule, worst)
        st = opt.state_dict()['state']
        assert len(st) == (len(rr.OPT_CASES[case][0]) if rule != 'sgd0' else 0)
        for s in st.values():
            assert set(s) == ({'step', 'exp_avg', 'exp_avg_sq'} if rule == 'adam' else {'momentum_buffer'})
            assert rule != 'adam' or float(s['step']) == rr.STEPS
    for key in sorted(worst):
        print('%-6s %-20s worst error over 8 steps %.2e' % (*key, worst[key]))
    assert {k[1] for k in worst} == {'oblique', 'poincare', 'poincare (clipped)'}


def test_step_at_the_rows_per_wave_thresholds():
    """A wave steps four rows of d <= 16, two of d <= 32, one above: d in {15, 16, 17, 31, 32, 33}, 5 rows each (so every parameter's last
    wave holds fewer rows than it could), Oblique and ball, all twelve parameters in ONE table, 3 steps of each rule against
    riemannian_ref.py in float64 on the same float32 inputs."""
    from sttode_amd import manifolds as mf
    rng = np.random.default_rng(20261206)
    specs = [(mname, c, d) for d in (15, 16, 17, 31, 32, 33) for mname, c in (('oblique', 1.0), ('poincare', 0.5))]
    x0, gs = [], []
    for mname, c, d in specs:
        v = rng.standard_normal((5, d))
        v /= np.linalg.norm(v, axis=-1, keepdims=True)
        x0.append((v if mname == 'oblique' else v * rng.uniform(0.05, 0.9, (5, 1)) / np.sqrt(c)).astype(np.float32))
        gs.append(rng.standard_normal((3, 5, d)).astype(np.float32))
    for rule in rr.RULES:
        ps = [mf.ManifoldParameter(_d(a), True, _man(mname, c)) for a, (mname, c, d) in zip(x0, specs)]
        opt = _optimizer(rule, ps, rr.LR)
        for step in range(3):
            for p, g in zip(ps, gs):
                p.grad = _d(g[step])
            opt.step()
        worst = 0.0
        for p, a, g, (mname, c, d) in zip(ps, x0, gs, specs):
            ref = rr.run_rule(rule, rr.make_manifold(mname, c), torch.from_numpy(a).double(), list(torch.from_numpy(g).double()), rr.LR)[-1]
            got = [p.detach()] + [opt.state[p][key] for key in STATE_KEYS[rule]]
            for t, r in zip(got, [r for r in ref if r is not None]):
                e = rr.err(t.cpu().numpy(), r.numpy())
                worst = max(worst, e)
                assert e <= BOUND, (rule, mname, d, e)
        print('%-5s d in {15..33}, twelve parameters in one table, 3 steps: worst error %.2e' % (rule, worst))


def test_three_parameter_case_is_bitwise_repeatable(fx):
    a, _ = _run(fx, 'three', 'adam')
    b, _ = _run(fx, 'three', 'adam')
    assert len(a) == 9 and all(torch.equal(s, t) for s, t in zip(a, b))
    a, _ = _run(fx, 'three', 'sgdm')
    b, _ = _run(fx, 'three', 'sgdm')
    assert len(a) == 6 and all(torch.equal(s, t) for s, t in zip(a, b))


def test_state_dict_round_trip_and_add_param_group(fx):
    """4 steps, state_dict into a fresh optimiser over fresh parameters, 4 more: bitwise the uninterrupted 8.  add_param_group after the
    first step rebuilds the table: the new group's parameter moves, the old ones go on as before."""
    from sttode_amd import manifolds as mf
    for rule in ('adam', 'sgdm'):
        whole, _ = _run(fx, 'three', rule)
        ps = _params(fx, 'three')
        opt = _optimizer(rule, ps, rr.LR)
        grads = [_d(fx['opt.three.p%d.g' % k]) for k in range(3)]
        for step in range(rr.STEPS):
            if step == 4:
                sd = opt.state_dict()
                assert rule != 'adam' or all(float(s['step']) == 4 for s in sd['state'].values())
                qs = [mf.ManifoldParameter(p.detach().clone(), True, p.manifold) for p in ps]
                for q in qs:
                    q.grad = torch.zeros_like(q)
                ps, opt = qs, _optimizer(rule, qs, rr.LR)
                opt.load_state_dict(sd)
            for p, g in zip(ps, grads):
                p.grad.copy_(g[step])
            opt.step()
        got = [p.detach() for p in ps] + [opt.state[p][key] for p in ps for key in STATE_KEYS[rule]]
        assert all(torch.equal(s, t) for s, t in zip(whole, got)), rule
    ps = _params(fx, 'obl')
    opt = _optimizer('adam', ps, rr.LR)
    g = _d(fx['opt.obl.p0.g'])
    ps[0].grad.copy_(g[0])
    opt.step()
    extra = _params(fx, 'ball.c0.5')[0]
    opt.add_param_group(dict(params=[extra], lr=0.01))
    before = extra.detach().clone()
    ps[0].grad.copy_(g[1])
    extra.grad.copy_(_d(fx['opt.ball.c0.5.p0.g'])[0])
    opt.step()
    assert not torch.equal(extra.detach(), before)
    assert rr.err(ps[0].detach().cpu().numpy(), fx[rr.opt_key('obl', 0, 'adam', 'x', 64)][1]) <= BOUND
    sd = opt.state_dict()
    assert [float(s['step']) for s in sd['state'].values()] == [2.0, 1.0] and sd['param_groups'][1]['lr'] == 0.01


# --------------------------------------------------------------------------------------------------- 3. plain parameters
def test_plain_parameters_follow_adam_bitwise_and_sgd_within_the_bound(fx):
    from sttode_amd import optim
    dev, rng = _dev(), np.random.default_rng(20261202)
    shapes = ((7,), (33, 5), (1,), (300, 9), (1025,))
    x0 = [rng.standard_normal(s).astype(np.float32) for s in shapes]
    gs = [[rng.standard_normal(s).astype(np.float32) for s in shapes] for _ in range(5)]

    def run(make, manifold_too):
        ps = [torch.nn.Parameter(_d(a)) for a in x0]
        extra = _params(fx, 'obl') if manifold_too else []
        opt = make(ps + extra)
        for step in range(5):
            for p, g in zip(ps, gs[step]):
                p.grad = _d(g)
            for q in extra:
                q.grad = _d(fx['opt.obl.p0.g'][step])
            opt.step()
        return [p.detach() for p in ps], opt, extra
    kw = dict(lr=0.01, betas=(0.9, 0.99), eps=1e-8, weight_decay=0.01)
    want, ref_opt, _ = run(lambda ps: optim.Adam(ps, **kw), False)
    got, opt, extra = run(lambda ps: optim.RiemannianAdam(ps, **kw), True)
    assert all(torch.equal(a, b) for a, b in zip(want, got)), 'plain parameters under RiemannianAdam differ from optim.Adam'
    sd, rsd = opt.state_dict()['state'], ref_opt.state_dict()['state']
    assert all(float(sd[i]['step']) == 5 and torch.equal(sd[i]['exp_avg_sq'], rsd[i]['exp_avg_sq']) for i in range(len(shapes)))
    assert float(sd[len(shapes)]['step']) == 5 and not torch.equal(extra[0].detach(), _d(fx['opt.obl.p0.x0']))
    for mom in (0.9, 0.0):
        want, _, _ = run(lambda ps: torch.optim.SGD(ps, lr=0.05, momentum=mom, weight_decay=0.01), False)
        got, opt, _ = run(lambda ps: optim.RiemannianSGD(ps, lr=0.05, momentum=mom, weight_decay=0.01), True)
        e = max(rr.err(a.cpu().numpy(), b.cpu().numpy()) for a, b in zip(got, want))
        print('RiemannianSGD momentum %s, plain parameters vs torch.optim.SGD over 5 steps: %.2e' % (mom, e))
        assert e <= BOUND


def test_unsupported_tensors_raise_at_the_first_step(fx):
    from sttode_amd import manifolds as mf, optim
    dev = _dev()
    for make in (lambda ps: optim.RiemannianAdam(ps), lambda ps: optim.RiemannianSGD(ps, lr=0.1)):
        for dtype, grad_of in ((torch.float64, torch.ones_like), (torch.float32, lambda p: torch.ones(16, 9, device=dev).t())):
            for cls in (lambda t: mf.ManifoldParameter(t, True, mf.Oblique()), torch.nn.Parameter):
                p = cls(torch.ones(9, 16, dtype=dtype, device=dev))
                p.grad = grad_of(p)
                with pytest.raises(ValueError, match='float64|contiguous'):
                    make([p]).step()
                assert (p == 1).all()


# --------------------------------------------------------------------------------------------------- 4. invariants and end-to-end uses
def test_parameters_stay_on_their_manifolds_over_200_steps():
    from sttode_amd import manifolds as mf, optim
    dev = _dev()
    gen = torch.Generator(device='cpu').manual_seed(20261203)
    c = 0.5
    xo = torch.randn(33, 16, generator=gen)
    xo = mf.ManifoldParameter((xo / xo.norm(dim=-1, keepdim=True)).to(dev), True, mf.Oblique())
    dirs = torch.randn(17, 8, generator=gen)
    dirs = (dirs / dirs.norm(dim=-1, keepdim=True)).to(dev)
    xb = mf.ManifoldParameter(dirs * (0.98 / c ** 0.5), True, mf.PoincareBall(c))             # sqrt(c) |x| = 0.98 ...
    Wo = torch.randn(16, 6, generator=gen).to(dev)
    To, Tb = torch.randn(33, 6, generator=gen).to(dev), dirs * (3.0 / c ** 0.5)               # ... and targets outside the ball, straight ahead
    opt = optim.RiemannianAdam([dict(params=[xo]), dict(params=[xb], lr=0.1)], lr=0.05)

    def closure():
        opt.zero_grad(set_to_none=False)
        loss = ((xo @ Wo - To) ** 2).mean() + ((xb - Tb) ** 2).mean()
        loss.backward()
        return loss.detach()
    first = float(closure())
    worst_o = torch.zeros((), dtype=torch.float64, device=dev)     # over ALL 200 steps, kept on the device: no round trip inside the loop
    worst_b = torch.zeros((), dtype=torch.float64, device=dev)
    for _ in range(200):
        last = opt.step(closure)
        worst_o = torch.maximum(worst_o, (xo.detach().double().norm(dim=-1) - 1).abs().max())
        worst_b = torch.maximum(worst_b, (c ** 0.5) * xb.detach().double().norm(dim=-1).max())
    print('200 steps: loss %.4f -> %.4f, max | |x| - 1 | %.2e, max sqrt(c) |x| %.7f (after the last step %.6f)'
          % (first, float(last), float(worst_o), float(worst_b), float((c ** 0.5) * xb.detach().double().norm(dim=-1).max())))
    assert float(worst_o) <= 1e-6
    assert float(worst_b) <= 1 - 1e-3 + 1e-6
    assert float(worst_b) >= 1 - 1e-3 - 1e-6, 'no row ever ended a step on the sphere project clips to: the clipped branch was not exercised'
    assert float(last) < first and float(closure()) < first


def test_frechet_mean_on_the_ball_through_pmath_dist():
    from sttode_amd import manifolds as mf, optim, pmath
    dev, c = _dev(), 0.5
    gen = torch.Generator(device='cpu').manual_seed(20261204)
    pts = pmath.expmap0((0.4 * torch.randn(20, 5, generator=gen) + 0.3).to(dev), c=c)
    mu = mf.ManifoldParameter(torch.zeros(1, 5, device=dev), True, mf.PoincareBall(c))
    opt = optim.RiemannianAdam([mu], lr=0.05)
    losses = []
    for _ in range(60):
        opt.zero_grad()
        loss = pmath.dist(mu.expand(20, 5), pts, c=c).pow(2).sum()
        loss.backward()
        assert mu.grad is not None and mu.grad.shape == (1, 5) and bool(mu.grad.abs().sum() > 0)
        opt.step()
        losses.append(float(loss.detach()))
    print('Frechet mean: sum of squared distances %.4f -> %.4f' % (losses[0], losses[-1]))
    assert losses[-1] < losses[0] and min(losses) < 0.9 * losses[0]
    assert float((c ** 0.5) * mu.detach().norm()) < 1 - 1e-3


def test_leading_eigenvector_on_oblique_rows():
    from sttode_amd import manifolds as mf, optim
    dev = _dev()
    gen = torch.Generator(device='cpu').manual_seed(20261205)
    Q, _ = torch.linalg.qr(torch.randn(8, 8, generator=gen, dtype=torch.float64))
    A = (Q * torch.tensor([3.0, 1.5, 1.2, 1.0, 0.8, 0.5, 0.3, 0.1], dtype=torch.float64)) @ Q.T
    v1 = torch.linalg.eigh(A)[1][:, -1]
    x = torch.randn(4, 8, generator=gen)
    x = mf.ManifoldParameter((x / x.norm(dim=-1, keepdim=True)).to(dev), True, mf.Oblique())
    Ad = A.float().to(dev)
    opt = optim.RiemannianSGD([x], lr=0.1, momentum=0.5)
    for _ in range(150):
        opt.zero_grad()
        (-((x @ Ad) * x).sum()).backward()
        opt.step()
    cos = (x.detach().double().cpu() @ v1).abs()
    print('leading eigenvector: 1 - |cos| per row', (1 - cos).tolist())
    assert bool((1 - cos <= 1e-3).all())
    assert float((x.detach().double().norm(dim=-1) - 1).abs().max()) <= 1e-6


# --------------------------------------------------------------------------------------------------- 5. graph capture
def test_captured_step_replays_as_eager_steps(fx):
    """One eager step, then a step captured with torch.cuda.graph and replayed 3 times, against 4 eager steps with the same (static)
    gradients: the same bits.  The captured Adam step reads its count from the device, so each replay advances the bias corrections."""
    for rule in ('adam', 'sgdm'):
        runs = []
        for captured in (False, True):
            ps = _params(fx, 'three')
            opt = _optimizer(rule, ps, rr.LR)
            for k, p in enumerate(ps):
                p.grad.copy_(_d(fx['opt.three.p%d.g' % k])[0])
            opt.step()
            if captured:
                torch.cuda.synchronize()
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    opt.step()
                for _ in range(3):
                    graph.replay()
            else:
                for _ in range(3):
                    opt.step()
            torch.cuda.synchronize()
            runs.append([p.detach().clone() for p in ps] + [opt.state[p][key].clone() for p in ps for key in STATE_KEYS[rule]])
            if rule == 'adam':
                assert all(float(s['step']) == 4 for s in opt.state_dict()['state'].values()), captured
        assert all(torch.equal(a, b) for a, b in zip(*runs)), rule
        assert not torch.equal(runs[0][0], _d(fx['opt.three.p0.x0']))
