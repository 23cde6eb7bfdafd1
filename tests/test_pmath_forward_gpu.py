"""GPU tests of the FORWARD VALUES of the Poincare-ball op library (csrc/pmath.hip through sttode_amd/pmath.py) at the shapes where such
kernels go wrong: one and two trips of the 64-lane loop +-1, every remainder of the four-rows-per-block grid, rows longer than a block,
grids with a tail, non-square pair shapes.

Yardstick: the same operation in float64 on the very float32 inputs the kernel received -- oracle/pmath_ref.py (dtype-generic, pinned to the
reference on the CPU by test_oracle_golden.py) and oracle.sttode_ref.oblique_proj / oblique_dist.  Metric: max |got - ref| / (1 + |ref|)
(pmath_vjp_cases.err).  Two bounds per op, over the op's cases in a test:
  hard   e_hip <= 1e-4 (pmath_vjp_cases.BOUND);
  tight  e_hip <= max(8 x e_oracle_fp32, 1e-6): e_oracle_fp32 is the oracle's own float32 run of the same cases, computed here on the CPU.
         The factor 8 is room for the kernel's per-lane partial sums and 6-step butterfly rounding differently from torch's reduction order
         and for device logf / tanhf / sqrtf being a few ulp where glibc's are within 1; 1e-6 is the project's floor for "one rounding to
         float32".  A dropped tail element or a swapped index passes neither.
NaN positions must be the yardstick's exactly, and the result is finite wherever the yardstick is (the functions allocate their own
outputs, so an unwritten tail shows as whatever the allocator left: it is never mistaken for a value because it must match to 1e-6).
Inputs are interior points, sqrt(c) |x| in [0.05, 0.9]; the clipped ball boundary is test_gpu_parity's golden test.

Measured on the MI355X (per op, the oracle's fp32 figure beside it): DESIGN.md 4q and 4r, profiles/pmath_grad/gputests.txt.
"""
import numpy as np
import pytest
import torch

import oracle.pmath_ref as ref
from helpers import yardstick_close
from hypnn_cases import SHAPES, case_arrays, function_cases
from oracle.sttode_ref import oblique_dist as ref_oblique_dist
from oracle.sttode_ref import oblique_proj as ref_oblique_proj
from pmath_vjp_cases import BOUND, CS, DIST_MATRIX, MATVEC, ROW_OPS, SCALAR_OPS, TWO_OPS, cases, err

pytestmark = pytest.mark.gpu

FACTOR, FLOOR = 8.0, 1e-6
ALL_ROW_OPS = ROW_OPS + ('oblique_proj',)
EDGE_D, EDGE_ROWS = (63, 64, 65, 127, 128, 129, 300), (3, 4, 5, 7)
OBL_EDGE = 1 - 1e-4      # core/manifolds/oblique.py:7, the clamp of the dot product


def _dev():
    assert torch.cuda.is_available(), 'these tests need the GPU'
    return torch.device('cuda:0')


def _ball(rng, shape, c, lo=0.05, hi=0.9):
    """Random directions with sqrt(c) |.| uniform in [lo, hi], float32."""
    v = rng.standard_normal(shape)
    return (v / np.linalg.norm(v, axis=-1, keepdims=True) * rng.uniform(lo, hi, shape[:-1] + (1,)) / np.sqrt(c)).astype(np.float32)


def _t(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype)


class Tally:
    """Worst error per op of the kernel and of the oracle's fp32 run, both against the float64 yardstick."""

    def __init__(self):
        self.hip, self.ora, self.bad = {}, {}, []

    def add(self, op, got, r64, r32, what, exact_zeros=False):
        got, r64, r32 = np.asarray(got), np.asarray(r64, np.float64), np.asarray(r32, np.float64)
        assert got.dtype == np.float32 and got.shape == r64.shape == r32.shape, (what, got.dtype, got.shape, r64.shape, r32.shape)
        nan, fin = np.isnan(r64), np.isfinite(r64)
        assert (nan | fin).all(), what + ': the yardstick has an infinity (not an interior case)'
        assert np.array_equal(np.isnan(got), nan), what + ': NaN positions differ from the yardstick'
        assert np.isfinite(got[fin]).all(), what + ': not finite where the yardstick is'
        if exact_zeros:
            assert not got[r64 == 0].any(), what + ': not exactly zero where the yardstick is'
        e = err(got[fin], r64[fin]) if fin.any() else 0.0
        both = fin & np.isfinite(r32)
        self.hip[op] = max(self.hip.get(op, 0.0), e)
        self.ora[op] = max(self.ora.get(op, 0.0), err(r32[both], r64[both]) if both.any() else 0.0)
        if not e <= BOUND:
            self.bad.append((what, e))

    def check(self, expect):
        for op in sorted(self.hip):
            print('%-24s worst error %.2e   (oracle fp32: %.2e)' % (op, self.hip[op], self.ora[op]))
        assert set(expect) == set(self.hip), set(expect) ^ set(self.hip)
        assert not self.bad, ('outside the hard bound', self.bad)
        loose = [(op, self.hip[op], self.ora[op]) for op in sorted(self.hip) if not self.hip[op] <= max(FACTOR * self.ora[op], FLOOR)]
        assert not loose, ('outside the tight bound max(8 x oracle fp32, 1e-6): (op, kernel, oracle fp32)', loose)


def _hip_row(pm, op, c, ts, keepdim=False):
    if op in ('p2k', 'k2p'):
        return getattr(pm, op)(*ts, c)
    if op == 'oblique_proj':
        return pm.oblique_proj(*ts)
    fn = getattr(pm, 'lorenz_factor' if op == 'lorenz' else op)
    return fn(*ts, c=c, keepdim=keepdim) if op in SCALAR_OPS else fn(*ts, c=c)


def _ora_row(op, c, arrays, dtype, keepdim=False):
    ts = [_t(a, dtype) for a in arrays]
    if op == 'oblique_proj':
        return ref_oblique_proj(*ts).numpy()
    fn = getattr(ref, 'lorenz_factor' if op == 'lorenz' else op)
    return (fn(*ts, c, keepdim=keepdim) if op in SCALAR_OPS else fn(*ts, c)).numpy()


def _row(tally, pm, op, c, arrays, what, dev_inputs=None, keepdim=False, exact_zeros=False):
    """One row op on the device against the oracle in float64 and float32; ``dev_inputs``: device tensors holding ``arrays``'s values."""
    ts = dev_inputs if dev_inputs is not None else [_t(a).to(_dev()) for a in arrays]
    got = _hip_row(pm, op, c, ts, keepdim).cpu().numpy()
    tally.add(op, got, _ora_row(op, c, arrays, torch.float64, keepdim), _ora_row(op, c, arrays, torch.float32, keepdim), what,
              exact_zeros=exact_zeros)
    return got


def _operands(op, x, y, u):
    ins = [x * np.float32(0.5)] if op == 'k2p' else [x]         # Klein coordinates: half the radius, as the fixture does
    if op in TWO_OPS:
        ins.append(u if op == 'expmap' else y)
    return ins


# --------------------------------------------------------------------------------------------------- 1. row ops
def test_row_ops_at_every_fixture_case(golden):
    """Every row-op case of pmath_vjp.npz / pmath_vjp_rows.npz: d in {1, 2, 16, 65, 130} x rows in {1, 9} x c in {1, 0.5} for the 12 ops, the
    clipped project rows, the zero rows (exactly the oracle's zeros) and the broadcast operands (the oracle's shape pins _row_fwd's
    broadcasting).  oblique_proj, which has no gradient case, runs on the x of every project case."""
    import sttode_amd.pmath as pm
    tally, n = Tally(), 0
    for case in cases(golden('pmath_vjp'), golden('pmath_vjp_rows')):
        if case['op'] not in ROW_OPS:
            continue
        n += 1
        zero = case['name'].startswith('zero.')
        got = _row(tally, pm, case['op'], case['c'], case['inputs'], case['name'], exact_zeros=zero)
        if case['name'] in ('zero.expmap0', 'zero.logmap0'):
            assert not case['inputs'][0][4].any() and not got[4].any(), case['name'] + ': the zero row must give exactly zero'
        if case['op'] == 'project':
            _row(tally, pm, 'oblique_proj', None, case['inputs'], case['name'] + ' (oblique_proj)')
    assert n == 12 * 20 + 2 + 3 + 2
    tally.check(ALL_ROW_OPS)


def test_row_ops_at_the_lane_loop_and_block_edges():
    """d at one and two trips of the 64-lane loop +-1 and at 300; rows over every remainder of the four-rows-per-block grid; all 13 ops."""
    import sttode_amd.pmath as pm
    dev, rng, tally = _dev(), np.random.default_rng(20261101), Tally()
    for d in EDGE_D:
        for rows in EDGE_ROWS:
            for c in CS:
                xyu = _ball(rng, (3, rows, d), c)
                half = xyu[0] * np.float32(0.5)
                dx, dy, du, dh = torch.from_numpy(np.concatenate([xyu, half[None]])).to(dev)       # one transfer per shape
                for op in ALL_ROW_OPS:
                    ins = _operands(op, *xyu)
                    dins = [dh if op == 'k2p' else dx] + ([du if op == 'expmap' else dy] if op in TWO_OPS else [])
                    _row(tally, pm, op, c, ins, '%s d%d rows%d c%s' % (op, d, rows, c), dev_inputs=dins)
    tally.check(ALL_ROW_OPS)


def test_row_ops_leading_dims_keepdim_and_strided_inputs():
    """A 3-D input [2, 3, d], keepdim=True of the four scalar ops (the oracle's shape), and a transposed view as input."""
    import sttode_amd.pmath as pm
    dev, rng, tally = _dev(), np.random.default_rng(20261102), Tally()
    c, d = 0.5, 65
    xyu = _ball(rng, (3, 2, 3, d), c)
    for op in ALL_ROW_OPS:
        got = _row(tally, pm, op, c, _operands(op, *xyu), op + ' [2,3,65]')
        assert got.shape == ((2, 3) if op in SCALAR_OPS else (2, 3, d)), op
        if op in SCALAR_OPS:
            assert _row(tally, pm, op, c, _operands(op, *xyu), op + ' [2,3,65] keepdim', keepdim=True).shape == (2, 3, 1), op
    xyu = _ball(rng, (3, 5, d), c)
    for op in ALL_ROW_OPS:
        ins = _operands(op, *xyu)
        views = [torch.from_numpy(np.ascontiguousarray(a.T)).to(dev).t() for a in ins]           # [d, 5] in memory, seen as [5, d]
        assert not any(v.is_contiguous() for v in views)
        _row(tally, pm, op, c, ins, op + ' transposed view', dev_inputs=views)
    tally.check(ALL_ROW_OPS)


def test_row_ops_give_nan_exactly_where_the_reference_does():
    """logmap(x, x) is 0/0 in the reference; on rows of dyadic coordinates every product is exact in float32, float64 and under fma
    contraction, so the whole result is NaN in the oracle and must be in the kernel.  A zero row of oblique_proj is NaN, the others not."""
    import sttode_amd.pmath as pm
    x = np.zeros((5, 65), np.float32)
    x[0, 0], x[1, 64], x[2, :2], x[3, 63:], x[4, 7] = 0.5, 0.5, 0.25, 0.25, -0.5
    tally = Tally()
    got = _row(tally, pm, 'logmap', 1.0, [x, x], 'logmap(x, x)')
    assert np.isnan(got).all()
    p = _ball(np.random.default_rng(20261103), (6, 65), 1.0)
    p[4] = 0
    got = _row(tally, pm, 'oblique_proj', None, [p], 'oblique_proj with a zero row')
    assert np.isnan(got[4]).all() and np.isfinite(np.delete(got, 4, 0)).all()
    tally.check(('logmap', 'oblique_proj'))


# --------------------------------------------------------------------------------------------------- 2. mobius_matvec
def test_mobius_matvec_forward(golden):
    """rowdot_kernel with O != d and the finishing row kernel over O: the five fixture cases (the zero row of mv.zero exactly zero) and
    one drawn here with O = 130 > 64, d = 65, 5 rows (rows % 4 != 0)."""
    import sttode_amd.pmath as pm
    dev, tally = _dev(), Tally()
    todo = [(c['name'], c['c'], c['inputs'], c['zero_row']) for c in cases(golden('pmath_vjp'), golden('pmath_vjp_rows'))
            if c['op'] == 'mobius_matvec']
    assert [t[0] for t in todo] == ['mv.' + tag for tag in MATVEC]
    rng = np.random.default_rng(20261104)
    for c in CS:      # m ~ 0.1 N(0,1): |mx| / |x| is about 1.1 at O = 130, so the result stays inside the ball
        todo.append(('mv.drawn.d65O130.c%s' % c, c, [(0.1 * rng.standard_normal((130, 65))).astype(np.float32), _ball(rng, (5, 65), c)], None))
    for name, c, (m, x), zero_row in todo:
        got = pm.mobius_matvec(_t(m).to(dev), _t(x).to(dev), c=c).cpu().numpy()
        r64, r32 = (ref.mobius_matvec(_t(m, dt), _t(x, dt), c).numpy() for dt in (torch.float64, torch.float32))
        tally.add('mobius_matvec', got, r64, r32, name, exact_zeros=zero_row is not None)
        if zero_row is not None:
            assert not x[zero_row].any() and not got[zero_row].any(), 'the zero row of x must give an exactly zero row'
    tally.check(('mobius_matvec',))


# --------------------------------------------------------------------------------------------------- 3. pair kernel
def test_dist_matrix_forward(golden):
    import sttode_amd.pmath as pm
    dev, tally, z = _dev(), Tally(), golden('pmath_vjp')
    for P, R, d in DIST_MATRIX:
        name = 'dm.P%dR%dd%d' % (P, R, d)
        x, y = z[name + '.x'], z[name + '.y']
        got = pm.dist_matrix(_t(x).to(dev), _t(y).to(dev), c=1.0).cpu().numpy()
        assert got.shape == (P, R)
        tally.add('dist_matrix', got, *(ref.dist_matrix(_t(x, dt), _t(y, dt), 1.0).numpy() for dt in (torch.float64, torch.float32)), name)
    tally.check(('dist_matrix',))


def test_mobius_addition_batch_and_hyperbolic_softmax_forward(golden):
    """Every hs.* and mab.* case of hypnn.npz, up to C = 67, B = 70, d = 300.  _hyperbolic_softmax's result is [B, C]: at the shapes with
    C != B single logits are also held to the oracle on that one (row of X, class) pair, so a transposed write cannot hide in a reshape."""
    import sttode_amd.pmath as pm
    dev, tally, z = _dev(), Tally(), golden('hypnn')
    todo = [(name, op, c) for name, op, c in function_cases() if op != 'clip']
    assert len(todo) == 2 * len(SHAPES)
    for (name, op, c), (B, C, d, _) in zip(todo, [s for s in SHAPES for _ in range(2)]):
        ins = case_arrays(z, name)[0]
        dins = [_t(a).to(dev) for a in ins]
        if op == 'hsoftmax':
            got = pm._hyperbolic_softmax(*dins, c).cpu().numpy()
            r64, r32 = (ref.hyperbolic_softmax(*[_t(a, dt) for a in ins], c).numpy() for dt in (torch.float64, torch.float32))
            assert got.shape == (B, C) == r64.shape, name
            if B != C:
                X, A, P = (_t(a, torch.float64) for a in ins)
                for b, k in ((0, C - 1), (B - 1, 0), (B // 2, C // 2)):
                    one = float(ref.hyperbolic_softmax(X[b:b + 1], A[k:k + 1], P[k:k + 1], c))
                    assert abs(got[b, k] - one) <= FLOOR * (1 + abs(one)), (name, 'logit of row %d, class %d' % (b, k), got[b, k], one)
            tally.add('_hyperbolic_softmax', got, r64, r32, name)
        else:
            got = pm._mobius_addition_batch(*dins, c).cpu().numpy()
            r64, r32 = (ref.mobius_addition_batch(*[_t(a, dt) for a in ins], c).numpy() for dt in (torch.float64, torch.float32))
            assert got.shape == (B, C, d), name
            tally.add('_mobius_addition_batch', got, r64, r32, name)
    tally.check(('_hyperbolic_softmax', '_mobius_addition_batch'))


# --------------------------------------------------------------------------------------------------- 4. poincare_mean
def test_poincare_mean_forward():
    """d = 1025 and 2050 enter the finishing kernel's blockDim-stride loop a second and a third time; 130 rows is its serial row loop."""
    import sttode_amd.pmath as pm
    dev, rng, tally = _dev(), np.random.default_rng(20261105), Tally()
    for rows, d in ((1, 1), (4, 16), (5, 65), (33, 130), (130, 1025), (3, 2050)):
        for c in CS:
            x = _ball(rng, (rows, d), c)
            got = pm.poincare_mean(_t(x).to(dev), dim=0, c=c).cpu().numpy()
            assert got.shape == (d,)
            tally.add('poincare_mean', got, *(ref.poincare_mean(_t(x, dt), c).numpy() for dt in (torch.float64, torch.float32)),
                      'poincare_mean rows%d d%d c%s' % (rows, d, c))
    tally.check(('poincare_mean',))


# --------------------------------------------------------------------------------------------------- 5. Oblique ops
def _oblique(tally, pm, a, b, what):
    """oblique_dist(oblique_proj(a), oblique_proj(b)): the projections against the oracle, the distance against the oracle ON THE
    PROJECTIONS THE KERNEL MADE.  Returns the mask of the entries at the clamp.  Those -- clamped dot product within 1e-6 of
    +-(1 - 1e-4) -- are held to the oracle's float32 run instead: the clamp constant itself differs between fp32 and float64, and acos has
    slope 70 there."""
    dev = _dev()
    pa, pb = pm.oblique_proj(_t(a).to(dev)), pm.oblique_proj(_t(b).to(dev))
    for p, src in ((pa, a), (pb, b)):
        tally.add('oblique_proj', p.cpu().numpy(), _ora_row('oblique_proj', None, [src], torch.float64),
                  _ora_row('oblique_proj', None, [src], torch.float32), what + ' (projection)')
    got = pm.oblique_dist(pa, pb).cpu().numpy()
    ha, hb = pa.cpu(), pb.cpu()
    r64, r32 = ref_oblique_dist(ha.double(), hb.double()).numpy(), ref_oblique_dist(ha, hb).numpy()
    assert got.shape == r64.shape == a.shape[:-2] + (b.shape[-2], a.shape[-2]), what
    inner = np.clip((hb.double() @ ha.double().transpose(-2, -1)).numpy(), -OBL_EDGE, OBL_EDGE)
    near = np.abs(np.abs(inner) - OBL_EDGE) <= 1e-6
    assert np.isfinite(got).all(), what
    np.testing.assert_allclose(got[near], r32[near], rtol=1e-4, atol=1e-5, err_msg=what + ' (entries at the clamp)')
    tally.add('oblique_dist', got[~near], r64[~near], r32[~near], what)
    return near


def test_oblique_dist_of_projected_rows():
    """n1 != n2 everywhere, so a transposed [.., n1, n2] result has the wrong shape and the wrong values; (1, 300, 2, 8) has more than one
    block of entries per batch.  Entries at the clamp may be at most 1 % of a case.  With independent a and b there are none -- except at
    d = 1, where a projected row is +-1, every dot product is +-1 and the single entry of the (1, 1, 1, 1) case is at the clamp by
    construction: that case is exempt from the cap and held, as such entries are, to the oracle's fp32 run."""
    import sttode_amd.pmath as pm
    rng, tally = np.random.default_rng(20261106), Tally()
    for nb, n1, n2, d in ((1, 1, 1, 1), (3, 5, 7, 65), (2, 67, 3, 130), (1, 300, 2, 8)):
        a, b = (rng.standard_normal((nb, n, d)).astype(np.float32) for n in (n1, n2))
        near = _oblique(tally, pm, a, b, 'oblique nb%d n1%d n2%d d%d' % (nb, n1, n2, d))
        assert near.all() if d == 1 else not near.any(), (d, int(near.sum()))
        assert d == 1 or near.mean() <= 0.01
    a, b = (rng.standard_normal((2, 2, n, 16)).astype(np.float32) for n in (5, 3))       # leading dims [2, 2]
    near = _oblique(tally, pm, a, b, 'oblique [2,2,n,16]')
    assert near.mean() <= 0.01
    a = rng.standard_normal((1, 5, 16)).astype(np.float32)                             # dist(a, a): the diagonal is at the clamp
    near = _oblique(tally, pm, a, a, 'oblique dist(a, a)')
    assert np.array_equal(near[0], np.eye(5, dtype=bool))
    tally.check(('oblique_proj', 'oblique_dist'))


# --------------------------------------------------------------------------------------------------- 6. scalar kernels, RiemannianGradient
def test_scalar_functions_and_their_backward_rules():
    """tanh, artanh, arsinh (which 0..2) and Artanh / Arsinh backward (which 3, 4, through .backward) at n around one 256-thread block and
    at 1000.  arsinh(x) = log(x + sqrt(1 + x^2)) cancels for x << 0 (test_oracle_golden.py, test_pmath_ops): it is ALSO held to the band of
    helpers.yardstick_close around the oracle's fp32 run, at the rtol / atol the golden test gives this kernel."""
    import sttode_amd.pmath as pm
    dev, rng, tally = _dev(), np.random.default_rng(20261107), Tally()
    for n in (1, 255, 256, 257, 1000):
        x = rng.uniform(-20, 20, n).astype(np.float32)
        if n > 1:
            x[:2] = 19.5, -19.5                                # beyond the +-15 clamp whatever the draw
        got = pm.tanh(_t(x).to(dev)).cpu().numpy()
        tally.add('tanh', got, *(ref.tanh_clamped(_t(x, dt)).numpy() for dt in (torch.float64, torch.float32)), 'tanh n%d' % n)
        for name, span, fwd, bwd in (('artanh', 0.999, ref.artanh, ref.artanh_backward), ('arsinh', 45.0, ref.arsinh, ref.arsinh_backward)):
            x, g = rng.uniform(-span, span, n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
            xt = _t(x).to(dev).requires_grad_()
            out = getattr(pm, name)(xt)
            out.backward(_t(g).to(dev))
            got, ggot = out.detach().cpu().numpy(), xt.grad.cpu().numpy()
            f64, f32 = (fwd(_t(x, dt)).numpy() for dt in (torch.float64, torch.float32))
            tally.add(name, got, f64, f32, '%s n%d' % (name, n))
            if name == 'arsinh':
                yardstick_close(got, f32, f64, rtol=1e-5, atol=1e-6, what='arsinh n%d' % n)
            tally.add(name + ' backward', ggot, *(bwd(_t(x, dt), _t(g, dt)).numpy() for dt in (torch.float64, torch.float32)),
                      '%s backward n%d' % (name, n))
    tally.check(('tanh', 'artanh', 'arsinh', 'artanh backward', 'arsinh backward'))


def test_artanh_at_its_clamp_follows_the_fp32_reference():
    """|x| >= 1 - 1e-5: the result is artanh of the fp32 clamp constant, which is 0.6 % off in 1 - x (fp32 6.102355, float64 6.103034), so
    value and derivative are held to the oracle's float32 run at the golden test's rtol 1e-4, atol 1e-6."""
    import sttode_amd.pmath as pm
    x = np.array([0.99999, 1.0, 1.5, -2.0, -1.0, -0.99999, 0.999995, 0.5], np.float32)
    g = np.array([1.0, -2.0, 0.5, 1.0, 3.0, -1.0, 1.0, 1.0], np.float32)
    xt = _t(x).to(_dev()).requires_grad_()
    out = pm.artanh(xt)
    out.backward(_t(g).to(_dev()))
    np.testing.assert_allclose(out.detach().cpu().numpy(), ref.artanh(_t(x)).numpy(), rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(xt.grad.cpu().numpy(), ref.artanh_backward(_t(x), _t(g)).numpy(), rtol=1e-4, atol=1e-6)
    assert abs(out[1].item() - 6.102355) < 1e-3 and abs(out[3].item() + 6.102355) < 1e-3


def test_riemannian_gradient_backward():
    """rows > 256 (a second block, with a tail) and d = 65; the forward is the identity."""
    import sttode_amd.pmath as pm
    dev, rng, tally = _dev(), np.random.default_rng(20261108), Tally()
    try:
        for rows, d in ((1, 1), (257, 65), (300, 16)):
            for c in CS:
                x, g = _ball(rng, (rows, d), c), rng.standard_normal((rows, d)).astype(np.float32)
                pm.RiemannianGradient.c = c
                xt = _t(x).to(dev).requires_grad_()
                y = pm.RiemannianGradient.apply(xt)
                assert torch.equal(y.detach(), xt.detach())
                y.backward(_t(g).to(dev))
                tally.add('RiemannianGradient', xt.grad.cpu().numpy(),
                          *(ref.riemannian_gradient_backward(_t(x, dt), _t(g, dt), c).numpy() for dt in (torch.float64, torch.float32)),
                          'riemannian rows%d d%d c%s' % (rows, d, c))
    finally:
        pm.RiemannianGradient.c = 1
    tally.check(('RiemannianGradient',))
