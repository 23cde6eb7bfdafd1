"""Poincare-ball math on HIP: same function names / argument meaning as hyptorch/pmath.py, forward values and gradients.

Every function takes CUDA(HIP) fp32 tensors and raises on CPU tensors (no fallback).  Leading dims are flattened to
rows; the last dim is the feature dim.  ``auto_select_c`` is host arithmetic (scipy gamma, pmath.py:496-505).

Gradients: ``project, lambda_x, mobius_add, dist, dist0, expmap, expmap0, logmap, logmap0, p2k, k2p, lorenz_factor``,
``mobius_matvec``, ``dist_matrix``, ``_mobius_addition_batch``, ``_hyperbolic_softmax`` and ``feature_clip`` are differentiable with respect
to their tensor arguments (``artanh``, ``arsinh`` and ``RiemannianGradient`` always were): fused backward kernels (csrc/pmath_grad.hip,
DESIGN.md 4q and 4r), first order only (``once_differentiable``).  A function takes that path only when grad mode is on and an input requires
grad; otherwise it makes exactly the calls of the forward-only path, and the forward values of the two paths are bitwise equal.

The curvature ``c`` is a Python number, which makes exactly the calls described above, or a 1-element float32 tensor on the inputs' device
(DESIGN.md 4w): the kernels then read it from the device -- it is never brought to the host, so the calls can be captured into a graph --
with results bitwise those of the float call at its value, and when it requires grad it gets a gradient of its own shape from the same
backward kernels (the tensor gradients stay bitwise those of the float path).  Any other tensor ``c`` raises ``capi.SttodeError`` before
any launch.  ``RiemannianGradient.c`` keeps a Python number; ``poincare_mean`` takes a tensor ``c`` only with ``differentiable=True``.

``mobius_matvec`` deviates from the reference in one place: a row with ``x m^T == 0`` gets a zero gradient (the reference: NaN).  ``_hyperbolic_softmax`` needs non-zero rows of ``A`` (the reference gives NaN for a zero row).
``poincare_mean``, ``oblique_proj`` and ``oblique_dist`` are FORWARD-ONLY by default: their results are cut off from the graph, and
``poincare_mean`` refuses a tensor ``c``.  The keyword ``differentiable=True`` opts in, as ``ops.mhgsa(differentiable=)`` does:
with grad mode on and an input that requires grad the result carries a graph whose backward pass is HIP (csrc/pmath_grad.hip: a group stage
and a row stage for the mean, fixed-order row sums for ``oblique_dist``), first order only; the forward bits are those of the call without
the keyword.  ``poincare_mean`` takes any rank >= 2 and any ``dim`` but the last, as the reference does, whatever the keyword.
``feature_clip(x, r)`` is not a function of the reference's pmath.py: it is the clipping of hyptorch/nn.py's ``ToPoincare(clip_r=r)``.
"""
import numpy as np
import torch
from torch.autograd.function import once_differentiable

from . import capi

_OPS = dict(project=0, lambda_x=1, mobius_add=2, dist=3, dist0=4, expmap=5, expmap0=6, logmap=7, logmap0=8, p2k=9, k2p=10,
            lorenz=11, oblique_proj=12)


def _prep(x):
    if not (isinstance(x, torch.Tensor) and x.is_cuda):
        raise capi.SttodeError('sttode_amd.pmath runs only on HIP tensors (no CPU fallback)')
    return x.to(torch.float32).contiguous()


def _wants_grad(*ts):
    return torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in ts)


def _curv(c, x):
    """The curvature as the entry points take it: a Python number as a float (the float-c entry points), a tensor as it is (the _c entry
    points, which read it on the device) after its dtype, size and device are checked -- by metadata alone, never by its value."""
    if not isinstance(c, torch.Tensor):
        return float(c)
    if c.dtype != torch.float32 or c.numel() != 1 or c.device != x.device:
        raise capi.SttodeError('a tensor curvature c must be a 1-element float32 tensor on the inputs\' device (%s): got %s, %d element(s), on %s'
                               % (x.device, c.dtype, c.numel(), c.device))
    return c


def _on_device(c):
    return isinstance(c, torch.Tensor)


def _gc_buffers(c, rows):
    """Workspace and result of dL/dc for an op of `rows` rows: one float64 per row, and the float that the finishing kernel writes."""
    return torch.empty(rows, dtype=torch.float64, device=c.device), torch.empty(1, dtype=torch.float32, device=c.device)


def _save_curv(ctx, c, *tensors):
    """Keeps a Function's tensors and its curvature for the backward pass: a tensor c with the tensors, a number as an attribute."""
    dev = isinstance(c, torch.Tensor)
    ctx.save_for_backward(*tensors, c if dev else None)
    ctx.c = None if dev else c


def _saved_curv(ctx):
    """(*tensors, c) as _save_curv took them."""
    saved = ctx.saved_tensors
    return saved if ctx.c is None else saved[:-1] + (ctx.c,)


def _wants(ctx, c):
    """Which gradients the backward entry point is given buffers for: needs_input_grad with a tensor c; all of them with a number, whose
    entry points require every buffer."""
    return ctx.needs_input_grad if _on_device(c) else (True,) * len(ctx.needs_input_grad)


def _bwd_call(name, c, want_c, gc_rows, *args):
    """Calls the backward entry point `name` (a number c) or name + '_c' (a tensor c, followed by dL/dc's float64 workspace of gc_rows
    rows and its result) with the curvature behind `args`.  Returns dL/dc in c's shape if want_c, else None."""
    if not _on_device(c):
        capi.call(name, *args, c, capi.stream_ptr())
        return None
    ws, gc = _gc_buffers(c, gc_rows)
    capi.call(name + '_c', *args, c, ws, gc, capi.stream_ptr())
    return gc.view(c.shape) if want_c else None


def _row(op, x, y=None, c=1.0, scalar=False, keepdim=False):
    x = _prep(x)
    if y is not None:
        y = _prep(y)
    c = _curv(c, x)
    if op != 'oblique_proj' and _wants_grad(x, y, c):
        return _RowOp.apply(x, y, op, c, scalar, keepdim)
    return _row_fwd(op, x, y, c, scalar, keepdim)


def _row_fwd(op, x, y, c, scalar, keepdim):
    if y is not None:
        x, y = torch.broadcast_tensors(x, y)
        x, y = x.contiguous(), y.contiguous()
    d = x.shape[-1]
    rows = x.numel() // d
    out = torch.empty(rows if scalar else (rows, d), dtype=torch.float32, device=x.device)
    capi.call('sttode_pmath_rowop_c' if _on_device(c) else 'sttode_pmath_rowop', _OPS[op], x, y, out, None, rows, d, c, capi.stream_ptr())
    if scalar:
        return out.view(*x.shape[:-1], 1) if keepdim else out.view(*x.shape[:-1])
    return out.view(x.shape)


class _RowOp(torch.autograd.Function):
    """A row op and its fused backward kernel (sttode_pmath_rowop_bwd; with a tensor c sttode_pmath_rowop_bwd_c, which also gives
    dL/dc).  Saves only its inputs; a broadcast operand's gradient is summed back to the operand's shape."""

    @staticmethod
    def forward(ctx, x, y, op, c, scalar, keepdim):
        _save_curv(ctx, c, x, y)
        ctx.op, ctx.scalar = op, scalar
        return _row_fwd(op, x, y, c, scalar, keepdim)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        x, y, c = _saved_curv(ctx)
        want_x, want_y, _, want_c, _, _ = _wants(ctx, c)
        return _row_bwd(ctx.op, x, y, c, g, ctx.scalar, want_x or want_y, want_c) + (None, None)


def _row_bwd(op, x, y, c, g, scalar, want_tensors, want_c):
    """The backward pass of a row op on broadcast operands: (gx, gy, None, gc), each gradient in its operand's shape."""
    xb, yb = x, y
    if y is not None:
        xb, yb = torch.broadcast_tensors(x, y)
        xb, yb = xb.contiguous(), yb.contiguous()
    d = xb.shape[-1]
    rows = xb.numel() // d
    g = _prep(g)
    assert g.numel() == (rows if scalar else rows * d)
    gx = torch.empty_like(xb) if want_tensors else None
    gy = torch.empty_like(yb) if want_tensors and y is not None else None
    gc = _bwd_call('sttode_pmath_rowop_bwd', c, want_c, rows, _OPS[op], xb, yb, g, gx, gy, rows, d)
    return gx.sum_to_size(x.shape) if gx is not None else None, gy.sum_to_size(y.shape) if gy is not None else None, None, gc


def _scalar(which, x):
    x = _prep(x)
    out = torch.empty_like(x)
    capi.call('sttode_pmath_scalar', which, x, out, x.numel(), capi.stream_ptr())
    return out


def tanh(x, clamp=15):
    assert clamp == 15
    return _scalar(0, x)


class Artanh(torch.autograd.Function):
    """hyptorch/pmath.py:16-27 (forward clamps to +-(1 - 1e-5); backward grad / (1 - x_clamped^2))."""

    @staticmethod
    def forward(ctx, x):
        ctx.save_for_backward(x)
        return _scalar(1, x)

    @staticmethod
    def backward(ctx, grad_output):
        (x,) = ctx.saved_tensors
        return _mul(grad_output, _scalar(3, x))


class Arsinh(torch.autograd.Function):
    """hyptorch/pmath.py:51-60."""

    @staticmethod
    def forward(ctx, x):
        ctx.save_for_backward(x)
        return _scalar(2, x)

    @staticmethod
    def backward(ctx, grad_output):
        (x,) = ctx.saved_tensors
        return _mul(grad_output, _scalar(4, x))


class RiemannianGradient(torch.autograd.Function):
    """hyptorch/pmath.py:30-45: identity forward, gradient rescaled by (1 - c |x|^2)^2 / 4 (class attribute ``c``)."""

    c = 1

    @staticmethod
    def forward(ctx, x):
        ctx.save_for_backward(x)
        return x.view_as(x)

    @staticmethod
    def backward(ctx, grad_output):
        (x,) = ctx.saved_tensors
        xs, g = _prep(x), _prep(grad_output)
        d = xs.shape[-1]
        out = torch.empty_like(g)
        capi.call('sttode_pmath_riemannian_grad', xs, g, out, xs.numel() // d, d, float(RiemannianGradient.c), capi.stream_ptr())
        return out.view_as(grad_output)


def _mul(a, b):
    a, b = _prep(a), _prep(b)
    out = torch.empty_like(a)
    capi.call('sttode_train_ewise', 0, out, a, b, None, None, out.numel(), 0, 0.0, capi.stream_ptr())
    return out


def artanh(x):
    return Artanh.apply(x)


def arsinh(x):
    return Arsinh.apply(x)


def project(x, *, c=1.0):
    return _row('project', x, c=c)


def lambda_x(x, *, c=1.0, keepdim=False):
    return _row('lambda_x', x, c=c, scalar=True, keepdim=keepdim)


def mobius_add(x, y, *, c=1.0):
    return _row('mobius_add', x, y, c=c)


def dist(x, y, *, c=1.0, keepdim=False):
    return _row('dist', x, y, c=c, scalar=True, keepdim=keepdim)


def dist0(x, *, c=1.0, keepdim=False):
    return _row('dist0', x, c=c, scalar=True, keepdim=keepdim)


def expmap(x, u, *, c=1.0):
    return _row('expmap', x, u, c=c)


def expmap0(u, *, c=1.0):
    return _row('expmap0', u, c=c)


def logmap(x, y, *, c=1.0):
    return _row('logmap', x, y, c=c)


def logmap0(y, *, c=1.0):
    return _row('logmap0', y, c=c)


def p2k(x, c):
    return _row('p2k', x, c=c)


def k2p(x, c):
    return _row('k2p', x, c=c)


def lorenz_factor(x, *, c=1.0, dim=-1, keepdim=False):
    assert dim in (-1, x.dim() - 1)
    return _row('lorenz', x, c=c, scalar=True, keepdim=keepdim)


def mobius_matvec(m, x, *, c=1.0):
    m, x = _prep(m), _prep(x)
    c = _curv(c, x)
    if _wants_grad(m, x, c):
        return _MatVec.apply(m, x, c)
    return _matvec_fwd(m, x, c)


def _matvec_fwd(m, x, c):
    O, d = m.shape
    rows = x.numel() // d
    mx = torch.empty(rows, O, dtype=torch.float32, device=x.device)
    xn = torch.empty(rows, dtype=torch.float32, device=x.device)
    out = torch.empty(rows, O, dtype=torch.float32, device=x.device)
    capi.call('sttode_pmath_matvec_c' if _on_device(c) else 'sttode_pmath_matvec', m, x, mx, xn, out, rows, d, O, c, capi.stream_ptr())
    return out.view(*x.shape[:-1], O)


class _MatVec(torch.autograd.Function):
    """mobius_matvec and its backward (sttode_pmath_matvec_bwd: a row kernel + the training GEMMs; with a tensor c
    sttode_pmath_matvec_bwd_c).  Saves only its inputs."""

    @staticmethod
    def forward(ctx, m, x, c):
        _save_curv(ctx, c, m, x)
        return _matvec_fwd(m, x, c)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        m, x, c = _saved_curv(ctx)
        want_m, want_x, want_c = _wants(ctx, c)
        O, d = m.shape
        rows = x.numel() // d
        g = _prep(g)
        f = dict(dtype=torch.float32, device=x.device)
        mx = torch.empty(rows, O, **f)
        gmx = torch.empty(rows, O, **f) if want_m or want_x else None
        gxn = None if _on_device(c) else torch.empty(rows, **f)   # an output only the float entry point requires; unused
        gx, gm = torch.empty_like(x) if want_x else None, torch.empty_like(m) if want_m else None
        return gm, gx, _bwd_call('sttode_pmath_matvec_bwd', c, want_c, rows, m, x, g, mx, gmx, gxn, gx, gm, rows, d, O)


class _DistMatrix(torch.autograd.Function):
    """dist_matrix and its backward (sttode_pmath_dist_matrix_bwd; with a tensor c sttode_pmath_dist_matrix_bwd_c).  Saves only its inputs."""

    @staticmethod
    def forward(ctx, x, y, c):
        _save_curv(ctx, c, x, y)
        return _pair(0, x, y, None, c, (x.shape[0], y.shape[0]))

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        x, y, c = _saved_curv(ctx)
        want_x, want_y, want_c = _wants(ctx, c)
        gx, gy = torch.empty_like(x) if want_x else None, torch.empty_like(y) if want_y else None
        return gx, gy, _bwd_call('sttode_pmath_dist_matrix_bwd', c, want_c, x.shape[0], x, y, _prep(g), gx, gy, x.shape[0], y.shape[0], x.shape[1])


def _pair(which, x, y, A, c, shape):
    x, y = _prep(x), _prep(y)
    out = torch.empty(shape, dtype=torch.float32, device=x.device)
    c = _curv(c, x)
    capi.call('sttode_pmath_pair_c' if _on_device(c) else 'sttode_pmath_pair', which, x, y, _prep(A) if A is not None else None, out,
              x.shape[0], y.shape[0], x.shape[1], c, capi.stream_ptr())
    return out


def dist_matrix(x, y, c=1.0):
    x, y = _prep(x), _prep(y)
    c = _curv(c, x)
    if _wants_grad(x, y, c):
        return _DistMatrix.apply(x, y, c)
    return _pair(0, x, y, None, c, (x.shape[0], y.shape[0]))


class _MobiusAdditionBatch(torch.autograd.Function):
    """_mobius_addition_batch and its backward: the forward is the pair kernel's; the backward is mobius_add's row kernel
    (sttode_pmath_rowop_bwd; with a tensor c sttode_pmath_rowop_bwd_c) on the broadcast operands, summed back to each operand's shape.
    Saves only its inputs."""

    @staticmethod
    def forward(ctx, x, y, c):
        _save_curv(ctx, c, x, y)
        return _pair(1, x, y, None, c, (x.shape[0], y.shape[0], x.shape[1]))

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        x, y, c = _saved_curv(ctx)
        want_x, want_y, want_c = _wants(ctx, c)
        gx, gy, _, gc = _row_bwd('mobius_add', x.unsqueeze(1), y.unsqueeze(0), c, g, False, want_x or want_y, want_c)
        return gx.view_as(x) if gx is not None else None, gy.view_as(y) if gy is not None else None, gc


def _mobius_addition_batch(x, y, c):
    x, y = _prep(x), _prep(y)
    c = _curv(c, x)
    if _wants_grad(x, y, c):
        return _MobiusAdditionBatch.apply(x, y, c)
    return _pair(1, x, y, None, c, (x.shape[0], y.shape[0], x.shape[1]))


class _HyperbolicSoftmax(torch.autograd.Function):
    """_hyperbolic_softmax and its backward (sttode_pmath_hsoftmax_bwd; with a tensor c sttode_pmath_hsoftmax_bwd_c).  Saves only its
    inputs."""

    @staticmethod
    def forward(ctx, X, A, P, c):
        _save_curv(ctx, c, X, A, P)
        return _pair(2, P, X, A, c, (X.shape[0], P.shape[0]))

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        X, A, P, c = _saved_curv(ctx)
        want_X, want_A, want_P, want_c = _wants(ctx, c)
        B, C, d = X.shape[0], P.shape[0], X.shape[1]
        ws = torch.empty(7 if _on_device(c) else 6, B, C, dtype=torch.float64, device=X.device)   # the seventh plane: g d logit / dc
        gX = torch.empty_like(X) if want_X else None
        gA, gP = (torch.empty_like(A), torch.empty_like(P)) if want_A or want_P else (None, None)
        gc = _bwd_call('sttode_pmath_hsoftmax_bwd', c, want_c, B, X, A, P, _prep(g), ws, gX, gA, gP, B, C, d)
        return gX, gA if want_A else None, gP if want_P else None, gc


def _hyperbolic_softmax(X, A, P, c):
    X, A, P = _prep(X), _prep(A), _prep(P)
    c = _curv(c, X)
    if _wants_grad(X, A, P, c):
        return _HyperbolicSoftmax.apply(X, A, P, c)
    return _pair(2, P, X, A, c, (X.shape[0], P.shape[0]))


def _clip_fwd(x, r):
    d = x.shape[-1]
    out = torch.empty_like(x)
    capi.call('sttode_pmath_clip', x, out, x.numel() // d, d, float(r), capi.stream_ptr())
    return out


class _FeatureClip(torch.autograd.Function):
    """feature_clip and its backward (sttode_pmath_clip_bwd).  Saves only x."""

    @staticmethod
    def forward(ctx, x, r):
        ctx.save_for_backward(x)
        ctx.r = r
        return _clip_fwd(x, r)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        d = x.shape[-1]
        gx = torch.empty_like(x)
        capi.call('sttode_pmath_clip_bwd', x, _prep(g), gx, x.numel() // d, d, ctx.r, capi.stream_ptr())
        return gx, None


def feature_clip(x, r):
    """x min(1, r / (|x| + 1e-5)) over the last dim: the clipping of hyptorch/nn.py's ToPoincare(clip_r=r) (nn.py:154-160)."""
    x = _prep(x)
    if _wants_grad(x):
        return _FeatureClip.apply(x, float(r))
    return _clip_fwd(x, float(r))


def _mean_shape(x, dim):
    """(outer, R, inner, d) of a mean over `dim` of x, and the result's shape: x as outer x R x inner rows of length d."""
    nd = x.dim()
    if nd < 2 or not -nd <= dim < nd:
        raise capi.SttodeError('poincare_mean takes points [..., d] of rank >= 2 and a dim inside it: got shape %s, dim %d' % (tuple(x.shape), dim))
    dim %= nd
    if dim == nd - 1:
        raise capi.SttodeError('poincare_mean: dim is the last (feature) dimension; the Lorentz factor is taken over the last dimension '
                               '(hyptorch/pmath.py:474), so a mean over it is not a mean of points')
    sh = tuple(x.shape)
    return int(np.prod(sh[:dim], dtype=np.int64)), sh[dim], int(np.prod(sh[dim + 1:-1], dtype=np.int64)), sh[-1], sh[:dim] + sh[dim + 1:]


def _mean_fwd(x, geom, c):
    outer, R, inner, d, shape = geom
    yl = torch.empty_like(x)
    lam = torch.empty(outer * R * inner, dtype=torch.float32, device=x.device)
    out = torch.empty(shape, dtype=torch.float32, device=x.device)
    if outer == 1 and inner == 1 and not _on_device(c):     # [rows, d] over dim 0 with a float c: the call this function always made
        capi.call('sttode_pmath_mean', x, yl, lam, out, R, d, c, capi.stream_ptr())
    else:
        capi.call('sttode_pmath_mean_seg', x, yl, lam, out, None, None, outer, R, inner, d, 0.0 if _on_device(c) else c,
                  c if _on_device(c) else None, capi.stream_ptr())
    return out


class _PoincareMean(torch.autograd.Function):
    """poincare_mean and its backward (sttode_pmath_mean_bwd; with a tensor c sttode_pmath_mean_bwd_c, which also gives dL/dc).  Saves
    only its inputs: the backward recomputes the Klein sums in float64."""

    @staticmethod
    def forward(ctx, x, geom, c):
        _save_curv(ctx, c, x)
        ctx.geom = geom
        return _mean_fwd(x, geom, c)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        x, c = _saved_curv(ctx)
        want_x, _, want_c = _wants(ctx, c)
        outer, R, inner, d, _ = ctx.geom
        groups = outer * inner
        g = _prep(g)
        assert g.numel() == groups * d
        gS = torch.empty(groups * d, dtype=torch.float64, device=x.device)
        gL = torch.empty(groups, dtype=torch.float64, device=x.device)
        gx = torch.empty_like(x) if want_x else None
        return gx, None, _bwd_call('sttode_pmath_mean_bwd', c, want_c, groups * R + groups, x, g, gS, gL, gx, outer, R, inner, d)


def poincare_mean(x, dim=0, c=1.0, *, differentiable=False):
    """hyptorch/pmath.py:472-479: the Einstein midpoint over `dim` (any but the last) of points [..., d]; the result has x's shape without
    `dim`.  differentiable=True: the result carries a graph (x, and a 1-element float32 tensor c), see the module docstring."""
    if isinstance(c, torch.Tensor) and not differentiable:
        raise capi.SttodeError('poincare_mean takes a Python number as c: it is forward-only, so a tensor curvature would get no gradient here')
    x = _prep(x)
    geom = _mean_shape(x, dim)
    if 0 in x.shape:
        raise capi.SttodeError('poincare_mean: empty shape %s' % (tuple(x.shape),))
    c = _curv(c, x)
    if differentiable and _wants_grad(x, c):
        return _PoincareMean.apply(x, geom, c)
    return _mean_fwd(x.detach(), geom, c.detach() if _on_device(c) else c)


def auto_select_c(d):
    """Ball radius such that the d-dimensional ball has volume pi (host arithmetic, pmath.py:496-505)."""
    from scipy.special import gamma
    dim2 = d / 2.0
    R = gamma(dim2 + 1) / (np.pi ** (dim2 - 1))
    R = R ** (1 / float(d))
    return 1 / (R ** 2)


# Oblique manifold (core/manifolds/oblique.py)
class _ObliqueProj(torch.autograd.Function):
    """oblique_proj and its backward (sttode_oblique_proj_bwd).  Saves only p."""

    @staticmethod
    def forward(ctx, p):
        ctx.save_for_backward(p)
        return _row_fwd('oblique_proj', p, None, 1.0, False, False)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        (p,) = ctx.saved_tensors
        d = p.shape[-1]
        gp = torch.empty_like(p)
        capi.call('sttode_oblique_proj_bwd', p, _prep(g), gp, p.numel() // d, d, capi.stream_ptr())
        return gp


def oblique_proj(p, *, differentiable=False):
    if differentiable and _wants_grad(p):
        return _ObliqueProj.apply(_prep(p))
    return _row('oblique_proj', p)


def _oblique_dist_fwd(p1, p2):
    n1, n2, d = p1.shape[-2], p2.shape[-2], p1.shape[-1]
    nb = p1.numel() // (n1 * d)
    out = torch.empty(*p1.shape[:-2], n2, n1, dtype=torch.float32, device=p1.device)
    capi.call('sttode_oblique_dist', p1, p2, out, nb, n1, n2, d, capi.stream_ptr())
    return out


class _ObliqueDist(torch.autograd.Function):
    """oblique_dist and its backward (sttode_oblique_dist_bwd).  Saves only its inputs."""

    @staticmethod
    def forward(ctx, p1, p2):
        ctx.save_for_backward(p1, p2)
        return _oblique_dist_fwd(p1, p2)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        p1, p2 = ctx.saved_tensors
        n1, n2, d = p1.shape[-2], p2.shape[-2], p1.shape[-1]
        want1, want2 = ctx.needs_input_grad
        g1, g2 = torch.empty_like(p1) if want1 else None, torch.empty_like(p2) if want2 else None
        capi.call('sttode_oblique_dist_bwd', p1, p2, _prep(g), g1, g2, p1.numel() // (n1 * d), n1, n2, d, capi.stream_ptr())
        return g1, g2


def oblique_dist(p1, p2, *, differentiable=False):
    """Oblique.dist(p1, p2): [..., n1, d], [..., n2, d] -> [..., n2, n1].  differentiable=True: see the module docstring; the clamp at
    +-(1 - 1e-4) has torch.clamp's gradient."""
    p1, p2 = _prep(p1), _prep(p2)
    if differentiable and _wants_grad(p1, p2):
        return _ObliqueDist.apply(p1, p2)
    return _oblique_dist_fwd(p1, p2)
