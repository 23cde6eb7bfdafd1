"""Poincare-ball math on HIP: same function names / argument meaning as hyptorch/pmath.py, forward values and gradients.

Every function takes CUDA(HIP) fp32 tensors and raises on CPU tensors (no fallback).  Leading dims are flattened to
rows; the last dim is the feature dim.  ``auto_select_c`` is host arithmetic (scipy gamma, pmath.py:496-505).

Gradients: ``project, lambda_x, mobius_add, dist, dist0, expmap, expmap0, logmap, logmap0, p2k, k2p, lorenz_factor``,
``mobius_matvec``, ``dist_matrix``, ``_mobius_addition_batch``, ``_hyperbolic_softmax`` and ``feature_clip`` are differentiable with respect
to their tensor arguments (``artanh``, ``arsinh`` and ``RiemannianGradient`` always were): fused backward kernels (csrc/pmath_grad.hip,
DESIGN.md 4q and 4r), first order only (``once_differentiable``).  A function takes that path only when grad mode is on and an input requires
grad; otherwise it makes exactly the calls of the forward-only path, and the forward values of the two paths are bitwise equal.  ``c`` is a
Python float and gets no gradient.  ``mobius_matvec`` deviates from the reference in one place: a row with ``x m^T == 0`` gets a zero
gradient (the reference: NaN).  ``_hyperbolic_softmax`` needs non-zero rows of ``A`` (the reference gives NaN for a zero row).
``poincare_mean`` and the Oblique ops stay FORWARD-ONLY: their results are cut off from the graph.
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
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in ts)


def _row(op, x, y=None, c=1.0, scalar=False, keepdim=False):
    x = _prep(x)
    if y is not None:
        y = _prep(y)
    if op != 'oblique_proj' and _wants_grad(x, y):
        return _RowOp.apply(x, y, op, float(c), scalar, keepdim)
    return _row_fwd(op, x, y, c, scalar, keepdim)


def _row_fwd(op, x, y, c, scalar, keepdim):
    if y is not None:
        x, y = torch.broadcast_tensors(x, y)
        x, y = x.contiguous(), y.contiguous()
    d = x.shape[-1]
    rows = x.numel() // d
    out = torch.empty(rows if scalar else (rows, d), dtype=torch.float32, device=x.device)
    capi.call('sttode_pmath_rowop', _OPS[op], x, y, out, None, rows, d, float(c), capi.stream_ptr())
    if scalar:
        return out.view(*x.shape[:-1], 1) if keepdim else out.view(*x.shape[:-1])
    return out.view(x.shape)


class _RowOp(torch.autograd.Function):
    """A row op and its fused backward kernel (sttode_pmath_rowop_bwd).  Saves only its inputs; a broadcast operand's gradient is
    summed back to the operand's shape."""

    @staticmethod
    def forward(ctx, x, y, op, c, scalar, keepdim):
        ctx.save_for_backward(x, y)
        ctx.op, ctx.c, ctx.scalar = op, c, scalar
        return _row_fwd(op, x, y, c, scalar, keepdim)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        x, y = ctx.saved_tensors
        xb, yb = x, y
        if y is not None:
            xb, yb = torch.broadcast_tensors(x, y)
            xb, yb = xb.contiguous(), yb.contiguous()
        d = xb.shape[-1]
        rows = xb.numel() // d
        g = _prep(g)
        assert g.numel() == (rows if ctx.scalar else rows * d)
        gx = torch.empty_like(xb)
        gy = torch.empty_like(yb) if y is not None else None
        capi.call('sttode_pmath_rowop_bwd', _OPS[ctx.op], xb, yb, g, gx, gy, rows, d, ctx.c, capi.stream_ptr())
        return gx.sum_to_size(x.shape), (gy.sum_to_size(y.shape) if y is not None else None), None, None, None, None


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
    if _wants_grad(m, x):
        return _MatVec.apply(m, x, float(c))
    return _matvec_fwd(m, x, c)


def _matvec_fwd(m, x, c):
    O, d = m.shape
    rows = x.numel() // d
    mx = torch.empty(rows, O, dtype=torch.float32, device=x.device)
    xn = torch.empty(rows, dtype=torch.float32, device=x.device)
    out = torch.empty(rows, O, dtype=torch.float32, device=x.device)
    capi.call('sttode_pmath_matvec', m, x, mx, xn, out, rows, d, O, float(c), capi.stream_ptr())
    return out.view(*x.shape[:-1], O)


class _MatVec(torch.autograd.Function):
    """mobius_matvec and its backward (sttode_pmath_matvec_bwd: a row kernel + the training GEMMs).  Saves only m and x."""

    @staticmethod
    def forward(ctx, m, x, c):
        ctx.save_for_backward(m, x)
        ctx.c = c
        return _matvec_fwd(m, x, c)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        m, x = ctx.saved_tensors
        O, d = m.shape
        rows = x.numel() // d
        g = _prep(g)
        f = dict(dtype=torch.float32, device=x.device)
        mx, gmx, gxn = torch.empty(rows, O, **f), torch.empty(rows, O, **f), torch.empty(rows, **f)   # gxn: an output the entry point requires; unused
        gx, gm = torch.empty_like(x), torch.empty_like(m)
        capi.call('sttode_pmath_matvec_bwd', m, x, g, mx, gmx, gxn, gx, gm, rows, d, O, ctx.c, capi.stream_ptr())
        return gm, gx, None


class _DistMatrix(torch.autograd.Function):
    """dist_matrix and its backward (sttode_pmath_dist_matrix_bwd).  Saves only x and y."""

    @staticmethod
    def forward(ctx, x, y, c):
        ctx.save_for_backward(x, y)
        ctx.c = c
        return _pair(0, x, y, None, c, (x.shape[0], y.shape[0]))

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        x, y = ctx.saved_tensors
        gx, gy = torch.empty_like(x), torch.empty_like(y)
        capi.call('sttode_pmath_dist_matrix_bwd', x, y, _prep(g), gx, gy, x.shape[0], y.shape[0], x.shape[1], ctx.c, capi.stream_ptr())
        return gx, gy, None


def _pair(which, x, y, A, c, shape):
    x, y = _prep(x), _prep(y)
    out = torch.empty(shape, dtype=torch.float32, device=x.device)
    capi.call('sttode_pmath_pair', which, x, y, _prep(A) if A is not None else None, out, x.shape[0], y.shape[0], x.shape[1], float(c),
              capi.stream_ptr())
    return out


def dist_matrix(x, y, c=1.0):
    x, y = _prep(x), _prep(y)
    if _wants_grad(x, y):
        return _DistMatrix.apply(x, y, float(c))
    return _pair(0, x, y, None, c, (x.shape[0], y.shape[0]))


class _MobiusAdditionBatch(torch.autograd.Function):
    """_mobius_addition_batch and its backward: the forward is the pair kernel's; the backward is mobius_add's row kernel
    (sttode_pmath_rowop_bwd) on the broadcast operands, summed back to each operand's shape.  Saves only x and y."""

    @staticmethod
    def forward(ctx, x, y, c):
        ctx.save_for_backward(x, y)
        ctx.c = c
        return _pair(1, x, y, None, c, (x.shape[0], y.shape[0], x.shape[1]))

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        x, y = ctx.saved_tensors
        shape = (x.shape[0], y.shape[0], x.shape[1])
        xb, yb = x.unsqueeze(1).expand(shape).contiguous(), y.unsqueeze(0).expand(shape).contiguous()
        gx, gy = torch.empty_like(xb), torch.empty_like(yb)
        capi.call('sttode_pmath_rowop_bwd', _OPS['mobius_add'], xb, yb, _prep(g), gx, gy, shape[0] * shape[1], shape[2], ctx.c, capi.stream_ptr())
        return gx.sum_to_size(x.unsqueeze(1).shape).view_as(x), gy.sum_to_size(y.unsqueeze(0).shape).view_as(y), None


def _mobius_addition_batch(x, y, c):
    x, y = _prep(x), _prep(y)
    if _wants_grad(x, y):
        return _MobiusAdditionBatch.apply(x, y, float(c))
    return _pair(1, x, y, None, float(c), (x.shape[0], y.shape[0], x.shape[1]))


class _HyperbolicSoftmax(torch.autograd.Function):
    """_hyperbolic_softmax and its backward (sttode_pmath_hsoftmax_bwd).  Saves only X, A and P."""

    @staticmethod
    def forward(ctx, X, A, P, c):
        ctx.save_for_backward(X, A, P)
        ctx.c = c
        return _pair(2, P, X, A, c, (X.shape[0], P.shape[0]))

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        X, A, P = ctx.saved_tensors
        B, C, d = X.shape[0], P.shape[0], X.shape[1]
        ws = torch.empty(6, B, C, dtype=torch.float64, device=X.device)
        gX, gA, gP = torch.empty_like(X), torch.empty_like(A), torch.empty_like(P)
        capi.call('sttode_pmath_hsoftmax_bwd', X, A, P, _prep(g), ws, gX, gA, gP, B, C, d, ctx.c, capi.stream_ptr())
        return gX, gA, gP, None


def _hyperbolic_softmax(X, A, P, c):
    X, A, P = _prep(X), _prep(A), _prep(P)
    if _wants_grad(X, A, P):
        return _HyperbolicSoftmax.apply(X, A, P, float(c))
    return _pair(2, P, X, A, float(c), (X.shape[0], P.shape[0]))


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


def poincare_mean(x, dim=0, c=1.0):
    assert dim == 0 and x.dim() == 2
    x = _prep(x)
    rows, d = x.shape
    yl = torch.empty_like(x)
    lam = torch.empty(rows, dtype=torch.float32, device=x.device)
    out = torch.empty(d, dtype=torch.float32, device=x.device)
    capi.call('sttode_pmath_mean', x, yl, lam, out, rows, d, float(c), capi.stream_ptr())
    return out


def auto_select_c(d):
    """Ball radius such that the d-dimensional ball has volume pi (host arithmetic, pmath.py:496-505)."""
    from scipy.special import gamma
    dim2 = d / 2.0
    R = gamma(dim2 + 1) / (np.pi ** (dim2 - 1))
    R = R ** (1 / float(d))
    return 1 / (R ** 2)


# Oblique manifold (core/manifolds/oblique.py)
def oblique_proj(p):
    return _row('oblique_proj', p)


def oblique_dist(p1, p2):
    """Oblique.dist(p1, p2): [..., n1, d], [..., n2, d] -> [..., n2, n1]."""
    p1, p2 = _prep(p1), _prep(p2)
    n1, n2, d = p1.shape[-2], p2.shape[-2], p1.shape[-1]
    nb = p1.numel() // (n1 * d)
    out = torch.empty(*p1.shape[:-2], n2, n1, dtype=torch.float32, device=p1.device)
    capi.call('sttode_oblique_dist', p1, p2, out, nb, n1, n2, d, capi.stream_ptr())
    return out
