"""Manifolds for Riemannian optimisation on HIP: the drop-in for core/manifolds (``Manifold``, ``ManifoldParameter``, ``Euclidean``,
``Oblique``), plus ``PoincareBall(c)``, the ball that ``sttode_amd.pmath`` and ``sttode_amd.hypnn`` work on.

Names, constructor signatures and argument orders are the reference's: ``expmap(u, p)``, ``proj_tan(u, p)``, ``ptransp(x, y, u)``,
``retr_transp(x, u, v)``.  ``sttode_amd.optim.RiemannianAdam`` / ``RiemannianSGD`` step a ``ManifoldParameter`` on its ``.manifold``.

All operations act on the last dimension and take any leading shape, with broadcast operands as ``pmath`` does.  They take fp32 HIP
tensors only: anything else raises ``capi.SttodeError`` (no CPU fallback).  ``Euclidean`` is the exception, its methods are the
reference's one-line identities and adds in plain torch.

The operations are FORWARD-ONLY by default: they run under ``no_grad`` semantics, on detached operands, and their results never require
grad.  ``differentiable(manifold)`` opts a manifold object in (the method signatures are the reference's, so it cannot be a
keyword): it sets ``manifold.differentiable = True`` and returns the manifold, and from then on every operation of that object is
differentiable in its tensor operands -- with grad mode on and an operand that requires grad the result carries a graph whose backward
pass is one HIP launch (``sttode_manifold_rowop_bwd``; ``proj`` / ``expmap`` / ``logmap`` / ``dist`` of the ball and ``proj`` / ``dist``
of Oblique go through ``pmath``'s own backward kernels), first order only.  Branches differentiate as taken: Oblique ``expmap`` below
``|u| = 1e-4`` as ``proj(p + u)``, the ball's ``retr`` through ``project``'s clip.  Forward bits are the same either way; without the flag,
under ``no_grad`` or with no operand that requires grad the calls are exactly the forward-only ones.  ``PoincareBall.c`` stays a Python
float, and the Riemannian optimisers never build a graph.

Where this deviates from the reference:
  * ``Oblique.inner`` and ``Oblique.logmap`` raise ``NotImplementedError``.  The reference's ``inner`` is a batched matmul that ignores
    ``p``; its ``logmap`` multiplies ``[n, d]`` by the ``[n, n]`` matrix ``dist`` returns and fails for every ``n != d`` with ``n > 1``.
  * ``Oblique.retr`` / ``retr_transp`` renormalise the row after the exponential map (the identity on the manifold in exact arithmetic);
    ``Oblique.expmap`` does not.
  * ``PoincareBall`` is not in the reference's package.  Its ``ptransp`` is the closed-form gyration in float64, not a composition of the
    reference's ``mobius_add``, whose ``+ 1e-5`` puts such a composition 1e-2 off.
"""
import math

import torch
from torch.autograd.function import once_differentiable
from torch.nn import Parameter

from . import capi, pmath

EPS = {torch.float32: 1e-4, torch.float64: 1e-7}


def _operands(*ts):
    """Detached fp32 HIP operands, broadcast against each other and made contiguous."""
    out = []
    for t in ts:
        if t is None:
            out.append(None)
            continue
        if not (isinstance(t, torch.Tensor) and t.is_cuda):
            raise capi.SttodeError('sttode_amd.manifolds runs only on HIP tensors (no CPU fallback)')
        if t.dtype != torch.float32:
            raise capi.SttodeError(f'sttode_amd.manifolds takes float32 tensors, got {t.dtype}')
        if t.dim() == 0:
            raise capi.SttodeError('sttode_amd.manifolds: operands need a last dimension to act on')
        out.append(t.detach())
    live = [t for t in out if t is not None]
    if len(live) > 1:
        bc = iter(torch.broadcast_tensors(*live))
        out = [None if t is None else next(bc) for t in out]
    return [None if t is None else t.contiguous() for t in out]


def _live(*ts):
    """Does grad mode ask for a graph through these operands?"""
    return torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in ts)


def differentiable(manifold):
    """Opt a manifold object in to gradients through its operations (the module docstring); returns the manifold."""
    manifold.differentiable = True
    return manifold


class _RowOpGrad(torch.autograd.Function):
    """A manifold row op and its backward kernel (sttode_manifold_rowop_bwd, one launch).  Saves only its operands; a broadcast operand's
    gradient is summed back to the operand's shape."""

    @staticmethod
    def forward(ctx, a, b, w, op, manifold, c, scalar, keepdim):
        ctx.save_for_backward(a, b, w)
        ctx.op, ctx.manifold, ctx.c = op, manifold, c
        out = _rowop(op, manifold, c, a, b, w, scalar, keepdim)
        if op == 'retr_transp':
            ctx.set_materialize_grads(False)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g, g2=None):
        a, b, w = ctx.saved_tensors
        ab, bb, wb = _operands(a, b, w)
        d = ab.shape[-1]
        rows = ab.numel() // d
        two = ctx.op == 'retr_transp'
        if two and g is None and g2 is None:
            return (None,) * 8
        g, g2 = [None if t is None else t.to(torch.float32).contiguous() for t in (g, g2 if two else None)]
        want = ctx.needs_input_grad
        takes_w = wb is not None and ctx.op in ('ptransp', 'retr_transp', 'inner')
        ga = torch.empty_like(ab) if want[0] else None
        gb = torch.empty_like(bb) if want[1] else None
        gw = torch.empty_like(wb) if takes_w and want[2] else None
        if rows and (ga is not None or gb is not None or gw is not None):
            with torch.cuda.device(ab.device):
                capi.call('sttode_manifold_rowop_bwd', capi.MANIFOLD_OPS[ctx.op], capi.MANIFOLDS[ctx.manifold], ab, bb, wb if takes_w else None,
                          g, g2, ga, gb, gw, rows, d, float(ctx.c), capi.stream_ptr())
        return (None if ga is None else ga.sum_to_size(a.shape), None if gb is None else gb.sum_to_size(b.shape),
                None if gw is None else gw.sum_to_size(w.shape), None, None, None, None, None)


def _op(man, op, a, b, w=None, scalar=False, keepdim=False):
    """A row op of manifold `man`: the forward-only call, or on a differentiable manifold with a live operand the autograd function."""
    c = getattr(man, 'c', 1.0)
    if man.differentiable and _live(a, b, w):
        _operands(a, b, w)      # (the operand checks, before autograd sees them)
        return _RowOpGrad.apply(a, b, w, op, man._code, c, scalar, keepdim)
    return _rowop(op, man._code, c, a, b, w, scalar, keepdim)


def _rowop(op, manifold, c, a, b, w=None, scalar=False, keepdim=False):
    with torch.no_grad():
        a, b, w = _operands(a, b, w)
        d = a.shape[-1]
        rows = a.numel() // d
        two = op == 'retr_transp'
        out = torch.empty(a.shape[:-1] if scalar else a.shape, dtype=torch.float32, device=a.device)
        out2 = torch.empty_like(a) if two else None
        if rows:
            with torch.cuda.device(a.device):
                capi.call('sttode_manifold_rowop', capi.MANIFOLD_OPS[op], capi.MANIFOLDS[manifold], a, b, w, out, out2, rows, d, float(c),
                          capi.stream_ptr())
        if scalar and keepdim:
            out = out.unsqueeze(-1)
        return (out, out2) if two else out


def _detached(fn, *ts, **kw):
    """A differentiable pmath function as a forward-only operation."""
    with torch.no_grad():
        return fn(*[t.detach() if isinstance(t, torch.Tensor) else t for t in ts], **kw)


def _routed(man, fn, *ts, **kw):
    """A pmath function as an operation of `man`: forward-only, or on a differentiable manifold with a live operand, itself."""
    if man.differentiable and _live(*ts):
        for t in ts:
            if isinstance(t, torch.Tensor) and t.dtype != torch.float32:
                raise capi.SttodeError(f'sttode_amd.manifolds takes float32 tensors, got {t.dtype}')
        return fn(*ts, **kw)
    return _detached(fn, *ts, **kw)


class Manifold(object):
    """Abstract class to define operations on a manifold (core/manifolds/base.py: the same method list)."""

    differentiable = False      # set by manifolds.differentiable(manifold): the operations of that object build a graph

    def __init__(self):
        super().__init__()
        self.eps = 10e-8

    def sqdist(self, p1, p2):
        """Squared distance between pairs of points."""
        raise NotImplementedError

    def egrad2rgrad(self, p, dp):
        """Converts Euclidean gradients to Riemannian gradients."""
        raise NotImplementedError

    def proj(self, p):
        """Projects point p on the manifold."""
        raise NotImplementedError

    def proj_tan(self, u, p):
        """Projects u on the tangent space of p."""
        raise NotImplementedError

    def proj_tan0(self, u):
        """Projects u on the tangent space of the origin."""
        raise NotImplementedError

    def expmap(self, u, p):
        """Exponential map of u at point p."""
        raise NotImplementedError

    def logmap(self, p1, p2):
        """Logarithmic map of point p1 at point p2."""
        raise NotImplementedError

    def init_weights(self, w, irange=1e-5):
        """Initializes random weights on the manifold."""
        raise NotImplementedError

    def inner(self, p, u, v=None, keepdim=False):
        """Inner product for tangent vectors at point p."""
        raise NotImplementedError

    def ptransp(self, x, y, u):
        """Parallel transport of u from x to y."""
        raise NotImplementedError

    def ptransp0(self, x, u):
        """Parallel transport of u from the origin to x."""
        raise NotImplementedError

    def retr(self, x, u):
        """Retraction from point x with direction u."""
        raise NotImplementedError

    def retr_transp(self, x, u, v):
        """Retraction and vector transport at once."""
        raise NotImplementedError


class ManifoldParameter(Parameter):
    """Subclass of torch.nn.Parameter for Riemannian optimization."""

    def __new__(cls, data, requires_grad, manifold):
        return Parameter.__new__(cls, data, requires_grad)

    def __init__(self, data, requires_grad, manifold):
        self.manifold = manifold

    def __repr__(self):
        return '{} Parameter containing:\n'.format(self.manifold.name) + super(Parameter, self).__repr__()


class Euclidean(Manifold):
    """Euclidean manifold (core/manifolds/euclidean.py): identities and adds, in plain torch."""

    def __init__(self):
        super(Euclidean, self).__init__()
        self.name = 'Euclidean'

    def normalize(self, p):
        p.view(-1, p.size(-1)).renorm_(2, 0, 1.)
        return p

    def sqdist(self, p1, p2):
        return (p1 - p2).pow(2).sum(dim=-1)

    def egrad2rgrad(self, p, dp):
        return dp

    def proj(self, p):
        return p

    def proj_tan(self, u, p):
        return u

    def proj_tan0(self, u):
        return u

    def expmap(self, u, p):
        return p + u

    def logmap(self, p1, p2):
        return p2 - p1

    def expmap0(self, u):
        return u

    def logmap0(self, p):
        return p

    def mobius_add(self, x, y, dim=-1):
        return x + y

    def mobius_matvec(self, m, x):
        return x @ m.transpose(-1, -2)

    def init_weights(self, w, irange=1e-5):
        w.data.uniform_(-irange, irange)
        return w

    def inner(self, p, u, v=None, keepdim=False):
        return (u * (u if v is None else v)).sum(dim=-1, keepdim=keepdim)

    def ptransp(self, x, y, v):
        return v

    def ptransp0(self, x, v):
        return x + v

    def retr(self, x, u):
        return self.expmap(u, x)

    def retr_transp(self, x, u, v):
        y = self.retr(x, u)
        return y, self.ptransp(x, y, v)


class Oblique(Manifold):
    """Rows of unit norm (core/manifolds/oblique.py)."""

    _code = 'oblique'

    def __init__(self):
        super().__init__()
        self.name = 'Oblique'

    def proj(self, p):
        return _routed(self, pmath.oblique_proj, p, **({'differentiable': True} if self.differentiable else {}))

    def proj_tan(self, u, p):
        return _op(self, 'proj_tan', p, u)

    def egrad2rgrad(self, p, dp):
        return _op(self, 'proj_tan', p, dp)

    def expmap(self, u, p):
        return _op(self, 'expmap', p, u)

    def dist(self, p1, p2, keepdim=False):
        if keepdim:
            raise NotImplementedError('Oblique.dist returns the [..., n2, n1] matrix of the reference, which has no reduced dimension to keep')
        return _routed(self, pmath.oblique_dist, p1, p2, **({'differentiable': True} if self.differentiable else {}))

    def logmap(self, p1, p2):
        raise NotImplementedError("Oblique.logmap: the reference multiplies the [n, d] tangent projection by the [n, n] matrix its dist returns, "
                                  'which fails for every n != d with n > 1; there is no behaviour to reproduce')

    def inner(self, p, u, v=None, keepdim=False):
        raise NotImplementedError("Oblique.inner: the reference's inner is the batched matmul u @ v^T and ignores p, it is not an inner product "
                                  'of tangent vectors at p; the optimisers use the row-wise <u, v> on the device')

    def ptransp(self, x, y, u):
        return _op(self, 'ptransp', x, y, u)

    def retr(self, x, u):
        return _op(self, 'retr', x, u)

    def retr_transp(self, x, u, v):
        return _op(self, 'retr_transp', x, u, v)


class PoincareBall(Manifold):
    """The Poincare ball of curvature -c of sttode_amd.pmath (hyptorch/pmath.py).  c: a Python float > 0."""

    _code = 'poincare'

    def __init__(self, c=1.0):
        super().__init__()
        if isinstance(c, torch.Tensor):
            raise ValueError('PoincareBall: c must be a positive finite Python float, not a tensor: the manifold ops and the Riemannian '
                             'optimisers take the curvature as a launch argument and give it no gradient (a trainable curvature is '
                             'pmath\'s and hypnn\'s: DESIGN.md 4w)')
        if isinstance(c, (bool, torch.Tensor)) or not isinstance(c, (int, float)) or not (0 < c < math.inf):
            raise ValueError(f'PoincareBall: c must be a positive finite Python float, got {c!r}')
        self.c = float(c)
        self.name = 'PoincareBall'

    def proj(self, p):
        return _routed(self, pmath.project, p, c=self.c)

    def proj_tan(self, u, p):
        return self._identity(u)

    def proj_tan0(self, u):
        return self._identity(u)

    def _identity(self, u):
        if self.differentiable and _live(u):
            _operands(u)
            return u.contiguous()
        return _operands(u)[0]

    def egrad2rgrad(self, p, dp):
        return _op(self, 'proj_tan', p, dp)

    def expmap(self, u, p):
        return _routed(self, pmath.expmap, p, u, c=self.c)

    def logmap(self, p1, p2):
        return _routed(self, pmath.logmap, p2, p1, c=self.c)

    def dist(self, p1, p2, keepdim=False):
        return _routed(self, pmath.dist, p1, p2, c=self.c, keepdim=keepdim)

    def sqdist(self, p1, p2):
        return self.dist(p1, p2).pow(2)

    def inner(self, p, u, v=None, keepdim=False):
        return _op(self, 'inner', p, u, v, scalar=True, keepdim=keepdim)

    def ptransp(self, x, y, u):
        return _op(self, 'ptransp', x, y, u)

    def retr(self, x, u):
        return _op(self, 'retr', x, u)

    def retr_transp(self, x, u, v):
        return _op(self, 'retr_transp', x, u, v)
