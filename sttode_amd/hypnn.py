"""Hyperbolic layers on HIP with the public surface of hyptorch/nn.py: the same class names, constructor and ``forward`` signatures,
attribute and parameter names, repr strings and initial values, so a checkpoint of the reference's modules loads with ``strict=True``.

Every ``forward`` is a short chain of ``sttode_amd.pmath`` calls: it trains through their fused backward kernels and,
like them, raises on CPU tensors.  The only torch arithmetic is parameter-sized (``HyperbolicMLR`` scales its normals by ``1 - c |p|^2``);
nothing batch-sized goes through torch.

The curvature ``c`` -- a constructor argument, and the per-call ``c=`` of the four layers that have one -- is a Python number or a 1-element
float32 tensor on the device, passed through to pmath.  An ``nn.Parameter`` given as ``c`` is registered under the name
``c`` and trained: ``ToPoincare(c=nn.Parameter(torch.tensor([0.7])))`` has the state dict of the reference's ``ToPoincare(0.7, train_c=True)``,
and one Parameter handed to several layers is one shared, learned curvature.  The constructor flag ``train_c=True`` itself stays refused;
its message names this spelling.
"""
import math

import torch
from torch import nn

from . import pmath


def _curvature(module, c):
    """The optional ``c=`` of a forward call: the module's own curvature unless the caller gives one."""
    return module.c if c is None else c


def _init_like_linear(weight, bias=None):
    """torch.nn.Linear's initialisation (the draws, and their order, that give the reference's initial values under one seed)."""
    nn.init.kaiming_uniform_(weight, a=math.sqrt(5))
    if bias is not None:
        span = 1 / math.sqrt(weight.shape[1])
        nn.init.uniform_(bias, -span, span)


class HyperbolicMLR(nn.Module):
    """Multiclass logistic regression on the ball: logits [rows, n_classes] of points x [rows, ball_dim].  ``p_vals`` are the
    hyperplanes' offsets as tangent vectors at the origin, ``a_vals`` their normals before the conformal rescaling."""

    def __init__(self, ball_dim, n_classes, c):
        super().__init__()
        self.ball_dim, self.n_classes, self.c = ball_dim, n_classes, c
        for name in ('a_vals', 'p_vals'):                         # registration order is state_dict order
            setattr(self, name, nn.Parameter(torch.empty(n_classes, ball_dim)))
        self.reset_parameters()

    def reset_parameters(self):
        for w in (self.a_vals, self.p_vals):
            _init_like_linear(w)

    def forward(self, x, c=None):
        c = _curvature(self, c)
        offsets = pmath.expmap0(self.p_vals, c=c)
        normals = self.a_vals * (1 - c * offsets.square().sum(-1, keepdim=True))
        return pmath._hyperbolic_softmax(x, normals, offsets, c)

    def extra_repr(self):
        return f'Poincare ball dim={self.ball_dim}, n_classes={self.n_classes}, c={self.c}'


class HypLinear(nn.Module):
    """Moebius matrix-vector product, then an optional bias (a tangent vector at the origin) added on the ball."""

    def __init__(self, in_features, out_features, c, bias=True):
        super().__init__()
        self.in_features, self.out_features, self.c = in_features, out_features, c
        self.weight = nn.Parameter(torch.empty(out_features, in_features))
        self.register_parameter('bias', nn.Parameter(torch.empty(out_features)) if bias else None)
        self.reset_parameters()

    def reset_parameters(self):
        _init_like_linear(self.weight, self.bias)

    def forward(self, x, c=None):
        c = _curvature(self, c)
        out = pmath.mobius_matvec(self.weight, x, c=c)
        if self.bias is not None:
            # no c= here on purpose: the reference adds the bias at mobius_add's default curvature 1 whatever the layer's c
            out = pmath.mobius_add(out, pmath.expmap0(self.bias, c=c))
        return pmath.project(out, c=c)

    def extra_repr(self):
        return f'in_features={self.in_features}, out_features={self.out_features}, bias={self.bias is not None}, c={self.c}'


class ConcatPoincareLayer(nn.Module):
    """Two inputs of different width joined on the ball: the Moebius sum of one bias-free HypLinear per input."""

    def __init__(self, d1, d2, d_out, c):
        super().__init__()
        self.d1, self.d2, self.d_out, self.c = d1, d2, d_out, c
        self.l1, self.l2 = (HypLinear(d, d_out, c, bias=False) for d in (d1, d2))

    def forward(self, x1, x2, c=None):
        return pmath.mobius_add(self.l1(x1), self.l2(x2), c=_curvature(self, c))

    def extra_repr(self):
        return f'dims {self.d1} and {self.d2} ---> dim {self.d_out}'


class HyperbolicDistanceLayer(nn.Module):
    """Row-wise geodesic distance, [rows, 1]."""

    def __init__(self, c):
        super().__init__()
        self.c = c

    def forward(self, x1, x2, c=None):
        return pmath.dist(x1, x2, c=_curvature(self, c), keepdim=True)

    def extra_repr(self):
        return f'c={self.c}'


class _BasePointMap(nn.Module):
    """What ToPoincare and FromPoincare share: a curvature (a number, a tensor, or an ``nn.Parameter``, which is trained) and, with
    ``train_x``, a trainable base point kept as the tangent vector ``xp`` at the origin (zero at the start, so the map starts as the one
    at the origin).  ``xp`` is registered before ``c``, the reference's order."""

    def __init__(self, c, train_c, train_x, ball_dim):
        super().__init__()
        if train_c:
            raise NotImplementedError('train_c=True is not supported: hand the trainable curvature in as c=nn.Parameter(torch.tensor([c0], '
                                      'device=...)) instead; it is registered under the name c, as the reference\'s train_c=True does')
        if train_x and ball_dim is None:
            raise ValueError('train_x=True needs ball_dim, the length of the trainable base point xp')
        self.register_parameter('xp', nn.Parameter(torch.zeros(ball_dim)) if train_x else None)
        self.c, self.train_x = c, train_x

    def base_point(self):
        return pmath.project(pmath.expmap0(self.xp, c=self.c), c=self.c)


class ToPoincare(_BasePointMap):
    """Euclidean features -> points of the ball (exponential map at the origin or at the trainable base point), optionally after
    clipping the features to norm ``clip_r`` (https://arxiv.org/pdf/2107.11472.pdf).  With ``riemannian`` the gradient that flows
    back is rescaled to the Riemannian one; as in the reference, constructing the module sets ``pmath.RiemannianGradient.c``, a
    class attribute shared by every instance."""

    def __init__(self, c, train_c=False, train_x=False, ball_dim=None, riemannian=True, clip_r=None):
        super().__init__(c, train_c, train_x, ball_dim)
        self.clip_r = clip_r
        self.riemannian = pmath.RiemannianGradient
        # the reference's float class attribute: the value c has NOW (a tensor's is read once, here; RiemannianGradient keeps a number)
        self.riemannian.c = float(c.detach()) if isinstance(c, torch.Tensor) else c
        self._rescale_grad = bool(riemannian)

    def grad_fix(self, y):
        return self.riemannian.apply(y) if self._rescale_grad else y

    def forward(self, x):
        if self.clip_r is not None:
            x = pmath.feature_clip(x, self.clip_r)
        y = pmath.expmap(self.base_point(), x, c=self.c) if self.train_x else pmath.expmap0(x, c=self.c)
        return self.grad_fix(pmath.project(y, c=self.c))

    def extra_repr(self):
        return f'c={self.c}, train_x={self.train_x}'


class FromPoincare(_BasePointMap):
    """Points of the ball -> Euclidean space: the logarithmic map at the origin or at the trainable base point."""

    def __init__(self, c, train_c=False, train_x=False, ball_dim=None):
        super().__init__(c, train_c, train_x, ball_dim)
        self.train_c = isinstance(c, nn.Parameter)

    def forward(self, x):
        return pmath.logmap(self.base_point(), x, c=self.c) if self.train_x else pmath.logmap0(x, c=self.c)

    def extra_repr(self):
        return f'train_c={self.train_c}, train_x={self.train_x}'
