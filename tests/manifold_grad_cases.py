"""The cases of tests/golden/manifold_grad.npz (written by tests/golden/make_manifold_grad_golden.py) and the yardsticks that need no
fixture, shared by test_manifold_grad.py (CPU) and test_manifold_grad_gpu.py.

Stored (the reference's own functions, differentiated by torch autograd in float64 on float32 inputs -- `*64` -- and once in float32 --
`*32`): poincare_mean, Oblique proj / proj_tan / expmap / dist / ptransp / retr_transp (under the loops of riemannian_ref.py, as
riemannian_ops.npz is), Oblique.inner as the matrix it is.  The Oblique row cases take their INPUTS from riemannian_ops.npz
(`op.obl.d<d>.in`: p, y, u, w), so only upstream gradients and results are stored here.

Not stored: the ball's egrad2rgrad / inner / ptransp / retr are not in the reference; their yardstick is riemannian_ref.py (pinned to the
reference's values by test_riemannian.py), differentiated by CPU autograd in float64 at test time (ball_case / ball_yardstick below).
"""
import numpy as np
import torch

import riemannian_ref as rr

SEED = 20270131
CS = (1.0, 0.5)
MEAN_R, MEAN_W, MEAN_D = (1, 2, 9), (1, 5), (1, 2, 16, 65, 130)
MEAN_RANK4 = (2, 3, 2, 16)                      # dim 1: outer 2, R 3, inner 2
MEAN_SPECIAL = (2, 5, 16)                       # in this shape: rows x[:, 1] are x, -x (Klein mean 0 over dim 0); x[0, 3] is a zero row
OBL_DIST = ((1, 1, 1, 2), (1, 9, 5, 16), (2, 3, 7, 65), (1, 2, 3, 300))     # (nb, n1, n2, d)
OBL_DIST_SPECIAL = (1, 9, 5, 16)                # in this case: p2[0, 0] == p1[0, 0] and p2[0, 1] == -p1[0, 1] (both clamped)
OBL_OPS = ('proj', 'proj_tan', 'expmap', 'ptransp', 'retr_transp')
# op -> (operand names among p, y, u, w, in the order their gradients are stored)
OBL_OPERANDS = dict(proj=('w',), proj_tan=('u', 'p'), expmap=('u', 'p'), ptransp=('p', 'y', 'w'), retr_transp=('p', 'u', 'w'))
EDGE_ZERO_ROW = 4                               # obl.edge: op.obl.d16's inputs with u[4] = 0 (expmap's proj(p + u) branch)


def mean_cases():
    """(name, shape, dim, c) of every poincare_mean case; the two dims of a shape and c share one input (mean_input_key)."""
    out = []
    for c in CS:
        for R in MEAN_R:
            for W in MEAN_W:
                for d in MEAN_D:
                    for dim in (0, 1):
                        out.append(('mean.R%d.W%d.d%d.c%s.dim%d' % (R, W, d, c, dim), (R, W, d), dim, c))
        out.append(('mean.r4.c%s.dim1' % c, MEAN_RANK4, 1, c))
    return out


def mean_input_key(name):
    return name.rsplit('.dim', 1)[0] + '.x'


MEAN_KINDS = ('x', 'g', 'out64', 'out32', 'gx64', 'gx32', 'gc64', 'gc32')


class MeanFixture:
    """The poincare_mean cases of manifold_grad.npz: every kind of array is stored once, flat, the cases one after the other."""

    def __init__(self, fx):
        self.case = {}
        pos, xs = {k: 0 for k in MEAN_KINDS}, {}

        def cut(kind, shape):
            n = int(np.prod(shape))
            a = fx['mean.' + kind][pos[kind]:pos[kind] + n].reshape(shape)
            pos[kind] += n
            return a
        for name, shape, dim, c in mean_cases():
            key = mean_input_key(name)
            if key not in xs:
                xs[key] = cut('x', shape)
            red = shape[:dim] + shape[dim + 1:]
            rec = dict(x=xs[key], g=cut('g', red))
            for tag in ('64', '32'):
                rec['out' + tag], rec['gx' + tag], rec['gc' + tag] = cut('out' + tag, red), cut('gx' + tag, shape), cut('gc' + tag, (1,))
            self.case[name] = rec
        assert all(pos[k] == fx['mean.' + k].size for k in MEAN_KINDS)

    def __getitem__(self, name):
        return self.case[name]


def pmean(x, dim, c):
    """poincare_mean (hyptorch/pmath.py:472-479) restated over the closed forms the kernels use: lambda xk = 2 x / q, lambda = (1 + c |x|^2) / q,
    q = 1 - c |x|^2.  dtype-generic; c a number or a tensor."""
    x2 = (x * x).sum(-1, keepdim=True)
    q = 1 - c * x2
    m = (2 * x / q).sum(dim) / ((1 + c * x2) / q).sum(dim)
    return m / (1 + torch.sqrt(1 - c * (m * m).sum(-1, keepdim=True)))


def obl_cases():
    """(stored name, input key of riemannian_ops.npz, d) of the Oblique row cases."""
    return [('obl.d%d' % d, 'op.obl.d%d.in' % d, d) for d in rr.DIMS if d > 1]


class TakenOblique(rr.ObliqueRef):
    """ObliqueRef whose expmap evaluates, per row, only the branch it takes.  The reference's torch.where evaluates both, and its autograd
    then gives NaN at u = 0 (a zero cotangent divided by |u| = 0 in the branch that was not taken); the values are the same.  A row with
    u == 0 is proj(p + u) -- the reference's own `retr` line (oblique.py:25) -- every other row must have |u| > 1e-4."""

    def expmap(self, u, p):
        u, p = torch.broadcast_tensors(u, p)
        n = u.detach().norm(dim=-1)
        zero = n == 0
        assert bool(((n > 1e-4) | zero).all())
        if not bool(zero.any()):
            return super().expmap(u, p)
        out = []
        for i in range(u.shape[0]):
            out.append(self.proj(p[i] + u[i]) if bool(zero[i]) else super().expmap(u[i:i + 1], p[i:i + 1])[0])
        return torch.stack(out)


def obl_run(man, op, p, y, u, w):
    """The result(s) of an Oblique op as a tuple, and the operands in OBL_OPERANDS order."""
    t = dict(p=p, y=y, u=u, w=w)
    res = {'proj': lambda: (man.proj(w),),      # (w: a row of norm 0.1 .. 2, off the sphere)
           'proj_tan': lambda: (man.proj_tan(u, p),), 'expmap': lambda: (man.expmap(u, p),),
           'ptransp': lambda: (man.ptransp(p, y, w),), 'retr_transp': lambda: man.retr_transp(p, u, w)}[op]()
    return res, [t[k] for k in OBL_OPERANDS[op]]


def vjp(fn, arrays, gs, dt):
    """Gradients of sum_k <g_k, out_k> of fn(*tensors) -> (tuple of results, list of operands) by torch autograd in dtype dt: float32 arrays
    (None where an operand got no gradient: stored as zeros)."""
    ts = [torch.from_numpy(np.ascontiguousarray(a)).to(dt).requires_grad_() for a in arrays]
    outs, operands = fn(*ts)
    loss = sum((o * torch.from_numpy(np.ascontiguousarray(g)).to(dt).reshape(o.shape)).sum() for o, g in zip(outs, gs))
    grads = torch.autograd.grad(loss, operands, allow_unused=True)
    return [o.detach().to(torch.float32).numpy() for o in outs], \
        [(torch.zeros_like(t) if g is None else g).to(torch.float32).numpy() for g, t in zip(grads, operands)]


# ---- the ball: inputs and yardstick at test time -----------------------------------------------------------------------------------------
BALL_OPS = ('egrad2rgrad', 'inner', 'ptransp', 'retr', 'retr_transp')
BALL_OPERANDS = dict(egrad2rgrad=('p', 'u'), inner=('p', 'u', 'w'), ptransp=('p', 'y', 'w'), retr=('p', 'u'), retr_transp=('p', 'u', 'w'))


def ball_run(man, op, p, y, u, w):
    t = dict(p=p, y=y, u=u, w=w)
    res = {'egrad2rgrad': lambda: (man.egrad2rgrad(p, u),), 'inner': lambda: (man.inner(p, u, w),), 'ptransp': lambda: (man.ptransp(p, y, w),),
           'retr': lambda: (man.retr(p, u),), 'retr_transp': lambda: man.retr_transp(p, u, w)}[op]()
    return res, [t[k] for k in BALL_OPERANDS[op]]


def ball_clip_case(c, d=16, rows=9):
    """Inputs (p, y, u, w) [4, rows, d] on the ball of curvature -c whose retraction is clipped by project in the odd rows and not in the
    even ones: p at sqrt(c) |p| = 0.9, u along p with a geodesic length of 8 (odd rows: expmap lands at 1 - 2e-7 of the radius, past the
    clip radius 1 - 1e-3) or 0.5 (even rows).  Asserted in float64: no |retr| within 1e-4 (relative) of the clip radius."""
    rng = np.random.default_rng(SEED + int(c * 100) + d)
    v = rng.standard_normal((4, rows, d))
    v /= np.linalg.norm(v, axis=-1, keepdims=True)
    p = v[0] * 0.9 / np.sqrt(c)
    y = v[1] * rng.uniform(0.05, 0.9, (rows, 1)) / np.sqrt(c)
    room = 1 - c * (p ** 2).sum(-1, keepdims=True)
    length = np.where(np.arange(rows)[:, None] % 2 == 1, 8.0, 0.5)           # geodesic length = lambda_p |u| = 2 |u| / room
    u = (0.9 * v[0] + 0.1 * v[2]) * length * room / 2 / np.sqrt(c)
    w = v[3] * 0.3 * room / np.sqrt(c)
    ins = np.stack([p, y, u, w]).astype(np.float32)
    man = rr.BallRef(c)
    with torch.no_grad():
        e = man.expmap(torch.from_numpy(ins[2]).double(), torch.from_numpy(ins[0]).double())
    rel = e.norm(dim=-1).numpy() * np.sqrt(c) / (1 - 1e-3)
    assert (np.abs(rel - 1) > 1e-4).all() and (rel[1::2] > 1).all() and (rel[0::2] < 1).all(), rel
    return ins


def upstream(tag, shape):
    """The upstream gradient of a test-time case: N(0, 1) from a seed fixed by the tag."""
    seed = SEED + sum((i + 1) * ord(ch) for i, ch in enumerate(tag))
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)
