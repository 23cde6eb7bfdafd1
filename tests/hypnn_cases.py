"""The cases of tests/golden/hypnn.npz (written by tests/golden/make_hypnn_golden.py) in one place, shared by the generator, test_hypnn.py
(CPU: the fixture checks itself, the module surface) and test_hypnn_gpu.py (the kernels and modules against the float64 yardstick).

Every gradient case <case> stores  <case>.in.<k> (inputs), <case>.p.<name> (module parameters), <case>.g (upstream gradient) and, for every
input and parameter, <case>.gin.<k>64 / 32d and <case>.gp.<name>64 / 32d: the reference differentiated in float64 on the float32 inputs (the
yardstick, stored rounded to float32) and the reference's own float32 run, stored as its difference from the yardstick.  g is float16.
Every mod.* case also stores the reference module's forward value the same way: <case>.out64 / out32d.
"""
import numpy as np

from pmath_vjp_cases import BOUND, err  # noqa: F401  (the project's bound and metric)

SHAPES = ((1, 1, 1, 1.0), (9, 5, 16, 1.0), (3, 67, 65, 0.5), (70, 3, 130, 1.0), (2, 3, 300, 1.0))   # (B, C, d, c)
CLIP_R = 2.3
CLIPS = ('clipped', 'unclipped', 'mixed')


def shape_tag(B, C, d, c):
    return 'B%dC%dd%dc%s' % (B, C, d, c)


# name -> constructor, called with the module namespace (hyptorch.nn or sttode_amd.hypnn).  Parameter values and inputs come from the fixture.
MODULES = {
    'hyplinear': lambda nn: nn.HypLinear(16, 8, c=0.5),
    'hyplinear_nobias': lambda nn: nn.HypLinear(65, 7, c=1.0, bias=False),
    'concat': lambda nn: nn.ConcatPoincareLayer(16, 5, 8, c=1.0),
    'distlayer': lambda nn: nn.HyperbolicDistanceLayer(c=0.5),
    'topoincare': lambda nn: nn.ToPoincare(c=1.0, clip_r=CLIP_R),
    'topoincare_euclidean_grad': lambda nn: nn.ToPoincare(c=1.0, riemannian=False),
    'topoincare_train_x': lambda nn: nn.ToPoincare(c=1.0, train_x=True, ball_dim=16),
    'frompoincare': lambda nn: nn.FromPoincare(c=1.0),
    'frompoincare_train_x': lambda nn: nn.FromPoincare(c=1.0, train_x=True, ball_dim=16),
}
MODULES.update({'mlr.' + shape_tag(B, C, d, c): (lambda nn, C=C, d=d, c=c: nn.HyperbolicMLR(d, C, c=c)) for B, C, d, c in SHAPES})

# the modules whose state_dict names, shapes and initial values under torch.manual_seed(0) are stored: init.<name>.names, init.<name>.<param>
INIT_MODULES = {
    'HyperbolicMLR': lambda nn: nn.HyperbolicMLR(8, 5, c=1.0),
    'HypLinear': lambda nn: nn.HypLinear(16, 8, c=1.0),
    'HypLinear.nobias': lambda nn: nn.HypLinear(16, 8, c=1.0, bias=False),
    'ConcatPoincareLayer': lambda nn: nn.ConcatPoincareLayer(16, 5, 8, c=0.5),
    'HyperbolicDistanceLayer': lambda nn: nn.HyperbolicDistanceLayer(c=1.0),
    'ToPoincare': lambda nn: nn.ToPoincare(c=1.0),
    'ToPoincare.train_x': lambda nn: nn.ToPoincare(c=1.0, train_x=True, ball_dim=16),
    'FromPoincare': lambda nn: nn.FromPoincare(c=1.0),
    'FromPoincare.train_x': lambda nn: nn.FromPoincare(c=1.0, train_x=True, ball_dim=16),
}

TRAIN_STEPS, TRAIN_ROWS, TRAIN_LR = 5, 32, 1e-2


def train_model(nn):
    """ToPoincare(c=1, clip_r=2.3) -> HypLinear(16, 8) -> HyperbolicMLR(8, 5)."""
    import torch
    return torch.nn.Sequential(nn.ToPoincare(c=1.0, clip_r=CLIP_R), nn.HypLinear(16, 8, c=1.0), nn.HyperbolicMLR(8, 5, c=1.0))


def function_cases():
    """[(case name, op, c)] of the raw functions: op in 'hsoftmax' (inputs X, A, P), 'mobius_addition_batch' (x, y), 'clip' (x)."""
    out = []
    for s in SHAPES:
        out.append(('hs.' + shape_tag(*s), 'hsoftmax', s[3]))
        out.append(('mab.' + shape_tag(*s), 'mobius_addition_batch', s[3]))
    return out + [('clip.' + k, 'clip', None) for k in CLIPS]


def case_arrays(z, case):
    """(inputs [arrays in call order], params {name: array}, g) of a stored case."""
    ins = []
    while '%s.in.%d' % (case, len(ins)) in z:
        ins.append(z['%s.in.%d' % (case, len(ins))])
    pre = case + '.p.'
    return ins, {k[len(pre):]: z[k] for k in z if k.startswith(pre)}, z[case + '.g'].astype(np.float32)


def case_forward(z, case):
    """(float64 yardstick, reference fp32) of the forward value of a stored mod.* case."""
    return z[case + '.out64'], z[case + '.out64'] + z[case + '.out32d']


def case_grads(z, case):
    """[(key, float64 yardstick, reference fp32)] of a stored case; key is 'gin.<k>' or 'gp.<name>'."""
    pre = case + '.g'
    return [(k[len(case) + 1:-2], z[k], z[k] + z[k[:-2] + '32d']) for k in sorted(z) if k.startswith(pre + 'in.') or k.startswith(pre + 'p.') if k.endswith('64')]
