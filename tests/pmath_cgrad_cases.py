"""The cases of tests/golden/pmath_cgrad.npz (written by tests/golden/make_pmath_cgrad_golden.py): the gradient of the curvature c through
the Poincare-ball operations and the hyperbolic layers.  Shared by test_pmath_cgrad.py (CPU: the fixture checks itself) and
test_pmath_cgrad_gpu.py.  Inputs and upstream gradients of the row-op, clip / zero / bcast, mobius_matvec and dist_matrix cases are the
arrays of pmath_vjp_rows.npz and pmath_vjp.npz (pmath_vjp_cases.cases); pmath_cgrad.npz adds only their c gradients, and the inputs of
the cases that are new here.  Every `gc` array is [2]: the float64 yardstick, then the reference's own float32 run."""
import numpy as np

from pmath_vjp_cases import BOUND, ROW_OPS, ROW_SHAPES, SCALAR_OPS, cases as vjp_cases, err  # noqa: F401  (re-exported)

EDGE_ROWS = (255, 256, 257, 1030)      # around the finishing kernel's 256 threads, and several strided rounds
EDGE_D, EDGE_C, EDGE_OPS = 5, 2.0, ('mobius_add', 'dist')
PAIR_SHAPES = ((1, 1, 2), (9, 7, 16), (67, 3, 65))     # (B, C, d) of _hyperbolic_softmax and _mobius_addition_batch
PAIR_C = float(np.float32(0.7))
MODULE_C = float(np.float32(0.7))
# name -> (parameters besides c, in state-dict order; inputs)
MODULES = {
    'mod.to': ((), ('x',)),
    'mod.to_xp_clip': (('xp',), ('x',)),
    'mod.from': ((), ('x',)),
    'mod.from_xp': (('xp',), ('x',)),
    'mod.net': (('w', 'b', 'a', 'p'), ('x',)),
}
CLIP_R = 2.3


def cases(zc, z, zr):
    """[{name, op, c, inputs, g, gc64, gc32}] for everything but the modules.  op: a row op, 'mobius_matvec', 'dist_matrix',
    '_hyperbolic_softmax' or '_mobius_addition_batch'."""
    out = []
    rows = zc['row.gc']
    k = {(op, sh): (i, j) for i, op in enumerate(ROW_OPS) for j, sh in enumerate(ROW_SHAPES)}
    for case in vjp_cases(z, zr):
        if case['name'].startswith('row.'):
            op, sh = case['op'], tuple(s for s in ROW_SHAPES if case['name'] == 'row.%s.d%d.n%d.c%s' % ((case['op'],) + s))[0]
            i, j = k[(op, sh)]
            gc = rows[:, i, j]
        else:
            gc = zc[case['name'] + '.gc']
        out.append(dict(name=case['name'], op=case['op'], c=case['c'], inputs=case['inputs'], g=case['g'], gc64=float(gc[0]), gc32=float(gc[1])))
    x, y, g = zc['edge.in']
    for n in EDGE_ROWS:
        for op in EDGE_OPS:
            name = 'edge.%s.n%d' % (op, n)
            gc = zc[name + '.gc']
            out.append(dict(name=name, op=op, c=EDGE_C, inputs=[x[:n], y[:n]], g=zc['edge.gs'][:n] if op in SCALAR_OPS else g[:n],
                            gc64=float(gc[0]), gc32=float(gc[1])))
    for B, C, d in PAIR_SHAPES:
        sh = 'B%dC%dd%d' % (B, C, d)
        X, A, P = (zc['pair.%s.%s' % (sh, n)] for n in 'XAP')
        for name, op, ins, g in (('hs.' + sh, '_hyperbolic_softmax', [X, A, P], zc['pair.%s.g' % sh]),
                                 ('mab.' + sh, '_mobius_addition_batch', [X, P], zc['pair.%s.g3' % sh])):
            gc = zc[name + '.gc']
            out.append(dict(name=name, op=op, c=PAIR_C, inputs=ins, g=g, gc64=float(gc[0]), gc32=float(gc[1])))
    return out
