"""The cases of tests/golden/pmath_vjp.npz and pmath_vjp_rows.npz (written by tests/golden/make_pmath_vjp_golden.py) as one list, shared by
test_pmath_grad.py (CPU: the fixture checks itself), test_pmath_grad_gpu.py (the backward kernels against the float64 yardstick) and
test_pmath_forward_gpu.py (the forward values at the same inputs against the oracle in float64)."""
import numpy as np

BOUND = 1e-4          # the bound of the project's golden comparisons, on max |got - ref| / (1 + |ref|)
ROW_OPS = ('project', 'lambda_x', 'mobius_add', 'dist', 'dist0', 'expmap', 'expmap0', 'logmap', 'logmap0', 'p2k', 'k2p', 'lorenz')
SCALAR_OPS = ('lambda_x', 'dist', 'dist0', 'lorenz')
TWO_OPS = ('mobius_add', 'dist', 'expmap', 'logmap')
DIMS, ROWS, CS = (1, 2, 16, 65, 130), (1, 9), (1.0, 0.5)
ROW_SHAPES = [(d, n, c) for d in DIMS for n in ROWS for c in CS]     # the whole product: 20 shapes for each of the 12 ops
MATVEC = ('d16O16', 'd5O33', 'd64O7', 'big', 'zero')
DIST_MATRIX = ((1, 1, 2), (5, 9, 16), (67, 3, 65), (3, 2, 300))   # the last: rows longer than the 256 elements a wave keeps in registers


def err(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float(np.max(np.abs(got - ref) / (1.0 + np.abs(ref))))


MATVEC_C = {'d5O33': 0.5}      # every other case outside the row-op product that does not carry c in its name: c = 1.0
LOGMAP0_ZERO_ROW = ('zero.logmap0', 4)   # the one row whose REFERENCE fp32 gradient is outside the bound (see cases())


def cases(z, zr):
    """The cases of pmath_vjp.npz (z) and pmath_vjp_rows.npz (zr), compositions excluded:
    [{name, op, c, inputs [arrays, in call order], g, grads [(name, float64 yardstick, reference fp32), one per input], zero_row}].
    op: a row op, 'mobius_matvec' or 'dist_matrix'."""
    out = []

    def add(name, op, c, inputs, g, stems, zero_row=None):
        out.append(dict(name=name, op=op, c=c, inputs=inputs, g=g, zero_row=zero_row,
                        grads=[(name + '.' + s, z[name + '.' + s + '64'], z[name + '.' + s + '32']) for s in stems]))
    for d, n, c in ROW_SHAPES:
        sh = 'd%d.n%d.c%s' % (d, n, c)
        (x, y, u, g), gs, grads = zr['in.' + sh], zr['gs.' + sh], zr['grads.' + sh]
        k = 0
        for op in ROW_OPS:
            ins = [x * np.float32(0.5)] if op == 'k2p' else [x]
            if op in TWO_OPS:
                ins.append(u if op == 'expmap' else y)
            name = 'row.%s.%s' % (op, sh)
            out.append(dict(name=name, op=op, c=c, inputs=ins, g=gs if op in SCALAR_OPS else g, zero_row=None,
                            grads=[(name + '.' + s, grads[k + 2 * i], grads[k + 2 * i + 1]) for i, s in enumerate(('gx', 'gy')[:len(ins)])]))
            k += 2 * len(ins)
        assert k == len(grads) == 32
    for c in CS:
        name = 'clip.project.c%s' % c
        add(name, 'project', c, [z[name + '.x']], z[name + '.g'], ('gx',))
    for op in ('expmap0', 'logmap0'):
        add('zero.' + op, op, 1.0, [z['zero.%s.x' % op]], z['zero.%s.g' % op], ('gx',))
    add('zero.expmap', 'expmap', 1.0, [z['zero.expmap.x'], z['zero.expmap.y']], z['zero.expmap.g'], ('gx', 'gy'))
    for op in ('mobius_add', 'dist'):
        name = 'bcast.' + op
        add(name, op, 1.0, [z[name + '.x'], z[name + '.y']], z[name + '.g'], ('gx', 'gy'))
    for tag in MATVEC:
        name = 'mv.' + tag
        add(name, 'mobius_matvec', MATVEC_C.get(tag, 1.0), [z[name + '.m'], z[name + '.x']], z[name + '.g'], ('gm', 'gx'),
            zero_row=int(z[name + '.row']) if tag == 'zero' else None)
    for P, R, d in DIST_MATRIX:
        name = 'dm.P%dR%dd%d' % (P, R, d)
        add(name, 'dist_matrix', 1.0, [z[name + '.x'], z[name + '.y']], z[name + '.g'], ('gx', 'gy'))
    return out


COMPOSITIONS = {'comp.topoincare': ('x',), 'comp.hyplinear': ('w', 'b', 'x'), 'comp.distlayer': ('x', 'y')}   # name -> inputs (gradient: 'g' + input)
