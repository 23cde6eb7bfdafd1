#!/usr/bin/env python3
"""One-off: the sixteen pmath entry points that come in a float-c and a device-c form, this tree's library against the
PARENT commit's on the same inputs, bit for bit.

    python profiles/pmath_curv/compare.py --parent /path/to/parent/libsttode_hip.so [--out profiles/pmath_curv/bits.txt]

The parent library is built from the parent commit (`make -C sttode_amd/csrc` in a checkout of it).  Inputs: every case of
tests/golden/pmath_vjp.npz, pmath_vjp_rows.npz and pmath_cgrad.npz (the edge rows 255 .. 1030 x 5, dm.P67R3d65 and pair.B67C3d65 among
them); the mean's backward runs on the 1030 x 5 edge rows as [2, 5, 103, 5] and on pair.B67C3d65's X as [1, 67, 1, 65].  Each entry runs
in every form of its optional buffers, both libraries write into NaN-prefilled buffers, and every output must be torch.equal as bit
patterns (so that a NaN both wrote, or both left, compares equal and one that only one wrote does not)."""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from sttode_amd import capi  # noqa: E402
from sttode_amd.pmath import _OPS  # noqa: E402
from pmath_cgrad_cases import SCALAR_OPS, cases  # noqa: E402

ENTRIES = ['sttode_pmath_' + p + s for p in ('rowop', 'matvec', 'pair', 'rowop_bwd', 'matvec_bwd', 'dist_matrix_bwd', 'hsoftmax_bwd', 'mean_bwd')
           for s in ('', '_c')]
DEV = torch.device('cuda:0')


def nans(*shape, dtype=torch.float32):
    return torch.full(shape, float('nan'), dtype=dtype, device=DEV)


class Both:
    """Runs an entry of both libraries on the same arguments; `outs` names the positions of the output buffers, which are allocated
    NaN-prefilled per library from the shapes given in their place."""

    def __init__(self, new, old):
        self.libs, self.calls, self.outputs, self.bad, self.seen = (new, old), 0, 0, [], set()

    def __call__(self, what, name, *args):
        res = []
        for L in self.libs:
            bufs = [nans(*a[1:], dtype=a[0]) if isinstance(a, tuple) else a for a in args]
            conv = [a.data_ptr() if isinstance(a, torch.Tensor) else a for a in bufs]
            rc = getattr(L, name)(*conv, capi.stream_ptr())
            assert rc == 0, (what, name, L.sttode_last_error())
            torch.cuda.synchronize()
            res.append([b for a, b in zip(args, bufs) if isinstance(a, tuple)])
        self.calls += 1
        self.seen.add(name)
        for i, (a, b) in enumerate(zip(*res)):
            self.outputs += 1
            iv = torch.int64 if a.dtype == torch.float64 else torch.int32
            if not torch.equal(a.view(iv), b.view(iv)):
                self.bad.append('%s %s output %d' % (what, name, i))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent', required=True)
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.abspath(__file__)), 'bits.txt'))
    a = ap.parse_args()
    new, old = capi.lib(), ctypes.CDLL(a.parent)
    old.sttode_last_error.restype = ctypes.c_char_p
    for n in ENTRIES:
        getattr(old, n).argtypes, getattr(old, n).restype = capi.SIGNATURES[n], ctypes.c_int
    both = Both(new, old)
    gold = lambda n: np.load(os.path.join(ROOT, 'tests', 'golden', n + '.npz'))
    zc = gold('pmath_cgrad')
    cs = cases(zc, gold('pmath_vjp'), gold('pmath_vjp_rows'))
    f32, f64 = torch.float32, torch.float64
    T = lambda v: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(DEV)
    P = 'sttode_pmath_'
    for case in cs:
        name, op, c = case['name'], case['op'], float(case['c'])
        cd = torch.full((1,), c, device=DEV)
        ins, g = [T(v) for v in case['inputs']], T(case['g'])
        if op in _OPS:
            x, y = (ins + [None])[:2]
            if y is not None:
                x, y = (t.contiguous() for t in torch.broadcast_tensors(x, y))
            d = x.shape[-1]
            rows = x.numel() // d
            o = (f32, rows) if op in SCALAR_OPS else (f32, rows, d)
            gy = (f32, rows, d) if y is not None else None
            both(name, P + 'rowop', _OPS[op], x, y, o, None, rows, d, c)
            both(name, P + 'rowop_c', _OPS[op], x, y, o, None, rows, d, cd)
            both(name, P + 'rowop_bwd', _OPS[op], x, y, g, (f32, rows, d), gy, rows, d, c)
            both(name, P + 'rowop_bwd_c', _OPS[op], x, y, g, (f32, rows, d), gy, rows, d, cd, (f64, rows), (f32, 1))
            both(name + ' (gc alone)', P + 'rowop_bwd_c', _OPS[op], x, y, g, None, None, rows, d, cd, (f64, rows), (f32, 1))
        elif op == 'mobius_matvec':
            m, x = ins
            (O, d), rows = m.shape, x.numel() // m.shape[1]
            ws, gx, gm, gc = (f32, rows, O), (f32, rows, d), (f32, O, d), ((f64, rows), (f32, 1))
            both(name, P + 'matvec', m, x, ws, (f32, rows), ws, rows, d, O, c)
            both(name, P + 'matvec_c', m, x, ws, (f32, rows), ws, rows, d, O, cd)
            both(name, P + 'matvec_bwd', m, x, g, ws, ws, (f32, rows), gx, gm, rows, d, O, c)
            both(name, P + 'matvec_bwd_c', m, x, g, ws, ws, (f32, rows), gx, gm, rows, d, O, cd, *gc)
            both(name + ' (gx)', P + 'matvec_bwd_c', m, x, g, ws, ws, None, gx, None, rows, d, O, cd, *gc)
            both(name + ' (gm)', P + 'matvec_bwd_c', m, x, g, ws, ws, None, None, gm, rows, d, O, cd, *gc)
            both(name + ' (gc alone)', P + 'matvec_bwd_c', m, x, g, ws, None, None, None, None, rows, d, O, cd, *gc)
        elif op in ('dist_matrix', '_mobius_addition_batch'):
            x, y = ins
            (Pn, d), R = x.shape, y.shape[0]
            which, o = (0, (f32, Pn, R)) if op == 'dist_matrix' else (1, (f32, Pn, R, d))
            both(name, P + 'pair', which, x, y, None, o, Pn, R, d, c)
            both(name, P + 'pair_c', which, x, y, None, o, Pn, R, d, cd)
            if which == 0:
                gx, gy, gc = (f32, Pn, d), (f32, R, d), ((f64, Pn), (f32, 1))
                both(name, P + 'dist_matrix_bwd', x, y, g, gx, gy, Pn, R, d, c)
                both(name, P + 'dist_matrix_bwd_c', x, y, g, gx, gy, Pn, R, d, cd, *gc)
                both(name + ' (gx)', P + 'dist_matrix_bwd_c', x, y, g, gx, None, Pn, R, d, cd, *gc)
                both(name + ' (gy)', P + 'dist_matrix_bwd_c', x, y, g, None, gy, Pn, R, d, cd, *gc)
                both(name + ' (gc alone)', P + 'dist_matrix_bwd_c', x, y, g, None, None, Pn, R, d, cd, *gc)
        else:
            assert op == '_hyperbolic_softmax', op
            X, A, Pt = ins
            (B, d), C = X.shape, Pt.shape[0]
            gX, gA, gc = (f32, B, d), (f32, C, d), ((f64, B), (f32, 1))
            both(name, P + 'pair', 2, Pt, X, A, (f32, B, C), C, B, d, c)
            both(name, P + 'pair_c', 2, Pt, X, A, (f32, B, C), C, B, d, cd)
            both(name, P + 'hsoftmax_bwd', X, A, Pt, g, (f64, 6, B, C), gX, gA, gA, B, C, d, c)
            both(name, P + 'hsoftmax_bwd_c', X, A, Pt, g, (f64, 7, B, C), gX, gA, gA, B, C, d, cd, *gc)
            both(name + ' (gX)', P + 'hsoftmax_bwd_c', X, A, Pt, g, (f64, 7, B, C), gX, None, None, B, C, d, cd, *gc)
            both(name + ' (gA, gP)', P + 'hsoftmax_bwd_c', X, A, Pt, g, (f64, 7, B, C), None, gA, gA, B, C, d, cd, *gc)
            both(name + ' (gc alone)', P + 'hsoftmax_bwd_c', X, A, Pt, g, (f64, 7, B, C), None, None, None, B, C, d, cd, *gc)
    xe, _, ge = (T(v) for v in zc['edge.in'])
    Xp, Ap = T(zc['pair.B67C3d65.X']), T(zc['pair.B67C3d65.A'])
    for name, x, g, (outer, R, inner, d), c in (('mean.edge[2,5,103,5]', xe, ge[:206], (2, 5, 103, 5), 2.0),
                                                ('mean.pair.B67C3d65.X[1,67,1,65]', Xp, Ap[:1], (1, 67, 1, 65), float(np.float32(0.7)))):
        cd = torch.full((1,), c, device=DEV)
        groups = outer * inner
        gS, gL, gx, gc = (f64, groups * d), (f64, groups), (f32, groups * R, d), ((f64, groups * R + groups), (f32, 1))
        both(name, P + 'mean_bwd', x, g.contiguous(), gS, gL, gx, outer, R, inner, d, c)
        both(name, P + 'mean_bwd_c', x, g.contiguous(), gS, gL, gx, outer, R, inner, d, cd, *gc)
        both(name + ' (gc alone)', P + 'mean_bwd_c', x, g.contiguous(), gS, gL, None, outer, R, inner, d, cd, *gc)
    assert both.seen == set(ENTRIES), sorted(set(ENTRIES) - both.seen)
    need = ('edge.mobius_add.n1030', 'edge.dist.n1030', 'dm.P67R3d65', 'hs.B67C3d65', 'mab.B67C3d65')
    assert all(n in {k['name'] for k in cs} for n in need)
    lines = ['this tree\'s libsttode_hip.so against the parent commit\'s, device: ' + torch.cuda.get_device_name(0),
             '%d cases of the three fixtures + 2 mean shapes, %d calls of the 16 entries per library, %d output buffers (NaN-prefilled) compared as bit patterns'
             % (len(cs), both.calls, both.outputs),
             'cases include: ' + ', '.join(need),
             'outputs that differ: %d' % len(both.bad)] + both.bad
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    with open(a.out, 'w') as f:
        f.write(text)
    return 1 if both.bad else 0


if __name__ == '__main__':
    sys.exit(main())
