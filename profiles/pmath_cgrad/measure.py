#!/usr/bin/env python3
"""For the record (no speed claim): the row backward (mobius_add, dist) at 8192 x 64 with a float c and with a tensor c,
and the float form of the PARENT commit's library on the same box, in alternating runs.

    python profiles/pmath_cgrad/measure.py --parent /path/to/parent/libsttode_hip.so [--out profiles/pmath_cgrad/rates.txt]

The parent library is built from the parent commit (`make -C sttode_amd/csrc` in a checkout of it).  Each run is LAUNCHES back-to-back
launches between two events; the variants alternate inside every one of RUNS rounds, so drift of the box hits all of them alike.  Written:
the median microseconds per launch of each variant, its run-to-run spread (max - min) / median, and the float form's ratio to the parent's.
The float form must be within the spread of the parent's: it runs an instantiation without the partial for c and without the gc_ws store.
"""
import argparse
import ctypes
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from sttode_amd import capi  # noqa: E402

ROWS, D, RUNS, LAUNCHES, WARMUP = 8192, 64, 15, 200, 20
OPS = {'mobius_add': 2, 'dist': 3}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent', required=True)
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.abspath(__file__)), 'rates.txt'))
    a = ap.parse_args()
    new, old = capi.lib(), ctypes.CDLL(a.parent)
    sig = capi.SIGNATURES['sttode_pmath_rowop_bwd']
    old.sttode_pmath_rowop_bwd.argtypes, old.sttode_pmath_rowop_bwd.restype = sig, ctypes.c_int
    dev = torch.device('cuda:0')
    g = torch.Generator(device='cpu').manual_seed(1)
    pts = lambda: (torch.nn.functional.normalize(torch.randn(ROWS, D, generator=g), dim=-1) * (0.05 + 0.85 * torch.rand(ROWS, 1, generator=g))).to(dev)
    x, y, gv, gs = pts(), pts(), torch.randn(ROWS, D, generator=g).to(dev), torch.randn(ROWS, generator=g).to(dev)
    gx, gy = torch.empty_like(x), torch.empty_like(y)
    c = torch.ones(1, device=dev)
    ws, gc = torch.empty(ROWS, dtype=torch.float64, device=dev), torch.empty(1, device=dev)
    st = capi.stream_ptr()
    P = lambda t: t.data_ptr()
    lines = ['row backward at %d x %d, microseconds per launch: median of %d runs of %d launches, spread = (max - min) / median'
             % (ROWS, D, RUNS, LAUNCHES), 'device: ' + torch.cuda.get_device_name(0)]
    for name, op in OPS.items():
        up = gs if name == 'dist' else gv
        variants = {
            'parent float c': lambda: old.sttode_pmath_rowop_bwd(op, P(x), P(y), P(up), P(gx), P(gy), ROWS, D, 1.0, st),
            'float c': lambda: new.sttode_pmath_rowop_bwd(op, P(x), P(y), P(up), P(gx), P(gy), ROWS, D, 1.0, st),
            'tensor c (gx, gy, gc)': lambda: new.sttode_pmath_rowop_bwd_c(op, P(x), P(y), P(up), P(gx), P(gy), ROWS, D, P(c), P(ws), P(gc), st),
            'tensor c (gc alone)': lambda: new.sttode_pmath_rowop_bwd_c(op, P(x), P(y), P(up), None, None, ROWS, D, P(c), P(ws), P(gc), st),
        }
        times = {k: [] for k in variants}
        for k, f in variants.items():
            for _ in range(WARMUP):
                assert f() == 0, k
        torch.cuda.synchronize()
        for _ in range(RUNS):
            for k, f in variants.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(LAUNCHES):
                    f()
                e1.record()
                e1.synchronize()
                times[k].append(e0.elapsed_time(e1) * 1e3 / LAUNCHES)
        med = {k: statistics.median(v) for k, v in times.items()}
        lines.append(name + ':')
        for k, v in times.items():
            lines.append('  %-24s %8.2f us   spread %.1f%%' % (k, med[k], 100.0 * (max(v) - min(v)) / med[k]))
        lines.append('  float c / parent float c = %.3f' % (med['float c'] / med['parent float c']))
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    with open(a.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
