"""Gromov delta on the MI355X: warmed, event-timed, repeated sttode_amd.delta.batched_deltas at n in {1500, 4096},
d = 128, 10 tries in one launch, on the symmetric path (what batched_delta_hyp takes for Euclidean distances) and on the general path
(the same distances with symmetric = 0), plus the distance launch alone.  The issue bound of the delta kernel is its (i, j, k) triples at
1.5 vector instructions per triple (one v_min_f32 per triple, a v_max3_f32 per two) over 256 CUs x 64 lanes x the shader clock read during
the run -- a bound on instruction issue, not a measured peak.  The reference formula's NumPy cost (float64, n x n x n array) at n = 400 on
this host is the comparison line.  Kernel times: run under `rocprofv3 --kernel-trace --stats` with --once.

    python profiles/delta/measure.py [--out FILE] [--reps R] [--once]
"""
import argparse
import json
import os
import re
import subprocess
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from sttode_amd import delta  # noqa: E402

CUS, LANES, IPT = 256, 64, 1.5


def sclk_mhz():
    """Current shader clock from rocm-smi (a read-only query); None if it cannot be read."""
    try:
        out = subprocess.run(['rocm-smi', '--showclocks'], capture_output=True, text=True, timeout=30).stdout
    except Exception:
        return None, ''
    m = re.findall(r'sclk.*?\((\d+)Mhz\)', out)
    return (float(m[0]) if m else None), out.strip()


def ref_numpy(D):
    row, col = D[0, :][None, :], D[:, 0][:, None]
    A = 0.5 * (row + col - D)
    return np.max(np.max(np.minimum(A[:, :, None], A[None, :, :]), axis=1) - A)


def time_ms(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out = []
    for _ in range(reps):
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--once', action='store_true', help='one warmed call per configuration (for a kernel trace)')
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    T, d = 10, 128
    res = {'T': T, 'd': d, 'instr_per_triple': IPT, 'cus': CUS, 'lanes_per_cu_clock': LANES, 'rows': {}}
    clocks = []
    for n in (1500, 4096):
        rng = np.random.default_rng(n)
        X = torch.from_numpy(rng.standard_normal((20000, d)).astype(np.float32)).to(dev)
        idx = torch.from_numpy(rng.integers(0, 20000, (T, n)).astype(np.int32)).to(dev)
        dist, diam = delta._dist(X, idx, T, n)
        ws = delta._workspace(T, n, dev)
        outd = torch.empty(T, dtype=torch.float32, device=dev)
        from sttode_amd import capi

        def hyp(sym):
            capi.call('sttode_delta_hyp', dist, T, n, dist.numel(), sym, ws, ws.numel(), outd, capi.stream_ptr())

        def dst():
            capi.call('sttode_delta_dist', X, X.shape[0], d, idx, T, n, dist, dist.numel(), diam, capi.stream_ptr())

        for f in (lambda: hyp(1), lambda: hyp(0), dst):
            f()
        torch.cuda.synchronize()
        hyp(1)
        s1 = outd.clone()
        hyp(0)
        assert torch.equal(s1, outd), 'symmetric and general paths differ'
        if a.once:
            for f in (lambda: hyp(1), lambda: hyp(0), dst):
                f()
            torch.cuda.synchronize()
            continue
        row = {}
        for name, fn, triples in (('symmetric', lambda: hyp(1), T * n ** 3 / 2), ('general', lambda: hyp(0), T * n ** 3),
                                  ('distances', dst, None)):
            ms = time_ms(fn, a.reps)
            clk, _ = sclk_mhz()
            clocks.append(clk)
            r = {'ms_median': float(np.median(ms)), 'ms_min': float(np.min(ms)), 'ms_max': float(np.max(ms)), 'reps': a.reps, 'sclk_mhz': clk}
            if triples is not None:
                f = (clk or 2400.0) * 1e6
                bound_ms = triples * IPT / (CUS * LANES * f) * 1e3
                r.update(triples=triples, issue_bound_ms=bound_ms, issue_bound_fraction=bound_ms / r['ms_median'],
                         clock_source='rocm-smi' if clk else 'nominal 2400 MHz (clock not readable)')
            row[name] = r
        res['rows'][str(n)] = row
        print(n, json.dumps(row), flush=True)
        del dist, X
        torch.cuda.empty_cache()
    if a.once:
        print('once: done')
        return
    # the reference formula in NumPy (float64, the n x n x n array), n = 400, on this host
    rng = np.random.default_rng(400)
    Xh = rng.standard_normal((400, d))
    Dh = np.sqrt(((Xh[:, None] - Xh[None]) ** 2).sum(-1))
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        ref_numpy(Dh)
        ts.append(time.perf_counter() - t0)
    res['numpy_reference_n400_s'] = float(min(ts))
    res['numpy_threads'] = os.environ.get('OMP_NUM_THREADS')
    res['sclk_raw'] = sclk_mhz()[1]
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, 'w').write(txt + '\n')


if __name__ == '__main__':
    main()
