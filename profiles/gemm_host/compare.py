"""One SHA-256 per output buffer of a fixed, seeded list of calls into the training GEMM entry points (sttode_tlinear, sttode_tlinear_tab,
sttode_twgrad, sttode_tlinear_bwd), at least one call per branch of their host code: every launch form, either side of each column
threshold, alone, inside an open sttode_tgemm_group, and (the LDS-tiled backward calls) between sttode_twgrad_defer(1, buf) .. (0).
usage: [STTODE_HIP_LIB=<library built from the parent commit>] python profiles/gemm_host/compare.py > hashes_<which>.txt
Run once per library on the same Python tree; the two files must be identical."""
import hashlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..'))
from sttode_amd import capi  # noqa: E402

DEV = torch.device('cuda:0')


class Run:
    """The call list; every phase draws the same inputs (the generator is re-seeded), so a call's hashes can be read across phases too."""

    def __init__(self):
        self.st = capi.stream_ptr()
        self.scratch = torch.zeros(1 << 20, device=DEV)
        self.small = torch.zeros(1000, device=DEV)            # smaller than one gradient of any twgrad case below
        self.out = []                                         # (label, buffer) in issue order
        self.keep = []                                        # inputs stay alive until the phase has been synchronized

    def begin(self, phase):
        self.phase, self.rng = phase, np.random.default_rng(2024)

    def t(self, *shape, scale=1.0):
        x = torch.from_numpy((scale * self.rng.standard_normal(shape)).astype(np.float32)).to(DEV)
        self.keep.append(x)
        return x

    def done(self, label, *bufs):
        for i, b in enumerate(bufs):
            self.out.append((f'{self.phase} | {label} | {i}', b))

    def flush(self):
        torch.cuda.synchronize()
        for label, b in self.out:
            print(hashlib.sha256(b.cpu().numpy().tobytes()).hexdigest(), label)
        self.out, self.keep = [], []

    # out[c] = act(W X[c / xdiv] + b); xpad / ypad: extra floats per row of X / Y (0 and 4 keep 16-byte rows: the vector and fast forms)
    def tlinear(self, cols, J, I, xdiv=1, act=2, xpad=5, ypad=3):
        rows = (cols + xdiv - 1) // xdiv
        X, W, b = self.t(rows, J + xpad)[:, :J], self.t(I, J, scale=J ** -0.5), self.t(I)
        Y = torch.full((cols, I + ypad), 7.0, device=DEV)
        capi.call('sttode_tlinear', X, X.stride(0), xdiv, W, J, 0, b, None, 0, Y, Y.stride(0), cols, J, I, act, 0, self.st)
        self.done(f'tlinear {cols}x{J}->{I} xdiv {xdiv} act {act} pads {xpad} {ypad}', Y)

    # dX[c] = mask(dY[c] W + dX[c]): trans = 1, mask, accumulate
    def tlinear_trans(self, cols, N, K):
        dY, W, mask, dX = self.t(cols, N), self.t(N, K, scale=N ** -0.5), self.t(cols, K), self.t(cols, K)
        capi.call('sttode_tlinear', dY, N, 1, W, K, 1, None, mask, K, dX, K, cols, N, K, 0, 1, self.st)
        self.done(f'tlinear trans {cols}x{N}->{K} mask accumulate', dX)

    def tlinear_tab(self, cols, J, I, tdiv, aligned, with_b, act):       # as tests/test_train_kernels_gpu.py _tab_run
        groups = (cols + tdiv - 1) // tdiv
        X, W, b = self.t(cols, J + 3)[:, :J], self.t(I, J, scale=J ** -0.5), self.t(I, scale=0.5)
        ldt = ((I + 1 + 3) // 4) * 4 if aligned else I + 3
        tabb = self.t(groups, ldt)
        tab = tabb[:, :I] if aligned else tabb[:, 1:I + 1]
        Y = torch.full((cols, (I + 7) // 4 * 4), 12345.0, device=DEV)
        capi.call('sttode_tlinear_tab', X, X.stride(0), W, J, b if with_b else None, tab, ldt, tdiv, Y, Y.stride(0), cols, J, I, act, self.st)
        self.done(f'tlinear_tab {cols}x{J}->{I} tdiv {tdiv}', Y)

    def twgrad(self, cols, N, K, xdiv=1, scratch='big', dest=None):
        rows = (cols + xdiv - 1) // xdiv
        dY, X = self.t(cols, N), self.t(rows, K + 5)[:, :K]
        dW, db = dest if dest is not None else (self.t(N, K), self.t(N))
        sc = {'big': self.scratch, 'none': None, 'small': self.small}[scratch]
        assert scratch != 'small' or sc.numel() < N * (K + 1)
        capi.call('sttode_twgrad', dY, N, X, X.stride(0), xdiv, dW, K, db, cols, N, K, sc, 0 if sc is None else sc.numel(), self.st)
        self.done(f'twgrad {cols}x{N}x{K} xdiv {xdiv} scratch {scratch}', dW, db)
        return dW, db

    def tlinear_bwd(self, cols, N, K, Kdx, xdiv=1, mask=True, accumulate=1, dest=None):
        rows = (cols + xdiv - 1) // xdiv
        dY, W, X = self.t(cols, N), self.t(N, K, scale=N ** -0.5), self.t(rows, K)
        m, dX = (self.t(cols, Kdx) if mask else None), self.t(cols, Kdx)
        dW, db = dest if dest is not None else (self.t(N, K), self.t(N))
        capi.call('sttode_tlinear_bwd', dY, N, W, K, m, Kdx if mask else 0, dX, Kdx, Kdx, accumulate, X, K, xdiv, dW, K, db, cols, N, K,
                  self.scratch, self.scratch.numel(), self.st)
        self.done(f'tlinear_bwd {cols}x{N}x{K} Kdx {Kdx} xdiv {xdiv}', dX, dW, db)
        return dW, db

    def everything(self):
        for cols, J, I in ((37, 67, 64), (33, 200, 24), (19, 1024, 64)):        # latency form: ksplit 1, 2, 4
            self.tlinear(cols, J, I)
        self.tlinear(1100, 67, 70)                                              # medium form
        self.tlinear(1536, 256, 8192, act=1)                                    # throughput form: 24 x 128 tiles >= TLIN_MEDIUM_BELOW
        self.tlinear(5000, 96, 288, act=3, xpad=0, ypad=4)                      # LDS-tiled, fast loads, vector epilogue
        self.tlinear(2049, 131, 33, xdiv=3, act=3)                              # LDS-tiled, generic loads
        self.tlinear_trans(601, 72, 100)                                        # either side of TGEMM_MIN_COLS_BWD
        self.tlinear_trans(600, 72, 100)
        self.tlinear_tab(17, 128, 70, 7, False, False, 1)                       # latency form
        self.tlinear_tab(2049, 128, 512, 21, False, True, 1)                    # LDS-tiled
        for cols in (37, 600, 601, 3001):
            self.twgrad(cols, 24, 67)
        self.twgrad(2049, 24, 67, xdiv=3)
        for cols in (601, 3001):
            self.twgrad(cols, 24, 67, scratch='none')
            self.twgrad(cols, 24, 67, scratch='small')
        self.tlinear_bwd(37, 64, 100, 100)
        self.tlinear_bwd(640, 20, 67, 67, mask=False, accumulate=0)
        self.tlinear_bwd(1024, 64, 100, 60)                                     # Kdx < K
        self.tlinear_bwd(1100, 64, 100, 100, xdiv=3)                            # broadcast rows: the two stand-alone entry points
        self.tlinear_bwd(2500, 64, 100, 64)
        self.tlinear_bwd(7392, 128, 256, 256)

    def deferred(self, grouped):
        """The LDS-tiled backward calls with their reductions deferred into a buffer that holds about two of them (early flushes), the
        same destination twice (another early flush); grouped: inside a group within the bracket, as a training step's backward pass."""
        buf = torch.zeros(150000, device=DEV)
        self.keep.append(buf)
        capi.call('sttode_twgrad_defer', 1, buf, buf.numel())
        try:
            if grouped:
                capi.call('sttode_tgemm_group', 1)
            dest = self.tlinear_bwd(2500, 64, 100, 64)
            self.tlinear_bwd(7392, 128, 256, 256)
            self.twgrad(3001, 24, 67)
            self.twgrad(601, 24, 67)
            self.tlinear_bwd(2500, 64, 100, 64, dest=dest)
            self.twgrad(2049, 24, 67, xdiv=3)
        finally:
            if grouped:
                capi.call('sttode_tgemm_group', 0)
            capi.call('sttode_twgrad_defer', 0, None, 0)


def main():
    r = Run()
    r.begin('alone')
    r.everything()
    r.flush()
    r.begin('group')
    capi.call('sttode_tgemm_group', 1)
    try:
        r.everything()
    finally:
        capi.call('sttode_tgemm_group', 0)
    r.flush()
    for grouped in (False, True):
        r.begin('deferred in a group' if grouped else 'deferred')
        r.deferred(grouped)
        r.flush()


if __name__ == '__main__':
    main()
