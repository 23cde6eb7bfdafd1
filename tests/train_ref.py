"""Plain restatements of the training-step kernels of csrc/train*.hip, for tests/test_train_kernels_*.py.

Each reference runs in the dtype of its inputs: float64 is the rounding-free yardstick, float32 is torch's own fp32 evaluation of the same
operation (how far a correct fp32 implementation may sit from float64).  Layouts are the kernels' (training.py block_fwd / block_bwd).
The element-wise ops are a float64 NumPy restatement of the comments of the ``EW_*`` enum.
"""
import numpy as np
import torch
import torch.nn.functional as F

HID = 96            # GRU hidden size of the decoder blocks (model/STTODE.py:68)


def gru_seq(gi, Whh, bhh, dh_last):
    """Unrolled torch GRU (gate order r | z | n) over gi [m, Tp, 288] = W_ih x_t + b_ih, h_{-1} = 0, and autograd of <dh_last, h_T>.
    -> dict H [Tp+1, m, 96] (H[0] = 0), tapes [Tp, m, 384] = r | z | n | gh_n, dgi [m, Tp, 288], dgh [Tp, m, 288] (gradient with respect to
    W_hh h + b_hh of each step)."""
    gi = gi.detach().clone().requires_grad_(True)
    Whh = Whh.detach().clone().requires_grad_(True)             # (so that every step's gh, the first one included, has a gradient)
    m, Tp = gi.shape[0], gi.shape[1]
    h = torch.zeros(m, HID, dtype=gi.dtype)
    H, tapes, ghs = [h], [], []
    for t in range(Tp):
        gh = h @ Whh.T + bhh
        gh.retain_grad()
        ghs.append(gh)
        g = gi[:, t]
        r = torch.sigmoid(g[:, :HID] + gh[:, :HID])
        z = torch.sigmoid(g[:, HID:2 * HID] + gh[:, HID:2 * HID])
        n = torch.tanh(g[:, 2 * HID:] + r * gh[:, 2 * HID:])
        h = (1 - z) * n + z * h
        H.append(h)
        tapes.append(torch.cat([r, z, n, gh[:, 2 * HID:]], 1))
    (h * dh_last).sum().backward()
    return dict(H=torch.stack(H).detach(), tapes=torch.stack(tapes).detach(), dgi=gi.grad.detach(),
                dgh=torch.stack([x.grad for x in ghs]).detach())


def gru_cell(gi, gh, hprev, dh):
    """One GRU cell: gi [m, 288], gh [m, 288], hprev [m, 96] or None (zeros).  -> hnew, tape [m, 384], dgi, dgh, dhprev (through h only:
    gh is held fixed, as sttode_gru_cell_bwd's dhprev = dh * z)."""
    gi = gi.detach().clone().requires_grad_(True)
    gh = gh.detach().clone().requires_grad_(True)
    hp = (torch.zeros(gi.shape[0], HID, dtype=gi.dtype) if hprev is None else hprev.detach().clone()).requires_grad_(True)
    r = torch.sigmoid(gi[:, :HID] + gh[:, :HID])
    z = torch.sigmoid(gi[:, HID:2 * HID] + gh[:, HID:2 * HID])
    n = torch.tanh(gi[:, 2 * HID:] + r * gh[:, 2 * HID:])
    h = (1 - z) * n + z * hp
    (h * dh).sum().backward()
    return dict(hnew=h.detach(), tape=torch.cat([r, z, n, gh[:, 2 * HID:]], 1).detach(), dgi=gi.grad, dgh=gh.grad, dhprev=hp.grad)


def conv(xa, adiv, xb, w, b, de):
    """conv1d(2 -> 32, k = 3, pad = 1) over x = xa[c / adiv] - xb[c] ([m, T, 2]), written out tap by tap.  de [m, T, 32] is the gradient of
    the pre-activation (already masked by the relu).  -> x, e = relu(conv) [m, T, 32], dx, dw [32, 2, 3], db [32] (the sums, without the
    accumulation into existing gradients)."""
    m, T = de.shape[0], de.shape[1]
    x = xa[torch.arange(m) // adiv] - (xb if xb is not None else 0)
    x = x.detach().clone().requires_grad_(True)
    w = w.detach().clone().requires_grad_(True)
    b = b.detach().clone().requires_grad_(True)
    xp = F.pad(x, (0, 0, 1, 1))                                   # [m, T + 2, 2]: taps t - 1, t, t + 1
    pre = b + sum(torch.einsum('mti,oi->mto', xp[:, k:k + T], w[:, :, k]) for k in range(3))
    (pre * de).sum().backward()
    return dict(x=x.detach(), e=torch.relu(pre).detach(), dx=x.grad, dw=w.grad, db=b.grad)


def add_ln(x, r, gamma, beta, dy, eps=1e-5):
    """LayerNorm(x + r) over the last dimension, written out.  -> y, xhat, rstd [rows], dsum (gradient with respect to x + r), dgamma,
    dbeta (the sums, without the accumulation)."""
    s = (x + (r if r is not None else 0)).detach().clone().requires_grad_(True)
    gamma = gamma.detach().clone().requires_grad_(True)
    beta = beta.detach().clone().requires_grad_(True)
    mu = s.mean(-1, keepdim=True)
    rstd = 1 / torch.sqrt(((s - mu) ** 2).mean(-1, keepdim=True) + eps)
    xhat = (s - mu) * rstd
    y = xhat * gamma + beta
    (y * dy).sum().backward()
    return dict(y=y.detach(), xhat=xhat.detach(), rstd=rstd[:, 0].detach(), dsum=s.grad, dgamma=gamma.grad, dbeta=beta.grad)


ACTS = {0: lambda v: v, 1: torch.relu, 2: torch.tanh, 3: torch.sigmoid}


def tlinear_tab(X, W, bias, tab, tdiv, act):
    """Y[c] = act(W X[c] + tab[c / tdiv] (+ bias))."""
    v = X @ W.T + tab[torch.arange(X.shape[0]) // tdiv]
    if bias is not None:
        v = v + bias
    return ACTS[act](v)


# ---- element-wise ops (sttode_train_ewise) ---------------------------------------------------------------------------------------------
EW_OPS = dict(MUL=0, AXPY=1, GATE_BWD=2, EULER_FWD=3, EULER_BWD=4, RSAMPLE=5, RELU_BWD=6, FILL=7, RSAMPLE_BWD=8, CUR_ADD=9, TANH_BWD=10,
              LATENT_BWD=11, SUM_CUR=12, EULER_BWD_CAT=13, SCALE_ADD=14, AXPY_ROWS=15)


def ewise(op, p, count, i0, f0):
    """float64 restatement of one sttode_train_ewise(op, p0..p4, count, i0, f0) call.  ``p``: list of five arrays (or None), flat.
    -> {index of the written buffer: (value, scale)} with the buffers as they are after the call (float64) and, per element, the largest
    magnitude among the terms that enter it (the yardstick of the element's rounding error)."""
    q = [None if a is None else np.asarray(a, np.float64).ravel().copy() for a in p]
    i = np.arange(count)
    out = {}

    def put(k, idx, val, *terms):
        if k not in out:
            out[k] = (q[k].copy(), np.zeros_like(q[k]))
        out[k][0][idx] = val
        out[k][1][idx] = np.max(np.abs(np.stack(np.broadcast_arrays(val, *terms))), axis=0)

    p0, p1, p2, p3, p4 = q
    if op == 0:
        put(0, i, p1[i] * p2[i])
    elif op == 1:
        put(0, i, p0[i] + f0 * p1[i], p0[i], f0 * p1[i])
    elif op == 2:
        d, t, s = p0[i], p1[i], p2[i]
        put(3, i, d * s * (1 - t * t), d * s, d * s * t * t)
        put(4, i, d * t * s * (1 - s), d * t * s, d * t * s * s)
    elif op == 3:
        put(0, i, np.maximum(p1[i] + f0 * p2[i], 0), p1[i], f0 * p2[i])
    elif op == 4:
        d = np.where(p1[i] > 0, p0[i], 0)
        put(3, i, p3[i] + d, p3[i], d)
        put(4, i, f0 * d)
    elif op == 5:
        r, c = i // i0, i % i0
        mu, lv = p1[r * 2 * i0 + c], p1[r * 2 * i0 + i0 + c]
        put(0, i, mu + p2[i] * np.exp(lv / 2), mu, p2[i] * np.exp(lv / 2))
    elif op == 6:
        put(0, i, np.where(p2[i] > 0, p1[i], 0))
    elif op == 7:
        put(0, i, np.full(count, f0))
    elif op == 8:
        r, c = i // i0, i % i0
        a, b = r * 2 * i0 + c, r * 2 * i0 + i0 + c
        inc = p0[i] * p2[i] * 0.5 * np.exp(0.5 * p1[b])
        put(3, a, p3[a] + p0[i], p3[a], p0[i])
        out[3][0][b] = p3[b] + inc
        out[3][1][b] = np.maximum(np.abs(p3[b]), np.abs(inc))
        out[3][1][b] = np.maximum(out[3][1][b], np.abs(out[3][0][b]))
    elif op == 9:
        add = p1[(i // i0) // int(f0) * 2 + (i % i0) % 2]
        put(0, i, p0[i] + add, p0[i], add)
    elif op == 10:
        put(0, i, p1[i] * (1 - p2[i] * p2[i]), p1[i], p1[i] * p2[i] * p2[i])
    elif op == 11:
        mode, nz = i0 & 3, i0 >> 2
        e = np.zeros(count) if mode == 0 else (p3[i % nz] if mode == 1 else p3[(i // int(f0)) * nz + i % nz])
        a = p2[i]
        t1, t2 = p0[i] * e, p1[i] * 2 * a / (a * a + 1e-8)
        put(4, i, t1 + t2, t1, t2)
    elif op == 12:
        v, terms = p1[i] + p2[i], [p1[i], p2[i]]
        if p3 is not None:
            add = p3[(i // i0) // int(f0) * 2 + (i % i0) % 2]
            v, terms = v + add, terms + [add]
        put(0, i, v, *terms)
    elif op == 13:
        D, ld = (i0 >> 16) or 64, i0 & 0xffff
        r, c = i // D, i % D
        d = np.where(p1[i] > 0, p0[r * ld + D + c], 0)
        put(3, i, p0[r * ld + c] + d, p0[r * ld + c], d)
        put(4, i, f0 * d)
    elif op == 14:
        add = p1[i] if p1 is not None else 0
        put(0, i, f0 * p0[i] + add, f0 * p0[i], add)
    elif op == 15:
        width, ld = i0 & 0xffff, i0 >> 16
        t = f0 * p1[(i // width) * ld + i % width]
        put(0, i, p0[i] + t, p0[i], t)
    else:
        raise ValueError(op)
    return out


def ulps_f32(scale, n=4):
    """n fp32 units in the last place at magnitude ``scale`` (elementwise)."""
    return n * np.spacing(np.abs(np.asarray(scale, np.float64)).astype(np.float32)).astype(np.float64)


def assert_f64_close(got, f64, f32, what='', factor=4.0, rtol=1e-5, atol_rel=1e-6):
    """|got - f64| <= max(factor |f32 - f64|, atol + rtol |f64|) element by element; atol = atol_rel * max |f64| of the output.  ``f32``: torch's
    own fp32 evaluation of the same operation on the same inputs.  Returns the worst error in units of its bound."""
    got, f64, f32 = (np.asarray(v, np.float64) for v in (got, f64, f32))
    assert got.shape == f64.shape == f32.shape, (what, got.shape, f64.shape, f32.shape)
    assert np.isfinite(got).all(), f'{what}: {int((~np.isfinite(got)).sum())} non-finite elements'
    atol = atol_rel * (np.abs(f64).max() if f64.size else 0.0)
    bound = np.maximum(factor * np.abs(f32 - f64), atol + rtol * np.abs(f64))
    err = np.abs(got - f64)
    bad = err > bound
    worst = float((err / np.where(bound > 0, bound, np.inf)).max()) if err.size else 0.0
    if bad.any():
        k = np.unravel_index(np.argmax(np.where(bad, err / np.where(bound > 0, bound, 1e-300), -1)), err.shape)
        raise AssertionError(f'{what}: {int(bad.sum())} / {bad.size} elements out of bound, worst at {k}: got {got[k]:.9g}, f64 {f64[k]:.9g}, '
                             f'fp32 {f32[k]:.9g}, bound {bound[k]:.3e}')
    return worst
