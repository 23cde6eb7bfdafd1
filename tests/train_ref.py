"""Plain restatements of the training-step kernels of csrc/train*.hip and of the stage-2 sampler kernels of csrc/sampler.hip, for
tests/test_train_kernels_*.py and tests/test_train_loss_kernels_gpu.py.

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


# ---- the objective of forward() (sttode_loss_objective and the three stand-alone loss entry points) ------------------------------------
def kl_rows(qzp):
    """Per row of qzp [n, 2 zd] = (mu | logvar): sum over zd of KL(N(mu, sigma) || N(0, 1)) in the two-distribution form of
    utils/dist.py:26-29 with p.sigma = 1 (term = x / (p.sigma + 1e-8))."""
    zd = qzp.shape[1] // 2
    mu, lv = qzp[:, :zd], qzp[:, zd:]
    ps = 1.0 + 1e-8
    t1, t2 = mu / ps, torch.exp(0.5 * lv) / ps
    return (0.5 * (t1 * t1 + t2 * t2) - 0.5 - torch.log(t2)).sum(1)


def scene_of(scene_ptr, n):
    """agent -> scene index of a CSR [S + 1] (the kernels' agent_scene)."""
    ptr = np.asarray(scene_ptr, np.int64)
    assert ptr[0] == 0 and ptr[-1] == n and (np.diff(ptr) > 0).all()
    return np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))


def scene_kl(qzp, scene_ptr, kl_denom):
    """The UNCLAMPED KL value of every scene (model/STTODE.py:378-382 before its clamp_min): the sum over all rows / kl_denom
    without a CSR, else per scene the sum over its rows / its agents."""
    klr = kl_rows(qzp)
    if scene_ptr is None:
        return (klr.sum() / kl_denom).reshape(1)
    ptr = [int(v) for v in scene_ptr]
    return torch.stack([klr[a:b].sum() / (b - a) for a, b in zip(ptr[:-1], ptr[1:])])


def objective(pred, rec, fut, past, qzp, scene_ptr, K1, scale_mse, scale_rec, kl_denom, min_clip):
    """The four terms of model/STTODE.py:372-395 for ONE decoder pass over K1 = 1 + K samples per agent, written out, and torch autograd of
    their sum.  pred [n, K1, D], rec [n, K1, Dp], fut [n, D], past [n, Dp], qzp [n, 2 zd]; scene_ptr None (one scene: KL sum / kl_denom,
    best-of-K mean over the n agents) or a CSR [S + 1] (KL: sum over scenes of clamp_min(scene sum / scene agents); best-of-K: sum over
    scenes of the per-scene means).  -> dict mse, rec, kl, diverse, total (0-d), dpred, drec, dqzp, best [n] (1..K: first minimum) and
    d2 [n, K] (the summed squared distances the minimum is taken over)."""
    n = pred.shape[0]
    assert pred.shape[1] == rec.shape[1] == K1
    P, Rc, Q = (v.detach().clone().requires_grad_(True) for v in (pred, rec, qzp))
    mse = (fut - P[:, 0]).pow(2).sum() * scale_mse
    recover = (past - Rc[:, 0]).pow(2).sum() * scale_rec
    kl = scene_kl(Q, scene_ptr, kl_denom).clamp_min(min_clip).sum()
    d2 = (fut[:, None, :] - P[:, 1:]).pow(2).sum(-1)                 # [n, K]
    mn, idx = d2.min(dim=1)                                          # (first minimum; its gradient goes to that sample alone)
    if scene_ptr is None:
        diverse = mn.mean()
    else:
        ptr = [int(v) for v in scene_ptr]
        diverse = sum(mn[a:b].mean() for a, b in zip(ptr[:-1], ptr[1:]))
    total = ((mse + recover) + kl) + diverse
    total.backward()
    return dict(mse=mse.detach(), rec=recover.detach(), kl=kl.detach(), diverse=diverse.detach(), total=total.detach(), dpred=P.grad,
                drec=Rc.grad, dqzp=Q.grad, best=(idx + 1).to(torch.int32), d2=d2.detach())


def kl_term(qzp, scene_ptr, kl_denom, min_clip):
    """sttode_loss_kl alone: the KL value of ``objective`` and its gradient."""
    Q = qzp.detach().clone().requires_grad_(True)
    kl = scene_kl(Q, scene_ptr, kl_denom).clamp_min(min_clip).sum()
    kl.backward()
    return dict(kl=kl.detach(), dqzp=Q.grad)


def sqerr(pred, target, scale):
    """sttode_loss_sqerr: scale * sum (pred - target)^2 and its gradient."""
    p = pred.detach().clone().requires_grad_(True)
    v = (target - p).pow(2).sum() * scale
    v.backward()
    return dict(value=v.detach(), dpred=p.grad)


# ---- geodesic self-attention backward (sttode_mhgsa_attn_bwd) ---------------------------------------------------------------------------
ATTN_CLAMP = 1e-4


def geodesic_self_attention(qkv, dO, L, Nb, hd):
    """out_i = sum_j softmax_j(-acos(clamp(k^_i . q^_j, -1 + 1e-4, 1 - 1e-4))) v_j per (slot, head), scores untransposed
    (hyptransformerlib.py:261-265); token (l, slot) is row l Nb + slot of qkv [L Nb, 3 * 8 hd] = (q | k | v).  -> dict out [L Nb, 8 hd],
    dqkv (autograd of <dO, out>), dots [Nb, 8, L, L] (the unclamped k^_i . q^_j)."""
    DM = 8 * hd
    x = qkv.detach().clone().requires_grad_(True)
    q, k, v = (x[:, i * DM:(i + 1) * DM].view(L, Nb, 8, hd) for i in range(3))
    qn, kn = q / q.norm(dim=-1, keepdim=True), k / k.norm(dim=-1, keepdim=True)
    dots = torch.einsum('inhd,jnhd->nhij', kn, qn)                   # [slot, head, key row i, query column j]
    P = torch.softmax(-torch.acos(dots.clamp(-1 + ATTN_CLAMP, 1 - ATTN_CLAMP)), dim=-1)
    out = torch.einsum('nhij,jnhd->inhd', P, v).reshape(L * Nb, DM)
    out.backward(dO.to(out.dtype))
    return dict(out=out.detach(), dqkv=x.grad, dots=dots.detach())


# ---- stage-2 sampler (csrc/sampler.hip) -------------------------------------------------------------------------------------------------
def sampler_latent(A, b, eps, mode, K):
    """sampler.py:47-54: z = b (mode 0) or A eps + b with eps shared [nz] (1) or per agent [n, nz] (2); logvar = log(A^2 + 1e-8).
    A, b [n K, nz], row = agent K + k."""
    if mode == 0:
        z = b.clone()
    elif mode == 1:
        z = A * eps[None, :] + b
    else:
        z = A * eps.repeat_interleave(K, dim=0) + b
    return dict(z=z, logvar=torch.log(A * A + 1e-8))


def sampler_loss(mu, logvar, pmu, plogvar, motion, scale, g_kld, g_div):
    """samplerloss.py:4-20 per agent: kld[a] = sum over the agent's K nz latent entries of KL(N(mu, logvar) || N(pmu, plogvar))
    (utils/dist.py:26-29; pmu / plogvar None: the standard normal), div[a] = mean over the K (K - 1) / 2 sample pairs of
    exp(-F.pdist(motion[a]) ** 2 / scale); motion [n, K, D].  -> kld, div [n] and autograd of <g_kld, kld> + <g_div, div>: dmu, dlogvar,
    dmotion."""
    n, K = motion.shape[0], motion.shape[1]
    m, lv, mo = (v.detach().clone().requires_grad_(True) for v in (mu, logvar, motion))
    pm = 0.0 if pmu is None else pmu
    ps = (1.0 if plogvar is None else torch.exp(0.5 * plogvar)) + 1e-8
    t1, t2 = (m - pm) / ps, torch.exp(0.5 * lv) / ps
    kld = (0.5 * (t1 * t1 + t2 * t2) - 0.5 - torch.log(t2)).reshape(n, -1).sum(1)
    div = torch.stack([(-(F.pdist(mo[a], 2) ** 2) / scale).exp().mean() for a in range(n)])
    ((kld * g_kld).sum() + (div * g_div).sum()).backward()
    return dict(kld=kld.detach(), div=div.detach(), dmu=m.grad, dlogvar=lv.grad, dmotion=mo.grad)


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
