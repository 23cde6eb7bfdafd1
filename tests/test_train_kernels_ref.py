"""The float64 references of tests/train_ref.py (the yardsticks of tests/test_train_kernels_gpu.py and test_train_loss_kernels_gpu.py) pinned against torch's own modules in
float64 and against hand-worked element-wise cases.  No GPU needed."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import train_ref as R

D64 = torch.float64


def test_unrolled_gru_is_nn_gru():
    """gru_seq on gi = W_ih x + b_ih is nn.GRU (h_0 = 0): every hidden state, and through autograd of <dh, h_T> the gradients of x, W_hh and
    b_hh (dW_hh = sum_t dgh_t^T h_{t-1}, db_hh = sum_t dgh_t)."""
    torch.manual_seed(3)
    m, Tp, E = 5, 7, 32
    gru = torch.nn.GRU(E, R.HID, batch_first=True).double()
    x = torch.randn(m, Tp, E, dtype=D64, requires_grad=True)
    dh = torch.randn(m, R.HID, dtype=D64)
    out, hT = gru(x)
    (hT[0] * dh).sum().backward()
    with torch.no_grad():
        gi = x @ gru.weight_ih_l0.T + gru.bias_ih_l0
    ref = R.gru_seq(gi, gru.weight_hh_l0.detach(), gru.bias_hh_l0.detach(), dh)
    assert torch.equal(ref['H'][0], torch.zeros(m, R.HID, dtype=D64))
    torch.testing.assert_close(ref['H'][1:].transpose(0, 1), out.detach(), rtol=1e-12, atol=1e-13)
    torch.testing.assert_close(ref['dgi'] @ gru.weight_ih_l0.detach(), x.grad, rtol=1e-11, atol=1e-13)
    dgh = ref['dgh'].reshape(Tp * m, -1)
    hprev = ref['H'][:Tp].reshape(Tp * m, -1)
    torch.testing.assert_close(dgh.T @ hprev, gru.weight_hh_l0.grad, rtol=1e-11, atol=1e-13)
    torch.testing.assert_close(dgh.sum(0), gru.bias_hh_l0.grad, rtol=1e-11, atol=1e-13)
    torch.testing.assert_close(ref['dgi'].sum((0, 1)), gru.bias_ih_l0.grad, rtol=1e-11, atol=1e-13)
    # tapes: r | z | n | gh_n with h_t = (1 - z) n + z h_{t-1}
    r, z, n = ref['tapes'][..., :96], ref['tapes'][..., 96:192], ref['tapes'][..., 192:288]
    torch.testing.assert_close((1 - z) * n + z * ref['H'][:Tp], ref['H'][1:], rtol=1e-13, atol=1e-14)
    torch.testing.assert_close(ref['tapes'][..., 288:], ref['H'][:Tp] @ gru.weight_hh_l0.detach()[192:].T + gru.bias_hh_l0.detach()[192:])
    assert ((r > 0) & (r < 1)).all()


def test_gru_cell_is_one_step_of_nn_grucell():
    torch.manual_seed(4)
    m, E = 6, 16
    cell = torch.nn.GRUCell(E, R.HID).double()
    x = torch.randn(m, E, dtype=D64)
    h = torch.randn(m, R.HID, dtype=D64, requires_grad=True)
    dh = torch.randn(m, R.HID, dtype=D64)
    hn = cell(x, h)
    (hn * dh).sum().backward()
    with torch.no_grad():
        gi = x @ cell.weight_ih.T + cell.bias_ih
        gh = h @ cell.weight_hh.T + cell.bias_hh
    ref = R.gru_cell(gi, gh, h.detach(), dh)
    torch.testing.assert_close(ref['hnew'], hn.detach(), rtol=1e-13, atol=1e-14)
    torch.testing.assert_close(ref['dhprev'] + ref['dgh'] @ cell.weight_hh.detach(), h.grad, rtol=1e-12, atol=1e-13)
    torch.testing.assert_close(ref['dgi'].sum(0), cell.bias_ih.grad, rtol=1e-12, atol=1e-13)
    torch.testing.assert_close(ref['dgh'].sum(0), cell.bias_hh.grad, rtol=1e-12, atol=1e-13)
    z = ref['tape'][:, 96:192]
    torch.testing.assert_close(ref['dhprev'], dh * z)
    # hprev None means zeros
    r0 = R.gru_cell(gi, gh, None, dh)
    r1 = R.gru_cell(gi, gh, torch.zeros(m, R.HID, dtype=D64), dh)
    for k in ('hnew', 'tape', 'dgi', 'dgh', 'dhprev'):
        assert torch.equal(r0[k], r1[k]), k


@pytest.mark.parametrize('T', [1, 2, 9])
@pytest.mark.parametrize('adiv,with_xb', [(1, False), (3, True)])
def test_conv_is_nn_conv1d(T, adiv, with_xb):
    torch.manual_seed(5 + T)
    m = 6
    conv = torch.nn.Conv1d(2, 32, 3, padding=1).double()
    xa = torch.randn((m + adiv - 1) // adiv, T, 2, dtype=D64)
    xb = torch.randn(m, T, 2, dtype=D64) if with_xb else None
    x = (xa[torch.arange(m) // adiv] - (xb if with_xb else 0)).requires_grad_(True)
    pre = conv(x.transpose(1, 2)).transpose(1, 2)                    # [m, T, 32]
    de = torch.randn(m, T, 32, dtype=D64) * (pre > 0)                # masked by the relu, as the kernel receives it
    (pre * de).sum().backward()
    ref = R.conv(xa, adiv, xb, conv.weight.detach(), conv.bias.detach(), de)
    torch.testing.assert_close(ref['x'], x.detach())
    torch.testing.assert_close(ref['e'], torch.relu(pre).detach(), rtol=1e-13, atol=1e-14)
    torch.testing.assert_close(ref['dx'], x.grad, rtol=1e-13, atol=1e-14)
    torch.testing.assert_close(ref['dw'], conv.weight.grad, rtol=1e-13, atol=1e-14)
    torch.testing.assert_close(ref['db'], conv.bias.grad, rtol=1e-13, atol=1e-14)


@pytest.mark.parametrize('D', [32, 64, 128])
@pytest.mark.parametrize('with_r', [False, True])
def test_layernorm_is_f_layer_norm(D, with_r):
    torch.manual_seed(D + with_r)
    rows = 9
    x = torch.randn(rows, D, dtype=D64) * 3 + 1
    r = torch.randn(rows, D, dtype=D64) if with_r else None
    gamma, beta = torch.randn(D, dtype=D64, requires_grad=True), torch.randn(D, dtype=D64, requires_grad=True)
    s = (x + (r if with_r else 0)).requires_grad_(True)
    y = F.layer_norm(s, (D,), gamma, beta, eps=1e-5)
    dy = torch.randn(rows, D, dtype=D64)
    (y * dy).sum().backward()
    ref = R.add_ln(x, r, gamma.detach(), beta.detach(), dy)
    torch.testing.assert_close(ref['y'], y.detach(), rtol=1e-12, atol=1e-13)
    xh = F.layer_norm(s.detach(), (D,), eps=1e-5)
    torch.testing.assert_close(ref['xhat'], xh, rtol=1e-12, atol=1e-13)
    torch.testing.assert_close(ref['rstd'], 1 / torch.sqrt(s.detach().var(-1, unbiased=False) + 1e-5), rtol=1e-13, atol=0)
    torch.testing.assert_close(ref['dsum'], s.grad, rtol=1e-11, atol=1e-12)
    torch.testing.assert_close(ref['dgamma'], gamma.grad, rtol=1e-12, atol=1e-13)
    torch.testing.assert_close(ref['dbeta'], beta.grad, rtol=1e-12, atol=1e-13)


def test_tlinear_tab_is_linear_on_the_concatenated_input():
    """The table form is nn.Linear on cat(shared, own) with the shared part's product (+ bias) precomputed per group of tdiv columns."""
    torch.manual_seed(6)
    groups, tdiv, Js, J, I = 4, 3, 5, 7, 6
    lin = torch.nn.Linear(Js + J, I).double()
    shared = torch.randn(groups, Js, dtype=D64)
    own = torch.randn(groups * tdiv, J, dtype=D64)
    full = lin(torch.cat([shared[torch.arange(groups * tdiv) // tdiv], own], 1))
    with torch.no_grad():
        tab = shared @ lin.weight[:, :Js].T + lin.bias
        W = lin.weight[:, Js:]
    for act, f in ((0, lambda v: v), (1, torch.relu), (2, torch.tanh), (3, torch.sigmoid)):
        torch.testing.assert_close(R.tlinear_tab(own, W, None, tab, tdiv, act), f(full).detach(), rtol=1e-13, atol=1e-14)
    torch.testing.assert_close(R.tlinear_tab(own, W, lin.bias.detach(), tab - lin.bias.detach(), tdiv, 0), full.detach(), rtol=1e-13, atol=1e-14)


def _ew(op, p, count, i0=0, f0=0.0):
    return R.ewise(R.EW_OPS[op], p, count, i0, f0)


def test_ewise_restatements_on_worked_cases():
    """Hand-worked values of every op code (the comments of the EW_* enum of csrc/train_ewise.hip)."""
    a, b = np.array([1.0, -2.0, 3.0]), np.array([4.0, 5.0, -6.0])
    assert np.array_equal(_ew('MUL', [np.zeros(3), a, b, None, None], 3)[0][0], [4.0, -10.0, -18.0])
    assert np.array_equal(_ew('AXPY', [a, b, None, None, None], 3, f0=0.5)[0][0], [3.0, 0.5, 0.0])
    o = _ew('GATE_BWD', [np.array([2.0]), np.array([0.5]), np.array([0.25]), np.zeros(1), np.zeros(1)], 1)
    assert o[3][0][0] == 2 * 0.25 * 0.75 and o[4][0][0] == 2 * 0.5 * 0.25 * 0.75
    assert np.array_equal(_ew('EULER_FWD', [np.zeros(3), a, b, None, None], 3, f0=0.5)[0][0], [3.0, 0.5, 0.0])
    o = _ew('EULER_BWD', [a, np.array([1.0, 0.0, -1.0]), None, np.ones(3), np.zeros(3)], 3, f0=2.0)
    assert np.array_equal(o[3][0], [2.0, 1.0, 1.0]) and np.array_equal(o[4][0], [2.0, 0.0, 0.0])
    # rsample: params [rows, 2 i0] = (mu | logvar)
    prm = np.array([1.0, 2.0, 0.0, np.log(4.0)])                     # one row, i0 = 2: mu = (1, 2), logvar = (0, log 4)
    o = _ew('RSAMPLE', [np.zeros(2), prm, np.array([3.0, 5.0]), None, None], 2, i0=2)
    assert np.allclose(o[0][0], [1 + 3 * 1, 2 + 5 * 2], rtol=1e-15)
    o = _ew('RSAMPLE_BWD', [np.array([1.0, 2.0]), prm, np.array([3.0, 5.0]), np.ones(4), None], 2, i0=2)
    assert np.allclose(o[3][0], [2.0, 3.0, 1 + 1 * 3 * 0.5 * 1, 1 + 2 * 5 * 0.5 * 2], rtol=1e-15)
    assert np.array_equal(_ew('RELU_BWD', [np.zeros(3), a, b, None, None], 3)[0][0], [1.0, -2.0, 0.0])
    assert np.array_equal(_ew('FILL', [np.zeros(3), None, None, None, None], 3, f0=7.0)[0][0], [7.0] * 3)
    # cur_add / sum_cur: row length i0 = 4, K = 2 rows per agent, p1 / p3 [agents, 2]
    cur = np.array([10.0, 20.0, 30.0, 40.0])
    o = _ew('CUR_ADD', [np.zeros(16), cur, None, None, None], 16, i0=4, f0=2.0)
    assert np.array_equal(o[0][0].reshape(4, 4), [[10, 20, 10, 20]] * 2 + [[30, 40, 30, 40]] * 2)
    o = _ew('SUM_CUR', [np.zeros(16), np.ones(16), np.full(16, 2.0), cur, None], 16, i0=4, f0=2.0)
    assert np.array_equal(o[0][0].reshape(4, 4), np.array([[10, 20, 10, 20]] * 2 + [[30, 40, 30, 40]] * 2) + 3)
    o = _ew('SUM_CUR', [np.zeros(16), np.ones(16), np.full(16, 2.0), None, None], 16, i0=4, f0=2.0)
    assert np.array_equal(o[0][0], np.full(16, 3.0))
    assert np.array_equal(_ew('TANH_BWD', [np.zeros(2), np.array([2.0, 3.0]), np.array([0.5, -1.0]), None, None], 2)[0][0], [1.5, 0.0])
    # latent_bwd: dA = dz e + dlogvar 2 a / (a^2 + 1e-8); i0 = nz << 2 | mode, f0 = K nz
    dz, dlv, A = np.array([1.0, 2.0, 3.0, 4.0]), np.array([0.5, 0.5, 0.5, 0.5]), np.array([1.0, 2.0, -1.0, 0.5])
    lat = dlv * 2 * A / (A * A + 1e-8)
    e_sh, e_pa = np.array([3.0, 4.0]), np.array([3.0, 4.0, 5.0, 6.0])
    assert np.allclose(_ew('LATENT_BWD', [dz, dlv, A, e_sh, np.zeros(4)], 4, i0=(2 << 2) | 0, f0=2.0)[4][0], lat, rtol=1e-15)
    assert np.allclose(_ew('LATENT_BWD', [dz, dlv, A, e_sh, np.zeros(4)], 4, i0=(2 << 2) | 1, f0=2.0)[4][0], dz * [3, 4, 3, 4] + lat, rtol=1e-15)
    # mode 2, K = 1: agent i / (K nz) = i / 2
    assert np.allclose(_ew('LATENT_BWD', [dz, dlv, A, e_pa, np.zeros(4)], 4, i0=(2 << 2) | 2, f0=2.0)[4][0], dz * [3, 4, 5, 6] + lat, rtol=1e-15)
    # euler_bwd_cat: rows of p0 = cat(dx0 [D] | dode [D]) with leading dimension ld; D = 0 means 64
    for D, ld in ((2, 5), (0, 130)):
        Dv = D or 64
        p0 = np.arange(3 * ld, dtype=np.float64)
        out = np.array([1.0, -1.0] * (3 * Dv // 2))
        o = _ew('EULER_BWD_CAT', [p0, out, None, np.zeros(3 * Dv), np.zeros(3 * Dv)], 3 * Dv, i0=ld | (D << 16), f0=0.5)
        rows = p0.reshape(3, ld)
        d = np.where(out.reshape(3, Dv) > 0, rows[:, Dv:2 * Dv], 0)
        assert np.array_equal(o[3][0].reshape(3, Dv), rows[:, :Dv] + d) and np.array_equal(o[4][0].reshape(3, Dv), 0.5 * d)
    assert np.array_equal(_ew('SCALE_ADD', [a.copy(), b, None, None, None], 3, f0=2.0)[0][0], [6.0, 1.0, 0.0])
    assert np.array_equal(_ew('SCALE_ADD', [a.copy(), None, None, None, None], 3, f0=2.0)[0][0], [2.0, -4.0, 6.0])
    # axpy_rows: p0 [r, width] += f0 * p1[r * ld + c]; i0 = width | ld << 16
    src = np.arange(10, dtype=np.float64)                            # two rows of ld = 5
    o = _ew('AXPY_ROWS', [np.ones(6), src, None, None, None], 6, i0=3 | (5 << 16), f0=2.0)
    assert np.array_equal(o[0][0], [1, 3, 5, 11, 13, 15])


def test_ewise_scale_is_the_largest_term():
    """The error yardstick of an element is its largest term, not its result: 1 - t t and p1 + f0 p2 cancel."""
    o = _ew('TANH_BWD', [np.zeros(1), np.array([3.0]), np.array([0.999]), None, None], 1)
    assert o[0][1][0] == 3.0
    o = _ew('AXPY', [np.array([1.0]), np.array([-1.0]), None, None, None], 1, f0=1.0)
    assert o[0][0][0] == 0.0 and o[0][1][0] == 1.0
    assert R.ulps_f32(1.0, 4) == 4 * 2.0 ** -23


def test_f64_yardstick_rule():
    f64 = np.array([1.0, 1e-3, 0.0])
    f32 = f64 + np.array([1e-7, 0.0, 0.0])
    R.assert_f64_close(f64 + np.array([3.9e-7, 1e-8, 1e-6]), f64, f32)
    with pytest.raises(AssertionError):
        R.assert_f64_close(f64 + np.array([0.0, 0.0, 1.1e-6]), f64, f32)
    with pytest.raises(AssertionError):
        R.assert_f64_close(f64 + np.array([1.2e-5, 0.0, 0.0]), f64, f32)
    with pytest.raises(AssertionError):
        R.assert_f64_close(np.array([np.nan, 1e-3, 0.0]), f64, f32)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the loss, attention-backward and sampler references of tests/test_train_loss_kernels_gpu.py
# ---------------------------------------------------------------------------------------------------------------------------------------
def _objective_inputs(seed, n, K1, D, Dp, zd, kl_scale):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=D64)
    return r(n, K1, D), r(n, K1, Dp), r(n, D), r(n, Dp), kl_scale * r(n, 2 * zd)


def test_kl_rows_is_torch_kl_divergence():
    """utils/dist.py:26-29 against torch.distributions: the only difference is the reference's 1e-8 on p.sigma (1e-8 relative)."""
    from torch.distributions import Normal, kl_divergence
    torch.manual_seed(7)
    n, zd = 6, 16
    qzp = 0.7 * torch.randn(n, 2 * zd, dtype=D64)
    mu, lv = qzp[:, :zd], qzp[:, zd:]
    want = kl_divergence(Normal(mu, torch.exp(0.5 * lv)), Normal(torch.zeros_like(mu), torch.ones_like(mu))).sum(1)
    torch.testing.assert_close(R.kl_rows(qzp), want, rtol=1e-7, atol=1e-9)
    # the stage-2 form with a general prior, summed per agent
    K, nz = 3, 5
    m, l, pm, pl = (0.8 * torch.randn(n * K, nz, dtype=D64) for _ in range(4))
    want = kl_divergence(Normal(m, torch.exp(0.5 * l)), Normal(pm, torch.exp(0.5 * pl))).reshape(n, -1).sum(1)
    motion = torch.randn(n, K, 4, dtype=D64)
    got = R.sampler_loss(m, l, pm, pl, motion, 2.0, torch.ones(n, dtype=D64), torch.ones(n, dtype=D64))
    torch.testing.assert_close(got['kld'], want, rtol=1e-7, atol=1e-9)
    got0 = R.sampler_loss(m, l, None, None, motion, 2.0, torch.ones(n, dtype=D64), torch.ones(n, dtype=D64))
    want0 = kl_divergence(Normal(m, torch.exp(0.5 * l)), Normal(torch.zeros_like(m), torch.ones_like(m))).reshape(n, -1).sum(1)
    torch.testing.assert_close(got0['kld'], want0, rtol=1e-7, atol=1e-9)


@pytest.mark.parametrize('csr', [None, (0, 2, 3, 7)])
@pytest.mark.parametrize('kl_scale', [0.1, 1.2])
def test_objective_values_and_gradients_against_closed_forms_and_a_finite_difference(csr, kl_scale):
    """The autograd gradients of R.objective against the hand-derived ones (NumPy, no autograd): 2 scale (p - t) on sample 0, 2 w (p - t) on
    the first-minimum sample, (mu, (sigma^2 - 1) / 2) / denom on the live KL rows and 0 on the clamped ones; and the directional derivative
    of `total` against a central difference."""
    n, K1, D, Dp, zd = 7, 5, 6, 4, 8
    pred, rec, fut, past, qzp = _objective_inputs(21, n, K1, D, Dp, zd, kl_scale)
    sm, sr, min_clip = 1 / 3.0, 1 / 2.0, 2.0
    o = R.objective(pred, rec, fut, past, qzp, csr, K1, sm, sr, float(n), min_clip)
    P, F_, Q = pred.numpy(), fut.numpy(), qzp.numpy()
    ptr = np.array(csr if csr is not None else (0, n))
    ags = R.scene_of(ptr, n)
    cnt = np.diff(ptr)[ags].astype(np.float64)
    d2 = ((F_[:, None] - P[:, 1:]) ** 2).sum(-1)
    best = np.argmin(d2, 1)
    assert np.array_equal(o['best'].numpy(), best + 1)
    np.testing.assert_allclose(o['mse'].item(), ((P[:, 0] - F_) ** 2).sum() * sm, rtol=1e-13)
    np.testing.assert_allclose(o['rec'].item(), ((rec.numpy()[:, 0] - past.numpy()) ** 2).sum() * sr, rtol=1e-13)
    np.testing.assert_allclose(o['diverse'].item(), (d2.min(1) / cnt).sum(), rtol=1e-13)
    mu, lv = Q[:, :zd], Q[:, zd:]
    klr = (0.5 * (mu ** 2 + np.exp(lv)) - 0.5 - 0.5 * lv).sum(1)
    kls = np.array([klr[a:b].sum() / (b - a) for a, b in zip(ptr[:-1], ptr[1:])])
    assert ((kls < 0.9 * min_clip) | (kls > 1.1 * min_clip)).all() and (kls > min_clip).all() == (kl_scale > 0.5)
    np.testing.assert_allclose(o['kl'].item(), np.maximum(kls, min_clip).sum(), rtol=1e-7, atol=1e-7)       # (the 1e-8 on p.sigma: 1e-8 per term)
    np.testing.assert_allclose(R.scene_kl(qzp, csr, float(n)).numpy(), kls, rtol=1e-7, atol=1e-7)
    np.testing.assert_allclose(o['total'].item(), o['mse'].item() + o['rec'].item() + o['kl'].item() + o['diverse'].item(), rtol=1e-14)
    dpred = np.zeros_like(P)
    dpred[:, 0] = 2 * sm * (P[:, 0] - F_)
    dpred[np.arange(n), best + 1] = 2 * (P[np.arange(n), best + 1] - F_) / cnt[:, None]
    np.testing.assert_allclose(o['dpred'].numpy(), dpred, rtol=1e-13, atol=1e-15)
    drec = np.zeros_like(rec.numpy())
    drec[:, 0] = 2 * sr * (rec.numpy()[:, 0] - past.numpy())
    np.testing.assert_allclose(o['drec'].numpy(), drec, rtol=1e-13, atol=1e-15)
    live = (kls > min_clip)[ags][:, None]
    dq = np.concatenate([mu, 0.5 * (np.exp(lv) - 1)], 1) / cnt[:, None] * live
    np.testing.assert_allclose(o['dqzp'].numpy(), dq, rtol=1e-7, atol=1e-7)
    k = R.kl_term(qzp, csr, float(n), min_clip)
    assert torch.equal(k['dqzp'], o['dqzp']) and k['kl'].item() == o['kl'].item()
    # central difference of total along a random direction of all three inputs
    g = torch.Generator().manual_seed(22)
    dP, dR, dQ = (torch.randn(v.shape, generator=g, dtype=D64) for v in (pred, rec, qzp))
    h = 1e-6
    tot = lambda s: R.objective(pred + s * dP, rec + s * dR, fut, past, qzp + s * dQ, csr, K1, sm, sr, float(n), min_clip)['total'].item()
    fd = (tot(h) - tot(-h)) / (2 * h)
    an = ((o['dpred'] * dP).sum() + (o['drec'] * dR).sum() + (o['dqzp'] * dQ).sum()).item()
    np.testing.assert_allclose(an, fd, rtol=1e-7)


def test_objective_best_is_the_first_minimum_on_exact_ties():
    n, K1, D = 4, 9, 6
    pred, rec, fut, past, qzp = _objective_inputs(23, n, K1, D, 4, 8, 0.3)
    pred[0, 6] = fut[0] + 1e-3
    pred[0, 2] = pred[0, 6]                                          # the duplicate at the lower index
    pred[1, 3] = fut[1] - 1e-3
    pred[1, 8] = pred[1, 3]                                          # ... at the higher index
    for dt in (D64, torch.float32):
        o = R.objective(*(v.to(dt) for v in (pred, rec, fut, past, qzp)), None, K1, 1.0, 1.0, float(n), 2.0)
        d2 = ((fut[:, None].to(dt) - pred[:, 1:].to(dt)) ** 2).sum(-1).numpy()
        assert np.array_equal(o['best'].numpy(), np.argmin(d2, 1) + 1)
        assert o['best'][0] == 2 and o['best'][1] == 3
        assert (o['dpred'][0, 6] == 0).all() and (o['dpred'][0, 2] != 0).all() and (o['dpred'][1, 8] == 0).all()
        assert o['dpred'].dtype == dt


def test_sqerr_reference():
    p, t = torch.tensor([1.0, 2.0, 4.0], dtype=D64), torch.tensor([0.0, 4.0, 4.0], dtype=D64)
    o = R.sqerr(p, t, 0.5)
    assert o['value'].item() == 2.5 and torch.equal(o['dpred'], torch.tensor([1.0, -2.0, 0.0], dtype=D64))


def test_attention_reference_edges():
    """L = 1: the softmax is over one key, so dq = dk = 0 and dv = dO.  A pair beyond the clamp (k_i = q_i: dot 1; k_i = -q_j: dot -1)
    passes nothing to q and k: moving q_j along a tangent direction changes the output through its other pairs only."""
    torch.manual_seed(8)
    hd, DM = 8, 64
    qkv, dO = torch.randn(3, 3 * DM, dtype=D64), torch.randn(3, DM, dtype=D64)
    r = R.geodesic_self_attention(qkv, dO, 1, 3, hd)
    assert torch.equal(r['dqkv'][:, :2 * DM], torch.zeros(3, 2 * DM, dtype=D64))
    torch.testing.assert_close(r['dqkv'][:, 2 * DM:], dO, rtol=1e-14, atol=0)
    # L = 2, one slot; every pair of head 0 beyond the clamp: k_0 = q_0, k_1 = q_1 (diagonal), and q_1 = -q_0 (off-diagonal dots -1)
    qkv, dO = torch.randn(2, 3 * DM, dtype=D64), torch.randn(2, DM, dtype=D64)
    qkv[1, :hd] = -qkv[0, :hd]
    qkv[:, DM:DM + hd] = qkv[:, :hd]
    r = R.geodesic_self_attention(qkv, dO, 2, 1, hd)
    assert (r['dots'][0, 0].abs() > 1 - 1e-9).all()
    assert torch.equal(r['dqkv'][:, :hd], torch.zeros(2, hd, dtype=D64)) and torch.equal(r['dqkv'][:, DM:DM + hd], torch.zeros(2, hd, dtype=D64))
    assert (r['dqkv'][:, hd:DM] != 0).all() and (r['dqkv'][:, 2 * DM:2 * DM + hd] != 0).all()      # the other heads, and head 0's dv


def test_sampler_references_on_worked_cases():
    A = torch.tensor([[2.0, 0.0], [-1.0, 1e-4], [3.0, 1.0], [0.5, -2.0]], dtype=D64)         # n = 2, K = 2, nz = 2
    b = torch.arange(8, dtype=D64).reshape(4, 2)
    assert torch.equal(R.sampler_latent(A, b, None, 0, 2)['z'], b)
    e1 = torch.tensor([10.0, 100.0], dtype=D64)
    assert torch.equal(R.sampler_latent(A, b, e1, 1, 2)['z'], A * e1 + b)
    e2 = torch.tensor([[10.0, 100.0], [1.0, 2.0]], dtype=D64)
    z = R.sampler_latent(A, b, e2, 2, 2)
    assert torch.equal(z['z'], torch.tensor([[20.0, 1.0], [-8.0, 3.01], [7.0, 7.0], [6.5, 3.0]], dtype=D64))
    np.testing.assert_allclose(z['logvar'].numpy(), np.log(A.numpy() ** 2 + 1e-8), rtol=1e-15)
    assert z['logvar'][0, 1].item() == np.log(1e-8)


def test_sampler_diversity_is_the_double_loop_over_pairs_and_coincident_samples_pass_no_gradient():
    torch.manual_seed(9)
    n, K, D, nz, scale = 3, 5, 6, 4, 0.5
    motion = 0.3 * torch.randn(n, K, D, dtype=D64)
    motion[1, 3] = motion[1, 0]                                      # two samples identical bit for bit
    mu, lv = torch.randn(n * K, nz, dtype=D64), torch.randn(n * K, nz, dtype=D64)
    g_kld, g_div = torch.randn(n, dtype=D64), torch.randn(n, dtype=D64)
    o = R.sampler_loss(mu, lv, None, None, motion, scale, g_kld, g_div)
    m = motion.numpy()
    div, dm = np.zeros(n), np.zeros_like(m)
    npairs = K * (K - 1) // 2
    for a in range(n):
        for i in range(K):
            for j in range(i + 1, K):
                s = ((m[a, i] - m[a, j]) ** 2).sum()
                e = np.exp(-s / scale)
                div[a] += e / npairs
                dm[a, i] += g_div[a].item() * e * (-2 / scale) * (m[a, i] - m[a, j]) / npairs
                dm[a, j] -= g_div[a].item() * e * (-2 / scale) * (m[a, i] - m[a, j]) / npairs
    np.testing.assert_allclose(o['div'].numpy(), div, rtol=1e-13)
    np.testing.assert_allclose(o['dmotion'].numpy(), dm, rtol=1e-12, atol=1e-15)
    assert np.isfinite(o['dmotion'].numpy()).all()
    np.testing.assert_allclose(o['dmu'].numpy(), (g_kld.repeat_interleave(K)[:, None] * mu).numpy(), rtol=1e-7)
    np.testing.assert_allclose(o['dlogvar'].numpy(), (g_kld.repeat_interleave(K)[:, None] * 0.5 * (lv.exp() - 1)).numpy(), rtol=1e-7, atol=1e-7)
