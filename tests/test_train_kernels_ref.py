"""The float64 references of tests/train_ref.py (the yardsticks of tests/test_train_kernels_gpu.py) pinned against torch's own modules in
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
