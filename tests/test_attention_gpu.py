"""GPU: the attention core with a running maximum (csrc/attention.hip: geodesic and dot-product scores, optional additive mask, forward and
backward), ops.mha / ops.mhgsa(attn_mask=...), the stand-alone modules of sttode_amd.attention and the ``euclidean=True`` layers.

Kernels are held to the float64 evaluation of the plain-torch restatement (tests/attention_ref.py) through helpers.yardstick_close with
the constants of test_stack_autograd.close: the HIP result may sit from the float64 value as far as a correct fp32 evaluation (torch on
the CPU, or the reference's own fp32 fixture tests/golden/attention.npz) does, times 4, plus rtol 1e-4 and a floor relative to the
tensor's largest entry (3e-4 for gradients, 1e-4 for outputs, as test_stack_autograd.compare uses).  Head-averaged weights lie in [0, 1]
and are compared with rtol 1e-4, atol 1e-6, as the fixture tests do; a weight row sums to 1 within 1e-5 + cols 2^-23 (each of the cols
terms carries a few ulps of relative error and they add up to 1)."""
import os

import numpy as np
import pytest
import torch

import attention_ref as AR
from helpers import assert_close
from test_attention import MODES, MODULE_CASES, attn_state, case_inputs, qkv, ref_module, stack_layer
from test_stack_autograd import close, compare, decoder_state, encoder_state, hip_run, oracle_run

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SC = 8 ** -0.5


def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def golden():
    return np.load(os.path.join(HERE, 'golden', 'attention.npz'))


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def operands(rows, cols, Nb, seed=0):
    rng = np.random.default_rng(rows * 1000 + cols + seed)
    R, C = rng.standard_normal((rows, Nb, 64)).astype(np.float32), rng.standard_normal((cols, Nb, 64)).astype(np.float32)
    V, dO = rng.standard_normal((cols, Nb, 64)).astype(np.float32), rng.standard_normal((rows, Nb, 64)).astype(np.float32)
    return R, C, V, dO


def make_mask(rows, cols, seed=0):
    """Finite entries ~ 2 N(0,1), a fifth of them -inf, every third row -inf over its whole first 128-column tile (a leading run the running
    maximum has to survive); the last column stays finite, so no row is masked everywhere."""
    rng = np.random.default_rng(7000 + rows * 1000 + cols + seed)
    m = (2 * rng.standard_normal((rows, cols))).astype(np.float32)
    m[rng.random((rows, cols)) < 0.2] = -np.inf
    m[1::3, :128] = -np.inf
    m[:, -1] = np.float32(0.25)
    return m


def padded(mask):
    """The mask as a view of a wider device buffer (ld_mask = cols + 5; the padding is NaN and must never be read)."""
    rows, cols = mask.shape
    buf = torch.full((rows, cols + 5), float('nan'), device=dev())
    buf[:, :cols] = t(mask)
    return buf, cols + 5


def hip_core(R, C, V, rs, cs, mode, mask=None, weights=True):
    from sttode_amd import capi
    rows, Nb, E = R.shape
    cols = C.shape[0]
    Rd, Cd, Vd = t(R), t(C), t(V)
    out = torch.full((rows, Nb, E), float('nan'), device=dev())
    wmax, wsum = (torch.full((Nb * 8 * rows,), float('nan'), device=dev()) for _ in range(2)) if weights else (None, None)
    wout = torch.full((Nb, rows, cols), float('nan'), device=dev()) if weights else None
    mbuf, ld = padded(mask) if mask is not None else (None, 0)
    st = Nb * E
    capi.call('sttode_attn_core', Rd, Cd, Vd, mbuf, ld, out, wmax, wsum, wout, rows, cols, Nb, st, E, st, E, st, E, st, E, rs, cs, mode,
              capi.stream_ptr())
    torch.cuda.synchronize()
    return out.cpu().numpy(), (wout.cpu().numpy() if weights else None)


def hip_core_bwd(R, C, V, dO, rs, cs, mode, mask=None):
    from sttode_amd import capi
    rows, Nb, E = R.shape
    cols = C.shape[0]
    Rd, Cd, Vd, dOd = t(R), t(C), t(V), t(dO)
    dR, dC, dV = (torch.full_like(a, float('nan')) for a in (Rd, Cd, Vd))
    mbuf, ld = padded(mask) if mask is not None else (None, 0)
    st = Nb * E
    capi.call('sttode_attn_core_bwd', Rd, Cd, Vd, mbuf, ld, dOd, dR, dC, dV, rows, cols, Nb, st, E, st, E, st, E, st, E, rs, cs, mode,
              capi.stream_ptr())
    torch.cuda.synchronize()
    return [a.cpu().numpy() for a in (dR, dC, dV)]


def ref_core(R, C, V, rs, cs, mode, mask, double, dO=None):
    ts = [torch.from_numpy(a) for a in (R, C, V)]
    if double:
        ts = [a.double() for a in ts]
    mk = None if mask is None else torch.from_numpy(mask)
    if dO is None:
        with torch.no_grad():
            o, w = AR.core(*ts, rs, cs, mode, mk)
        return o.numpy(), w.numpy()
    ts = [a.requires_grad_(True) for a in ts]
    o, _ = AR.core(*ts, rs, cs, mode, mk)
    o.backward(torch.from_numpy(dO).double() if double else torch.from_numpy(dO))
    return [a.grad.numpy() for a in ts]


# ---------------------------------------------------------------------------------------------------------------------------------
# kernels
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('masked', [False, True], ids=['unmasked', 'masked'])
@pytest.mark.parametrize('mode', [0, 1], ids=['geodesic', 'dot'])
@pytest.mark.parametrize('rows,cols,Nb', [(1, 1, 1), (5, 5, 3), (63, 129, 2), (64, 128, 1), (65, 257, 2), (130, 127, 1)])
def test_forward_kernel_vs_float64(rows, cols, Nb, mode, masked):
    R, C, V, _ = operands(rows, cols, Nb)
    mask = make_mask(rows, cols) if masked else None
    rs, cs = (1.0, SC) if rows == cols else (SC, 1.0)
    out, w = hip_core(R, C, V, rs, cs, mode, mask)
    o32, w32 = ref_core(R, C, V, rs, cs, mode, mask, False)
    o64, w64 = ref_core(R, C, V, rs, cs, mode, mask, True)
    assert np.isfinite(out).all() and np.isfinite(w).all()
    what = f'attn core fwd mode {mode} masked {masked} {rows}x{cols} Nb={Nb}'
    close(out, o32, o64, what + ' out', floor=1e-4)
    assert_close(w, w64, rtol=1e-4, atol=1e-6, what=what + ' weights')
    assert np.abs(w.sum(-1) - 1).max() <= 1e-5 + cols * 2.0 ** -23, what
    if masked:
        assert (w[:, np.isneginf(mask)] == 0).all(), what
    out2, _ = hip_core(R, C, V, rs, cs, mode, mask, weights=False)           # without the workspaces: the same output bits
    assert np.array_equal(out, out2), what


@pytest.mark.parametrize('orient', ['rows_keys', 'rows_queries'])
@pytest.mark.parametrize('mode', [0, 1], ids=['geodesic', 'dot'])
@pytest.mark.parametrize('rows,cols,Nb', [(1, 1, 1), (5, 5, 3), (65, 129, 2), (130, 127, 1)])
def test_backward_kernel_vs_float64(rows, cols, Nb, mode, orient):
    R, C, V, dO = operands(rows, cols, Nb, seed=1)
    rs, cs = (1.0, SC) if orient == 'rows_keys' else (SC, 1.0)
    for mask in (make_mask(rows, cols, seed=1), None):
        got = hip_core_bwd(R, C, V, dO, rs, cs, mode, mask)
        g32 = ref_core(R, C, V, rs, cs, mode, mask, False, dO)
        g64 = ref_core(R, C, V, rs, cs, mode, mask, True, dO)
        for nm, a, b, c in zip(('dR', 'dC', 'dV'), got, g32, g64):
            assert np.isfinite(a).all(), nm
            close(a, b, c, f'attn core bwd mode {mode} {orient} masked {mask is not None} {rows}x{cols} Nb={Nb} {nm}')


def test_forward_and_backward_are_deterministic():
    rows, cols, Nb = 65, 257, 2
    R, C, V, dO = operands(rows, cols, Nb, seed=2)
    mask = make_mask(rows, cols, seed=2)
    for mode in (0, 1):
        for mk in (mask, None):
            a, b = hip_core(R, C, V, SC, 1.0, mode, mk), hip_core(R, C, V, SC, 1.0, mode, mk)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (mode, mk is None)
            ga, gb = hip_core_bwd(R, C, V, dO, SC, 1.0, mode, mk), hip_core_bwd(R, C, V, dO, SC, 1.0, mode, mk)
            assert all(np.array_equal(x, y) for x, y in zip(ga, gb)), (mode, mk is None)


def test_fully_masked_row_is_nan_and_only_that_row():
    rows, cols, Nb = 65, 130, 2
    R, C, V, _ = operands(rows, cols, Nb, seed=3)
    mask = make_mask(rows, cols, seed=3)
    mask[[0, 64], :] = -np.inf
    for mode in (0, 1):
        out, w = hip_core(R, C, V, SC, 1.0, mode, mask)
        o64, w64 = ref_core(R, C, V, SC, 1.0, mode, mask, True)
        assert (np.isnan(out) == np.isnan(o64)).all() and (np.isnan(w) == np.isnan(w64)).all()
        assert np.isnan(out[[0, 64]]).all() and np.isfinite(np.delete(out, [0, 64], axis=0)).all()
        ok = ~np.isnan(o64)
        assert_close(out[ok], o64[ok], what=f'mode {mode}: rows beside a fully masked one')


def test_forward_under_graph_capture_replays_bitwise():
    """No host synchronisation and no allocation inside the C entry: it can be captured, and the replay recomputes the eager bits."""
    from sttode_amd import capi
    rows, cols, Nb = 65, 257, 2
    R, C, V, _ = operands(rows, cols, Nb, seed=4)
    mask = make_mask(rows, cols, seed=4)
    for mode in (0, 1):
        want, wantw = hip_core(R, C, V, SC, 1.0, mode, mask)
        Rd, Cd, Vd = t(R), t(C), t(V)
        mbuf, ld = padded(mask)
        out = torch.empty(rows, Nb, 64, device=dev())
        wmax, wsum = torch.empty(Nb * 8 * rows, device=dev()), torch.empty(Nb * 8 * rows, device=dev())
        wout = torch.empty(Nb, rows, cols, device=dev())
        st = Nb * 64
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            capi.call('sttode_attn_core', Rd, Cd, Vd, mbuf, ld, out, wmax, wsum, wout, rows, cols, Nb, st, 64, st, 64, st, 64, st, 64, SC, 1.0,
                      mode, capi.stream_ptr())
        for _ in range(2):
            out.fill_(float('nan'))
            wout.fill_(float('nan'))
            g.replay()
            torch.cuda.synchronize()
            assert np.array_equal(out.cpu().numpy(), want) and np.array_equal(wout.cpu().numpy(), wantw), mode
        del g


def test_backward_refuses_shapes_over_its_lds_bound():
    from sttode_amd import capi
    a = torch.zeros(469, 1, 64, device=dev())
    d = torch.full_like(a, 7.0)
    with pytest.raises(capi.SttodeError, match='sttode_attn_core_bwd.*64 KiB'):
        capi.call('sttode_attn_core_bwd', a, a, a, None, 0, a, d, d, d, 469, 469, 1, 64, 64, 64, 64, 64, 64, 64, 64, 1.0, 1.0, 1, capi.stream_ptr())
    torch.cuda.synchronize()
    assert (d == 7.0).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# ops and modules against the reference's fixture
# ---------------------------------------------------------------------------------------------------------------------------------
def params():
    sd = attn_state()
    return [sd[n].to(dev()) for n in ('in_proj_weight', 'in_proj_bias', 'out_proj.weight', 'out_proj.bias')]


@pytest.mark.parametrize('case', MODULE_CASES)
@pytest.mark.parametrize('mod', ['hyp', 'euc'])
def test_ops_forward_vs_reference_fixture(golden, mod, case):
    from sttode_amd import ops
    tag = f'{mod}_{case}'
    inputs, mask, _ = case_inputs(golden, tag)
    xs = [t(x) for x in inputs]
    op = ops.mhgsa if mod == 'hyp' else ops.mha
    out, w = op(*qkv(xs), *params(), need_weights=True, attn_mask=None if mask is None else t(mask))
    assert not out.requires_grad
    assert_close(out.cpu().numpy(), golden[f'{tag}_out'], what=f'{tag} out')
    assert_close(w.cpu().numpy(), golden[f'{tag}_w'], rtol=1e-4, atol=1e-6, what=f'{tag} weights')
    out2, w2 = op(*qkv(xs), *params(), attn_mask=None if mask is None else t(mask))
    assert w2 is None and torch.equal(out, out2)


@pytest.mark.parametrize('case', MODULE_CASES)
@pytest.mark.parametrize('mod', ['hyp', 'euc'])
def test_modules_vs_reference_fixture(golden, mod, case):
    from sttode_amd import attention
    tag = f'{mod}_{case}'
    m = (attention.Hyp_mhsa if mod == 'hyp' else attention.MultiheadAttention)(64, 8)
    m.load_state_dict(attn_state(), strict=True)
    m = m.to(dev())
    inputs, mask, G = case_inputs(golden, tag)
    mk_d = None if mask is None else t(mask)
    mk_c = None if mask is None else torch.from_numpy(mask)
    with torch.no_grad():
        y0, w0 = m(*qkv([t(x) for x in inputs]), attn_mask=mk_d, key_padding_mask=torch.ones(inputs[0].shape[1], inputs[-1].shape[0],
                                                                                            dtype=torch.bool, device=dev()))
    assert_close(w0.cpu().numpy(), golden[f'{tag}_w'], rtol=1e-4, atol=1e-6, what=f'{tag} weights')   # (the padding mask is ignored)
    hip = hip_run(m, inputs, lambda *xs: m(*qkv(xs), attn_mask=mk_d)[0], G)
    assert np.array_equal(hip[0], y0.cpu().numpy())                          # the graph path runs the same forward kernels
    assert_close(hip[0], golden[f'{tag}_out'], what=f'{tag} out')
    o = ref_module(MODES[mod])
    run_o = lambda mm, *xs: mm(*qkv(xs), attn_mask=mk_c)[0]
    compare(hip, oracle_run(o, inputs, run_o, G, False), oracle_run(o, inputs, run_o, G, True), tag, golden=golden, tag=tag)


@pytest.mark.parametrize('tag', ['edec', 'eenc'])
def test_euclidean_layers_vs_reference_fixture(golden, tag):
    from sttode_amd import hypertransformer as ht
    if tag == 'edec':
        m = ht.TransformerDecoderLayer(64, 8, 256, euclidean=True)
        m.load_state_dict(decoder_state(), strict=True)
        run_h, run_o = (lambda a, b: m(a, b, seq_mask=True)[0]), (lambda mm, a, b: mm(a, b))
    else:
        m = ht.TransformerEncoderLayer(64, 8, 256, euclidean=True)
        m.load_state_dict(encoder_state(), strict=True)
        run_h, run_o = (lambda a: m(a)), (lambda mm, a: mm(a))
    m = m.to(dev())
    inputs, _, G = case_inputs(golden, tag)
    o = stack_layer(tag)
    hip = hip_run(m, inputs, run_h, G)
    o64 = oracle_run(o, inputs, run_o, G, True)
    assert_close(hip[0], golden[f'{tag}_out'], what=f'{tag} out vs reference fixture')
    compare(hip, oracle_run(o, inputs, run_o, G, False), o64, f'euclidean {tag}', golden=golden, tag=tag)
    with torch.no_grad():                                                     # and the default stays geodesic: another result
        geo = ht.TransformerEncoderLayer(64, 8, 256) if tag == 'eenc' else ht.TransformerDecoderLayer(64, 8, 256)
        geo.load_state_dict(m.state_dict(), strict=True)
        y = geo.to(dev())(*[t(x) for x in inputs])
        y = y[0] if isinstance(y, tuple) else y
    assert np.abs(y.cpu().numpy() - hip[0]).max() > 1e-3


def test_overflow_case_is_finite_and_matches_float64(golden):
    from sttode_amd import ops
    tag = 'euc_overflow'
    inputs, _, _ = case_inputs(golden, tag)
    assert float(golden['euc_overflow_maxscore']) > 89.0
    out, w = ops.mha(*qkv([t(x) for x in inputs]), *params(), need_weights=True)
    out, w = out.cpu().numpy(), w.cpu().numpy()
    assert np.isfinite(out).all() and np.isfinite(w).all()
    o = ref_module(1, double=True)
    with torch.no_grad():
        y64, w64 = o(*qkv([torch.from_numpy(x).double() for x in inputs]))
    close(out, golden[f'{tag}_out'], y64.numpy(), tag + ' out', floor=1e-4)
    close(w, golden[f'{tag}_w'], w64.numpy(), tag + ' weights', floor=1e-4)


@pytest.mark.parametrize('mod', ['hyp', 'euc'])
def test_fully_masked_row_matches_the_fixture(golden, mod):
    from sttode_amd import ops
    tag = f'{mod}_nanrow'
    inputs, mask, _ = case_inputs(golden, tag)
    op = ops.mhgsa if mod == 'hyp' else ops.mha
    out, w = op(*qkv([t(x) for x in inputs]), *params(), need_weights=True, attn_mask=t(mask))
    out, w = out.cpu().numpy(), w.cpu().numpy()
    nan = golden[f'{tag}_nan']
    assert (np.isnan(out) == nan).all() and np.isfinite(out[~nan]).all()
    assert (np.isnan(w) == np.isnan(golden[f'{tag}_w'])).all()
    assert_close(out[~nan], golden[f'{tag}_out'][~nan], what=tag + ' out')
    fin = ~np.isnan(w)
    assert_close(w[fin], golden[f'{tag}_w'][fin], rtol=1e-4, atol=1e-6, what=tag + ' weights')


def test_unchanged_paths_and_zero_mask():
    from sttode_amd import ops
    rng = np.random.default_rng(5)
    x = t(rng.standard_normal((9, 4, 64)).astype(np.float32))
    mem = t(rng.standard_normal((6, 4, 64)).astype(np.float32))
    for q, kv in ((x, x), (x, mem)):
        a, wa = ops.mhgsa(q, kv, kv, *params(), need_weights=True)
        b, wb = ops.mhgsa(q, kv, kv, *params(), need_weights=True, attn_mask=None)
        assert torch.equal(a, b) and torch.equal(wa, wb)
        z, wz = ops.mhgsa(q, kv, kv, *params(), need_weights=True, attn_mask=torch.zeros(q.shape[0], kv.shape[0], device=dev()))
        assert_close(z.cpu().numpy(), a.cpu().numpy(), what='zero mask out')
        assert_close(wz.cpu().numpy(), wa.cpu().numpy(), rtol=1e-4, atol=1e-6, what='zero mask weights')


def test_graph_rule_aliasing_and_refusals():
    from sttode_amd import capi, ops
    rng = np.random.default_rng(6)
    P = [p.clone().requires_grad_(True) for p in params()]
    x = t(rng.standard_normal((7, 3, 64)).astype(np.float32)).requires_grad_(True)
    mask = t(make_mask(7, 7, seed=6))
    G = t(rng.standard_normal((7, 3, 64)).astype(np.float32))
    for op in (ops.mha, ops.mhgsa):
        out, w = op(x, x, x, *P, need_weights=True, attn_mask=mask)
        assert not out.requires_grad                                          # values only by default
        with torch.no_grad():
            assert not op(x, x, x, *P, attn_mask=mask, differentiable=True)[0].requires_grad
        out, w = op(x, x, x, *P, need_weights=True, attn_mask=mask, differentiable=True)
        assert out.requires_grad and not w.requires_grad
        x.grad = None
        (out * G).sum().backward()
        g_alias = x.grad.clone()                                              # one accumulated gradient for the aliased inputs
        xs = [x.detach().clone().requires_grad_(True) for _ in range(3)]
        (op(*xs, *P, attn_mask=mask, differentiable=True)[0] * G).sum().backward()
        tot = (xs[0].grad + xs[1].grad + xs[2].grad).cpu().numpy()
        assert_close(g_alias.cpu().numpy(), tot, rtol=1e-5, atol=1e-5 * float(np.abs(tot).max()), what='aliased inputs')
        out = op(x, x, x, *P, attn_mask=mask, differentiable=True)[0]
        (g1,) = torch.autograd.grad((out * out).sum(), [x], create_graph=True)
        with pytest.raises(RuntimeError, match='differentiate twice|once_differentiable'):
            g1.sum().backward()
        mk = mask.clone()
        out = op(x, x, x, *P, attn_mask=mk, differentiable=True)[0]
        mk[0, 0] = 1.0                                                         # the mask is saved for the backward: an edit in between is caught
        with pytest.raises(RuntimeError, match='modified by an inplace operation'):
            (out * G).sum().backward()
        with pytest.raises(ValueError):
            op(x, x, x, *P, attn_mask=mask.clone().requires_grad_(True))
        with pytest.raises(ValueError):
            op(x, x, x, *P, attn_mask=mask.double())
        with pytest.raises(ValueError):
            op(x, x, x, *P, attn_mask=mask[:, :6])
        with pytest.raises(ValueError):
            op(x, x, x, *P, attn_mask=mask.cpu())
        with pytest.raises(NotImplementedError):
            op(x, x, x, *P, num_heads=4)
        with pytest.raises(NotImplementedError):
            op(x[..., :32], x[..., :32], x[..., :32], *P)
    with pytest.raises(capi.SttodeError, match='sttode_attn_core'):
        capi.call('sttode_attn_core', x, x, x, None, 0, x, None, None, x, 7, 7, 3, 192, 64, 192, 64, 192, 64, 192, 64, 1.0, 1.0, 0, capi.stream_ptr())
