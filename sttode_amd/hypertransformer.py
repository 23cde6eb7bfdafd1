"""Op-level drop-ins for the reference's geodesic transformer blocks (hypertransformer.py, ode_demo.py) on the HIP kernels,
with an opt-in HIP backward.  STTODENet itself uses the fused encoder path (csrc/encoder.hip); these classes cover the parts of the
file the model never instantiates -- the decoder-side stack with cross-attention over a memory of a different length
 -- with the reference's constructor arguments, parameter names and call signatures:

    Hypattention(d_model, nhead)                      hypertransformer.py:19-89   (MHGSA, then tanh(info) * sigmoid(gate))
    TransformerEncoderLayer(d_model, nhead, ff)       :91-153
    TransformerDecoderLayer(d_model, nhead, ff)       :156-236  (self-attn, cross-attn, relu FFN, three post-LayerNorms)
    ODEG(decoder_layer, nlayer, time)                 ode_demo.py:195-213 over TransformerDecoder_ode :74-133 (one Euler step + relu)
    ODEG_Encoder(encoder_layer, nlayer, time)         ode_demo.py:217-231

d_model = 64, nhead = 8 (the kernels' build); dropout must be 0 (the only value the repo passes); attention / padding masks
and ``seq_mask`` are accepted and ignored exactly as Hypattention.forward ignores them (:69-72 builds a mask nobody reads).
(The stand-alone attention modules that DO apply ``attn_mask`` are in attention.py.)

``euclidean=True`` (keyword-only, on Hypattention and the two layers) swaps the attention core for dot-product attention (ops.mha, the
transformerlib.MultiheadAttention computation with the same parameters): the geodesic-versus-Euclidean ablation on the device.  Rows then
follow the queries for every L, S; gate, FFN, LayerNorms and the ODEG stacks are unchanged.  The default is today's code bit for bit.

By default every forward computes values only: outputs carry no graph, whatever grad mode says.  ``trainable(module)`` switches
autograd on for every drop-in inside ``module`` (the flag survives ``copy.deepcopy``, so ODEG / ODEG_Encoder clones keep it).  A graph is
then built when grad mode is on and an input or parameter requires grad: torch.autograd.Functions run the same forward kernels (values
bitwise the default path's) and a HIP backward -- sttode_mhgsa_attn_rc_bwd for the attention core, sttode_tlinear_bwd for the linear
layers, sttode_ln_bwd for the LayerNorms, sttode_train_ewise for the gate, the Euler step + relu and the integrators' stage combinations.
Backward functions are once-differentiable (double backward raises); attention weights are not differentiable.
"""
import copy

import torch
from torch import nn
from torch.autograd.function import once_differentiable

from . import capi
from .attention import Hyp_mhsa, MultiheadAttention
from .ops import linear_bwd, linear_cols, mha, mhgsa, scratch
from .model import _HypMHSA


def _gpu(t):
    if t.device.type != 'cuda':
        raise capi.SttodeError('hypertransformer ops run only on a HIP device (no CPU fallback)')


def _add_ln_fwd(x2, r2, gamma, beta):
    rows = x2.shape[0]
    y, xh, rs = torch.empty_like(x2), torch.empty_like(x2), torch.empty(rows, device=x2.device)
    capi.call('sttode_add_ln_fwd', x2, r2, gamma, beta, y, xh, rs, rows, x2.shape[-1], capi.stream_ptr())
    return y, xh, rs


class _AddLN(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x2, r2, gamma, beta):
        y, xh, rs = _add_ln_fwd(x2, r2, gamma, beta)
        ctx.save_for_backward(xh, rs, gamma)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        xh, rs, gamma = ctx.saved_tensors
        rows, D = xh.shape
        dsum, dg, db = torch.empty_like(xh), torch.zeros_like(gamma), torch.zeros_like(gamma)
        sc = scratch(xh.device)
        capi.call('sttode_ln_bwd', dy.contiguous(), xh, rs, gamma, dsum, dg, db, rows, D, sc, sc.numel(), capi.stream_ptr())
        return dsum, dsum, dg, db


def _add_ln(x, r, norm, grad=False):
    """LayerNorm(x + r) over the last (64) dimension on sttode_add_ln_fwd."""
    shape = x.shape
    x2, r2 = x.reshape(-1, 64).contiguous(), r.reshape(-1, 64).contiguous()
    if grad:
        return _AddLN.apply(x2, r2, norm.weight, norm.bias).view(shape)
    return _add_ln_fwd(x2, r2, norm.weight, norm.bias)[0].view(shape)


def _gate_fwd(o2, info, gate):
    """tanh(info(o2)) * sigmoid(gate(o2)) (hypertransformer.py:81-83) -> (g, t, s)."""
    rows, D = o2.shape
    t = linear_cols(o2, info.weight, info.bias, act='tanh')
    s = torch.empty_like(t)
    capi.call('sttode_tlinear', o2, D, 1, gate.weight, D, 0, gate.bias, None, 0, s, D, rows, D, D, 3, 0, capi.stream_ptr())
    g = torch.empty_like(t)
    capi.call('sttode_train_ewise', 0, g, t, s, None, None, g.numel(), 0, 0.0, capi.stream_ptr())
    return g, t, s


class _Gate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, o2, info, gate, Wi, bi, Wg, bg):
        g, t, s = _gate_fwd(o2, info, gate)
        ctx.save_for_backward(o2, t, s, Wi, Wg)
        return g

    @staticmethod
    @once_differentiable
    def backward(ctx, dg):
        o2, t, s, Wi, Wg = ctx.saved_tensors
        du, dv = torch.empty_like(t), torch.empty_like(t)
        capi.call('sttode_train_ewise', 2, dg.contiguous(), t, s, du, dv, t.numel(), 0, 0.0, capi.stream_ptr())
        dWi, dbi, dWg, dbg = torch.zeros_like(Wi), torch.zeros(Wi.shape[0], device=t.device), torch.zeros_like(Wg), torch.zeros(Wg.shape[0], device=t.device)
        do = linear_bwd(du, Wi, o2, torch.empty_like(o2), dWi, dbi)
        linear_bwd(dv, Wg, o2, do, dWg, dbg, accumulate=True)
        return do, None, None, dWi, dbi, dWg, dbg


class Hypattention(nn.Module):
    def __init__(self, d_model, nhead, dropout=0., motion_only=True, cross_range=0, num_conv_layer=3, *, euclidean=False):
        super().__init__()
        if d_model != 64 or nhead != 8 or dropout != 0.:
            raise NotImplementedError('HIP attention is built for d_model=64, nhead=8, dropout=0')
        self.model_dim = d_model
        self.euclidean = bool(euclidean)          # the attention core is ops.mha (dot product, rows = queries) instead of ops.mhgsa
        self.temporal_attention_before = _HypMHSA(d_model, nhead)
        self.temporal_info = nn.Linear(d_model, d_model)
        self.temporal_gate = nn.Linear(d_model, d_model)
        self._trainable = False

    def forward(self, query, key, value, key_padding_mask=None, need_weights=False, attn_mask=None, seq_mask=False):
        _gpu(query)
        assert len(query.shape) == len(key.shape) == len(value.shape) == 4            # [T, N, sample_num, D]
        assert query.shape[1] == key.shape[1] == value.shape[1] and query.shape[2] == key.shape[2] == value.shape[2]
        assert key.shape[0] == value.shape[0]
        grad = _graph(self, query, key, value)
        with torch.set_grad_enabled(grad):
            Lq, A, Sn, D = query.shape
            Lk = key.shape[0]
            m = self.temporal_attention_before
            q3 = query.reshape(Lq, A * Sn, D)
            k3 = q3 if key is query else key.reshape(Lk, A * Sn, D)
            v3 = k3 if value is key else (q3 if value is query else value.reshape(Lk, A * Sn, D))
            op = mha if getattr(self, 'euclidean', False) else mhgsa
            out, w = op(q3, k3, v3, m.in_proj_weight, m.in_proj_bias, m.out_proj.weight, m.out_proj.bias, need_weights=True,
                        differentiable=grad)
            o2 = out.reshape(out.shape[0] * out.shape[1], D)
            if grad:
                ti, tg = self.temporal_info, self.temporal_gate
                g = _Gate.apply(o2, ti, tg, ti.weight, ti.bias, tg.weight, tg.bias)
            else:
                g = _gate_fwd(o2, self.temporal_info, self.temporal_gate)[0]
            # NB with L == S the reference's untransposed scores make the output rows follow the KEYS (hyptransformerlib.py:261-265);
            # mhgsa returns [rows, A*Sn, D] accordingly and rows == Lq in every case (mha: rows follow the queries, always)
            return g.view(out.shape[0], A, Sn, D), w


class _FFN(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x2, W1, b1, W2, b2):
        h = linear_cols(x2, W1, b1, act='relu')
        ctx.save_for_backward(x2, h, W1, W2)
        return linear_cols(h, W2, b2)

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        x2, h, W1, W2 = ctx.saved_tensors
        dev = x2.device
        dW1, db1, dW2, db2 = torch.zeros_like(W1), torch.zeros(W1.shape[0], device=dev), torch.zeros_like(W2), torch.zeros(W2.shape[0], device=dev)
        dh = linear_bwd(dy.contiguous(), W2, h, torch.empty_like(h), dW2, db2, mask=h)          # relu backward: the mask h > 0
        dx = linear_bwd(dh, W1, x2, torch.empty_like(x2), dW1, db1)
        return dx, dW1, db1, dW2, db2


def _ffn(x, lin1, lin2, grad=False):
    x2 = x.reshape(-1, 64).contiguous()
    if grad:
        return _FFN.apply(x2, lin1.weight, lin1.bias, lin2.weight, lin2.bias).view(x.shape)
    return linear_cols(linear_cols(x2, lin1.weight, lin1.bias, act='relu'), lin2.weight, lin2.bias).view(x.shape)


def _graph(mod, *inputs):
    """Build a graph: the module opted in, grad mode is on, and an input or a parameter requires grad."""
    return (getattr(mod, "_trainable", False) and torch.is_grad_enabled()
            and (any(t is not None and t.requires_grad for t in inputs) or any(p.requires_grad for p in mod.parameters())))


class TransformerEncoderLayer(nn.Module):
    def __init__(self, d_model, nhead, dim_feedforward=2048, dropout=0., activation='relu', *, euclidean=False):
        super().__init__()
        if activation != 'relu' or dim_feedforward % 16:
            raise NotImplementedError('relu FFN with a hidden width that is a multiple of 16')
        self.self_attn = Hypattention(d_model, nhead, dropout=dropout, euclidean=euclidean)
        self.linear1, self.linear2 = nn.Linear(d_model, dim_feedforward), nn.Linear(dim_feedforward, d_model)
        self.norm1, self.norm2 = nn.LayerNorm(d_model), nn.LayerNorm(d_model)
        self._trainable = False

    def forward(self, src, src_mask=None, src_key_padding_mask=None):
        grad = _graph(self, src)
        with torch.set_grad_enabled(grad):
            src = _add_ln(src, self.self_attn(src, src, src)[0], self.norm1, grad)
            return _add_ln(src, _ffn(src, self.linear1, self.linear2, grad), self.norm2, grad)


class TransformerDecoderLayer(nn.Module):
    def __init__(self, d_model, nhead, dim_feedforward=2048, dropout=0., activation='relu', cross_motion_only=False, *, euclidean=False):
        super().__init__()
        if activation != 'relu' or dim_feedforward % 16:
            raise NotImplementedError('relu FFN with a hidden width that is a multiple of 16')
        self.self_attn = Hypattention(d_model, nhead, dropout=dropout, euclidean=euclidean)
        self.cross_attn = Hypattention(d_model, nhead, dropout=dropout, euclidean=euclidean)
        self.linear1, self.linear2 = nn.Linear(d_model, dim_feedforward), nn.Linear(dim_feedforward, d_model)
        self.norm1, self.norm2, self.norm3 = nn.LayerNorm(d_model), nn.LayerNorm(d_model), nn.LayerNorm(d_model)
        self.cross_motion_only = cross_motion_only
        self._trainable = False

    def forward(self, tgt, memory, tgt_mask=None, memory_mask=None, seq_mask=False, tgt_key_padding_mask=None,
                memory_key_padding_mask=None, need_weights=False):
        grad = _graph(self, tgt, memory)
        with torch.set_grad_enabled(grad):
            a, w_self = self.self_attn(tgt, tgt, tgt, seq_mask=seq_mask)
            tgt = _add_ln(tgt, a, self.norm1, grad)
            a, w_cross = self.cross_attn(tgt, memory, memory)
            tgt = _add_ln(tgt, a, self.norm2, grad)
            tgt = _add_ln(tgt, _ffn(tgt, self.linear1, self.linear2, grad), self.norm3, grad)
            return tgt, w_self, w_cross


def _euler_relu_fwd(x, y, time):
    out = torch.empty_like(x)
    capi.call('sttode_train_ewise', 3, out, x, y, None, None, out.numel(), 0, float(time), capi.stream_ptr())
    return out


class _EulerRelu(torch.autograd.Function):
    """relu(x + time * y) (ewise op 3); backward ewise op 4."""

    @staticmethod
    def forward(ctx, x, y, time):
        out = _euler_relu_fwd(x, y, time)
        ctx.time = float(time)
        ctx.save_for_backward(out)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        out, = ctx.saved_tensors
        dx, dy = torch.zeros_like(out), torch.empty_like(out)
        capi.call('sttode_train_ewise', 4, dout.contiguous(), out, None, dx, dy, out.numel(), 0, ctx.time, capi.stream_ptr())
        return dx, dy, None


def _euler_relu(x, y, time, grad=False):
    if grad:
        return _EulerRelu.apply(x.contiguous(), y.contiguous(), time)
    return _euler_relu_fwd(x.contiguous(), y.contiguous(), time)


def _axpy(y, a, x):
    """y += a * x (in place, HIP element kernel)."""
    capi.call('sttode_train_ewise', 1, y, x.contiguous(), None, None, None, y.numel(), 0, float(a), capi.stream_ptr())
    return y


def _relu_(x, grad=False):
    z = torch.zeros_like(x)
    if grad:
        return _EulerRelu.apply(x.contiguous(), z, 0.0)
    out = torch.empty_like(x)
    capi.call('sttode_train_ewise', 3, out, x.contiguous(), z, None, None, out.numel(), 0, 0.0, capi.stream_ptr())
    return out


class _Comb(torch.autograd.Function):
    """y + sum_i a_i k_i out of place: a zeroed buffer, y added, then the a_i k_i in order (ewise op 1) -- the bits of the in-place chain
    of _axpy calls on a copy of y that the no-grad path runs.  Backward: dy = dout, dk_i = a_i dout (ewise op 1 on zeroed buffers)."""

    @staticmethod
    def forward(ctx, coefs, y, *ks):
        out = torch.zeros_like(y)
        _axpy(out, 1.0, y)
        for a, k in zip(coefs, ks):
            _axpy(out, a, k)
        ctx.coefs = coefs
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        dout = dout.contiguous()
        dks = []
        for a in ctx.coefs:
            dks.append(_axpy(torch.zeros_like(dout), a, dout))
        return (None, dout) + tuple(dks)


def _lin(y, terms, inplace, grad):
    """y + sum a k over terms [(a, k)]: in place on y (inplace), on a copy of y, or (grad) as an autograd-aware out-of-place op."""
    if grad:
        return _Comb.apply(tuple(float(a) for a, _ in terms), y, *[k.contiguous() for _, k in terms])
    out = y if inplace else y.clone()
    for a, k in terms:
        _axpy(out, a, k)
    return out


def ode_integrate(f, y0, t1, method='euler', steps=1, grad=False):
    """Fixed-grid integration of the autonomous system y' = f(y) over [0, t1] in ``steps`` equal steps (what torchdiffeq's
    fixed-grid solvers do on a uniform grid).  The reference only ever takes ONE Euler step (ode_demo.py:186-190 with t = [0, time]
    and no step_size); the multi-step / Runge-Kutta variants are provided because the north star names them and are checked
    against the CPU oracle only (the reference never runs them, torchdiffeq is not installed: parity unpinned).
      'euler'   y += h f(y)
      'rk4'     the 3/8-rule step torchdiffeq's fixed-grid 'rk4' uses (rk4_alt_step_func)
      'rk4_classic'  the classical 1/6 (k1 + 2 k2 + 2 k3 + k4) step
    ``grad``: every combination is an out-of-place autograd op with the same launches in the same order (same bits); autograd's
    discrete adjoint of this program is odestages.integrate_adjoint's."""
    h = float(t1) / steps
    y = y0.contiguous() if grad else y0.contiguous().clone()
    for _ in range(steps):
        k1 = f(y)
        if method == 'euler':
            y = _lin(y, [(h, k1)], True, grad)
            continue
        if method == 'rk4':
            k2 = f(_lin(y, [(h / 3, k1)], False, grad))
            k3 = f(_lin(y, [(h, k2), (-h / 3, k1)], False, grad))
            k4 = f(_lin(y, [(h, k1), (-h, k2), (h, k3)], False, grad))
            y = _lin(y, [(h / 8, k1), (3 * h / 8, k2), (3 * h / 8, k3), (h / 8, k4)], True, grad)
        elif method == 'rk4_classic':
            k2 = f(_lin(y, [(h / 2, k1)], False, grad))
            k3 = f(_lin(y, [(h / 2, k2)], False, grad))
            k4 = f(_lin(y, [(h, k3)], False, grad))
            y = _lin(y, [(h / 6, k1), (h / 3, k2), (h / 3, k3), (h / 6, k4)], True, grad)
        else:
            raise ValueError(f'unknown ODE method {method!r}')
    return y


class ODEG(nn.Module):
    """relu(tgt + time * DecoderStack(tgt, memory)): torchdiffeq's fixed-grid Euler on t = [0, time] is ONE step (ode_demo.py:151-166)."""

    def __init__(self, decoder_layers, nlayer, time):
        super().__init__()
        self.layers = nn.ModuleList([copy.deepcopy(decoder_layers) for _ in range(nlayer)])     # _get_clones
        self.time = float(time)
        self._trainable = False

    def forward(self, tgt, memory, tgt_mask=None, memory_mask=None, seq_mask=False, tgt_key_padding_mask=None,
                memory_key_padding_mask=None, need_weights=False, num_agent=1):
        grad = _graph(self, tgt, memory)
        with torch.set_grad_enabled(grad):
            x, ws, wc = tgt, [], []
            for m in self.layers:
                x, a, b = m(x, memory, seq_mask=seq_mask)
                ws.append(a)
                wc.append(b)
            return _euler_relu(tgt, x, self.time, grad), {'self_attn_weights': ws, 'cross_attn_weights': wc}


class ODEG_Encoder(nn.Module):
    """ode_demo.py:217-231.  ``method`` / ``steps`` default to the reference's single Euler step; see ``ode_integrate``."""

    def __init__(self, encoder_layer, nlayer, time, method='euler', steps=1):
        super().__init__()
        self.layers = nn.ModuleList([copy.deepcopy(encoder_layer) for _ in range(nlayer)])
        self.time, self.method, self.steps = float(time), method, int(steps)
        self._trainable = False

    def _rhs(self, x):
        for m in self.layers:
            x = m(x)
        return x

    def forward(self, src, mask=None, src_key_padding_mask=None, num_agent=1):
        grad = _graph(self, src)
        with torch.set_grad_enabled(grad):
            if self.method == 'euler' and self.steps == 1:
                return _euler_relu(src, self._rhs(src), self.time, grad)
            return _relu_(ode_integrate(self._rhs, src, self.time, self.method, self.steps, grad=grad), grad)


_DROPINS = (Hypattention, TransformerEncoderLayer, TransformerDecoderLayer, ODEG, ODEG_Encoder, Hyp_mhsa, MultiheadAttention)


def trainable(module, on=True):
    """Opt in (``on``) or out of autograd for every drop-in inside ``module`` (itself included); returns ``module``."""
    for m in module.modules():
        if isinstance(m, _DROPINS):
            m._trainable = bool(on)
    return module
