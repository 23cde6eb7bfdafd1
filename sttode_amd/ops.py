"""Stand-alone operators over the C ABI (op-level drop-ins for the reference's functions).

mhgsa(...)  ==  Hyp_mhsa.forward / hyp_mhsa() (hyptransformerlib.py:29-311,403-454) for embed_dim = 64, 8 heads,
no bias_kv / zero_attn / dropout (the only configuration the reference instantiates, hypertransformer.py:29,
model/STTODE.py:190-194), with the optional additive ``attn_mask`` [L, S] of :290-292 (``key_padding_mask`` is dead code in the
reference and has no counterpart here).
mha(...)    ==  transformerlib.MultiheadAttention.forward / multi_head_attention_forward() (transformerlib.py:30-292): the Euclidean
dot-product twin, same shapes, same mask.
Without a mask mhgsa runs sttode_mhgsa_attn (scores in [-pi, 0], no running maximum); a mask, and every mha call, goes through
sttode_attn_core (csrc/attention.hip: running maximum, mode 0 geodesic / mode 1 dot product).
"""
import numpy as np
import torch
from torch.autograd.function import once_differentiable

from . import capi, packing

_PK_CACHE = {}


def _pk16_cached(w):
    """Fragment-ordered copy of a weight, cached per (storage address, version).  The entry keeps ``w`` alive, so the address
    cannot be recycled for a different tensor while the entry exists."""
    key = (w.data_ptr(), w._version, tuple(w.shape), str(w.device))
    if key not in _PK_CACHE:
        if len(_PK_CACHE) > 64:
            _PK_CACHE.clear()
        _PK_CACHE[key] = (w, torch.from_numpy(packing.pk16(w.detach().cpu().numpy())).to(w.device))
    return _PK_CACHE[key][1]


_ACT = {None: 0, 'none': 0, 'relu': 1, 'tanh': 2}


def linear_cols(x, weight, bias=None, relu=False, act=None):
    """y = act(x @ weight.T + bias) on the MFMA column-chain kernel. x [cols, K] (K, N multiples of 16); act None|'relu'|'tanh'."""
    code = 1 if relu else _ACT[act]
    x = x.contiguous()
    cols, K = x.shape
    N = weight.shape[0]
    out = torch.empty(cols, N, dtype=torch.float32, device=x.device)
    capi.call('sttode_linear_cols', x, K, K, None, 0, 0, _pk16_cached(weight), bias.contiguous() if bias is not None else None,
              out, N, cols, N, code, capi.stream_ptr())
    return out


def _mhgsa_fwd(query, key, value, W, b, out_proj_weight, out_proj_bias, need_weights):
    """The forward launches: in-projections, attention core, out_proj.  Returns (out, weights | None, tensors for the backward)."""
    L, Nb, E = query.shape
    S = key.shape[0]
    q = linear_cols(query.reshape(L * Nb, E), W[:E].contiguous(), b[:E])
    k = linear_cols(key.reshape(S * Nb, E), W[E:2 * E].contiguous(), b[E:2 * E])
    v = linear_cols(value.reshape(S * Nb, E), W[2 * E:].contiguous(), b[2 * E:])
    scale = float(E // 8) ** -0.5
    if L == S:
        # scores [S, L] used untransposed (hyptransformerlib.py:261-265): rows = keys, columns = queries
        R, C, rows, cols, rs, cs = k, q, S, L, 1.0, scale
    else:
        R, C, rows, cols, rs, cs = q, k, L, S, scale, 1.0
    attn = torch.empty(rows * Nb, E, dtype=torch.float32, device=query.device)
    rowsum = torch.empty(Nb * 8 * rows, dtype=torch.float32, device=query.device) if need_weights else None
    wout = torch.empty(Nb, rows, cols, dtype=torch.float32, device=query.device) if need_weights else None
    st = Nb * E
    capi.call('sttode_mhgsa_attn', R, C, v, attn, rowsum, wout, rows, cols, Nb, st, E, st, E, st, E, st, E, rs, cs, capi.stream_ptr())
    out = linear_cols(attn, out_proj_weight, out_proj_bias).view(rows, Nb, E)
    return out, wout, (q, k, v, attn, rows, cols, rs, cs)


_SCRATCH = {}


def scratch(device):
    """Per-device workspace of the backward kernels (split weight-gradient partials, LayerNorm partials); stream-ordered reuse."""
    key = str(device)
    if key not in _SCRATCH:
        _SCRATCH[key] = torch.empty(4 << 20, dtype=torch.float32, device=device)
    return _SCRATCH[key]


def linear_bwd(dY, W, X, dX, dW, db, mask=None, accumulate=False):
    """Backward of one nn.Linear on sttode_tlinear_bwd: dX = mask(dY W) (+ dX), dW += dY^T X, db += sum dY.  2-d row-major operands."""
    cols, N = dY.shape
    K = W.shape[1]
    sc = scratch(dY.device)
    capi.call('sttode_tlinear_bwd', dY, dY.stride(0), W, W.stride(0), mask, mask.stride(0) if mask is not None else 0, dX, dX.stride(0), K,
              int(accumulate), X, X.stride(0), 1, dW, dW.stride(0), db, cols, N, K, sc, sc.numel(), capi.stream_ptr())
    return dX


class _Mhgsa(torch.autograd.Function):
    """mhgsa with a HIP backward: out_proj (sttode_tlinear_bwd), the attention core (sttode_mhgsa_attn_rc_bwd), the three in-projections
    into one [3E, E] weight gradient.  Inputs that are the same tensor (self-attention, key = value) get one accumulated gradient."""

    @staticmethod
    def forward(ctx, need_weights, slots, query, key, value, W, b, Wo, bo):
        out, wout, (q, k, v, attn, rows, cols, rs, cs) = _mhgsa_fwd(query, key, value, W, b, Wo, bo, need_weights)
        ctx.meta = (slots, rows, cols, rs, cs)
        ctx.save_for_backward(query, key, value, W, Wo, q, k, v, attn)
        if wout is not None:
            ctx.mark_non_differentiable(wout)
        return out, wout

    @staticmethod
    @once_differentiable
    def backward(ctx, dout, _dw):
        query, key, value, W, Wo, q, k, v, attn = ctx.saved_tensors
        slots, rows, cols, rs, cs = ctx.meta
        L, Nb, E = query.shape
        S = key.shape[0]
        dev = query.device
        dO = dout.reshape(rows * Nb, E).contiguous()
        dWo, dbo = torch.zeros_like(Wo), torch.zeros(E, device=dev)
        dattn = linear_bwd(dO, Wo, attn, torch.empty(rows * Nb, E, device=dev), dWo, dbo)
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        dR, dC = (dk, dq) if L == S else (dq, dk)
        R, C = (k, q) if L == S else (q, k)
        st = Nb * E
        capi.call('sttode_mhgsa_attn_rc_bwd', R, C, v, dattn, dR, dC, dv, rows, cols, Nb, st, E, st, E, st, E, st, E, rs, cs, capi.stream_ptr())
        dW, db = torch.zeros_like(W), torch.zeros(3 * E, device=dev)
        xs = (query, key, value)
        dx = [None, None, None]
        for i, (d, x) in enumerate(zip((dq, dk, dv), xs)):
            s = slots[i]                                             # index of the first input that is the same tensor as input i
            first = dx[s] is None
            if first:
                dx[s] = torch.empty(x.shape[0] * Nb, E, device=dev)
            linear_bwd(d, W[i * E:(i + 1) * E], x.reshape(-1, E), dx[s], dW[i * E:(i + 1) * E], db[i * E:(i + 1) * E], accumulate=not first)
        dx = [None if d is None else d.view(xs[i].shape) for i, d in enumerate(dx)]
        return None, None, dx[0], dx[1], dx[2], dW, db, dWo, dbo


def _check(name, query, key, value, num_heads, attn_mask):
    if query.device.type != 'cuda':
        raise capi.SttodeError(f'{name} runs only on a HIP device (no CPU fallback)')
    L, Nb, E = query.shape
    if E != 64 or num_heads != 8:
        raise NotImplementedError(f'{name} kernel is built for embed_dim=64, num_heads=8')
    if key.shape != value.shape or key.shape[1] != Nb:
        raise ValueError('key/value shape mismatch')
    if attn_mask is not None:
        if (not isinstance(attn_mask, torch.Tensor) or attn_mask.dtype != torch.float32 or tuple(attn_mask.shape) != (L, key.shape[0])
                or attn_mask.device != query.device):
            raise ValueError(f'{name}: attn_mask must be a float32 [L, S] = [{L}, {key.shape[0]}] tensor on the inputs\' device')
        if attn_mask.requires_grad:
            raise ValueError(f'{name}: no gradient with respect to attn_mask (detach it)')


def _attn_fwd(mode, mask, query, key, value, W, b, out_proj_weight, out_proj_bias, need_weights):
    """In-projections, sttode_attn_core (mode 0 geodesic | 1 dot product, optional mask [rows, cols]), out_proj.  Mode 0 keeps mhgsa's
    orientation (L == S: rows = keys); mode 1 has rows = queries always (transformerlib.py:251), q scaled by head_dim ** -0.5."""
    L, Nb, E = query.shape
    S = key.shape[0]
    q = linear_cols(query.reshape(L * Nb, E), W[:E].contiguous(), b[:E])
    k = linear_cols(key.reshape(S * Nb, E), W[E:2 * E].contiguous(), b[E:2 * E])
    v = linear_cols(value.reshape(S * Nb, E), W[2 * E:].contiguous(), b[2 * E:])
    scale = float(E // 8) ** -0.5
    if mode == 0 and L == S:
        R, C, rows, cols, rs, cs = k, q, S, L, 1.0, scale
    else:
        R, C, rows, cols, rs, cs = q, k, L, S, scale, 1.0
    dev = query.device
    if mask is not None:
        mask = mask.contiguous()
    attn = torch.empty(rows * Nb, E, dtype=torch.float32, device=dev)
    wmax = torch.empty(Nb * 8 * rows, dtype=torch.float32, device=dev) if need_weights else None
    wsum = torch.empty(Nb * 8 * rows, dtype=torch.float32, device=dev) if need_weights else None
    wout = torch.empty(Nb, rows, cols, dtype=torch.float32, device=dev) if need_weights else None
    st = Nb * E
    capi.call('sttode_attn_core', R, C, v, mask, cols if mask is not None else 0, attn, wmax, wsum, wout, rows, cols, Nb, st, E, st, E, st, E,
              st, E, rs, cs, mode, capi.stream_ptr())
    out = linear_cols(attn, out_proj_weight, out_proj_bias).view(rows, Nb, E)
    return out, wout, (q, k, v, attn, mask, rows, cols, rs, cs)


class _Attn(torch.autograd.Function):
    """_attn_fwd with a HIP backward: _Mhgsa's plan with sttode_attn_core_bwd for the core.  The mask is a constant."""

    @staticmethod
    def forward(ctx, mode, mask, need_weights, slots, query, key, value, W, b, Wo, bo):
        out, wout, (q, k, v, attn, mask, rows, cols, rs, cs) = _attn_fwd(mode, mask, query, key, value, W, b, Wo, bo, need_weights)
        ctx.meta = (mode, slots, rows, cols, rs, cs)
        ctx.save_for_backward(query, key, value, W, Wo, q, k, v, attn, mask)      # mask: a constant, or None
        if wout is not None:
            ctx.mark_non_differentiable(wout)
        return out, wout

    @staticmethod
    @once_differentiable
    def backward(ctx, dout, _dw):
        query, key, value, W, Wo, q, k, v, attn, mask = ctx.saved_tensors
        mode, slots, rows, cols, rs, cs = ctx.meta
        L, Nb, E = query.shape
        dev = query.device
        dO = dout.reshape(rows * Nb, E).contiguous()
        dWo, dbo = torch.zeros_like(Wo), torch.zeros(E, device=dev)
        dattn = linear_bwd(dO, Wo, attn, torch.empty(rows * Nb, E, device=dev), dWo, dbo)
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        swapped = mode == 0 and L == key.shape[0]
        dR, dC = (dk, dq) if swapped else (dq, dk)
        R, C = (k, q) if swapped else (q, k)
        st = Nb * E
        capi.call('sttode_attn_core_bwd', R, C, v, mask, cols if mask is not None else 0, dattn, dR, dC, dv, rows, cols, Nb, st, E, st, E,
                  st, E, st, E, rs, cs, mode, capi.stream_ptr())
        dW, db = torch.zeros_like(W), torch.zeros(3 * E, device=dev)
        xs = (query, key, value)
        dx = [None, None, None]
        for i, (d, x) in enumerate(zip((dq, dk, dv), xs)):
            s = slots[i]
            first = dx[s] is None
            if first:
                dx[s] = torch.empty(x.shape[0] * Nb, E, device=dev)
            linear_bwd(d, W[i * E:(i + 1) * E], x.reshape(-1, E), dx[s], dW[i * E:(i + 1) * E], db[i * E:(i + 1) * E], accumulate=not first)
        dx = [None if d is None else d.view(xs[i].shape) for i, d in enumerate(dx)]
        return None, None, None, None, dx[0], dx[1], dx[2], dW, db, dWo, dbo


def _attn(mode, attn_mask, need_weights, differentiable, args):
    if differentiable and torch.is_grad_enabled() and any(t.requires_grad for t in args):
        xs = args[:3]
        slots = tuple(next(j for j in range(3) if xs[j] is xs[i]) for i in range(3))
        return _Attn.apply(mode, attn_mask, need_weights, slots, *args)
    with torch.no_grad():
        out, wout, _ = _attn_fwd(mode, attn_mask, *args, need_weights)
    return out, wout


def mha(query, key, value, in_proj_weight, in_proj_bias, out_proj_weight, out_proj_bias, num_heads=8, need_weights=False, attn_mask=None,
        differentiable=False):
    """Multi-head dot-product attention, the Euclidean twin of ``mhgsa`` (transformerlib.py:30-292).  query [L,Nb,64], key/value [S,Nb,64]
    -> (out [L,Nb,64], weights [Nb,L,S] | None); rows follow the queries, q carries head_dim ** -0.5.  ``attn_mask``: float32 [L, S], added
    to the scores before the softmax (-inf allowed; a row masked everywhere comes out NaN, as torch's softmax leaves it).
    ``differentiable`` as in ``mhgsa``; the mask is a constant and must not require grad."""
    _check('mha', query, key, value, num_heads, attn_mask)
    return _attn(1, attn_mask, need_weights, differentiable,
                 (query, key, value, in_proj_weight, in_proj_bias, out_proj_weight, out_proj_bias))


def mhgsa(query, key, value, in_proj_weight, in_proj_bias, out_proj_weight, out_proj_bias, num_heads=8, need_weights=False,
          differentiable=False, attn_mask=None):
    """Multi-head geodesic self/cross attention. query [L,Nb,64], key/value [S,Nb,64] -> (out [L,Nb,64], weights [Nb,L,S] | None).
    ``differentiable``: with grad mode on and an input or parameter that requires grad, the output carries a graph whose backward runs on
    HIP kernels (the weights are not differentiable); otherwise forward values only, as by default.
    ``attn_mask``: float32 [L, S], added to the geodesic scores before the softmax (hyptransformerlib.py:290-292).  With L == S the
    reference uses the scores untransposed (rows = keys, columns = queries) and adds mask element [i][j] to score element [i][j] of that
    matrix as it stands; so does this.  -inf is allowed; a row masked everywhere comes out NaN.  The mask must not require grad."""
    _check('mhgsa', query, key, value, num_heads, attn_mask)
    args = (query, key, value, in_proj_weight, in_proj_bias, out_proj_weight, out_proj_bias)
    if attn_mask is not None:
        return _attn(0, attn_mask, need_weights, differentiable, args)
    if differentiable and torch.is_grad_enabled() and any(t.requires_grad for t in args):
        xs = (query, key, value)
        slots = tuple(next(j for j in range(3) if xs[j] is xs[i]) for i in range(3))
        return _Mhgsa.apply(need_weights, slots, *args)
    with torch.no_grad():
        out, wout, _ = _mhgsa_fwd(*args, need_weights)
    return out, wout
