#!/usr/bin/env python3
"""Generate tests/golden/attention.npz: outputs, head-averaged weights and gradients of the reference's two stand-alone attention modules
(hyptransformerlib.Hyp_mhsa, transformerlib.MultiheadAttention) with and without ``attn_mask``, and of the reference's transformer layers
with the Euclidean attention swapped in, by IMPORTING THE REFERENCE under make_golden.install_shims() (run in the authoring container
only, like make_stack_grads_golden.py):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_attention_golden.py

Data only, and small: inputs and the loss weight G are drawn from the seeds and shapes the file records (make_stack_grads_golden.seeded),
masks are stored whole, weight-matrix gradients as digests (make_stack_grads_golden.digest), vectors whole.  Parameters are
sttode_amd.weights.make_decoder_layer_weights(61)'s cross_attn.temporal_attention_before.* (modules) / the whole layer (stack cases; the
encoder layer as in make_stack_grads_golden.encoder_weights).

Module cases, '<mod>_<form>_<mask>' with mod = hyp | euc; loss = sum(out * G):
  form  self   query = key = value                      [7,3,64]
        kv     key is value, another length             query [6,3,64], memory [9,3,64]
        eq     key is value, equal length, other source query [7,3,64], memory [7,3,64]
        lead   as kv with S = 129                       query [5,2,64], memory [129,2,64]
  mask  none | rand (finite, seeded) | causal (-inf above the diagonal) | lead (rows 1 and 3: the first 128 columns -inf)
Forward-only cases: '<mod>_nanrow' (self, [6,2,64]; row 2 of the mask -inf everywhere: '_nan' records where the output is NaN) and
'euc_overflow' (kv shapes, inputs x 30: exp(score) overflows fp32 without a running maximum; '_maxscore' records the largest score).
Stack cases: 'edec' (TransformerDecoderLayer, tgt [6,5,2,64], memory [9,5,2,64]) and 'eenc' (TransformerEncoderLayer, src [5,7,1,64]) with
every temporal_attention_before replaced by a transformerlib.MultiheadAttention holding the same parameters.
'<mod>_sd_names' / '<mod>_sd_shapes': each module's state_dict."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402  (puts the repository root on sys.path)
from make_stack_grads_golden import DIGEST_MIN, decoder_weights, digest, encoder_weights, seeded  # noqa: E402

PREFIX = 'cross_attn.temporal_attention_before.'
FORMS = {'self': [(7, 3, 64)], 'kv': [(6, 3, 64), (9, 3, 64)], 'eq': [(7, 3, 64), (7, 3, 64)], 'lead': [(5, 2, 64), (129, 2, 64)]}
CASES = [('self', 'none'), ('self', 'rand'), ('self', 'causal'), ('kv', 'none'), ('kv', 'rand'), ('kv', 'causal'), ('eq', 'rand'),
         ('eq', 'causal'), ('lead', 'lead')]


def attn_weights():
    return {k[len(PREFIX):]: v for k, v in decoder_weights().items() if k.startswith(PREFIX)}


def make_mask(kind, L, S, seed):
    if kind == 'none':
        return None
    if kind == 'rand':
        return seeded(seed + 50, (L, S))
    m = np.zeros((L, S), np.float32)
    if kind == 'causal':
        for i in range(L):
            m[i, i + 1:] = -np.inf
    elif kind == 'lead':
        m[1, :128] = m[3, :128] = -np.inf
    return m


def store_grads(out, tag, module, xs):
    for i, x in enumerate(xs):
        out[f'{tag}_dinput::{i}'] = x.grad.numpy().copy()
    for name, p in module.named_parameters():
        g = p.grad.numpy()
        if g.size > DIGEST_MIN:
            out[f'{tag}_gradd::{name}'] = digest(g)
        else:
            out[f'{tag}_grad::{name}'] = g.copy()


def call(module, xs, mask):
    q = xs[0]
    kv = xs[0] if len(xs) == 1 else xs[1]
    return module(q, kv, kv, attn_mask=None if mask is None else torch.from_numpy(mask.copy()))


def record_module(out, tag, module, shapes, kind, seed):
    xs = [torch.from_numpy(seeded(seed + 1 + i, sh)).requires_grad_(True) for i, sh in enumerate(shapes)]
    mask = make_mask(kind, shapes[0][0], shapes[-1][0], seed)
    module.zero_grad()
    y, w = call(module, xs, mask)
    (y * torch.from_numpy(seeded(seed, y.shape))).sum().backward()
    out[f'{tag}_seed'] = np.array(seed)
    out[f'{tag}_shapes'] = np.array(shapes, np.int64)
    if mask is not None:
        out[f'{tag}_mask'] = mask
    out[f'{tag}_out'] = y.detach().numpy().copy()
    out[f'{tag}_w'] = w.detach().numpy().copy()
    store_grads(out, tag, module, xs)


def record_forward(out, tag, module, shapes, mask, seed, scale=1.0):
    xs = [torch.from_numpy(seeded(seed + 1 + i, sh) * np.float32(scale)) for i, sh in enumerate(shapes)]
    with torch.no_grad():
        y, w = call(module, xs, mask)
    out[f'{tag}_seed'] = np.array(seed)
    out[f'{tag}_shapes'] = np.array(shapes, np.int64)
    out[f'{tag}_scale'] = np.array(scale, np.float32)
    if mask is not None:
        out[f'{tag}_mask'] = mask
    out[f'{tag}_out'] = y.numpy().copy()
    out[f'{tag}_w'] = w.numpy().copy()
    return xs, y


def record_stack(out, tag, layer, shapes, run, seed):
    xs = [torch.from_numpy(seeded(seed + 1 + i, sh)).requires_grad_(True) for i, sh in enumerate(shapes)]
    layer.zero_grad()
    y = run(*xs)
    (y * torch.from_numpy(seeded(seed, y.shape))).sum().backward()
    out[f'{tag}_seed'] = np.array(seed)
    out[f'{tag}_shapes'] = np.array(shapes, np.int64)
    out[f'{tag}_out'] = y.detach().numpy().copy()
    store_grads(out, tag, layer, xs)


def swap_in_euclidean(layer, MultiheadAttention):
    """Every Hypattention's temporal_attention_before -> a transformerlib.MultiheadAttention with the same parameters."""
    for m in list(layer.modules()):
        if hasattr(m, 'temporal_attention_before'):
            e = MultiheadAttention(64, 8, dropout=0.0)
            e.load_state_dict(m.temporal_attention_before.state_dict(), strict=True)
            m.temporal_attention_before = e
    return layer


def main():
    make_golden.install_shims()
    from hypertransformer import TransformerDecoderLayer, TransformerEncoderLayer
    from hyptransformerlib import Hyp_mhsa
    from transformerlib import MultiheadAttention
    out = {}
    mods = {'hyp': Hyp_mhsa(64, 8).eval(), 'euc': MultiheadAttention(64, 8).eval()}
    seed = 1000
    for mod, m in mods.items():
        m.load_state_dict(attn_weights(), strict=True)
        sd = m.state_dict()
        out[f'{mod}_sd_names'] = np.array(list(sd))
        out[f'{mod}_sd_shapes'] = np.array([list(v.shape) + [0] * (2 - v.dim()) for v in sd.values()], np.int64)
        for form, kind in CASES:
            seed += 100
            record_module(out, f'{mod}_{form}_{kind}', m, FORMS[form], kind, seed)
        seed += 100
        mask = np.zeros((6, 6), np.float32)
        mask[2, :] = -np.inf
        _, y = record_forward(out, f'{mod}_nanrow', m, [(6, 2, 64)], mask, seed)
        nan = torch.isnan(y).numpy()
        assert nan.any() and not nan.all()
        out[f'{mod}_nanrow_nan'] = nan
    seed += 100
    m = mods['euc']
    xs, y = record_forward(out, 'euc_overflow', m, FORMS['kv'], None, seed, scale=30.0)
    W, b = m.in_proj_weight.detach(), m.in_proj_bias.detach()
    q = (xs[0] @ W[:64].T + b[:64]).view(6, 3, 8, 8) * 8 ** -0.5
    k = (xs[1] @ W[64:128].T + b[64:128]).view(9, 3, 8, 8)
    smax = float(torch.einsum('lbhd,sbhd->bhls', q, k).max())
    assert smax > 100 and torch.isfinite(y).all(), smax                     # exp(89) already overflows fp32
    out['euc_overflow_maxscore'] = np.array(smax)

    dec = TransformerDecoderLayer(64, 8, 256, dropout=0.0).eval()
    dec.load_state_dict(decoder_weights(), strict=True)
    swap_in_euclidean(dec, MultiheadAttention)
    record_stack(out, 'edec', dec, [(6, 5, 2, 64), (9, 5, 2, 64)], lambda t, mm: dec(t, mm, seq_mask=True)[0], 5000)
    enc = TransformerEncoderLayer(64, 8, 256, dropout=0.0).eval()
    enc.load_state_dict(encoder_weights(), strict=True)
    swap_in_euclidean(enc, MultiheadAttention)
    record_stack(out, 'eenc', enc, [(5, 7, 1, 64)], lambda s: enc(s), 5100)
    path = os.path.join(HERE, 'attention.npz')
    np.savez_compressed(path, **out)
    print('attention.npz bytes:', os.path.getsize(path), len(out), 'arrays')


if __name__ == '__main__':
    main()
