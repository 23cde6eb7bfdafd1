#!/usr/bin/env python3
"""Generate tests/golden/stack_grads.npz: outputs and gradients of the reference's geodesic transformer blocks, by IMPORTING THE
REFERENCE under make_golden.install_shims() (run in the authoring container only, like make_golden.py):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_stack_grads_golden.py

For a loss sum(out * G) with a seeded G, each case stores the output, the gradient of every input and of every parameter (keyed by the
drop-ins' parameter names).  Data only, and small: the inputs and G are not stored but drawn from the seeds and shapes the file records
(``seeded``), and a weight-matrix gradient (more than DIGEST_MIN entries) is kept as a digest ([L2 norm, max |g|] + DIGEST_N entries at
evenly spaced flat positions, ``digest``) under '<tag>_gradd::<name>'; vectors (biases, LayerNorm parameters) are kept whole under
'<tag>_grad::<name>'.  Weights are NOT stored: the decoder layer loads sttode_amd.weights.make_decoder_layer_weights(61) with
strict=True (as make_golden.decoder_stack_cases does); the encoder layer the same weights without cross_attn.* / norm3.*, their linear
weights scaled by 0.3 (as tests/test_gpu_parity.py's ODEG_Encoder test does).

Cases (tag: what):
  dec    TransformerDecoderLayer, tgt [6,5,2,64], memory [9,5,2,64] (the decoder_stack shapes: cross-attention L != S)
  deceq  TransformerDecoderLayer, tgt and memory both [7,3,2,64] (equal-length cross-attention from distinct sources)
  odeg   ODEG(layer, 2, 3) at the dec shapes
  enc    ODEG_Encoder(encoder layer, 1, 0.9): the reference's one Euler step, src [5,7,1,64]
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402  (puts the repository root on sys.path)


def decoder_weights():
    from sttode_amd.weights import make_decoder_layer_weights, to_torch_state_dict
    return to_torch_state_dict(make_decoder_layer_weights(61, d=64, ff=256))


def encoder_weights():
    sd = {k: v for k, v in decoder_weights().items() if not k.startswith('cross_attn') and not k.startswith('norm3')}
    return {k: (v * 0.3 if k.endswith('weight') and 'norm' not in k else v) for k, v in sd.items()}


def local_name(name):
    """Reference parameter name -> the drop-ins' name (ODEG / ODEG_Encoder keep their clones under odeblock.odefunc.layers)."""
    return name.replace('odeblock.odefunc.', '')


DIGEST_MIN, DIGEST_N = 512, 64


def seeded(seed, shape):
    """An input / loss weight of a case: standard normal float32 from numpy's default_rng(seed)."""
    return np.random.default_rng(int(seed)).standard_normal(tuple(int(d) for d in shape)).astype(np.float32)


def digest(g):
    """[L2 norm, max |g|, DIGEST_N entries at evenly spaced flat positions] of a gradient, in float64."""
    f = np.asarray(g, np.float64).ravel()
    idx = np.linspace(0, f.size - 1, DIGEST_N).astype(np.int64)
    return np.concatenate([[np.linalg.norm(f), np.abs(f).max()], f[idx]])


def record(out, tag, module, shapes, run, seed):
    """Inputs i = seeded(seed + 1 + i, shapes[i]), G = seeded(seed, out.shape); loss = sum(run(*inputs) * G).  Stores '<tag>_seed',
    '<tag>_shapes', '_out', '_dinput::<i>', '_grad::<param>' (vectors) / '_gradd::<param>' (digests of matrices)."""
    inputs = [seeded(seed + 1 + i, sh) for i, sh in enumerate(shapes)]
    xs = [torch.from_numpy(x).requires_grad_(True) for x in inputs]
    module.zero_grad()
    y = run(*xs)
    (y * torch.from_numpy(seeded(seed, y.shape))).sum().backward()
    out[f'{tag}_seed'] = np.array(seed)
    out[f'{tag}_shapes'] = np.array(shapes, np.int64)
    out[f'{tag}_out'] = y.detach().numpy().copy()
    for i in range(len(inputs)):
        out[f'{tag}_dinput::{i}'] = xs[i].grad.numpy().copy()
    for name, p in module.named_parameters():
        g = p.grad.numpy()
        if g.size > DIGEST_MIN:
            out[f'{tag}_gradd::{local_name(name)}'] = digest(g)
        else:
            out[f'{tag}_grad::{local_name(name)}'] = g.copy()


def main():
    make_golden.install_shims()
    from hypertransformer import TransformerDecoderLayer, TransformerEncoderLayer
    from ode_demo import ODEG, ODEG_Encoder
    out = {}
    layer = TransformerDecoderLayer(64, 8, 256, dropout=0.0).eval()
    layer.load_state_dict(decoder_weights(), strict=True)
    record(out, 'dec', layer, [(6, 5, 2, 64), (9, 5, 2, 64)], lambda t, m: layer(t, m, seq_mask=True)[0], 100)
    record(out, 'deceq', layer, [(7, 3, 2, 64), (7, 3, 2, 64)], lambda t, m: layer(t, m, seq_mask=True)[0], 200)
    ode = ODEG(layer, 2, 3).eval()                          # _get_clones: both layers start as copies of ``layer``
    record(out, 'odeg', ode, [(6, 5, 2, 64), (9, 5, 2, 64)], lambda t, m: ode(t, m, seq_mask=True)[0], 300)
    enc_layer = TransformerEncoderLayer(64, 8, 256, dropout=0.0).eval()
    enc_layer.load_state_dict(encoder_weights(), strict=True)
    enc = ODEG_Encoder(enc_layer, 1, 0.9).eval()
    record(out, 'enc', enc, [(5, 7, 1, 64)], lambda s: enc(s), 400)
    path = os.path.join(HERE, 'stack_grads.npz')
    np.savez_compressed(path, **out)
    print('stack_grads.npz bytes:', os.path.getsize(path), len(out), 'arrays')


if __name__ == '__main__':
    main()
