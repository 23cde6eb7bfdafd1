"""Forward + backward rate of the op-level drop-ins with autograd on (hypertransformer.trainable): TransformerDecoderLayer at tgt 12 /
memory 8 steps x 32 agents x 20 samples, and ODEG_Encoder('rk4', 4) at 12 steps x 32 x 20.  For comparison: float32 torch autograd of
the oracle restatement (oracle/sttode_ref.py, profile-only, never on the product path) on the same GPU.  ms per forward + backward
(loss = sum(out * G)), eager, median of --reps after --warmup.  Prints one JSON line per case.
Usage: python profiles/exp_stack_train_rate.py [--reps 30] [--warmup 5] [--only decoder|encoder] [--once]   (--once: warm-up, an idle gap, then one step, for a trace)"""
import argparse
import copy
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.sttode_ref import DecoderLayer, EncoderLayer, ode_integrate_ref   # noqa: E402
from sttode_amd import hypertransformer as ht                                  # noqa: E402
from sttode_amd.weights import make_decoder_layer_weights, to_torch_state_dict  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--reps', type=int, default=30)
ap.add_argument('--warmup', type=int, default=5)
ap.add_argument('--only', choices=('decoder', 'encoder'))
ap.add_argument('--once', action='store_true')
a = ap.parse_args()
dev = torch.device('cuda')
rng = np.random.default_rng(0)
sd = to_torch_state_dict(make_decoder_layer_weights(61, d=64, ff=256))
esd = {k: (v * 0.3 if k.endswith('weight') and 'norm' not in k else v) for k, v in sd.items()
       if not k.startswith('cross_attn') and not k.startswith('norm3')}


def rand(*s):
    return torch.from_numpy(rng.standard_normal(s).astype(np.float32)).to(dev)


def timed(step):
    for _ in range(a.warmup):
        step()
    torch.cuda.synchronize()
    if a.once:                      # one more step after an idle gap: a trace summary takes the dispatches after the largest gap
        time.sleep(0.2)
        step()
        torch.cuda.synchronize()
        return float('nan')
    ts = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        step()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def rate(name, hip_mod, ref_mod, run_h, run_r, inputs, G):
    xs = [x.clone().requires_grad_(True) for x in inputs]

    def step(mod, run):
        def f():
            mod.zero_grad()
            for x in xs:
                x.grad = None
            (run(mod, *xs) * G).sum().backward()
        return f
    out = {'case': name, 'hip_ms': timed(step(hip_mod, run_h))}
    if not a.once:
        out['torch_oracle_fp32_ms'] = timed(step(ref_mod, run_r))
        out['hip_over_torch'] = out['hip_ms'] / out['torch_oracle_fp32_ms']
    print(json.dumps(out), flush=True)


if a.only in (None, 'decoder'):
    m = ht.trainable(ht.TransformerDecoderLayer(64, 8, 256))
    m.load_state_dict(sd, strict=True)
    o = DecoderLayer(64, 8, 256)
    o.load_state_dict(sd, strict=True)
    tgt, mem = rand(12, 32, 20, 64), rand(8, 32, 20, 64)
    rate('TransformerDecoderLayer tgt 12 / memory 8 x 32 x 20', m.to(dev), o.to(dev), lambda mm, t, k: mm(t, k)[0],
         lambda mm, t, k: mm(t, k)[0], [tgt, mem], rand(12, 32, 20, 64))
if a.only in (None, 'encoder'):
    layer = ht.TransformerEncoderLayer(64, 8, 256)
    layer.load_state_dict(esd, strict=True)
    enc = ht.trainable(ht.ODEG_Encoder(layer, 1, 0.9, method='rk4', steps=4)).to(dev)
    o = EncoderLayer(64, 8, 256)
    o.load_state_dict(esd, strict=True)
    o = copy.deepcopy(o).to(dev)
    rate("ODEG_Encoder('rk4', 4) 12 x 32 x 20", enc, o, lambda mm, x: mm(x), lambda mm, x: torch.relu(ode_integrate_ref(mm, x, 0.9, 'rk4', 4)),
         [rand(12, 32, 20, 64)], rand(12, 32, 20, 64))
