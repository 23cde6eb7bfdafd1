"""Cost of global-norm clipping and the non-finite guard in the one-launch Adam, on the model's parameters with random gradients laid out
as views of one flat buffer (the training engine's layout).  Device-event time per optimizer step, the forms alternating in one process:

    plain      sttode_amd.optim.Adam.step()
    guarded    Adam(max_grad_norm=c, skip_nonfinite=True).step()
    torch+     torch.nn.utils.clip_grad_norm_(params, c) followed by the plain step()
    ours+      sttode_amd.optim.clip_grad_norm_(params, c) followed by the plain step()
    copy       nothing: every form's step is preceded by a copy of the step's gradients into the flat buffer (the stand-alone clips scale
               them in place, and a second clip of clipped gradients would have nothing to do); this row is that copy alone, to subtract

    python profiles/grad_clip/measure.py [--steps 400] [--rounds 7] > profiles/grad_clip/rates.txt

Wall time per step (host + device, the stream drained once at the end of a batch of steps) is printed beside it: torch's clip costs host
time as well."""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=400)
    ap.add_argument('--rounds', type=int, default=7)
    a = ap.parse_args()
    from helpers import make_args
    from sttode_amd import STTODENet, optim
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    base = list(STTODENet(make_args('eth', 8, 12), dev).parameters())
    total = sum((p.numel() + 3) // 4 * 4 for p in base)

    def setup(**kw):
        ps = [torch.nn.Parameter(p.detach().clone()) for p in base]
        flat, off = torch.randn(total, device=dev), 0
        for p in ps:
            p.grad = flat[off: off + p.numel()].view(p.shape)
            off += (p.numel() + 3) // 4 * 4
        return ps, flat, optim.Adam(ps, lr=1e-4, **kw)
    c = 0.5 * float(torch.linalg.vector_norm(setup()[1]))
    forms = {}
    ps, flat, opt = setup()
    forms['plain'] = (flat, opt.step)
    ps, flat, opt = setup(max_grad_norm=c, skip_nonfinite=True)
    forms['guarded'] = (flat, opt.step)

    def with_clip(clip):
        ps, flat, opt = setup()

        def step():
            clip(ps, c)
            opt.step()
        return flat, step
    forms['torch+'] = with_clip(torch.nn.utils.clip_grad_norm_)
    forms['ours+'] = with_clip(optim.clip_grad_norm_)
    forms['copy'] = (setup()[1], lambda: None)
    keep = {k: f[0].clone() for k, f in forms.items()}
    dev_us, wall_us = {k: [] for k in forms}, {k: [] for k in forms}
    for r in range(a.rounds + 1):                                   # round 0 warms every form up
        for k, (flat, step) in forms.items():
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            for _ in range(a.steps):
                flat.copy_(keep[k])
                step()
            e1.record()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            if r:
                dev_us[k].append(e0.elapsed_time(e1) * 1e3 / a.steps)
                wall_us[k].append((t1 - t0) * 1e6 / a.steps)
    print(f'{torch.cuda.get_device_name(0)}; {len(base)} parameters, {sum(p.numel() for p in base)} elements; {a.steps} steps per sample, '
          f'{a.rounds} samples per form, forms alternating; us per optimizer step: median (min .. max)')
    for k in forms:
        d, w = dev_us[k], wall_us[k]
        print(f'{k:8s} events {statistics.median(d):8.1f} ({min(d):.1f} .. {max(d):.1f})   wall {statistics.median(w):8.1f} ({min(w):.1f} .. {max(w):.1f})')


if __name__ == '__main__':
    main()
