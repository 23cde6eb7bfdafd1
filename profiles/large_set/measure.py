"""Scores of a whole oversampled set on the MI355X: 512 ETH-shaped scenes (the benchmark's headline batch), M sampled
futures per agent in the round-major buffer [R, n, 20, 12, 2] that inference_reduced fills (here: the scenes' futures plus seeded noise --
the kernels' time does not depend on the values).  In ONE process, by HIP events after a warm-up, the shader clock (sttode_clock_probe) read
on both sides of every measurement:

  select    metrics.large_select with ks = (1, 5, 10, 20) and the scenes as segments (best-of-M, prefix minima, joint best-of-M)
  kde       metrics.large_kde_nll
  spread    metrics.large_spread with the ground truth (pair means, DLow value, energy scores)
  reduce    metrics.reduce_samples to K = 20, ten iterations, on the same buffer: what a raw pass adds to an eval_scenes_reduced call

at M = 400 (20 rounds) and M = 2000 (100 rounds); the spread also at M = 4096 on the first `--big-agents` agents.  Beside each entry the
same quantity composed from torch ops on the device (float32 norms / min / argmin and index_add for the selection; float64 torch.cdist per
frame for the spread; a batched covariance and logsumexp in float64 for the KDE).  The torch spread needs M^2 doubles per agent and frame
set, so it runs over the first `--yard-agents` agents in blocks, and the kernel is timed on those agents as well.

    python profiles/large_set/measure.py [--out FILE] [--passes 3] [--scenes 512] [--yard-agents 256] [--big-agents 300]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from sttode_amd import capi, metrics, scenes  # noqa: E402


def clock_ghz():
    clk = torch.zeros(2, dtype=torch.int64, device='cuda:0')
    capi.call('sttode_clock_probe', clk, capi.stream_ptr())
    c = clk.tolist()
    return c[0] / (10.0 * c[1]) if c[1] else None


def timed(fn, passes, warm=1):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    c0 = clock_ghz()
    ms = []
    for _ in range(passes):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return {'median_ms': float(np.median(ms)), 'min_ms': float(min(ms)), 'max_ms': float(max(ms)), 'clock_ghz': [c0, clock_ghz()]}


def torch_select(buf, gt, sp, seg_of, ks):
    R, n, K_in = buf.shape[:3]
    d = (buf - gt[None, :, None]).norm(dim=-1)                                        # [R, n, K_in, Tf]
    ade = d.mean(dim=-1).permute(1, 0, 2).reshape(n, R * K_in)
    fde = d[..., -1].permute(1, 0, 2).reshape(n, R * K_in)
    out = [ade.min(dim=1), fde.min(dim=1)] + [ade[:, :k].min(dim=1).values for k in ks] + [fde[:, :k].min(dim=1).values for k in ks]
    S = sp.numel() - 1
    cnt = (sp[1:] - sp[:-1]).double().unsqueeze(1)
    for v in (ade, fde):
        out.append((torch.zeros(S, v.shape[1], dtype=torch.float64, device=v.device).index_add_(0, seg_of, v.double()) / cnt).min(dim=1))
    return out


def torch_kde(buf, gt, block=1024):
    R, n, K_in, Tf = buf.shape[:4]
    M = R * K_in
    f2 = float(M) ** (-1.0 / 3.0)
    out = []
    for a0 in range(0, n, block):
        X = buf[:, a0:a0 + block].permute(1, 0, 2, 3, 4).reshape(-1, M, Tf, 2).double()
        d = X - X.mean(dim=1, keepdim=True)
        c00, c01, c11 = (d[..., 0] ** 2).sum(1) / (M - 1), (d[..., 0] * d[..., 1]).sum(1) / (M - 1), (d[..., 1] ** 2).sum(1) / (M - 1)
        det = c00 * c11 - c01 * c01
        g = gt[a0:a0 + block].double().unsqueeze(1) - X
        e = -0.5 * (c11.unsqueeze(1) * g[..., 0] ** 2 - 2.0 * c01.unsqueeze(1) * g[..., 0] * g[..., 1] + c00.unsqueeze(1) * g[..., 1] ** 2) / (
            f2 * det).unsqueeze(1)
        lp = torch.logsumexp(e, dim=1) - np.log(M) - 0.5 * torch.log((2.0 * np.pi * f2) ** 2 * det)
        out.append(-lp.clamp(min=-20.0).mean(dim=1))
    return torch.cat(out)


def torch_spread(buf, gt, div_scale, block):
    R, n, K_in, Tf = buf.shape[:4]
    M = R * K_in
    iu = torch.triu_indices(M, M, 1, device=buf.device)
    out = []
    for a0 in range(0, n, block):
        X = buf[:, a0:a0 + block].permute(1, 0, 2, 3, 4).reshape(-1, M, Tf, 2).double()
        t = torch.cdist(X.reshape(-1, M, Tf * 2), X.reshape(-1, M, Tf * 2))[:, iu[0], iu[1]]
        per = torch.zeros_like(t)
        for f in range(Tf):
            last = torch.cdist(X[:, :, f], X[:, :, f])[:, iu[0], iu[1]]
            per += last
        G = (X - gt[a0:a0 + block].double().unsqueeze(1)).norm(dim=-1)
        c = (M - 1) / (2.0 * M)
        pade, fpd = (per / Tf).mean(dim=1), last.mean(dim=1)
        out.append(torch.stack([t.mean(dim=1), fpd, pade, torch.exp(-t * t / div_scale).mean(dim=1), G.mean(dim=-1).mean(dim=1) - c * pade,
                                G[..., -1].mean(dim=1) - c * fpd], dim=1))
    return torch.cat(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--passes', type=int, default=3)
    ap.add_argument('--scenes', type=int, default=512)
    ap.add_argument('--yard-agents', type=int, default=256)
    ap.add_argument('--big-agents', type=int, default=300)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('profiles/large_set/measure.py needs the GPU: nothing here is measured without one')
    dev = torch.device('cuda:0')
    sb = scenes.make_scene_batch(range(a.scenes), 'eth')
    n, K_in, Tf = sb.n_agents, 20, sb.future.shape[1]
    gt = torch.from_numpy(sb.future).to(dev)
    sp = torch.as_tensor(sb.scene_ptr, dtype=torch.int32).to(dev)
    seg_of = torch.repeat_interleave(torch.arange(sp.numel() - 1, device=dev), (sp[1:] - sp[:-1]).long())
    ks, div = (1, 5, 10, 20), 2.0
    gen = torch.Generator(device=dev).manual_seed(20261021)
    res = {'scenes': a.scenes, 'agents': n, 'K_in': K_in, 'Tf': Tf, 'ks': ks, 'passes': a.passes, 'yard_agents': min(a.yard_agents, n)}

    def buffer(R, agents):
        drift = 0.3 * torch.randn(R, agents, K_in, 1, 2, device=dev, generator=gen) * torch.linspace(0.3, 1.0, Tf, device=dev).view(1, 1, 1, Tf, 1)
        return (gt[:agents].unsqueeze(0).unsqueeze(2) + drift + 0.03 * torch.randn(R, agents, K_in, Tf, 2, device=dev, generator=gen)).contiguous()
    for M in (400, 2000):
        R, Y = M // K_in, min(a.yard_agents, n)
        buf = buffer(R, n)
        sub, sub_gt = buf[:, :Y].contiguous(), gt[:Y].contiguous()
        row = {'M': M, 'rounds': R}
        row['select'] = timed(lambda: metrics.large_select(buf, gt, ks=ks, seg_ptr=sp), a.passes)
        row['select_torch'] = timed(lambda: torch_select(buf, gt, sp, seg_of, ks), a.passes)
        row['kde'] = timed(lambda: metrics.large_kde_nll(buf, gt), a.passes)
        row['kde_torch'] = timed(lambda: torch_kde(buf, gt), a.passes)
        row['spread'] = timed(lambda: metrics.large_spread(buf, gt, div_scale=div), a.passes)
        row['spread_yard_agents'] = timed(lambda: metrics.large_spread(sub, sub_gt, div_scale=div), a.passes)
        row['spread_torch_yard_agents'] = timed(lambda: torch_spread(sub, sub_gt, div, 64 if M == 400 else 8), a.passes)
        row['reduce_samples'] = timed(lambda: metrics.reduce_samples(buf, 20, iters=10), a.passes)
        # the two forms compute the same thing
        ls, ts = metrics.large_select(buf, gt, ks=ks, seg_ptr=sp), torch_select(buf, gt, sp, seg_of, ks)
        sk, tk = metrics.large_kde_nll(buf, gt), torch_kde(buf, gt)
        ss, tsp = metrics.large_spread(sub, sub_gt, div_scale=div), torch_spread(sub, sub_gt, div, 64 if M == 400 else 8)
        row['agree'] = {'ade_max_rel': float(((ls.ade - ts[0].values).abs() / ts[0].values).max()),
                        'ade_idx_equal': float((ls.best_ade_idx == ts[0].indices).float().mean()),
                        'joint_idx_equal': float((ls.seg_jade_idx == ts[-2].indices).float().mean()),
                        'kde_max_abs': float((sk - tk).abs().max()),
                        'spread_max_rel': float(((torch.stack([ss.apd, ss.fpd, ss.pade, ss.dlow, ss.es_ade, ss.es_fde], 1) - tsp).abs()
                                                 / tsp.abs().clamp(min=1e-300)).max())}
        pairs = M * (M - 1) // 2
        row['spread_pair_frames_per_s'] = n * pairs * Tf / (row['spread']['median_ms'] * 1e-3)
        res['M%d' % M] = row
        print(json.dumps(row), flush=True)
        del buf, sub
        torch.cuda.empty_cache()
    B = min(a.big_agents, n)
    big = buffer(4096 // K_in + 1, B).permute(1, 0, 2, 3, 4).reshape(B, -1, Tf, 2)[:, :4096].contiguous()         # [B, 4096, Tf, 2]: R = 1
    row = {'M': 4096, 'agents': B, 'spread': timed(lambda: metrics.large_spread(big, gt[:B], div_scale=div), a.passes),
           'select': timed(lambda: metrics.large_select(big, gt[:B], ks=ks), a.passes),
           'kde': timed(lambda: metrics.large_kde_nll(big, gt[:B]), a.passes)}
    row['spread_pair_frames_per_s'] = B * (4096 * 4095 // 2) * Tf / (row['spread']['median_ms'] * 1e-3)
    res['M4096'] = row
    print(json.dumps(row), flush=True)
    txt = json.dumps(res, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, 'w').write(txt + '\n')
    print(txt)


if __name__ == '__main__':
    main()
