"""Cost of the stage-2 objective's ground-truth terms (csrc/sampler_objective.hip).  One job of two steps, each a fresh child
process under its own time limit; the job stops at the first step that fails.  Writes profiles/sampler_objective/rates.txt (or --out): one
JSON line per step, then the three ratios.

    python profiles/sampler_objective/measure.py                 # both steps
    python profiles/sampler_objective/measure.py --step kernel   # one step, prints its JSON line

  kernel  the agents of 512 ETH-shaped scenes (n = 8 729), K = 20, Tf = 12, nz = 32, a ragged 0/1 mask.  Three forward + backward pairs on the
          same tensors, alternated window by window: `parent` = sttode_sampler_loss + _bwd (kld and div alone), `fused` =
          sttode_sampler_objective + _bwd (all five terms), `torch` = the parent's pair plus the reconstruction and energy terms written
          with torch ops on the device and autograd (what a user would write without the new kernels).  Each warmed, then `--reps` rounds
          of one window per form, a window = `--launches` back-to-back pairs between two device events; median window / launches.
  step    trainer.train_sampler_epoch over `--scenes` nine-pedestrian ETH-shaped scenes (one scene per step, as trainsampler.py), terms off
          and on (recon=True, energy_weight=1), alternated per round, each epoch timed from a device synchronise to a device synchronise.
"""
import argparse
import copy
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

LIMITS = {'kernel': 300, 'step': 300}   # seconds per step


def window(fn, launches):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        fn()
    e1.record()
    e1.synchronize()
    return 1e3 * e0.elapsed_time(e1) / launches


def device_facts():
    import torch
    p = torch.cuda.get_device_properties(0)
    mhz = 0.0
    try:                                                               # (read only) the engine clock the first device reports right now
        txt = subprocess.run(['rocm-smi', '-d', '0', '--showclocks'], capture_output=True, text=True, timeout=20).stdout
        for line in txt.splitlines():
            if 'sclk' in line and 'Mhz' in line:
                mhz = float(line.split('(')[-1].split('Mhz')[0])
                break
    except (OSError, ValueError, subprocess.SubprocessError):
        pass
    return {'device': p.name, 'compute_units': p.multi_processor_count, 'engine_clock_mhz': mhz}


def step_kernel(a):
    import numpy as np
    import torch
    from sttode_amd import capi, scenes
    dev = torch.device('cuda:0')
    sb = scenes.make_scene_batch(range(20000, 20512), 'eth')
    n, K, Tf, nz = sb.n_agents, 20, 12, 32
    rng = np.random.default_rng(0)
    f = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32)).to(dev)
    gt = torch.from_numpy(sb.future).to(dev).contiguous()
    drift = rng.normal(0, 1.0, (n, K, 1, 2)) * np.linspace(0.3, 1.0, Tf)[None, None, :, None]
    mo = (gt[:, None] + torch.from_numpy((drift + rng.normal(0, 0.1, (n, K, Tf, 2))).astype(np.float32)).to(dev)).contiguous()
    mask = torch.from_numpy((rng.random((n, Tf)) < 0.8).astype(np.float32)).to(dev)
    mu, lv, pmu, plv = f(n * K, nz), 0.5 * f(n * K, nz), 0.5 * f(n * K, nz), 0.5 * f(n * K, nz)
    g = [torch.full((n,), w / n, device=dev) for w in (0.1, 1.0, 5.0, 1.0)]
    st = capi.stream_ptr()
    o = [torch.empty(n, device=dev) for _ in range(6)]
    best = torch.empty(n, dtype=torch.int32, device=dev)
    dmu, dlv, dmo = torch.empty_like(mu), torch.empty_like(lv), torch.empty_like(mo)
    D, scale = 2 * Tf, 1.0

    def parent():
        capi.call('sttode_sampler_loss', mu, lv, pmu, plv, mo, n, K, nz, D, scale, o[0], o[1], st)
        capi.call('sttode_sampler_loss_bwd', mu, lv, pmu, plv, mo, g[0], g[1], n, K, nz, D, scale, dmu, dlv, dmo, st)

    def fused():
        capi.call('sttode_sampler_objective', mu, lv, pmu, plv, mo, gt, mask, n, K, nz, D, scale, o[0], o[1], o[2], best, o[3], o[4], st)
        capi.call('sttode_sampler_objective_bwd', mu, lv, pmu, plv, mo, gt, mask, g[0], g[1], g[2], g[3], None, n, K, nz, D, scale, dmu, dlv,
                  dmo, st)

    w4, w5 = mask[:, None, :, None], mask[:, None, None, :, None]

    def composed():
        parent()
        x = mo.detach().requires_grad_(True)
        diff = (x - gt[:, None]) * w4
        rec = diff.pow(2).sum(dim=-1).sum(dim=-1).min(dim=1)[0]
        pd = ((x[:, :, None] - x[:, None]) * w5).norm(dim=-1)
        es = diff.norm(dim=-1).mean(-1).mean(1) - 0.5 * pd.mean(-1).sum(dim=(1, 2)) / (K * K)
        (5.0 * rec.mean() + es.mean()).backward()
        return x.grad.add_(dmo)

    forms = {'parent': parent, 'fused': fused, 'torch': composed}
    # the values agree before anything is timed
    fused()
    fused_dmo = dmo.clone()
    rec_k, es_k = o[2].clone(), o[3].clone()
    tg = composed()
    x = mo.detach().double()
    diff = (x - gt[:, None].double()) * w4.double()
    rec64 = diff.pow(2).sum(dim=-1).sum(dim=-1).min(dim=1)[0]
    out = {'agents': n, 'K': K, 'Tf': Tf, 'nz': nz, 'launches_per_window': a.launches, 'rounds': a.reps,
           'max_abs_dmotion_fused_minus_torch': float((fused_dmo - tg).abs().max()), 'max_abs_dmotion': float(fused_dmo.abs().max()),
           'max_rel_rec_vs_float64': float(((rec_k.double() - rec64).abs() / rec64.clamp_min(1e-30)).max()), 'es_ade_mean': float(es_k.mean())}
    for fn in forms.values():
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    us = {k: [] for k in forms}
    for _ in range(a.reps):
        for k, fn in forms.items():
            us[k].append(window(fn, a.launches if k != 'torch' else max(a.launches // 10, 5)))
    for k, v in us.items():
        out[k] = {'median_us': float(np.median(v)), 'min_us': float(min(v)), 'max_us': float(max(v))}
    out.update(device_facts())
    out['fused_over_parent'] = out['fused']['median_us'] / out['parent']['median_us']
    out['torch_over_fused'] = out['torch']['median_us'] / out['fused']['median_us']
    return out


def step_step(a):
    import numpy as np
    import torch
    from helpers import make_args, sampler_args
    from sttode_amd import STTODENet, Sampler, samplerloss, scenes
    from sttode_amd.trainer import train_sampler_epoch
    from sttode_amd.weights import make_sampler_weights, make_weights, to_torch_state_dict
    dev = torch.device('cuda:0')
    net = STTODENet(make_args('eth', 8, 12), dev).eval()
    net.load_state_dict(to_torch_state_dict(make_weights(1234)), strict=True)
    smp = Sampler(sampler_args('eth', 8, 12))
    smp.load_state_dict(to_torch_state_dict(make_sampler_weights()), strict=True)
    smp.set_device(dev)
    loader = []
    for s in range(4242, 4242 + a.scenes):
        ob, pr = scenes.eth_scene(s, n_min=9, n_max=9)
        ob, pr = torch.from_numpy(ob), torch.from_numpy(pr)
        N = ob.shape[0]
        loader.append([ob[None], pr[None], ob[None], pr[None], torch.zeros(1, N), torch.ones(1, N), torch.ones(1, N, 8), torch.ones(1, N, 12),
                       torch.tensor([[10]]), ['seq']])
    cfg = samplerloss.get_diversity_config('eth')
    kinds = {'off': {}, 'on': {'recon': True, 'energy_weight': 1.0}}
    t = {k: [] for k in kinds}
    last = {}
    for r in range(a.rounds + 1):                                      # round 0 warms both forms
        for k, kw in kinds.items():
            s = copy.deepcopy(smp).train()
            opt = torch.optim.Adam(s.parameters(), lr=1e-3)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            losses = train_sampler_epoch(s.args, 0, net, s, opt, None, [copy.copy(b) for b in loader], cfg, log=None, **kw)
            torch.cuda.synchronize()
            if r:
                t[k].append((time.perf_counter() - t0) / len(loader))
            last[k] = losses[-1]
    out = {'scenes': a.scenes, 'agents_per_scene': 9, 'rounds': a.rounds, **device_facts(), 'last_loss': last}
    for k, v in t.items():
        out[k] = {'median_ms_per_step': 1e3 * float(np.median(v)), 'min_ms_per_step': 1e3 * float(min(v)), 'max_ms_per_step': 1e3 * float(max(v))}
    out['on_over_off'] = out['on']['median_ms_per_step'] / out['off']['median_ms_per_step']
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--step', choices=sorted(LIMITS))
    ap.add_argument('--launches', type=int, default=100)
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--scenes', type=int, default=24)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.abspath(__file__)), 'rates.txt'))
    a = ap.parse_args()
    if a.step:
        print(json.dumps({'kernel': step_kernel, 'step': step_step}[a.step](a)))
        return 0
    res = {}
    for step in ('kernel', 'step'):
        cmd = [sys.executable, os.path.abspath(__file__), '--step', step, '--launches', str(a.launches), '--reps', str(a.reps), '--scenes',
               str(a.scenes), '--rounds', str(a.rounds)]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=LIMITS[step])
        except subprocess.TimeoutExpired:
            print(f'step {step}: no result within {LIMITS[step]} s; stopping', file=sys.stderr)
            return 124
        if p.returncode != 0:
            print(f'step {step}: exit status {p.returncode}; stopping\n{p.stderr[-4000:]}', file=sys.stderr)
            return p.returncode if p.returncode > 0 else 1
        res[step] = json.loads(p.stdout.strip().splitlines()[-1])
        print(step, json.dumps(res[step]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    k, s = res['kernel'], res['step']
    with open(a.out, 'w') as f:
        f.write('kernel ' + json.dumps(k) + '\n')
        f.write('step ' + json.dumps(s) + '\n')
        f.write('forward + backward, n = %d, K = %d, Tf = %d (median us): parent %.1f, fused %.1f, torch composition %.1f\n' % (
            k['agents'], k['K'], k['Tf'], k['parent']['median_us'], k['fused']['median_us'], k['torch']['median_us']))
        f.write('fused / parent %.3f   torch composition / fused %.3f   training step on / off %.3f (%.3f ms / %.3f ms)\n' % (
            k['fused_over_parent'], k['torch_over_fused'], s['on_over_off'], s['on']['median_ms_per_step'], s['off']['median_ms_per_step']))
        f.write('%s, %d compute units, engine clock %.0f MHz after the kernel step, %.0f MHz after the training step\n' % (
            k['device'], k['compute_units'], k['engine_clock_mhz'], s['engine_clock_mhz']))
    return 0


if __name__ == '__main__':
    sys.exit(main())
