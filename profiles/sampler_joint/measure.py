"""Cost of the scene-level (joint) forms of the stage-2 sampler's terms (csrc/sampler_joint.hip) beside the marginal
objective, on the same device, in the same run, at the same shape.  The measurement runs in a fresh child process under a time limit.
Writes profiles/sampler_joint/rates.txt (or --out): the JSON line, then the times and their ratio.

    python profiles/sampler_joint/measure.py                 # the job
    python profiles/sampler_joint/measure.py --step kernel   # the measurement itself, prints its JSON line

  kernel  the agents of 512 ETH-shaped scenes (n = 8 729), K = 20, Tf = 12, nz = 32, a ragged 0/1 mask, the scenes as segments.  Forward +
          backward pairs on the same tensors, alternated window by window: `marginal` = sttode_sampler_objective + _bwd, `joint` =
          sttode_sampler_objective_joint + _bwd; and each of the four calls alone, to say where the time goes.  Each warmed, then `--reps`
          rounds of one window per form, a window = `--launches` back-to-back calls between two device events; median window / launches.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

LIMIT = 300   # seconds


def window(fn, launches):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        fn()
    e1.record()
    e1.synchronize()
    return 1e3 * e0.elapsed_time(e1) / launches


def step_kernel(a):
    import numpy as np
    import torch
    from sttode_amd import capi, scenes
    dev = torch.device('cuda:0')
    sb = scenes.make_scene_batch(range(20000, 20512), 'eth')
    n, K, Tf, nz = sb.n_agents, 20, 12, 32
    sp = torch.from_numpy(np.asarray(sb.scene_ptr, np.int32)).to(dev)
    S = sp.numel() - 1
    rng = np.random.default_rng(0)
    f = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32)).to(dev)
    gt = torch.from_numpy(sb.future).to(dev).contiguous()
    mo = (gt[:, None] + torch.from_numpy(rng.normal(0, 0.15, (n, K, Tf, 2)).astype(np.float32)).to(dev)).contiguous()
    mask = torch.from_numpy((rng.random((n, Tf)) < 0.8).astype(np.float32)).to(dev)
    mu, lv, pmu, plv = f(n * K, nz), 0.5 * f(n * K, nz), 0.5 * f(n * K, nz), 0.5 * f(n * K, nz)
    ga = [torch.full((n,), w / n, device=dev) for w in (0.1, 1.0, 5.0, 1.0)]
    gs = [ga[0]] + [torch.full((S,), w, device=dev) for w in (1.0 / S, 5.0 / n, 1.0 / S)]
    st = capi.stream_ptr()
    o = [torch.empty(n, device=dev) for _ in range(6)]
    os_ = [torch.empty(S, device=dev) for _ in range(3)]
    best, bests = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(S, dtype=torch.int32, device=dev)
    dmu, dlv, dmo = torch.empty_like(mu), torch.empty_like(lv), torch.empty_like(mo)
    D, scale = 2 * Tf, 1.0
    nb = capi.sampler_joint_ws(n, K, S)
    ws = torch.empty(nb // 8 + 1, dtype=torch.float64, device=dev)

    def m_fwd():
        capi.call('sttode_sampler_objective', mu, lv, pmu, plv, mo, gt, mask, n, K, nz, D, scale, o[0], o[1], o[2], best, o[3], o[4], st)

    def m_bwd():
        capi.call('sttode_sampler_objective_bwd', mu, lv, pmu, plv, mo, gt, mask, ga[0], ga[1], ga[2], ga[3], None, n, K, nz, D, scale, dmu, dlv,
                  dmo, st)

    def j_fwd():
        capi.call('sttode_sampler_objective_joint', mu, lv, pmu, plv, mo, gt, mask, sp, S, n, K, nz, D, scale, ws, nb, o[0], os_[0], os_[1], bests,
                  os_[2], st)

    def j_bwd():
        capi.call('sttode_sampler_objective_joint_bwd', mu, lv, pmu, plv, mo, gt, mask, sp, S, *gs, n, K, nz, D, scale, ws, nb, dmu, dlv, dmo, st)

    forms = {'marginal': lambda: (m_fwd(), m_bwd()), 'joint': lambda: (j_fwd(), j_bwd()), 'marginal_fwd': m_fwd, 'marginal_bwd': m_bwd,
             'joint_fwd': j_fwd, 'joint_bwd': j_bwd}
    for fn in forms.values():
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    p = torch.cuda.get_device_properties(0)
    out = {'agents': n, 'segments': S, 'largest_segment': int((sp[1:] - sp[:-1]).max()), 'K': K, 'Tf': Tf, 'nz': nz, 'workspace_bytes': nb,
           'launches_per_window': a.launches, 'rounds': a.reps, 'device': p.name, 'compute_units': p.multi_processor_count,
           'div_mean': float(os_[0].mean()), 'rec_sum_over_n': float(os_[1].sum() / n), 'es_mean': float(os_[2].mean()),
           'dmotion_finite': bool(torch.isfinite(dmo).all())}
    us = {k: [] for k in forms}
    for _ in range(a.reps):
        for k, fn in forms.items():
            us[k].append(window(fn, a.launches))
    for k, v in us.items():
        out[k] = {'median_us': float(np.median(v)), 'min_us': float(min(v)), 'max_us': float(max(v))}
    out['joint_over_marginal'] = out['joint']['median_us'] / out['marginal']['median_us']
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--step', choices=['kernel'])
    ap.add_argument('--launches', type=int, default=50)
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.abspath(__file__)), 'rates.txt'))
    a = ap.parse_args()
    if a.step:
        print(json.dumps(step_kernel(a)))
        return 0
    cmd = [sys.executable, os.path.abspath(__file__), '--step', 'kernel', '--launches', str(a.launches), '--reps', str(a.reps)]
    try:
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=LIMIT)
    except subprocess.TimeoutExpired:
        print(f'no result within {LIMIT} s; stopping', file=sys.stderr)
        return 124
    if p.returncode != 0:
        print(f'exit status {p.returncode}; stopping\n{p.stderr[-4000:]}', file=sys.stderr)
        return p.returncode if p.returncode > 0 else 1
    k = json.loads(p.stdout.strip().splitlines()[-1])
    print('kernel', json.dumps(k), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write('kernel ' + json.dumps(k) + '\n')
        f.write('forward + backward, n = %d in %d scene segments (largest %d), K = %d, Tf = %d (median us): marginal %.1f, joint %.1f, joint / marginal %.3f\n' % (
            k['agents'], k['segments'], k['largest_segment'], k['K'], k['Tf'], k['marginal']['median_us'], k['joint']['median_us'],
            k['joint_over_marginal']))
        f.write('alone (median us): marginal forward %.1f, backward %.1f; joint forward %.1f, backward %.1f; workspace %d bytes\n' % (
            k['marginal_fwd']['median_us'], k['marginal_bwd']['median_us'], k['joint_fwd']['median_us'], k['joint_bwd']['median_us'],
            k['workspace_bytes']))
        f.write('%s, %d compute units\n' % (k['device'], k['compute_units']))
    return 0


if __name__ == '__main__':
    sys.exit(main())
