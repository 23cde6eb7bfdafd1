"""Rates of the attention core with a running maximum (csrc/attention.hip) against what it stands beside:

  (a) sttode_attn_core mode 0, unmasked and masked, against the existing sttode_mhgsa_attn: the price of the running maximum and of the mask
  (b) sttode_attn_core mode 1 against torch's own bmm - softmax - bmm composition on the same device
  (c) sttode_attn_core_bwd (mode 0 unmasked / masked, mode 1) against sttode_mhgsa_attn_rc_bwd

at rows = cols = 512, Nb = 10 (one config-5 attention group) and 128 x 128, Nb = 11.  Both backward kernels keep their operands in 64 KiB
of LDS and refuse 512 x 512; (c) runs at 448 x 448, Nb = 10 instead.  Every comparison alternates the two sides in pairs inside one
process: a sample is the device-event time of a batch of launches sized to ~50 ms, after a warm-up of every shape; the figure is the
median of the samples, the spread their min and max.

    python profiles/exp_attention_rate.py [--out profiles/attention]     every step in a child process under its own time limit
    python profiles/exp_attention_rate.py --resources [--out ...]        no GPU: the compiler's register / scratch / LDS figures
"""
import argparse
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STEPS = [('fwd', 512, 10), ('fwd', 128, 11), ('torch', 512, 10), ('torch', 128, 11), ('bwd', 448, 10), ('bwd', 128, 11)]
STEP_LIMIT = 150                                        # seconds per child


def sample(fn, n):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n             # us per launch


def compare(sides, repeats=9):
    """sides: name -> callable.  Warm up, size the batches, then ``repeats`` alternating rounds.  -> name -> sorted samples (us)."""
    import torch
    n = {}
    for k, f in sides.items():
        sample(f, 20)
        n[k] = max(10, int(50e3 / max(sample(f, 20), 1.0)))
    torch.cuda.synchronize()
    got = {k: [] for k in sides}
    for _ in range(repeats):
        for k, f in sides.items():
            got[k].append(sample(f, n[k]))
    return {k: sorted(v) for k, v in got.items()}


def report(title, res, base):
    med = {k: v[len(v) // 2] for k, v in res.items()}
    lines = [title]
    for k, v in res.items():
        lines.append(f'  {k:34s} {med[k]:9.2f} us  (min {v[0]:.2f}, max {v[-1]:.2f})   x{med[k] / med[base]:.3f} of {base}')
    return lines


def step(kind, n, Nb):
    import torch
    from sttode_amd import capi
    dev = torch.device('cuda:0')
    torch.manual_seed(1)
    E, st, sc = 64, Nb * 64, 8 ** -0.5
    R, C, V, dO = (torch.randn(n, Nb, E, device=dev) for _ in range(4))
    mask = torch.randn(n, n, device=dev)
    mask[torch.rand(n, n, device=dev) < 0.2] = float('-inf')
    mask[:, -1] = 0.0
    out = torch.empty(n, Nb, E, device=dev)
    s = capi.stream_ptr()
    ss = (st, E) * 4
    core = lambda mode, mk: capi.call('sttode_attn_core', R, C, V, mk, n if mk is not None else 0, out, None, None, None, n, n, Nb, *ss, sc,
                                      1.0, mode, s)
    if kind == 'fwd':
        sides = {'sttode_mhgsa_attn': lambda: capi.call('sttode_mhgsa_attn', R, C, V, out, None, None, n, n, Nb, *ss, sc, 1.0, s),
                 'attn_core mode 0': lambda: core(0, None), 'attn_core mode 0 masked': lambda: core(0, mask),
                 'attn_core mode 1': lambda: core(1, None), 'attn_core mode 1 masked': lambda: core(1, mask)}
        return report(f'(a) forward {n} x {n}, Nb = {Nb}', compare(sides), 'sttode_mhgsa_attn')
    if kind == 'torch':
        q = (R * sc).view(n, Nb * 8, 8).transpose(0, 1).contiguous()
        k = C.view(n, Nb * 8, 8).transpose(0, 1).contiguous()
        v = V.view(n, Nb * 8, 8).transpose(0, 1).contiguous()
        kt = k.transpose(1, 2).contiguous()
        sides = {'torch bmm-softmax-bmm': lambda: torch.bmm(torch.softmax(torch.bmm(q, kt), dim=-1), v),
                 'torch baddbmm(mask)-softmax-bmm': lambda: torch.bmm(torch.softmax(torch.baddbmm(mask, q, kt), dim=-1), v),
                 'attn_core mode 1': lambda: core(1, None), 'attn_core mode 1 masked': lambda: core(1, mask)}
        with torch.no_grad():
            ref = torch.bmm(torch.softmax(torch.baddbmm(mask, q, kt), dim=-1), v).transpose(0, 1).reshape(n, Nb, E)
            core(1, mask)
            err = float((out - ref).abs().max())
            res = compare(sides)
        return report(f'(b) dot-product forward {n} x {n}, Nb = {Nb} (torch operands already head-major; max |diff| {err:.2e})', res,
                      'torch bmm-softmax-bmm')
    dR, dC, dV = (torch.empty_like(R) for _ in range(3))
    bwd = lambda mode, mk: capi.call('sttode_attn_core_bwd', R, C, V, mk, n if mk is not None else 0, dO, dR, dC, dV, n, n, Nb, *ss, sc, 1.0,
                                     mode, s)
    sides = {'sttode_mhgsa_attn_rc_bwd': lambda: capi.call('sttode_mhgsa_attn_rc_bwd', R, C, V, dO, dR, dC, dV, n, n, Nb, *ss, sc, 1.0, s),
             'attn_core_bwd mode 0': lambda: bwd(0, None), 'attn_core_bwd mode 0 masked': lambda: bwd(0, mask),
             'attn_core_bwd mode 1': lambda: bwd(1, None), 'attn_core_bwd mode 1 masked': lambda: bwd(1, mask)}
    return report(f'(c) backward {n} x {n}, Nb = {Nb}', compare(sides, repeats=5), 'sttode_mhgsa_attn_rc_bwd')


def resources(out_dir):
    src = os.path.join(ROOT, 'sttode_amd', 'csrc', 'attention.hip')
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    r = subprocess.run([hipcc, '-O3', '-std=c++17', '-fPIC', '--offload-arch=gfx950', '-Rpass-analysis=kernel-resource-usage', '-c', src, '-o',
                        os.devnull], capture_output=True, text=True, check=True)
    demangle = {'_Z16attn_core_kernel': 'attn_core_kernel', '_Z24attn_core_weights_kernel': 'attn_core_weights_kernel',
                '_Z20attn_core_bwd_kernel': 'attn_core_bwd_kernel'}
    lines, cur = ['kernel<MODE, MASKED>                          VGPRs  SGPRs  scratch B/lane  waves/SIMD  static LDS B'], {}
    spills = []
    for ln in r.stderr.splitlines():
        m = re.search(r'remark: .*?(Function Name|TotalSGPRs|VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\S+)', ln)
        if not m or m.group(1) == 'VGPRs' and 'AGPR' in ln:
            continue
        cur[m.group(1)] = m.group(2)
        if m.group(1).startswith('LDS'):
            f = cur['Function Name']
            t = re.match(r'(_Z\d+[a-z_]+)ILi(\d)ELb(\d)E', f)
            name = f'{demangle.get(t.group(1), t.group(1))}<{t.group(2)}, {"true" if t.group(3) == "1" else "false"}>' if t else f
            lines.append(f'{name:44s} {cur["VGPRs"]:>5s}  {cur["TotalSGPRs"]:>5s}  {cur["ScratchSize [bytes/lane]"]:>14s}  '
                         f'{cur["Occupancy [waves/SIMD]"]:>10s}  {cur["LDS Size [bytes/block]"]:>12s}')
            if cur['ScratchSize [bytes/lane]'] != '0':
                spills.append(name)
            cur = {}
    lines.append('(hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage; the backward kernels use dynamic LDS:')
    lines.append(' (19 rows + 16 cols) * 4 bytes, at most 64 KiB.  ' + ('No kernel uses scratch.)' if not spills else f'Scratch in: {spills})'))
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, 'resource_usage.txt'), 'w') as f:
        f.write('\n'.join(lines) + '\n')
    print('\n'.join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'attention'))
    ap.add_argument('--resources', action='store_true')
    ap.add_argument('--step', default=None, help='(child) kind,n,Nb')
    a = ap.parse_args()
    if a.resources:
        return resources(a.out)
    if a.step:
        kind, n, Nb = a.step.split(',')
        print('\n'.join(step(kind, int(n), int(Nb))))
        return
    os.makedirs(a.out, exist_ok=True)
    path = os.path.join(a.out, 'rates.txt')
    with open(path, 'w') as f:
        for kind, n, Nb in STEPS:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), '--step', f'{kind},{n},{Nb}'], capture_output=True, text=True,
                               timeout=STEP_LIMIT)
            f.write(r.stdout)
            f.flush()
            print(r.stdout, end='', flush=True)
            if r.returncode != 0:                       # a failed step ends the run: nothing more is started on the device
                f.write(f'step {kind},{n},{Nb} failed (status {r.returncode})\n{r.stderr[-2000:]}\n')
                print(r.stderr[-2000:])
                sys.exit(1)


if __name__ == '__main__':
    main()
