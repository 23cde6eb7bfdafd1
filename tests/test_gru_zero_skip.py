"""The streamed conv + GRU (csrc/chain32.hip gru32_steps) skips products whose operands are known to be zero: the recurrent tiles of
step 0 (h = 0) and the fragment groups of a conv tile outside its frames t-1 .. t+1.  A skipped product adds an exact zero, so the
default must give the same values as STTODE_GRU_ZERO_SKIP=0 (every tile in full): the chain's predictions in its three launch forms
(trajectory groups alone, fused with latency-form roles, lagged behind throughput-form roles), the tables the throughput-form roles
write, and sttode_gru_cols32 -- at Tp 5, 8, 10 and 16 (ldx 16 and 32, one to four conv fragment groups) with ragged column counts.

The switch is read once per process, so each setting runs in a child process (this file run as a script) that saves its outputs."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TPS = (5, 8, 10, 16)


def _outputs(path):
    import torch
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    from helpers import make_args
    from sttode_amd import STTODENet, capi, packing, scenes
    from sttode_amd.weights import make_weights, to_torch_state_dict
    dev = torch.device('cuda:0')
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    out = {}
    for Tp in TPS:
        sd = make_weights(1234, past_length=Tp, future_length=12)
        # sttode_gru_cols32 (the stand-alone streaming GRU)
        G = packing.gru32_stream(sd, 0, Tp)
        ldx = 16 * packing.tiles_x(Tp)
        for ncols in (31, 300):
            rng = np.random.default_rng(100 * Tp + ncols)
            xin = np.zeros((ncols, ldx), np.float32)
            xin[:, :2 * Tp] = rng.standard_normal((ncols, 2 * Tp)).astype(np.float32)
            st = torch.zeros(ncols, 96, device=dev)
            capi.call('sttode_gru_cols32', t(xin), ldx, t(G['pool']), t(G['prog']), G['prog_len'], t(G['consts']), st, ncols, Tp, capi.stream_ptr())
            out[f'gru_cols32_Tp{Tp}_n{ncols}'] = st.cpu().numpy()
        # the chain: 37 scenes of ragged sizes (the last trajectory group is partly empty)
        m = STTODENet(make_args('eth', Tp, 12), dev).eval()
        m.load_state_dict(to_torch_state_dict(sd), strict=True)
        sb = scenes.make_scene_batch(range(2000, 2037), 'eth', obs_len=Tp, pred_len=12)
        n, S = sb.n_agents, sb.n_scenes
        inp = (t(sb.past), t(sb.future), t(sb.scene_ptr))
        z = t(scenes.latents(300, n))
        nat = m.native()
        try:
            nat.set_chain(1)
            for fused in (0, 1):                              # 0: trajectory groups alone (FUSE 0); 1: latency-form roles in front (FUSE 1)
                nat.set_fused(fused)
                m.set_scene_batch(*inp)
                out[f'chain_fused{fused}_Tp{Tp}'] = m.inference(None, z=z).cpu().numpy()
            nat.set_fused(1)
            m.reset_async()
            hs = []
            for _ in range(3):                                # lagged launches (FUSE 2): throughput-form roles of a call + groups of an earlier one
                m.set_scene_batch(*inp)
                hs.append(m.inference_async(z=z))
            preds = [m.wait(h).clone() for h in hs]
            torch.cuda.synchronize()
            for i, p in enumerate(preds):
                out[f'chain_lagged{i}_Tp{Tp}'] = p.cpu().numpy()
            h = hs[-1]
            buf = m._async_bufs[(n, S, h['slot'])][0]
            off, _ = nat.layout(n, S)
            for k, w in (('pf', 128), ('state0', 96), ('A0x', 512), ('A0y', 512), ('A1y', 512)):
                out[f'roles_{k}_Tp{Tp}'] = m._view(buf, off, k, n, w).cpu().numpy()
        finally:
            nat.set_chain(-1)
            nat.set_fused(1)
            m.reset_async()
    np.savez(path, **out)


def _run(skip, path):
    env = dict(os.environ, STTODE_GRU_ZERO_SKIP=str(skip))
    cmd = [sys.executable] + (['-s'] if sys.flags.no_user_site else []) + [os.path.abspath(__file__), path]
    subprocess.run(cmd, env=env, check=True, timeout=600, cwd=ROOT)
    return dict(np.load(path))


def test_zero_skip_gives_the_values_of_the_full_products(tmp_path):
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    full = _run(0, str(tmp_path / 'full.npz'))
    skip = _run(1, str(tmp_path / 'skip.npz'))
    assert sorted(full) == sorted(skip)
    assert len(full) == len(TPS) * (2 + 2 + 3 + 5)
    for k in sorted(full):
        assert np.isfinite(full[k]).all(), k
        assert np.array_equal(full[k], skip[k]), f'{k}: max |diff| {np.abs(full[k] - skip[k]).max():.3e}'


if __name__ == '__main__':
    _outputs(sys.argv[1])
