"""GPU tests of the latent-set generator (sttode_latent_set, csrc/latents.hip) and the layers above it: latents.draw,
latents.LatentSource, STTODENet.latent_source and the z_fn of the evaluation loops.

Bounds.  The integer stage is held to tests/latents_ref.py bit for bit (torch.equal).  The value stage is held to
float32(torch.special.ndtri(u)) with u rebuilt in float64 from the device's own bits, within one float32 ulp (numpy.spacing): both sides
round one float64 quantile whose implementations differ by ~1e-15 relative, so they differ at a rounding tie at most.  The truncated form
is held the same way to the quantile of ndtr(-t) + u (ndtr(t) - ndtr(-t)), clamped, in the well-conditioned form of
latents_ref.quantiles (the sum next to ndtr(-t), evaluated as written in float64, is itself ten float32 ulps off near the mode).
Moments of the i.i.d. kind: five standard errors of N(0, 1).
Through the model: bitwise where the same kernels read the same tensor, the tolerance of tests/test_gpu_parity.py between the lagged and
the serial form (rtol = atol = 2e-5) where the forms differ.

No input here is beyond the entry's limits except in the refusal test, whose calls launch nothing."""
import numpy as np
import pytest
import torch

import latents_ref as ref
from test_reduce_gpu import _dataset, _gpu, _model

pytestmark = pytest.mark.gpu
SHAPES = [(1, 1, 1, 4), (3, 20, 1, 32), (130, 7, 3, 36), (2, 64, 1, 1), (1, 4096, 16, 8), (5, 65, 1, 1024), (2, 5, 2, 7)]     # (n, K, R, zdim)
MODES = [('sobol', None), ('sobol', 'shift'), ('sobol', 'owen'), ('random', None)]
FIRST = (0, 5, (1 << 32) + 3)
SEED = 0x9e3779b97f4a7c15


def _draw(n, K, zdim, rounds=1, **kw):
    """latents.draw with bits -> (z float32 [R, n K, zdim], bits uint32 of the same shape) as NumPy arrays."""
    from sttode_amd import latents
    z, bits = latents.draw(n, K, zdim, rounds=rounds, device=_gpu(), return_bits=True, **kw)
    torch.cuda.synchronize()
    assert z.dtype == torch.float32 and bits.dtype == torch.int32 and tuple(z.shape) == tuple(bits.shape) == ((n * K, zdim) if rounds == 1 else (rounds, n * K, zdim))
    return z.cpu().numpy().reshape(rounds, n * K, zdim), bits.cpu().numpy().view(np.uint32).reshape(rounds, n * K, zdim)


def _one_ulp(z, want64, what):
    w = want64.astype(np.float32)
    assert np.isfinite(z).all(), what
    err = np.abs(z.astype(np.float64) - w.astype(np.float64))
    assert (err <= np.spacing(np.abs(w)).astype(np.float64)).all(), (what, float((err / np.spacing(np.abs(w))).max()))


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'n%d_K%d_R%d_z%d' % s)
def test_bits_equal_the_restatement_and_values_the_quantile(shape):
    """M not a power of two, M = 65536 on one agent, zdim = 1, the largest table, the 64-bit agent counter, and (the last shape) a zdim
    whose last quad is a scalar tail of three: the integers bit for bit, and every value within one float32 ulp of ndtri of its own
    integer, finite, |z| <= 6.34."""
    n, K, R, zdim = shape
    for kind, scramble in MODES:
        for fa in FIRST:
            z, bits = _draw(n, K, zdim, rounds=R, kind=kind, scramble=scramble, seed=SEED, first_agent=fa)
            want, _ = ref.set_ints(n, K, R, zdim, kind=kind, scramble=scramble, seed=SEED, first_agent=fa)
            assert torch.equal(torch.from_numpy(bits.view(np.int32)), torch.from_numpy(ref.to_rounds(want, K).view(np.int32))), (shape, kind, scramble, fa)
            if fa == FIRST[-1]:
                _one_ulp(z, ref.quantiles(bits), (shape, kind, scramble))
                assert np.abs(z).max() <= 6.34
    if shape == SHAPES[2]:                                              # the raw sequence starts in the corner: for checks only
        z, bits = _draw(n, K, zdim, rounds=R, scramble=None, seed=SEED)
        assert (bits[0, ::K] == 0).all() and (z[0, ::K] < -6.33).all()


@pytest.mark.parametrize('t', [0.01, 1.0, 2.5])
def test_truncated_values(t):
    n, K, R, zdim = SHAPES[2]
    for kind, scramble in (('sobol', 'owen'), ('sobol', None), ('random', None)):
        z, bits = _draw(n, K, zdim, rounds=R, kind=kind, scramble=scramble, seed=SEED, truncate=t)
        plain, pbits = _draw(n, K, zdim, rounds=R, kind=kind, scramble=scramble, seed=SEED)
        assert np.array_equal(bits, pbits)                             # the integer stage does not know about the truncation
        _one_ulp(z, ref.quantiles(bits, t), (t, kind, scramble))
        assert (np.abs(z) <= np.float32(t)).all()
        assert np.array_equal(np.sign(z[np.abs(plain) > 1e-3]), np.sign(plain[np.abs(plain) > 1e-3]))


@pytest.mark.parametrize('M', [2, 3, 20, 21])
def test_set_composition(M):
    """z[c + H + j] == -z[c + j] bitwise, the centre row exactly 0, the drawn rows the rows of the plain draw with the same seed, and the
    round / column placement that of a [n, M, zdim] view of the restatement -- for M in one round, in M rounds of one, and in 3 x 7."""
    n, zdim = 3, 6
    for K, R in ((M, 1), (1, M)) + (((7, 3),) if M == 21 else ()):
        z0, b0 = _draw(n, K, zdim, rounds=R, seed=77)
        z0s = ref.from_rounds(z0, n, K)
        assert np.array_equal(ref.from_rounds(b0, n, K), ref.set_ints(n, K, R, zdim, seed=77)[0])
        for anti in (False, True):
            for cen in (False, True):
                z, b = _draw(n, K, zdim, rounds=R, seed=77, antithetic=anti, center=cen)
                zs, bs = ref.from_rounds(z, n, K), ref.from_rounds(b, n, K)
                c, H, B = ref.drawn_points(M, anti, cen)
                want, sign = ref.set_ints(n, K, R, zdim, antithetic=anti, center=cen, seed=77)
                assert np.array_equal(bs, want), (M, K, R, anti, cen)
                assert (zs[:, :c].view(np.uint32) == 0).all() and np.array_equal(zs[:, c:c + H], z0s[:, :H]), (M, K, R, anti, cen)
                assert np.array_equal(zs[:, c + H:].view(np.uint32), (-zs[:, c:c + B - H]).view(np.uint32)), (M, K, R, anti, cen)
                assert (sign[:, c + H:] == -1).all() and zs.shape[1] == M


@pytest.mark.parametrize('scramble', ['owen', 'shift'])
def test_net_and_stratification_on_the_device_output(scramble):
    n, M, zdim = 130, 64, 32
    _, bits = _draw(n, M, zdim, scramble=scramble, seed=SEED)
    p = bits.reshape(n, M, zdim)
    for a in range(n):
        assert ref.is_net_1d(p[a], M), (scramble, a)
        assert ref.is_net_2d(p[a][:, 0], p[a][:, 1], M), (scramble, a)


def test_repeatable_seeded_and_independent_of_the_batch():
    n, K, R, zdim = 130, 7, 3, 36
    z, b = _draw(n, K, zdim, rounds=R, seed=SEED)
    z2, b2 = _draw(n, K, zdim, rounds=R, seed=SEED)
    assert np.array_equal(b, b2) and np.array_equal(z.view(np.uint32), z2.view(np.uint32))
    _, b3 = _draw(n, K, zdim, rounds=R, seed=SEED + 1)
    assert not np.array_equal(b, b3)
    per = ref.from_rounds(b, n, K)
    assert all(not np.array_equal(per[0], per[a]) for a in range(1, n))                    # every agent has its own randomisation
    # agents 5 .. 8 drawn alone are rows 5 .. 8 of the draw of 130, and stay what they are with agents appended behind
    zs, bs = _draw(4, K, zdim, rounds=R, seed=SEED, first_agent=5)
    assert np.array_equal(ref.from_rounds(bs, 4, K), per[5:9])
    assert np.array_equal(ref.from_rounds(zs, 4, K).view(np.uint32), ref.from_rounds(z, n, K)[5:9].view(np.uint32))
    zl, bl = _draw(n + 37, K, zdim, rounds=R, seed=SEED)
    assert np.array_equal(ref.from_rounds(bl, n + 37, K)[:n], per)
    _, br = _draw(n, K, zdim, rounds=R, seed=SEED, kind='random')
    _, bs = _draw(4, K, zdim, rounds=R, seed=SEED, kind='random', first_agent=5)
    assert np.array_equal(ref.from_rounds(bs, 4, K), ref.from_rounds(br, n, K)[5:9])
    # seed=None: 63 bits of torch's generator -- reproducible under manual_seed, and not a constant
    from sttode_amd import latents
    torch.manual_seed(123)
    a1 = latents.draw(3, 20, 32, device=_gpu())
    a2 = latents.draw(3, 20, 32, device=_gpu())
    torch.manual_seed(123)
    a3 = latents.draw(3, 20, 32, device=_gpu())
    assert torch.equal(a1, a3) and not torch.equal(a1, a2)


def test_moments_of_the_random_kind():
    z, _ = _draw(130, 64, 32, kind='random', seed=ref.MOMENT_SEED)
    N = z.size
    z = z.astype(np.float64)
    assert N == 130 * 64 * 32 and abs(z.mean()) <= 5 / np.sqrt(N) and abs(z.var() - 1.0) <= 5 * np.sqrt(2.0 / N)


def test_refused_calls_leave_the_sentinels_and_null_bits_is_accepted():
    from sttode_amd import capi, latents
    dev = _gpu()
    n, K, R, zdim = 2, 20, 2, 32
    z = torch.full((R, n * K, zdim), 7.25, device=dev)
    bits = torch.full((R, n * K, zdim), -77, dtype=torch.int32, device=dev)
    dirs = latents.directions(zdim, dev)
    good = dict(z=z, bits=bits, dirs=dirs, n=n, K=K, R=R, zdim=zdim, first_agent=0, seed=1, kind=0, scramble=2, antithetic=0, center=0, truncate=0.0)
    for bad in (dict(z=None), dict(n=0), dict(K=0), dict(R=0), dict(K=65536, R=2), dict(zdim=0), dict(zdim=1025), dict(first_agent=-1), dict(kind=2),
                dict(scramble=3), dict(antithetic=2), dict(center=2), dict(truncate=0.005), dict(truncate=float('nan')), dict(truncate=-1.0),
                dict(dirs=None), dict(K=1, R=1, center=1)):
        a = {**good, **bad}
        with pytest.raises(capi.SttodeError, match='sttode_latent_set: '):
            capi.call('sttode_latent_set', *[a[k] for k in good], capi.stream_ptr())
    torch.cuda.synchronize()
    assert (z == 7.25).all() and (bits == -77).all()
    capi.call('sttode_latent_set', *[{**good, 'bits': None}[k] for k in good], capi.stream_ptr())
    capi.call('sttode_latent_set', *[{**good, 'kind': 1, 'dirs': None, 'bits': None, 'z': torch.empty_like(z)}[k] for k in good], capi.stream_ptr())
    torch.cuda.synchronize()
    want = latents.draw(n, K, zdim, rounds=R, seed=1, device=dev)
    assert torch.equal(z, want) and (bits == -77).all()


# ----- through the model ---------------------------------------------------------------------------------------------------------------

def _batch61(m):
    from sttode_amd import scenes
    sb = scenes.make_scene_batch(range(4000, 4061), 'eth')
    m.set_scene_batch(sb.past, sb.future, sb.scene_ptr)
    return sb


def test_model_takes_its_latents_from_the_source():
    from helpers import assert_close
    from sttode_amd import capi, latents
    m = _model('eth')
    sb = _batch61(m)
    n, K, zdim = sb.n_agents, m.args.sample_k, m.args.zdim
    opts = dict(seed=4242, antithetic=True, device=m.device)
    calls = []
    real = capi.call
    try:
        m.native().set_chain(1)
        # inference(): the source's tensor, handed in as z
        m.latent_source = latents.LatentSource(K, zdim, **opts)
        got = m.inference(None).clone()
        z = latents.draw(n, K, zdim, **opts)
        assert torch.equal(got, m.inference(None, z=z))
        assert m.latent_source.first_agent == n
        # inference_async + wait: the next n agents; against the serial form on the same tensor at the tolerance between those two forms
        m.set_scene_batch(sb.past, sb.future, sb.scene_ptr)
        h = m.inference_async()
        z2 = latents.draw(n, K, zdim, first_agent=n, **opts)
        assert torch.equal(h['z'], z2)
        out = m.wait(h).clone()
        m.reset_async()
        m.set_scene_batch(sb.past, sb.future, sb.scene_ptr)
        assert_close(out.cpu().numpy(), m.inference(None, z=z2).cpu().numpy(), rtol=2e-5, atol=2e-5, what='inference_async with a source vs the serial form')
        # inference_reduced(rounds=3): the round buffer is three inference(z=draw(..., rounds=3)[r]) calls, bitwise
        m.latent_source = latents.LatentSource(K, zdim, rounds=3, **opts)
        m.inference_reduced(3)
        buf = m.reduced_samples.clone()
        z3 = latents.draw(n, K, zdim, rounds=3, **opts)
        for r in range(3):
            assert torch.equal(buf[r], m.inference(None, z=z3[r]).permute(1, 0, 2, 3)), r
        # a source that does not fit the call
        with pytest.raises(ValueError, match='latent_source is built for'):
            m.inference_reduced(2)
        m.latent_source = latents.LatentSource(K, 16, **opts)
        with pytest.raises(ValueError, match='latent_source is built for'):
            m.inference(None)
        # cleared: a default call makes the default calls
        m.latent_source = None
        capi.call = lambda name, *a, **k: (calls.append(name), real(name, *a, **k))[1]
        timing, capi.TIMING = capi.TIMING, []                           # (inference() then launches through capi.call)
        try:
            torch.manual_seed(9)
            a1 = m.inference(None).clone()
            torch.manual_seed(9)
            zr = torch.randn(n * K, zdim, device=m.device)
        finally:
            capi.call, capi.TIMING = real, timing
        assert calls == ['sttode_inference_scenes'] and torch.equal(a1, m.inference(None, z=zr))
    finally:
        capi.call = real
        m.latent_source = None
        m.reset_async()
        m.native().set_chain(-1)


def test_evaluation_loops_take_a_source_as_z_fn():
    from sttode_amd import latents
    from sttode_amd.evaluate import eval_scenes, eval_scenes_reduced
    m = _model('eth')
    ds = _dataset(range(5200, 5261), 'eth')
    n, K, zdim = int(ds.obs_traj.shape[0]), m.args.sample_k, m.args.zdim
    src = latents.LatentSource(K, zdim, seed=99, device=m.device)
    kw = dict(traj_scale=1.3, scenes_per_call=25)
    ser = eval_scenes(m, ds, z_fn=src, pipelined=False, **kw)
    assert src.first_agent == n == ser[2]                              # every agent of the dataset got its own randomisation
    src.reset()
    pip = eval_scenes(m, ds, z_fn=src, pipelined=True, **kw)
    assert pip[2] == n and all(abs(p - s) <= 1e-5 * (1 + s) for p, s in zip(pip[:2], ser[:2]))
    # what the loop computed is the loop on the same latents handed in as plain tensors
    zall = latents.draw(n, K, zdim, seed=99, device=m.device)
    pos = [0]

    def z_fn(rows):
        pos[0] += rows
        return zall[pos[0] - rows:pos[0]]
    assert eval_scenes(m, ds, z_fn=z_fn, pipelined=False, **kw) == ser
    # the reduced loops: one group of `rounds` calls per scene batch
    src3 = latents.LatentSource(K, zdim, rounds=3, seed=99, device=m.device)
    rser = eval_scenes_reduced(m, ds, 3, z_fn=src3, pipelined=False, iters=4, **kw)
    assert src3.first_agent == n and src3._group is None
    src3.reset()
    rpip = eval_scenes_reduced(m, ds, 3, z_fn=src3, pipelined=True, iters=4, **kw)
    assert rser.n_agents == rpip.n_agents == n and len(rser.scene_ade) == len(rpip.scene_ade) == len(ds)
    assert np.isfinite([rser.ade, rser.fde, rpip.ade, rpip.fde]).all()
    # (at rounds > 1 the pipelined samples differ from the serial ones by fp32 rounding, which k-means may amplify: as for any z_fn, the two
    # loops are compared at one round, where the reduction is the identity)
    src1 = latents.LatentSource(K, zdim, rounds=1, seed=99, device=m.device)
    r1s = eval_scenes_reduced(m, ds, 1, z_fn=src1, pipelined=False, **kw)
    src1.reset()
    r1p = eval_scenes_reduced(m, ds, 1, z_fn=src1, pipelined=True, **kw)
    np.testing.assert_allclose(r1p.scene_ade, r1s.scene_ade, rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(r1p.scene_fde, r1s.scene_fde, rtol=1e-5, atol=1e-6)
    assert abs(r1s.ade - ser[0]) <= 1e-5 * (1 + ser[0])
