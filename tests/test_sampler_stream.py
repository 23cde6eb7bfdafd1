"""CPU tests of the stage-2 sampler's weight stream (packing.sampler_stream) and its C-ABI surface.

A float64 NumPy walk of the stream -- tile by tile in the chunk program's order, exactly the order csrc/role32.hpp qnet32 consumes them --
reproduces the Q-net's latents z of the CPU oracle (oracle/sampler_ref.py, sampler.py:39-51) from given past features."""
import argparse
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _args(qnet_mlp=(512, 256), nz=32, K=20):
    return argparse.Namespace(sample_k=K, nz=nz, share_eps=True, train_w_mean=True, qnet_mlp=list(qnet_mlp), dataset='eth')


def _oracle(qnet_mlp, seed=7):
    from oracle.sampler_ref import SamplerRef
    torch.manual_seed(seed)
    s = SamplerRef(_args(qnet_mlp)).eval()
    with torch.no_grad():
        for p in s.parameters():                          # weights of the scale a trained Q-net has, biases included
            p.copy_(torch.randn_like(p) * (0.6 / np.sqrt(p.shape[-1])))
    return s


def _oracle_z(s, pf, mode, eps):
    """The z of SamplerRef.forward (sampler.py:39-51) from past features, float64."""
    s = s.double()
    with torch.no_grad():
        qh = s.q_mlp(s.linear(torch.from_numpy(pf)))
        A, b = s.q_A(qh).view(-1, s.nz), s.q_b(qh).view(-1, s.nz)
        if mode == 0:
            return b.numpy()
        e = torch.from_numpy(eps).double()
        e = e.repeat(pf.shape[0] * s.nk, 1) if mode == 1 else e.repeat_interleave(s.nk, dim=0)
        return (A * e + b).numpy()


def _unpk32(t):
    """Inverse of packing.pk32_tile: 1024 floats -> the [32 rows, 32 k] block."""
    return np.asarray(t, np.float64).reshape(4, 2, 32, 4).transpose(2, 0, 1, 3).reshape(32, 32)


class _Feed:
    """The tiles of a chunk program in order (TileFeed of csrc/role32.hpp)."""

    def __init__(self, pool, prog):
        self.tiles = [int(first) + i for first, cnt in prog for i in range(int(cnt))]
        self.pool, self.i = pool, 0

    def mma(self, acc, B):
        W = _unpk32(self.pool[self.tiles[self.i]])
        self.i += 1
        return acc + W @ B


def walk(S, pf, mode, eps):
    """qnet32 in float64: columns = agents, features = rows; returns z [n K, 32] (row agent K + k)."""
    K, h1t, h2t = S['K'], S['h1'] // 32, S['h2'] // 32
    bias = S['biases'].astype(np.float64)
    bl, b1 = bias[:64], bias[64:64 + S['h1']]
    b2 = bias[64 + S['h1']:64 + S['h1'] + S['h2']]
    bb = bias[64 + S['h1'] + S['h2']:][:32 * K]
    bA = bias[64 + S['h1'] + S['h2'] + 32 * K:]
    fd = _Feed(S['pool'], S['prog_eps'] if mode else S['prog_mean'])
    n = pf.shape[0]
    P = [pf.T[32 * kt:32 * kt + 32] for kt in range(4)]
    H0 = []
    for j in range(2):
        acc = np.repeat(bl[32 * j:32 * j + 32, None], n, axis=1)
        for kt in range(4):
            acc = fd.mma(acc, P[kt])
        H0.append(acc)
    H2 = [np.zeros((32, n)) for _ in range(h2t)]
    for ht in range(h1t):
        hid = np.repeat(b1[32 * ht:32 * ht + 32, None], n, axis=1)
        hid = np.tanh(fd.mma(fd.mma(hid, H0[0]), H0[1]))
        for j in range(h2t):
            H2[j] = fd.mma(H2[j], hid)
    H2 = [np.tanh(H2[j] + b2[32 * j:32 * j + 32, None]) for j in range(h2t)]
    E = None if mode == 0 else (np.repeat(eps.reshape(32, 1), n, axis=1) if mode == 1 else eps.T.astype(np.float64))
    z = np.zeros((n, K, 32))
    for k in range(K):
        zb = np.repeat(bb[32 * k:32 * k + 32, None], n, axis=1)
        for j in range(h2t):
            zb = fd.mma(zb, H2[j])
        if mode:
            za = np.repeat(bA[32 * k:32 * k + 32, None], n, axis=1)
            for j in range(h2t):
                za = fd.mma(za, H2[j])
            zb = za * E + zb
        z[:, k] = zb.T
    assert fd.i == len(fd.tiles), 'the program holds tiles the Q-net does not consume'
    return z.reshape(n * K, 32)


@pytest.mark.parametrize('qnet_mlp', [(512, 256), (128, 128)])
@pytest.mark.parametrize('mode', [0, 1, 2])
def test_stream_walk_reproduces_the_oracle_latents(qnet_mlp, mode):
    from sttode_amd import packing
    s = _oracle(qnet_mlp)
    S = packing.sampler_stream({k: v.detach().numpy() for k, v in s.state_dict().items()})
    rng = np.random.default_rng(11)
    n = 37
    pf = np.maximum(rng.standard_normal((n, 128)), 0.0)        # past features are relu outputs (ode_demo.py:231)
    eps = rng.standard_normal((1 if mode == 1 else n, 32))
    got = walk(S, pf, mode, eps)
    ref = _oracle_z(s, pf, mode, eps)
    # float32 weights on both sides; float64 arithmetic: the walk and the oracle differ only by summation order
    assert np.abs(got - ref).max() <= 1e-6 * max(1.0, np.abs(ref).max()), np.abs(got - ref).max()


def test_stream_programs_cover_the_pool_in_chunks_of_three():
    from sttode_amd import packing
    s = _oracle((512, 256))
    S = packing.sampler_stream({k: v.detach().numpy() for k, v in s.state_dict().items()})
    T = S['pool'].shape[0]
    assert S['pool'].shape[1] == 1024 and S['pool'].dtype == np.float32
    assert T == 8 + 16 * (2 + 8) + 20 * 8 * 2
    for key in ('prog_eps', 'prog_mean'):
        prog = S[key]
        assert prog.dtype == np.int32 and prog.shape[1] == 2
        assert (prog[:, 1] >= 1).all() and (prog[:, 1] <= 3).all() and (prog[:, 0] >= 0).all() and (prog.sum(axis=1) <= T).all()
        assert len(prog) <= 4096
    seq = [int(f) + i for f, c in S['prog_eps'] for i in range(int(c))]
    assert seq == list(range(T))                                # every tile once, in pool order
    mean = [int(f) + i for f, c in S['prog_mean'] for i in range(int(c))]
    assert len(mean) == 8 + 16 * 10 + 20 * 8 and mean == sorted(mean)   # the q_A tiles are skipped in mean mode
    assert S['biases'].shape == (64 + 512 + 256 + 2 * 20 * 32,)


def test_refusal_reasons_are_listed():
    from sttode_amd import Sampler
    assert Sampler(_args()).unsupported_reason() is None
    assert 'nz' in Sampler(_args(nz=16)).unsupported_reason()
    assert 'two hidden layers' in Sampler(_args((256, 256, 128))).unsupported_reason()
    assert 'multiples of 32' in Sampler(_args((48, 256))).unsupported_reason()
    assert '<= 256' in Sampler(_args((512, 512))).unsupported_reason()


def test_qnet_entry_point_refuses_plans_it_cannot_stream():
    """Refused before anything touches a device (no GPU here): each bad plan fails with a message naming the entry point."""
    from sttode_amd import capi
    L = capi.lib()
    fake = 256                                                  # never dereferenced: the checks come first

    def plan(**kw):
        d = dict(pool=fake, prog=fake, prog_len=116, biases=fake, K=20, nz=32, h1=512, h2=256, eps_mode=0, eps=None)
        d.update(kw)
        return capi.SamplerPlan(**d)
    for bad in (dict(nz=16), dict(h1=48), dict(h2=288), dict(eps_mode=1), dict(eps_mode=3, eps=fake), dict(prog_len=0), dict(pool=None),
                dict(K=0), dict(prog_len=5)):
        p = plan(**bad)
        rc = L.sttode_sampler_qnet(ctypes.addressof(p), fake, 4, fake, None)
        assert rc != 0, bad
        assert 'sttode_sampler_qnet' in L.sttode_last_error().decode(), bad
    assert L.sttode_sampler_qnet(None, None, 0, None, None) != 0


def test_plan_structs_mirror_the_header():
    from sttode_amd import capi
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'sttode_hip.h')).read(), flags=re.S)

    def fields(name):
        body = re.search(r'typedef struct %s \{(.*?)\}' % name, src, flags=re.S).group(1)
        return [re.split(r'[\s\*]+', d.strip())[-1] for d in body.split(';') if d.strip()]
    assert fields('SttodeSamplerPlan') == [f for f, _ in capi.SamplerPlan._fields_]
    assert fields('SttodeAsyncOpts') == [f for f, _ in capi.AsyncOpts._fields_]
    assert fields('SttodeAsyncOpts')[-1] == 'sampler'
