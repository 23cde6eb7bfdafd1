"""CPU tests of the latent-set generator (sttode_latent_set, csrc/latents.hip, sttode_amd/latents.py): the NumPy
restatement of tests/latents_ref.py against torch's own SobolEngine, the Random123 known answers and the net properties it must keep;
the C ABI's export and refusals; the Python layer's refusals and the LatentSource bookkeeping on a stub ``draw``; and STTODENet's call
sequence with ``latent_source`` unset (what it was) and set."""
import ctypes
import types

import numpy as np
import pytest
import torch

import latents_ref as ref

SCRAMBLES = (None, 'shift', 'owen')


# ----- the restatement -----------------------------------------------------------------------------------------------------------------

def test_philox_known_answers():
    """Random123's kat_vectors for philox4x32-10: the all-zero, the all-ones and the pi-digits inputs."""
    for ctr, key, want in (((0, 0, 0, 0), 0, (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
                           ((0xffffffff,) * 4, 0xffffffffffffffff, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
                           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0x299f31d0 << 32) | 0xa4093822,
                            (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))):
        assert tuple(int(v) for v in ref.philox4x32_10(*ctr, key)) == want


def test_unscrambled_integers_are_torchs_sobol_sequence():
    x = ref.sobol_ints(70, 36)
    want = torch.quasirandom.SobolEngine(36, scramble=False).draw(70, dtype=torch.float64).numpy() * 2.0 ** 30
    assert np.array_equal((x >> np.uint32(2)).astype(np.float64), want)
    assert (x & np.uint32(3) == 0).all() and (ref.point_ints(3, 70, 36, scramble=None, seed=9, first_agent=4) == x[None]).all()


@pytest.mark.parametrize('M', [16, 64, 1024])
@pytest.mark.parametrize('scramble', SCRAMBLES)
def test_scrambles_keep_the_net(M, scramble):
    """Every dimension's top log2(M) bits are a permutation of 0 .. M-1, and dimensions (0, 1) form a (0, m, 2)-net: one point in every
    elementary interval of area 1 / M -- for the raw sequence and under both scrambles, per agent."""
    p = ref.point_ints(3, M, 6, scramble=scramble, seed=0x1234567890abcdef, first_agent=(1 << 32) + 3)
    for a in range(3):
        assert ref.is_net_1d(p[a], M) and ref.is_net_2d(p[a][:, 0], p[a][:, 1], M)
    if scramble is not None:
        assert not np.array_equal(p[0], p[1]) and not np.array_equal(p[0], ref.point_ints(1, M, 6, scramble=scramble, seed=5)[0])


def test_scrambles_are_what_the_definition_says():
    """One element by hand: the digital shift is an XOR with s(a, d); the nested scramble is brev(h(brev(x), s)), h in Python integers."""
    a0, zdim, seed = 77, 7, 0xfeedfacecafebeef
    x = ref.sobol_ints(9, zdim)
    s = ref.philox_words([a0], zdim, [0], seed)[0, 0]
    assert int(s[5]) == int(ref.philox4x32_10(a0, 0, 1, 0, seed)[1])                     # d = 5: quad 1, word 1
    sh, ow = (ref.point_ints(1, 9, zdim, scramble=k, seed=seed, first_agent=a0)[0] for k in ('shift', 'owen'))
    assert np.array_equal(sh, x ^ s[None])

    def rev(v):
        return int(format(v, '032b')[::-1], 2)
    for j, d in ((0, 0), (3, 5), (8, 6)):
        v = (rev(int(x[j, d])) + int(s[d])) & 0xffffffff
        for mul in (0x6c50b47c, 0xb82f1e52, 0xc7afe638, 0x8d22f6e6):
            v ^= (v * mul) & 0xffffffff
        assert int(ow[j, d]) == rev(v)


def test_set_composition_and_layout_of_the_restatement():
    n, K, R, zdim = 2, 7, 3, 5
    for anti in (False, True):
        for cen in (False, True):
            bits, sign = ref.set_ints(n, K, R, zdim, antithetic=anti, center=cen, seed=3)
            c, H, B = ref.drawn_points(R * K, anti, cen)
            assert (c, B) == (int(cen), 21 - int(cen)) and H == ((B + 1) // 2 if anti else B)
            assert (sign[:, :c] == 0).all() and (sign[:, c:c + H] == 1).all() and (sign[:, c + H:] == -1).all() and sign.shape[1] - c - H == B - H
            assert (bits[:, :c] == 0).all() and (bits[:, c + H:] == 0).all()
            assert np.array_equal(bits[:, c:c + H], ref.point_ints(n, H, zdim, seed=3))
    x = np.arange(n * R * K * zdim).reshape(n, R * K, zdim)
    z = ref.to_rounds(x, K)
    assert z.shape == (R, n * K, zdim) and all((z[m // K, a * K + m % K] == x[a, m]).all() for a in range(n) for m in range(R * K))
    assert np.array_equal(ref.from_rounds(z, n, K), x)
    u = ref.uniforms(np.array([0, 2 ** 32 - 1, 2 ** 31], np.uint32))
    assert u[0] == 2.0 ** -33 and u[1] == 1.0 - 2.0 ** -33 and u[2] == 0.5 + 2.0 ** -33


def test_truncated_yardstick_is_the_formula_where_float64_can_evaluate_it():
    """latents_ref.quantiles(bits, t) against ndtri(ndtr(-t) + u (ndtr(t) - ndtr(-t))) evaluated as written: equal to 1e-9 relative where
    |z| >= 1e-3 (there the sum's rounding, 2^-53 absolute, is below that); its two branches agree at their seam; odd in u - 0.5; and for the
    raw sequence's point 1 (u - 0.5 = 2^-33) the as-written form is off by more than a float32 ulp while the yardstick is sqrt(2 pi) q."""
    x = np.random.default_rng(3).integers(0, 1 << 32, 200000, dtype=np.uint64).astype(np.uint32)
    for t in (0.01, 1.0, 2.5):
        tf = float(np.float32(t))
        lo, hi = (float(v) for v in torch.special.ndtr(torch.tensor([-tf, tf], dtype=torch.float64)))
        z = ref.quantiles(x, t)
        naive = np.clip(torch.special.ndtri(torch.from_numpy(lo + ref.uniforms(x) * (hi - lo))).numpy(), -tf, tf)
        far = np.abs(z) >= 1e-3
        assert far.sum() > 0.8 * x.size and (np.abs(z[far] - naive[far]) <= 1e-9 * np.abs(z[far])).all()
        assert (np.abs(z) <= tf).all() and (np.abs(ref.quantiles(~x, t) + z) <= 1e-12 * np.abs(z)).all()   # ~x: u -> 1 - u
        w = hi - lo
        seam = np.round((0.5 + np.array([1.0, -1.0]) * 2.0 ** -8 / w) * 2.0 ** 32 - 0.5).astype(np.int64)
        if t > 0.1:
            around = (seam[:, None] + np.arange(-3, 4)[None, :]).ravel().astype(np.uint32)
            zs = ref.quantiles(around, t)
            q = (ref.uniforms(around) - 0.5) * w
            assert (np.abs(q) >= 2.0 ** -8).any() and (np.abs(q) < 2.0 ** -8).any()
            assert (np.abs(zs / q - np.sqrt(2.0 * np.pi) * (1.0 + np.pi / 3.0 * q * q)) <= 1e-8).all()
            assert np.abs(np.diff(zs.reshape(2, 7), axis=1) / (np.sqrt(2 * np.pi) * w * 2.0 ** -32) - 1.0).max() <= 1e-3    # no jump across the seam
        mode = np.array([1 << 31], np.uint32)
        zm, q = ref.quantiles(mode, t)[0], 2.0 ** -33 * w
        assert abs(zm / (np.sqrt(2.0 * np.pi) * q) - 1.0) <= 1e-15
        nm = float(torch.special.ndtri(torch.tensor(lo + ref.uniforms(mode)[0] * w, dtype=torch.float64)))
        assert abs(nm - zm) > np.spacing(np.float32(zm))


def test_moments_of_the_random_kind_on_the_restatement():
    """The seed the GPU moment test uses: the restatement itself is within five standard errors of N(0, 1) there."""
    x = ref.point_ints(130, 64, 32, kind='random', seed=ref.MOMENT_SEED)
    z = ref.quantiles(x)
    N = z.size
    assert N == 130 * 64 * 32 and abs(z.mean()) <= 5 / np.sqrt(N) and abs(z.var() - 1.0) <= 5 * np.sqrt(2.0 / N)


# ----- the C ABI -----------------------------------------------------------------------------------------------------------------------

def test_entry_point_exported_declared_and_abi_version():
    from sttode_amd import capi
    from test_capi_symbols import header_functions
    fns, L = header_functions(), capi.lib()
    assert capi.ABI_VERSION == 15 and L.sttode_abi_version() == 15
    name = 'sttode_latent_set'
    assert name in fns and name in capi.SIGNATURES and hasattr(L, name)
    assert len(fns[name]) == len(capi.SIGNATURES[name]) == 15
    assert fns[name][7] == 'long long first_agent' and fns[name][8] == 'unsigned long long seed'
    assert ctypes.sizeof(capi.SIGNATURES[name][7]) == 8 and capi.SIGNATURES[name][8] is ctypes.c_ulonglong


def test_argument_checks_before_launch():
    """Every limit is refused by name (host logic only: nothing launches, and the sentinels behind z and bits stay)."""
    from sttode_amd import capi
    L = capi.lib()
    z = np.full(4 * 20 * 32, 7.25, np.float32)
    bits = np.full(4 * 20 * 32, -77, np.int32)
    dirs = np.zeros(32 * 30, np.uint32)
    order = ('z', 'bits', 'dirs', 'n', 'K', 'R', 'zdim', 'first_agent', 'seed', 'kind', 'scramble', 'antithetic', 'center', 'truncate')
    good = dict(z=z.ctypes.data, bits=bits.ctypes.data, dirs=dirs.ctypes.data, n=2, K=20, R=2, zdim=32, first_agent=0, seed=1, kind=0, scramble=2,
                antithetic=0, center=0, truncate=0.0)

    def R(match, **kw):
        a = {**good, **kw}
        rc = L.sttode_latent_set(*[a[k] for k in order], None)
        msg = L.sttode_last_error().decode()
        assert rc == 1 and msg.startswith('sttode_latent_set: ') and match in msg, (kw, rc, msg)
    R('null', z=None)
    R('n must be', n=0)
    R('n must be', n=-3)
    R('M = R K', K=0)
    R('M = R K', R=0)
    R('M = R K', K=-1)
    R('M = R K', K=65537, R=1)
    R('M = R K', K=257, R=256)                          # M = 65792
    R('M = R K', K=65536, R=65536)                      # the product does not wrap
    R('M = R K', K=1 << 20, R=1 << 12)
    R('zdim must be', zdim=0)
    R('zdim must be', zdim=1025)
    R('first_agent', first_agent=-1)
    R('kind must be', kind=2)
    R('kind must be', kind=-1)
    R('scramble must be', scramble=3)
    R('scramble must be', scramble=-1)
    R('0 or 1', antithetic=2)
    R('0 or 1', center=-1)
    for t in (-1.0, 0.009, float('inf'), float('-inf'), float('nan')):
        R('truncate must be', truncate=t)
    R('needs dirs', dirs=None)
    R('center needs', K=1, R=1, center=1)
    assert (z == 7.25).all() and (bits == -77).all()


# ----- the kernel's work items, run on the host -----------------------------------------------------------------------------------------

_HOST = {}


def _host_program(tmp_path_factory):
    """tests/latents_host.hip built once per process: the work items of csrc/latents.hip are host and device functions."""
    if 'exe' not in _HOST:
        import os
        import subprocess
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        d = tmp_path_factory.mktemp('latents_host')
        exe = str(d / 'latents_host')
        hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
        subprocess.run([hipcc, '-O2', '-std=c++17', '--offload-arch=gfx950', os.path.join(root, 'tests', 'latents_host.hip'), '-o', exe],
                       check=True, timeout=600)
        _HOST['exe'], _HOST['dir'] = exe, d
    return _HOST['exe'], _HOST['dir']


def _host_draw(tmp_path_factory, n, K, R, zdim, first_agent=0, seed=1, kind='sobol', scramble='owen', antithetic=False, center=False, truncate=0.0):
    import subprocess
    exe, d = _host_program(tmp_path_factory)
    dirs, out = str(d / ('dirs%d.bin' % zdim)), str(d / 'out')
    ref.directions(zdim).tofile(dirs)
    r = subprocess.run([exe, dirs, out] + [str(v) for v in (n, K, R, zdim, first_agent, seed, ref.KINDS[kind], ref.SCRAMBLES[scramble], int(antithetic),
                                                            int(center), truncate)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr)                    # 4: a guard word written; 5: an element left unwritten
    z = np.fromfile(out + '.z', np.float32).reshape(R, n * K, zdim)
    return z, np.fromfile(out + '.bits', np.uint32).reshape(R, n * K, zdim), int(r.stdout.split()[0])


def test_work_items_on_the_host_write_the_restatement_inside_their_bounds(tmp_path_factory):
    """The code the kernel runs per thread, looped over on the host between guard zones: every element written, none outside, the integers
    of the restatement, the values within a float32 ulp of the yardstick -- 16-byte and scalar stores, a chunk that starts past point 8
    (bit 2 of gray(j0) is bit 3 of j0), the 64-bit agent counter, the composition, the truncated raw sequence (u - 0.5 = 2^-33 at point 1)."""
    seed = 0x9e3779b97f4a7c15
    for (n, K, R, zdim), vec in (((3, 20, 1, 32), 1), ((9, 7, 3, 36), 1), ((2, 64, 1, 1), 0), ((2, 5, 2, 7), 0), ((1, 300, 1, 8), 1)):
        for kind, scramble in (('sobol', None), ('sobol', 'shift'), ('sobol', 'owen'), ('random', None)):
            fa = (1 << 32) + 3 if scramble == 'owen' else 5
            z, bits, v = _host_draw(tmp_path_factory, n, K, R, zdim, fa, seed, kind, scramble)
            want, _ = ref.set_ints(n, K, R, zdim, kind=kind, scramble=scramble, seed=seed, first_agent=fa)
            assert v == vec and np.array_equal(bits, ref.to_rounds(want, K)), (n, K, R, zdim, kind, scramble)
            zr = ref.quantiles(bits).astype(np.float32)
            assert (np.abs(z.astype(np.float64) - zr) <= np.spacing(np.abs(zr))).all() and np.abs(z).max() <= 6.34
    for M in (2, 3, 21):
        for anti in (False, True):
            for cen in (False, True):
                z, bits, _ = _host_draw(tmp_path_factory, 3, M, 1, 6, seed=77, antithetic=anti, center=cen)
                z0, _, _ = _host_draw(tmp_path_factory, 3, M, 1, 6, seed=77)
                c, H, B = ref.drawn_points(M, anti, cen)
                assert np.array_equal(bits[0].reshape(3, M, 6), ref.set_ints(3, M, 1, 6, antithetic=anti, center=cen, seed=77)[0])
                zs, z0s = z[0].reshape(3, M, 6), z0[0].reshape(3, M, 6)
                assert (zs[:, :c].view(np.uint32) == 0).all() and np.array_equal(zs[:, c:c + H], z0s[:, :H])
                assert np.array_equal(zs[:, c + H:].view(np.uint32), (-zs[:, c:c + B - H]).view(np.uint32))
    for t in (0.01, 2.5):
        z, bits, _ = _host_draw(tmp_path_factory, 9, 7, 3, 36, seed=seed, scramble=None, truncate=t)
        zr = ref.quantiles(bits, t).astype(np.float32)
        assert (np.abs(z.astype(np.float64) - zr) <= np.spacing(np.abs(zr))).all() and (np.abs(z) <= np.float32(t)).all()
        assert (bits[0, 1::7] == 1 << 31).all()                                                   # point 1 of every agent: the mode


# ----- the Python layer ----------------------------------------------------------------------------------------------------------------

def test_draw_refuses_bad_arguments_and_cpu_devices(monkeypatch):
    from sttode_amd import capi, latents
    monkeypatch.setattr(capi, 'call', lambda *a, **k: pytest.fail('a refused draw reached the library'))
    monkeypatch.setattr(torch, 'empty', lambda *a, **k: pytest.fail('a refused draw allocated'))
    for kw, match in ((dict(n=0), 'positive'), (dict(K=0), 'positive'), (dict(rounds=0), 'positive'), (dict(n=2.5), 'must be an int'),
                      (dict(K=True), 'must be an int'), (dict(K=4097, rounds=16), 'M = rounds'), (dict(zdim=0), 'zdim'), (dict(zdim=1025), 'zdim'),
                      (dict(first_agent=-1), 'first_agent'), (dict(first_agent=1 << 63), 'first_agent'), (dict(kind='halton'), 'kind'),
                      (dict(scramble='Owen'), 'scramble'), (dict(scramble=2), 'scramble'), (dict(seed=-1), 'seed'), (dict(seed=1 << 64), 'seed'),
                      (dict(seed=0.5), 'seed'), (dict(K=1, center=True), 'center'), (dict(truncate=0.0), 'truncate'), (dict(truncate=0.005), 'truncate'),
                      (dict(truncate=float('nan')), 'truncate'), (dict(truncate=float('inf')), 'truncate')):
        with pytest.raises(ValueError, match=match):
            latents.draw(**{**dict(n=3, K=20, zdim=32, seed=1, device='cpu'), **kw})
    with pytest.raises(capi.SttodeError, match='no CPU fallback'):
        latents.draw(3, 20, 32, seed=1, device='cpu')
    with pytest.raises(capi.SttodeError, match='no CPU fallback'):
        latents.draw(3, 20, 32, seed=1, device=torch.device('cpu'))
    with pytest.raises(ValueError, match='unknown options'):
        latents.LatentSource(20, 32, first_agent=3)
    with pytest.raises(ValueError, match='truncate'):
        latents.LatentSource(20, 32, truncate=0.001)
    with pytest.raises(ValueError, match='M = rounds'):
        latents.LatentSource(4097, 32, rounds=16)


def _stub_draw(log):
    """A stand-in for latents.draw: element [r, row, 0] = 1e6 first_agent + 1000 r + row, so a slice tells where it came from."""
    def draw(n, K, zdim, rounds=1, first_agent=0, **kw):
        log.append((n, K, zdim, rounds, first_agent, kw))
        z = torch.zeros(rounds, n * K, zdim)
        z[:, :, 0] = 1e6 * first_agent + 1000.0 * torch.arange(rounds)[:, None] + torch.arange(n * K)[None, :]
        return z[0] if rounds == 1 else z
    return draw


def test_latent_source_bookkeeping(monkeypatch):
    from sttode_amd import latents
    log = []
    monkeypatch.setattr(latents, 'draw', _stub_draw(log))
    torch.manual_seed(5)
    src = latents.LatentSource(4, 3, rounds=3, kind='sobol', antithetic=True)
    torch.manual_seed(5)
    assert src.options['seed'] == int(torch.empty((), dtype=torch.int64).random_()) & 0x7fffffffffffffff   # fixed once, from torch's generator
    assert latents.LatentSource(4, 3, seed=11).options['seed'] == 11
    # a group: `rounds` calls return the rounds of ONE draw, in round order; first_agent advances by n behind it
    got = [src(8) for _ in range(3)]
    assert [tuple(g.shape) for g in got] == [(8, 3)] * 3 and [float(g[5, 0]) for g in got] == [5.0, 1005.0, 2005.0]
    assert len(log) == 1 and log[0][:5] == (2, 4, 3, 3, 0) and log[0][5] == dict(kind='sobol', antithetic=True, seed=src.options['seed'])
    got = [src(20) for _ in range(3)]                                        # another batch size: agents 2 .. 6
    assert [float(g[19, 0]) for g in got] == [2e6 + 19, 2e6 + 1019, 2e6 + 2019] and log[1][:5] == (5, 4, 3, 3, 2) and src.first_agent == 7
    # rows that change inside a group, rows that are no multiple of K
    src(8)
    with pytest.raises(ValueError, match='rows changed'):
        src(12)
    with pytest.raises(ValueError, match='open group'):
        src.draw_rounds(2)
    assert float(src(8)[0, 0]) == 7e6 + 1000 and float(src(8)[0, 0]) == 7e6 + 2000 and src.first_agent == 9      # the group goes on
    for bad in (0, 7, -4):
        with pytest.raises(ValueError, match='multiple of K'):
            src(bad)
    assert src.first_agent == 9 and len(log) == 3
    # draw_rounds: the whole set, advances; reset rewinds
    z = src.draw_rounds(3)
    assert tuple(z.shape) == (3, 12, 3) and float(z[2, 11, 0]) == 9e6 + 2011 and src.first_agent == 12
    src(4)
    src.reset()
    assert src.first_agent == 0 and float(src(8)[0, 0]) == 0.0 and log[-1][:5] == (2, 4, 3, 3, 0)
    # rounds = 1: every call is a draw of its own; K = 1 gives the [n, zdim] an eps_fn is asked for
    one = latents.LatentSource(1, 6, seed=2)
    assert tuple(one(5).shape) == (5, 6) and tuple(one(1).shape) == (1, 6) and one.first_agent == 6 and log[-1][:5] == (1, 1, 6, 1, 5)
    assert tuple(one.draw_rounds(2).shape) == (1, 2, 6)


# ----- the model -----------------------------------------------------------------------------------------------------------------------

class _Source:
    """A stand-in for latents.LatentSource that records how it is asked."""

    def __init__(self, log, K=20, zdim=32, rounds=1):
        self.log, self.K, self.zdim, self.rounds = log, K, zdim, rounds

    def __call__(self, rows):
        self.log.append(('source', rows))
        return torch.full((rows, self.zdim), 0.5)

    def draw_rounds(self, n):
        self.log.append(('draw_rounds', n))
        return torch.arange(self.rounds, dtype=torch.float32)[:, None, None].expand(self.rounds, n * self.K, self.zdim).contiguous()


def _recorded_model(monkeypatch, log):
    """STTODENet on the CPU with the device taken away underneath it: capi.call, torch.randn and the reduction record into ``log``."""
    from helpers import make_args
    from sttode_amd import STTODENet, capi, metrics
    m = STTODENet(make_args(), 'cpu').eval()
    m.set_data(None, torch.zeros(3, 2, 8), torch.zeros(3, 2, 12))
    nat = types.SimpleNamespace(h=None, timeout_word=types.SimpleNamespace(value=0), raise_if_timed_out=lambda: None,
                                layout=lambda n, S: ({}, 8), init_workspace=lambda buf, n, S: None)
    m._require_gpu = lambda: None
    m.native = lambda check_weights=True: nat
    m._workspace = lambda n, S: (torch.zeros(8), {'scene_orig': 0})
    m.next_async_stream = lambda n: None

    def call(name, *a, **k):
        opts = capi.AsyncOpts.from_address(a[-2]) if name.endswith('_async') else None
        z = a[5]
        log.append((name, None if opts is None else int(opts.device_latents), tuple(z.shape), float(z.flatten()[0]) if opts is None or not opts.device_latents else None))
    real_randn = torch.randn

    def randn(*shape, **kw):
        log.append(('randn',) + tuple(shape))
        return real_randn(*shape, **kw)
    monkeypatch.setattr(capi, 'call', call)
    monkeypatch.setattr(capi, 'TIMING', [])                    # (inference() then launches through capi.call)
    monkeypatch.setattr(capi, 'stream_ptr', lambda: None)
    monkeypatch.setattr(capi, 'lib', lambda: types.SimpleNamespace(sttode_async_is_lagged=lambda h, n: 1))
    monkeypatch.setattr(torch, 'randn', randn)
    monkeypatch.setattr(metrics, 'reduce_samples', lambda buf, K, **kw: (log.append(('reduce_samples', tuple(buf.shape), K)),
                                                                         types.SimpleNamespace(centroids=torch.zeros(buf.shape[1], K, 12, 2)))[1])
    return m


def test_latent_source_unset_makes_the_calls_made_before_and_set_replaces_the_draw(monkeypatch):
    from sttode_amd import STTODENet, capi
    assert STTODENet.latent_source is None and 'latent_source' not in STTODENet.__init__.__code__.co_varnames
    log = []
    m = _recorded_model(monkeypatch, log)
    assert m.latent_source is None and 'latent_source' not in m.state_dict()

    def run(f):
        del log[:]
        f()
        return [e if e[0] in ('randn', 'source', 'draw_rounds', 'reduce_samples') else e[:3] for e in log], list(log)
    serial, asyn = ('sttode_inference_scenes', None, (60, 32)), 'sttode_inference_scenes_async'
    default = {}
    for unset in (False, True):                                 # never set, and cleared after use
        if unset:
            m.latent_source = _Source(log)
            m.inference(None)
            m.latent_source = None
        default['inference'] = run(lambda: m.inference(None))[0]
        assert default['inference'] == [('randn', 60, 32), serial]
        assert run(lambda: m.inference_async())[0] == [(asyn, 1, (60, 32))]                       # the launch draws: device_latents armed
        m.device_latents = False
        assert run(lambda: m.inference_async())[0] == [('randn', 60, 32), (asyn, 0, (60, 32))]
        m.device_latents = True
        assert run(lambda: m.inference_reduced(2))[0] == [('randn', 60, 32), serial] * 2 + [('reduce_samples', (2, 3, 20, 12, 2), 20)]
        z = torch.full((60, 32), 3.0)
        assert run(lambda: m.inference(None, z=z))[1] == [serial + (3.0,)]
    # set: the source is asked instead, its tensor is what the launch gets, nothing else changes
    m.latent_source = _Source(log)
    assert run(lambda: m.inference(None))[1] == [('source', 60), serial + (0.5,)]
    assert run(lambda: m.inference_async())[1] == [('source', 60), (asyn, 0, (60, 32), 0.5)]
    assert run(lambda: m.inference(None, z=z))[1] == [serial + (3.0,)]                            # an explicit z wins
    assert run(lambda: m.inference_async(z=z))[1] == [(asyn, 0, (60, 32), 3.0)]
    m.latent_source = _Source(log, rounds=3)
    assert run(lambda: m.inference_reduced(3))[1] == [('draw_rounds', 3), serial + (0.0,), serial + (1.0,), serial + (2.0,),
                                                      ('reduce_samples', (3, 3, 20, 12, 2), 20)]
    # a source built for another K, zdim or rounds: refused before any launch or slot
    calls = m._async_calls
    for src, f in ((_Source(log, K=19), lambda: m.inference(None)), (_Source(log, zdim=16), lambda: m.inference_async()),
                   (_Source(log, rounds=3), lambda: m.inference_reduced(2)), (_Source(log, K=5, rounds=2), lambda: m.inference_reduced(2))):
        m.latent_source = src
        del log[:]
        with pytest.raises(ValueError, match='latent_source is built for'):
            f()
        assert log == [] and m._async_calls == calls
    # a call refused for another argument has not asked the source either
    m.latent_source = _Source(log)
    del log[:]
    with pytest.raises(ValueError, match='metrics_gt'):
        m.inference_async(metrics_gt=torch.zeros(3, 12, 2))
    assert log == [] and m._async_calls == calls
    # a sampler plan fills z itself: refused together with a source, like z
    with pytest.raises(capi.SttodeError, match='sampler plan'):
        m.inference_async(sampler_plan=capi.SamplerPlan())
    assert log == [] and m._async_calls == calls
