"""Direct float64 tests of the inference stage kernels (csrc/frontend.hip, encoder.hip, decoder.hip, chain32.hip): every stage entry
point through capi.call at the sizes its code branches on, and the forms that have no entry point of their own (the per-agent roles, the
latency bodies, the one-launch scene form, the fused and the lagged launches) through STTODENet.

References: tests/inference_ref.py (pinned on the CPU by tests/test_inference_ref.py) in float64 and in torch fp32, both evaluated on the
very fp32 values the kernel received.  Yardstick of one stage (tests/train_ref.py, unchanged):
    |hip - f64| <= max(4 |torch_fp32 - f64|, 1e-6 max|f64| + 1e-5 |f64|)   per element.
Chained launches (sttode_traj_chain, the model-level forms: the output lies many stages behind the inputs) take the tensor-wide maximum
of |torch_fp32 - f64| in the first term: the rounding errors of two correct fp32 evaluations of a deep chain are not aligned element by
element.  No bound in this file comes from what a kernel returned.

Relations that hold exactly are bitwise: front-end outputs that are copies or single subtractions, sttode_ode_state_to_pf, grouped
against single attention launches, the latency against the throughput form of a stage (include/sttode_hip.h: "results are bitwise
independent of the setting"), a case run twice.  Every output is a slice of a larger buffer with guard rows (and guard columns where the
leading dimension exceeds the width) of sentinels around a payload that starts as NaN: a guard that changes, or an element left NaN,
fails.  A refusal passes only arguments the host-side STT_REQUIRE rejects before any launch, and then checks the outputs untouched.

sttode_set_latency_tiles is process-wide: the ``tiles`` fixture forces the throughput kernels with (0, 0, 0) and restores the defaults
(512, 1024, 1024); RAN counts, per stage, the forms the host-side rule actually selected."""
import collections
import functools

import numpy as np
import pytest
import torch

import inference_ref as I

from test_train_kernels_gpu import _capi, _close, _gpu, _worst
from test_trunk_ode_kernels_gpu import GUARD, _Buf, _biteq, _check

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
DEFAULT_TILES = (512, 1024, 1024)
RAN = collections.Counter()                  # (stage, 'latency' | 'throughput') -> launches
ISENT, IUNSET = 123456, -7                   # sentinel / "not written" of the int32 outputs


# ---------------------------------------------------------------------------------------------------------------------------------------
# plumbing
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def tiles():
    """use('latency' | 'throughput'): the process-wide crossover of the stage kernels; the defaults come back whatever happens."""
    capi = _capi()

    def use(form):
        capi.call('sttode_set_latency_tiles', *(DEFAULT_TILES if form == 'latency' else (0, 0, 0)))
        return form
    try:
        yield use
    finally:
        capi.call('sttode_set_latency_tiles', *DEFAULT_TILES)


def _ran(stage, setting, ntiles, lat_ok=True):
    """Counts the form the host selects (csrc/decoder.hip, encoder.hip: the latency kernel serves ntiles <= the stage's crossover)."""
    limit = dict(gru=DEFAULT_TILES[0], mlp=DEFAULT_TILES[1], enc=DEFAULT_TILES[2])[stage.split(':')[1]] if setting == 'latency' else 0
    form = 'latency' if (ntiles <= limit and lat_ok) else 'throughput'
    RAN[(stage.split(':')[0], form)] += 1
    return form


class _IBuf:
    """int32 counterpart of _Buf: [rows] payload (IUNSET) between GUARD sentinels on each side."""

    def __init__(self, dev, rows):
        self.rows = rows
        self.buf = torch.full((rows + 2 * GUARD,), ISENT, dtype=torch.int32, device=dev)
        self.v = self.buf[GUARD:GUARD + rows]
        self.v[:] = IUNSET

    def get(self, what=''):
        b = self.buf.cpu()
        assert bool((b[:GUARD] == ISENT).all() and (b[GUARD + self.rows:] == ISENT).all()), f'{what}: a sentinel around the output changed'
        p = b[GUARD:GUARD + self.rows].clone()
        assert not bool((p == IUNSET).any()), f'{what}: {int((p == IUNSET).sum())} elements were not written'
        return p

    def untouched(self):
        b = self.buf.cpu()
        return bool((b[:GUARD] == ISENT).all() and (b[GUARD + self.rows:] == ISENT).all() and (b[GUARD:GUARD + self.rows] == IUNSET).all())


def _d(dev, a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t.to(dtype) if dtype is not None else t).to(dev)


def _T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _chain_close(got, f64, f32, what):
    """The chained yardstick: 4 x the tensor-wide max |torch_fp32 - f64| in place of the element's own."""
    f64 = f64.double().reshape(got.shape)
    spread = float((f32.double().reshape(got.shape) - f64).abs().max())
    return _close(got, f64, f64 + spread, what)


def _refuses(fn, match):
    capi = _capi()
    with pytest.raises(capi.SttodeError, match=match):
        fn()


_DEVPACK = {}


class _Packs:
    """model.py's recipe (STTODENet.packed): pack_trunk / pack_block / chain_stream of the seed's weights as device tensors, each group
    packed on first use."""

    def __init__(self, dev, Tp, Tf, seed):
        self.dev, self.Tp, self.Tf, self.seed, self.groups = dev, Tp, Tf, seed, {}

    def __getitem__(self, g):
        from sttode_amd import packing
        if g not in self.groups:
            sd = I.nets(self.seed, self.Tp, self.Tf)['sd']
            host = {'past': lambda: packing.pack_trunk(sd, 'past_encoder.', self.Tp),
                    'blk0': lambda: packing.pack_block(sd, 0, self.Tp, self.Tf, first=True),
                    'blk1': lambda: packing.pack_block(sd, 1, self.Tp, self.Tf, first=False),
                    'chain': lambda: packing.chain_stream(sd, self.Tp, self.Tf)}[g]()
            self.groups[g] = {k: (_d(self.dev, v) if isinstance(v, np.ndarray) else v) for k, v in host.items()}
        return self.groups[g]


def _packs(dev, Tp, Tf, seed=1234):
    return _DEVPACK.setdefault((str(dev), Tp, Tf, seed), _Packs(dev, Tp, Tf, seed))


# ---------------------------------------------------------------------------------------------------------------------------------------
# front-end
# ---------------------------------------------------------------------------------------------------------------------------------------
def _sizes(S, seed):
    return [int(v) for v in np.random.default_rng(seed).integers(1, 5, S)]


# (agents per scene, Tp, vel_from_norm): S = 1, 3, 16 (single workgroup), 17 and n = 1025 (two launches); scenes of one agent
FE_CASES = [((7,), 8, 1), ((1,), 8, 0), ((1, 5, 1), 5, 1), (tuple(_sizes(16, 1)), 8, 0), (tuple(_sizes(17, 2)), 10, 1),
            (tuple(_sizes(17, 3)), 8, 0), ((400, 1, 300, 324), 8, 1), ((2, 1), 10, 0)]
_feid = lambda c: 'S%d-n%d-Tp%d-vel%d' % (len(c[0]), sum(c[0]), c[1], c[2])


def _sub32(a, b):
    return (np.asarray(a, np.float32) - np.asarray(b, np.float32)).astype(np.float32)


@pytest.mark.parametrize('c', FE_CASES, ids=_feid)
def test_frontend_scenes_vs_float64(c):
    dev, capi = _gpu(), _capi()
    sizes, Tp, vel = c
    past, _, ptr = I.scene_case(list(sizes), Tp, 12, seed=len(sizes))
    n, S, TPX = past.shape[0], len(sizes), I.tiles_x(Tp)
    r64, r32 = I.frontend_scenes(past, ptr, vel, np.float64), I.frontend_scenes(past, ptr, vel, np.float32)
    out = dict(scene_orig=_Buf(dev, S, 2), xpad=_Buf(dev, n, 16 * TPX), enc_in=_Buf(dev, n, 4 * Tp), cur=_Buf(dev, n, 2), orig=_Buf(dev, n, 2))
    iout = dict(agent_scene=_IBuf(dev, n), last=_IBuf(dev, n))
    runs = []
    for _ in range(2):
        capi.call('sttode_frontend_scenes', _d(dev, past), _d(dev, ptr), n, S, Tp, TPX, vel, out['scene_orig'].v, iout['agent_scene'].v,
                  out['xpad'].v, out['enc_in'].v, out['cur'].v, out['orig'].v, iout['last'].v, capi.stream_ptr())
        torch.cuda.synchronize()
        runs.append({k: b.get(f'{_feid(c)} {k}') for k, b in list(out.items()) + list(iout.items())})
    got = runs[0]
    for k in got:
        assert torch.equal(got[k], runs[1][k]), f'{k}: two runs differ'
    worst = {k: _check(k, got[k], _T(r64[k]), _T(r32[k]), 'frontend_scenes ' + _feid(c)) for k in out}
    k = max(worst, key=worst.get)
    _worst(f'frontend_scenes {_feid(c)} (at {k})', worst[k])
    assert got['agent_scene'].tolist() == r64['agent_scene'].tolist() and got['last'].tolist() == r64['last'].tolist()
    # copies and single subtractions of the kernel's own scene origin
    so = got['scene_orig'].numpy()
    orig = so[r64['agent_scene']]
    _biteq(got['orig'], _T(orig), 'orig = scene_orig[agent_scene]')
    norm = _sub32(past, orig[:, None, :])
    xp = np.zeros((n, 16 * TPX), np.float32)
    xp[:, :2 * Tp] = norm.reshape(n, 2 * Tp)
    _biteq(got['xpad'], _T(xp), 'xpad = past - orig, zero padded')
    enc = got['enc_in'].reshape(n, Tp, 4)
    _biteq(enc[..., :2].contiguous(), _T(norm), 'enc_in[..., :2] = past - orig')
    _biteq(got['cur'], _T(norm[:, -1]), 'cur = the last normalised frame')
    src = norm if vel else past
    v = _sub32(src[:, 1:], src[:, :-1])
    _biteq(enc[..., 2:].contiguous(), _T(np.concatenate([v[:, :1], v], axis=1)), 'velocities: one subtraction each, the first duplicated')


@pytest.mark.parametrize('B,N,Tp', [(1, 10, 5), (3, 11, 5), (1, 11, 10), (3, 10, 8)])
def test_frontend_nba_vs_float64(B, N, Tp):
    dev, capi = _gpu(), _capi()
    past, _ = I.nba_case(B, N, Tp, 10)
    n, TPX = B * N, I.tiles_x(Tp)
    r64 = I.frontend_nba(past, N)
    out = dict(xpad=_Buf(dev, n, 16 * TPX), enc_in=_Buf(dev, n, 4 * Tp), cur=_Buf(dev, n, 2), orig=_Buf(dev, n, 2))
    last = _IBuf(dev, n)
    capi.call('sttode_frontend_nba', _d(dev, past), n, N, Tp, TPX, out['xpad'].v, out['enc_in'].v, out['cur'].v, out['orig'].v, last.v,
              capi.stream_ptr())
    torch.cuda.synchronize()
    got = {k: b.get(f'frontend_nba {k}') for k, b in out.items()}
    r32 = I.frontend_nba(past, N, np.float32)
    _worst(f'frontend_nba B{B} N{N} Tp{Tp}', max(_check(k, got[k], _T(r64[k]), _T(r32[k]), 'frontend_nba') for k in out))
    for k in out:                                           # copies, zeros and single subtractions: the fp32 restatement's bits
        _biteq(got[k], _T(r32[k]).reshape(got[k].shape), f'frontend_nba {k}')
    assert last.get('last').tolist() == r64['last'].tolist()


@pytest.mark.parametrize('mode', [0, 1], ids=['scenes', 'nba'])
@pytest.mark.parametrize('Tf', [10, 12, 40])
def test_frontend_future_vs_float64(mode, Tf):
    dev, capi = _gpu(), _capi()
    if mode == 0:
        past, fut, ptr = I.scene_case([1, 6, 130, 3], 8, Tf, seed=Tf)
        fe = I.frontend_scenes(past, ptr, 0, np.float32)
        so, ags = fe['scene_orig'], fe['agent_scene']
    else:
        past, fut = I.nba_case(13, 11, 5, Tf)
        so = ags = ptr = None
    n = past.shape[0]
    last_past = np.ascontiguousarray(past[:, -1])
    enc = _Buf(dev, n, 4 * Tf)
    capi.call('sttode_frontend_future', _d(dev, fut), _d(dev, last_past), n, Tf, mode, 11 if mode else 1, None if mode else _d(dev, so),
              None if mode else _d(dev, ags), None if mode else _d(dev, ptr), enc.v, capi.stream_ptr())
    torch.cuda.synchronize()
    got = enc.get('frontend_future')
    r64 = I.frontend_future(fut, last_past, mode, so, ags)
    r32 = I.frontend_future(fut, last_past, mode, so, ags, np.float32)
    _worst(f'frontend_future mode {mode} Tf {Tf}', _check('enc_in', got, _T(r64), _T(r32), 'frontend_future'))
    _biteq(got, _T(r32).reshape(got.shape), 'frontend_future: one subtraction per element')
    if mode == 0:
        _refuses(lambda: capi.call('sttode_frontend_future', _d(dev, fut), _d(dev, last_past), n, Tf, 0, 1, None, None, None, enc.v,
                                   capi.stream_ptr()), 'bad arguments')


@pytest.mark.parametrize('n,Tp,Tf', [(1, 8, 0), (6, 8, 12), (300, 10, 40), (5, 5, 0)])
def test_rotate_scene_vs_float64(n, Tp, Tf):
    dev, capi = _gpu(), _capi()
    past, fut, _ = I.scene_case([n], Tp, max(Tf, 1), seed=3)
    fut = fut if Tf else None
    c, s = float(np.cos(np.float32(0.7))), float(np.sin(np.float32(0.7)))
    p, f = _Buf(dev, n, 2 * Tp), (_Buf(dev, n, 2 * Tf) if Tf else None)
    p.v.copy_(_d(dev, past.reshape(n, -1)))
    if Tf:
        f.v.copy_(_d(dev, fut.reshape(n, -1)))
    capi.call('sttode_rotate_scene', p.v, f.v if Tf else None, n, Tp, Tf, c, s, capi.stream_ptr())
    torch.cuda.synchronize()
    r64, r32 = I.rotate_scene(past, fut, np.float32(c), np.float32(s)), I.rotate_scene(past, fut, c, s, np.float32)
    w = _check('past', p.get('rotate past'), _T(r64[0]), _T(r32[0]), 'rotate_scene')
    if Tf:
        w = max(w, _check('fut', f.get('rotate fut'), _T(r64[1]), _T(r32[1]), 'rotate_scene'))
    _worst(f'rotate_scene n{n} Tp{Tp} Tf{Tf}', w)


def test_frontend_refusals_write_nothing():
    dev, capi = _gpu(), _capi()
    past, _, ptr = I.scene_case([3, 2], 8, 12)
    outs = [_Buf(dev, 2, 2), _IBuf(dev, 5), _Buf(dev, 5, 16), _Buf(dev, 5, 32), _Buf(dev, 5, 2), _Buf(dev, 5, 2), _IBuf(dev, 5)]
    args = lambda Tp, TPX: (_d(dev, past), _d(dev, ptr), 5, 2, Tp, TPX, 1) + tuple(o.v for o in outs) + (capi.stream_ptr(),)
    _refuses(lambda: capi.call('sttode_frontend_scenes', *args(10, 1)), '2\\*Tp <= 16\\*TPX')
    _refuses(lambda: capi.call('sttode_frontend_scenes', *args(1, 1)), 'Tp >= 2')
    _refuses(lambda: capi.call('sttode_frontend_nba', _d(dev, past), 5, 2, 8, 1, outs[2].v, outs[3].v, outs[4].v, outs[5].v, outs[6].v,
                               capi.stream_ptr()), 'n % N == 0')
    torch.cuda.synchronize()
    assert all(o.untouched() for o in outs)


# ---------------------------------------------------------------------------------------------------------------------------------------
# embedding + in-projection
# ---------------------------------------------------------------------------------------------------------------------------------------
# every n at Tlen 8 (16-agent tiles, 64-agent workgroups of the throughput form), every Tlen at n = 17 (14 is the longest the latency
# form's LDS takes: (Tlen 256 + 512) 16 <= 64 KiB; 15 and 16 fall back to the throughput kernel), the three flag patterns
EMBED_CASES = ([(n, 8, 'ragged') for n in (1, 15, 16, 17, 63, 64, 65)] + [(17, T_, 'ragged') for T_ in (2, 5, 10, 14, 15, 16)]
               + [(17, 8, 'none'), (17, 8, 'all'), (65, 16, 'all'), (1, 2, 'all')])
_emid = lambda c: 'n%d-T%d-%s' % c


@functools.lru_cache(maxsize=None)
def _embed_refs(n, Tlen, flags):
    c = I.embed_case(n, Tlen, flags)
    with torch.no_grad():
        return c, I.embed_qkv(I.nets(1234, Tlen, 12)['f64'].past_encoder, c['enc_in'], c['last']), \
            I.embed_qkv(I.nets(1234, Tlen, 12)['f32'].past_encoder, c['enc_in'], c['last'])


def _embed_run(dev, c, W):
    capi = _capi()
    g, qkv = _Buf(dev, c['n'], 64), _Buf(dev, c['n'], 192)
    capi.call('sttode_embed_qkv', W['fc1P'], W['fc1b'], W['posP'], W['peb'], W['fc2P'], W['fc2b'], W['fc3P'], W['fc3b'], W['fc3last'],
              W['inP'], W['inb'], _d(dev, c['enc_in']), _d(dev, c['last']), g.v, qkv.v, c['n'], c['Tlen'], capi.stream_ptr())
    torch.cuda.synchronize()
    return dict(g=g.get('embed g'), qkv=qkv.get('embed qkv'))


@pytest.mark.parametrize('c', EMBED_CASES, ids=_emid)
def test_embed_qkv_vs_float64_both_forms(c, tiles):
    dev = _gpu()
    n, Tlen, flags = c
    case, r64, r32 = _embed_refs(n, Tlen, flags)
    W = _packs(dev, Tlen, 12)['past']
    got, forms = {}, set()
    for setting in ('latency', 'throughput'):
        tiles(setting)
        forms.add(_ran('embed_qkv:enc', setting, (n + 15) // 16, (Tlen * 256 + 512) * 16 <= 64 * 1024))
        got[setting] = _embed_run(dev, case, W)
        w = max(_check(k, got[setting][k], r64[k], r32[k], f'embed_qkv {_emid(c)} {setting}') for k in ('g', 'qkv'))
        _worst(f'embed_qkv {_emid(c)} {setting} setting', w)
    assert forms == ({'latency', 'throughput'} if Tlen <= 14 else {'throughput'})
    for k in ('g', 'qkv'):
        _biteq(got['latency'][k], got['throughput'][k], f'embed_qkv {k}: latency against throughput form')


# ---------------------------------------------------------------------------------------------------------------------------------------
# geodesic attention
# ---------------------------------------------------------------------------------------------------------------------------------------
class _Attn:
    """Operands of one attention problem (or `groups` of them) in the model's strided q | k | v layout (rows = keys: R at + 8 hd, C at 0,
    V at + 16 hd of rows of 24 hd floats) or contiguous [len, Nb, 8 hd] tensors, and guarded outputs with a padded row stride."""

    def __init__(self, dev, rows, cols, Nb, layout, hd=8, groups=1, seed=0):
        E = 8 * hd
        self.rows, self.cols, self.Nb, self.hd, self.groups, self.E = rows, cols, Nb, hd, groups, E
        rng = np.random.default_rng(1000 * rows + 10 * cols + Nb + seed)
        mk = lambda l: rng.standard_normal((groups, l, Nb, E)).astype(np.float32)
        self.R, self.C, self.V = mk(rows), mk(cols), mk(cols)
        if layout == 'model':
            a = rng.standard_normal((groups, rows, Nb, 3 * E)).astype(np.float32)
            b = rng.standard_normal((groups, cols, Nb, 3 * E)).astype(np.float32)
            a[..., E:2 * E], b[..., :E], b[..., 2 * E:] = self.R, self.C, self.V
            self.da, self.db = _d(dev, a), _d(dev, b)
            e = 4
            self.ptr = (self.da.data_ptr() + E * e, self.db.data_ptr(), self.db.data_ptr() + 2 * E * e)
            self.strides = (Nb * 3 * E, 3 * E, Nb * 3 * E, 3 * E, Nb * 3 * E, 3 * E)
            self.gs = (rows * Nb * 3 * E, cols * Nb * 3 * E, cols * Nb * 3 * E)
        else:
            self.dR, self.dC, self.dV = _d(dev, self.R), _d(dev, self.C), _d(dev, self.V)
            self.ptr = (self.dR.data_ptr(), self.dC.data_ptr(), self.dV.data_ptr())
            self.strides = (Nb * E, E, Nb * E, E, Nb * E, E)
            self.gs = (rows * Nb * E, cols * Nb * E, cols * Nb * E)
        self.ld = Nb * E + 8                                               # output rows padded: the pad columns are guards
        self.dev = dev

    def out_buf(self):
        return _Buf(self.dev, self.groups * self.rows, self.Nb * self.E, self.ld)

    def refs(self, g=0):
        sc = float(self.hd) ** -0.5
        with torch.no_grad():
            return tuple(I.attention(_T(self.R[g]).to(dt), _T(self.C[g]).to(dt), _T(self.V[g]).to(dt), 1.0, sc, self.hd) for dt in (F64, F32))

    def single(self, g=0, rowsum=None, wout=None):
        capi = _capi()
        out = _Buf(self.dev, self.rows, self.Nb * self.E, self.ld)
        p = [q + 4 * g * s for q, s in zip(self.ptr, self.gs)]
        capi.call('sttode_mhgsa_attn', p[0], p[1], p[2], out.v, rowsum, wout, self.rows, self.cols, self.Nb, *self.strides, self.ld, self.E,
                  1.0, float(self.hd) ** -0.5, capi.stream_ptr())
        torch.cuda.synchronize()
        return out

    def grouped(self, groups=None, hd=None):
        capi = _capi()
        out = self.out_buf()
        capi.call('sttode_mhgsa_attn_groups', *self.ptr, out.v, self.groups if groups is None else groups, *self.gs, self.rows * self.ld,
                  self.rows, self.cols, self.Nb, *self.strides, self.ld, self.E, 1.0, float(self.hd) ** -0.5, self.hd if hd is None else hd,
                  capi.stream_ptr())
        torch.cuda.synchronize()
        return out


# rows 1 / 63 / 64 / 65 (64-row workgroups), cols 1 / 127 / 128 / 129 / 257 (ATT_TJ = 128), rows != cols, Nb 1 / 11, both layouts
ATTN_CASES = [(1, 1, 1, 'model'), (63, 127, 1, 'contig'), (64, 128, 11, 'model'), (65, 129, 1, 'contig'), (65, 257, 1, 'model'),
              (1, 257, 11, 'contig'), (64, 1, 1, 'model'), (17, 17, 11, 'model'), (129, 65, 1, 'contig')]
_atid = lambda c: 'r%d-c%d-Nb%d-%s' % c


@pytest.mark.parametrize('c', ATTN_CASES, ids=_atid)
def test_mhgsa_attn_vs_float64(c):
    dev = _gpu()
    rows, cols, Nb, layout = c
    a = _Attn(dev, rows, cols, Nb, layout)
    r64, r32 = a.refs()
    rs, wo = _Buf(dev, Nb * 8, rows), _Buf(dev, Nb * rows, cols)
    full = a.single(0, rs.v, wo.v)
    got = full.get('attn out')
    worst = dict(out=_check('out', got, r64['out'], r32['out'], 'mhgsa_attn ' + _atid(c)),
                 rowsum=_check('rowsum', rs.get('rowsum'), r64['rowsum'], r32['rowsum'], 'mhgsa_attn ' + _atid(c)),
                 weights=_check('weights', wo.get('weights'), r64['weights'], r32['weights'], 'mhgsa_attn ' + _atid(c)))
    k = max(worst, key=worst.get)
    _worst(f'mhgsa_attn {_atid(c)} (at {k})', worst[k])
    # the optional outputs do not change the result; a second run gives the same bits; one group of the grouped entry point likewise
    rs2 = _Buf(dev, Nb * 8, rows)
    _biteq(a.single(0, rs2.v, None).get('rowsum only'), got, 'rowsum given, weights null')
    _biteq(rs2.get('rowsum'), rs.get('rowsum'), 'rowsum of the two calls')
    _biteq(a.single().get('both null'), got, 'rowsum and weights null')
    _biteq(a.grouped().get('one group'), got, 'sttode_mhgsa_attn_groups with one group')


@pytest.mark.parametrize('hd', [4, 8, 16])
@pytest.mark.parametrize('layout', ['model', 'contig'])
def test_mhgsa_attn_groups_vs_float64_and_single_launches(hd, layout):
    dev = _gpu()
    rows, cols, Nb = (65, 65, 3) if layout == 'model' else (33, 129, 2)
    a = _Attn(dev, rows, cols, Nb, layout, hd=hd, groups=3)
    got = a.grouped().get('groups').reshape(3, rows, Nb * a.E)
    w = 0.0
    for g in range(3):
        r64, r32 = a.refs(g)
        w = max(w, _check(f'group {g}', got[g], r64['out'], r32['out'], f'mhgsa_attn_groups hd {hd} {layout}'))
        if hd == 8:
            _biteq(a.single(g).get('single'), got[g].contiguous(), f'group {g} against the single launch')
    _worst(f'mhgsa_attn_groups hd {hd} {layout}', w)
    _biteq(a.grouped().get('again').reshape(got.shape), got, 'a second grouped launch')
    # groups = 1 of the same operands: the first group's bits, the other groups' rows untouched
    one = a.out_buf()
    capi = _capi()
    capi.call('sttode_mhgsa_attn_groups', *a.ptr, one.v, 1, *a.gs, rows * a.ld, rows, cols, Nb, *a.strides, a.ld, a.E, 1.0, float(hd) ** -0.5, hd,
              capi.stream_ptr())
    torch.cuda.synchronize()
    assert one.sentinels_ok() and bool(torch.isnan(one.v[rows:, :Nb * a.E]).all())
    _biteq(one.v[:rows, :Nb * a.E].cpu().contiguous(), got[0].contiguous(), 'groups = 1')


def test_mhgsa_attn_refusals_write_nothing():
    dev, capi = _gpu(), _capi()
    a = _Attn(dev, 5, 5, 2, 'contig')
    out, wo = a.out_buf(), _Buf(dev, 2 * 5, 5)
    _refuses(lambda: capi.call('sttode_mhgsa_attn_groups', *a.ptr, out.v, 1, *a.gs, 5 * a.ld, 5, 5, 2, *a.strides, a.ld, 64, 1.0, 0.35, 5,
                               capi.stream_ptr()), 'head_dim must be 4, 8 or 16')
    _refuses(lambda: capi.call('sttode_mhgsa_attn', *a.ptr, out.v, None, wo.v, 5, 5, 2, *a.strides, a.ld, 64, 1.0, 0.35, capi.stream_ptr()),
             'needs the rowsum workspace')
    torch.cuda.synchronize()
    assert out.untouched() and wo.untouched()


# ---------------------------------------------------------------------------------------------------------------------------------------
# post-attention layer
# ---------------------------------------------------------------------------------------------------------------------------------------
POST_W = ('outP', 'outb', 'infoP', 'infob', 'gateP', 'gateb', 'ln1w', 'ln1b', 'l1P', 'l1b', 'l2P', 'l2b', 'ln2w', 'ln2b')


@functools.lru_cache(maxsize=None)
def _post_case(n, ld):
    """g, the attention operand at row stride ld (192: the model's qkv rows, value part; 64: a seeded stand-alone tensor) and references."""
    c = I.trunk_state_case(n)
    attn = c['qkv'][:, 128:] if ld == 192 else I.normals(n, n, 64, scale=0.7)
    nets = I.nets(1234)
    with torch.no_grad():
        refs = {dt: dict(pf=I.post_attn(nets[dt].past_encoder, c['g'], attn), k=I.post_attn_rhs(nets[dt].past_encoder, c['g'], attn))
                for dt in ('f64', 'f32')}
    return c, attn, refs


@pytest.mark.parametrize('n', [1, 15, 16, 17, 33])
@pytest.mark.parametrize('ld', [64, 192])
def test_post_attn_and_rhs_vs_float64(n, ld):
    dev, capi = _gpu(), _capi()
    c, attn, refs = _post_case(n, ld)
    W = _packs(dev, 8, 12)['past']
    g = _d(dev, c['g'])
    src = _d(dev, c['qkv']) if ld == 192 else _d(dev, attn)
    ap = src.data_ptr() + (128 * 4 if ld == 192 else 0)
    pf, k = _Buf(dev, n, 128), _Buf(dev, n, 64)
    capi.call('sttode_post_attn', *[W[x] for x in POST_W], g, ap, ld, pf.v, n, I.ODE_TIME, capi.stream_ptr())
    capi.call('sttode_post_attn_rhs', *[W[x] for x in POST_W], g, ap, ld, k.v, n, capi.stream_ptr())
    torch.cuda.synchronize()
    gp, gk = pf.get('post_attn pf'), k.get('post_attn_rhs k')
    _worst(f'post_attn n{n} ld{ld}', _check('pf', gp, refs['f64']['pf'], refs['f32']['pf'], f'post_attn n{n} ld{ld}'))
    _worst(f'post_attn_rhs n{n} ld{ld}', _check('k', gk, refs['f64']['k'], refs['f32']['k'], f'post_attn_rhs n{n} ld{ld}'))
    _biteq(gp[:, :64].contiguous(), _T(c['g']), 'pf[:, :64] = g')
    pf2 = _Buf(dev, n, 128)
    capi.call('sttode_post_attn', *[W[x] for x in POST_W], g, ap, ld, pf2.v, n, I.ODE_TIME, capi.stream_ptr())
    torch.cuda.synchronize()
    _biteq(pf2.get('again'), gp, 'post_attn run twice')


def test_post_attn_rows_of_small_variance_weigh_the_layernorm_epsilon():
    """The state scaled by 0.01 and a zero attention output: the rows that enter LayerNorm 1 then have a variance of 1e-3 .. 3e-3 (the gate
    is tanh(info(b_o)) sigmoid(gate(b_o))), so eps = 1e-5 is about 0.5 % of the variance instead of 1e-5 of it.  An epsilon of 1e-6 moves
    the float64 result by 160 (k) to 250 (pf) times the yardstick's bound here, and by 0.3 of it on the rows of the test above."""
    dev, capi = _gpu(), _capi()
    n = 17
    g, attn = (0.01 * I.trunk_state_case(n)['g']).astype(np.float32), np.zeros((n, 64), np.float32)
    nets = I.nets(1234)
    with torch.no_grad():
        refs = {dt: dict(pf=I.post_attn(nets[dt].past_encoder, g, attn), k=I.post_attn_rhs(nets[dt].past_encoder, g, attn)) for dt in ('f64', 'f32')}
    W = _packs(dev, 8, 12)['past']
    pf, k = _Buf(dev, n, 128), _Buf(dev, n, 64)
    capi.call('sttode_post_attn', *[W[x] for x in POST_W], _d(dev, g), _d(dev, attn), 64, pf.v, n, I.ODE_TIME, capi.stream_ptr())
    capi.call('sttode_post_attn_rhs', *[W[x] for x in POST_W], _d(dev, g), _d(dev, attn), 64, k.v, n, capi.stream_ptr())
    torch.cuda.synchronize()
    _worst('post_attn, small-variance rows', _check('pf', pf.get('pf'), refs['f64']['pf'], refs['f32']['pf'], 'post_attn, small-variance rows'))
    _worst('post_attn_rhs, small-variance rows', _check('k', k.get('k'), refs['f64']['k'], refs['f32']['k'], 'post_attn_rhs, small-variance rows'))


def test_post_attn_refuses_a_bad_leading_dimension():
    dev, capi = _gpu(), _capi()
    c, attn, _ = _post_case(17, 64)
    W = _packs(dev, 8, 12)['past']
    g, a = _d(dev, c['g']), _d(dev, np.zeros((17, 192), np.float32))
    pf, k = _Buf(dev, 17, 128), _Buf(dev, 17, 64)
    for ld in (66, 60):
        _refuses(lambda: capi.call('sttode_post_attn', *[W[x] for x in POST_W], g, a, ld, pf.v, 17, I.ODE_TIME, capi.stream_ptr()), 'ld_attn')
        _refuses(lambda: capi.call('sttode_post_attn_rhs', *[W[x] for x in POST_W], g, a, ld, k.v, 17, capi.stream_ptr()), 'ld_attn')
    torch.cuda.synchronize()
    assert pf.untouched() and k.untouched()


@pytest.mark.parametrize('method', [0, 1, 2])
@pytest.mark.parametrize('steps', [1, 3])
@pytest.mark.parametrize('n', [17, 1])
def test_post_attn_ode_vs_float64(method, steps, n):
    dev, capi = _gpu(), _capi()
    c = I.trunk_state_case(n)
    W = _packs(dev, 8, 12)['past']
    nets = I.nets(1234)
    with torch.no_grad():
        r64, r32 = (I.post_attn_ode(nets[dt].past_encoder, c['g'], method, steps) for dt in ('f64', 'f32'))
    pf = _Buf(dev, n, 128)
    capi.call('sttode_post_attn_ode', *[W[x] for x in POST_W], W['inP'], W['inb'], _d(dev, c['g']), pf.v, n, I.ODE_TIME, method, steps,
              capi.stream_ptr())
    torch.cuda.synchronize()
    got = pf.get('post_attn_ode')
    w = _check('pf', got, r64, r32, f'post_attn_ode method {method} steps {steps}')
    _worst(f'post_attn_ode n{n} method {method} steps {steps}', w)
    _biteq(got[:, :64].contiguous(), _T(c['g']), 'pf[:, :64] = g')
    if (method, steps) == (0, 1):                                   # what sttode_post_attn computes at attention length 1: the same yardstick
        with torch.no_grad():
            p64, p32 = (I.post_attn(nets[dt].past_encoder, c['g'], c['qkv'][:, 128:]) for dt in ('f64', 'f32'))
        _check('pf', got, p64, p32, 'post_attn_ode (Euler, one step) against post_attn at attention length 1')


@pytest.mark.parametrize('n', [1, 3, 4, 5, 1000])
def test_ode_state_to_pf_is_bitwise(n):
    dev, capi = _gpu(), _capi()
    g, y = I.normals(n, n, 64), I.normals(n + 1, n, 64)
    pf = _Buf(dev, n, 128)
    capi.call('sttode_ode_state_to_pf', _d(dev, g), _d(dev, y), pf.v, n, capi.stream_ptr())
    torch.cuda.synchronize()
    _biteq(pf.get('ode_state_to_pf'), torch.cat([_T(g), torch.relu(_T(y))], dim=1), 'pf = cat(g, relu(y))')
    _refuses(lambda: capi.call('sttode_ode_state_to_pf', _d(dev, g), _d(dev, y), pf.v, 0, capi.stream_ptr()), 'bad argument')


# ---------------------------------------------------------------------------------------------------------------------------------------
# decoder: conv + GRU, per-agent pre-activations, the MLP blocks
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('ncols', [1, 15, 16, 17, 50])
@pytest.mark.parametrize('Tp', [1, 5, 8, 10])
def test_gru_cols_vs_float64_both_forms(ncols, Tp, tiles):
    dev, capi = _gpu(), _capi()
    c = I.decoder_case(ncols, 1, Tp, 12)
    TPX = I.tiles_x(Tp)
    nets = I.nets(1234, Tp, 12)
    worst = 0.0
    for blk, key in ((0, 'xpad'), (1, 'dbuf')):                       # block 0 on the track, block 1 on the residual it sees in the chain
        xin = np.ascontiguousarray(c[key][:, :16 * TPX])
        with torch.no_grad():
            r64, r32 = (I.gru_state(nets[dt].decoder.decompose[blk], xin, Tp) for dt in ('f64', 'f32'))
        P = _packs(dev, Tp, 12)['blk%d' % blk]
        got = {}
        for setting in ('latency', 'throughput'):
            tiles(setting)
            _ran('gru_cols:gru', setting, (ncols + 15) // 16)
            st = _Buf(dev, ncols, 96)
            capi.call('sttode_gru_cols', _d(dev, xin), P['convP'], P['convB'], P['wihP'], P['whhP'], P['gbias'], st.v, ncols, Tp, TPX,
                      capi.stream_ptr())
            torch.cuda.synchronize()
            got[setting] = st.get(f'gru_cols block {blk} {setting}')
            worst = max(worst, _check('state', got[setting], r64, r32, f'gru_cols ncols {ncols} Tp {Tp} block {blk} {setting}'))
        _biteq(got['latency'], got['throughput'], 'gru_cols: latency against throughput form')
    _worst(f'gru_cols ncols {ncols} Tp {Tp}', worst)


def test_gru_cols_refusal_writes_nothing():
    dev, capi = _gpu(), _capi()
    P = _packs(dev, 10, 12)['blk0']
    st = _Buf(dev, 5, 96)
    x = _d(dev, np.zeros((5, 32), np.float32))
    for Tp, TPX in ((10, 1), (8, 3), (0, 1)):
        _refuses(lambda: capi.call('sttode_gru_cols', x, P['convP'], P['convB'], P['wihP'], P['whhP'], P['gbias'], st.v, 5, Tp, TPX,
                                   capi.stream_ptr()), 'bad ncols/Tp/TPX')
    torch.cuda.synchronize()
    assert st.untouched()


@pytest.mark.parametrize('n', [1, 16, 17, 64, 65])
def test_agent_preact_vs_float64(n):
    dev, capi = _gpu(), _capi()
    c = I.decoder_case(n, 1, 8, 12)
    nets = I.nets(1234, 8, 12)
    with torch.no_grad():
        r64, r32 = (I.agent_preact(nets[dt].decoder, c['pf'], c['state0']) for dt in ('f64', 'f32'))
    P = _packs(dev, 8, 12)
    b0, b1 = P['blk0'], P['blk1']
    out = {k: _Buf(dev, n, 512) for k in ('A0x', 'A0y', 'A1y')}
    capi.call('sttode_agent_preact', _d(dev, c['pf']), _d(dev, c['state0']), b0['x_WA'], b0['x_b1'], b0['y_WA'], b0['y_b1'], b1['y_WA'],
              b1['y_b1'], out['A0x'].v, out['A0y'].v, out['A1y'].v, n, capi.stream_ptr())
    torch.cuda.synchronize()
    _worst(f'agent_preact n{n}', max(_check(k, out[k].get(k), r64[k], r32[k], f'agent_preact n{n}') for k in out))


# (n, K): ncols = n K = 1, 63 (twice), 64, 65, 140 (twice); K = 7 and 20 put an agent's columns across a 16-column tile and a 64-column group
MLP_NK = [(1, 1), (63, 1), (9, 7), (64, 1), (65, 1), (20, 7), (7, 20)]
MLP_CASES = [(n, K, 8, 12) for n, K in MLP_NK] + [(n, K, Tp, Tf) for Tp, Tf in ((8, 8), (10, 40)) for n, K in ((9, 7), (65, 1), (7, 20))]
_mlid = lambda c: 'n%d-K%d-Tp%d-Tf%d' % c


@functools.lru_cache(maxsize=None)
def _mlp_refs(n, K, Tp, Tf):
    c = I.decoder_case(n, K, Tp, Tf)
    nets = I.nets(1234, Tp, Tf)
    out = {}
    with torch.no_grad():
        for dt in ('f64', 'f32'):
            dec = nets[dt].decoder
            o = I.mlp_block0(dec, c['A0x'], c['A0y'], c['z'], c['xpad'], K, Tp, Tf)
            o['pred'] = I.mlp_block1(dec, c['A1y'], c['z'], c['state1'], c['ybuf'], c['cur'], c['orig'], K, Tf)
            o['xh1'] = I.mlp_cols(dec.decompose[1].decoder_x, c['A1y'], c['z'], c['state1'], K, I.tiles_x(Tp))
            out[dt] = o
    return c, out


@pytest.mark.parametrize('c', MLP_CASES, ids=_mlid)
def test_mlp_blocks_vs_float64_both_forms(c, tiles):
    dev, capi = _gpu(), _capi()
    n, K, Tp, Tf = c
    case, refs = _mlp_refs(*c)
    m, TPX, NOY = n * K, I.tiles_x(Tp), I.tiles_y(Tf)
    P = _packs(dev, Tp, Tf)
    b0, b1 = P['blk0'], P['blk1']
    D = {k: _d(dev, case[k]) for k in ('A0x', 'A0y', 'A1y', 'z', 'state1', 'ybuf', 'cur', 'orig')}
    xpad = _d(dev, case['xpad'][:, :16 * TPX])
    got, worst = {}, {}
    for setting in ('latency', 'throughput'):
        tiles(setting)
        _ran('mlp_block0:mlp', setting, (m + 15) // 16)
        _ran('mlp_block1:mlp', setting, (m + 15) // 16)
        dbuf, ybuf, pred = _Buf(dev, m, 16 * TPX), _Buf(dev, m, 16 * NOY), _Buf(dev, m, 2 * Tf)
        capi.call('sttode_mlp_block0', D['A0x'], D['A0y'], b0['stream'], b0['n_chunks'], D['z'], xpad, dbuf.v, ybuf.v, m, K, TPX, NOY,
                  capi.stream_ptr())
        capi.call('sttode_mlp_block1', D['A1y'], b1['stream'], b1['n_chunks'], D['z'], D['state1'], D['ybuf'], D['cur'], D['orig'], pred.v, m, K,
                  Tf, NOY, capi.stream_ptr())
        torch.cuda.synchronize()
        got[setting] = dict(dbuf=dbuf.get('dbuf'), ybuf=ybuf.get('ybuf'), pred=pred.get('pred'))
        for k in got[setting]:
            worst[k + ' ' + setting] = _check(k, got[setting][k], refs['f64'][k], refs['f32'][k], f'mlp_block {_mlid(c)} {setting}')
    for k in ('dbuf', 'ybuf', 'pred'):
        _biteq(got['latency'][k], got['throughput'][k], f'{k}: latency against throughput form')
    # the generic MLP (one form): block 1's decoder_x on [z | state1], block 1's pf table standing in for its per-agent part
    xh = _Buf(dev, m, 16 * TPX)
    capi.call('sttode_mlp_cols', D['A1y'], b1['x_stream'], b1['x_n_chunks'], D['z'], D['state1'], xh.v, m, K, TPX, capi.stream_ptr())
    torch.cuda.synchronize()
    RAN[('mlp_cols', 'throughput')] += 1
    worst['mlp_cols'] = _check('xh1', xh.get('mlp_cols'), refs['f64']['xh1'], refs['f32']['xh1'], f'mlp_cols {_mlid(c)}')
    k = max(worst, key=worst.get)
    _worst(f'mlp_block0 / mlp_block1 / mlp_cols {_mlid(c)} (at {k})', worst[k])


def test_mlp_chunk_count_refusals_write_nothing():
    dev, capi = _gpu(), _capi()
    case, _ = _mlp_refs(9, 7, 8, 12)
    P = _packs(dev, 8, 12)
    b0, b1 = P['blk0'], P['blk1']
    D = {k: _d(dev, case[k]) for k in ('A0x', 'A0y', 'A1y', 'z', 'state1', 'ybuf', 'cur', 'orig')}
    xpad = _d(dev, case['xpad'][:, :16])
    outs = [_Buf(dev, 63, 16), _Buf(dev, 63, 32), _Buf(dev, 63, 24), _Buf(dev, 63, 16)]
    _refuses(lambda: capi.call('sttode_mlp_block0', D['A0x'], D['A0y'], b0['stream'], b0['n_chunks'] - 1, D['z'], xpad, outs[0].v, outs[1].v,
                               63, 7, 1, 2, capi.stream_ptr()), 'weight stream must hold')
    _refuses(lambda: capi.call('sttode_mlp_block0', D['A0x'], D['A0y'], b0['stream'], b0['n_chunks'], D['z'], xpad, outs[0].v, outs[1].v,
                               63, 7, 1, 3, capi.stream_ptr()), 'weight stream must hold')
    _refuses(lambda: capi.call('sttode_mlp_block1', D['A1y'], b1['stream'], b1['n_chunks'] + 1, D['z'], D['state1'], D['ybuf'], D['cur'],
                               D['orig'], outs[2].v, 63, 7, 12, 2, capi.stream_ptr()), 'weight stream must hold')
    _refuses(lambda: capi.call('sttode_mlp_block1', D['A1y'], b1['stream'], 33, D['z'], D['state1'], D['ybuf'], D['cur'], D['orig'], outs[2].v,
                               63, 7, 12, 1, capi.stream_ptr()), 'bad ncols/K/Tf/NOY')
    _refuses(lambda: capi.call('sttode_mlp_cols', D['A1y'], b1['x_stream'], b1['x_n_chunks'] + 1, D['z'], D['state1'], outs[3].v, 63, 7, 1,
                               capi.stream_ptr()), 'chunk count')
    torch.cuda.synchronize()
    assert all(o.untouched() for o in outs)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the fused per-trajectory chain
# ---------------------------------------------------------------------------------------------------------------------------------------
# ncols = n K = 1, 31, 32, 33, 127, 128, 129, 260 (32-column waves, 128-trajectory groups); K = 7 / 20 put an agent across a wave and a
# group; (Tp, Tf) -> NY 1 / 2 / 3; ldx 16 / 32; wgs_per_cu 1 / 2
CHAIN_CASES = [(1, 1, 8, 12, 16, 2), (31, 1, 8, 12, 32, 1), (32, 1, 5, 10, 16, 2), (33, 1, 8, 12, 16, 1), (127, 1, 1, 12, 16, 2),
               (128, 1, 8, 20, 32, 2), (129, 1, 10, 40, 32, 1), (13, 20, 8, 12, 16, 2), (19, 7, 8, 12, 16, 1), (5, 7, 5, 10, 32, 2),
               (13, 20, 10, 40, 32, 2), (13, 20, 8, 20, 16, 1), (7, 20, 1, 12, 32, 1)]
_chid = lambda c: 'n%d-K%d-Tp%d-Tf%d-ldx%d-wgs%d' % c


@functools.lru_cache(maxsize=None)
def _chain_refs(n, K, Tp, Tf):
    c = I.decoder_case(n, K, Tp, Tf)
    nets = I.nets(1234, Tp, Tf)
    with torch.no_grad():
        return c, {dt: I.traj_chain(nets[dt].decoder, c['A0x'], c['A0y'], c['A1y'], c['z'], c['xpad'], c['cur'], c['orig'], K, Tp, Tf)['pred']
                   for dt in ('f64', 'f32')}


def _chain_run(dev, case, ldx, wgs, prog_len=None, pred=None):
    capi = _capi()
    n, K, Tp, Tf = case['n'], case['K'], case['Tp'], case['Tf']
    C = _packs(dev, Tp, Tf)['chain']
    pred = _Buf(dev, n * K, 2 * Tf) if pred is None else pred
    counter = torch.zeros(1, dtype=torch.int32, device=dev)
    D = {k: _d(dev, case[k]) for k in ('A0x', 'A0y', 'A1y', 'z', 'cur', 'orig')}
    capi.call('sttode_traj_chain', D['A0x'], D['A0y'], D['A1y'], C['pool'], C['prog'], C['prog_len'] if prog_len is None else prog_len,
              C['consts'], D['z'], _d(dev, case['xpad'][:, :16] if ldx == 16 else case['xpad']), ldx, D['cur'], D['orig'], pred.v, counter,
              n * K, K, Tp, Tf, wgs, capi.stream_ptr())
    torch.cuda.synchronize()
    return pred


@pytest.mark.parametrize('c', CHAIN_CASES, ids=_chid)
def test_traj_chain_vs_float64(c):
    dev = _gpu()
    n, K, Tp, Tf, ldx, wgs = c
    case, refs = _chain_refs(n, K, Tp, Tf)
    got = _chain_run(dev, case, ldx, wgs).get('traj_chain pred')
    _worst(f'traj_chain {_chid(c)}', _chain_close(got, refs['f64'], refs['f32'], 'traj_chain ' + _chid(c)))
    _biteq(_chain_run(dev, case, ldx, wgs).get('again'), got, 'traj_chain run twice')
    if 2 * Tp <= 16:                                               # the other row stride of xpad and the other residency: the same bits
        _biteq(_chain_run(dev, case, 48 - ldx, 3 - wgs).get('other ldx'), got, 'traj_chain: ldx 16 against 32, wgs_per_cu 1 against 2')


def test_traj_chain_refusals_write_nothing():
    dev = _gpu()
    case, _ = _chain_refs(5, 7, 8, 12)
    pred = _Buf(dev, 35, 24)
    C = _packs(dev, 8, 12)['chain']
    _refuses(lambda: _chain_run(dev, case, 16, 2, prog_len=C['prog_len'] - 1, pred=pred), 'chunk program length')
    _refuses(lambda: _chain_run(dev, case, 24, 2, pred=pred), 'ldx must be 16 or 32')
    _refuses(lambda: _chain_run(dev, case, 16, 3, pred=pred), 'wgs_per_cu')
    case10, _ = _chain_refs(129, 1, 10, 40)
    pred10 = _Buf(dev, 129, 80)
    _refuses(lambda: _chain_run(dev, case10, 16, 2, pred=pred10), 'xpad rows shorter')
    torch.cuda.synchronize()
    assert pred.untouched() and pred10.untouched()


# ---------------------------------------------------------------------------------------------------------------------------------------
# the forms without an entry point of their own, through STTODENet
# ---------------------------------------------------------------------------------------------------------------------------------------
_MODELS = {}


def _model(dataset, Tp, Tf):
    from helpers import make_args
    from sttode_amd import STTODENet
    from sttode_amd.weights import to_torch_state_dict
    key = (dataset, Tp, Tf)
    if key not in _MODELS:
        m = STTODENet(make_args(dataset, Tp, Tf), _gpu()).eval()
        m.load_state_dict(to_torch_state_dict(I.nets(1234, Tp, Tf)['sd']), strict=True)
        _MODELS[key] = m
    return _MODELS[key]


@functools.lru_cache(maxsize=None)
def _batch(kind):
    """The smallest ragged batches: scenes of 1, 15, 16, 17 and 33 agents in one call; one NBA call B = 3, N = 11; the long horizon, B = 2."""
    from sttode_amd import scenes
    if kind == 'scenes':
        Tp, Tf = 8, 12
        past, fut, ptr = I.scene_case([1, 15, 16, 17, 33], Tp, Tf, seed=9)
        B = N = 0
    else:
        Tp, Tf, B, N = (5, 10, 3, 11) if kind == 'nba' else (10, 40, 2, 10)
        past, fut = I.nba_case(B, N, Tp, Tf, seed=2)
        ptr = None
    n = past.shape[0]
    z = scenes.latents(77, n)
    nets = I.nets(1234, Tp, Tf, 'eth' if kind == 'scenes' else 'nba')
    refs = {}
    with torch.no_grad():
        for dt in ('f64', 'f32'):
            refs[dt] = I.inference_scenes(nets[dt], past, ptr, z) if kind == 'scenes' else I.inference_nba(nets[dt], past, B, N, z)
    return dict(kind=kind, Tp=Tp, Tf=Tf, B=B, N=N, n=n, past=past, fut=fut, ptr=ptr, z=z, refs=refs)


def _feed(m, b):
    dev = m.device
    if b['kind'] == 'scenes':
        m.set_scene_batch(_d(dev, b['past']), _d(dev, b['fut']), _d(dev, b['ptr']))
    else:
        m.set_data_nba({'past_traj': _d(dev, b['past']).reshape(b['B'], b['N'], b['Tp'], 2),
                        'future_traj': _d(dev, b['fut']).reshape(b['B'], b['N'], b['Tf'], 2)})


def _model_check(b, name, got, what, refs=None):
    refs = b['refs'] if refs is None else refs
    r64, r32 = refs['f64'][name], refs['f32'][name]
    r64, r32 = (torch.as_tensor(v) for v in (r64, r32))
    return _chain_close(got.detach().cpu().reshape(r64.shape), r64, r32, what)


@pytest.mark.parametrize('kind', ['scenes', 'nba', 'nba_long'])
def test_model_forms_vs_float64_oracle(kind, tiles):
    """inference() in the three-kernel form, the fused chain launch and (scene batches) the one-launch scene form, each with the latency
    tiles forced both ways; inference_async() with the lagged form off, on 2 and on 3 streams.  past_feature and the predictions of every
    form, and state0 / dbuf / ybuf where the form leaves them in the workspace (the three-kernel form), against the float64 stages."""
    b = _batch(kind)
    m = _model('eth' if kind == 'scenes' else 'nba', b['Tp'], b['Tf'])
    dev, n, K, Tf = m.device, b['n'], 20, b['Tf']
    z = _d(dev, b['z'])
    nat = m.native()
    worst, ran = {}, []
    try:
        sync_forms = [('three-kernel', 0, 0), ('fused chain', 1, 0)] + ([('one-launch scene', 0, -1)] if kind == 'scenes' else [])
        first = {}
        for form, chain, scene_launch in sync_forms:
            for setting in ('latency', 'throughput'):
                tiles(setting)
                nat.set_chain(chain)
                nat.set_scene_launch(scene_launch)
                _feed(m, b)
                out = m.inference(None, z=z)
                torch.cuda.synchronize()
                tag = f'{form}, {setting} tiles'
                ran.append(tag)
                pred = out.permute(1, 0, 2, 3).contiguous()
                assert torch.isfinite(pred).all(), tag
                worst['pred ' + tag] = _model_check(b, 'pred', pred, f'{kind} {tag}: predictions')
                worst['pf ' + tag] = _model_check(b, 'pf', m.past_feature, f'{kind} {tag}: past_feature')
                if kind == 'scenes':
                    so = m.scene_orig
                    worst['scene_orig ' + tag] = _model_check(b, 'scene_orig', so, f'{kind} {tag}: scene_orig')
                if form == 'three-kernel':
                    for k in ('state0', 'dbuf', 'ybuf'):
                        worst[f'{k} {tag}'] = _model_check(b, k, m._dbg[k], f'{kind} {tag}: {k}')
                first.setdefault(form, pred.clone())
                _biteq(pred.cpu(), first[form].cpu(), f'{kind} {form}: latency against throughput tiles')
        tiles('latency')
        nat.set_chain(1)
        nat.set_scene_launch(-1)
        for streams in (0, 2, 3):
            nat.set_lagged(streams)
            m.reset_async()
            _feed(m, b)
            lagged = bool(_capi().lib().sttode_async_is_lagged(nat.h, n))
            assert lagged == (streams > 0)
            hs = [m.inference_async(z=z) for _ in range(2)] + [m.inference_async(z=None)]
            outs = [m.wait(h).permute(1, 0, 2, 3).contiguous().clone() for h in hs]
            torch.cuda.synchronize()
            tag = f'lagged {streams}'
            ran.append(tag)
            worst['pred ' + tag] = _model_check(b, 'pred', outs[0], f'{kind} {tag}: predictions')
            _biteq(outs[1].cpu(), outs[0].cpu(), f'{kind} {tag}: the same call twice')
            if streams == 0:
                _biteq(outs[0].cpu(), first['fused chain'].cpu(), f'{kind}: asynchronous call with the lagged form off against inference()')
            # the call that drew its own latents: the float64 stages on the latents it reports
            zown = hs[2]['z'].cpu().numpy()
            nets = I.nets(1234, b['Tp'], b['Tf'], 'eth' if kind == 'scenes' else 'nba')
            with torch.no_grad():
                own = {dt: dict(pred=(I.inference_scenes(nets[dt], b['past'], b['ptr'], zown) if kind == 'scenes' else
                                      I.inference_nba(nets[dt], b['past'], b['B'], b['N'], zown))['pred']) for dt in ('f64', 'f32')}
            worst['pred own latents ' + tag] = _model_check(b, 'pred', outs[2], f'{kind} {tag}: own latents', own)
    finally:
        nat.set_chain(-1)
        nat.set_scene_launch(-1)
        m.reset_async()
        nat.set_lagged(3)
    for k in sorted(worst):
        _worst(f'model {kind} {k}', worst[k])
    print(f'[forms] model {kind}: ' + '; '.join(ran))
    assert len(ran) == 2 * len(sync_forms) + 3


def test_zz_both_forms_of_every_stage_ran():
    """The counters of the tests above: every stage with a latency and a throughput kernel ran in both (the stages this session ran)."""
    stages = sorted({s for s, _ in RAN})
    for s in stages:
        print(f'[forms] {s}: latency {RAN[(s, "latency")]}, throughput {RAN[(s, "throughput")]}')
        if s != 'mlp_cols':
            assert RAN[(s, 'latency')] > 0 and RAN[(s, 'throughput')] > 0, s
