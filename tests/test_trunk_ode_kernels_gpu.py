"""Direct float64 tests of the fused trunk and ODE-stage training kernels (csrc/train_trunk.hip, train_ode.hip, ode_body.hpp): the entry
points sttode_ttrunk_fwd, sttode_ttrunk_ode_fwd, sttode_ode_stage_bwd and sttode_ode_combine through capi.call, at the sizes their code
branches on (one agent, tiles with dead lanes, exactly 16 agents, T = 1 and the LDS maximum T = 12, ld_feat > 128, null DROP / LAST, two
trunks of different n and T in one launch, the phase split, programs of several steps, two stage-backward jobs of different tile counts,
strided terms, the grid-stride second trip of the combination kernel).

References: tests/trunk_ode_ref.py (pinned on the CPU by tests/test_trunk_ode_ref.py) in float64 and in torch fp32 on the very fp32
inputs the kernel received; yardstick of tests/train_ref.py: |hip - f64| <= max(4 |torch_fp32 - f64|, 1e-6 max|f64| + 1e-5 |f64|) per
element.  Relations that hold exactly (copies, the phase split, grouped against single launches) are bitwise.  Every output is a slice
of a larger buffer with guard rows of sentinels around a payload that starts as NaN: a guard that changes, or an element left NaN, fails.

The stage-backward inputs come from trunk_ode_ref.stage_inputs: every hidden unit's float64 pre-activation lies at least 16 x torch's
own fp32 error away from 0, so no correct fp32 kernel flips a relu mask against float64; nothing is excluded on the GPU side."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import train_ref as R
import trunk_ode_ref as T

from test_train_kernels_gpu import SENT, _capi, _close, _gpu, _worst

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
GUARD = 3                                # guard rows on each side of a payload
TAPE = dict(posin=128, tp=64, h3in=68, feat=128, xc=64, qkv=192, ao=64, tt=64, ss=64, h=64, xh1=64, rs1=1, f1=1024, xh2=64, rs2=1, ode=64)
PHASE1 = ('posin', 'tp', 'h3in', 'xc', 'qkv')           # written up to the in-projection (and feat[:, :64])
LATER = ('ao', 'tt', 'ss', 'h', 'xh1', 'rs1', 'f1', 'xh2', 'rs2', 'ode')


def _records():
    from sttode_amd import training
    return training._OdeCombine, training._OdeProgram, training._OdeStageBwd


class _Buf:
    """A [rows, width] payload (NaN) at row stride ``ld`` inside a buffer with GUARD rows of sentinels before and after; the columns
    width .. ld - 1 of the payload rows hold sentinels too."""

    def __init__(self, dev, rows, width, ld=None):
        self.rows, self.width, self.ld = rows, width, ld or width
        self.buf = torch.full(((rows + 2 * GUARD), self.ld), SENT, dtype=F32, device=dev)
        self.v = self.buf[GUARD:GUARD + rows]
        self.v[:, :width] = float('nan')

    def ptr(self):
        return self.v.data_ptr()

    def sentinels_ok(self):
        b = self.buf.cpu()
        return bool((b[:GUARD] == SENT).all() and (b[GUARD + self.rows:] == SENT).all() and (b[GUARD:GUARD + self.rows, self.width:] == SENT).all())

    def untouched(self):
        return self.sentinels_ok() and bool(torch.isnan(self.v[:, :self.width]).all())

    def get(self, what=''):
        """The payload on the host; every guard intact and no element left NaN."""
        assert self.sentinels_ok(), f'{what}: a sentinel around the output changed'
        p = self.v[:, :self.width].cpu().clone()
        assert not torch.isnan(p).any(), f'{what}: {int(torch.isnan(p).sum())} elements were not written'
        return p


def _check(name, got, r64, r32, what):
    """The plain yardstick on one tensor (no tensor of these kernels needs a wider atol: the fused chains stay below 0.7 of the bound,
    profiles/trunk_ode_tests/gputests.txt) -> worst error in units of the bound."""
    return _close(got, r64.reshape(got.shape), r32.reshape(got.shape), f'{what} {name}')


def _biteq(a, b, what):
    assert a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32)), f'{what}: not bitwise equal'


# ---------------------------------------------------------------------------------------------------------------------------------------
# fused trunk forward
# ---------------------------------------------------------------------------------------------------------------------------------------
# (n, T, ld_feat, drop, last)
TRUNK_CASES = [(1, 1, 128, False, False), (15, 8, 128, True, True), (16, 12, 132, True, True), (17, 12, 256, False, True),
               (33, 8, 128, True, False)]
_tid = lambda c: 'n%d-T%d-ld%d-%s-%s' % (c[0], c[1], c[2], 'drop' if c[3] else 'nodrop', 'last' if c[4] else 'nolast')


@functools.lru_cache(maxsize=None)
def _trunk_refs(n, T_, drop, last):
    case = T.trunk_case(n, T_, drop, last)
    with torch.no_grad():
        return case, T.trunk_refs(case, F64), T.trunk_refs(case, F32)


class _Trunk:
    """Device copies of one case's inputs, fresh output buffers, and the pointer table of sttode_ttrunk_fwd."""

    def __init__(self, dev, case, ld_feat=128, attn=None, null=()):
        n, T_ = case['n'], case['T']
        self.n, self.T, self.ld_feat, self.case = n, T_, ld_feat, case
        self.inp = {k: v.to(dev) for k, v in case['W'].items()}
        self.inp.update(enc_in=case['enc_in'].to(dev), pe=case['pe'].to(dev),
                        drop=None if case['drop'] is None else case['drop'].to(dev), last=None if case['last'] is None else case['last'].to(dev))
        self.out = {k: _Buf(dev, n * T_ if k in ('posin', 'tp') else n, w, ld_feat if k == 'feat' else None) for k, w in TAPE.items()}
        self.attn = attn
        self.null = null

    def ptrs(self):
        capi = _capi()
        src = dict(self.inp, attn=self.attn, **{k: b.v for k, b in self.out.items()})
        return [None if (k in self.null or src[k] is None) else src[k].data_ptr() for k in capi.TRUNK_PTRS]

    def launch(self, phase=0, count=None, T_=None, ld_feat=None):
        capi = _capi()
        p = self.ptrs()
        self.tbl = (ctypes.c_void_p * len(p))(*p)                   # (kept until after the synchronisation)
        capi.call('sttode_ttrunk_fwd', self.tbl, len(p) if count is None else count, self.n, self.T if T_ is None else T_,
                  self.ld_feat if ld_feat is None else ld_feat, float(self.case['ode_time']), phase, capi.stream_ptr())

    def get(self, names=tuple(TAPE), what=''):
        torch.cuda.synchronize()
        return {k: self.out[k].get(f'{what} {k}') for k in names}

    def untouched(self, names=tuple(TAPE)):
        torch.cuda.synchronize()
        return all(self.out[k].untouched() for k in names)


def _phase0(dev, c):
    n, T_, ld, drop, last = c
    case, r64, r32 = _trunk_refs(n, T_, drop, last)
    t = _Trunk(dev, case, ld)
    t.launch(0)
    return t, t.get(what=_tid(c)), r64, r32


@pytest.mark.parametrize('c', TRUNK_CASES, ids=_tid)
def test_ttrunk_fwd_phase0_vs_float64(c):
    dev = _gpu()
    n, T_, ld, drop, last = c
    t, got, r64, r32 = _phase0(dev, c)
    worst = {}
    for k in TAPE:
        worst[k] = _check(k, got[k], r64[k], r32[k], 'ttrunk_fwd ' + _tid(c))
    k = max(worst, key=worst.get)
    _worst(f'ttrunk_fwd {_tid(c)} (at {k})', worst[k])
    # pure copies
    case = t.case
    _biteq(got['posin'][:, 64:], case['pe'][:T_].repeat(n, 1), 'posin[:, 64:] = pe[t]')
    _biteq(got['feat'][:, :64], got['xc'], 'feat[:, :64] = xc')
    _biteq(got['feat'][:, 64:], got['ode'], 'feat[:, 64:128] = ode')
    cat = torch.zeros(n, 4)
    if last:
        cat[:, 2] = (case['last'] != 0).float()
    _biteq(got['h3in'][:, 64:], cat, 'h3in[:, 64:68] = [0, 0, last, 0]')
    assert (got['f1'] >= 0).all()


@pytest.mark.parametrize('c', TRUNK_CASES, ids=_tid)
def test_ttrunk_fwd_phase_split_is_bitwise_phase0(c):
    dev = _gpu()
    n, T_, ld, drop, last = c
    _, whole, _, _ = _phase0(dev, c)
    t = _Trunk(dev, _trunk_refs(n, T_, drop, last)[0], ld)
    t.launch(1)
    first = t.get(PHASE1, what='phase 1')
    assert t.untouched(LATER), 'phase 1 wrote a tensor behind the in-projection'
    feat = t.out['feat']
    assert feat.sentinels_ok() and bool(torch.isnan(feat.v[:, 64:128]).all()) and not bool(torch.isnan(feat.v[:, :64]).any())
    for k in PHASE1:
        _biteq(first[k], whole[k], f'phase 1 {k}')
    t.attn = torch.empty(n, 64, dtype=F32, device=dev)
    t.attn.copy_(t.out['qkv'].v[:, 128:192])
    t.launch(2)
    both = t.get(what='phase 1 + 2')
    for k in TAPE:
        _biteq(both[k], whole[k], f'phase 1 + 2 {k}')


def _group(on):
    _capi().call('sttode_tgemm_group', on)


def test_ttrunk_fwd_group_of_two_is_bitwise_the_single_launches():
    dev = _gpu()
    cases = [(17, 8, 128, True, True), (5, 12, 132, True, True)]
    single = [_phase0(dev, c)[1] for c in cases]
    ts = [_Trunk(dev, _trunk_refs(c[0], c[1], c[3], c[4])[0], c[2]) for c in cases]
    _group(1)
    try:
        for t in ts:
            t.launch(0)
    except BaseException:
        _group(-1)
        raise
    _group(0)
    for c, t, ref in zip(cases, ts, single):
        got = t.get(what='group ' + _tid(c))
        for k in TAPE:
            _biteq(got[k], ref[k], f'group {_tid(c)} {k}')


def test_ttrunk_fwd_group_of_one_runs_when_the_group_closes():
    dev = _gpu()
    c = (17, 8, 128, True, True)
    ref = _phase0(dev, c)[1]
    t = _Trunk(dev, _trunk_refs(c[0], c[1], c[3], c[4])[0], c[2])
    _group(1)
    try:
        t.launch(0)
    except BaseException:
        _group(-1)
        raise
    _group(0)
    got = t.get(what='group of one')
    for k in TAPE:
        _biteq(got[k], ref[k], f'group of one {k}')


def test_ttrunk_fwd_group_does_not_pair_trunks_of_different_streams():
    """The second call of a group arrives on another stream: the queued trunk leaves alone on its own stream, the second one when the
    group closes."""
    dev = _gpu()
    cases = [(17, 8, 128, True, True), (5, 12, 132, True, True)]
    single = [_phase0(dev, c)[1] for c in cases]
    ts = [_Trunk(dev, _trunk_refs(c[0], c[1], c[3], c[4])[0], c[2]) for c in cases]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()                                         # (the buffers were filled on the default stream)
    _group(1)
    try:
        for t, s in zip(ts, streams):
            with torch.cuda.stream(s):
                t.launch(0)
    except BaseException:
        _group(-1)
        raise
    _group(0)
    for c, t, ref in zip(cases, ts, single):
        got = t.get(what='two streams ' + _tid(c))
        for k in TAPE:
            _biteq(got[k], ref[k], f'two streams {_tid(c)} {k}')


# ---------------------------------------------------------------------------------------------------------------------------------------
# sttode_ttrunk_ode_fwd
# ---------------------------------------------------------------------------------------------------------------------------------------
PROGRAMS = [('euler', 1), ('euler', 3), ('rk4', 1), ('rk4', 2), ('rk4_classic', 2)]
ODE_TRUNKS = [((1, 1),), ((17, 8),), ((17, 8), (5, 12)), ((5, 12), (33, 8))]          # (n, T) per trunk; drop and last given


def _program(method, steps, ode_time):
    from sttode_amd import odestages
    _, _OdeProgram, _ = _records()
    A, B = odestages.TABLEAU[method]
    prog = _OdeProgram(stages=len(B), steps=steps, h=float(ode_time) / steps)
    for i, row in enumerate(A):
        for j, c in enumerate(row):
            prog.a[4 * i + j] = c
    for i, c in enumerate(B):
        prog.b[i] = c
    return prog


def _ode_bufs(dev, trunks, prog):
    nst = max(prog.steps, 1) * prog.stages
    return [_Buf(dev, nst * t.n, 64) for t in trunks], [_Buf(dev, t.n, 64) for t in trunks]


def _ode_launch(trunks, prog, ys, yT, count=None, ntrunks=None, T_=None, ld_feat=None, null_ys=False):
    """One sttode_ttrunk_ode_fwd launch over ``trunks`` [_Trunk] into the buffers ``ys`` / ``yT`` -> everything that must outlive the
    launch (host memory: the pointer table, n, T, ld_feat, the tape pointers, the program)."""
    capi = _capi()
    m = len(trunks)
    p = [x for t in trunks for x in t.ptrs()]
    keep = [(ctypes.c_void_p * len(p))(*p), (ctypes.c_int * m)(*[t.n for t in trunks]), (ctypes.c_int * m)(*(T_ or [t.T for t in trunks])),
            (ctypes.c_long * m)(*(ld_feat or [t.ld_feat for t in trunks])), (ctypes.c_void_p * m)(*[None if null_ys else b.ptr() for b in ys]),
            (ctypes.c_void_p * m)(*[b.ptr() for b in yT]), prog]
    capi.call('sttode_ttrunk_ode_fwd', keep[0], len(p) if count is None else count, m if ntrunks is None else ntrunks, keep[1], keep[2], keep[3],
              keep[4], keep[5], ctypes.byref(prog), capi.stream_ptr())
    return keep


@functools.lru_cache(maxsize=None)
def _ode_refs(n, T_, method, steps):
    from sttode_amd import odestages
    case, r64, r32 = _trunk_refs(n, T_, True, True)
    prog = T.program(method, steps, case['ode_time'], odestages.TABLEAU, f32=True)
    with torch.no_grad():
        return (T.ode_program(T.as_dtype(case['W'], F64), r64['xc'], prog), T.ode_program(case['W'], r32['xc'], prog))


def _ode_run(dev, cfg, method, steps):
    trunks = [_Trunk(dev, _trunk_refs(n, T_, True, True)[0], 128 + 4 * i) for i, (n, T_) in enumerate(cfg)]
    prog = _program(method, steps, trunks[0].case['ode_time'])
    ys, yT = _ode_bufs(dev, trunks, prog)
    keep = _ode_launch(trunks, prog, ys, yT)
    torch.cuda.synchronize()
    del keep
    res = []
    for t, a, b in zip(trunks, ys, yT):
        assert t.untouched(LATER), 'the integration launch wrote a tape tensor behind the in-projection'
        d = t.get(PHASE1, what='ode_fwd')
        d.update(ys=a.get('ys'), yT=b.get('yT'), feat=t.out['feat'].get('feat'))
        res.append(d)
    return res


@pytest.mark.parametrize('cfg', ODE_TRUNKS, ids=lambda cfg: '+'.join('n%d-T%d' % c for c in cfg))
@pytest.mark.parametrize('method,steps', PROGRAMS)
def test_ttrunk_ode_fwd_vs_float64(cfg, method, steps):
    dev = _gpu()
    got = _ode_run(dev, cfg, method, steps)
    what = f'ttrunk_ode_fwd {method} x{steps} ' + '+'.join('n%d-T%d' % c for c in cfg)
    worst = {}
    for (n, T_), g in zip(cfg, got):
        r64, r32 = _ode_refs(n, T_, method, steps)
        for k in ('ys', 'yT'):
            worst[f'{k} n{n}'] = _check(k, g[k], r64[k], r32[k], what)
        worst[f'relu n{n}'] = _check('relu', g['feat'][:, 64:], r64['relu'], r32['relu'], what)
        _biteq(g['feat'][:, 64:], torch.relu(g['yT']), 'feat[:, 64:128] = relu(yT)')
        _biteq(g['ys'][:n], g['xc'], 'ys rows [0, n) = xc')
        _biteq(g['feat'][:, :64], g['xc'], 'feat[:, :64] = xc')
        # the layers in front are sttode_ttrunk_fwd phase 1 on the same inputs
        t = _Trunk(dev, _trunk_refs(n, T_, True, True)[0])
        t.launch(1)
        first = t.get(PHASE1, what='phase 1')
        for k in PHASE1:
            _biteq(g[k], first[k], f'ode_fwd {k} vs phase 1')
        if (method, steps) == ('euler', 1):                         # one Euler step of size ode_time: phase 0's encoder output
            _, t64, t32 = _trunk_refs(n, T_, True, True)
            worst[f'euler1 vs ode n{n}'] = _check('ode', g['feat'][:, 64:], t64['ode'], t32['ode'], what)
    if len(cfg) == 2:                                                # two trunks in one launch = the two one-trunk launches
        for c, g in zip(cfg, got):
            one = _ode_run(dev, (c,), method, steps)[0]
            for k in g:
                _biteq(g[k], one[k], f'two trunks vs one, {k}')
    k = max(worst, key=worst.get)
    _worst(f'{what} (at {k})', worst[k])


# ---------------------------------------------------------------------------------------------------------------------------------------
# sttode_ode_stage_bwd
# ---------------------------------------------------------------------------------------------------------------------------------------
STAGE_JOBS = [(n,) for n in T.STAGE_NS] + list(T.STAGE_PAIRS)
STAGE_OUT = dict(dy=64, attn=64, ao=64, h=64, f1=1024, dsum2=64, df1=1024, du=64, dv=64, dao=64, dattn=64, ln=256)


@functools.lru_cache(maxsize=None)
def _stage_refs(n, kb_form, next_form):
    inp = T.stage_inputs(n, T.STAGE_BASE[n])
    assert inp is not None
    return inp, T.stage_refs(inp, kb_form, next_form, F64), T.stage_refs(inp, kb_form, next_form, F32)


class _StageJob:
    """Device inputs, fresh outputs and the record fields of one sttode_ode_stage_bwd job."""

    def __init__(self, dev, inp, kb_form, next_form):
        n = inp['n']
        self.n = n
        self.W = [inp['W'][k].to(dev) for k in T.ODE_W]
        self.Y = inp['Y'].to(dev)
        self.dinp = dict(vals=[v.to(dev) for v in inp['vals']], wide=inp['wide'].to(dev), coef=inp['coef'])
        self.kb, self.nx = T.stage_terms(self.dinp, kb_form, next_form)
        self.out = {k: _Buf(dev, n, w) for k, w in STAGE_OUT.items()}
        self.next = None if self.nx is None else _Buf(dev, n, 64, 192 if next_form == 'next5ld192' else 64)

    def fill(self, J):
        for i, w in enumerate(self.W):
            J.w[i] = w.data_ptr()
        J.y, J.n = self.Y.data_ptr(), self.n
        for i, (c, v) in enumerate(self.kb):
            assert v.stride(1) == 1
            J.kb.v[i], J.kb.ld[i], J.kb.c[i] = v.data_ptr(), v.stride(0), c
        J.kb.nterms, J.kb.rows = len(self.kb), self.n
        if self.nx is not None:
            for i, (c, v) in enumerate(self.nx):
                J.next.v[i], J.next.ld[i], J.next.c[i] = v.data_ptr(), v.stride(0), c
            J.next.nterms, J.next.rows, J.next.out, J.next.ld_out = len(self.nx), self.n, self.next.ptr(), self.next.ld
        for k, b in self.out.items():
            setattr(J, k, b.ptr())

    def bufs(self):
        return list(self.out.values()) + ([self.next] if self.next is not None else [])


def _stage_launch(jobs, count=None, edit=None):
    capi = _capi()
    _, _, _OdeStageBwd = _records()
    tab = (_OdeStageBwd * max(len(jobs), 1))()
    for J, job in zip(tab, jobs):
        job.fill(J)
    if edit:
        edit(tab)
    try:
        capi.call('sttode_ode_stage_bwd', tab, len(jobs) if count is None else count, capi.stream_ptr())
    finally:
        torch.cuda.synchronize()                                     # (the table and the jobs' tensors are alive until here)
    return tab


@pytest.mark.parametrize('next_form', T.NEXT_FORMS)
@pytest.mark.parametrize('kb_form', T.KB_FORMS)
@pytest.mark.parametrize('ns', STAGE_JOBS, ids=lambda ns: 'n' + '+'.join(map(str, ns)))
def test_ode_stage_bwd_vs_float64(ns, kb_form, next_form):
    dev = _gpu()
    refs = [_stage_refs(n, kb_form, next_form) for n in ns]
    jobs = [_StageJob(dev, r[0], kb_form, next_form) for r in refs]
    _stage_launch(jobs)
    what = f'ode_stage_bwd n{"+".join(map(str, ns))} {kb_form} {next_form}'
    worst = {}
    for n, job, (_, r64, r32) in zip(ns, jobs, refs):
        got = {k: b.get(f'{what} {k}') for k, b in job.out.items()}
        for k in STAGE_OUT:
            worst[f'{k} n{n}'] = _check(k, got[k], r64[k], r32[k], what)
        if job.next is not None:
            nxt = job.next.get(f'{what} next.out')
            worst[f'next n{n}'] = _check('next', nxt, r64['next'], r32['next'], what)
            if next_form == 'next0':
                _biteq(nxt, got['dy'], 'next.out = dy without terms')
        assert bool((got['df1'][got['f1'] == 0] == 0).all()), f'{what}: df1 != 0 where the kernel\'s own f1 == 0'
        assert torch.equal(got['f1'] > 0, r64['pre'] > 0), f'{what}: a relu mask differs from float64 despite the margin'
    k = max(worst, key=worst.get)
    _worst(f'{what} (at {k})', worst[k])


# ---------------------------------------------------------------------------------------------------------------------------------------
# sttode_ode_combine
# ---------------------------------------------------------------------------------------------------------------------------------------
COMBINE_ROWS = [(1,), (17,), (4097,), (1, 17, 33, 4097)]            # 4097 x 64 elements: beyond the 1024 x 256-thread grid
COMBINE_FORMS = {1: ('plain', 'mask+relu'), 4: ('mixed',)}          # 'mixed': job i of 4 is plain | mask | relu | mask + relu


@functools.lru_cache(maxsize=None)
def _combine_case(rows, width, nterms, pad, form):
    rng = np.random.default_rng(100000 * len(rows) + 1000 * rows[-1] % 7919 + 100 * width + 10 * nterms + pad)
    ld = width + pad
    jobs = []
    for i, r in enumerate(rows):
        kind = ('plain', 'mask', 'relu', 'mask+relu')[i] if form == 'mixed' else form
        terms = [(float(np.float32(rng.uniform(-2, 2))), rng.standard_normal((r, ld)).astype(np.float32)) for _ in range(nterms)]
        mask = None
        if 'mask' in kind:
            mask = rng.standard_normal((r, ld)).astype(np.float32)
            flat = mask.reshape(-1)
            flat[0::4] = np.float32(0.0)                             # + 0.0, - 0.0, a negative and a positive entry in every group of 4
            flat[1::4] = np.float32(-0.0)
            flat[2::4] = -np.abs(flat[2::4]) - np.float32(1e-3)
            flat[3::4] = np.abs(flat[3::4]) + np.float32(1e-3)
            flat[:] = flat[rng.permutation(flat.size)]
            assert flat.size < 4 or {(float(x) > 0, bool(np.signbit(x)), float(x) == 0) for x in flat} == \
                {(True, False, False), (False, True, False), (False, False, True), (False, True, True)}
        jobs.append(dict(terms=terms, mask=mask, relu='relu' in kind, rows=r))
    return jobs, T.combine(jobs, width)


def _combine_fill(dev, jobs, width, ld, tab):
    keep, outs = [], []
    for J, j in zip(tab, jobs):
        for t, (c, v) in enumerate(j['terms']):
            d = torch.from_numpy(v).to(dev)
            keep.append(d)
            J.v[t], J.ld[t], J.c[t] = d.data_ptr(), ld, c
        out = _Buf(dev, j['rows'], width, ld)
        relu = _Buf(dev, j['rows'], width, ld) if j['relu'] else None
        if j['mask'] is not None:
            m = torch.from_numpy(j['mask']).to(dev)
            keep.append(m)
            J.mask, J.ld_mask = m.data_ptr(), ld
        if relu is not None:
            J.relu_out, J.ld_relu = relu.ptr(), ld
        J.out, J.ld_out, J.nterms, J.rows = out.ptr(), ld, len(j['terms']), j['rows']
        outs.append((out, relu))
    return keep, outs


@pytest.mark.parametrize('pad', [0, 5])
@pytest.mark.parametrize('nterms', [1, 6])
@pytest.mark.parametrize('width', [1, 3, 64])
@pytest.mark.parametrize('rows,form', [(r, f) for r in COMBINE_ROWS for f in COMBINE_FORMS[len(r)]],
                         ids=lambda v: v if isinstance(v, str) else 'rows' + 'x'.join(map(str, v)))
def test_ode_combine_vs_float64(rows, form, width, nterms, pad):
    dev = _gpu()
    capi = _capi()
    _OdeCombine, _, _ = _records()
    jobs, refs = _combine_case(rows, width, nterms, pad, form)
    tab = (_OdeCombine * len(jobs))()
    keep, outs = _combine_fill(dev, jobs, width, width + pad, tab)
    capi.call('sttode_ode_combine', tab, len(jobs), width, capi.stream_ptr())
    torch.cuda.synchronize()
    worst = 0.0
    for j, r, (out, relu) in zip(jobs, refs, outs):
        got = out.get('combine out')
        g = got.double().numpy()
        bound = R.ulps_f32(r['scale'], n=nterms + 1)
        err = np.abs(g - r['out'])
        assert (err[~r['masked']] <= bound[~r['masked']]).all(), (rows, width, nterms, float((err / bound)[~r['masked']].max()))
        assert (got.numpy()[r['masked']] == 0).all(), 'a masked element is not exactly 0'
        if j['mask'] is not None and r['masked'].size >= 64:       # (both kinds of entry are among the columns the job reads)
            assert r['masked'].any() and (~r['masked']).any()
        worst = max(worst, float((err / bound)[~r['masked']].max()) if (~r['masked']).any() else 0.0)
        if relu is not None:
            _biteq(relu.get('combine relu_out'), torch.clamp_min(got, 0.0), 'relu_out = max(out, 0)')
    _worst(f'ode_combine rows{"x".join(map(str, rows))} w{width} t{nterms} pad{pad} {form}', worst)


# ---------------------------------------------------------------------------------------------------------------------------------------
# refusals: each is refused by the host code before any launch, and no output is written
# ---------------------------------------------------------------------------------------------------------------------------------------
_TCASE = (5, 8, 128, True, True)


def _refused(fn):
    with pytest.raises(_capi().SttodeError):
        fn()
    torch.cuda.synchronize()


@pytest.mark.parametrize('bad', ['T13', 'ld124', 'ld130', 'phase3', 'count', 'null_xc', 'null_fc2_w', 'null_attn_phase2'])
def test_ttrunk_fwd_refuses(bad):
    dev = _gpu()
    n, T_, ld, drop, last = _TCASE
    case = T.trunk_case(n, 13, drop, last) if bad == 'T13' else _trunk_refs(n, T_, drop, last)[0]      # (buffers of T = 13 frames)
    null = {'null_xc': ('xc',), 'null_fc2_w': ('fc2_w',)}.get(bad, ())
    t = _Trunk(dev, case, 132 if bad in ('ld124', 'ld130') else ld, null=null)
    kw = {'ld124': dict(ld_feat=124), 'ld130': dict(ld_feat=130), 'phase3': dict(phase=3), 'count': dict(count=len(_capi().TRUNK_PTRS) - 1),
          'null_attn_phase2': dict(phase=2)}.get(bad, {})            # (phase 2: attn stays None)
    _refused(lambda: t.launch(**kw))
    assert t.untouched()


@pytest.mark.parametrize('bad', ['T13', 'ld124', 'ld130', 'count', 'null_xc', 'null_ys', 'trunks0', 'trunks3', 'stages2', 'steps0'])
def test_ttrunk_ode_fwd_refuses(bad):
    dev = _gpu()
    n, T_, ld, drop, last = _TCASE
    case = _trunk_refs(n, T_, drop, last)[0]
    t = _Trunk(dev, case, 132, null=('xc',) if bad == 'null_xc' else ())
    prog = _program('rk4', 2, 12.0)
    kw = {}
    if bad == 'T13':
        kw = dict(T_=[13])
    elif bad in ('ld124', 'ld130'):
        kw = dict(ld_feat=[int(bad[2:])])
    elif bad == 'count':
        kw = dict(count=len(_capi().TRUNK_PTRS) + 1)
    elif bad == 'null_ys':
        kw = dict(null_ys=True)
    elif bad in ('trunks0', 'trunks3'):
        kw = dict(ntrunks=int(bad[-1]))
    elif bad == 'stages2':
        prog.stages = 2
    elif bad == 'steps0':
        prog.steps = 0
    ys, yT = _ode_bufs(dev, [t], prog)                              # (made before the call: inspected after the refusal)
    _refused(lambda: _ode_launch([t], prog, ys, yT, **kw))
    assert t.untouched() and ys[0].untouched() and yT[0].untouched()


@pytest.mark.parametrize('bad', ['count0', 'count5', 'width0', 'nterms0', 'nterms7', 'ld_term', 'ld_out', 'ld_mask', 'ld_relu', 'null_term',
                                 'null_out'])
def test_ode_combine_refuses(bad):
    dev = _gpu()
    capi = _capi()
    _OdeCombine, _, _ = _records()
    width, pad = 3, 5
    jobs, _ = _combine_case((17,), width, 6, pad, 'mask+relu')
    tab = (_OdeCombine * 5)()                                        # (five records: a refused count of 5 reads none of them)
    keep, outs = _combine_fill(dev, jobs, width, width + pad, tab)
    J, count, w = tab[0], 1, width
    if bad == 'count0':
        count = 0
    elif bad == 'count5':
        count = 5
    elif bad == 'width0':
        w = 0
    elif bad == 'nterms0':
        J.nterms = 0
    elif bad == 'nterms7':
        J.nterms = 7
    elif bad == 'ld_term':
        J.ld[4] = width - 1
    elif bad == 'ld_out':
        J.ld_out = width - 1
    elif bad == 'ld_mask':
        J.ld_mask = width - 1
    elif bad == 'ld_relu':
        J.ld_relu = width - 1
    elif bad == 'null_term':
        J.v[5] = None
    elif bad == 'null_out':
        J.out = None
    _refused(lambda: capi.call('sttode_ode_combine', tab, count, w, capi.stream_ptr()))
    assert all(b.untouched() for pair in outs for b in pair if b is not None)


@pytest.mark.parametrize('bad', ['count0', 'count3', 'null_dy', 'null_ln', 'null_weight', 'kb0', 'kb_ld', 'next_ld_term', 'next_ld_out', 'n0',
                                 'second_job_null_df1'])
def test_ode_stage_bwd_refuses(bad):
    dev = _gpu()
    two = bad == 'second_job_null_df1'
    jobs = [_StageJob(dev, _stage_refs(n, 'kb4strided', 'next5')[0], 'kb4strided', 'next5') for n in ((17, 5) if two else (5,))]
    count = {'count0': 0, 'count3': 3}.get(bad)

    def edit(tab):
        J = tab[0]
        if bad == 'null_dy':
            J.dy = None
        elif bad == 'null_ln':
            J.ln = None
        elif bad == 'null_weight':
            J.w[11] = None
        elif bad == 'kb0':
            J.kb.nterms = 0
        elif bad == 'kb_ld':
            J.kb.ld[2] = 63
        elif bad == 'next_ld_term':
            J.next.ld[3] = 60
        elif bad == 'next_ld_out':
            J.next.ld_out = 63
        elif bad == 'n0':
            J.n = 0
        elif two:
            tab[1].df1 = None
    _refused(lambda: _stage_launch(jobs, count=count, edit=edit))
    assert all(b.untouched() for job in jobs for b in job.bufs())
