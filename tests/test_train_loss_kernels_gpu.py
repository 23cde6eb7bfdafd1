"""Direct float64 tests of the loss, live-column, attention-backward and stage-2 sampler entry points (csrc/train.hip, train_ewise.hip
live_rows_gather, train_attn.hip attn_bwd / attn_bwd_pairs, sampler.hip), called through capi.call at the shapes where their code paths
change.  A sibling of tests/test_train_kernels_gpu.py with the same yardstick (tests/train_ref.py):
|hip - f64| <= max(4 |torch_fp32 - f64|, atol + rtol |f64|) per element, f64 the same operation in float64 on the very fp32 inputs the kernel
received; integer outputs and row shuffles are bitwise.  Every output sits inside a larger buffer: its interior starts as NaN (or a
sentinel), so an element the kernel does not write fails, and its margins must keep their sentinel.

The inputs obey conditions that are checked on the CPU while they are built, so that which side of a branch a case takes is never an
accident of a seed: every scene's float64 KL lies at least 10 % away from min_clip; every agent's smallest and second-smallest float64
distance differ by more than 1e-5 relative (apart from the constructed bit-for-bit ties); no attention pair lies within 1e-6 of the
acos clamp."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import train_ref as R

from test_train_kernels_gpu import SENT, _capi, _close, _gpu, _worst

pytestmark = pytest.mark.gpu

ISENT = -99
MIN_CLIP = 2.0


class _Out:
    """An output of ``shape`` inside a larger buffer: margins of sentinels on both sides, the interior ``.v`` filled with ``fill``."""

    def __init__(self, dev, shape, fill=float('nan'), dtype=torch.float32, margin=8):
        self.n, self.m = int(np.prod(shape)), margin
        self.sent = SENT if dtype.is_floating_point else ISENT
        self.buf = torch.full((self.n + 2 * margin,), self.sent, dtype=dtype, device=dev)
        self.v = self.buf[margin:margin + self.n].view(shape)
        self.v.fill_(fill)

    def margins_ok(self):
        b = self.buf.cpu()
        return bool((b[:self.m] == self.sent).all() and (b[self.m + self.n:] == self.sent).all())

    def untouched(self):
        return bool((self.buf == self.sent).all())


def _dev(dev, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the objective of forward(): sttode_loss_objective, its live form, and the three stand-alone entry points
# ---------------------------------------------------------------------------------------------------------------------------------------
# (n, K1, D, Dp, zd): one agent and K = 1 | NBA shapes | the shape of test_fused_objective_kernel_vs_the_three_loss_entry_points | more than
# 256 agents (the stride loops of objective_sum_kernel) and a long horizon | K = 64 fills the wave, D and Dp beyond 256 (the per-agent
# stride loops)
LOSS_CASES = [(1, 2, 24, 16, 32), (2, 21, 20, 10, 16), (37, 21, 24, 16, 32), (300, 21, 80, 20, 64), (5, 65, 258, 260, 32)]
# scene CSRs per n: one-agent scenes, a single-scene CSR (S = 1), a scene of more than 256 agents
LOSS_CSRS = {1: [(0, 1)], 2: [(0, 1, 2)], 37: [(0, 5, 6, 20, 37)], 300: [(0, 7, 8, 290, 300)], 5: [(0, 5), (0, 2, 3, 5)]}
# constructed ties per n: (agent, index of the winner, index of its bit-for-bit duplicate), 0-based among the K prior samples = the lane of
# the best-of-K butterfly.  K = 64: pairs across lane 32 in both orders, both above it, and the two lanes next to it.
LOSS_TIES = {1: [], 2: [(0, 12, 7)], 37: [(0, 0, 19), (5, 19, 0), (6, 3, 4), (36, 17, 9)], 300: [(0, 1, 2), (256, 19, 5), (299, 0, 19)],
             5: [(0, 5, 50), (1, 50, 5), (2, 33, 60), (3, 32, 31)]}
LOSS_PARAMS = [(case, csr, mode) for case in LOSS_CASES for csr in [None] + LOSS_CSRS[case[0]]
               for mode in ('clamped', 'live') + (('mixed',) if csr is not None and len(csr) > 2 else ())]
_loss_id = lambda p: 'n%d-K1_%d-D%d-Dp%d-zd%d-%s-%s' % (*p[0], 'one' if p[1] is None else 'csr' + 'x'.join(map(str, p[1])), p[2])


@functools.lru_cache(maxsize=None)
def _loss_inputs(case, csr, mode):
    """fp32 inputs of one case, its float64 and torch-fp32 references (computed once, shared, never written), and the input conditions."""
    n, K1, D, Dp, zd = case
    rng = np.random.default_rng(1000 * n + K1 + (len(csr) if csr else 0) * 7 + {'clamped': 0, 'live': 1, 'mixed': 2}[mode])
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    pred, rec, fut, past = f(n, K1, D), f(n, K1, Dp), f(n, D), f(n, Dp)
    for a, w, dup in LOSS_TIES[n]:
        pred[a, 1 + w] = fut[a] + np.float32(1e-3) * f(D)            # the winner: the target plus small noise
        pred[a, 1 + dup] = pred[a, 1 + w]                            # ... and its duplicate, bit for bit
    # KL: 0.1 randn rows sit below min_clip, 0.6 randn rows above; per scene, the scale moves on until the float64 value is 10 % away
    ptr = np.array(csr if csr is not None else (0, n))
    S = len(ptr) - 1
    want_live = [mode == 'live' or (mode == 'mixed' and s % 2 == 1) for s in range(S)]
    base = f(n, 2 * zd)
    qzp = np.empty_like(base)
    for s in range(S):
        a, b = ptr[s], ptr[s + 1]
        denom = float(b - a) if csr is not None else float(n)
        sc = 0.6 if want_live[s] else 0.1
        for _ in range(40):
            rows = (np.float32(sc) * base[a:b]).astype(np.float32)
            v = float(R.kl_rows(torch.from_numpy(rows).double()).sum()) / denom
            if (v >= 1.1 * MIN_CLIP) if want_live[s] else (v <= 0.9 * MIN_CLIP):
                break
            sc = sc * 1.25 if want_live[s] else sc / 1.25
        qzp[a:b] = rows
    sm, sr = 2.0 / D, 2.0 / Dp                                       # 1 / (B Tf), 1 / (B Tp) with B = 1
    t32 = [torch.from_numpy(v) for v in (pred, rec, fut, past, qzp)]
    r64 = R.objective(*[v.double() for v in t32], csr, K1, sm, sr, float(n), MIN_CLIP)
    r32 = R.objective(*t32, csr, K1, sm, sr, float(n), MIN_CLIP)
    kls = R.scene_kl(t32[4].double(), csr, float(n)).numpy()
    assert (np.abs(kls - MIN_CLIP) >= 0.1 * MIN_CLIP).all() and np.array_equal(kls > MIN_CLIP, want_live), (kls, want_live)
    # best-of-K: no agent's minimum is an accident of rounding
    d2 = np.sort(r64['d2'].numpy(), axis=1)
    tied = {a for a, _, _ in LOSS_TIES[n]}
    for a in range(n):
        if a in tied:
            assert d2[a, 0] == d2[a, 1]
        rest = d2[a, (2 if a in tied else 1):]
        assert rest.size == 0 or rest[0] - d2[a, 0] > 1e-5 * rest[0], (a, d2[a, :3])
    best = r64['best'].numpy()
    for a, w, dup in LOSS_TIES[n]:
        assert best[a] == 1 + min(w, dup)
    assert np.array_equal(best, r32['best'].numpy())
    return dict(case=case, csr=csr, S=S if csr is not None else 0, ptr=ptr, ags=R.scene_of(ptr, n).astype(np.int32), live_scene=kls > MIN_CLIP,
                np=(pred, rec, fut, past, qzp), sm=sm, sr=sr, r64=r64, r32=r32)


def _objective_call(capi, dev, inp, live, scratch_floats=None, fill=float('nan'), refused=False, **over):
    """One sttode_loss_objective(_live) call with the documented minimum of scratch.  -> dict of _Out (out, dpred, drec, dqzp, best,
    scratch)."""
    n, K1, D, Dp, zd = inp['case']
    csr = inp['csr']
    P, Rc, F_, PA, Q = (_dev(dev, v) for v in inp['np'])
    a = dict(sp=_dev(dev, np.asarray(csr, np.int32)) if csr is not None else None, ag=_dev(dev, inp['ags']) if csr is not None else None,
             S=inp['S'], K1=K1, kl_denom=float(n), with_best=live)
    a.update(over)
    rows = 2 if live else K1
    need = 3 * n + (inp['S'] if csr is not None else n)
    o = dict(out=_Out(dev, (5,), fill), dpred=_Out(dev, (n, rows, D), fill), drec=_Out(dev, (n, rows, Dp), fill), dqzp=_Out(dev, (n, 2 * zd), fill),
             best=_Out(dev, (n,), ISENT, torch.int32), scratch=_Out(dev, (need,), SENT))
    head = (P, Rc, F_, PA, Q, a['sp'], a['ag'], a['S'], n, a['K1'], D, Dp, zd, inp['sm'], inp['sr'], a['kl_denom'], MIN_CLIP, o['out'].v, o['dpred'].v,
            o['drec'].v, o['dqzp'].v)
    tail = (o['scratch'].v, need if scratch_floats is None else scratch_floats, capi.stream_ptr())
    def go():
        if live:
            capi.call('sttode_loss_objective_live', *head, o['best'].v if a['with_best'] else None, *tail)
        else:
            capi.call('sttode_loss_objective', *head, *tail)
    if refused:
        with pytest.raises(capi.SttodeError):
            go()
    else:
        go()
    torch.cuda.synchronize()
    return o


def _exact_loss_properties(inp, dpred_dense, dqzp, kl_value, what):
    """What must hold to the bit: the clamped scenes' value and zero gradient rows; one live prior row per agent, the reference's."""
    n, K1 = inp['case'][0], inp['case'][1]
    live_row = torch.from_numpy(inp['live_scene'][R.scene_of(inp['ptr'], n)])
    dq = dqzp.cpu()
    assert (dq[~live_row] == 0).all(), f'{what}: a clamped scene passes a gradient to its rows'
    assert (dq[live_row] != 0).any(1).all(), f'{what}: a live scene has a zero gradient row'
    if not inp['live_scene'].any():
        assert float(kl_value) == MIN_CLIP * len(inp['live_scene']), f'{what}: the clamped value is not min_clip'
    if dpred_dense is not None:
        nz = (dpred_dense.cpu() != 0).any(-1)                         # [n, K]: the rows of the prior samples with a gradient
        assert (nz.sum(1) == 1).all(), f'{what}: not exactly one prior sample per agent has a gradient'
        assert torch.equal(nz.int().argmax(1).int() + 1, inp['r64']['best']), f'{what}: the gradient went to another sample than the first minimum'


@pytest.mark.parametrize('param', LOSS_PARAMS, ids=_loss_id)
def test_fused_objective_and_the_three_loss_entry_points_vs_float64(param):
    """sttode_loss_objective: its five values and three gradients against float64; what the older sibling-kernel comparison asserts (values
    of the fused call within 2e-6 of sttode_loss_sqerr / _kl / _diverse on the slices, gradients bit for bit, zero rows of drec); the
    stand-alone entry points' own values against float64, with and without their optional gradient."""
    capi, dev = _capi(), _gpu()
    st = capi.stream_ptr()
    inp = _loss_inputs(*param)
    n, K1, D, Dp, zd = inp['case']
    K, r64, r32, S, csr = K1 - 1, inp['r64'], inp['r32'], inp['S'], inp['csr']
    what = 'objective ' + _loss_id(param)
    o = _objective_call(capi, dev, inp, False)
    worst = {}
    vals = o['out'].v.cpu()
    for i, k in enumerate(('mse', 'rec', 'kl', 'diverse', 'total')):
        worst['value ' + k] = _close(vals[i:i + 1], r64[k].reshape(1), r32[k].reshape(1), f'{what} {k}')
    for k in ('dpred', 'drec', 'dqzp'):
        worst[k] = _close(o[k].v, r64[k], r32[k], f'{what} {k}')
    assert (o['drec'].v[:, 1:] == 0).all()
    _exact_loss_properties(inp, o['dpred'].v[:, 1:], o['dqzp'].v, vals[2], what)
    for k, v in o.items():
        assert v.margins_ok(), f'{what}: wrote outside {k}'
    assert (o['best'].v == ISENT).all()
    # the three stand-alone entry points on the slices
    P, Rc, F_, PA, Q = (_dev(dev, v) for v in inp['np'])
    sp, ag = (_dev(dev, np.asarray(csr, np.int32)), _dev(dev, inp['ags'])) if csr is not None else (None, None)
    p0, r0, pk = P[:, 0].contiguous(), Rc[:, 0].contiguous(), P[:, 1:].contiguous()
    ref, ref_nograd = _Out(dev, (4,)), _Out(dev, (4,))
    g0, g1, gq, gk = _Out(dev, (n, D)), _Out(dev, (n, Dp)), _Out(dev, (n, 2 * zd)), _Out(dev, (n, K, D))
    skl, sdv = _Out(dev, (max(S, 1),), SENT), _Out(dev, (n,), SENT)
    capi.call('sttode_loss_sqerr', p0, F_, n * D, inp['sm'], ref.v[0:], g0.v, st)
    capi.call('sttode_loss_sqerr', r0, PA, n * Dp, inp['sr'], ref.v[1:], g1.v, st)
    capi.call('sttode_loss_kl', Q, sp, S, n, zd, float(n), MIN_CLIP, ref.v[2:], gq.v, skl.v, st)
    capi.call('sttode_loss_diverse', pk, F_, sp, ag, n, K, D, ref.v[3:], gk.v, sdv.v, st)
    capi.call('sttode_loss_sqerr', p0, F_, n * D, inp['sm'], ref_nograd.v[0:], None, st)
    capi.call('sttode_loss_sqerr', r0, PA, n * Dp, inp['sr'], ref_nograd.v[1:], None, st)
    capi.call('sttode_loss_kl', Q, sp, S, n, zd, float(n), MIN_CLIP, ref_nograd.v[2:], None, skl.v, st)
    capi.call('sttode_loss_diverse', pk, F_, sp, ag, n, K, D, ref_nograd.v[3:], None, sdv.v, st)
    torch.cuda.synchronize()
    r = ref.v.cpu()
    np.testing.assert_allclose(vals[:4].numpy(), r.numpy(), rtol=2e-6)
    np.testing.assert_allclose(vals[4].item(), r.numpy().sum(), rtol=2e-6)
    assert torch.equal(o['dpred'].v[:, 0], g0.v) and torch.equal(o['drec'].v[:, 0], g1.v) and torch.equal(o['dqzp'].v, gq.v)
    assert torch.equal(o['dpred'].v[:, 1:], gk.v)
    assert torch.equal(ref.v, ref_nograd.v), f'{what}: an entry point\'s value depends on whether it writes its gradient'
    for i, k in enumerate(('mse', 'rec', 'kl', 'diverse')):
        worst['entry ' + k] = _close(r[i:i + 1], r64[k].reshape(1), r32[k].reshape(1), f'{what} entry point {k}')
    _exact_loss_properties(inp, gk.v, gq.v, r[2], what + ' entry points')
    for k, v in dict(ref=ref, ref_nograd=ref_nograd, g0=g0, g1=g1, gq=gq, gk=gk, skl=skl, sdv=sdv).items():
        assert v.margins_ok(), f'{what}: an entry point wrote outside {k}'
    k = max(worst, key=worst.get)
    _worst(f'loss family {_loss_id(param)} (at {k})', worst[k])


@pytest.mark.parametrize('param', LOSS_PARAMS, ids=_loss_id)
def test_live_objective_is_bitwise_the_dense_objective_on_its_two_rows(param):
    capi, dev = _capi(), _gpu()
    inp = _loss_inputs(*param)
    n = inp['case'][0]
    what = 'live objective ' + _loss_id(param)
    dense = _objective_call(capi, dev, inp, False)
    live = _objective_call(capi, dev, inp, True)
    best = live['best'].v.cpu()
    assert torch.equal(best, inp['r64']['best']), f'{what}: best {best.tolist()} != {inp["r64"]["best"].tolist()}'
    assert torch.equal(live['out'].v, dense['out'].v) and torch.equal(live['dqzp'].v, dense['dqzp'].v)
    dp, dp2 = dense['dpred'].v.cpu(), live['dpred'].v.cpu()
    assert torch.equal(dp2[:, 0], dp[:, 0])
    assert torch.equal(dp2[:, 1], dp[torch.arange(n), best.long()])
    others = torch.ones(dp.shape[:2], dtype=torch.bool)
    others[:, 0] = False
    others[torch.arange(n), best.long()] = False
    assert (dp[others] == 0).all()
    dr, dr2 = dense['drec'].v.cpu(), live['drec'].v.cpu()
    assert torch.equal(dr2[:, 0], dr[:, 0]) and (dr2[:, 1] == 0).all() and (dr[:, 1:] == 0).all()
    _exact_loss_properties(inp, None, live['dqzp'].v, live['out'].v[2].cpu(), what)
    for k, v in live.items():
        assert v.margins_ok(), f'{what}: wrote outside {k}'


@pytest.mark.parametrize('with_dpred', [True, False])
def test_sqerr_vs_float64(with_dpred):
    """One workgroup of 256 threads: one element, one short of a full pass, a full pass, one more, and NBA's 32 x 11 x 20 elements."""
    capi, dev = _capi(), _gpu()
    st = capi.stream_ptr()
    rng = np.random.default_rng(41)
    worst = 0.0
    for count in (1, 255, 256, 257, 7040):
        p, t = rng.standard_normal(count).astype(np.float32), rng.standard_normal(count).astype(np.float32)
        scale = 1.0 / 7
        out, g = _Out(dev, (1,)), _Out(dev, (count,))
        capi.call('sttode_loss_sqerr', _dev(dev, p), _dev(dev, t), count, scale, out.v, g.v if with_dpred else None, st)
        torch.cuda.synchronize()
        a = [torch.from_numpy(p), torch.from_numpy(t)]
        r64, r32 = R.sqerr(a[0].double(), a[1].double(), scale), R.sqerr(*a, scale)
        worst = max(worst, _close(out.v, r64['value'].reshape(1), r32['value'].reshape(1), f'sqerr count={count} value'))
        if with_dpred:
            worst = max(worst, _close(g.v, r64['dpred'], r32['dpred'], f'sqerr count={count} dpred'))
        else:
            assert torch.isnan(g.v).all()
        assert out.margins_ok() and g.margins_ok(), count
    _worst(f'sqerr dpred={with_dpred}', worst)


def test_loss_refusals_write_nothing():
    """K1 outside 2..65, scratch one float short of 3 n + max(S, n), a CSR without agent_scene, kl_denom = 0 without a CSR, and for the live
    form a null best: each raises, and every output keeps its sentinel."""
    capi, dev = _capi(), _gpu()
    inp = _loss_inputs((37, 21, 24, 16, 32), None, 'live')
    inp_csr = _loss_inputs((2, 21, 20, 10, 16), (0, 1, 2), 'mixed')          # S == n: 3 n + S == 3 n + max(S, n)
    bad = [('K1 = 1', inp, dict(K1=1)), ('K1 = 66', inp, dict(K1=66)), ('scratch one float short', inp, dict(scratch_floats=4 * 37 - 1)),
           ('scratch one float short, CSR', inp_csr, dict(scratch_floats=3 * 2 + 2 - 1)), ('a CSR without agent_scene', inp_csr, dict(ag=None)),
           ('kl_denom = 0 without a CSR', inp, dict(kl_denom=0.0))]
    for live in (False, True):
        for label, case, over in bad + ([('a null best', inp, dict(with_best=False))] if live else []):
            o = _objective_call(capi, dev, case, live, fill=SENT, refused=True, **over)
            for k, v in o.items():
                assert v.untouched(), f'{label} (live={live}): refused, but wrote {k}'


# ---------------------------------------------------------------------------------------------------------------------------------------
# sttode_live_rows_gather: bitwise against NumPy indexing
# ---------------------------------------------------------------------------------------------------------------------------------------
class _GatherItem(ctypes.Structure):                 # include/sttode_hip.h sttode_live_rows_gather: 40 bytes
    _fields_ = [('src', ctypes.c_void_p), ('dst', ctypes.c_void_p), ('src_plane', ctypes.c_long), ('dst_plane', ctypes.c_long),
                ('row', ctypes.c_int), ('outer', ctypes.c_int)]


# (row floats, planes, source offset in floats, floats between planes beyond the plane itself): rows of 96 and 512 floats on 16-byte
# addresses, the same one float off them, rows that are no multiple of four floats (2, 30) and one that is (24), planes further apart than
# they are long (by a multiple of four floats, and not)
GATHER_SPECS = [(96, 1, 0, 0), (512, 1, 0, 0), (2, 1, 0, 0), (24, 1, 0, 0), (30, 1, 0, 0), (96, 1, 1, 0), (512, 3, 1, 3), (96, 4, 0, 8), (24, 2, 0, 5),
                (30, 3, 0, 2), (2, 5, 1, 1), (512, 2, 0, 4)]


def _gather_case(dev, rng, n, K1, count, best):
    """-> (table, sources, [(destination buffer, its expected content)])."""
    items, keep, outs = [], [], []
    bc = np.clip(best, 0, K1 - 1)                                   # the kernel clamps a `best` nobody wrote to rows 0 and K1 - 1, by design
    for i in range(count):
        row, outer, off, gap = GATHER_SPECS[i % len(GATHER_SPECS)]
        sp_, dp_ = n * K1 * row + gap, 2 * n * row + gap
        src = rng.standard_normal(off + outer * sp_).astype(np.float32)
        lead = 4 if i % 3 else 5                                    # the destination on a 16-byte address, or one float off it
        dst = np.full(lead + outer * dp_ + 7, SENT, np.float32)
        exp = dst.copy()
        for o in range(outer):
            s = src[off + o * sp_: off + o * sp_ + n * K1 * row].reshape(n, K1, row)
            d = exp[lead + o * dp_: lead + o * dp_ + 2 * n * row].reshape(n, 2, row)
            d[:, 0] = s[:, 0]
            d[:, 1] = s[np.arange(n), bc]
        sd, dd = _dev(dev, src), _dev(dev, dst)
        keep += [sd, dd]
        items.append(_GatherItem(sd.data_ptr() + 4 * off, dd.data_ptr() + 4 * lead, sp_, dp_, row, outer))
        outs.append((dd, exp))
    return (_GatherItem * count)(*items), keep, outs


def test_live_rows_gather_is_bitwise_numpy_indexing():
    capi, dev = _capi(), _gpu()
    st = capi.stream_ptr()
    rng = np.random.default_rng(42)
    for n, K1, count in ((1, 2, 1), (1, 21, 32), (37, 21, 1), (37, 21, 32), (37, 65, 12)):
        best = rng.integers(1, K1, n).astype(np.int32)
        variants = [best]
        if n > 1:
            wild = best.copy()
            wild[3], wild[5], wild[n - 1] = -7, K1 + 3, K1 - 1
            variants.append(wild)
        else:
            variants += [np.array([-7], np.int32), np.array([K1 + 3], np.int32)]
        for bv in variants:
            table, keep, outs = _gather_case(dev, rng, n, K1, count, bv)
            capi.call('sttode_live_rows_gather', table, count, _dev(dev, bv), n, K1, st)
            torch.cuda.synchronize()
            for i, (dd, exp) in enumerate(outs):
                assert np.array_equal(dd.cpu().numpy(), exp), f'gather n={n} K1={K1} count={count} item {i} {GATHER_SPECS[i % len(GATHER_SPECS)]} best={bv.tolist()}'
    # refused: 33 tensors, a null best -- nothing is written
    table, keep, outs = _gather_case(dev, rng, 3, 4, 32, np.array([1, 2, 3], np.int32))
    big = (_GatherItem * 33)(*(list(table) + [table[0]]))
    bd = _dev(dev, np.array([1, 2, 3], np.int32))
    with pytest.raises(capi.SttodeError):
        capi.call('sttode_live_rows_gather', big, 33, bd, 3, 4, st)
    with pytest.raises(capi.SttodeError):
        capi.call('sttode_live_rows_gather', table, 32, None, 3, 4, st)
    torch.cuda.synchronize()
    for dd, _ in outs:
        assert (dd == SENT).all()


# ---------------------------------------------------------------------------------------------------------------------------------------
# sttode_mhgsa_attn_bwd: one thread per row, and the pair-parallel form where L >= 4 and its L x L terms fit the LDS
# ---------------------------------------------------------------------------------------------------------------------------------------
def _attn_form(L, hd):
    """The host's choice (csrc/train_attn.hip sttode_mhgsa_attn_bwd): 3 L^2 + L (4 hd + 4) floats within 150 KiB."""
    return 'pairs' if L >= 4 and 4 * (3 * L * L + L * (4 * hd + 4)) <= 150 * 1024 else 'row'


# smallest L and the switch at L = 4 | the last pair-form L and the first row-form L at head_dim 8, 4, 16 | the row form past 256 threads
ATTN_CASES = [(1, 3, 8, 'row'), (2, 3, 8, 'row'), (3, 2, 8, 'row'), (4, 2, 8, 'pairs'), (107, 1, 8, 'pairs'), (108, 1, 8, 'row'), (109, 1, 4, 'pairs'),
              (110, 1, 4, 'row'), (102, 1, 16, 'pairs'), (103, 1, 16, 'row'), (257, 1, 8, 'row'), (300, 1, 8, 'row')]
ATTN_CLAMP_CASES = [(16, 2, 8, 'pairs'), (3, 2, 8, 'row'), (128, 1, 8, 'row')]


@functools.lru_cache(maxsize=None)
def _attn_inputs(L, Nb, hd, clamp):
    """qkv, dO from the seed rule 100 L + hd (reseeded while a pair lies within 1e-6 of the clamp), the two references, and how many pairs
    lie beyond the clamp.  ``clamp``: in heads 0 and 5 k_i = q_i for three rows (the diagonal dot is 1), in head 2 k_i = -q_j for two pairs."""
    DM = 8 * hd
    seed = 100 * L + hd
    for _ in range(8):
        g = torch.Generator().manual_seed(seed)
        qkv = torch.randn(L * Nb, 3 * DM, generator=g)
        dO = torch.randn(L * Nb, DM, generator=g)
        if clamp:
            x = qkv.view(L, Nb, 3, 8, hd)
            for h in (0, 5):
                for i in sorted({0, L // 2, L - 1}):
                    x[i, :, 1, h] = x[i, :, 0, h]
            for i, j in ((0, L - 1), (1, 0)):
                x[i, :, 1, 2] = -x[j, :, 0, 2]
        r64 = R.geodesic_self_attention(qkv.double(), dO.double(), L, Nb, hd)
        near = ((r64['dots'].abs() - (1 - R.ATTN_CLAMP)).abs() < 1e-6).sum().item()
        if near == 0:
            break
        seed += 1000003
    assert near == 0
    r32 = R.geodesic_self_attention(qkv, dO, L, Nb, hd)
    return qkv, dO, r64, r32, int((r64['dots'].abs() > 1 - R.ATTN_CLAMP).sum().item())


def _attn_run(L, Nb, hd, form, clamp):
    capi, dev = _capi(), _gpu()
    assert _attn_form(L, hd) == form, f'L={L} head_dim={hd}: the case was chosen for the {form} form'
    qkv, dO, r64, r32, beyond = _attn_inputs(L, Nb, hd, clamp)
    got = _Out(dev, (L * Nb, 24 * hd))
    capi.call('sttode_mhgsa_attn_bwd', qkv.to(dev), dO.to(dev), got.v, L, Nb, hd, capi.stream_ptr())
    torch.cuda.synchronize()
    w = _close(got.v, r64['dqkv'], r32['dqkv'], f'attn_bwd L={L} Nb={Nb} hd={hd} {form} clamp={clamp} ({beyond} pairs beyond the clamp)')
    assert got.margins_ok()
    _worst(f'attn_bwd {form} L={L} Nb={Nb} hd={hd} clamp={clamp} ({beyond} pairs beyond the clamp)', w)
    return beyond


@pytest.mark.parametrize('L,Nb,hd,form', ATTN_CASES)
def test_attention_backward_forms_vs_float64(L, Nb, hd, form):
    """Both sides of every switch between the two forms, L = 1 and 2, and the row form's stride loops.  (L = 1: the softmax is over one key,
    so the reference has dq = dk = 0 and dv = dO.)  (109, 1, 4) holds a pair beyond the clamp by nature: a wanted case."""
    beyond = _attn_run(L, Nb, hd, form, False)
    if (L, Nb, hd) == (109, 1, 4):
        assert beyond >= 1


def test_attention_backward_form_switch_sits_where_the_cases_expect_it():
    """3 L^2 + L (4 hd + 4) floats <= 150 KiB: the last pair-form L is 107 at head_dim 8, 109 at 4, 102 at 16."""
    for hd, last in ((8, 107), (4, 109), (16, 102)):
        assert _attn_form(last, hd) == 'pairs' and _attn_form(last + 1, hd) == 'row' and _attn_form(4, hd) == 'pairs' and _attn_form(3, hd) == 'row'


@pytest.mark.parametrize('L,Nb,hd,form', ATTN_CLAMP_CASES)
def test_attention_backward_pairs_beyond_the_clamp_vs_float64(L, Nb, hd, form):
    """k_i = q_i and k_i = -q_j: those pairs contribute nothing to dq and dk, and their full softmax weight to dv."""
    beyond = _attn_run(L, Nb, hd, form, True)
    assert beyond >= Nb * (2 * len({0, L // 2, L - 1}) + 2)


# ---------------------------------------------------------------------------------------------------------------------------------------
# stage-2 sampler: sttode_sampler_latent, sttode_sampler_loss, sttode_sampler_loss_bwd
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', [0, 1, 2])
def test_sampler_latent_vs_float64(mode):
    """Totals that are no multiple of the 256-thread workgroup; entries of A at 0, +-1e-6 and +-1e-4 (logvar down to log 1e-8)."""
    capi, dev = _capi(), _gpu()
    st = capi.stream_ptr()
    rng = np.random.default_rng(43 + mode)
    worst = 0.0
    for n, K, nz in ((1, 1, 5), (3, 20, 32), (9, 7, 33)):
        A = rng.standard_normal((n * K, nz)).astype(np.float32)
        small = np.array([0.0, 1e-6, -1e-6, 1e-4, -1e-4], np.float32)
        A.ravel()[:: max(A.size // 5, 1)][:5] = small
        assert set(small.tolist()) <= set(A.ravel().tolist())
        b = rng.standard_normal((n * K, nz)).astype(np.float32)
        eps = None if mode == 0 else rng.standard_normal(nz if mode == 1 else (n, nz)).astype(np.float32)
        z, lv = _Out(dev, (n * K, nz)), _Out(dev, (n * K, nz))
        capi.call('sttode_sampler_latent', _dev(dev, A), _dev(dev, b), _dev(dev, eps), mode, z.v, lv.v, n, K, nz, st)
        torch.cuda.synchronize()
        a = [torch.from_numpy(A), torch.from_numpy(b), None if eps is None else torch.from_numpy(eps)]
        r64 = R.sampler_latent(*[None if v is None else v.double() for v in a], mode, K)
        r32 = R.sampler_latent(*a, mode, K)
        for k, got in (('z', z), ('logvar', lv)):
            worst = max(worst, _close(got.v, r64[k], r32[k], f'sampler_latent mode={mode} n={n} K={K} nz={nz} {k}'))
            assert got.margins_ok()
    _worst(f'sampler_latent mode {mode}', worst)


# (n, K, nz, D): one pair | the shape of the older test | K nz no multiple of 64 | K D = 4096, all of the LDS
SAMPLER_CASES = [(1, 2, 5, 4), (19, 20, 32, 24), (3, 3, 5, 20), (2, 64, 32, 64)]


@functools.lru_cache(maxsize=None)
def _sampler_inputs(case, prior, scale):
    n, K, nz, D = case
    rng = np.random.default_rng(44 + 10 * n + K + (1 if prior else 0))
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    mu, lv = f(n * K, nz), np.float32(0.5) * f(n * K, nz)
    pmu, plv = (np.float32(0.5) * f(n * K, nz), np.float32(0.5) * f(n * K, nz)) if prior else (None, None)
    # samples around a per-agent centre, spread so that |m_i - m_j|^2 / scale is of order one (each pair's term counts)
    motion = (f(n, 1, D) + np.float32(np.sqrt(scale / (2 * D))) * f(n, K, D)).astype(np.float32)
    if K > 2:
        motion[n - 1, K - 1] = motion[n - 1, 0]                     # two samples identical bit for bit: exp(0) forward, no gradient through it
    g_kld, g_div = f(n), f(n)
    a = [None if v is None else torch.from_numpy(v) for v in (mu, lv, pmu, plv, motion)]
    g = [torch.from_numpy(g_kld), torch.from_numpy(g_div)]
    r64 = R.sampler_loss(*[None if v is None else v.double() for v in a], scale, g[0].double(), g[1].double())
    r32 = R.sampler_loss(*a, scale, *g)
    return (mu, lv, pmu, plv, motion, g_kld, g_div), r64, r32


@pytest.mark.parametrize('scale', [2.0, 0.5])                       # the default and samplerloss.get_diversity_config('sdd')
@pytest.mark.parametrize('prior', [False, True])
@pytest.mark.parametrize('case', SAMPLER_CASES)
def test_sampler_loss_forward_and_backward_vs_float64(case, prior, scale):
    from sttode_amd import samplerloss
    assert scale in (samplerloss.get_diversity_config(None)['scale'], samplerloss.get_diversity_config('sdd')['scale'])
    capi, dev = _capi(), _gpu()
    st = capi.stream_ptr()
    n, K, nz, D = case
    arrs, r64, r32 = _sampler_inputs(case, prior, scale)
    mu, lv, pmu, plv, motion, g_kld, g_div = (_dev(dev, v) for v in arrs)
    o = dict(kld=_Out(dev, (n,)), div=_Out(dev, (n,)), dmu=_Out(dev, (n * K, nz)), dlogvar=_Out(dev, (n * K, nz)), dmotion=_Out(dev, (n, K, D)))
    capi.call('sttode_sampler_loss', mu, lv, pmu, plv, motion, n, K, nz, D, scale, o['kld'].v, o['div'].v, st)
    capi.call('sttode_sampler_loss_bwd', mu, lv, pmu, plv, motion, g_kld, g_div, n, K, nz, D, scale, o['dmu'].v, o['dlogvar'].v, o['dmotion'].v, st)
    torch.cuda.synchronize()
    what = f'sampler_loss n={n} K={K} nz={nz} D={D} prior={prior} scale={scale}'
    worst = {}
    for k, v in o.items():
        worst[k] = _close(v.v, r64[k], r32[k], f'{what} {k}')
        assert v.margins_ok(), f'{what}: wrote outside {k}'
    k = max(worst, key=worst.get)
    _worst(f'sampler family {what} (at {k})', worst[k])


def test_sampler_loss_refusals_write_nothing():
    """K = 1, K D = 4097 (one float more than the LDS holds) and scale 0: forward and backward refuse, every output keeps its sentinel."""
    capi, dev = _capi(), _gpu()
    st = capi.stream_ptr()
    for n, K, nz, D, scale in ((2, 1, 4, 8, 2.0), (2, 17, 4, 241, 2.0), (2, 3, 4, 8, 0.0)):
        z = lambda *s: torch.zeros(*s, device=dev)
        mu, lv, motion, g = z(n * K, nz), z(n * K, nz), z(n, K, D), z(n)
        o = dict(kld=_Out(dev, (n,), SENT), div=_Out(dev, (n,), SENT), dmu=_Out(dev, (n * K, nz), SENT), dlogvar=_Out(dev, (n * K, nz), SENT),
                 dmotion=_Out(dev, (n, K, D), SENT))
        with pytest.raises(capi.SttodeError):
            capi.call('sttode_sampler_loss', mu, lv, None, None, motion, n, K, nz, D, scale, o['kld'].v, o['div'].v, st)
        with pytest.raises(capi.SttodeError):
            capi.call('sttode_sampler_loss_bwd', mu, lv, None, None, motion, g, g, n, K, nz, D, scale, o['dmu'].v, o['dlogvar'].v, o['dmotion'].v, st)
        torch.cuda.synchronize()
        for k, v in o.items():
            assert v.untouched(), f'sampler_loss K={K} D={D} scale={scale}: refused, but wrote {k}'
