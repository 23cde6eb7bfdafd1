"""GPU tests of the kernels every displacement number comes from -- best_of_k_kernel, bok_select_kernel, bok_segments_kernel and
horizon_metrics_kernel (csrc/frontend.hip) -- called through capi.call at the shapes where their code paths change
(tests/metric_root_cases.py) and held, agent by agent, to the same operation in float64 on the very float32 inputs they received
(tests/metric_root_ref.py).  The bounds are derived there from the operation count, not measured: (Tf + 8) 2^-24 relative for a mean
displacement, 6 2^-24 for a final one, (h + 8) 2^-24 for horizon h, (ceil(na / 64) + 8) 2^-24 for a segment mean of na agents against the
float64 mean of the device's own per-agent values.  Indices and miss flags are the float64 ones exactly (the cases keep every agent's
runner-up and every miss threshold more than four bounds away); copies and the agreements between entry points are bitwise.

Every output sits inside a larger buffer: the interior starts as NaN (-7 / 99 for integers), so an element the kernel leaves out fails,
and the margins must keep their sentinels.

Non-finite samples (include/sttode_hip.h): a NaN sample is skipped; an agent whose samples are all NaN gets +inf from sttode_best_of_k,
and from sttode_best_of_k_select +inf at K < 64 and NaN at K = 64, index 0 and its sample 0 as `best`.

Measured on the MI355X, the worst error of each kernel over all of its cases, in units of 2^-24 relative to float64
(test_worst_error_per_kernel prints them; DESIGN.md 4k, profiles/metric_root/gputests.txt):
  best_of_k  ade 6.10 (bounds 9 .. 208)  fde 1.65 (6)         select   ade 6.10  fde 1.69 (with the 200-agent batch)
  horizon    mean 7.11 (9 .. 108)  frame 2.07 (6)             segments 2.18 against the device's per-agent values (9 .. 12), 2.13 all float64
"""
import functools

import numpy as np
import pytest
import torch

import metric_root_cases as C
import metric_root_ref as R
from helpers import horizon_metrics_np

pytestmark = pytest.mark.gpu

SENT, ISENT, BSENT = 12345.0, -99, 77
WORST = {}


def _dev():
    assert torch.cuda.is_available(), 'these tests need the GPU'
    return torch.device('cuda:0')


def _capi():
    from sttode_amd import capi
    return capi


class _Out:
    """An output of ``shape`` inside a larger buffer: margins of sentinels on both sides, the interior ``.v`` NaN (floats), -7 (int32) or
    99 (bytes)."""

    def __init__(self, shape, dtype=torch.float32, margin=8):
        self.n, self.m = int(np.prod(shape)), margin
        self.sent, fill = {torch.float32: (SENT, float('nan')), torch.int32: (ISENT, -7), torch.uint8: (BSENT, 99)}[dtype]
        self.buf = torch.full((self.n + 2 * margin,), self.sent, dtype=dtype, device=_dev())
        self.v = self.buf[margin:margin + self.n].view(shape)
        self.v.fill_(fill)
        self.before = self.buf.cpu().numpy().tobytes()

    def get(self):
        """The interior as NumPy, after checking that the margins kept their sentinel."""
        b = self.buf.cpu().numpy()
        assert (b[:self.m] == self.sent).all() and (b[self.m + self.n:] == self.sent).all(), 'a write outside the output'
        return b[self.m:self.m + self.n].reshape(tuple(self.v.shape)).copy()

    def untouched(self):
        return self.buf.cpu().numpy().tobytes() == self.before


def _t(a):
    return torch.from_numpy(np.array(a)).to(_dev())                # (a copy: the cases' arrays are read-only)


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def _within(kernel, got, ref, bound, what):
    """|got - ref| <= bound |ref| elementwise (exact zero where ref is zero); the worst figure is kept for the printout."""
    u = R.units(got, ref)
    WORST[kernel] = max(WORST.get(kernel, 0.0), float(np.max(u)))
    assert (u <= np.asarray(bound) / R.U).all(), (kernel, what, 'worst, in units of 2^-24:', float(np.max(u)), 'bound:', np.max(np.asarray(bound)) / R.U)


def _bok(pred, gt, scale):
    """sttode_best_of_k -> (ade [n], fde [n])."""
    capi = _capi()
    n, K, Tf = pred.shape[:3]
    ade, fde = _Out((n,)), _Out((n,))
    capi.call('sttode_best_of_k', _t(pred), _t(gt), n, K, Tf, float(scale), ade.v, fde.v, capi.stream_ptr())
    return ade.get(), fde.get()


SELECT_OUTS = ('ade', 'fde', 'best_ade_idx', 'best_fde_idx', 'miss', 'best', 'seg_ade', 'seg_fde', 'seg_miss')


def _select(pred, gt, scale, thr, seg_ptr=None, null=()):
    """sttode_best_of_k_select -> a dict of its outputs; those named in ``null`` are passed as NULL (None in the dict), and without seg_ptr
    the three segment outputs are."""
    capi = _capi()
    n, K, Tf = pred.shape[:3]
    S = 0 if seg_ptr is None else len(seg_ptr) - 1
    outs = {'ade': _Out((n,)), 'fde': _Out((n,)), 'best_ade_idx': _Out((n,), torch.int32), 'best_fde_idx': _Out((n,), torch.int32),
            'miss': _Out((n,), torch.uint8), 'best': _Out((n, Tf, 2))}
    if S:
        outs.update({'seg_ade': _Out((S,)), 'seg_fde': _Out((S,)), 'seg_miss': _Out((S,), torch.int32)})
    sp = None if seg_ptr is None else _t(np.asarray(seg_ptr, np.int32))
    args = [outs[k].v if k in outs and k not in null else None for k in SELECT_OUTS]
    capi.call('sttode_best_of_k_select', _t(pred), _t(gt), n, K, Tf, float(scale), float(thr), sp, S, *args, capi.stream_ptr())
    torch.cuda.synchronize()
    for k in null:
        assert outs[k].untouched(), k
    return {k: (outs[k].get() if k in outs and k not in null else None) for k in SELECT_OUTS}


def _plant(pred, gt):
    """A copy of pred whose last agent's last sample is the ground truth, bit for bit."""
    p = pred.copy()
    p[-1, -1] = gt[-1]
    return p


# -------------------------------------------------------------------------------------------------------------------------------------
# sttode_best_of_k
# -------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _bok_case(case):
    n, K, Tf = case
    pred, gt = C.inputs(*case)
    out = {}
    for scale in C.SCALES:
        ref = C.reference(*case, scale)
        ade, fde = _bok(pred, gt, scale)
        _within('best_of_k ade', ade, ref['ade'], R.bound_ade(Tf), (case, scale))
        _within('best_of_k fde', fde, ref['fde'], R.bound_fde, (case, scale))
        # a sample that equals the ground truth (the last sample of the last agent: the tail of the k loop): exact zeros, the rest unmoved
        zade, zfde = _bok(_plant(pred, gt), gt, scale)
        assert zade[-1] == 0 and zfde[-1] == 0, (case, scale, zade[-1], zfde[-1])
        assert _bits(zade[:-1]) == _bits(ade[:-1]) and _bits(zfde[:-1]) == _bits(fde[:-1]), (case, scale)
        out[scale] = (ade, fde)
    return out


@pytest.mark.parametrize('case', C.BOK_CASES, ids=C.case_id)
def test_best_of_k_every_agent_against_float64(case):
    _bok_case(case)


# -------------------------------------------------------------------------------------------------------------------------------------
# sttode_best_of_k_select, per agent
# -------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _select_case(case):
    n, K, Tf = case
    pred, gt = C.inputs(*case)
    rows = np.arange(n)
    for scale in C.SCALES:
        ref = C.reference(*case, scale)
        ade, fde = _bok_case(case)[scale]
        for thr in C.THRESHOLDS:
            r = _select(pred, gt, scale, thr)
            _within('select ade', r['ade'], ref['ade'], R.bound_ade(Tf), (case, scale))
            _within('select fde', r['fde'], ref['fde'], R.bound_fde, (case, scale))
            assert _bits(r['ade']) == _bits(ade) and _bits(r['fde']) == _bits(fde), (case, scale)        # the bits of sttode_best_of_k
            np.testing.assert_array_equal(r['best_ade_idx'], ref['ade_idx'], err_msg=str((case, scale)))
            np.testing.assert_array_equal(r['best_fde_idx'], ref['fde_idx'], err_msg=str((case, scale)))
            np.testing.assert_array_equal(r['miss'], ref['fde'] > thr, err_msg=str((case, scale, thr)))
            assert _bits(r['best']) == _bits(pred[rows, ref['ade_idx']]), (case, scale)                  # the gather, bit for bit
        # every optional output NULL in turn: it is not written, the others are what they were (r: the last threshold's)
        for k in ('best_ade_idx', 'best_fde_idx', 'miss', 'best'):
            q = _select(pred, gt, scale, C.THRESHOLDS[-1], null=(k,))
            assert all(q[f] is None or _bits(q[f]) == _bits(r[f]) for f in SELECT_OUTS), (case, scale, k)
        q = _select(pred, gt, scale, C.THRESHOLDS[-1], null=('best_ade_idx', 'best_fde_idx', 'miss', 'best'))
        assert _bits(q['ade']) == _bits(r['ade']) and _bits(q['fde']) == _bits(r['fde']), (case, scale)
        # a sample that equals the ground truth: exact zeros, and it is the one chosen
        z = _select(_plant(pred, gt), gt, scale, 1.0)
        assert z['ade'][-1] == 0 and z['fde'][-1] == 0 and z['best_ade_idx'][-1] == K - 1 and z['best_fde_idx'][-1] == K - 1 and z['miss'][-1] == 0
        assert _bits(z['best'][-1]) == _bits(gt[-1]) and _bits(z['ade'][:-1]) == _bits(ade[:-1]), (case, scale)
    return True


@pytest.mark.parametrize('case', C.SELECT_CASES, ids=C.case_id)
def test_select_every_agent_against_float64(case):
    _select_case(case)


# -------------------------------------------------------------------------------------------------------------------------------------
# bok_segments_kernel
# -------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _segments_case(name):
    n, K, Tf = C.SEG_CASE
    pred, gt = C.inputs(*C.SEG_CASE)
    sp = C.SEG_CSRS[name]
    sizes = [b - a for a, b in R.clamp_csr(sp, n)]
    empty = np.array([na == 0 for na in sizes])
    assert name != 'empty_and_clamped' or (empty.sum() == 2 and min(sp) < 0 and max(sp) > n)
    for scale in C.SCALES:
        ref = C.reference(*C.SEG_CASE, scale)
        for thr in C.THRESHOLDS:
            r = _select(pred, gt, scale, thr, seg_ptr=sp)
            _within('select ade', r['ade'], ref['ade'], R.bound_ade(Tf), (name, scale))
            _within('select fde', r['fde'], ref['fde'], R.bound_fde, (name, scale))
            own, full = R.segments64(r['ade'], r['fde'], sp, thr), R.segments64(ref['ade'], ref['fde'], sp, thr)
            np.testing.assert_array_equal(r['seg_miss'], full[2], err_msg=str((name, scale, thr)))
            assert (r['seg_miss'][empty] == 0).all()
            for j, f in enumerate(('seg_ade', 'seg_fde')):
                assert np.array_equal(np.isnan(r[f]), empty), (name, f, r[f])                  # an empty segment: NaN, nothing else is
                for s, na in enumerate(sizes):
                    if na:
                        _within('segments', r[f][s], own[j][s], R.bound_seg(na), (name, scale, f, s))
                        _within('segments, all float64', r[f][s], full[j][s], R.bound_seg(na) + (R.bound_ade(Tf), R.bound_fde)[j],
                                (name, scale, f, s))
        again = _select(pred, gt, scale, C.THRESHOLDS[-1], seg_ptr=sp)
        assert all(_bits(again[f]) == _bits(r[f]) for f in SELECT_OUTS), (name, scale)         # two runs: equal bits
        for k in ('seg_ade', 'seg_fde', 'seg_miss'):
            q = _select(pred, gt, scale, C.THRESHOLDS[-1], seg_ptr=sp, null=(k,))
            assert all(q[f] is None or _bits(q[f]) == _bits(r[f]) for f in SELECT_OUTS), (name, scale, k)
    return True


@pytest.mark.parametrize('name', list(C.SEG_CSRS))
def test_segments_against_float64(name):
    _segments_case(name)


# -------------------------------------------------------------------------------------------------------------------------------------
# sttode_horizon_metrics
# -------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _horizon_case(case):
    capi = _capi()
    n, K, Tf = case
    pred, gt = C.inputs(*case)
    for scale in C.SCALES:
        out = _Out((n, Tf, 2))
        capi.call('sttode_horizon_metrics', _t(pred), _t(gt), n, K, Tf, float(scale), out.v, capi.stream_ptr())
        hm, ref = out.get(), C.reference(*case, scale)['horizon']
        _within('horizon mean', hm[..., 0], ref[..., 0], R.bound_horizon(Tf)[None, :, 0], (case, scale))
        _within('horizon frame', hm[..., 1], ref[..., 1], R.bound_horizon(Tf)[None, :, 1], (case, scale))
        assert _bits(hm) == _bits(horizon_metrics_np(pred, gt, scale)), (case, scale)
    return True


@pytest.mark.parametrize('case', C.HORIZON_CASES, ids=C.case_id)
def test_horizon_metrics_every_agent_against_float64(case):
    _horizon_case(case)


@pytest.mark.parametrize('K,Tf', C.HORIZON_REFUSED, ids=lambda v: str(v))
def test_horizon_metrics_refuses_above_its_limits(K, Tf):
    """K = 65 and K Tf = 2079 (K <= 64): refused by name before anything is written."""
    capi = _capi()
    assert K > 64 or K * Tf > 2048
    pred, gt = C.draw(np.random.default_rng(K * Tf), 2, K, Tf, 4.0)
    out = _Out((2, Tf, 2))
    with pytest.raises(capi.SttodeError, match=r'sttode_horizon_metrics: need 0 < K <= 64 and K \* Tf <= 2048'):
        capi.call('sttode_horizon_metrics', _t(pred), _t(gt), 2, K, Tf, 1.0, out.v, capi.stream_ptr())
    torch.cuda.synchronize()
    assert out.untouched()


# -------------------------------------------------------------------------------------------------------------------------------------
# non-finite samples
# -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K,Tf', C.NONFINITE_SHAPES, ids=lambda v: str(v))
def test_nan_samples_are_skipped_and_an_all_nan_agent_is_as_the_header_says(K, Tf):
    pred, gt, half, nan_k, dead = C.nonfinite_inputs(K, Tf)
    clean, _ = C.inputs(5, K, Tf)
    others = [a for a in range(5) if a not in (half, dead)]
    for scale in C.SCALES:
        ref = R.best64(pred, gt, scale)                              # first_min: a NaN never wins; all NaN: +inf, index 0
        assert np.isinf(ref['ade'][dead]) and ref['ade_idx'][dead] == 0 and ref['ade_idx'][half] not in nan_k
        assert C.reference(5, K, Tf, scale)['ade_idx'][half] in nan_k                              # the minimum had to move to the rest
        ade, fde = _bok(pred, gt, scale)
        cade, cfde = _bok(clean, gt, scale)
        live = [a for a in range(5) if a != dead]
        _within('best_of_k ade', ade[live], ref['ade'][live], R.bound_ade(Tf), ('nan', K, scale))
        _within('best_of_k fde', fde[live], ref['fde'][live], R.bound_fde, ('nan', K, scale))
        assert ade[dead] == np.inf and fde[dead] == np.inf                                           # at any K
        assert _bits(ade[others]) == _bits(cade[others]) and _bits(fde[others]) == _bits(cfde[others])   # the neighbours are unaffected
        for thr in C.THRESHOLDS:
            r = _select(pred, gt, scale, thr)
            assert _bits(r['ade'][live]) == _bits(ade[live]) and _bits(r['fde'][live]) == _bits(fde[live])   # one finite sample: the bits
            np.testing.assert_array_equal(r['best_ade_idx'], ref['ade_idx'])                          # (the all-NaN agent: index 0)
            np.testing.assert_array_equal(r['best_fde_idx'], ref['fde_idx'])
            np.testing.assert_array_equal(r['miss'][live], ref['fde'][live] > thr)
            assert _bits(r['best']) == _bits(pred[np.arange(5), ref['ade_idx']])                      # (the all-NaN agent: its sample 0)
            if K < 64:                                               # idle lanes hold +inf, fminf skips the NaN: +inf, a miss
                assert r['ade'][dead] == np.inf and r['fde'][dead] == np.inf and r['miss'][dead] == 1
            else:                                                    # every lane holds a NaN: NaN, and NaN > thr is false
                assert np.isnan(r['ade'][dead]) and np.isnan(r['fde'][dead]) and r['miss'][dead] == 0


# -------------------------------------------------------------------------------------------------------------------------------------
def test_worst_error_per_kernel():
    """Runs whatever of the cases above has not run yet, then prints the worst error of every kernel in units of 2^-24 relative."""
    for c in C.BOK_CASES:
        _bok_case(c)
    for c in C.SELECT_CASES:
        _select_case(c)
    for name in C.SEG_CSRS:
        _segments_case(name)
    for c in C.HORIZON_CASES:
        _horizon_case(c)
    for k in sorted(WORST):
        print('[worst] %-24s %6.2f units of 2^-24' % (k, WORST[k]))
    assert set(WORST) == {'best_of_k ade', 'best_of_k fde', 'select ade', 'select fde', 'segments', 'segments, all float64',
                          'horizon mean', 'horizon frame'}
