"""CPU tests of the large-set scores (sttode_large_select / _kde_nll / _spread, csrc/large_set.hip): the yardsticks of
tests/large_set_ref.py against loop-form restatements, scipy and the stored fixture; the C ABI's exports and refusals; the Python layers'
refusals; and the evaluation loop's call sequence with and without the raw pass.

The inputs of a case regenerate from the seed tests/golden/make_large_set_golden.py found (the fixture stores the seed, a checksum and
the expected outputs); the near-tie conditions the maker asserts are asserted again here on the regenerated inputs."""
import ctypes
import inspect
import types

import numpy as np
import pytest

import large_set_ref as ref

SMALL = ('m3_t1', 'm64_t12', 'm65_far', 'm65_nan', 'm65_degen', 'm400_r20_dup')   # what the loop-form restatements walk in a second or two
_INPUTS = {}


def case(golden, tag):
    """(case dict, fixture, pred5, flat x, gt, dup info) of a stored case, regenerated once per process and checked against its checksum."""
    g = golden('large_set')
    if tag not in _INPUTS:
        pred5, gt, info = ref.case_inputs(tag, int(g[tag + '/seed']))
        assert ref.checksum(pred5, gt) == float(g[tag + '/checksum']), f'{tag}: the regenerated inputs are not the ones the fixture was made of'
        x = ref.flat(pred5)
        for v in (pred5, x, gt):
            v.setflags(write=False)
        _INPUTS[tag] = (pred5, x, gt, info)
    return (ref.CASES[tag], g) + _INPUTS[tag]


# ----- the yardsticks ------------------------------------------------------------------------------------------------------------------

def test_fixture_lists_the_cases(golden):
    g = golden('large_set')
    assert sorted(map(str, g['cases'])) == sorted(ref.CASES)
    ms = {c['R'] * c['K_in'] for c in ref.CASES.values()}
    assert {3, 64, 65, 256, 257, 400, 2000, 4096} <= ms
    for tag, c in ref.CASES.items():
        M = c['R'] * c['K_in']
        assert list(g[tag + '/ks']) == ref.case_ks(c) and {1, c['K_in'], M} <= set(ref.case_ks(c))
        assert ((tag + '/kde' in g) == ('k' in c['parts'])) and ((tag + '/apd' in g) == ('p' in c['parts']))


@pytest.mark.parametrize('tag', [t for t in SMALL if 's' in ref.CASES[t]['parts']])
def test_selection_loop_form_against_the_fixture(golden, tag):
    """Per agent and sample a scalar walk over the frames; minima by an explicit scan with the entry's rule (< only, from +inf / index 0);
    a segment's values added agent by agent.  Against the stored array-form values: indices equal, values to 1e-12 relative."""
    c, g, pred5, x, gt, info = case(golden, tag)
    X, Y, sc = x.astype(np.float64), gt.astype(np.float64), float(np.float32(c['scale']))     # bok_dist's formula: |(x - g) scale|
    n, M, Tf = X.shape[:3]
    va, vf = np.zeros((n, M)), np.zeros((n, M))
    for a in range(n):
        for m in range(M):
            s = d = 0.0
            for t in range(Tf):
                d = float(np.hypot((X[a, m, t, 0] - Y[a, t, 0]) * sc, (X[a, m, t, 1] - Y[a, t, 1]) * sc))
                s += d
            va[a, m], vf[a, m] = s / Tf, d

    def scan(v):
        best, idx = np.inf, 0
        for m, y in enumerate(v):
            if y < best:
                best, idx = y, m
        return best, idx
    ks = list(g[tag + '/ks'])
    for name, v in (('ade', va), ('fde', vf)):
        for a in range(n):
            best, idx = scan(v[a])
            assert idx == g[f'{tag}/{name}_idx'][a], (tag, name, a)
            want = g[f'{tag}/{name}'][a]
            assert best == want == np.inf or abs(best - want) <= 1e-12 * abs(want), (tag, name, a)
            for i, k in enumerate(ks):
                bk, wk = scan(v[a, :k])[0], g[f'{tag}/{name}_at'][a, i]
                assert bk == wk == np.inf or abs(bk - wk) <= 1e-12 * abs(wk), (tag, name, a, k)
        sp = g[tag + '/seg_ptr']
        for s in range(len(sp) - 1):
            want, widx = g[f'{tag}/seg_j{name}'][s], g[f'{tag}/seg_j{name}_idx'][s]
            if sp[s + 1] == sp[s]:
                assert np.isnan(want) and widx == -1
                continue
            tot = [0.0] * M
            for a in range(sp[s], sp[s + 1]):
                for m in range(M):
                    tot[m] += v[a, m]
            best, idx = scan(np.array(tot) / float(sp[s + 1] - sp[s]))
            assert idx == widx and (best == want == np.inf or abs(best - want) <= 1e-12 * abs(want)), (tag, name, s)
    assert (g[tag + '/miss'] == (g[tag + '/fde'] > c['thr'])).all()
    for a, b, to in info:                                                  # the copies tie exactly: the lower index is the stored one
        assert (x[a, b] == x[a, to]).all() and b // c['K_in'] != to // c['K_in']
        assert g[tag + ('/fde_idx' if a == 1 else '/ade_idx')][a] == min(b, to)
    if c['edit'] == 'nan':
        assert g[tag + '/ade'][ref.NAN_ALL] == np.inf and g[tag + '/ade_idx'][ref.NAN_ALL] == 0
        assert g[tag + '/ade_at'][1, 0] == np.inf and g[tag + '/ade_at'][2, 0] == np.inf            # a prefix with no finite sample


@pytest.mark.parametrize('tag', [t for t, c in ref.CASES.items() if 's' in c['parts']])
def test_stored_selections_hold_their_gaps(golden, tag):
    """The maker's near-tie conditions on the regenerated inputs: best and runner-up differ by 16 Tf 2^-23 relative, for every agent, prefix
    and segment, apart from the exact copies."""
    c, g, pred5, x, gt, info = case(golden, tag)
    need = ref.GAP * c['Tf'] * ref.EPS32
    copies = {}
    for a, b, to in info:
        copies.setdefault(a, []).extend([b, to])
    sp = g[tag + '/seg_ptr']
    for v in ref.select_f64(x, gt, c['scale']):
        for a in range(v.shape[0]):
            for k in list(g[tag + '/ks']) + [v.shape[1]]:
                assert k == 1 or ref.runner_up_gap(v[a, :k], [e for e in copies.get(a, []) if e < k]) >= need, (tag, a, k)
        for s in range(len(sp) - 1):
            if sp[s + 1] > sp[s]:
                one = copies.get(int(sp[s]), []) if sp[s + 1] - sp[s] == 1 else []
                assert ref.runner_up_gap(v[sp[s]:sp[s + 1]].sum(axis=0), one) >= need, (tag, s)


@pytest.mark.parametrize('tag', [t for t in SMALL if 'k' in ref.CASES[t]['parts']])
def test_kde_restatement_against_the_fixture_and_scipy(golden, tag):
    """kde_np (4l's formulas, frame by frame) against the stored scipy values and against gaussian_kde itself; the samples in reversed order
    change nothing above 1e-10; gaussian_kde raises exactly on the frames built degenerate."""
    pytest.importorskip('scipy.stats')
    c, g, pred5, x, gt, info = case(golden, tag)
    want = g[tag + '/kde']
    fwd, rev = ref.kde_np(x, gt, c['scale']), ref.kde_np(x, gt, c['scale'], reverse=True)
    sc, raised = ref.kde_scipy(x, gt, c['scale'])
    ok = ~np.isnan(want)
    assert (np.isnan(fwd) == ~ok).all() and (np.isnan(sc) == ~ok).all()
    np.testing.assert_allclose(fwd[ok], want[ok], rtol=0, atol=1e-8)
    np.testing.assert_allclose(sc[ok], want[ok], rtol=0, atol=1e-12)
    np.testing.assert_allclose(fwd[ok], rev[ok], rtol=0, atol=1e-10)
    built = sorted((a, t) for a, ts in ref.DEGEN_FRAMES.items() for t in ts) if c['edit'] == 'degen' else []
    assert sorted(raised) == built
    if c['edit'] == 'degen':
        assert list(np.nonzero(~ok)[0]) == sorted(ref.DEGEN_FRAMES)
    if c['edit'] == 'far':
        assert (want[::2] == 20.0).all() and (want[1::2] < 20.0).all()                                  # every frame clipped at -20


@pytest.mark.parametrize('tag', [t for t in SMALL if 'p' in ref.CASES[t]['parts']])
def test_spread_loop_form_against_the_fixture(golden, tag):
    """The pair statistics pair by pair (F.pdist order), frames in a scalar loop, against the stored array-form values."""
    c, g, pred5, x, gt, info = case(golden, tag)
    X, Y = ref.coords(x, c['scale']), ref.coords(gt, c['scale'])
    n, M, Tf = X.shape[:3]
    for a in range(min(n, 3)):
        tot = np.zeros(4)
        for i in range(M):
            d = np.sqrt(((X[a, i] - X[a, i + 1:]) ** 2).sum(axis=-1))       # [M - i - 1, Tf]
            s2 = np.zeros(len(d))
            s1 = np.zeros(len(d))
            for t in range(Tf):
                s2 += d[:, t] ** 2
                s1 += d[:, t]
            tot += [np.sqrt(s2).sum(), d[:, -1].sum() if len(d) else 0.0, (s1 / Tf).sum(), np.exp(-s2 / c['div']).sum()]
        tot /= M * (M - 1) / 2.0
        G = np.sqrt(((X[a] - Y[a]) ** 2).sum(axis=-1))
        cc = (M - 1) / (2.0 * M)
        for name, v in zip(('apd', 'fpd', 'pade', 'dlow'), tot):
            assert abs(v - g[f'{tag}/{name}'][a]) <= 1e-12 * abs(v), (tag, name, a)
        assert abs(G.mean(axis=-1).mean() - cc * tot[2] - g[tag + '/es_ade'][a]) <= 1e-12 * g[tag + '/es_ade_mag'][a]
        assert abs(G[:, -1].mean() - cc * tot[1] - g[tag + '/es_fde'][a]) <= 1e-12 * g[tag + '/es_fde_mag'][a]


@pytest.mark.parametrize('tag', ['m3_t1', 'm64_t12', 'm65_far'])
def test_energy_scores_are_the_double_sum(golden, tag):
    """es = (1/M) sum D(x_m, y) - ((M-1) / (2M)) (pair mean) is E|X - y| - E|X - X'| / 2 with the explicit 1 / M^2 sum over all ordered pairs."""
    c, g, pred5, x, gt, info = case(golden, tag)
    ea, ef = ref.energy_double_sum(x, gt, c['scale'])
    np.testing.assert_allclose(ea, g[tag + '/es_ade'], rtol=0, atol=1e-12 * g[tag + '/es_ade_mag'].max())
    np.testing.assert_allclose(ef, g[tag + '/es_fde'], rtol=0, atol=1e-12 * g[tag + '/es_fde_mag'].max())


def test_round_major_layout_is_a_permutation():
    pred5 = np.arange(3 * 2 * 4 * 5 * 2, dtype=np.float32).reshape(3, 2, 4, 5, 2)
    x = ref.flat(pred5)
    assert x.shape == (2, 12, 5, 2) and all((x[a, r * 4 + k] == pred5[r, a, k]).all() for a in range(2) for r in range(3) for k in range(4))


# ----- the C ABI -----------------------------------------------------------------------------------------------------------------------

ENTRIES = {'sttode_large_select': 26, 'sttode_large_kde_nll': 9, 'sttode_large_spread': 17, 'sttode_large_select_ws': 2,
           'sttode_large_spread_ws': 2}


def test_entry_points_exported_declared_and_abi_version():
    from sttode_amd import capi
    from test_capi_symbols import header_functions
    fns = header_functions()
    L = capi.lib()
    assert capi.ABI_VERSION == 15 and L.sttode_abi_version() == 15
    for name, arity in ENTRIES.items():
        assert name in fns and name in capi.SIGNATURES and hasattr(L, name), name
        assert len(fns[name]) == len(capi.SIGNATURES[name]) == arity, name
    assert capi.RESTYPES['sttode_large_select_ws'] is capi.RESTYPES['sttode_large_spread_ws'] is ctypes.c_longlong
    assert L.sttode_large_select_ws(7, 80) == 2 * 7 * 80 * 4
    assert L.sttode_large_spread_ws(7, 64) == 7 * 1 * 4 * 8 and L.sttode_large_spread_ws(7, 65) == 7 * 3 * 4 * 8
    assert L.sttode_large_spread_ws(2, 4096) == 2 * 64 * 4 * 8                        # never more than 64 workgroups per agent
    for bad in ((0, 80), (7, 0), (7, 4097)):
        assert L.sttode_large_select_ws(*bad) == -1 and b'sttode_large_select_ws' in L.sttode_last_error()
    for bad in ((0, 80), (7, 1), (7, 4097), (1 << 26, 4096)):
        assert L.sttode_large_spread_ws(*bad) == -1 and b'sttode_large_spread_ws' in L.sttode_last_error()


def test_argument_checks_before_launch():
    """Every limit is refused with a message naming the entry point (host logic only: no device pointer is dereferenced, nothing launches)."""
    from sttode_amd import capi
    L = capi.lib()
    p = ctypes.c_void_p(0x1000)          # never dereferenced: every call below fails its checks first
    ks = (ctypes.c_int * 3)(1, 20, 60)
    big = 1 << 40

    def refused(entry, order, good, match, **kw):
        a = {**good, **kw}
        rc = getattr(L, entry)(*[a[k] for k in order], None)
        assert rc != 0, (entry, kw)
        msg = L.sttode_last_error().decode()
        assert entry in msg and match in msg, (entry, kw, msg)

    sel = ('pred', 'gt', 'n', 'R', 'K_in', 'Tf', 'scale', 'thr', 'ks', 'nk', 'seg_ptr', 'S', 'ws', 'ws_bytes', 'ade', 'fde', 'ia', 'ifd', 'miss',
           'ade_at', 'fde_at', 'jade', 'jfde', 'jai', 'jfi')
    good = dict(pred=p, gt=p, n=5, R=3, K_in=20, Tf=12, scale=1.0, thr=1.0, ks=ctypes.cast(ks, ctypes.c_void_p), nk=3, seg_ptr=p, S=2, ws=p,
                ws_bytes=big, ade=p, fde=p, ia=p, ifd=p, miss=p, ade_at=p, fde_at=p, jade=p, jfde=p, jai=p, jfi=p)
    R = lambda match, **kw: refused('sttode_large_select', sel, good, match, **kw)   # noqa: E731
    for name in ('pred', 'gt', 'ade', 'fde'):
        R('null', **{name: None})
    R('n must be', n=0)
    R('n must be', n=-2)
    R('M = R K_in', R=0)
    R('M = R K_in', K_in=0)
    R('M = R K_in', R=205)                              # M = 4100
    R('M = R K_in', R=1 << 20, K_in=1 << 20)            # the product does not wrap
    R('Tf must be', Tf=0)
    R('Tf must be', Tf=201)
    R('nk must be', nk=-1)
    R('nk must be', nk=17)
    R('null', ks=None)
    R('null', ade_at=None)
    R('need ks', nk=0)                                  # ade_at / fde_at without ks
    for vals in ((0, 20, 60), (1, 20, 61), (1, 20, 20), (20, 1, 60)):
        R('strictly ascending', ks=ctypes.cast((ctypes.c_int * 3)(*vals), ctypes.c_void_p))
    R('null', jade=None)
    R('null', seg_ptr=None)                             # joint outputs without a CSR
    R('S must be', S=0)
    R('workspace', ws=None)
    R('workspace', ws_bytes=2 * 5 * 60 * 4 - 1)

    kde = ('pred', 'gt', 'n', 'R', 'K_in', 'Tf', 'scale', 'nll')
    goodk = dict(pred=p, gt=p, n=5, R=3, K_in=20, Tf=12, scale=1.0, nll=p)
    K = lambda match, **kw: refused('sttode_large_kde_nll', kde, goodk, match, **kw)   # noqa: E731
    for name in ('pred', 'gt', 'nll'):
        K('null', **{name: None})
    K('n must be', n=0)
    K('M = R K_in', R=205)
    K('M = R K_in', R=0)
    K('>= 3', R=1, K_in=2)
    K('>= 3', R=2, K_in=1)
    K('Tf must be', Tf=201)
    K('Tf must be', Tf=0)

    spr = ('pred', 'gt', 'n', 'R', 'K_in', 'Tf', 'scale', 'div', 'ws', 'ws_bytes', 'apd', 'fpd', 'pade', 'dlow', 'es_ade', 'es_fde')
    goods = dict(pred=p, gt=p, n=5, R=3, K_in=20, Tf=12, scale=1.0, div=1.0, ws=p, ws_bytes=big, apd=p, fpd=p, pade=p, dlow=p, es_ade=p, es_fde=p)
    S = lambda match, **kw: refused('sttode_large_spread', spr, goods, match, **kw)   # noqa: E731
    for name in ('pred', 'apd', 'fpd', 'pade', 'dlow'):
        S('null', **{name: None})
    S('need gt', gt=None)
    S('n must be', n=0)
    S('M = R K_in', K_in=2000)
    S('>= 2', R=1, K_in=1)
    S('Tf must be', Tf=201)
    S('div_scale', div=0.0)
    S('div_scale', div=float('inf'))
    S('div_scale', div=float('nan'))
    S('workspace', ws=None)
    S('workspace', ws_bytes=5 * 1 * 4 * 8 - 1)
    S('too large', n=1 << 26, R=64, K_in=64)


# ----- the Python layers ---------------------------------------------------------------------------------------------------------------

def test_python_layers_refuse_bad_input():
    import torch
    from helpers import make_args
    from sttode_amd import STTODENet, capi, metrics
    from sttode_amd.evaluate import eval_scenes_reduced_raw
    x, y = torch.zeros(3, 80, 12, 2), torch.zeros(3, 12, 2)
    for f in (lambda: metrics.large_select(x, y), lambda: metrics.large_kde_nll(x, y), lambda: metrics.large_spread(x),
              lambda: metrics.large_select(x.numpy(), y), lambda: metrics.large_spread(torch.zeros(4, 3, 20, 12, 2), y)):
        with pytest.raises(capi.SttodeError, match='HIP'):
            f()                                                                        # CPU tensors: no fallback
    m = STTODENet(make_args(), 'cpu')
    m.set_data(None, torch.zeros(3, 2, 8), torch.zeros(3, 2, 12))
    with pytest.raises(capi.SttodeError):
        m.score_samples(x)
    with pytest.raises(capi.SttodeError):
        m.inference_reduced_samples(3)
    with pytest.raises(ValueError, match='rounds'):
        eval_scenes_reduced_raw(m, [], 0)
    with pytest.raises(ValueError, match='4096'):
        eval_scenes_reduced_raw(m, [], 4096 // m.args.sample_k + 1)

    class OnDevice(torch.Tensor):                                                      # shapes and dtypes are refused before any device work
        is_cuda = True

    def dev(*shape, dtype=torch.float32):
        return torch.zeros(*shape, dtype=dtype).as_subclass(OnDevice)
    for f, match in ((lambda: metrics.large_select(dev(3, 80, 12), y), 'pred must be'),
                     (lambda: metrics.large_select(dev(3, 80, 12, 3), y), 'pred must be'),
                     (lambda: metrics.large_select(dev(3, 0, 12, 2), y), 'pred must be'),
                     (lambda: metrics.large_select(dev(3, 80, 12, 2, dtype=torch.float64), y), 'float32'),
                     (lambda: metrics.large_select(dev(3, 4097, 1, 2), y), 'M <= 4096'),
                     (lambda: metrics.large_select(dev(5, 3, 1000, 1, 2), y), 'M <= 4096'),
                     (lambda: metrics.large_kde_nll(dev(3, 2, 12, 2), y), '3 <= M'),
                     (lambda: metrics.large_spread(dev(3, 1, 12, 2)), '2 <= M'),
                     (lambda: metrics.large_select(dev(3, 80, 201, 2), y), 'Tf <= 200')):
        with pytest.raises(ValueError, match=match):
            f()


def test_result_classes_back_their_fields_with_one_allocation_per_dtype():
    import torch
    from sttode_amd import metrics
    ls = metrics.LargeSelection(5, 80, (1, 20, 80), 3, torch.device('cpu'))
    assert ls.ade_at.shape == ls.fde_at.shape == (5, 3) and ls.seg_jade.shape == ls.seg_jfde_idx.shape == (3,) and ls.miss.dtype == torch.bool
    f = [t for t in ls.args() if t is not None and t.dtype == torch.float32]
    i = [t for t in ls.args() if t is not None and t.dtype == torch.int32]
    assert len(f) == 6 and len(i) == 4
    assert len({t.untyped_storage().data_ptr() for t in f}) == 1 and len({t.untyped_storage().data_ptr() for t in i}) == 1
    assert len({t.data_ptr() for t in f}) == 6 and len({t.data_ptr() for t in i}) == 4
    assert ls.at(20)[0].data_ptr() == ls.ade_at[:, 1].data_ptr()
    with pytest.raises(ValueError):
        ls.at(5)
    none = metrics.LargeSelection(5, 80, (), 0, torch.device('cpu'))
    assert none.ade_at is None and none.seg_jade is None and none.seg_jfde_idx is None and len(none.args()) == 11
    sp = metrics.LargeSpread(5, 80, torch.device('cpu'), 2.0, True)
    assert len({t.untyped_storage().data_ptr() for t in sp.args()}) == 1 and len({t.data_ptr() for t in sp.args()}) == 6
    assert metrics.LargeSpread(5, 80, torch.device('cpu'), 2.0, False).es_ade is None
    assert all(hasattr(c, '__slots__') and hasattr(c, 'record_stream') for c in (metrics.LargeSelection, metrics.LargeSpread))


def test_signatures():
    """The loops that existed keep their signatures; the raw loop takes eval_scenes_reduced's parameters, defaults included, and
    inference_reduced_samples takes inference_reduced's."""
    from sttode_amd import STTODENet, metrics
    from sttode_amd import evaluate as ev

    def params(f):
        return [(p.name, p.default) for p in inspect.signature(f).parameters.values()]
    E = inspect.Parameter.empty
    assert params(ev.eval_scenes_reduced)[-1] == ('kde', False) and params(ev.eval_scenes_reduced_raw) == params(ev.eval_scenes_reduced)
    assert params(STTODENet.inference_reduced_samples) == params(STTODENet.inference_reduced)
    assert params(STTODENet.score_samples) == [('self', E), ('pred', E), ('gt', None), ('scale', 1.0), ('miss_threshold', 1.0), ('ks', ()),
                                               ('seg_ptr', None), ('kde', False), ('spread', False), ('div_scale', 1.0)]
    assert params(metrics.large_select) == [('pred', E), ('gt', E), ('scale', 1.0), ('miss_threshold', 1.0), ('ks', ()), ('seg_ptr', None)]
    assert params(metrics.large_kde_nll) == [('pred', E), ('gt', E), ('scale', 1.0)]
    assert params(metrics.large_spread) == [('pred', E), ('gt', None), ('scale', 1.0), ('div_scale', 1.0)]
    import dataclasses
    names = [f.name for f in dataclasses.fields(ev.EvalReport)]
    raw = ['raw_m', 'raw_ade', 'raw_fde', 'raw_miss_rate', 'raw_ade_at_k', 'raw_fde_at_k', 'raw_joint_ade', 'raw_joint_fde', 'raw_kde_nll',
           'raw_kde_invalid', 'raw_apd', 'raw_fpd', 'raw_pade', 'raw_dlow', 'raw_energy_ade', 'raw_energy_fde']
    at = names.index('raw_m')                       # (in front of the spread block, which tests/test_sample_spread.py keeps trailing)
    assert names[at:at + len(raw)] == raw and names[at - 1] == 'weighted_agents' and names[at + len(raw)] == 'apd'
    assert all(f.default is None for f in dataclasses.fields(ev.EvalReport) if f.name in raw)


class _Recorder:
    """A stand-in for STTODENet on the CPU that records what the evaluation loop calls, in order."""

    def __init__(self):
        import torch
        self.calls, self.device, self.async_depth = [], torch.device('cpu'), 4
        self.args = types.SimpleNamespace(sample_k=4, zdim=2, future_length=3, dataset='eth')

    def set_scene_batch(self, past, future, scene_ptr):
        import torch
        self.calls.append(('set_scene_batch', len(scene_ptr) - 1))
        self._scene_ptr, self.n = torch.as_tensor(np.asarray(scene_ptr), dtype=torch.int32), past.shape[0]

    def _round_buffer(self, rounds, n):
        import torch
        return torch.zeros(rounds, n, 4, 3, 2)

    def inference(self, data, z=None):
        import torch
        self.calls.append(('inference', tuple(z.shape)))
        return torch.zeros(4, self.n, 3, 2)

    def select_best_of_k(self, pred, **kw):
        import torch
        from sttode_amd import metrics
        self.calls.append(('select_best_of_k', tuple(pred.shape), sorted(kw)))
        sel = metrics.Selection(self.n, int(self._scene_ptr.numel()) - 1, 3, torch.device('cpu'), False)
        for t in sel.args():
            if t is not None:
                t.zero_()
        return sel

    def select_joint(self, pred, **kw):
        import torch
        from sttode_amd import metrics
        self.calls.append(('select_joint', tuple(pred.shape)))
        js = metrics.JointSelection(int(self._scene_ptr.numel()) - 1, torch.device('cpu'), None)
        for t in (js.seg_jade, js.seg_jade_idx):
            t.zero_()
        js.seg_jfde.zero_(), js.seg_jfde_idx.zero_()
        return js

    def kde_nll(self, pred, **kw):
        import torch
        self.calls.append(('kde_nll', tuple(pred.shape)))
        return torch.zeros(self.n, dtype=torch.float64)

    def score_samples(self, pred, **kw):
        import torch
        from sttode_amd import metrics
        self.calls.append(('score_samples', tuple(pred.shape), {k: (v if not isinstance(v, torch.Tensor) else 'tensor') for k, v in kw.items()}))
        S = int(self._scene_ptr.numel()) - 1 if kw['seg_ptr'] is not False else 0
        ls = metrics.LargeSelection(self.n, pred.shape[0] * pred.shape[2], kw['ks'], S, torch.device('cpu'))
        for i, t in enumerate(ls.args()):
            if t is not None:
                t.fill_(i)
        return metrics.SampleScores(ls, torch.full((self.n,), 2.5, dtype=torch.float64) if kw['kde'] else None)


def test_default_loop_makes_the_calls_it_made_and_the_raw_loop_one_more(monkeypatch):
    """eval_scenes_reduced on a recording stand-in: per batch set_scene_batch, `rounds` inference calls, the reduction, the selection -- and
    nothing else; eval_scenes_reduced_raw: the same with score_samples on the round buffer in front of the reduction.  Every field that
    existed is equal between the two reports."""
    import dataclasses
    import torch
    from sttode_amd import evaluate as ev
    from sttode_amd import metrics
    log = []

    def reduce_samples(buf, K, **kw):
        log.append(('reduce_samples', tuple(buf.shape), K))
        return types.SimpleNamespace(centroids=torch.zeros(buf.shape[1], K, 3, 2))
    monkeypatch.setattr(metrics, 'reduce_samples', reduce_samples)

    class DS:
        sizes = ((2, 1), (3,))

        def __len__(self):
            return 3

        def scene_batch(self, ids):
            sz = self.sizes[0] if ids[0] == 0 else self.sizes[1]
            n = sum(sz)
            return types.SimpleNamespace(past=np.zeros((n, 8, 2), np.float32), future=np.zeros((n, 3, 2), np.float32),
                                         scene_ptr=ref.seg_ptr_of(sz), n_agents=n)

    def run(fn, **kw):
        m = _Recorder()
        m.calls = log
        del log[:]
        rep = fn(m, DS(), 5, scenes_per_call=2, z_fn=lambda rows: torch.zeros(rows, 2), pipelined=False, **kw)
        return rep, list(log)
    rep0, calls0 = run(ev.eval_scenes_reduced)
    per = lambda n, S: [('set_scene_batch', S)] + [('inference', (n * 4, 2))] * 5 + [   # noqa: E731
        ('reduce_samples', (5, n, 4, 3, 2), 4), ('select_best_of_k', (n, 4, 3, 2), ['miss_threshold', 'scale', 'seg_ptr'])]
    assert calls0 == per(3, 2) + per(3, 1)
    rep1, calls1 = run(ev.eval_scenes_reduced_raw, ks=(1, 5, 30), kde=False)
    assert [c for c in calls1 if c[0] != 'score_samples'] == calls0
    raw = [(i, c) for i, c in enumerate(calls1) if c[0] == 'score_samples']
    assert len(raw) == 2 and all(calls1[i + 1][0] == 'reduce_samples' for i, _ in raw)
    assert raw[0][1][1] == (5, 3, 4, 3, 2)
    assert raw[0][1][2] == dict(scale=1.0, miss_threshold=1.0, ks=[1, 4, 5], seg_ptr=False, kde=False, spread=False, div_scale=1.0)
    for f in dataclasses.fields(rep0):
        u, v = getattr(rep0, f.name), getattr(rep1, f.name)
        if f.name.startswith('raw_'):
            assert u is None
        elif isinstance(u, np.ndarray):
            assert u.tobytes() == v.tobytes(), f.name
        else:
            assert u == v, f.name
    assert rep1.raw_m == 20 and rep1.raw_ade == 0.0 and rep1.raw_fde == 1.0 and rep1.raw_ade_at_k == {1: 5.0, 4: 5.0, 5: 5.0}
    assert rep1.raw_miss_rate == 1.0 and rep1.raw_joint_ade is None and rep1.raw_kde_nll is None and rep1.raw_apd is None
    rep2, calls2 = run(ev.eval_scenes_reduced_raw, joint=True, kde=True, traj_scale=1.5, miss_threshold=0.3)
    kw = [c for c in calls2 if c[0] == 'score_samples'][0][2]
    assert kw['seg_ptr'] == 'tensor' and kw['kde'] is True and kw['scale'] == 1.5 and kw['miss_threshold'] == 0.3 and kw['ks'] == [1, 4, 5, 10]
    assert rep2.raw_joint_ade == 7.0 and rep2.raw_joint_fde == 8.0 and rep2.raw_kde_nll == 2.5 and rep2.raw_kde_invalid == 0
