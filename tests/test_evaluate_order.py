"""The evaluation loops of sttode_amd/evaluate.py as sequences of calls, on the CPU: a stub model, sampler and dataset / loader record every
call the loops make (method, agent count, z shape, scale, options, handle id) and return CPU tensors of the right shapes.  The order of the
z_fn calls, of set_* / launch / follow-up / wait, and the points of reset_async ARE the behaviour of these loops (the window of calls in
flight, the drain when too many batch shapes are cached), and no GPU test sees them.

tests/golden/evaluate_order.json and .npz hold what ``record()`` below returned for the evaluate.py of the commit BEFORE the loops were folded
into one scene driver and one NBA driver: per case the trace (options as indices into the case's table of distinct option sets), the rows
z_fn / eps_fn were asked for, and every returned value (the arrays' bytes in the .npz, in the order the JSON names them).  The tests ask for equality, exactly.  (eval_nba_report pipelined synchronises a CUDA stream: it stays with the GPU tests.)"""
import dataclasses
import json
import os
import types

import numpy as np
import pytest
import torch

K, ZD, TP, TF = 3, 2, 3, 2
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'evaluate_order')


def _vals(seed, *shape, dtype=torch.float32):
    """Deterministic values that differ from call to call (so a sum taken in another order, or over other calls, differs)."""
    numel = int(np.prod(shape)) if shape else 1
    return ((torch.arange(numel, dtype=torch.float64) * 0.37 + float(seed) * 1.13) % 5.0).reshape(shape).to(dtype)


def _ints(seed, *shape):
    return (_vals(seed, *shape, dtype=torch.float64) * 3).to(torch.int32)


def _sum(t):
    return round(float(torch.as_tensor(t).double().sum()), 4)


class _Scenes:
    def __init__(self, sizes):
        self.sizes = list(sizes)

    def __len__(self):
        return len(self.sizes)

    def scene_batch(self, indices):
        idx = list(indices)
        n = sum(self.sizes[i] for i in idx)
        return types.SimpleNamespace(n_agents=n, n_scenes=len(idx), past=_vals(idx[0], n, TP, 2), future=_vals(idx[0] + 0.5, n, TF, 2),
                                     scene_ptr=np.cumsum([0] + [self.sizes[i] for i in idx]).astype(np.int32))


def _loader(shapes):
    return [{'past_traj': _vals(i, B, N, TP, 2).numpy(), 'future_traj': _vals(i + 0.5, B, N, TF, 2).numpy()} for i, (B, N) in enumerate(shapes)]


class _Model:
    """Everything the loops ask of STTODENet.  ``log`` is the trace."""

    def __init__(self):
        self.log, self.opts = [], []
        self.args = types.SimpleNamespace(sample_k=K, zdim=ZD, future_length=TF, dataset='eth')
        self.device = torch.device('cpu')
        self.async_depth = 6
        self._async_bufs = {}
        self._calls = self._serial = 0

    # ---- what is recorded of an argument
    def _arg(self, v):
        if isinstance(v, (torch.Tensor, np.ndarray)):
            for tag in ('future', 'scene_ptr'):                  # the batch's own tensors are recorded by name
                if v is getattr(self, '_' + tag, None):
                    return tag
            return torch.as_tensor(v).tolist()
        return v

    def _opts(self, kw):
        o = sorted([k, self._arg(v)] for k, v in kw.items())
        if o not in self.opts:
            self.opts.append(o)
        return self.opts.index(o)

    @staticmethod
    def _shape(z):
        return None if z is None else list(z.shape)

    # ---- data
    def set_scene_batch(self, past, future, scene_ptr):
        self.n, self._S, self._scene_ptr, self._future, self._mode = past.shape[0], len(scene_ptr) - 1, scene_ptr, future, 'scenes'
        self.log.append(('set_scene_batch', self.n, self._S))

    def set_data_nba(self, data):
        past = torch.as_tensor(data['past_traj'])
        self.n, self._S, self._mode = int(np.prod(past.shape[:-2])), 0, 'nba'
        self._future = torch.as_tensor(data['future_traj']).reshape(self.n, TF, 2)
        self.log.append(('set_data_nba', list(past.shape)))

    def packed(self):
        self.log.append(('packed',))

    def next_async_stream(self, n):
        self.log.append(('next_async_stream', n))
        return None

    def _async_shapes(self, slots=0):
        return len(self._async_bufs) + sum((self.n, self._S, s) not in self._async_bufs for s in range(slots))

    def reset_async(self):
        self.log.append(('reset_async',))
        self._async_bufs = {}

    def _round_buffer(self, rounds, n):
        return torch.zeros(rounds, n, K, TF, 2)

    # ---- calls
    def _launch(self, who, z, *more):
        slot = self._calls % self.async_depth
        self._calls += 1
        self._async_bufs[(self.n, self._S, slot)] = True
        self.log.append((who, self.n, self._shape(z)) + more + (slot, self._calls))
        return {'id': self._calls, 'n': self.n, 'S': self._S, 'pred': _vals(self._calls, self.n, K, TF, 2)}

    def inference_async(self, z=None, metrics_gt=None, metrics_scale=1.0):
        return self._launch('inference_async', z, self._arg(metrics_gt), metrics_scale)

    def _run(self, who, z, *more):
        self._serial += 1
        self.log.append((who, self.n, self._shape(z)) + more)
        return _vals(1000 + self._serial, K, self.n, TF, 2)

    def inference(self, data=None, z=None):
        return self._run('inference', z, data is not None)

    def wait(self, h):
        self.log.append(('wait', h['id']))
        return h['pred'].permute(1, 0, 2, 3)

    # ---- metric passes: the *_async forms are seeded by the handle, the serial forms by the predictions they are given
    def best_of_k_async(self, h, gt=None, scale=1.0):
        self.log.append(('best_of_k_async', h['id'], self._arg(gt), scale))
        return _vals(h['id'], h['n']), _vals(h['id'] + 0.5, h['n'])

    def best_of_k(self, p, gt=None, scale=1.0):
        self.log.append(('best_of_k', list(p.shape), _sum(p), self._arg(gt), scale))
        return _vals(_sum(p), p.shape[0]), _vals(_sum(p) + 0.5, p.shape[0])

    def _segments(self, seg_ptr, h=None):
        if isinstance(seg_ptr, str):
            return h['S']
        return 0 if seg_ptr is None else len(seg_ptr) - 1

    @staticmethod
    def _selection(seed, n, S, gather):
        return types.SimpleNamespace(ade=_vals(seed, n), fde=_vals(seed + 0.25, n), seg_ade=_vals(seed + 0.5, S), seg_fde=_vals(seed + 0.75, S),
                                     seg_miss=_ints(seed, S), best_ade_idx=_ints(seed + 1, n), best_fde_idx=_ints(seed + 2, n),
                                     best=_vals(seed + 3, n, TF, 2) if gather else None)

    @staticmethod
    def _joint(seed, S, radius):
        return types.SimpleNamespace(seg_jade=_vals(seed + 4, S), seg_jfde=_vals(seed + 5, S), seg_jade_idx=_ints(seed + 6, S),
                                     seg_col=None if radius is None else _ints(seed + 7, S),
                                     seg_gt_col=None if radius is None else _ints(seed + 8, S))

    @staticmethod
    def _kde(seed, n):
        v = _vals(seed + 9, n, dtype=torch.float64)
        if n > 1:
            v[1] = float('nan')                                  # an agent whose samples' covariance is singular
        return v

    @staticmethod
    def _spread(seed, n):
        names = ('apd', 'fpd', 'pade', 'dlow', 'es_ade', 'es_fde')
        return types.SimpleNamespace(ade_at_k=_vals(seed + 16, n, K), fde_at_k=_vals(seed + 17, n, K),
                                     **{f: _vals(seed + 10 + i, n, dtype=torch.float64) for i, f in enumerate(names)})

    def select_best_of_k_async(self, h, **kw):
        self.log.append(('select_best_of_k_async', h['id'], self._opts(kw)))
        return self._selection(h['id'], h['n'], self._segments(kw.get('seg_ptr'), h), kw.get('gather', False))

    def select_best_of_k(self, p, **kw):
        self.log.append(('select_best_of_k', list(p.shape), _sum(p), self._opts(kw)))
        return self._selection(_sum(p), p.shape[0], self._segments(kw.get('seg_ptr')), kw.get('gather', False))

    def select_joint_async(self, h, **kw):
        self.log.append(('select_joint_async', h['id'], self._opts(kw)))
        return self._joint(h['id'], self._segments(kw.get('seg_ptr', 'scenes'), h), kw.get('collision_radius'))

    def select_joint(self, p, **kw):
        self.log.append(('select_joint', list(p.shape), _sum(p), self._opts(kw)))
        return self._joint(_sum(p), self._segments(kw['seg_ptr']), kw.get('collision_radius'))

    def kde_nll_async(self, h, **kw):
        self.log.append(('kde_nll_async', h['id'], self._opts(kw)))
        return self._kde(h['id'], h['n'])

    def kde_nll(self, p, **kw):
        self.log.append(('kde_nll', list(p.shape), _sum(p), self._opts(kw)))
        return self._kde(_sum(p), p.shape[0])

    def sample_spread_async(self, h, **kw):
        self.log.append(('sample_spread_async', h['id'], self._opts(kw)))
        return self._spread(h['id'], h['n'])

    def sample_spread(self, p, **kw):
        self.log.append(('sample_spread', list(p.shape), _sum(p), self._opts(kw)))
        return self._spread(_sum(p), p.shape[0])

    def horizon_metrics_async(self, h, **kw):
        self.log.append(('horizon_metrics_async', h['id'], self._opts(kw)))
        return _vals(h['id'], h['n'], TF, 2)


class _Sampler:
    def __init__(self, share_eps):
        self.share_eps = share_eps

    def inference_async(self, model, mean=True, eps=None, metrics_gt=None, metrics_scale=1.0):
        return model._launch('sampler.inference_async', None, mean, model._shape(eps), model._arg(metrics_gt), metrics_scale)

    def inference(self, model, mean=True, eps=None):
        return model._run('sampler.inference', None, mean, model._shape(eps))


def _plain(x, arrays):
    """A returned value as JSON (an EvalReport without its None fields); an array is appended to ``arrays`` and leaves its dtype and shape."""
    if dataclasses.is_dataclass(x):
        x = {f.name: getattr(x, f.name) for f in dataclasses.fields(x) if getattr(x, f.name) is not None}
    if isinstance(x, torch.Tensor):
        x = x.numpy()
    if isinstance(x, np.ndarray):
        arrays.append(x)
        return {'@': [str(x.dtype), list(x.shape)]}
    if isinstance(x, dict):
        return {str(k): _plain(v, arrays) for k, v in x.items()}
    if isinstance(x, (tuple, list)):
        return [_plain(v, arrays) for v in x]
    return x.item() if isinstance(x, np.generic) else x


SEVEN = [2, 1, 3, 2, 2, 1, 4]                                    # scenes_per_call=1: 7 calls, more than the window of 4; =3: a ragged last batch
FIFTEEN = list(range(1, 16))                                     # 15 batch shapes: more than 12 cached -> drain and reset_async
ALL_ON = dict(gather=True, joint=True, kde=True, collision_radius=0.3, spread=True, ks=(1, 2, 10))
NBA_A, NBA_B = (2, 3), (1, 3)


def _cases():
    """name -> run(ev) -> returned value; run gets the model, z_fn and eps_fn through its ``s`` namespace."""
    out = {}
    for dname, sizes, per in (('seven', SEVEN, 1), ('ragged', SEVEN, 3), ('shapes', FIFTEEN, 1)):
        for pip in (True, False):
            tag = f'{dname}-{"pipelined" if pip else "serial"}'
            kw = dict(traj_scale=1.5, scenes_per_call=per, pipelined=pip)
            ds = _Scenes(sizes)
            out[f'eval_scenes-{tag}'] = lambda ev, s, ds=ds, kw=kw: ev.eval_scenes(s.model, ds, z_fn=s.z_fn, **kw)
            out[f'eval_sampler-mean-{tag}'] = lambda ev, s, ds=ds, kw=kw: ev.eval_sampler(s.model, _Sampler(False), ds, mean=True,
                                                                                          eps_fn=s.eps_fn, **kw)
            for share in (True, False):
                out[f'eval_sampler-eps-share{int(share)}-{tag}'] = lambda ev, s, ds=ds, kw=kw, share=share: ev.eval_sampler(
                    s.model, _Sampler(share), ds, mean=False, eps_fn=s.eps_fn, **kw)
            for oname, o in (('plain', {}), ('all', ALL_ON)):
                out[f'eval_scenes_report-{oname}-{tag}'] = lambda ev, s, ds=ds, kw=kw, o=o: ev.eval_scenes_report(
                    s.model, ds, z_fn=s.z_fn, miss_threshold=2.0, **o, **kw)
                out[f'eval_sampler_report-{oname}-{tag}'] = lambda ev, s, ds=ds, kw=kw, o=o: ev.eval_sampler_report(
                    s.model, _Sampler(False), ds, mean=False, eps_fn=s.eps_fn, miss_threshold=2.0, **o, **kw)
    for pip in (True, False):
        tag = 'pipelined' if pip else 'serial'
        out[f'eval_scenes_reduced-{tag}'] = lambda ev, s, pip=pip: ev.eval_scenes_reduced(
            s.model, _Scenes(SEVEN), 7, K=2, traj_scale=1.5, scenes_per_call=3, z_fn=s.z_fn, pipelined=pip, spread=True, div_scale=2.0, ks=(1, 2))
        out[f'eval_scenes_reduced-shapes-{tag}'] = lambda ev, s, pip=pip: ev.eval_scenes_reduced(
            s.model, _Scenes(FIFTEEN[:8]), 2, scenes_per_call=1, z_fn=s.z_fn, pipelined=pip)
        for lname, shapes, per in (('alternating', [NBA_A, NBA_B] * 4 + [NBA_A], 2), ('one-shape', [NBA_A] * 9, 16),
                                   ('runs', [NBA_A] * 3 + [NBA_B] * 2 + [NBA_A] + [NBA_B] * 3, 2)):
            out[f'eval_nba-{lname}-{tag}'] = lambda ev, s, shapes=shapes, per=per, pip=pip: ev.eval_nba(
                s.model, _loader(shapes), traj_scale=1.5, z_fn=s.z_fn, pipelined=pip, groups_per_call=per)
    for lname, shapes in (('alternating', [NBA_A, NBA_B, NBA_A]), ('one-shape', [NBA_A] * 3)):
        for oname, o in (('plain', {}), ('all', ALL_ON)):
            out[f'eval_nba_report-{oname}-{lname}-serial'] = lambda ev, s, shapes=shapes, o=o: ev.eval_nba_report(
                s.model, _loader(shapes), traj_scale=1.5, z_fn=s.z_fn, pipelined=False, miss_threshold=2.0, **o)
    return out


CASES = _cases()
# the trace names a method by a short tag (the file holds some 2 400 calls)
TAGS = {'set_scene_batch': 'set', 'set_data_nba': 'set_nba', 'next_async_stream': 'stream', 'reset_async': 'reset', 'inference_async': 'async',
        'inference': 'serial', 'sampler.inference_async': 's.async', 'sampler.inference': 's.serial', 'best_of_k': 'bok',
        'select_best_of_k': 'sel', 'select_joint': 'joint', 'kde_nll': 'kde', 'sample_spread': 'spread', 'horizon_metrics': 'hm',
        'reduce_samples': 'reduce'}


def _tag(name):
    return TAGS.get(name) or (TAGS[name[:-6]] + '_async' if name.endswith('_async') else name)


def run_case(ev, name):
    """One case against the module ``ev``: ({'trace', 'opts', 'z_rows', 'eps_rows', 'result'} as plain JSON values, [arrays])."""
    from sttode_amd import metrics
    s = types.SimpleNamespace(model=_Model(), z_rows=[], eps_rows=[])

    def z_fn(rows):
        s.z_rows.append(rows)
        return _vals(len(s.z_rows), rows, ZD)

    def eps_fn(rows):
        s.eps_rows.append(rows)
        return _vals(len(s.eps_rows), rows, ZD)

    def reduce_samples(buf, Kc, iters=10, from_frame=0, init='first'):   # the k-means is a device pass: here a recorded stand-in
        s.model.log.append(('reduce_samples', list(buf.shape), _sum(buf), Kc, iters, from_frame, init))
        return types.SimpleNamespace(centroids=buf[0, :, :Kc].contiguous())
    s.z_fn, s.eps_fn = z_fn, eps_fn
    real, metrics.reduce_samples = metrics.reduce_samples, reduce_samples
    try:
        result = CASES[name](ev, s)
    finally:
        metrics.reduce_samples = real
    arrays = []
    trace = ';'.join(' '.join([_tag(c[0])] + [v if isinstance(v, str) else json.dumps(v, separators=(',', ':')) for v in c[1:]]) for c in s.model.log)   # 'tag arg arg;...'
    plain = {'trace': trace, 'opts': s.model.opts, 'z_rows': s.z_rows, 'eps_rows': s.eps_rows, 'result': _plain(result, arrays)}
    return json.loads(json.dumps(plain)), arrays


def record(ev, path=GOLDEN):
    """Write the golden pair from the evaluate module ``ev``."""
    runs = {name: run_case(ev, name) for name in CASES}
    with open(path + '.json', 'w') as f:
        f.write('{\n' + ',\n'.join(f'{json.dumps(n)}:{json.dumps(r[0], separators=(",", ":"))}' for n, r in runs.items()) + '\n}\n')
    np.savez_compressed(path + '.npz', bytes=np.frombuffer(b''.join(a.tobytes() for n in sorted(runs) for a in runs[n][1]), dtype=np.uint8))


@pytest.fixture(scope='module')
def golden():
    with open(GOLDEN + '.json') as f, np.load(GOLDEN + '.npz') as z:
        cases, blob, arrays = json.load(f), z['bytes'].tobytes(), {}

    def take(x, out):                                            # the arrays of a recorded value, in the order _plain met them
        nonlocal blob
        if isinstance(x, dict) and list(x) == ['@']:
            a = np.frombuffer(blob, dtype=x['@'][0], count=int(np.prod(x['@'][1]))).reshape(x['@'][1])
            out.append(a)
            blob = blob[a.nbytes:]
        elif isinstance(x, (dict, list)):
            for v in (x.values() if isinstance(x, dict) else x):
                take(v, out)
    for name in sorted(cases):
        take(cases[name]['result'], arrays.setdefault(name, []))
    assert not blob
    return cases, arrays


def test_the_golden_files_have_exactly_these_cases(golden):
    assert sorted(golden[0]) == sorted(CASES)


@pytest.mark.parametrize('name', sorted(CASES))
def test_loop_makes_the_calls_of_the_recorded_trace_and_returns_the_recorded_values(golden, name):
    from sttode_amd import evaluate
    (got, arrays), want = run_case(evaluate, name), golden[0][name]
    assert got['z_rows'] == want['z_rows'] and got['eps_rows'] == want['eps_rows'] and got['opts'] == want['opts']
    for i, (g, w) in enumerate(zip(got['trace'].split(';'), want['trace'].split(';'))):
        assert g == w, f'{name}: call {i} is {g}, recorded {w}'
    assert got['trace'] == want['trace']
    assert got['result'] == want['result']                             # every scalar, exactly; every array's place, dtype and shape
    for i, (a, w) in enumerate(zip(arrays, golden[1][name])):
        assert np.array_equal(a, w, equal_nan=True), f'{name}: array {i} of the result'


def test_the_cases_reach_the_window_the_ragged_batch_and_the_drain(golden):
    """What the cases are for, read off the recorded traces themselves."""
    def names(case):
        return [c.split()[0] for c in golden[0][case]['trace'].split(';')]
    t = names('eval_scenes-seven-pipelined')
    assert t.count('async') == 7 and t.index('wait') > [i for i, c in enumerate(t) if c == 'async'][4]   # 5 launched, then the first wait
    assert t.count('reset') == 1 and t[-1] == 'reset'
    assert [c for c in golden[0]['eval_scenes-ragged-pipelined']['trace'].split(';') if c.startswith('set ')] == ['set 6 3', 'set 5 3', 'set 4 1']
    assert names('eval_scenes-shapes-pipelined').count('reset') == 2                               # the drain, and the end of the loop
    assert names('eval_scenes_report-all-shapes-pipelined').count('reset') == 2
    assert names('eval_scenes_reduced-pipelined').count('async') == 7 * 3
    assert names('eval_scenes_reduced-shapes-pipelined').count('reset') == 2                       # the 7th shape: 12 cached + 6 slots > 16, one reset in the loop
    assert names('eval_nba-alternating-pipelined').count('async') == 9
    assert names('eval_nba-one-shape-pipelined').count('async') == 1
    assert names('eval_nba-runs-pipelined').count('async') == 6
