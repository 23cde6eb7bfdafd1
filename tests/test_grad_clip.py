"""CPU tests of global-norm gradient clipping and the non-finite guard of sttode_amd.optim.Adam: the exports, the options' validation, the
state_dict surface, and the fallback (torch's own pieces, here on CPU tensors) against torch.nn.utils.clip_grad_norm_ + torch.optim.Adam."""
import math

import pytest
import torch

SHAPES = [(1,), (3,), (37,), (5, 3), (1025,)]


def _params(seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(s, generator=g)) for s in SHAPES]


def test_exports_and_abi_version():
    from sttode_amd import capi
    assert capi.ABI_VERSION == 15
    for name in ('sttode_grad_norm', 'sttode_adam_step_guarded', 'sttode_grad_scale'):
        assert name in capi.SIGNATURES
        assert hasattr(capi.lib(), name)
    # struct SttodeGradGroup of the header: four 8-byte slots (n padded), three doubles, one long
    import ctypes
    assert ctypes.sizeof(capi.GradGroup) == 64 and capi.GradGroup.gbase.offset == 24 and capi.GradGroup.step.offset == 56


def test_header_table_and_null_argument_checks_cover_the_new_rows():
    import test_capi_symbols as t
    t.test_ctypes_table_matches_header()
    t.test_library_exports_every_header_symbol()
    t.test_every_entry_point_rejects_null_arguments()
    from sttode_amd import capi
    L = capi.lib()
    for name in ('sttode_grad_norm', 'sttode_adam_step_guarded', 'sttode_grad_scale'):
        assert getattr(L, name)(*[0.0 if a in (capi._D, capi._F) else (0 if a in (capi._I, capi._L) else None) for a in capi.SIGNATURES[name]]) != 0
        assert name in L.sttode_last_error().decode()
    # arguments are checked before any launch: a bad max_norm, too many groups, a group without a table
    arr = (capi.GradGroup * 1)()
    for ngroups, max_norm in ((1, -1.0), (1, math.nan), (capi.GRAD_MAX_GROUPS + 1, 1.0), (1, 1.0)):
        assert L.sttode_grad_norm(arr, ngroups, 1, 1, max_norm, 0, 1, None) != 0
        assert 'sttode_grad_norm' in L.sttode_last_error().decode()


def test_fallback_clips_and_skips_like_torch_with_the_bad_step_left_out():
    from sttode_amd.optim import Adam
    ps_a, ps_b = _params(7), _params(7)
    oa = Adam(ps_a, lr=1e-2, max_grad_norm=0.5, skip_nonfinite=True)
    ob = torch.optim.Adam(ps_b, lr=1e-2, foreach=False)
    g = torch.Generator().manual_seed(8)
    for it in range(4):
        grads = [torch.randn(p.shape, generator=g) for p in ps_a]
        if it == 2:
            grads[4][1024] = math.nan
        for pa, ga in zip(ps_a, grads):
            pa.grad = ga.clone()
        oa.step()
        if it != 2:                                               # the reference run leaves the bad step out
            for pb, gb in zip(ps_b, grads):
                pb.grad = gb.clone()
            torch.nn.utils.clip_grad_norm_(ps_b, 0.5)
            ob.step()
            torch.testing.assert_close(oa.last_grad_norm, torch.linalg.vector_norm(torch.cat([x.flatten() for x in grads])), rtol=1e-6, atol=0)
        else:
            assert not math.isfinite(float(oa.last_grad_norm))
    for pa, pb in zip(ps_a, ps_b):
        assert torch.equal(pa, pb)
        for k in ('exp_avg', 'exp_avg_sq'):
            assert torch.equal(oa.state[pa][k], ob.state[pb][k])
    sd = oa.state_dict()
    assert all(float(st['step']) == 3 for st in sd['state'].values())
    assert oa.skipped_steps == 1
    # torch's class takes this state, and loading resets the counters from the loaded step
    torch.optim.Adam(ps_b, lr=1.0, foreach=False).load_state_dict(sd)
    oa.load_state_dict(ob.state_dict())
    assert oa.skipped_steps == 0
    assert all(float(st['step']) == 3 for st in oa.state_dict()['state'].values())


def test_guard_alone_and_clip_alone_on_the_fallback():
    from sttode_amd.optim import Adam
    ps_a, ps_b = _params(9), _params(9)
    oa, ob = Adam(ps_a, lr=1e-2, skip_nonfinite=True), torch.optim.Adam(ps_b, lr=1e-2, foreach=False)
    for it, bad in enumerate((False, True, False)):
        for pa, pb in zip(ps_a, ps_b):
            pa.grad = torch.full(pa.shape, 0.25 * (it + 1))
            pb.grad = pa.grad.clone()
        if bad:
            ps_a[1].grad[0] = math.inf
        oa.step()
        if not bad:
            ob.step()
    assert all(torch.equal(pa, pb) for pa, pb in zip(ps_a, ps_b)) and oa.skipped_steps == 1
    # clipping without the guard: a NaN norm reaches the parameters, as with torch's clip + step
    ps_c = _params(9)
    oc = Adam(ps_c, lr=1e-2, max_grad_norm=1.0)
    for pc in ps_c:
        pc.grad = torch.ones(pc.shape)
    ps_c[0].grad[0] = math.nan
    oc.step()
    assert all(torch.isnan(pc).all() for pc in ps_c) and oc.skipped_steps == 0


def test_clip_grad_norm_on_cpu_tensors_is_torchs():
    from sttode_amd import optim
    for max_norm, norm_type in ((0.5, 2.0), (100.0, 2.0), (0.5, 1.0), (0.5, math.inf)):
        ps_a, ps_b = _params(11), _params(11)
        for pa, pb in zip(ps_a, ps_b):
            pa.grad = torch.randn(pa.shape, generator=torch.Generator().manual_seed(pa.numel()))
            pb.grad = pa.grad.clone()
        ra = optim.clip_grad_norm_(ps_a, max_norm, norm_type=norm_type)
        rb = torch.nn.utils.clip_grad_norm_(ps_b, max_norm, norm_type=norm_type)
        assert torch.equal(ra, rb)
        assert all(torch.equal(pa.grad, pb.grad) for pa, pb in zip(ps_a, ps_b))
    p = torch.nn.Parameter(torch.zeros(3))
    p.grad = torch.tensor([1.0, math.nan, 0.0])
    with pytest.raises(RuntimeError):
        optim.clip_grad_norm_([p], 1.0, error_if_nonfinite=True)
    assert float(optim.clip_grad_norm_(p, 1.0)) != float(optim.clip_grad_norm_(p, 1.0))      # a single tensor, a NaN norm


@pytest.mark.parametrize('bad', [0, -1.0, 0.0, math.nan, math.inf, '1.0', [1.0], True])
def test_max_grad_norm_is_validated(bad):
    from sttode_amd.optim import Adam
    with pytest.raises(ValueError):
        Adam(_params(1), max_grad_norm=bad)


def test_options_are_not_param_group_entries():
    from sttode_amd.optim import Adam
    ps = _params(2)
    ref = torch.optim.Adam(ps).state_dict()['param_groups'][0]
    assert set(Adam(ps).state_dict()['param_groups'][0]) == set(ref)
    o = Adam(ps, max_grad_norm=2, skip_nonfinite=True)
    assert set(o.state_dict()['param_groups'][0]) == set(ref)
    assert o.max_grad_norm == 2.0 and o.skip_nonfinite is True and o.last_grad_norm is None and o.skipped_steps == 0


def test_train_epoch_prints_the_norm_only_when_asked():
    """trainer.train_epoch(log_grad_norm=True) appends the norm and the skipped count to the line it prints; the default line is unchanged."""
    import types
    from sttode_amd import trainer

    class Model:
        def train(self): pass
        def set_data(self, *a): pass
        def step_annealer(self): pass
        def forward(self):
            z = torch.zeros((), requires_grad=True)
            return z * 1.0, 0.0, 0.0, 0.0, 0.0
    opt = types.SimpleNamespace(zero_grad=lambda: None, step=lambda: None, last_grad_norm=torch.tensor(1.5), skipped_steps=2)
    args = types.SimpleNamespace(dataset='eth')
    batch = [[torch.zeros(1)] for _ in range(8)] + [['seq'], ['frame']]
    for flag, o in ((False, opt), (True, opt), (True, types.SimpleNamespace(zero_grad=opt.zero_grad, step=opt.step))):
        lines = []
        trainer.train_epoch(args, 0, Model(), o, None, [list(batch)], log=lines.append, log_grad_norm=flag)
        assert len(lines) == 1 and lines[0].startswith('Epochs: 00/01| It: 0000/0001 | Total loss: 0.000000|')
        assert lines[0].endswith('| Grad norm: 1.500000| Skipped steps: 2') == (flag and o is opt)
        assert ('Grad norm' in lines[0]) == (flag and o is opt)
