"""CPU tests of the hyperbolic layers (sttode_amd/hypnn.py): the fixture tests/golden/hypnn.npz checks itself, the modules have
the reference's surface (state_dict names, shapes, initial values under the same seed), and the new entry points refuse bad arguments by
name before any launch.  The kernels themselves: test_hypnn_gpu.py."""
import ctypes

import numpy as np
import pytest
import torch

from hypnn_cases import BOUND, INIT_MODULES, MODULES, TRAIN_STEPS, case_arrays, case_forward, case_grads, err, function_cases


def all_cases():
    return [name for name, _, _ in function_cases()] + ['mod.' + name for name in MODULES]


def test_fixture_holds_every_case_and_the_reference_fp32_is_within_the_bound(golden):
    z = golden('hypnn')
    worst = worst_fwd = 0.0
    for case in all_cases():
        ins, _, g = case_arrays(z, case)
        grads = case_grads(z, case)
        assert ins and g.dtype == np.float32 and len(grads) >= len(ins), case
        assert all(a.dtype == np.float32 for a in ins), case
        for key, ref, r32 in grads:
            assert ref.dtype == np.float32 and np.isfinite(ref).all() and np.isfinite(r32).all(), (case, key)
            e = err(r32, ref)
            worst = max(worst, e)
            assert e <= BOUND, (case, key, e)
        if case.startswith('mod.'):                                    # the module's forward value: the shape of g, fp32 run within the bound
            ref, r32 = case_forward(z, case)
            assert ref.dtype == np.float32 and ref.size == g.size and np.isfinite(ref).all() and np.isfinite(r32).all(), case
            e = err(r32, ref)
            worst_fwd = max(worst_fwd, e)
            assert e <= BOUND, (case, 'out', e)
        else:
            assert case + '.out64' not in z, case
    assert len(all_cases()) == 27 and sum(k.endswith('.out64') for k in z) == sum(k.endswith('.out32d') for k in z) == len(MODULES) == 14
    assert z['train.loss64'].shape == z['train.loss32'].shape == (TRAIN_STEPS,) and z['train.loss64'].dtype == np.float64
    assert err(z['train.loss32'], z['train.loss64']) <= BOUND
    print('worst reference fp32 error over the fixture: %.2e (gradients), %.2e (module forward values)' % (worst, worst_fwd))


def test_modules_have_the_reference_state_dict_and_initial_values(golden):
    import sttode_amd.hypnn as hn
    z = golden('hypnn')
    for name, make in INIT_MODULES.items():
        torch.manual_seed(0)
        sd = make(hn).state_dict()
        assert list(sd) == list(z['init.%s.names' % name]), name
        for k, v in sd.items():
            ref = z['init.%s.%s' % (name, k)]
            assert tuple(v.shape) == ref.shape and v.dtype == torch.float32, (name, k)
            assert np.array_equal(v.numpy(), ref), (name, k)
    assert any(len(z['init.%s.names' % n]) for n in INIT_MODULES)


def test_surface_of_the_modules():
    import sttode_amd.hypnn as hn
    from sttode_amd import pmath
    assert repr(hn.HyperbolicMLR(8, 5, c=1.0)) == 'HyperbolicMLR(Poincare ball dim=8, n_classes=5, c=1.0)'
    assert repr(hn.HypLinear(16, 8, c=0.5, bias=False)) == 'HypLinear(in_features=16, out_features=8, bias=False, c=0.5)'
    assert 'dims 16 and 5 ---> dim 8' in repr(hn.ConcatPoincareLayer(16, 5, 8, c=1.0))
    assert repr(hn.HyperbolicDistanceLayer(c=0.5)) == 'HyperbolicDistanceLayer(c=0.5)'
    assert repr(hn.FromPoincare(c=1.0)) == 'FromPoincare(train_c=False, train_x=False)'
    try:
        m = hn.ToPoincare(c=0.5, clip_r=2.3)
        assert repr(m) == 'ToPoincare(c=0.5, train_x=False)' and m.clip_r == 2.3 and m.xp is None
        assert m.riemannian is pmath.RiemannianGradient and pmath.RiemannianGradient.c == 0.5      # as the reference: a class attribute
    finally:
        pmath.RiemannianGradient.c = 1
    for cls in (hn.ToPoincare, hn.FromPoincare):
        with pytest.raises(ValueError, match='ball_dim'):
            cls(c=1.0, train_x=True)
        assert tuple(cls(c=1.0, train_x=True, ball_dim=7).xp.shape) == (7,)
        with pytest.raises(NotImplementedError, match='train_c'):
            cls(c=1.0, train_c=True)
    pmath.RiemannianGradient.c = 1


def test_modules_refuse_cpu_tensors():
    import sttode_amd.hypnn as hn
    from sttode_amd import capi, pmath
    x = 0.1 * torch.ones(3, 8)
    try:
        for call in (lambda: hn.HyperbolicMLR(8, 5, c=1.0)(x), lambda: hn.HypLinear(8, 4, c=1.0)(x), lambda: hn.ToPoincare(c=1.0, clip_r=1.0)(x),
                     lambda: hn.ConcatPoincareLayer(8, 8, 4, c=1.0)(x, x), lambda: hn.HyperbolicDistanceLayer(c=1.0)(x, x),
                     lambda: hn.FromPoincare(c=1.0)(x), lambda: pmath.feature_clip(x, 1.0), lambda: pmath._hyperbolic_softmax(x, x, x, 1.0),
                     lambda: pmath._mobius_addition_batch(x, x, 1.0)):
            with pytest.raises(capi.SttodeError, match='HIP tensors'):
                call()
    finally:
        pmath.RiemannianGradient.c = 1


def test_new_exports_are_present_and_the_abi_version_is_unchanged():
    from sttode_amd import capi, pmath
    L = capi.lib()
    assert capi.ABI_VERSION == 15 and L.sttode_abi_version() == 15
    for name in ('sttode_pmath_hsoftmax_bwd', 'sttode_pmath_clip', 'sttode_pmath_clip_bwd'):
        assert name in capi.SIGNATURES and hasattr(L, name)
    assert callable(pmath.feature_clip)


def test_new_entry_points_refuse_bad_arguments_by_name_without_a_launch():
    """Every refusal comes from the argument check in front of the launch, so this runs without a GPU; the pointers are host addresses that
    a launch would never be handed."""
    from sttode_amd import capi
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    hs = 'sttode_pmath_hsoftmax_bwd'
    for args, word in (((None,) * 8 + (3, 4, 8, 1.0), 'null pointer'), ((p, p, p, p, None, p, p, p, 3, 4, 8, 1.0), 'null pointer'),
                       ((p,) * 8 + (0, 4, 8, 1.0), 'positive'), ((p,) * 8 + (3, 0, 8, 1.0), 'positive'), ((p,) * 8 + (3, 4, 0, 1.0), 'positive'),
                       ((p,) * 8 + (1 << 16, 1 << 16, 8, 1.0), 'pairs'), ((p,) * 8 + (3, 4, 8, 0.0), 'curvature'),
                       ((p,) * 8 + (3, 4, 8, -1.0), 'curvature')):
        with pytest.raises(capi.SttodeError, match=hs + '.*' + word):
            capi.call(hs, *args, None)
    for args, word in (((None, p, 3, 8, 1.0), 'null pointer'), ((p, p, 0, 8, 1.0), 'empty shape'), ((p, p, 3, 8, 0.0), 'radius'),
                       ((p, p, 3, 8, -2.0), 'radius')):
        with pytest.raises(capi.SttodeError, match='sttode_pmath_clip: .*' + word):
            capi.call('sttode_pmath_clip', *args, None)
    for args, word in (((p, None, p, 3, 8, 1.0), 'null pointer'), ((p, p, p, 3, 0, 1.0), 'empty shape'), ((p, p, p, 3, 8, 0.0), 'radius')):
        with pytest.raises(capi.SttodeError, match='sttode_pmath_clip_bwd: .*' + word):
            capi.call('sttode_pmath_clip_bwd', *args, None)
    assert buf.raw == b'\0' * 64
