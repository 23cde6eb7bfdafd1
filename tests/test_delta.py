"""CPU tests of the Gromov delta-hyperbolicity drop-in (sttode_amd.delta, csrc/delta.hip, hyptorch/delta.py): the entry points are
exported and declared, the argument checks refuse bad shapes / limits before anything launches, the Python module refuses CPU tensors and
bad matrices, and the float32 NumPy restatement the GPU tests compare bitwise against agrees with the reference's own outputs."""
import ctypes

import numpy as np
import pytest

ENTRY = ('sttode_delta_dist', 'sttode_delta_workspace', 'sttode_delta_hyp')


def delta_f32(D, chunk=8):
    """delta.py:12-23 restated in float32, chunked over i: A = 0.5f ((D[0, j] + D[i, 0]) - D[i, j]), C[i, j] = max_k min(A[i, k], A[k, j]),
    max(C - A).  Min / max are exact, so this is the value any fp32 evaluation of the formula in this order gives, bit for bit."""
    D = np.asarray(D, np.float32)
    A = np.float32(0.5) * ((D[0, :][None, :] + D[:, 0][:, None]) - D)
    best = np.float32(-np.inf)
    for i0 in range(0, D.shape[0], chunk):
        C = np.minimum(A[i0:i0 + chunk, :, None], A[None, :, :]).max(axis=1)
        best = max(best, (C - A[i0:i0 + chunk]).max())
    return np.float32(best)


def dist_f64(X):
    X = np.asarray(X, np.float64)
    return np.sqrt(((X[:, None, :] - X[None, :, :]) ** 2).sum(-1))


def test_entry_points_exported_and_declared():
    from sttode_amd import capi
    from test_capi_symbols import header_functions
    fns = header_functions()
    L = capi.lib()
    assert capi.ABI_VERSION == 15 and L.sttode_abi_version() == 15
    for name in ENTRY:
        assert name in fns and name in capi.SIGNATURES and hasattr(L, name), name
        assert len(fns[name]) == len(capi.SIGNATURES[name]), name
    import sttode_amd.delta as d
    for name in ('delta_hyp', 'delta_hyp_device', 'batched_delta_hyp', 'get_delta'):
        assert callable(getattr(d, name)), name
    from sttode_amd import evaluate
    assert callable(evaluate.embedding_delta)


def test_argument_checks_before_launch():
    """Every limit is refused with a message naming the entry point (host logic only: no pointer is dereferenced, nothing launches)."""
    from sttode_amd import capi
    L = capi.lib()
    p = ctypes.c_void_p(0x1000)          # never dereferenced: every call below fails its checks first

    def refused(name, *args, match):
        assert getattr(L, name)(*args) != 0, (name, args)
        msg = L.sttode_last_error().decode()
        assert name in msg and match in msg, (name, msg)
    f = ctypes.c_long(-1)
    refused('sttode_delta_workspace', 1, 0, ctypes.byref(f), match='n must be')
    refused('sttode_delta_workspace', 1, 32769, ctypes.byref(f), match='n must be')
    refused('sttode_delta_workspace', 0, 10, ctypes.byref(f), match='T must be')
    refused('sttode_delta_workspace', 1, 10, None, match='null')
    assert L.sttode_delta_workspace(3, 300, ctypes.byref(f)) == 0 and f.value == 3 * 3 * 3       # 128 x 128 tiles: 3 x 3 per try
    assert L.sttode_delta_workspace(2, 32768, ctypes.byref(f)) == 0 and f.value == 2 * 256 * 256
    refused('sttode_delta_hyp', p, 1, 0, 0, 0, p, 100, p, None, match='n must be')
    refused('sttode_delta_hyp', p, 1, 32769, 1 << 40, 0, p, 1 << 20, p, None, match='n must be')
    refused('sttode_delta_hyp', p, 10, 1500, 10 * 1500 * 1500 - 1, 1, p, 10 ** 6, p, None, match='T n^2')
    refused('sttode_delta_hyp', p, 2, 32768, 2 * 32768 ** 2 - 1, 1, p, 10 ** 6, p, None, match='T n^2')   # 64-bit n^2
    refused('sttode_delta_hyp', p, 10, 1500, 10 * 1500 * 1500, 0, p, 10 * 144 - 1, p, None, match='workspace')
    refused('sttode_delta_hyp', p, 1, 10, 100, 2, p, 100, p, None, match='symmetric')
    refused('sttode_delta_dist', p, 100, 0, p, 1, 10, p, 100, p, None, match='d >= 1')
    refused('sttode_delta_dist', p, 100, 8, None, 2, 100, p, 2 * 100 * 100, p, None, match='without idx')
    refused('sttode_delta_dist', p, 100, 8, None, 1, 50, p, 50 * 50, p, None, match='without idx')
    refused('sttode_delta_dist', p, 100, 8, p, 10, 1500, p, 10 * 1500 * 1500 - 1, p, None, match='T n^2')
    refused('sttode_delta_dist', p, 100, 8, p, 1, 32769, p, 1 << 40, p, None, match='n must be')


def test_python_module_refuses_bad_input():
    import torch
    from sttode_amd import capi, delta
    with pytest.raises(capi.SttodeError, match='HIP'):
        delta.delta_hyp(torch.zeros(4, 4))                                  # CPU tensor: no fallback
    with pytest.raises(capi.SttodeError, match='HIP'):
        delta.delta_hyp_device(torch.zeros(4, 4))
    with pytest.raises(capi.SttodeError, match='HIP'):
        delta.batched_delta_hyp(torch.zeros(10, 3), n_tries=1, batch_size=4)
    with pytest.raises(capi.SttodeError, match='square'):
        delta.delta_hyp(np.zeros((3, 4)))
    with pytest.raises(capi.SttodeError, match='square'):
        delta.delta_hyp(np.zeros(5))
    with pytest.raises(capi.SttodeError, match='n <= '):
        delta.delta_hyp(np.zeros((0, 0)))
    for bad in (np.inf, -np.inf, np.nan):
        D = np.zeros((3, 3))
        D[1, 2] = bad
        with pytest.raises(capi.SttodeError, match='non-finite'):
            delta.delta_hyp(D)


def test_get_delta_needs_a_feature_extractor():
    from sttode_amd import capi, delta
    with pytest.raises(capi.SttodeError, match='feature_fn.*network'):
        delta.get_delta([(np.zeros((2, 3)), None)])


def test_f32_restatement_matches_the_reference_outputs(golden):
    """The restatement the GPU tests pin the kernel to bitwise is the reference's formula: against delta.npz (reference in float64)."""
    g = golden('delta')
    for tag in ('gauss', 'circle', 'clusters', 'n1', 'n2', 'n3', 'n65'):
        X = g['dh_%s_X' % tag]
        D = dist_f64(X)
        assert abs(D.max() - g['dh_%s_diam' % tag]) <= 1e-9 * (1 + g['dh_%s_diam' % tag])
        assert abs(float(delta_f32(D)) - g['dh_%s_delta' % tag]) <= 2e-6 * max(D.max(), 1.0), tag
    assert abs(float(delta_f32(g['ns_D'])) - g['ns_delta']) <= 2e-6 * g['ns_D'].max()
    # the reference's delta >= 0 for any input: k = i is a candidate of C[i, i]
    assert all(g['dh_%s_delta' % t] >= 0 for t in ('gauss', 'circle', 'clusters', 'n1', 'n2', 'n3', 'n65'))
