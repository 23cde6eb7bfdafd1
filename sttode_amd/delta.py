"""Gromov delta-hyperbolicity on HIP: same names / meaning as hyptorch/delta.py (Khrulkov et al., "Hyperbolic Image Embeddings").

``delta_hyp(D)`` is the Gromov delta of a distance matrix w.r.t. the base point 0 (delta.py:12-23); ``batched_delta_hyp(X)`` the mean and
(population) std of delta / diam over ``n_tries`` samples of ``batch_size`` rows drawn with replacement from numpy's global RNG
(delta.py:26-35); ``get_delta`` the absolute (delta, diam) of one 1500-row sample of features (delta.py:47-72), with the feature extractor
supplied by the caller.  The work is csrc/delta.hip (include/sttode_hip.h sttode_delta_*): no n x n x n array exists, and every try of a
call shares one launch.  CPU tensors raise (no fallback).  DESIGN.md §4m.
"""
import ctypes

import numpy as np
import torch

from . import capi

MAX_N = 32768


def _device(x=None):
    if isinstance(x, torch.Tensor):
        if not x.is_cuda:
            raise capi.SttodeError('sttode_amd.delta runs only on HIP tensors (no CPU fallback)')
        return x.device
    if not torch.cuda.is_available():
        raise capi.SttodeError('sttode_amd.delta needs a HIP device (no CPU fallback)')
    return torch.device('cuda', torch.cuda.current_device())


def _f32(x, what, shape_check=None):
    """numpy (any real dtype) or HIP tensor -> contiguous fp32 HIP tensor.  CPU tensors raise; a numpy input is checked (shape_check, and
    finiteness when asked) on the host before anything is copied."""
    if isinstance(x, torch.Tensor):
        dev = _device(x)
        if shape_check:
            shape_check(tuple(x.shape))
        return x.detach().to(dev, torch.float32).contiguous()
    a = np.asarray(x)
    if a.dtype.kind not in 'fiu':
        raise capi.SttodeError(f'{what}: expected a real-valued array, got dtype {a.dtype}')
    if shape_check:
        shape_check(a.shape)
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(_device())


def _check_n(n, what):
    if not 1 <= n <= MAX_N:
        raise capi.SttodeError(f'{what}: need 1 <= n <= {MAX_N} points, got {n}')


def _workspace(T, n, dev):
    f = ctypes.c_long()
    capi.call('sttode_delta_workspace', int(T), int(n), ctypes.byref(f))
    return torch.empty(int(f.value), dtype=torch.float32, device=dev)


def _delta(dist, T, n, symmetric):
    """dist [T, n, n] fp32 HIP -> delta [T] (device, no sync): one sttode_delta_hyp call."""
    ws = _workspace(T, n, dist.device)
    out = torch.empty(T, dtype=torch.float32, device=dist.device)
    capi.call('sttode_delta_hyp', dist, int(T), int(n), dist.numel(), int(bool(symmetric)), ws, ws.numel(), out, capi.stream_ptr())
    return out


def _dist(X, idx, T, n):
    """X [rows, d] fp32 HIP, idx [T, n] int32 HIP or None -> (dist [T, n, n], diam [T]) on the device (one sttode_delta_dist call)."""
    dist = torch.empty(T, n, n, dtype=torch.float32, device=X.device)
    diam = torch.empty(T, dtype=torch.float32, device=X.device)
    capi.call('sttode_delta_dist', X, X.shape[0], X.shape[1], idx, int(T), int(n), dist, dist.numel(), diam, capi.stream_ptr())
    return dist, diam


def _square_shape(shape):
    if len(shape) != 2 or shape[0] != shape[1]:
        raise capi.SttodeError(f'delta_hyp: dismat must be a square matrix, got shape {tuple(shape)}')
    _check_n(shape[0], 'delta_hyp')


def _square(dismat, finite):
    if finite and not isinstance(dismat, torch.Tensor) and not np.isfinite(np.asarray(dismat, dtype=np.float32)).all():
        _square_shape(np.shape(dismat))
        raise capi.SttodeError('delta_hyp: dismat has non-finite entries')
    D = _f32(dismat, 'delta_hyp', _square_shape)
    if finite and isinstance(dismat, torch.Tensor) and not bool(torch.isfinite(D).all()):    # the one host check (a sync)
        raise capi.SttodeError('delta_hyp: dismat has non-finite entries')
    return D


def delta_hyp_device(dismat, symmetric=False):
    """delta_hyp (delta.py:12-23) as a 0-d fp32 device tensor, without a synchronisation.  ``symmetric=True`` only when the caller knows
    dismat is bitwise symmetric (then only the upper triangle of tiles runs; same value).  No finiteness check: non-finite entries give an
    unspecified value."""
    D = _square(dismat, False)
    return _delta(D, 1, D.shape[0], symmetric)[0]


def delta_hyp(dismat):
    """Gromov delta of the distance matrix ``dismat`` [n, n] (numpy of any float dtype, copied as fp32, or a HIP tensor) w.r.t. point 0, as
    np.float64.  The general (non-symmetric) form, like the reference, which never checks symmetry."""
    D = _square(dismat, True)
    return np.float64(_delta(D, 1, D.shape[0], False)[0].item())


def _rows_shape(shape):
    if len(shape) != 2 or shape[0] < 1 or shape[1] < 1:
        raise capi.SttodeError(f'batched_delta_hyp: X must be [rows >= 1, d >= 1], got shape {tuple(shape)}')


def _rows(X):
    return _f32(X, 'batched_delta_hyp', _rows_shape)


def batched_deltas(X, idx, metric='euclidean', c=1.0):
    """delta and diam of the samples X[idx[t]] for every t, as two device tensors [T] (no sync).  idx [T, n] integer row indices."""
    X = _rows(X)
    idx = np.asarray(idx)
    if idx.ndim != 2 or idx.shape[0] < 1:
        raise capi.SttodeError(f'batched_delta_hyp: idx must be [n_tries >= 1, batch_size], got shape {idx.shape}')
    T, n = idx.shape
    _check_n(n, 'batched_delta_hyp')
    if idx.min() < 0 or idx.max() >= X.shape[0]:
        raise capi.SttodeError(f'batched_delta_hyp: idx outside [0, {X.shape[0]})')
    ix = torch.from_numpy(np.ascontiguousarray(idx, dtype=np.int32)).to(X.device)
    if metric == 'euclidean':
        dist, diam = _dist(X, ix, T, n)
        return _delta(dist, T, n, True), diam
    if metric == 'poincare':
        from . import pmath
        dist = torch.stack([pmath.dist_matrix(X[ix[t].long()], X[ix[t].long()], c) for t in range(T)])   # not bitwise symmetric
        return _delta(dist, T, n, False), dist.amax(dim=(1, 2))
    raise capi.SttodeError(f"batched_delta_hyp: metric must be 'euclidean' or 'poincare', got {metric!r}")


def batched_delta_hyp(X, n_tries=10, batch_size=1500, metric='euclidean', c=1.0, idx=None):
    """delta.py:26-35: ``n_tries`` samples of ``batch_size`` rows of X [rows, d] (numpy or HIP tensor), each drawn by
    ``np.random.choice(len(X), batch_size)`` in turn (the same rows and the same global RNG state afterwards as the reference); per sample
    delta_hyp(distance matrix) / its maximum.  Returns (mean, std) as np.float64 (population std; a sample of identical rows gives NaN, as
    the reference does).  ``idx`` [n_tries, batch_size]: explicit samples, the RNG untouched.  ``metric='poincare'``: Poincare-ball distances
    (pmath.dist_matrix with curvature c) and the general delta path.  All tries share one launch; one D2H copy at the end."""
    if idx is None:
        idx = np.stack([np.random.choice(len(X), batch_size) for _ in range(n_tries)])
    delta, diam = batched_deltas(X, idx, metric, c)
    both = torch.stack([delta, diam]).cpu().numpy().astype(np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        vals = both[0] / both[1]
    return np.mean(vals), np.std(vals)


def get_delta(loader, feature_fn=None, sample=1500):
    """delta.py:47-72: features of every image batch of ``loader`` (items ``(batch, label)``) by ``feature_fn(batch)`` -> rows, ONE sample
    of ``sample`` rows by ``np.random.choice``, returns the absolute (delta, diam) as np.float64.  The reference's extractor is a pretrained
    VGG16 (torchvision, weights fetched from the network): this project does not fetch it, so the caller passes its own."""
    if feature_fn is None:
        raise capi.SttodeError('get_delta needs feature_fn: the reference extracts features with torchvision vgg16(pretrained=True), whose '
                               'weights come from the network; this project fetches nothing -- pass a feature extractor')
    feats = []
    with torch.no_grad():
        for batch, _ in loader:
            f = feature_fn(batch)
            feats.append(f.reshape(f.shape[0], -1).float() if isinstance(f, torch.Tensor) else
                         torch.from_numpy(np.asarray(f, np.float32).reshape(len(f), -1)))
    X = _rows(torch.cat([f.to(_device()) for f in feats]))
    idx = np.random.choice(len(X), sample)[None]
    delta, diam = batched_deltas(X, idx)
    d = torch.stack([delta, diam]).cpu().numpy().astype(np.float64)
    return np.float64(d[0, 0]), np.float64(d[1, 0])
