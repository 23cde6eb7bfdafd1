"""Best-of-K metrics on the device: utils/metrics.py of the reference, on the HIP selection kernel (csrc/frontend.hip
sttode_best_of_k_select).

``joint_select`` and ``kde_nll`` (csrc/metrics.hip) are the scene-level metrics the reference does not compute: joint min ADE / FDE
and collision counts per segment, and the KDE NLL per agent.  ``sample_spread`` compares an agent's samples with each other:
pairwise distances, the DLow kernel value, energy scores and best-of-k for every k.  ``multimodal`` (csrc/multimodal.hip)
scores them against the futures of all agents with a similar history, over a whole dataset: MMADE / MMFDE.  ``reduce_samples`` (csrc/reduce.hip)
clusters M sampled futures per agent to K representatives, ``reduce_scenes`` (csrc/reduce_scenes.hip) a segment's M scene
futures, all its agents under one label, so that representative k is a coherent scene future.  ``weighted_set`` (csrc/weighted.hip) scores K samples with
probabilities -- those representatives and their cluster shares -- as a weighted set: expected errors, energy scores, the KDE NLL of the
weighted mixture, probability-ranked best-of-k.  ``large_select`` / ``large_kde_nll`` / ``large_spread`` (csrc/large_set.hip)
score the M <= 4096 samples themselves, before any reduction: best-of-M with prefix minima, joint best-of-M, KDE NLL, pair statistics
(DESIGN.md 4ac).

``select`` is the kernel call: per agent the min-over-K ADE / FDE, the index of the best sample by ADE and by final displacement
(``get_best_idx``), the miss flag (``count_miss_samples``) and optionally the best trajectory; per CSR segment (a scene, an NBA batch) the
mean ADE / FDE and the miss count.  ``STTODENet.select_best_of_k`` / ``select_best_of_k_async`` call it on a model's data and pipeline.

``compute_ADE``, ``compute_FDE``, ``get_best_idx`` and ``count_miss_samples`` take the reference's arguments -- a list of [K, Tf, 2] arrays
and gt [n, Tf, 2], or stacked [n, K, Tf, 2] -- and return its types, so a script can swap ``from utils.metrics import ...`` for
``from sttode_amd.metrics import ...``.  They need a HIP device (there is no CPU fallback).
"""
import ctypes

import numpy as np
import torch

from . import capi


class Selection:
    """Outputs of one selection pass (device tensors).  Per agent: ``ade``, ``fde`` [n] float32; ``best_ade_idx``, ``best_fde_idx`` [n]
    int32; ``miss`` [n] bool; ``best`` [n, Tf, 2] (``gather=True``, else None).  Per segment (``seg_ptr`` given, else None): ``seg_ade``,
    ``seg_fde`` [S] float32, ``seg_miss`` [S] int32."""
    __slots__ = ('ade', 'fde', 'best_ade_idx', 'best_fde_idx', 'miss', 'best', 'seg_ade', 'seg_fde', 'seg_miss')

    def __init__(self, n, S, Tf, device, gather):
        f = torch.empty(2 * n + 2 * S, dtype=torch.float32, device=device)
        i = torch.empty(2 * n + S, dtype=torch.int32, device=device)
        self.ade, self.fde = f[:n], f[n:2 * n]
        self.best_ade_idx, self.best_fde_idx = i[:n], i[n:2 * n]
        self.miss = torch.empty(n, dtype=torch.bool, device=device)
        self.best = torch.empty(n, Tf, 2, dtype=torch.float32, device=device) if gather else None
        self.seg_ade = f[2 * n:2 * n + S] if S else None
        self.seg_fde = f[2 * n + S:] if S else None
        self.seg_miss = i[2 * n:] if S else None

    def args(self):
        """Output pointers in the order of sttode_best_of_k_select."""
        return (self.ade, self.fde, self.best_ade_idx, self.best_fde_idx, self.miss, self.best, self.seg_ade, self.seg_fde, self.seg_miss)

    def record_stream(self, stream):
        """Keep the outputs' memory from the caching allocator until the work queued on ``stream`` so far has run."""
        for t in (self.ade, self.best_ade_idx, self.miss, self.best):   # (views: the record covers the whole allocation)
            if t is not None:
                t.record_stream(stream)


def check_k(K):
    if K > 64:
        raise ValueError(f'best-of-K selection supports K <= 64 samples (one lane per sample), got K = {K}')


def seg_ptr_tensor(seg_ptr, device):
    """seg_ptr as a contiguous int32 device tensor (returned as is when it already is one)."""
    if isinstance(seg_ptr, torch.Tensor) and seg_ptr.dtype == torch.int32 and seg_ptr.device == device and seg_ptr.is_contiguous():
        return seg_ptr
    return torch.as_tensor(np.asarray(seg_ptr) if not isinstance(seg_ptr, torch.Tensor) else seg_ptr, dtype=torch.int32).to(device).contiguous()


@torch.no_grad()
def select(pred_nk, gt, scale=1.0, miss_threshold=1.0, seg_ptr=None, gather=False):
    """Best-of-K selection of pred_nk [n, K, Tf, 2] against gt [n, Tf, 2] (device tensors, float32) on the current stream of their device.
    ``scale`` multiplies the displacements (traj_scale); ``miss_threshold`` is compared with the scaled FDE, strictly (count_miss_samples);
    ``seg_ptr`` [S+1] (device or host, int): per-segment outputs.  Returns a ``Selection``."""
    if not (isinstance(pred_nk, torch.Tensor) and pred_nk.is_cuda):
        raise capi.SttodeError('best-of-K selection runs on a HIP device only (no CPU fallback): pass device tensors')
    dev = pred_nk.device
    pred_nk = pred_nk.to(torch.float32).contiguous()
    n, K, Tf = pred_nk.shape[:3]
    check_k(K)
    gt = torch.as_tensor(gt, dtype=torch.float32).to(dev).contiguous()
    if tuple(gt.shape) != (n, Tf, 2):
        raise ValueError(f'gt must be [{n}, {Tf}, 2], got {tuple(gt.shape)}')
    sp = seg_ptr_tensor(seg_ptr, dev) if seg_ptr is not None else None
    S = int(sp.numel()) - 1 if sp is not None else 0
    out = Selection(n, S, Tf, dev, gather)
    with torch.cuda.device(dev):
        capi.call('sttode_best_of_k_select', pred_nk, gt, n, K, Tf, float(scale), float(miss_threshold), sp, S, *out.args(),
                  capi.stream_ptr())
    return out


# ----- scene-level metrics (csrc/metrics.hip: sttode_joint_select, sttode_kde_nll) -------------------------------------------

class JointSelection:
    """Outputs of one joint pass (device tensors), per segment s of ``seg_ptr``: ``seg_jade`` / ``seg_jfde`` [S] float32 (min over k of the
    segment's mean ADE / FDE of sample k), ``seg_jade_idx`` / ``seg_jfde_idx`` [S] int32 (that k, the lowest on exact ties); with a collision
    radius ``seg_col`` [S] int32 (colliding agents summed over the K samples) and ``seg_gt_col`` [S] int32 (colliding agents of the ground
    truth), else None."""
    __slots__ = ('seg_jade', 'seg_jfde', 'seg_jade_idx', 'seg_jfde_idx', 'seg_col', 'seg_gt_col', 'radius')

    def __init__(self, S, device, radius):
        f = torch.empty(2 * S, dtype=torch.float32, device=device)
        i = torch.empty((4 if radius else 2) * S, dtype=torch.int32, device=device)
        self.seg_jade, self.seg_jfde = f[:S], f[S:]
        self.seg_jade_idx, self.seg_jfde_idx = i[:S], i[S:2 * S]
        self.seg_col = i[2 * S:3 * S] if radius else None
        self.seg_gt_col = i[3 * S:] if radius else None
        self.radius = radius

    def args(self):
        """radius and output pointers in the order of sttode_joint_select."""
        return (float(self.radius or 0.0), self.seg_jade, self.seg_jfde, self.seg_jade_idx, self.seg_jfde_idx, self.seg_col, self.seg_gt_col)

    def record_stream(self, stream):
        for t in (self.seg_jade, self.seg_jade_idx):   # (views: the record covers the whole allocation)
            t.record_stream(stream)


def check_radius(collision_radius):
    """None (no collision pass) or a positive float."""
    if collision_radius is None:
        return None
    r = float(collision_radius)
    if not r > 0.0:
        raise ValueError(f'collision_radius must be positive (or None: no collision pass), got {collision_radius}')
    return r


def check_kde_k(K):
    if K < 2 or K > 64:
        raise ValueError(f'KDE NLL needs 2 <= K <= 64 samples (a covariance; one LDS tile per frame block), got K = {K}')


def _inputs(pred_nk, gt, what, need_gt=True):
    if not (isinstance(pred_nk, torch.Tensor) and pred_nk.is_cuda):
        raise capi.SttodeError(f'{what} runs on a HIP device only (no CPU fallback): pass device tensors')
    if pred_nk.dim() != 4 or pred_nk.shape[3] != 2 or 0 in pred_nk.shape:
        raise ValueError(f'pred_nk must be [n, K, Tf, 2] with n, K, Tf > 0, got {tuple(pred_nk.shape)}')
    dev = pred_nk.device
    pred_nk = pred_nk.to(torch.float32).contiguous()
    n, K, Tf = pred_nk.shape[:3]
    if gt is None and not need_gt:
        return pred_nk, None, n, K, Tf
    gt = torch.as_tensor(gt, dtype=torch.float32).to(dev).contiguous()
    if tuple(gt.shape) != (n, Tf, 2):
        raise ValueError(f'gt must be [{n}, {Tf}, 2], got {tuple(gt.shape)}')
    return pred_nk, gt, n, K, Tf


def check_seg_ptr(sp, n):
    """A CSR [S+1] with S >= 1; a host one must also run non-decreasing from 0 to n (a device one is not read back: the kernels clamp every
    segment to [0, n])."""
    if isinstance(sp, torch.Tensor) and sp.is_cuda:
        if sp.dim() != 1 or sp.numel() < 2:
            raise ValueError(f'seg_ptr must be a CSR [S+1] with S >= 1, got shape {tuple(sp.shape)}')
        return
    v = sp.numpy() if isinstance(sp, torch.Tensor) else np.asarray(sp)
    if v.ndim != 1 or v.size < 2 or v[0] != 0 or v[-1] != n or (np.diff(v) < 0).any():
        raise ValueError(f'seg_ptr must be a non-decreasing CSR [S+1] from 0 to n = {n}')


@torch.no_grad()
def joint_select(pred_nk, gt, seg_ptr, scale=1.0, collision_radius=None):
    """Joint (scene-level) best-of-K of pred_nk [n, K, Tf, 2] against gt [n, Tf, 2] per segment of the CSR ``seg_ptr`` [S+1] (device or
    host), on the current stream: one sample index k for the whole segment, min over k of the mean over its agents of ADE(a, k) / FDE(a, k)
    (summed in double); with ``collision_radius`` r > 0 also the collision counts of the samples and of the ground truth (an agent collides
    if another agent of its segment comes closer than r, strictly, at some frame of the same sample).  K <= 64.  Returns a
    ``JointSelection``."""
    pred_nk, gt, n, K, Tf = _inputs(pred_nk, gt, 'joint selection')
    check_k(K)
    r = check_radius(collision_radius)
    check_seg_ptr(seg_ptr, n)
    sp = seg_ptr_tensor(seg_ptr, pred_nk.device)
    out = JointSelection(int(sp.numel()) - 1, pred_nk.device, r)
    with torch.cuda.device(pred_nk.device):
        capi.call('sttode_joint_select', pred_nk, gt, n, K, Tf, float(scale), sp, int(sp.numel()) - 1, *out.args(), capi.stream_ptr())
    return out


@torch.no_grad()
def kde_nll(pred_nk, gt, scale=1.0):
    """KDE negative log-likelihood of gt [n, Tf, 2] under the K samples of pred_nk [n, K, Tf, 2] per agent (Trajectron++'s
    compute_kde_nll: a Gaussian KDE with Scott's bandwidth per frame, log-density clipped below at -20, averaged over the frames), in
    float64 on the current stream.  Returns a float64 tensor [n]: NaN for an agent whose samples have a singular covariance at some frame
    (where scipy.stats.gaussian_kde raises).  2 <= K <= 64."""
    pred_nk, gt, n, K, Tf = _inputs(pred_nk, gt, 'KDE NLL')
    check_kde_k(K)
    out = torch.empty(n, dtype=torch.float64, device=pred_nk.device)
    with torch.cuda.device(pred_nk.device):
        capi.call('sttode_kde_nll', pred_nk, gt, n, K, Tf, float(scale), out, capi.stream_ptr())
    return out


# ----- spread of the samples among themselves (csrc/metrics.hip: sttode_sample_spread) --------------------------------------

class SampleSpread:
    """Outputs of one spread pass (device tensors), per agent.  float64 [n]: ``apd`` (mean over the sample pairs of the trajectory
    distance: DLow's APD), ``fpd`` (of the final-frame distance), ``pade`` (of the mean per-frame distance), ``dlow`` (of
    exp(-d_traj^2 / div_scale): the per-agent term of ``samplerloss.diversity_loss``); with a ground truth, else None: ``es_ade`` /
    ``es_fde`` [n] float64 (energy scores on the ADE / FDE distance) and ``ade_at_k`` / ``fde_at_k`` [n, K] float32 (column k-1: min ADE /
    FDE over the first k samples)."""
    __slots__ = ('apd', 'fpd', 'pade', 'dlow', 'es_ade', 'es_fde', 'ade_at_k', 'fde_at_k', 'K', 'div_scale')

    def __init__(self, n, K, device, div_scale, has_gt):
        d = torch.empty((6 if has_gt else 4) * n, dtype=torch.float64, device=device)
        self.apd, self.fpd, self.pade, self.dlow = d[:n], d[n:2 * n], d[2 * n:3 * n], d[3 * n:4 * n]
        self.es_ade = d[4 * n:5 * n] if has_gt else None
        self.es_fde = d[5 * n:] if has_gt else None
        f = torch.empty(2 * n * K, dtype=torch.float32, device=device) if has_gt else None
        self.ade_at_k = f[:n * K].view(n, K) if has_gt else None
        self.fde_at_k = f[n * K:].view(n, K) if has_gt else None
        self.K, self.div_scale = K, div_scale

    def args(self):
        """div_scale and output pointers in the order of sttode_sample_spread."""
        return (float(self.div_scale), self.apd, self.fpd, self.pade, self.dlow, self.es_ade, self.es_fde, self.ade_at_k, self.fde_at_k)

    def at(self, k):
        """(min ADE, min FDE) [n] over the first ``k`` samples, 1 <= k <= K (needs a ground truth)."""
        if self.ade_at_k is None:
            raise ValueError('best-of-k columns need a ground truth (sample_spread was called without gt)')
        k = int(k)
        if not 1 <= k <= self.K:
            raise ValueError(f'k must be in [1, {self.K}], got {k}')
        return self.ade_at_k[:, k - 1], self.fde_at_k[:, k - 1]

    def record_stream(self, stream):
        for t in (self.apd, self.ade_at_k):   # (views: the record covers the whole allocation)
            if t is not None:
                t.record_stream(stream)


def check_spread(K, div_scale):
    """div_scale as a float, after the checks of sttode_sample_spread."""
    if K < 2 or K > 64:
        raise ValueError(f'sample spread needs 2 <= K <= 64 samples (a pair; one lane per sample), got K = {K}')
    ds = float(div_scale)
    if not (ds > 0.0 and ds != float('inf')):
        raise ValueError(f'div_scale must be positive and finite, got {div_scale}')
    return ds


@torch.no_grad()
def sample_spread(pred_nk, gt=None, scale=1.0, div_scale=1.0):
    """How spread out the K samples of pred_nk [n, K, Tf, 2] are among themselves, per agent, in float64 on the current stream
    (include/sttode_hip.h sttode_sample_spread states every value): average / final pairwise distance, the DLow kernel value at
    ``div_scale``, and with gt [n, Tf, 2] the energy scores and the best-of-k minima for every k <= K.  2 <= K <= 64.  Returns a
    ``SampleSpread``."""
    pred_nk, gt, n, K, Tf = _inputs(pred_nk, gt, 'sample spread', need_gt=False)
    ds = check_spread(K, div_scale)
    out = SampleSpread(n, K, pred_nk.device, ds, gt is not None)
    with torch.cuda.device(pred_nk.device):
        capi.call('sttode_sample_spread', pred_nk, gt, n, K, Tf, float(scale), *out.args(), capi.stream_ptr())
    return out


# ----- weighted sample sets (csrc/weighted.hip: sttode_weighted_set) --------------------------------------------------------

class WeightedSet:
    """Outputs of one weighted-set pass (device tensors), per agent.  float64 [n]: ``eade`` / ``efde`` (expected ADE / FDE under the
    normalised weights), ``es_ade`` / ``es_fde`` (energy scores), ``apd`` / ``fpd`` (expected trajectory / final-frame distance between two
    different draws; NaN with a single positive weight), ``kde_nll`` (the NLL under scipy's weighted gaussian_kde; NaN with fewer than three
    positive weights or a singular covariance), ``brier_ade`` / ``brier_fde`` (min ADE / FDE + (1 - p of that sample)^2), ``neff`` (1 / sum
    p^2).  float32 [n, K]: ``ade_top`` / ``fde_top`` (column k-1: min ADE / FDE over the k most probable samples).  A row whose weights
    are negative, non-finite or all zero is NaN everywhere."""
    F64 = ('eade', 'efde', 'es_ade', 'es_fde', 'apd', 'fpd', 'kde_nll', 'brier_ade', 'brier_fde', 'neff')
    __slots__ = F64 + ('ade_top', 'fde_top', 'K')

    def __init__(self, n, K, device):
        d = torch.empty(len(self.F64) * n, dtype=torch.float64, device=device)
        for i, name in enumerate(self.F64):
            setattr(self, name, d[i * n:(i + 1) * n])
        f = torch.empty(2 * n * K, dtype=torch.float32, device=device)
        self.ade_top, self.fde_top = f[:n * K].view(n, K), f[n * K:].view(n, K)
        self.K = K

    def args(self):
        """Output pointers in the order of sttode_weighted_set."""
        return tuple(getattr(self, name) for name in self.F64) + (self.ade_top, self.fde_top)

    def at(self, k):
        """(min ADE, min FDE) [n] over the ``k`` most probable samples, 1 <= k <= K."""
        k = int(k)
        if not 1 <= k <= self.K:
            raise ValueError(f'k must be in [1, {self.K}], got {k}')
        return self.ade_top[:, k - 1], self.fde_top[:, k - 1]

    def record_stream(self, stream):
        for t in (self.eade, self.ade_top):   # (views: the record covers the whole allocation)
            t.record_stream(stream)


def check_weighted_k(K):
    if K < 1 or K > 64:
        raise ValueError(f'a weighted sample set needs 1 <= K <= 64 samples (one lane per sample), got K = {K}')


@torch.no_grad()
def weighted_set(pred_nk, weights, gt, scale=1.0):
    """The K samples of pred_nk [n, K, Tf, 2] as a weighted set -- ``weights`` [n, K] float32, raw: ``Reduction.weights``,
    ``Reduction.counts.float()`` or any mode probabilities, normalised per agent on the device -- scored against gt [n, Tf, 2], in float64
    on the current stream (include/sttode_hip.h sttode_weighted_set states every value).  A sample with weight 0 is not part of the set.
    1 <= K <= 64.  Returns a ``WeightedSet``."""
    pred_nk, gt, n, K, Tf = _inputs(pred_nk, gt, 'a weighted sample set')
    check_weighted_k(K)
    if not (isinstance(weights, torch.Tensor) and weights.is_cuda):
        raise capi.SttodeError('a weighted sample set runs on a HIP device only (no CPU fallback): pass the weights as a device tensor')
    if weights.dtype != torch.float32:
        raise ValueError(f'weights must be float32 (Reduction.weights, or Reduction.counts.float()), got {weights.dtype}')
    if tuple(weights.shape) != (n, K) or weights.device != pred_nk.device:
        raise ValueError(f'weights must be [{n}, {K}] on {pred_nk.device}, got {tuple(weights.shape)} on {weights.device}')
    out = WeightedSet(n, K, pred_nk.device)
    with torch.cuda.device(pred_nk.device):
        capi.call('sttode_weighted_set', pred_nk, weights.contiguous(), gt, n, K, Tf, float(scale), *out.args(), capi.stream_ptr())
    return out


# ----- multi-modal ground truth over a dataset (csrc/multimodal.hip: sttode_multimodal) -------------------------------------

MM_MAX_AGENTS = 1 << 20


class MultiModal:
    """Outputs of one multi-modal pass (device tensors), per agent: ``count`` [n] int32 (the agents of its segment whose anchored history
    lies within eps of its own, itself included), ``mmade`` / ``mmfde`` [n] float64 (the mean over those neighbours of the best sample's
    ADE / FDE against the neighbour's future translated to the agent's anchor)."""
    __slots__ = ('count', 'mmade', 'mmfde', 'eps', 'hist_frames')

    def __init__(self, n, device, eps, hist_frames):
        d = torch.empty(2 * n, dtype=torch.float64, device=device)
        self.mmade, self.mmfde = d[:n], d[n:]
        self.count = torch.empty(n, dtype=torch.int32, device=device)
        self.eps, self.hist_frames = eps, hist_frames

    def args(self):
        """Output pointers in the order of sttode_multimodal."""
        return (self.count, self.mmade, self.mmfde)

    def record_stream(self, stream):
        for t in (self.count, self.mmade):   # (views: the record covers the whole allocation)
            t.record_stream(stream)


def check_multimodal(n, K, Tp, Tf, eps, hist_frames, scale):
    """(eps, hist_frames) as a float and an int (None: Tp - 1), after the checks of sttode_multimodal."""
    if not 1 <= n <= MM_MAX_AGENTS:
        raise ValueError(f'multi-modal ground truth needs 1 <= n <= 2^20 agents, got n = {n}')
    if K < 1 or K > 64:
        raise ValueError(f'multi-modal ground truth needs 1 <= K <= 64 samples (one lane per sample), got K = {K}')
    if Tp < 2:
        raise ValueError(f'multi-modal ground truth needs Tp >= 2 (an anchor and one history frame), got Tp = {Tp}')
    h = Tp - 1 if hist_frames is None else int(hist_frames)
    if not 1 <= h <= Tp - 1:
        raise ValueError(f'hist_frames must be in [1, Tp - 1 = {Tp - 1}], got {hist_frames}')
    e = float(eps)
    if not (e >= 0.0 and e != float('inf')):
        raise ValueError(f'eps must be non-negative and finite, got {eps}')
    if not np.isfinite(float(scale)):
        raise ValueError(f'scale must be finite, got {scale}')
    return e, h


@torch.no_grad()
def multimodal(pred_nk, past, gt, eps, hist_frames=None, scale=1.0, seg_ptr=None):
    """MMADE / MMFDE of pred_nk [n, K, Tf, 2] over the whole set of agents, in float64 on the current stream (include/sttode_hip.h
    sttode_multimodal states every value): the neighbours of agent i are the agents of its segment -- ``seg_ptr`` [S+1], device or host; all
    agents without it -- whose last ``hist_frames`` (default Tp - 1) frames of past [n, Tp, 2], relative to the last observed position, lie
    within ``eps`` (scaled units, Euclidean over the 2 hist_frames numbers) of its own; their futures gt [n, Tf, 2], translated to i's last
    position, are scored against i's K samples.  n <= 2^20, K <= 64.  The workspace is the function's own.  Returns a ``MultiModal``."""
    pred_nk, gt, n, K, Tf = _inputs(pred_nk, gt, 'multi-modal ground truth')
    dev = pred_nk.device
    past = torch.as_tensor(past, dtype=torch.float32).to(dev).contiguous()
    if past.dim() != 3 or past.shape[0] != n or past.shape[2] != 2:
        raise ValueError(f'past must be [{n}, Tp, 2], got {tuple(past.shape)}')
    Tp = int(past.shape[1])
    e, h = check_multimodal(n, K, Tp, Tf, eps, hist_frames, scale)
    sp, S = None, 0
    if seg_ptr is not None:
        check_seg_ptr(seg_ptr, n)
        sp = seg_ptr_tensor(seg_ptr, dev)
        S = int(sp.numel()) - 1
    out = MultiModal(n, dev, e, h)
    ws = torch.empty((2 * h + 2) * n, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        capi.call('sttode_multimodal', pred_nk, past, gt, sp, S, n, K, Tp, Tf, h, float(scale), e, ws, int(ws.numel()), *out.args(),
                  capi.stream_ptr())
    return out


# ----- oversample and reduce (csrc/reduce.hip: sttode_reduce_samples) ------------------------------------------------------

class Reduction:
    """Outputs of one reduction (device tensors): ``centroids`` [n, K, Tf, 2] float32 (full mean trajectories), ``labels`` [n, M] int32 (the
    cluster of every sample), ``counts`` [n, K] int32 (cluster sizes) and ``weights`` [n, K] float32 = counts / M."""
    __slots__ = ('centroids', 'labels', 'counts', 'M', '_weights')

    def __init__(self, n, M, K, Tf, device):
        self.centroids = torch.empty(n, K, Tf, 2, dtype=torch.float32, device=device)
        i = torch.empty(n * M + n * K, dtype=torch.int32, device=device)
        self.labels, self.counts = i[:n * M].view(n, M), i[n * M:].view(n, K)
        self.M = M
        self._weights = None

    @property
    def weights(self):
        if self._weights is None:
            self._weights = self.counts.to(torch.float32) / float(self.M)
        return self._weights


REDUCE_INIT = {'first': 0, 'maximin': 1}


def _need_device(pred, what):
    if not (isinstance(pred, torch.Tensor) and pred.is_cuda):
        raise capi.SttodeError(f'{what} runs on a HIP device only (no CPU fallback): pass device tensors')


def _round_major(pred):
    """``pred`` as [R, n, K_in, Tf, 2]: [n, M, Tf, 2] is R = 1."""
    if pred.dim() == 4:
        pred = pred.unsqueeze(0)
    if pred.dim() != 5 or pred.shape[4] != 2 or 0 in pred.shape:
        raise ValueError(f'pred must be [n, M, Tf, 2] or [R, n, K_in, Tf, 2] with no empty dimension, got {tuple(pred.shape)}')
    return pred


def _reduce_args(K, iters, from_frame, init, n, M, Tf, dev, what):
    """(K, iters, first frame in [0, Tf), init mode, init tensor or None) of the two reductions after their checks."""
    K, iters, from_frame = int(K), int(iters), int(from_frame)
    if not -Tf <= from_frame < Tf:
        raise ValueError(f'from_frame must be in [-{Tf}, {Tf}), got {from_frame}')
    if isinstance(init, str):
        if init not in REDUCE_INIT:
            raise ValueError(f"init must be 'first', 'maximin' or a tensor [n, K, Tf, 2], got {init!r}")
        mode, init_t = REDUCE_INIT[init], None
    else:
        mode, init_t = 2, torch.as_tensor(init, dtype=torch.float32).to(dev).contiguous()
        if tuple(init_t.shape) != (n, K, Tf, 2):
            raise ValueError(f'init must be [{n}, {K}, {Tf}, 2], got {tuple(init_t.shape)}')
    if not 1 <= K <= 64 or not K <= M <= 4096:
        raise ValueError(f'{what} needs 1 <= K <= 64 and K <= M <= 4096, got K = {K}, M = {M}')
    return K, iters, from_frame % Tf, mode, init_t


@torch.no_grad()
def reduce_samples(pred, K, iters=10, from_frame=0, init='first'):
    """Lloyd k-means of every agent's M sampled futures to K representatives, on the current stream (include/sttode_hip.h
    sttode_reduce_samples states the iteration).  ``pred``: [n, M, Tf, 2], or [R, n, K_in, Tf, 2] -- R stacked outputs of inference,
    M = R K_in, sample m = r K_in + k.  ``from_frame``: the first frame the distances look at (0: whole trajectories; -1: endpoints; negative
    values count from the end); the representatives are full mean trajectories either way.  ``init``: 'first' (samples 0 .. K-1), 'maximin'
    (farthest-point, deterministic) or a tensor [n, K, Tf, 2].  K <= 64, K <= M <= 4096.  Returns a ``Reduction``."""
    _need_device(pred, 'sample reduction')
    pred = _round_major(pred).to(torch.float32).contiguous()
    dev = pred.device
    R, n, K_in, Tf = pred.shape[:4]
    K, iters, f0, mode, init_t = _reduce_args(K, iters, from_frame, init, n, R * K_in, Tf, dev, 'sample reduction')
    out = Reduction(n, R * K_in, K, Tf, dev)
    with torch.cuda.device(dev):
        capi.call('sttode_reduce_samples', pred, n, R, K_in, Tf, K, iters, f0, mode, init_t, out.centroids, out.labels, out.counts,
                  capi.stream_ptr())
    return out


# ----- oversample and reduce whole scenes (csrc/reduce_scenes.hip: sttode_reduce_scenes) ----------------------------------

class SceneReduction:
    """Outputs of one scene-level reduction (device tensors): ``centroids`` [n, K, Tf, 2] float32 (representative k of a segment's agents is
    one scene future), ``labels`` [S, M] int32 (the cluster of every scene future), ``counts`` [S, K] int32, ``weights`` [S, K] float32 =
    counts / M, ``seg_ptr`` [S+1] int32 as used, and ``agent_weights`` [n, K] float32: every agent's segment row of ``weights`` (a gather on
    the device; 0 for an agent outside every segment), what ``weighted_set`` takes."""
    __slots__ = ('centroids', 'labels', 'counts', 'seg_ptr', 'M', '_weights', '_agent_weights')

    def __init__(self, n, S, M, K, Tf, device, seg_ptr):
        self.centroids = torch.empty(n, K, Tf, 2, dtype=torch.float32, device=device)
        i = torch.empty(S * M + S * K, dtype=torch.int32, device=device)
        self.labels, self.counts = i[:S * M].view(S, M), i[S * M:].view(S, K)
        self.seg_ptr, self.M = seg_ptr, M
        self._weights = self._agent_weights = None

    @property
    def weights(self):
        if self._weights is None:
            self._weights = self.counts.to(torch.float32) / float(self.M)
        return self._weights

    @property
    def agent_weights(self):
        if self._agent_weights is None:
            n, S = self.centroids.shape[0], self.counts.shape[0]
            sp = torch.cummax(self.seg_ptr.to(torch.int64).clamp(0, n), dim=0)[0]      # (as the kernel clamps a device CSR)
            a = torch.arange(n, device=sp.device)
            seg = torch.bucketize(a, sp[1:], right=True)                               # the segment whose [start, end) holds agent a
            inside = ((a >= sp[0]) & (a < sp[-1])).unsqueeze(1)
            self._agent_weights = torch.where(inside, self.weights[seg.clamp(max=S - 1)], torch.zeros((), device=sp.device))
        return self._agent_weights


@torch.no_grad()
def reduce_scenes(pred, seg_ptr=None, K=None, iters=10, from_frame=0, init='first', *, seg_len=None):
    """Lloyd k-means of every segment's M sampled SCENE futures to K representatives, on the current stream (include/sttode_hip.h
    sttode_reduce_scenes states the iteration): sample m of a segment is sample m of all its agents together, so its agents share one label
    per sample and representative k is a coherent scene future again -- what the joint metrics, the collision rate and ``weighted_set`` need.
    ``pred``: [n, M, Tf, 2] or [R, n, K_in, Tf, 2] as for ``reduce_samples``.  ``seg_ptr``: CSR [S+1] (tensor, array or list; a host one must
    run non-decreasing from 0 to n), or ``seg_len=N``: uniform segments of N agents (NBA games).  ``iters``, ``from_frame``, ``init`` as
    ``reduce_samples`` ('maximin' picks whole scene futures).  K <= 64, K <= M <= 4096; a segment may be all n agents.  Returns a
    ``SceneReduction``."""
    _need_device(pred, 'scene reduction')
    if K is None:
        raise ValueError('scene reduction needs K, the number of representatives')
    pred = _round_major(pred).to(torch.float32).contiguous()
    dev = pred.device
    R, n, K_in, Tf = pred.shape[:4]
    if (seg_ptr is None) == (seg_len is None):
        raise ValueError('scene reduction needs seg_ptr [S+1] or seg_len=N (uniform segments), one of them')
    if seg_len is not None:
        N = int(seg_len)
        if N < 1 or n % N:
            raise ValueError(f'seg_len must be a positive divisor of n = {n}, got {seg_len}')
        seg_ptr = torch.arange(0, n + 1, N, dtype=torch.int32, device=dev)
    else:
        check_seg_ptr(seg_ptr, n)
    sp = seg_ptr_tensor(seg_ptr, dev)
    S = int(sp.numel()) - 1
    K, iters, f0, mode, init_t = _reduce_args(K, iters, from_frame, init, n, R * K_in, Tf, dev, 'scene reduction')
    if not 1 <= iters <= 1000:
        raise ValueError(f'iters must be in [1, 1000], got {iters}')
    out = SceneReduction(n, S, R * K_in, K, Tf, dev, sp)
    with torch.cuda.device(dev):
        capi.call('sttode_reduce_scenes', pred, n, R, K_in, Tf, K, iters, f0, mode, init_t, sp, S, out.centroids, out.labels, out.counts,
                  capi.stream_ptr())
    return out


# ----- scores of a whole oversampled set (csrc/large_set.hip: sttode_large_select / _kde_nll / _spread) -------------------

LARGE_MAX_M, LARGE_MAX_TF, LARGE_MAX_KS = 4096, 200, 16


class LargeSelection:
    """Outputs of one ``large_select`` pass (device tensors).  Per agent: ``ade``, ``fde`` [n] float32 (min over the M samples),
    ``best_ade_idx``, ``best_fde_idx`` [n] int32 (the lowest m that attains it; +inf and 0 for an agent without a finite sample), ``miss``
    [n] bool; ``ade_at`` / ``fde_at`` [n, len(ks)] float32 (column i: the minimum over the first ``ks[i]`` samples; None without ``ks``).
    Per segment (``seg_ptr`` given, else None): ``seg_jade`` / ``seg_jfde`` [S] float32 and ``seg_jade_idx`` / ``seg_jfde_idx`` [S] int32
    (an empty segment: NaN and -1).  ``M``, ``ks``."""
    __slots__ = ('ade', 'fde', 'best_ade_idx', 'best_fde_idx', 'miss', 'ade_at', 'fde_at', 'seg_jade', 'seg_jfde', 'seg_jade_idx',
                 'seg_jfde_idx', 'M', 'ks')

    def __init__(self, n, M, ks, S, device):
        nk = len(ks)
        f = torch.empty(2 * n + 2 * n * nk + 2 * S, dtype=torch.float32, device=device)
        i = torch.empty(2 * n + 2 * S, dtype=torch.int32, device=device)
        self.ade, self.fde = f[:n], f[n:2 * n]
        self.ade_at = f[2 * n:2 * n + n * nk].view(n, nk) if nk else None
        self.fde_at = f[2 * n + n * nk:2 * n + 2 * n * nk].view(n, nk) if nk else None
        o = 2 * n + 2 * n * nk
        self.seg_jade = f[o:o + S] if S else None
        self.seg_jfde = f[o + S:] if S else None
        self.best_ade_idx, self.best_fde_idx = i[:n], i[n:2 * n]
        self.seg_jade_idx = i[2 * n:2 * n + S] if S else None
        self.seg_jfde_idx = i[2 * n + S:] if S else None
        self.miss = torch.empty(n, dtype=torch.bool, device=device)
        self.M, self.ks = M, tuple(ks)

    def args(self):
        """Output pointers in the order of sttode_large_select."""
        return (self.ade, self.fde, self.best_ade_idx, self.best_fde_idx, self.miss, self.ade_at, self.fde_at, self.seg_jade, self.seg_jfde,
                self.seg_jade_idx, self.seg_jfde_idx)

    def at(self, k):
        """(min ADE, min FDE) [n] over the first ``k`` samples, ``k`` one of ``ks``."""
        if int(k) not in self.ks:
            raise ValueError(f'k must be one of ks = {self.ks}, got {k}')
        c = self.ks.index(int(k))
        return self.ade_at[:, c], self.fde_at[:, c]

    def record_stream(self, stream):
        for t in (self.ade, self.best_ade_idx, self.miss):   # (views: the record covers the whole allocation)
            t.record_stream(stream)


class LargeSpread:
    """Outputs of one ``large_spread`` pass (device tensors), per agent, float64 [n]: ``apd``, ``fpd``, ``pade``, ``dlow`` as
    ``SampleSpread``'s, over the M (M-1) / 2 pairs; with a ground truth, else None: ``es_ade`` / ``es_fde``.  ``M``, ``div_scale``."""
    __slots__ = ('apd', 'fpd', 'pade', 'dlow', 'es_ade', 'es_fde', 'M', 'div_scale')

    def __init__(self, n, M, device, div_scale, has_gt):
        d = torch.empty((6 if has_gt else 4) * n, dtype=torch.float64, device=device)
        self.apd, self.fpd, self.pade, self.dlow = d[:n], d[n:2 * n], d[2 * n:3 * n], d[3 * n:4 * n]
        self.es_ade = d[4 * n:5 * n] if has_gt else None
        self.es_fde = d[5 * n:] if has_gt else None
        self.M, self.div_scale = M, div_scale

    def args(self):
        """Output pointers in the order of sttode_large_spread."""
        return (self.apd, self.fpd, self.pade, self.dlow, self.es_ade, self.es_fde)

    def record_stream(self, stream):
        self.apd.record_stream(stream)   # (views: the record covers the whole allocation)


class SampleScores:
    """What ``STTODENet.score_samples`` returns: ``select`` (a ``LargeSelection``), ``kde_nll`` (float64 [n], or None) and ``spread`` (a
    ``LargeSpread``, or None)."""
    __slots__ = ('select', 'kde_nll', 'spread')

    def __init__(self, select, kde_nll=None, spread=None):
        self.select, self.kde_nll, self.spread = select, kde_nll, spread


def _large_inputs(pred, gt, what, need_gt=True, m_min=1):
    """(pred [R, n, K_in, Tf, 2] -- the caller's memory when it is contiguous float32 --, gt, R, n, K_in, Tf) after the entries' checks."""
    _need_device(pred, what)
    pred = _round_major(pred)
    if pred.dtype != torch.float32:
        raise ValueError(f'pred must be float32, got {pred.dtype}')
    R, n, K_in, Tf = pred.shape[:4]
    if not m_min <= R * K_in <= LARGE_MAX_M:
        raise ValueError(f'{what} needs {m_min} <= M <= {LARGE_MAX_M} samples, got M = {R * K_in}')
    if Tf > LARGE_MAX_TF:
        raise ValueError(f'{what} needs Tf <= {LARGE_MAX_TF}, got Tf = {Tf}')
    pred = pred.contiguous()
    if gt is None and not need_gt:
        return pred, None, R, n, K_in, Tf
    gt = torch.as_tensor(gt, dtype=torch.float32).to(pred.device).contiguous()
    if tuple(gt.shape) != (n, Tf, 2):
        raise ValueError(f'gt must be [{n}, {Tf}, 2], got {tuple(gt.shape)}')
    return pred, gt, R, n, K_in, Tf


@torch.no_grad()
def large_select(pred, gt, scale=1.0, miss_threshold=1.0, ks=(), seg_ptr=None):
    """Best-of-M over a whole oversampled set, on the current stream (include/sttode_hip.h sttode_large_select states every value).
    ``pred``: [n, M, Tf, 2], or [R, n, K_in, Tf, 2] -- the round buffer of ``inference_reduced``, M = R K_in, sample m = r K_in + k -- float32,
    read in place; gt [n, Tf, 2].  1 <= M <= 4096.  ``ks``: up to 16 prefix sizes, strictly ascending in [1, M]: the minima over the first k
    samples (best-of-20 beside best-of-M from one pass).  ``seg_ptr`` [S+1] (device or host): joint best-of-M per segment.  Returns a
    ``LargeSelection``."""
    pred, gt, R, n, K_in, Tf = _large_inputs(pred, gt, 'large-set selection')
    M = R * K_in
    ks = [int(k) for k in ks]
    if len(ks) > LARGE_MAX_KS or any(not 1 <= k <= M for k in ks) or any(b <= a for a, b in zip(ks, ks[1:])):
        raise ValueError(f'ks must be at most {LARGE_MAX_KS} values, strictly ascending in [1, M = {M}], got {ks}')
    sp, S, ws = None, 0, None
    if seg_ptr is not None:
        check_seg_ptr(seg_ptr, n)
        sp = seg_ptr_tensor(seg_ptr, pred.device)
        S = int(sp.numel()) - 1
        ws = torch.empty(capi.large_set_ws('sttode_large_select', n, M), dtype=torch.uint8, device=pred.device)
    out = LargeSelection(n, M, ks, S, pred.device)
    kh = (ctypes.c_int * len(ks))(*ks) if ks else None
    with torch.cuda.device(pred.device):
        capi.call('sttode_large_select', pred, gt, n, R, K_in, Tf, float(scale), float(miss_threshold),
                  ctypes.cast(kh, ctypes.c_void_p) if ks else None, len(ks), sp, S, ws, int(ws.numel()) if ws is not None else 0, *out.args(),
                  capi.stream_ptr())
    return out


@torch.no_grad()
def large_kde_nll(pred, gt, scale=1.0):
    """``kde_nll`` over a whole oversampled set (3 <= M <= 4096; Trajectron++ reports it at 2000 samples), float64 on the current stream.
    ``pred`` as ``large_select``.  Returns a float64 tensor [n], NaN where the covariance is singular at some frame."""
    pred, gt, R, n, K_in, Tf = _large_inputs(pred, gt, 'large-set KDE NLL', m_min=3)
    out = torch.empty(n, dtype=torch.float64, device=pred.device)
    with torch.cuda.device(pred.device):
        capi.call('sttode_large_kde_nll', pred, gt, n, R, K_in, Tf, float(scale), out, capi.stream_ptr())
    return out


@torch.no_grad()
def large_spread(pred, gt=None, scale=1.0, div_scale=1.0):
    """``sample_spread``'s pair statistics over a whole oversampled set (2 <= M <= 4096: up to 8.4 million pairs per agent), float64 on the
    current stream.  ``pred`` as ``large_select``.  The best-of-k columns are ``large_select``'s (``ks``).  Returns a ``LargeSpread``."""
    pred, gt, R, n, K_in, Tf = _large_inputs(pred, gt, 'large-set spread', need_gt=False, m_min=2)
    ds = float(div_scale)
    if not (ds > 0.0 and ds != float('inf')):
        raise ValueError(f'div_scale must be positive and finite, got {div_scale}')
    out = LargeSpread(n, R * K_in, pred.device, ds, gt is not None)
    ws = torch.empty(capi.large_set_ws('sttode_large_spread', n, R * K_in), dtype=torch.uint8, device=pred.device)
    with torch.cuda.device(pred.device):
        capi.call('sttode_large_spread', pred, gt, n, R, K_in, Tf, float(scale), ds, ws, int(ws.numel()), *out.args(), capi.stream_ptr())
    return out


# ----- drop-ins for utils/metrics.py ---------------------------------------------------------------------------------------------------

def _device():
    if not torch.cuda.is_available():
        raise capi.SttodeError('sttode_amd.metrics needs a HIP device (no CPU fallback)')
    return torch.device('cuda', torch.cuda.current_device())


def _stack(pred_arr, gt_arr):
    """(pred [n, K, Tf, 2], gt [n, Tf, 2]) device tensors from the reference's arguments (zip semantics: the shorter one sets n)."""
    def dev_of(x):
        return x.device if isinstance(x, torch.Tensor) and x.is_cuda else None
    dev = dev_of(pred_arr) or dev_of(gt_arr) or _device()
    if isinstance(pred_arr, (list, tuple)):
        if len(pred_arr) == 0:
            raise ZeroDivisionError('no agents')
        pred = torch.stack([torch.as_tensor(p, dtype=torch.float32).to(dev) for p in pred_arr])
    else:
        pred = torch.as_tensor(pred_arr, dtype=torch.float32).to(dev)
    gt = torch.as_tensor(np.asarray(gt_arr) if not isinstance(gt_arr, torch.Tensor) else gt_arr, dtype=torch.float32).to(dev)
    n = min(pred.shape[0], gt.shape[0])
    if n == 0:
        raise ZeroDivisionError('no agents')
    return pred[:n], gt[:n]


def compute_ADE(pred_arr, gt_arr):
    """Mean over agents of the min over samples of the mean displacement (utils/metrics.py:7-15)."""
    sel = select(*_stack(pred_arr, gt_arr))
    return np.float64(sel.ade.double().sum().item() / sel.ade.numel())


def compute_FDE(pred_arr, gt_arr):
    """Mean over agents of the min over samples of the final displacement (utils/metrics.py:18-26)."""
    sel = select(*_stack(pred_arr, gt_arr))
    return np.float64(sel.fde.double().sum().item() / sel.fde.numel())


def get_best_idx(pred_arr, gt_arr):
    """Per agent, the index of the sample with the smallest mean displacement, the first one on ties (utils/metrics.py:29-36)."""
    return select(*_stack(pred_arr, gt_arr)).best_ade_idx.cpu().tolist()


def count_miss_samples(pred_arr, gt_arr, mr_threshold=1):
    """Number of agents whose min-over-samples final displacement exceeds mr_threshold (utils/metrics.py:39-48)."""
    return int(select(*_stack(pred_arr, gt_arr), miss_threshold=float(mr_threshold)).miss.sum().item())
