"""Best-of-K metrics on the device: utils/metrics.py of the reference, on the HIP selection kernel (csrc/frontend.hip
sttode_best_of_k_select).

``select`` is the kernel call: per agent the min-over-K ADE / FDE, the index of the best sample by ADE and by final displacement
(``get_best_idx``), the miss flag (``count_miss_samples``) and optionally the best trajectory; per CSR segment (a scene, an NBA batch) the
mean ADE / FDE and the miss count.  ``STTODENet.select_best_of_k`` / ``select_best_of_k_async`` call it on a model's data and pipeline.

``compute_ADE``, ``compute_FDE``, ``get_best_idx`` and ``count_miss_samples`` take the reference's arguments -- a list of [K, Tf, 2] arrays
and gt [n, Tf, 2], or stacked [n, K, Tf, 2] -- and return its types, so a script can swap ``from utils.metrics import ...`` for
``from sttode_amd.metrics import ...``.  They need a HIP device (there is no CPU fallback).
"""
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
