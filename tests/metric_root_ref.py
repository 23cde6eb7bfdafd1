"""Float64 yardstick of the per-agent displacement kernels of csrc/frontend.hip (best_of_k_kernel, bok_select_kernel, bok_segments_kernel,
horizon_metrics_kernel), a float32 restatement of what a correct fp32 evaluation in their order gives, and the bounds between the two.
Plain NumPy: importable without a GPU.

The bounds are derived, not measured; u = 2^-24 is the unit roundoff of float32, and every bound is relative to the float64 value.
  one distance  dx and dy are rounded twice each (the difference, the product with scale): under 2 u relative in each, so under 2 u in
                the norm; dy*dy and the fma round once each under the root, which halves them: 1 u; sqrtf rounds once: 1 u.  Under
                5 u to first order.
  ADE           Tf - 1 additions of non-negative terms (each at most 1 u of the running sum) and one division:
                bound_ade(Tf) = (Tf + 8) u.
  FDE           one distance: bound_fde = 6 u.
  min over k    is one of the per-sample values: no more than the worst per-sample error (given the gaps metric_root_cases asserts).
  horizon h     the running mean of the first h frames: (h + 8) u; its last-frame value: bound_fde.
  segment mean  of na agents against the float64 mean of the very float32 per-agent values that were added (which isolates
                bok_segments_kernel): a lane adds at most ceil(na / 64) values (ceil(na / 64) - 1 additions), a six-step tree adds the 64
                partial sums, one division: bound_seg(na) = (ceil(na / 64) + 8) u.
"""
import numpy as np

from helpers import bok_dist_np

U = 2.0 ** -24


def bound_ade(Tf):
    return (Tf + 8) * U


bound_fde = 6 * U


def bound_horizon(Tf):
    """[Tf, 2]: the bounds of out[:, h - 1] = (running mean over h frames, frame h)."""
    return np.stack([(np.arange(1, Tf + 1) + 8) * U, np.full(Tf, bound_fde)], axis=-1)


def bound_seg(na):
    return (-(-int(na) // 64) + 8) * U


# -------------------------------------------------------------------------------------------------------------------------------------
# float64
# -------------------------------------------------------------------------------------------------------------------------------------
def dist64(pred, gt, scale):
    """pred [n,K,Tf,2], gt [n,Tf,2]: the float32 arrays the kernel receives -> |scale (pred - gt)| [n,K,Tf], the difference, the product
    with float64(float32(scale)) and the norm all in float64."""
    assert pred.dtype == np.float32 and gt.dtype == np.float32
    s = np.float64(np.float32(scale))
    d = (pred.astype(np.float64) - gt.astype(np.float64)[:, None]) * s
    return np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1])


def per_sample(d):
    """Distances [n,K,Tf] -> (ADE [n,K] = mean over frames, FDE [n,K] = last frame), in d's type for float64; see per_sample32."""
    return d.mean(axis=-1), d[..., -1]


def first_min(v):
    """v [n,K] -> (minimum over k [n], its first index [n]); a NaN entry never wins (fminf), an all-NaN row gives (+inf, 0)."""
    w = np.where(np.isnan(v), np.inf, v)
    i = np.argmin(w, axis=1)
    return w[np.arange(len(w)), i], i


def best64(pred, gt, scale):
    """The float64 values of every per-agent output: a dict of ade_k / fde_k [n,K], ade / fde [n], ade_idx / fde_idx [n]."""
    ak, fk = per_sample(dist64(pred, gt, scale))
    (a, ia), (f, jf) = first_min(ak), first_min(fk)
    return {'ade_k': ak, 'fde_k': fk, 'ade': a, 'fde': f, 'ade_idx': ia, 'fde_idx': jf}


def horizon_from(d):
    """Distances [n,K,Tf] (float64) -> [n,Tf,2], the layout of sttode_horizon_metrics: (min_k of the running mean, min_k of frame h)."""
    run = np.cumsum(d, axis=-1) / np.arange(1, d.shape[-1] + 1)
    return np.stack([run.min(axis=1), d.min(axis=1)], axis=-1)


def horizon64(pred, gt, scale):
    return horizon_from(dist64(pred, gt, scale))


def clamp_csr(seg_ptr, n):
    """bok_segments_kernel's rule: [(a0, a1)] per segment, bounds clamped to [0, n] with a1 >= a0."""
    sp = [int(v) for v in seg_ptr]
    out = []
    for lo, hi in zip(sp[:-1], sp[1:]):
        a0 = min(max(lo, 0), n)
        out.append((a0, min(max(hi, a0), n)))
    return out


def segments64(ade, fde, seg_ptr, thr):
    """Per-agent ade / fde [n] (any float type, taken to float64) -> (seg_ade [S], seg_fde [S] float64 means, seg_miss [S] counts of
    fde > float32(thr)) over the clamped CSR; an empty segment gives NaN means and a zero count."""
    a64, f64 = np.asarray(ade, np.float64), np.asarray(fde, np.float64)
    t = np.float64(np.float32(thr))
    sa, sf, sm = [], [], []
    for a0, a1 in clamp_csr(seg_ptr, len(a64)):
        sa.append(a64[a0:a1].mean() if a1 > a0 else np.nan)
        sf.append(f64[a0:a1].mean() if a1 > a0 else np.nan)
        sm.append(int((f64[a0:a1] > t).sum()))
    return np.array(sa, np.float64), np.array(sf, np.float64), np.array(sm, np.int64)


# -------------------------------------------------------------------------------------------------------------------------------------
# float32, in the kernels' order: the measure of what a correct fp32 evaluation does
# -------------------------------------------------------------------------------------------------------------------------------------
def per_sample32(pred, gt, scale):
    """(ADE [n,K], FDE [n,K]) float32 as best_of_k_kernel / bok_select_kernel compute them: bok_dist (helpers.bok_dist_np), the frames added
    in frame order, the sum divided by float32(Tf)."""
    d = bok_dist_np(pred, gt, scale)
    s = np.zeros(d.shape[:2], np.float32)
    for t in range(d.shape[2]):
        s = (s + d[:, :, t]).astype(np.float32)
    return (s / np.float32(d.shape[2])).astype(np.float32), d[..., -1]


def best32(pred, gt, scale):
    ak, fk = per_sample32(pred, gt, scale)
    (a, ia), (f, jf) = first_min(ak), first_min(fk)
    return {'ade_k': ak, 'fde_k': fk, 'ade': a, 'fde': f, 'ade_idx': ia, 'fde_idx': jf}


def segments32(ade, fde, seg_ptr, thr):
    """bok_segments_kernel on float32 per-agent values: lane l adds agents a0 + l, a0 + l + 64, ... in order, the 64 partial sums go through
    the xor tree (offsets 32 .. 1), lane 0 divides by float32(a1 - a0).  -> (seg_ade, seg_fde float32 [S], seg_miss [S])."""
    ade, fde = np.asarray(ade, np.float32), np.asarray(fde, np.float32)
    lanes = np.arange(64)
    out = ([], [], [])
    for a0, a1 in clamp_csr(seg_ptr, len(ade)):
        for v, dst in ((ade, out[0]), (fde, out[1])):
            part = np.zeros(64, np.float32)
            for a in range(a0, a1):
                part[(a - a0) % 64] = part[(a - a0) % 64] + v[a]
            for o in (32, 16, 8, 4, 2, 1):
                part = (part + part[lanes ^ o]).astype(np.float32)
            with np.errstate(invalid='ignore', divide='ignore'):
                dst.append(part[0] / np.float32(a1 - a0))
        out[2].append(int((fde[a0:a1] > np.float32(thr)).sum()))
    return np.array(out[0], np.float32), np.array(out[1], np.float32), np.array(out[2], np.int64)


def units(got, ref):
    """|got - ref| / |ref| in units of u, elementwise; 0 where both are zero, inf where only ref is."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    with np.errstate(invalid='ignore', divide='ignore'):
        e = np.abs(got - ref) / (np.abs(ref) * U)
    return np.where(ref == 0, np.where(got == 0, 0.0, np.inf), e)
