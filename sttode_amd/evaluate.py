"""Caller-side evaluation loops over the HIP path (the reference's test.py flows, without plotting):

  eval_scenes  == test.py:163-208  (ETH/UCY/SDD): per scene set_data + inference, ADE/FDE best-of-K per agent,
                  AverageMeter weighted by agent_num  ==  plain mean over all agents of the per-agent minima.
                  Here many scenes go through ONE batched call (set_scene_batch) instead of a Python loop per scene.
  eval_nba     == test.py:495-552  (NBA): per DataLoader batch, min-over-K of the mean / final displacement at the horizons
                  1..future_length (the reference prints every 0.4 s step), weighted by batch size.
  eval_scenes_report / eval_sampler_report / eval_nba_report: the same loops returning an EvalReport -- global ADE / FDE and miss rate,
                  per-scene (per NBA batch) ADE / FDE / miss count, the best sample of every agent (utils/metrics.py:29-48); on request
                  the scene-level metrics of DESIGN.md 4l: joint min ADE / FDE, collision rates, KDE NLL; and the spread of the samples
                  among themselves of DESIGN.md 4s: APD / FPD, the DLow kernel value, energy scores, best-of-k.
  eval_scenes_reduced  oversample and reduce: `rounds` calls per scene batch, k-means of the rounds * sample_k futures of every
                  agent to K representatives on the device, then the selection of eval_scenes_report on the representatives.
  embedding_delta  how tree-like the encoder's past features (or the observed tracks) of a dataset are: delta / diam of hyptorch/delta.py's
                   batched_delta_hyp over all agents.
"""
import contextlib
import dataclasses

import numpy as np
import torch


@torch.no_grad()
def eval_scenes(model, dataset, traj_scale=1.0, scenes_per_call=512, z_fn=None, pipelined=True):
    """dataset: sttode_amd.datasets.TrajectoryDataset / SDD_Dataset (or anything with ``scene_batch(indices)``).
    Returns (ADE, FDE, n_agents).  ``z_fn(n_rows)`` may supply latents (tests); otherwise torch.randn like the reference.
    ``pipelined`` (default): the calls go through ``inference_async`` -- up to four in flight, best-of-K ADE / FDE computed by the calls' own
    trajectory groups (what bench.py times) -- instead of one serial ``inference()`` + ``best_of_k`` per batch."""
    tot_a = tot_f = 0.0
    tot_n = 0
    K, zd = model.args.sample_k, model.args.zdim
    pend = []

    def finish(h):
        nonlocal tot_a, tot_f
        ade, fde = model.best_of_k_async(h, scale=traj_scale)
        model.wait(h)
        tot_a += float(ade.double().sum())
        tot_f += float(fde.double().sum())
    for s0 in range(0, len(dataset), scenes_per_call):
        sb = dataset.scene_batch(range(s0, min(s0 + scenes_per_call, len(dataset))))
        model.set_scene_batch(sb.past, sb.future, sb.scene_ptr)
        rows = sb.n_agents * K
        z = z_fn(rows) if z_fn is not None else torch.randn(rows, zd, device=model.device)
        tot_n += sb.n_agents
        if pipelined:
            if len(model._async_bufs) > 12:                               # batches of ever new sizes: per-shape slot buffers are dropped in time
                while pend:
                    finish(pend.pop(0))
                model.reset_async()
            pend.append(model.inference_async(z=z, metrics_gt=model._future, metrics_scale=traj_scale))
            if len(pend) > 4:
                finish(pend.pop(0))
            continue
        pred = model.inference(None, z=z)                                  # [K, n, Tf, 2]
        ade, fde = model.best_of_k(pred.permute(1, 0, 2, 3), scale=traj_scale)
        tot_a += float(ade.double().sum())
        tot_f += float(fde.double().sum())
    while pend:
        finish(pend.pop(0))
    if pipelined:
        model.reset_async()
    return tot_a / tot_n, tot_f / tot_n, tot_n


@torch.no_grad()
def eval_sampler(model, sampler, dataset, traj_scale=1.0, scenes_per_call=512, mean=True, eps_fn=None, pipelined=True):
    """Stage-2 evaluation, test_sampler.py:117-212: the latents come from the sampler's Q-net (mean mode by default, as test_sampler.py:136),
    ADE / FDE best-of-K per agent weighted by agent count.  Returns (ADE, FDE, n_agents).  As eval_scenes: many scenes per call
    (``dataset.scene_batch``), and ``pipelined`` (default) runs the calls through ``sampler.inference_async`` -- several in flight, the metrics
    computed by the calls' own trajectory groups; ``pipelined=False``: one serial ``sampler.inference`` + ``best_of_k`` per batch.
    ``mean=False``: sampled latents, eps drawn like sampler.py:41-46 or by ``eps_fn(rows)`` (rows = 1 with share_eps, else the call's agents)."""
    tot_a = tot_f = 0.0
    tot_n = 0
    pend = []

    def finish(h):
        nonlocal tot_a, tot_f
        ade, fde = model.best_of_k_async(h, scale=traj_scale)
        model.wait(h)
        tot_a += float(ade.double().sum())
        tot_f += float(fde.double().sum())
    for s0 in range(0, len(dataset), scenes_per_call):
        sb = dataset.scene_batch(range(s0, min(s0 + scenes_per_call, len(dataset))))
        model.set_scene_batch(sb.past, sb.future, sb.scene_ptr)
        eps = None
        if not mean and eps_fn is not None:
            eps = eps_fn(1 if sampler.share_eps else sb.n_agents)
        tot_n += sb.n_agents
        if pipelined:
            if len(model._async_bufs) > 12:                               # batches of ever new sizes: per-shape slot buffers are dropped in time
                while pend:
                    finish(pend.pop(0))
                model.reset_async()
            pend.append(sampler.inference_async(model, mean=mean, eps=eps, metrics_gt=model._future, metrics_scale=traj_scale))
            if len(pend) > 4:
                finish(pend.pop(0))
            continue
        pred = sampler.inference(model, mean=mean, eps=eps)                 # [K, n, Tf, 2]
        ade, fde = model.best_of_k(pred.permute(1, 0, 2, 3), scale=traj_scale)
        tot_a += float(ade.double().sum())
        tot_f += float(fde.double().sum())
    while pend:
        finish(pend.pop(0))
    if pipelined:
        model.reset_async()
    return tot_a / tot_n, tot_f / tot_n, tot_n


@torch.no_grad()
def eval_nba(model, loader, traj_scale=1.0, z_fn=None, pipelined=True, groups_per_call=16):
    """loader yields seq_collate dicts (data/dataloader_nba.py:7-18).  Returns {h: (avg_h, dest_h)} for h = 1..Tf, each the
    batch-size-weighted mean over batches of mean_n min_k (test.py:530-551).
    ``pipelined`` (default): up to ``groups_per_call`` consecutive loader batches of equal shape travel as ONE call (set_data_nba with
    [G,B,N,...]: the attention stays within each batch, exactly what the reference's one call per batch computes) through ``inference_async``
    -- several calls in flight -- and the per-horizon min-over-K metric is one HIP kernel on the call's own stream
    (``horizon_metrics_async``); the host only adds up [Tf, 2] sums.  ``pipelined=False``: one serial ``inference()`` per loader batch and
    the metric as torch ops (the round-4 loop; kept as the cross-check of tests/test_gpu_parity.py)."""
    Tf, K = model.args.future_length, model.args.sample_k
    dev = model.device
    acc = np.zeros((Tf, 2))
    count = 0
    if not pipelined:
        for data in loader:
            model.set_data_nba(data)
            n = data['past_traj'].shape[0] * data['past_traj'].shape[1]
            z = z_fn(n * K) if z_fn is not None else None
            pred = model.inference(data, z=z) * traj_scale                     # [K, n, Tf, 2]
            gt = torch.as_tensor(data['future_traj'], dtype=torch.float32).to(pred.device).reshape(n, Tf, 2) * traj_scale
            d = (pred - gt[None]).norm(dim=-1)                                 # [K, n, Tf]
            cum = d.cumsum(dim=2) / torch.arange(1, Tf + 1, device=d.device)   # mean over the first h frames
            B = data['past_traj'].shape[0]
            acc[:, 0] += cum.min(dim=0)[0].mean(dim=0).double().cpu().numpy() * B
            acc[:, 1] += d.min(dim=0)[0].mean(dim=0).double().cpu().numpy() * B
            count += B
        acc /= count
        return {h + 1: (float(acc[h, 0]), float(acc[h, 1])) for h in range(Tf)}

    pend, totals = [], []

    def finish(item):
        h, hm, B, N, G = item
        model.wait(h)
        # mean over the agents of a batch, times its batch size, summed over the call's batches == sum over all agents / N
        totals.append(hm.double().sum(dim=0) / N)

    def submit(group):
        B, N = group[0]['past_traj'].shape[:2]
        G = len(group)
        past = torch.stack([torch.as_tensor(d['past_traj'], dtype=torch.float32) for d in group])
        fut = torch.stack([torch.as_tensor(d['future_traj'], dtype=torch.float32) for d in group])
        n = G * B * N
        model.packed()
        st = model.next_async_stream(n)
        with torch.cuda.stream(st) if st is not None else contextlib.nullcontext():
            model.set_data_nba({'past_traj': past.to(dev, non_blocking=True), 'future_traj': fut.to(dev, non_blocking=True)})
            # z_fn is asked once per LOADER batch (its rows: B N K), as the serial loop asks it; the call's latents are their concatenation
            z = torch.cat([torch.as_tensor(z_fn(B * N * K)).to(dev) for _ in group]) if z_fn is not None else None
            h = model.inference_async(z=z)
        hm = model.horizon_metrics_async(h, gt=model._future, scale=traj_scale)
        pend.append((h, hm, B, N, G))
        if len(pend) > 3:
            finish(pend.pop(0))

    group = []
    for data in loader:
        shape = tuple(data['past_traj'].shape)
        if group and (tuple(group[0]['past_traj'].shape) != shape or len(group) >= groups_per_call):
            submit(group)
            group = []
        group.append(data)
        count += shape[0]
    if group:
        submit(group)
    while pend:
        finish(pend.pop(0))
    model.reset_async()
    acc = torch.stack(totals).sum(dim=0).cpu().numpy() / count
    return {h + 1: (float(acc[h, 0]), float(acc[h, 1])) for h in range(Tf)}


# ----- report forms: per-scene results, best samples and miss rate (utils/metrics.py:29-48, test.py:193-205, test_sampler.py:214-217) ------

@dataclasses.dataclass
class EvalReport:
    """What the report loops return.  Global: ``ade`` / ``fde`` (mean over agents, the values eval_scenes / eval_sampler return),
    ``n_agents``, ``miss_count`` / ``miss_rate`` (agents whose best FDE exceeds ``miss_threshold``, count_miss_samples).  Per scene -- per
    loader batch for NBA -- in dataset order: ``scene_ade`` / ``scene_fde`` (compute_ADE / compute_FDE of that scene alone), ``scene_miss``
    (its miss count), ``scene_agents``.  Per agent in dataset order: ``best_idx`` (get_best_idx: the sample with the smallest ADE, the first
    on ties), ``best_fde_idx``, and with ``gather=True`` ``best`` [n, Tf, 2], the predictions of that sample (unscaled).

    Scene-level metrics, None unless asked; segments are scenes (NBA: games of N players), in dataset order.  ``joint=True``:
    ``joint_ade`` / ``joint_fde`` (mean over segments of the min over k of the segment's mean ADE / FDE of sample k), ``scene_joint_ade`` /
    ``scene_joint_fde`` [S] and ``scene_joint_idx`` [S] (the k of the joint ADE, the lowest on ties).  ``collision_radius=r``:
    ``collision_rate`` (colliding agent-samples / (K n)), ``gt_collision_rate`` (colliding agents of the ground truth / n) and
    ``scene_collision`` [S, 2] (per segment: colliding agent-samples, colliding ground-truth agents).  ``kde=True``: ``kde_nll`` (mean over
    the agents whose NLL is finite), ``kde_nll_agents`` [n] float64 (NaN where the samples' covariance is singular) and ``kde_invalid`` (the
    number of NaN agents).

    Spread of the samples among themselves, None unless ``spread=True``: ``apd`` / ``fpd`` / ``pade`` (mean over agents of the
    mean pairwise trajectory / final-frame / per-frame distance), ``dlow`` (mean over agents of the DLow kernel value at ``div_scale``:
    diversity_loss's loss_unweighted), ``energy_ade`` / ``energy_fde`` (mean energy score), all float64 sums over agents in dataset order;
    ``spread_agents`` [n, 6] float64 (the six values per agent, in that order); ``ade_at_k`` / ``fde_at_k``: a dict k -> mean over agents of
    the min ADE / FDE over the first k samples, for each k <= K of ``ks``."""
    ade: float
    fde: float
    n_agents: int
    miss_count: int
    miss_rate: float
    miss_threshold: float
    scene_ade: np.ndarray
    scene_fde: np.ndarray
    scene_miss: np.ndarray
    scene_agents: np.ndarray
    best_idx: np.ndarray
    best_fde_idx: np.ndarray
    best: np.ndarray = None
    joint_ade: float = None
    joint_fde: float = None
    scene_joint_ade: np.ndarray = None
    scene_joint_fde: np.ndarray = None
    scene_joint_idx: np.ndarray = None
    collision_radius: float = None
    collision_rate: float = None
    gt_collision_rate: float = None
    scene_collision: np.ndarray = None
    kde_nll: float = None
    kde_nll_agents: np.ndarray = None
    kde_invalid: int = None
    apd: float = None
    fpd: float = None
    pade: float = None
    dlow: float = None
    energy_ade: float = None
    energy_fde: float = None
    spread_agents: np.ndarray = None
    ade_at_k: dict = None
    fde_at_k: dict = None


class _ReportAcc:
    """Host side of a report loop: per call, the same double sums eval_scenes forms (so the global ADE / FDE agree bit for bit), and the
    small per-scene / per-agent arrays."""

    def __init__(self, miss_threshold, joint=False, kde=False, collision_radius=None, K=None, spread=False, div_scale=None, ks=(1, 5, 10),
                 dataset=None):
        from .metrics import check_radius, check_spread
        self.thr = float(miss_threshold)
        self.tot_a = self.tot_f = 0.0
        self.n = 0
        self.parts = []
        self.joint, self.kde, self.radius, self.K = bool(joint), bool(kde), check_radius(collision_radius), K
        self.jparts, self.kparts = [], []
        self.spread = bool(spread)
        if self.spread:
            if div_scale is None:
                from .samplerloss import get_diversity_config
                div_scale = get_diversity_config(dataset)['scale'] if dataset is not None else 1.0
            self.div_scale = check_spread(K, div_scale)
            self.ks = [int(k) for k in ks if 1 <= int(k) <= K]
            self.sparts = []

    @property
    def scene_metrics(self):
        """Whether a joint pass runs (for the joint values, the collision counts or both)."""
        return self.joint or self.radius is not None

    def add_spread(self, ss):
        cols = torch.tensor([k - 1 for k in self.ks], dtype=torch.long, device=ss.apd.device)
        self.sparts.append((torch.stack([ss.apd, ss.fpd, ss.pade, ss.dlow, ss.es_ade, ss.es_fde], dim=1).cpu().numpy(),
                            ss.ade_at_k[:, cols].cpu().numpy(), ss.fde_at_k[:, cols].cpu().numpy()))

    def add_scene_metrics(self, js, kd, ss=None):
        if ss is not None:
            self.add_spread(ss)
        if js is not None:
            self.jparts.append((js.seg_jade.cpu().numpy(), js.seg_jfde.cpu().numpy(), js.seg_jade_idx.cpu().numpy(),
                                None if js.seg_col is None else torch.stack([js.seg_col, js.seg_gt_col], dim=1).cpu().numpy()))
        if kd is not None:
            self.kparts.append(kd.cpu().numpy())

    def add(self, sel, seg_ptr):
        self.tot_a += float(sel.ade.double().sum())
        self.tot_f += float(sel.fde.double().sum())
        self.n += int(sel.ade.numel())
        sp = seg_ptr.cpu().numpy() if isinstance(seg_ptr, torch.Tensor) else np.asarray(seg_ptr)
        self.parts.append((sel.seg_ade.cpu().numpy(), sel.seg_fde.cpu().numpy(), sel.seg_miss.cpu().numpy(), np.diff(sp),
                           sel.best_ade_idx.cpu().numpy(), sel.best_fde_idx.cpu().numpy(), None if sel.best is None else sel.best.cpu().numpy()))

    def report(self, gather):
        cat = [np.concatenate([p[i] for p in self.parts]) for i in range(6)]
        miss = int(cat[2].sum())
        rep = EvalReport(ade=self.tot_a / self.n, fde=self.tot_f / self.n, n_agents=self.n, miss_count=miss, miss_rate=miss / self.n,
                         miss_threshold=self.thr, scene_ade=cat[0], scene_fde=cat[1], scene_miss=cat[2], scene_agents=cat[3].astype(np.int64),
                         best_idx=cat[4], best_fde_idx=cat[5], best=np.concatenate([p[6] for p in self.parts]) if gather else None)
        if self.joint:
            rep.scene_joint_ade, rep.scene_joint_fde, rep.scene_joint_idx = (np.concatenate([p[i] for p in self.jparts]) for i in range(3))
            rep.joint_ade = float(rep.scene_joint_ade.astype(np.float64).mean())
            rep.joint_fde = float(rep.scene_joint_fde.astype(np.float64).mean())
        if self.radius is not None:
            col = np.concatenate([p[3] for p in self.jparts]).astype(np.int64)
            rep.collision_radius, rep.scene_collision = self.radius, col
            rep.collision_rate = int(col[:, 0].sum()) / (self.K * self.n)
            rep.gt_collision_rate = int(col[:, 1].sum()) / self.n
        if self.kde:
            v = np.concatenate(self.kparts)
            ok = np.isfinite(v)
            rep.kde_nll_agents, rep.kde_invalid = v, int((~ok).sum())
            rep.kde_nll = float(v[ok].mean()) if ok.any() else float('nan')
        if self.spread:
            v, ak, fk = (np.concatenate([p[i] for p in self.sparts]) for i in range(3))
            rep.spread_agents = v
            rep.apd, rep.fpd, rep.pade, rep.dlow, rep.energy_ade, rep.energy_fde = (float(x) for x in v.sum(axis=0) / v.shape[0])
            rep.ade_at_k = {k: float(ak[:, i].astype(np.float64).sum() / ak.shape[0]) for i, k in enumerate(self.ks)}
            rep.fde_at_k = {k: float(fk[:, i].astype(np.float64).sum() / fk.shape[0]) for i, k in enumerate(self.ks)}
        return rep


def _scenes_report(model, dataset, scenes_per_call, pipelined, traj_scale, miss_threshold, gather, launch, serial, joint, kde,
                   collision_radius, spread=False, div_scale=None, ks=(1, 5, 10)):
    acc = _ReportAcc(miss_threshold, joint, kde, collision_radius, model.args.sample_k, spread, div_scale, ks,
                     getattr(model.args, 'dataset', None))
    pend = []

    def finish(item):
        h, sel, sp, js, kd, ss = item
        model.wait(h)
        acc.add(sel, sp)
        acc.add_scene_metrics(js, kd, ss)
    for s0 in range(0, len(dataset), scenes_per_call):
        sb = dataset.scene_batch(range(s0, min(s0 + scenes_per_call, len(dataset))))
        model.set_scene_batch(sb.past, sb.future, sb.scene_ptr)
        if pipelined:
            if len(model._async_bufs) > 12:                               # batches of ever new sizes: per-shape slot buffers are dropped in time
                while pend:
                    finish(pend.pop(0))
                model.reset_async()
            h = launch(sb)
            sel = model.select_best_of_k_async(h, scale=traj_scale, miss_threshold=miss_threshold, seg_ptr='scenes', gather=gather)
            js = model.select_joint_async(h, seg_ptr='scenes', scale=traj_scale, collision_radius=acc.radius) if acc.scene_metrics else None
            kd = model.kde_nll_async(h, scale=traj_scale) if kde else None
            ss = model.sample_spread_async(h, scale=traj_scale, div_scale=acc.div_scale) if spread else None
            pend.append((h, sel, sb.scene_ptr, js, kd, ss))
            if len(pend) > 4:
                finish(pend.pop(0))
            continue
        pred = serial(sb)                                                  # [K, n, Tf, 2]
        sel = model.select_best_of_k(pred.permute(1, 0, 2, 3), scale=traj_scale, miss_threshold=miss_threshold, seg_ptr=model._scene_ptr,
                                     gather=gather)
        acc.add(sel, sb.scene_ptr)
        if acc.scene_metrics or kde or spread:
            pnk = pred.permute(1, 0, 2, 3).contiguous()
            acc.add_scene_metrics(model.select_joint(pnk, seg_ptr=model._scene_ptr, scale=traj_scale, collision_radius=acc.radius)
                                  if acc.scene_metrics else None, model.kde_nll(pnk, scale=traj_scale) if kde else None,
                                  model.sample_spread(pnk, scale=traj_scale, div_scale=acc.div_scale) if spread else None)
    while pend:
        finish(pend.pop(0))
    if pipelined:
        model.reset_async()
    return acc.report(gather)


@torch.no_grad()
def eval_scenes_report(model, dataset, traj_scale=1.0, scenes_per_call=512, z_fn=None, pipelined=True, miss_threshold=1.0, gather=False,
                       joint=False, kde=False, collision_radius=None, spread=False, div_scale=None, ks=(1, 5, 10)):
    """eval_scenes with the per-scene breakdown, the best sample of every agent and the miss rate (an ``EvalReport``).  The same calls, latents
    and global ADE / FDE as eval_scenes; each call adds one selection pass on its own pipeline stream (``select_best_of_k_async``).
    ``joint`` / ``collision_radius`` / ``kde`` add the scene-level passes (``select_joint_async``, ``kde_nll_async``; after the serial call
    with ``pipelined=False``); every other field is the same with them on or off.  ``spread`` adds the spread pass (``sample_spread_async``:
    APD / FPD, the DLow kernel value at ``div_scale`` -- default: the scale of samplerloss.get_diversity_config for the model's dataset -- the
    energy scores and best-of-k for each k of ``ks``) in the same way."""
    K, zd = model.args.sample_k, model.args.zdim

    def latents(sb):
        rows = sb.n_agents * K
        return z_fn(rows) if z_fn is not None else torch.randn(rows, zd, device=model.device)
    return _scenes_report(model, dataset, scenes_per_call, pipelined, traj_scale, miss_threshold, gather,
                          lambda sb: model.inference_async(z=latents(sb), metrics_gt=model._future, metrics_scale=traj_scale),
                          lambda sb: model.inference(None, z=latents(sb)), joint, kde, collision_radius, spread, div_scale, ks)


@torch.no_grad()
def eval_scenes_reduced(model, dataset, rounds, K=None, iters=10, from_frame=0, init='first', traj_scale=1.0, scenes_per_call=512, z_fn=None,
                        pipelined=True, miss_threshold=1.0, spread=False, div_scale=None, ks=(1, 5, 10)):
    """Oversample and reduce as an evaluation loop: per scene batch ``rounds`` inference calls -- M = rounds * sample_k futures
    per agent -- reduced to ``K`` (default sample_k) representatives per agent by ``metrics.reduce_samples`` (``iters``, ``from_frame``,
    ``init`` as there), and the best-of-K selection of eval_scenes_report on the representatives.  Returns an ``EvalReport``.
    ``z_fn(rows)`` is asked once per round, in round order.  ``pipelined`` (default): the rounds go through ``inference_async``, never more
    in flight than ``async_depth`` allows; each is waited for and copied into the round buffer before its slot is taken again.  The reduction
    and the selection run on the caller's stream.  The two forms' samples differ by fp32 rounding (as inference_async and inference do), so
    with rounds > 1 a near-tied label may legitimately differ between them.  ``spread`` / ``div_scale`` / ``ks`` as eval_scenes_report, on the
    representatives: what the reduction does to the diversity of the set."""
    from . import metrics
    rounds = int(rounds)
    if rounds < 1:
        raise ValueError(f'eval_scenes_reduced needs rounds >= 1, got {rounds}')
    Ks, zd = model.args.sample_k, model.args.zdim
    K = Ks if K is None else int(K)
    acc = _ReportAcc(miss_threshold, K=K, spread=spread, div_scale=div_scale, ks=ks, dataset=getattr(model.args, 'dataset', None))
    depth = max(2, min(8, int(model.async_depth)))
    for s0 in range(0, len(dataset), scenes_per_call):
        sb = dataset.scene_batch(range(s0, min(s0 + scenes_per_call, len(dataset))))
        model.set_scene_batch(sb.past, sb.future, sb.scene_ptr)
        rows = sb.n_agents * Ks
        buf = model._round_buffer(rounds, sb.n_agents)
        if pipelined:
            new = sum((sb.n_agents, model._S, s) not in model._async_bufs for s in range(depth))
            if len(model._async_bufs) + new > 16:                         # batches of ever new sizes: per-shape slot buffers are dropped in time
                model.reset_async()                                       # (nothing is in flight between batches)
            pend = []

            def finish(item):
                r, h = item
                buf[r].copy_(model.wait(h).permute(1, 0, 2, 3))             # [n, sample_k, Tf, 2], on the caller's stream: in front of the slot's next call
            for r in range(rounds):
                if len(pend) >= depth - 1:
                    finish(pend.pop(0))
                z = z_fn(rows) if z_fn is not None else torch.randn(rows, zd, device=model.device)
                pend.append((r, model.inference_async(z=z)))
            while pend:
                finish(pend.pop(0))
        else:
            for r in range(rounds):
                z = z_fn(rows) if z_fn is not None else torch.randn(rows, zd, device=model.device)
                buf[r].copy_(model.inference(None, z=z).permute(1, 0, 2, 3))
        red = metrics.reduce_samples(buf, K, iters=iters, from_frame=from_frame, init=init)
        acc.add(model.select_best_of_k(red.centroids, scale=traj_scale, miss_threshold=miss_threshold, seg_ptr=model._scene_ptr), sb.scene_ptr)
        if spread:
            acc.add_spread(model.sample_spread(red.centroids, scale=traj_scale, div_scale=acc.div_scale))
    if pipelined:
        model.reset_async()
    return acc.report(False)


@torch.no_grad()
def eval_sampler_report(model, sampler, dataset, traj_scale=1.0, scenes_per_call=512, mean=True, eps_fn=None, pipelined=True,
                        miss_threshold=1.0, gather=False, joint=False, kde=False, collision_radius=None, spread=False, div_scale=None,
                        ks=(1, 5, 10)):
    """eval_sampler with the per-scene breakdown, the best sample of every agent and the miss rate (an ``EvalReport``; test_sampler.py:214-217
    asks count_miss_samples of the same loop).  ``joint`` / ``collision_radius`` / ``kde`` / ``spread`` / ``div_scale`` / ``ks`` as
    eval_scenes_report."""
    def eps_of(sb):
        return eps_fn(1 if sampler.share_eps else sb.n_agents) if (not mean and eps_fn is not None) else None
    return _scenes_report(model, dataset, scenes_per_call, pipelined, traj_scale, miss_threshold, gather,
                          lambda sb: sampler.inference_async(model, mean=mean, eps=eps_of(sb), metrics_gt=model._future,
                                                             metrics_scale=traj_scale),
                          lambda sb: sampler.inference(model, mean=mean, eps=eps_of(sb)), joint, kde, collision_radius, spread, div_scale, ks)


@torch.no_grad()
def eval_nba_report(model, loader, traj_scale=1.0, z_fn=None, pipelined=True, groups_per_call=16, miss_threshold=1.0, gather=False,
                    joint=False, kde=False, collision_radius=None, spread=False, div_scale=None, ks=(1, 5, 10)):
    """NBA evaluation (test.py:495-552) as an ``EvalReport``: ADE / FDE over the whole horizon (the last horizon of eval_nba), the miss rate,
    per loader batch its ADE / FDE / miss count, the best sample of every agent.  Calls as eval_nba: up to ``groups_per_call`` loader batches
    of one shape per call, several in flight, the selection on each call's pipeline stream with one segment per loader batch.
    ``joint`` / ``collision_radius`` / ``kde`` / ``spread`` / ``div_scale`` / ``ks`` as eval_scenes_report; the joint and collision segments
    are games (N players each)."""
    Tf, K = model.args.future_length, model.args.sample_k
    dev = model.device
    acc = _ReportAcc(miss_threshold, joint, kde, collision_radius, K, spread, div_scale, ks, getattr(model.args, 'dataset', 'nba'))
    if not pipelined:
        for data in loader:
            model.set_data_nba(data)
            n = data['past_traj'].shape[0] * data['past_traj'].shape[1]
            z = z_fn(n * K) if z_fn is not None else None
            pred = model.inference(data, z=z)                                   # [K, n, Tf, 2]
            sp = np.array([0, n], dtype=np.int32)
            acc.add(model.select_best_of_k(pred.permute(1, 0, 2, 3), scale=traj_scale, miss_threshold=miss_threshold, seg_ptr=sp,
                                           gather=gather), sp)
            if acc.scene_metrics or kde or spread:
                pnk = pred.permute(1, 0, 2, 3).contiguous()
                games = np.arange(0, n + 1, data['past_traj'].shape[1], dtype=np.int32)
                acc.add_scene_metrics(model.select_joint(pnk, seg_ptr=games, scale=traj_scale, collision_radius=acc.radius)
                                      if acc.scene_metrics else None, model.kde_nll(pnk, scale=traj_scale) if kde else None,
                                      model.sample_spread(pnk, scale=traj_scale, div_scale=acc.div_scale) if spread else None)
        return acc.report(gather)

    pend = []
    seg_ptrs = {}

    def finish(item):
        h, sel, sp, js, kd, ss = item
        model.wait(h)
        acc.add(sel, sp)
        acc.add_scene_metrics(js, kd, ss)

    def submit(group):
        B, N = group[0]['past_traj'].shape[:2]
        G = len(group)
        past = torch.stack([torch.as_tensor(d['past_traj'], dtype=torch.float32) for d in group])
        fut = torch.stack([torch.as_tensor(d['future_traj'], dtype=torch.float32) for d in group])
        n = G * B * N
        if (G, B * N) not in seg_ptrs:                                     # one segment per loader batch, complete before any stream reads it
            seg_ptrs[(G, B * N)] = torch.arange(0, n + 1, B * N, dtype=torch.int32, device=dev)
            torch.cuda.current_stream(dev).synchronize()
        sp = seg_ptrs[(G, B * N)]
        if acc.scene_metrics and ('games', G * B, N) not in seg_ptrs:                # one segment per game
            seg_ptrs[('games', G * B, N)] = torch.arange(0, n + 1, N, dtype=torch.int32, device=dev)
            torch.cuda.current_stream(dev).synchronize()
        model.packed()
        st = model.next_async_stream(n)
        with torch.cuda.stream(st) if st is not None else contextlib.nullcontext():
            model.set_data_nba({'past_traj': past.to(dev, non_blocking=True), 'future_traj': fut.to(dev, non_blocking=True)})
            z = torch.cat([torch.as_tensor(z_fn(B * N * K)).to(dev) for _ in group]) if z_fn is not None else None
            h = model.inference_async(z=z)
        sel = model.select_best_of_k_async(h, gt=model._future, scale=traj_scale, miss_threshold=miss_threshold, seg_ptr=sp, gather=gather)
        js = (model.select_joint_async(h, gt=model._future, seg_ptr=seg_ptrs[('games', G * B, N)], scale=traj_scale, collision_radius=acc.radius)
              if acc.scene_metrics else None)
        kd = model.kde_nll_async(h, gt=model._future, scale=traj_scale) if kde else None
        ss = model.sample_spread_async(h, gt=model._future, scale=traj_scale, div_scale=acc.div_scale) if spread else None
        pend.append((h, sel, np.arange(0, n + 1, B * N), js, kd, ss))
        if len(pend) > 3:
            finish(pend.pop(0))

    group = []
    for data in loader:
        shape = tuple(data['past_traj'].shape)
        if group and (tuple(group[0]['past_traj'].shape) != shape or len(group) >= groups_per_call):
            submit(group)
            group = []
        group.append(data)
    if group:
        submit(group)
    while pend:
        finish(pend.pop(0))
    model.reset_async()
    return acc.report(gather)


@torch.no_grad()
def embedding_delta(model, source, n_tries=10, batch_size=1500, scenes_per_call=512, what='past_feature', metric='euclidean'):
    """Gromov delta / diam (sttode_amd.delta.batched_delta_hyp) of one row per agent of a dataset; returns (mean, std) as np.float64.
    ``source``: a scene dataset (``scene_batch(indices)``, as eval_scenes takes), ``scenes_per_call`` scenes per set_scene_batch, or an NBA
    loader of seq_collate dicts (as eval_nba takes), one set_data_nba per batch.  Rows, gathered on the device in dataset order:
    ``what='past_feature'`` -- encode_history()'s [n, 128] encoder output (model/STTODE.py:488-496); ``'past_traj'`` -- the observed track
    relative to the current location, [n, 2 Tp].  The samples are drawn from numpy's global RNG as batched_delta_hyp draws them."""
    from .delta import batched_delta_hyp
    if what not in ('past_feature', 'past_traj'):
        raise ValueError(f"embedding_delta: what must be 'past_feature' or 'past_traj', got {what!r}")
    rows = []

    def take():
        pf = model.encode_history()
        if what == 'past_feature':
            rows.append(pf.clone())                                       # a view into the model's workspace: the next batch overwrites it
        else:
            rows.append((model.past_traj - model.cur_location).reshape(model.past_traj.shape[0], -1).contiguous())
    if hasattr(source, 'scene_batch'):
        for s0 in range(0, len(source), scenes_per_call):
            sb = source.scene_batch(range(s0, min(s0 + scenes_per_call, len(source))))
            model.set_scene_batch(sb.past, sb.future, sb.scene_ptr)
            take()
    else:
        for data in source:
            model.set_data_nba(data)
            take()
    if not rows:
        raise ValueError('embedding_delta: the source yielded no agents')
    return batched_delta_hyp(torch.cat(rows), n_tries=n_tries, batch_size=batch_size, metric=metric)
