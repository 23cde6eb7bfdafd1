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
                  agent to K representatives on the device, then the selection of eval_scenes_report on the representatives; with
                  level='scene'  k-means of every scene's futures as whole scene futures, and on request the joint,
                  collision and KDE passes on the representatives of either level.
  eval_scenes_reduced_raw  the same loop that also scores the raw set the representatives are cut from: best-of-M with its
                  prefixes, joint best-of-M, KDE NLL and the pair statistics over all M = rounds * sample_k <= 4096 samples per agent.
  eval_scenes_multimodal  MMADE / MMFDE: the samples of the whole dataset gathered on the device, then one pass that scores every
                  agent's samples against the futures of all agents with a similar history.
  embedding_delta  how tree-like the encoder's past features (or the observed tracks) of a dataset are: delta / diam of hyptorch/delta.py's
                   batched_delta_hyp over all agents.
"""
import collections
import contextlib
import dataclasses

import numpy as np
import torch


def _latents(model, rows, z_fn):
    return z_fn(rows) if z_fn is not None else torch.randn(rows, model.args.zdim, device=model.device)


def _scene_loop(model, dataset, scenes_per_call, pipelined, launch, finish, serial):
    """The loop over scene batches of every scene evaluation: ``scenes_per_call`` scenes per set_scene_batch.  Pipelined: ``launch(sb)``
    enqueues the batch's call (and what follows it on the call's stream) and returns what ``finish`` takes once more than four calls are in
    flight, and at the end.  Else ``serial(sb)`` does the whole batch."""
    pend = []

    def drain():
        while pend:
            finish(pend.pop(0))
    for s0 in range(0, len(dataset), scenes_per_call):
        sb = dataset.scene_batch(range(s0, min(s0 + scenes_per_call, len(dataset))))
        model.set_scene_batch(sb.past, sb.future, sb.scene_ptr)
        if not pipelined:
            serial(sb)
            continue
        if model._async_shapes() > 12:                                    # batches of ever new sizes: per-shape slot buffers are dropped in time
            drain()
            model.reset_async()
        pend.append(launch(sb))
        if len(pend) > 4:
            finish(pend.pop(0))
    drain()
    if pipelined:
        model.reset_async()


def _scenes_best_of_k(model, dataset, traj_scale, scenes_per_call, pipelined, launch, serial):
    tot_a = tot_f = 0.0
    tot_n = 0

    def add(ade, fde):
        nonlocal tot_a, tot_f, tot_n
        tot_a += float(ade.double().sum())
        tot_f += float(fde.double().sum())
        tot_n += int(ade.numel())

    def finish(h):
        ade, fde = model.best_of_k_async(h, scale=traj_scale)
        model.wait(h)
        add(ade, fde)
    _scene_loop(model, dataset, scenes_per_call, pipelined, launch, finish,
                lambda sb: add(*model.best_of_k(serial(sb).permute(1, 0, 2, 3), scale=traj_scale)))     # serial(sb): [K, n, Tf, 2]
    return tot_a / tot_n, tot_f / tot_n, tot_n


def _scene_calls(model, traj_scale, z_fn):
    """(launch, serial) of a scene batch on latents from z_fn / torch.randn."""
    def z(sb):
        return _latents(model, sb.n_agents * model.args.sample_k, z_fn)
    return (lambda sb: model.inference_async(z=z(sb), metrics_gt=model._future, metrics_scale=traj_scale),
            lambda sb: model.inference(None, z=z(sb)))


def _sampler_calls(model, sampler, traj_scale, mean, eps_fn):
    """(launch, serial) of a scene batch on the stage-2 sampler's latents."""
    def eps(sb):
        return eps_fn(1 if sampler.share_eps else sb.n_agents) if (not mean and eps_fn is not None) else None
    return (lambda sb: sampler.inference_async(model, mean=mean, eps=eps(sb), metrics_gt=model._future, metrics_scale=traj_scale),
            lambda sb: sampler.inference(model, mean=mean, eps=eps(sb)))


@torch.no_grad()
def eval_scenes(model, dataset, traj_scale=1.0, scenes_per_call=512, z_fn=None, pipelined=True):
    """dataset: sttode_amd.datasets.TrajectoryDataset / SDD_Dataset (or anything with ``scene_batch(indices)``).
    Returns (ADE, FDE, n_agents).  ``z_fn(n_rows)`` may supply latents (tests); otherwise torch.randn like the reference.
    ``pipelined`` (default): the calls go through ``inference_async`` -- up to four in flight, best-of-K ADE / FDE computed by the calls' own
    trajectory groups (what bench.py times) -- instead of one serial ``inference()`` + ``best_of_k`` per batch."""
    return _scenes_best_of_k(model, dataset, traj_scale, scenes_per_call, pipelined, *_scene_calls(model, traj_scale, z_fn))


@torch.no_grad()
def eval_sampler(model, sampler, dataset, traj_scale=1.0, scenes_per_call=512, mean=True, eps_fn=None, pipelined=True):
    """Stage-2 evaluation, test_sampler.py:117-212: the latents come from the sampler's Q-net (mean mode by default, as test_sampler.py:136),
    ADE / FDE best-of-K per agent weighted by agent count.  Returns (ADE, FDE, n_agents).  As eval_scenes: many scenes per call
    (``dataset.scene_batch``), and ``pipelined`` (default) runs the calls through ``sampler.inference_async`` -- several in flight, the metrics
    computed by the calls' own trajectory groups; ``pipelined=False``: one serial ``sampler.inference`` + ``best_of_k`` per batch.
    ``mean=False``: sampled latents, eps drawn like sampler.py:41-46 or by ``eps_fn(rows)`` (rows = 1 with share_eps, else the call's agents)."""
    return _scenes_best_of_k(model, dataset, traj_scale, scenes_per_call, pipelined, *_sampler_calls(model, sampler, traj_scale, mean, eps_fn))


def _nba_loop(model, loader, z_fn, groups_per_call, follow, finish):
    """The pipelined loop over an NBA loader: up to ``groups_per_call`` consecutive loader batches of equal shape travel as ONE call
    (set_data_nba with [G,B,N,...]), staged on the pipeline stream the call will run on.  ``follow(h, G, B, N)`` enqueues what follows the
    call on that stream and returns what ``finish`` takes once more than three calls are in flight, and at the end."""
    K, dev = model.args.sample_k, model.device
    pend = []

    def submit(group):
        B, N = group[0]['past_traj'].shape[:2]
        past = torch.stack([torch.as_tensor(d['past_traj'], dtype=torch.float32) for d in group])
        fut = torch.stack([torch.as_tensor(d['future_traj'], dtype=torch.float32) for d in group])
        model.packed()
        st = model.next_async_stream(len(group) * B * N)
        with torch.cuda.stream(st) if st is not None else contextlib.nullcontext():
            model.set_data_nba({'past_traj': past.to(dev, non_blocking=True), 'future_traj': fut.to(dev, non_blocking=True)})
            # z_fn is asked once per LOADER batch (its rows: B N K), as the serial loop asks it; the call's latents are their concatenation
            z = torch.cat([torch.as_tensor(z_fn(B * N * K)).to(dev) for _ in group]) if z_fn is not None else None
            h = model.inference_async(z=z)
        pend.append(follow(h, len(group), B, N))
        if len(pend) > 3:
            finish(pend.pop(0))
    group = []
    for data in loader:
        if group and (group[0]['past_traj'].shape != data['past_traj'].shape or len(group) >= groups_per_call):
            submit(group)
            group = []
        group.append(data)
    if group:
        submit(group)
    while pend:
        finish(pend.pop(0))
    model.reset_async()


@torch.no_grad()
def eval_nba(model, loader, traj_scale=1.0, z_fn=None, pipelined=True, groups_per_call=16):
    """loader yields seq_collate dicts (data/dataloader_nba.py:7-18).  Returns {h: (avg_h, dest_h)} for h = 1..Tf, each the
    batch-size-weighted mean over batches of mean_n min_k (test.py:530-551).
    ``pipelined`` (default): up to ``groups_per_call`` consecutive loader batches of equal shape travel as ONE call (set_data_nba with
    [G,B,N,...]: the attention stays within each batch, exactly what the reference's one call per batch computes) through ``inference_async``
    -- several calls in flight -- and the per-horizon min-over-K metric is one HIP kernel on the call's own stream
    (``horizon_metrics_async``); the host only adds up [Tf, 2] sums.  ``pipelined=False``: one serial ``inference()`` per loader batch and
    the metric as torch ops (the plain per-batch loop; kept as the cross-check of tests/test_gpu_parity.py)."""
    Tf, K = model.args.future_length, model.args.sample_k
    count = 0
    if not pipelined:
        acc = np.zeros((Tf, 2))
        for data in loader:
            model.set_data_nba(data)
            B = data['past_traj'].shape[0]
            n = B * data['past_traj'].shape[1]
            z = z_fn(n * K) if z_fn is not None else None
            pred = model.inference(data, z=z) * traj_scale                     # [K, n, Tf, 2]
            gt = torch.as_tensor(data['future_traj'], dtype=torch.float32).to(pred.device).reshape(n, Tf, 2) * traj_scale
            d = (pred - gt[None]).norm(dim=-1)                                 # [K, n, Tf]
            cum = d.cumsum(dim=2) / torch.arange(1, Tf + 1, device=d.device)   # mean over the first h frames
            acc[:, 0] += cum.min(dim=0)[0].mean(dim=0).double().cpu().numpy() * B
            acc[:, 1] += d.min(dim=0)[0].mean(dim=0).double().cpu().numpy() * B
            count += B
        acc /= count
    else:
        totals = []

        def follow(h, G, B, N):
            nonlocal count
            count += G * B
            return h, model.horizon_metrics_async(h, gt=model._future, scale=traj_scale), N

        def finish(item):
            h, hm, N = item
            model.wait(h)
            # mean over the agents of a batch, times its batch size, summed over the call's batches == sum over all agents / N
            totals.append(hm.double().sum(dim=0) / N)
        _nba_loop(model, loader, z_fn, groups_per_call, follow, finish)
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
    the min ADE / FDE over the first k samples, for each k <= K of ``ks``.

    The samples as a weighted set, None unless ``weighted=True`` (eval_scenes_reduced: the centroids with the clusters'
    shares as weights): ``w_kde_nll`` (KDE NLL under the weighted mixture), ``w_es_ade`` / ``w_es_fde`` (energy scores), ``w_apd`` / ``w_fpd``
    (expected distance between two different draws), ``eade`` / ``efde`` (expected ADE / FDE), ``brier_ade`` / ``brier_fde``, ``mean_neff`` --
    each the mean over the agents whose value is finite, as ``kde_nll`` -- ``w_kde_invalid`` (agents whose weighted KDE NLL is NaN),
    ``weighted_agents`` [n, 10] float64 (per agent: eade, efde, es_ade, es_fde, apd, fpd, kde_nll, brier_ade, brier_fde, neff) and
    ``ade_top_k`` / ``fde_top_k``: a dict k -> mean over agents of the min ADE / FDE over the k most probable samples, for k = 1 and each
    k <= K of ``ks``.

    The raw oversampled set, None unless eval_scenes_reduced_raw ran: the M = rounds * sample_k samples the representatives
    were cut from, scored by ``score_samples``.  ``raw_m`` = M; ``raw_ade`` / ``raw_fde`` (mean over agents of best-of-M: the oracle bound of
    any reduction), ``raw_miss_rate``; ``raw_ade_at_k`` / ``raw_fde_at_k``: a dict k -> mean over agents of the minimum over the first k
    samples, for k = sample_k and each k <= M of ``ks``; with ``joint``: ``raw_joint_ade`` / ``raw_joint_fde`` (mean over scenes of joint
    best-of-M); with ``kde``: ``raw_kde_nll`` (mean over the finite agents) and ``raw_kde_invalid``; with ``spread``: ``raw_apd`` /
    ``raw_fpd`` / ``raw_pade`` / ``raw_dlow`` / ``raw_energy_ade`` / ``raw_energy_fde`` (means over agents, as the fields without the
    prefix)."""
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
    w_kde_nll: float = None
    w_kde_invalid: int = None
    w_es_ade: float = None
    w_es_fde: float = None
    w_apd: float = None
    w_fpd: float = None
    eade: float = None
    efde: float = None
    brier_ade: float = None
    brier_fde: float = None
    ade_top_k: dict = None
    fde_top_k: dict = None
    mean_neff: float = None
    weighted_agents: np.ndarray = None
    raw_m: int = None
    raw_ade: float = None
    raw_fde: float = None
    raw_miss_rate: float = None
    raw_ade_at_k: dict = None
    raw_fde_at_k: dict = None
    raw_joint_ade: float = None
    raw_joint_fde: float = None
    raw_kde_nll: float = None
    raw_kde_invalid: int = None
    raw_apd: float = None
    raw_fpd: float = None
    raw_pade: float = None
    raw_dlow: float = None
    raw_energy_ade: float = None
    raw_energy_fde: float = None
    apd: float = None
    fpd: float = None
    pade: float = None
    dlow: float = None
    energy_ade: float = None
    energy_fde: float = None
    spread_agents: np.ndarray = None
    ade_at_k: dict = None
    fde_at_k: dict = None


def _np(t):
    return t.cpu().numpy() if isinstance(t, torch.Tensor) else t


class _ReportAcc:
    """Host side of a report loop: per call, the same double sums eval_scenes forms (so the global ADE / FDE agree bit for bit), and the
    small per-scene / per-agent arrays, kept per call under the name of the EvalReport field they become."""

    def __init__(self, miss_threshold, joint=False, kde=False, collision_radius=None, K=None, spread=False, div_scale=None, ks=(1, 5, 10),
                 dataset=None, weighted=False):
        from .metrics import check_radius, check_spread
        self.thr = float(miss_threshold)
        self.tot_a = self.tot_f = 0.0
        self.n = 0
        self.parts = collections.defaultdict(list)
        self.joint, self.kde, self.radius, self.K = bool(joint), bool(kde), check_radius(collision_radius), K
        self.spread, self.div_scale = bool(spread), None
        if self.spread:
            if div_scale is None:
                from .samplerloss import get_diversity_config
                div_scale = get_diversity_config(dataset)['scale'] if dataset is not None else 1.0
            self.div_scale = check_spread(K, div_scale)
            self.ks = [int(k) for k in ks if 1 <= int(k) <= K]
        self.weighted = bool(weighted)
        if self.weighted:
            self.wks = sorted({1} | {int(k) for k in ks if 1 <= int(k) <= K})

    @property
    def scene_metrics(self):
        """Whether a joint pass runs (for the joint values, the collision counts or both)."""
        return self.joint or self.radius is not None

    def _put(self, **arrays):
        for name, a in arrays.items():
            self.parts[name].append(_np(a))

    def _cat(self, name):
        return np.concatenate(self.parts[name])

    def add_spread(self, ss):
        cols = torch.tensor([k - 1 for k in self.ks], dtype=torch.long, device=ss.apd.device)
        self._put(spread_agents=torch.stack([ss.apd, ss.fpd, ss.pade, ss.dlow, ss.es_ade, ss.es_fde], dim=1), ade_at_k=ss.ade_at_k[:, cols],
                  fde_at_k=ss.fde_at_k[:, cols])

    def add_weighted(self, ws):
        cols = torch.tensor([k - 1 for k in self.wks], dtype=torch.long, device=ws.eade.device)
        self._put(weighted_agents=torch.stack([getattr(ws, f) for f in ws.F64], dim=1), ade_top_k=ws.ade_top[:, cols],
                  fde_top_k=ws.fde_top[:, cols])

    def add_scene_metrics(self, js, kd, ss=None):
        if ss is not None:
            self.add_spread(ss)
        if js is not None:
            self._put(scene_joint_ade=js.seg_jade, scene_joint_fde=js.seg_jfde, scene_joint_idx=js.seg_jade_idx)
            if js.seg_col is not None:
                self._put(scene_collision=torch.stack([js.seg_col, js.seg_gt_col], dim=1))
        if kd is not None:
            self._put(kde_nll_agents=kd)

    def add_raw(self, sc):
        """A batch's ``metrics.SampleScores`` of the raw set."""
        ls = sc.select
        self.raw_m, self.raw_ks = ls.M, ls.ks
        self._put(raw_sel=torch.stack([ls.ade, ls.fde], dim=1), raw_miss=ls.miss, raw_ade_at=ls.ade_at, raw_fde_at=ls.fde_at)
        if self.joint:
            self._put(raw_joint=torch.stack([ls.seg_jade, ls.seg_jfde], dim=1))
        if sc.kde_nll is not None:
            self._put(raw_kde=sc.kde_nll)
        if sc.spread is not None:
            sp = sc.spread
            self._put(raw_spread=torch.stack([sp.apd, sp.fpd, sp.pade, sp.dlow, sp.es_ade, sp.es_fde], dim=1))

    def report_raw(self, rep):
        v, miss = self._cat('raw_sel').astype(np.float64), self._cat('raw_miss')
        ak, fk = self._cat('raw_ade_at').astype(np.float64), self._cat('raw_fde_at').astype(np.float64)
        rep.raw_m = self.raw_m
        rep.raw_ade, rep.raw_fde = (float(x) for x in v.sum(axis=0) / v.shape[0])
        rep.raw_miss_rate = int(miss.sum()) / v.shape[0]
        rep.raw_ade_at_k = {k: float(ak[:, i].sum() / ak.shape[0]) for i, k in enumerate(self.raw_ks)}
        rep.raw_fde_at_k = {k: float(fk[:, i].sum() / fk.shape[0]) for i, k in enumerate(self.raw_ks)}
        if 'raw_joint' in self.parts:
            rep.raw_joint_ade, rep.raw_joint_fde = (float(x) for x in self._cat('raw_joint').astype(np.float64).mean(axis=0))
        if 'raw_kde' in self.parts:
            kd = self._cat('raw_kde')
            ok = np.isfinite(kd)
            rep.raw_kde_invalid = int((~ok).sum())
            rep.raw_kde_nll = float(kd[ok].mean()) if ok.any() else float('nan')
        if 'raw_spread' in self.parts:
            sv = self._cat('raw_spread')
            (rep.raw_apd, rep.raw_fpd, rep.raw_pade, rep.raw_dlow, rep.raw_energy_ade,
             rep.raw_energy_fde) = (float(x) for x in sv.sum(axis=0) / sv.shape[0])
        return rep

    def add(self, sel, seg_ptr):
        self.tot_a += float(sel.ade.double().sum())
        self.tot_f += float(sel.fde.double().sum())
        self.n += int(sel.ade.numel())
        self._put(scene_ade=sel.seg_ade, scene_fde=sel.seg_fde, scene_miss=sel.seg_miss, scene_agents=np.diff(_np(seg_ptr)),
                  best_idx=sel.best_ade_idx, best_fde_idx=sel.best_fde_idx)
        if sel.best is not None:
            self._put(best=sel.best)

    def report(self, gather):
        miss = int(self._cat('scene_miss').sum())
        rep = EvalReport(ade=self.tot_a / self.n, fde=self.tot_f / self.n, n_agents=self.n, miss_count=miss, miss_rate=miss / self.n,
                         miss_threshold=self.thr, scene_agents=self._cat('scene_agents').astype(np.int64),
                         best=self._cat('best') if gather else None,
                         **{f: self._cat(f) for f in ('scene_ade', 'scene_fde', 'scene_miss', 'best_idx', 'best_fde_idx')})
        if self.joint:
            rep.scene_joint_ade, rep.scene_joint_fde, rep.scene_joint_idx = (self._cat('scene_joint_' + f) for f in ('ade', 'fde', 'idx'))
            rep.joint_ade = float(rep.scene_joint_ade.astype(np.float64).mean())
            rep.joint_fde = float(rep.scene_joint_fde.astype(np.float64).mean())
        if self.radius is not None:
            col = self._cat('scene_collision').astype(np.int64)
            rep.collision_radius, rep.scene_collision = self.radius, col
            rep.collision_rate = int(col[:, 0].sum()) / (self.K * self.n)
            rep.gt_collision_rate = int(col[:, 1].sum()) / self.n
        if self.kde:
            v = self._cat('kde_nll_agents')
            ok = np.isfinite(v)
            rep.kde_nll_agents, rep.kde_invalid = v, int((~ok).sum())
            rep.kde_nll = float(v[ok].mean()) if ok.any() else float('nan')
        if self.spread:
            v, ak, fk = (self._cat(f) for f in ('spread_agents', 'ade_at_k', 'fde_at_k'))
            rep.spread_agents = v
            rep.apd, rep.fpd, rep.pade, rep.dlow, rep.energy_ade, rep.energy_fde = (float(x) for x in v.sum(axis=0) / v.shape[0])
            rep.ade_at_k = {k: float(ak[:, i].astype(np.float64).sum() / ak.shape[0]) for i, k in enumerate(self.ks)}
            rep.fde_at_k = {k: float(fk[:, i].astype(np.float64).sum() / fk.shape[0]) for i, k in enumerate(self.ks)}
        if self.weighted:
            v, ak, fk = (self._cat(f) for f in ('weighted_agents', 'ade_top_k', 'fde_top_k'))

            def mean(x):                                                # over the agents whose value is finite, as kde_nll
                x = x.astype(np.float64)
                ok = np.isfinite(x)
                return float(x[ok].mean()) if ok.any() else float('nan')
            rep.weighted_agents = v
            (rep.eade, rep.efde, rep.w_es_ade, rep.w_es_fde, rep.w_apd, rep.w_fpd, rep.w_kde_nll, rep.brier_ade, rep.brier_fde,
             rep.mean_neff) = (mean(v[:, i]) for i in range(v.shape[1]))
            rep.w_kde_invalid = int((~np.isfinite(v[:, 6])).sum())
            rep.ade_top_k = {k: mean(ak[:, i]) for i, k in enumerate(self.wks)}
            rep.fde_top_k = {k: mean(fk[:, i]) for i, k in enumerate(self.wks)}
        return rep


class _ReportPasses:
    """The metric passes of a report loop's calls, issued into a _ReportAcc (``options``: its arguments behind the threshold): ``follow`` behind
    a pipelined call on its own stream (``finish`` once it is waited for), ``serial`` after a serial call."""

    def __init__(self, model, traj_scale, miss_threshold, gather, *options):
        self.model, self.scale, self.miss_threshold, self.gather = model, traj_scale, miss_threshold, gather
        self.acc = _ReportAcc(miss_threshold, *options)

    def follow(self, h, seg_ptr, joint_ptr, host_ptr, **gt):
        """The passes of the pipelined call ``h`` on its own stream: the selection over ``seg_ptr``, the joint pass over ``joint_ptr``, KDE NLL
        and spread as asked (``gt=``: as the passes take it).  Returns what ``finish`` takes; ``host_ptr``: seg_ptr on the host."""
        m, acc = self.model, self.acc
        sel = m.select_best_of_k_async(h, scale=self.scale, miss_threshold=self.miss_threshold, seg_ptr=seg_ptr, gather=self.gather, **gt)
        js = m.select_joint_async(h, seg_ptr=joint_ptr, scale=self.scale, collision_radius=acc.radius, **gt) if acc.scene_metrics else None
        kd = m.kde_nll_async(h, scale=self.scale, **gt) if acc.kde else None
        ss = m.sample_spread_async(h, scale=self.scale, div_scale=acc.div_scale, **gt) if acc.spread else None
        return h, sel, host_ptr, js, kd, ss

    def finish(self, item):
        h, sel, host_ptr, js, kd, ss = item
        self.model.wait(h)
        self.acc.add(sel, host_ptr)
        self.acc.add_scene_metrics(js, kd, ss)

    def serial(self, pred, seg_ptr, joint_ptr, host_ptr):
        """The same passes on the predictions [K, n, Tf, 2] of a serial call, on the caller's stream."""
        m, acc, pnk = self.model, self.acc, pred.permute(1, 0, 2, 3)
        acc.add(m.select_best_of_k(pnk, scale=self.scale, miss_threshold=self.miss_threshold, seg_ptr=seg_ptr, gather=self.gather), host_ptr)
        if acc.scene_metrics or acc.kde or acc.spread:
            pnk = pnk.contiguous()
            acc.add_scene_metrics(m.select_joint(pnk, seg_ptr=joint_ptr, scale=self.scale, collision_radius=acc.radius)
                                   if acc.scene_metrics else None, m.kde_nll(pnk, scale=self.scale) if acc.kde else None,
                                   m.sample_spread(pnk, scale=self.scale, div_scale=acc.div_scale) if acc.spread else None)

    def report(self):
        return self.acc.report(self.gather)


def _scenes_report(model, dataset, scenes_per_call, pipelined, calls, traj_scale, miss_threshold, gather, *options):
    launch, serial = calls
    p = _ReportPasses(model, traj_scale, miss_threshold, gather, *options, getattr(model.args, 'dataset', None))
    _scene_loop(model, dataset, scenes_per_call, pipelined, lambda sb: p.follow(launch(sb), 'scenes', 'scenes', sb.scene_ptr), p.finish,
                lambda sb: p.serial(serial(sb), model._scene_ptr, model._scene_ptr, sb.scene_ptr))
    return p.report()


@torch.no_grad()
def eval_scenes_report(model, dataset, traj_scale=1.0, scenes_per_call=512, z_fn=None, pipelined=True, miss_threshold=1.0, gather=False,
                       joint=False, kde=False, collision_radius=None, spread=False, div_scale=None, ks=(1, 5, 10)):
    """eval_scenes with the per-scene breakdown, the best sample of every agent and the miss rate (an ``EvalReport``).  The same calls, latents
    and global ADE / FDE as eval_scenes; each call adds one selection pass on its own pipeline stream (``select_best_of_k_async``).
    ``joint`` / ``collision_radius`` / ``kde`` add the scene-level passes (``select_joint_async``, ``kde_nll_async``; after the serial call
    with ``pipelined=False``); every other field is the same with them on or off.  ``spread`` adds the spread pass (``sample_spread_async``:
    APD / FPD, the DLow kernel value at ``div_scale`` -- default: the scale of samplerloss.get_diversity_config for the model's dataset -- the
    energy scores and best-of-k for each k of ``ks``) in the same way."""
    return _scenes_report(model, dataset, scenes_per_call, pipelined, _scene_calls(model, traj_scale, z_fn), traj_scale, miss_threshold, gather,
                          joint, kde, collision_radius, model.args.sample_k, spread, div_scale, ks)


@torch.no_grad()
def eval_scenes_reduced(model, dataset, rounds, K=None, iters=10, from_frame=0, init='first', traj_scale=1.0, scenes_per_call=512, z_fn=None,
                        pipelined=True, miss_threshold=1.0, spread=False, div_scale=None, ks=(1, 5, 10), weighted=False, level='agent',
                        joint=False, collision_radius=None, kde=False):
    """Oversample and reduce as an evaluation loop: per scene batch ``rounds`` inference calls -- M = rounds * sample_k futures
    per agent -- reduced to ``K`` (default sample_k) representatives per agent by ``metrics.reduce_samples`` (``iters``, ``from_frame``,
    ``init`` as there), and the best-of-K selection of eval_scenes_report on the representatives.  Returns an ``EvalReport``.
    ``z_fn(rows)`` is asked once per round, in round order.  ``pipelined`` (default): the rounds go through ``inference_async``, never more
    in flight than ``async_depth`` allows; each is waited for and copied into the round buffer before its slot is taken again.  The reduction
    and the selection run on the caller's stream.  The two forms' samples differ by fp32 rounding (as inference_async and inference do), so
    with rounds > 1 a near-tied label may legitimately differ between them.  ``spread`` / ``div_scale`` / ``ks`` as eval_scenes_report, on the
    representatives: what the reduction does to the diversity of the set.  ``weighted`` adds the weighted-set pass (``weighted_set``) on the
    representatives with the clusters' shares ``Reduction.weights`` as their probabilities: the ``w_*``, ``eade`` / ``efde``, ``brier_*``,
    ``*_top_k`` (k = 1 and each k of ``ks``) and ``mean_neff`` fields; with it off the loop makes the calls it made before.
    ``level='scene'`` reduces whole scenes by ``metrics.reduce_scenes`` over the batch's scene_ptr: representative k of a
    scene's agents is one coherent scene future, and ``weighted`` takes ``SceneReduction.agent_weights``.  ``joint`` / ``collision_radius`` /
    ``kde`` add ``select_joint`` / ``kde_nll`` on the representatives, at either level, into the scene-metric fields of the report: what
    each kind of reduction does to the joint numbers (per-agent representatives share nothing but their cluster's number across agents;
    scene representatives are scene futures).  With these four at their defaults the loop makes the calls it made before.
    ``eval_scenes_reduced_raw`` is this loop with the raw set scored as well."""
    return _eval_scenes_reduced(model, dataset, rounds, K, iters, from_frame, init, traj_scale, scenes_per_call, z_fn, pipelined, miss_threshold,
                                spread, div_scale, ks, weighted, level, joint, collision_radius, kde, False)


@torch.no_grad()
def eval_scenes_reduced_raw(model, dataset, rounds, K=None, iters=10, from_frame=0, init='first', traj_scale=1.0, scenes_per_call=512,
                            z_fn=None, pipelined=True, miss_threshold=1.0, spread=False, div_scale=None, ks=(1, 5, 10), weighted=False,
                            level='agent', joint=False, collision_radius=None, kde=False):
    """eval_scenes_reduced -- the same arguments, calls and report fields, bit for bit -- that also scores the raw set the representatives are
    cut from: per batch, before the reduction, ``model.score_samples`` on the round buffer of M = rounds * sample_k <= 4096
    samples per agent, with ``ks=(sample_k, *ks)`` (sorted, those <= M), ``kde`` and ``spread`` as this loop's own keywords, joint best-of-M
    over the scenes with ``joint``, and the loop's ``traj_scale``, ``miss_threshold`` and ``div_scale``.  Fills the ``raw_*`` fields of the
    ``EvalReport``: what the reduction costs against the oracle bound (``raw_ade`` against ``ade``), and what it does to the diversity
    (``raw_apd`` against ``apd``)."""
    return _eval_scenes_reduced(model, dataset, rounds, K, iters, from_frame, init, traj_scale, scenes_per_call, z_fn, pipelined, miss_threshold,
                                spread, div_scale, ks, weighted, level, joint, collision_radius, kde, True)


def _eval_scenes_reduced(model, dataset, rounds, K, iters, from_frame, init, traj_scale, scenes_per_call, z_fn, pipelined, miss_threshold, spread,
                         div_scale, ks, weighted, level, joint, collision_radius, kde, raw):
    from . import metrics
    rounds = int(rounds)
    if rounds < 1:
        raise ValueError(f'eval_scenes_reduced needs rounds >= 1, got {rounds}')
    if level not in ('agent', 'scene'):
        raise ValueError(f"level must be 'agent' or 'scene', got {level!r}")
    Ks = model.args.sample_k
    K = Ks if K is None else int(K)
    acc = _ReportAcc(miss_threshold, joint=joint, kde=kde, collision_radius=collision_radius, K=K, spread=spread, div_scale=div_scale, ks=ks,
                     dataset=getattr(model.args, 'dataset', None), weighted=weighted)
    depth = max(2, min(8, int(model.async_depth)))
    if raw:
        if rounds * Ks > metrics.LARGE_MAX_M:
            raise ValueError(f'the raw set needs M = rounds * sample_k <= {metrics.LARGE_MAX_M}, got {rounds * Ks}')
        raw_ks = sorted({int(k) for k in (Ks, *ks) if 1 <= int(k) <= rounds * Ks})
        raw_div = acc.div_scale if spread else 1.0
    for s0 in range(0, len(dataset), scenes_per_call):
        sb = dataset.scene_batch(range(s0, min(s0 + scenes_per_call, len(dataset))))
        model.set_scene_batch(sb.past, sb.future, sb.scene_ptr)
        rows = sb.n_agents * Ks
        buf = model._round_buffer(rounds, sb.n_agents)
        if pipelined:
            if model._async_shapes(depth) > 16:                           # batches of ever new sizes: per-shape slot buffers are dropped in time
                model.reset_async()                                       # (nothing is in flight between batches)
            pend = []

            def finish(item):
                r, h = item
                buf[r].copy_(model.wait(h).permute(1, 0, 2, 3))             # [n, sample_k, Tf, 2], on the caller's stream: in front of the slot's next call
            for r in range(rounds):
                if len(pend) >= depth - 1:
                    finish(pend.pop(0))
                pend.append((r, model.inference_async(z=_latents(model, rows, z_fn))))
            while pend:
                finish(pend.pop(0))
        else:
            for r in range(rounds):
                buf[r].copy_(model.inference(None, z=_latents(model, rows, z_fn)).permute(1, 0, 2, 3))
        if raw:
            acc.add_raw(model.score_samples(buf, scale=traj_scale, miss_threshold=miss_threshold, ks=raw_ks,
                                            seg_ptr=model._scene_ptr if joint else False, kde=kde, spread=spread, div_scale=raw_div))
        if level == 'scene':
            red = metrics.reduce_scenes(buf, model._scene_ptr, K, iters=iters, from_frame=from_frame, init=init)
        else:
            red = metrics.reduce_samples(buf, K, iters=iters, from_frame=from_frame, init=init)
        acc.add(model.select_best_of_k(red.centroids, scale=traj_scale, miss_threshold=miss_threshold, seg_ptr=model._scene_ptr), sb.scene_ptr)
        if spread:
            acc.add_spread(model.sample_spread(red.centroids, scale=traj_scale, div_scale=acc.div_scale))
        if acc.scene_metrics or acc.kde:
            acc.add_scene_metrics(model.select_joint(red.centroids, seg_ptr=model._scene_ptr, scale=traj_scale, collision_radius=acc.radius)
                                  if acc.scene_metrics else None, model.kde_nll(red.centroids, scale=traj_scale) if acc.kde else None)
        if weighted:
            acc.add_weighted(model.weighted_set(red.centroids, red.agent_weights if level == 'scene' else red.weights, scale=traj_scale))
    if pipelined:
        model.reset_async()
    return acc.report_raw(acc.report(False)) if raw else acc.report(False)


@dataclasses.dataclass
class MultiModalReport:
    """What eval_scenes_multimodal returns.  ``mmade`` / ``mmfde``: the means over all agents of the per-agent MMADE / MMFDE
    (float64 sums in dataset order); ``n_agents``; ``mean_count``: the mean size of an agent's neighbour set, itself included;
    ``frac_multi``: the share of agents with more than one neighbour (count > 1); ``mmade_multi`` / ``mmfde_multi``: the means over those
    agents alone, NaN if there are none; ``eps``, ``hist_frames``, ``within`` as used; per agent in dataset order ``count`` [n] int32 and
    ``mmade_agents`` / ``mmfde_agents`` [n] float64."""
    mmade: float
    mmfde: float
    n_agents: int
    mean_count: float
    frac_multi: float
    mmade_multi: float
    mmfde_multi: float
    eps: float
    hist_frames: int
    within: str
    count: np.ndarray
    mmade_agents: np.ndarray
    mmfde_agents: np.ndarray


def multimodal_segments(dataset, scene_ptr, within):
    """The agent segments inside which eval_scenes_multimodal looks for neighbours, as a CSR over the agents of ``scene_ptr`` [S+1] (the
    whole dataset's scenes in order), or None for one segment: ``within='dataset'`` -- None; ``'file'`` -- consecutive scenes with equal
    ``dataset.seq_name`` form a segment (recordings with different homographies do not mix); ``'scene'`` -- ``scene_ptr`` itself."""
    ptr = np.asarray(scene_ptr, dtype=np.int64)
    if within == 'dataset':
        return None
    if within == 'scene':
        return ptr.astype(np.int32)
    if within != 'file':
        raise ValueError(f"within must be 'dataset', 'file' or 'scene', got {within!r}")
    names = getattr(dataset, 'seq_name', None)
    if names is None or len(names) != len(ptr) - 1:
        raise ValueError("within='file' needs dataset.seq_name with one name per scene")
    first = [s for s in range(len(names)) if s == 0 or names[s] != names[s - 1]]
    return ptr[first + [len(names)]].astype(np.int32)


@torch.no_grad()
def eval_scenes_multimodal(model, dataset, eps, hist_frames=None, within='dataset', traj_scale=1.0, scenes_per_call=512, z_fn=None,
                           pipelined=True, sampler=None, mean=True, eps_fn=None):
    """MMADE / MMFDE of a scene dataset (a ``MultiModalReport``): do the K samples of an agent cover the futures that agents
    with a similar history actually had?  The calls and latents of eval_scenes (of eval_sampler with ``sampler``; ``mean`` / ``eps_fn`` as
    there); every call's samples are copied into one device buffer [n, K, Tf, 2] for the whole dataset -- a pipelined call is waited for and
    copied on the caller's stream before its slot is taken again -- and ONE ``metrics.multimodal`` pass runs over all agents, with the
    dataset's own observed and future tracks.  ``eps`` (in units of ``traj_scale`` times the data's) and ``hist_frames`` (default
    past_length - 1) define the neighbours, ``within`` where they are looked for (``multimodal_segments``)."""
    from . import metrics
    if within not in ('dataset', 'file', 'scene'):
        raise ValueError(f"within must be 'dataset', 'file' or 'scene', got {within!r}")
    whole = dataset.scene_batch(range(len(dataset)))
    n, K, Tf = whole.n_agents, model.args.sample_k, model.args.future_length
    e, h = metrics.check_multimodal(n, K, int(whole.past.shape[1]), Tf, eps, hist_frames, traj_scale)
    seg = multimodal_segments(dataset, whole.scene_ptr, within)
    buf = torch.empty(n, K, Tf, 2, dtype=torch.float32, device=model.device)
    pos = 0

    def put(pred):                                                        # [K, n_call, Tf, 2] of the next call in dataset order
        nonlocal pos
        buf[pos:pos + pred.shape[1]].copy_(pred.permute(1, 0, 2, 3))
        pos += int(pred.shape[1])
    launch, serial = _scene_calls(model, traj_scale, z_fn) if sampler is None else _sampler_calls(model, sampler, traj_scale, mean, eps_fn)
    _scene_loop(model, dataset, scenes_per_call, pipelined, launch, lambda h_: put(model.wait(h_)), lambda sb: put(serial(sb)))
    assert pos == n, (pos, n)
    mm = metrics.multimodal(buf, whole.past, whole.future, e, hist_frames=h, scale=traj_scale, seg_ptr=seg)
    count, a, f = mm.count.cpu().numpy(), mm.mmade.cpu().numpy(), mm.mmfde.cpu().numpy()
    multi = count > 1
    nan = float('nan')
    return MultiModalReport(mmade=float(a.sum() / n), mmfde=float(f.sum() / n), n_agents=n, mean_count=float(count.sum(dtype=np.int64) / n),
                            frac_multi=float(multi.sum() / n), mmade_multi=float(a[multi].sum() / multi.sum()) if multi.any() else nan,
                            mmfde_multi=float(f[multi].sum() / multi.sum()) if multi.any() else nan, eps=e, hist_frames=h, within=within,
                            count=count, mmade_agents=a, mmfde_agents=f)


@torch.no_grad()
def eval_sampler_report(model, sampler, dataset, traj_scale=1.0, scenes_per_call=512, mean=True, eps_fn=None, pipelined=True,
                        miss_threshold=1.0, gather=False, joint=False, kde=False, collision_radius=None, spread=False, div_scale=None,
                        ks=(1, 5, 10)):
    """eval_sampler with the per-scene breakdown, the best sample of every agent and the miss rate (an ``EvalReport``; test_sampler.py:214-217
    asks count_miss_samples of the same loop).  ``joint`` / ``collision_radius`` / ``kde`` / ``spread`` / ``div_scale`` / ``ks`` as
    eval_scenes_report."""
    return _scenes_report(model, dataset, scenes_per_call, pipelined, _sampler_calls(model, sampler, traj_scale, mean, eps_fn), traj_scale, miss_threshold, gather,
                          joint, kde, collision_radius, model.args.sample_k, spread, div_scale, ks)


@torch.no_grad()
def eval_nba_report(model, loader, traj_scale=1.0, z_fn=None, pipelined=True, groups_per_call=16, miss_threshold=1.0, gather=False,
                    joint=False, kde=False, collision_radius=None, spread=False, div_scale=None, ks=(1, 5, 10)):
    """NBA evaluation (test.py:495-552) as an ``EvalReport``: ADE / FDE over the whole horizon (the last horizon of eval_nba), the miss rate,
    per loader batch its ADE / FDE / miss count, the best sample of every agent.  Calls as eval_nba: up to ``groups_per_call`` loader batches
    of one shape per call, several in flight, the selection on each call's pipeline stream with one segment per loader batch.
    ``joint`` / ``collision_radius`` / ``kde`` / ``spread`` / ``div_scale`` / ``ks`` as eval_scenes_report; the joint and collision segments
    are games (N players each)."""
    K, dev = model.args.sample_k, model.device
    p = _ReportPasses(model, traj_scale, miss_threshold, gather, joint, kde, collision_radius, K, spread, div_scale, ks,
                      getattr(model.args, 'dataset', 'nba'))
    if not pipelined:
        for data in loader:
            model.set_data_nba(data)
            B, N = data['past_traj'].shape[:2]
            z = z_fn(B * N * K) if z_fn is not None else None
            sp = np.array([0, B * N], dtype=np.int32)
            p.serial(model.inference(data, z=z), sp, np.arange(0, B * N + 1, N, dtype=np.int32), sp)
        return p.report()
    seg_ptrs = {}

    def csr(n, step):                                            # a device CSR of equal segments, complete before any stream reads it
        if (n, step) not in seg_ptrs:
            seg_ptrs[(n, step)] = torch.arange(0, n + 1, step, dtype=torch.int32, device=dev)
            torch.cuda.current_stream(dev).synchronize()
        return seg_ptrs[(n, step)]

    def follow(h, G, B, N):                                      # one selection segment per loader batch, one joint segment per game
        n = G * B * N
        return p.follow(h, csr(n, B * N), csr(n, N) if p.acc.scene_metrics else None, np.arange(0, n + 1, B * N), gt=model._future)
    _nba_loop(model, loader, z_fn, groups_per_call, follow, p.finish)
    return p.report()


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
