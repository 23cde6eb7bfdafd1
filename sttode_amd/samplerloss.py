"""Stage-2 objective: drop-in for samplerloss.py:4-73 (values; the per-agent reductions run in ``sttode_sampler_loss``)."""
import torch

from . import capi


def get_diversity_config(dataset):
    """trainsampler.py:102-116."""
    return {'sdd': {'weight': 0.5, 'scale': 0.5}, 'eth': {'weight': 1, 'scale': 1}, 'univ': {'weight': 10, 'scale': 10.0},
            'nba': {'weight': 1, 'scale': 1.0}}.get(dataset, {'weight': 3, 'scale': 2})


class _PerAgentLoss(torch.autograd.Function):
    """(kld[a], div[a]) = sttode_sampler_loss; backward = sttode_sampler_loss_bwd (gradients wrt mu, logvar, motion)."""

    @staticmethod
    def forward(ctx, mu, logvar, motion, pmu, plogvar, scale):
        n, K = motion.shape[:2]
        D = motion[0, 0].numel()
        nz = mu.shape[-1]
        kld = torch.empty(n, device=mu.device)
        div = torch.empty(n, device=mu.device)
        capi.call('sttode_sampler_loss', mu, logvar, pmu, plogvar, motion, n, K, nz, D, float(scale), kld, div, capi.stream_ptr())
        ctx.save_for_backward(mu, logvar, motion, *([pmu, plogvar] if pmu is not None else []))
        ctx.dims = (n, K, nz, D, float(scale))
        return kld, div

    @staticmethod
    def backward(ctx, g_kld, g_div):
        mu, logvar, motion, *pp = ctx.saved_tensors
        pmu, plogvar = pp if pp else (None, None)
        n, K, nz, D, scale = ctx.dims
        dmu, dlv, dmo = torch.empty_like(mu), torch.empty_like(logvar), torch.empty_like(motion)
        capi.call('sttode_sampler_loss_bwd', mu, logvar, pmu, plogvar, motion, g_kld.contiguous(), g_div.contiguous(), n, K, nz, D, scale,
                  dmu, dlv, dmo, capi.stream_ptr())
        return dmu, dlv, dmo, None, None, None


def _per_agent(q, p, motion, scale):
    """(kld[a], div[a]) for motion [n,K,Tf,2], q/p Normal over [n*K, nz]; differentiable wrt q.mu, q.logvar and motion."""
    if q.mu.device.type != 'cuda':
        raise capi.SttodeError('sampler loss runs only on a HIP device (no CPU fallback)')
    f = lambda t: t.contiguous().float()
    return _PerAgentLoss.apply(f(q.mu), f(q.logvar), f(motion), None if p is None else f(p.mu).detach(),
                               None if p is None else f(p.logvar).detach(), scale)


def compute_z_kld(q_z_dist_dlow, p_z_dist_infer, agent_num, min_clip, weight, _kld=None):
    s = (_kld if _kld is not None else q_z_dist_dlow.kl(p_z_dist_infer)).sum()
    uw = (s / agent_num).clamp_min(min_clip)
    return uw * weight, uw


def diversity_loss(infer_dec_motion, agent_num, weight, scale, _div=None):
    if _div is None:
        n, K = infer_dec_motion.shape[:2]
        zeros = torch.zeros(n * K, 16, device=infer_dec_motion.device)
        from .dist import Normal
        _, _div = _per_agent(Normal(mu=zeros, logvar=zeros), None, infer_dec_motion, scale)
    uw = _div.sum() / agent_num
    return uw * weight, uw


class _Objective(torch.autograd.Function):
    """(kld, div, rec, es_ade, es_fde)[a] = sttode_sampler_objective (one launch); backward = sttode_sampler_objective_bwd (one launch,
    one summed dmotion).  An output nobody uses reaches the kernel as a NULL upstream gradient (= zero)."""

    @staticmethod
    def forward(ctx, mu, logvar, motion, pmu, plogvar, gt, mask, scale):
        n, K = motion.shape[:2]
        D = motion[0, 0].numel()
        nz = mu.shape[-1]
        kld, div, rec, es_ade, es_fde = (torch.empty(n, device=mu.device) for _ in range(5))
        best = torch.empty(n, dtype=torch.int32, device=mu.device)
        capi.call('sttode_sampler_objective', mu, logvar, pmu, plogvar, motion, gt, mask, n, K, nz, D, float(scale), kld, div, rec, best,
                  es_ade, es_fde, capi.stream_ptr())
        ctx.save_for_backward(mu, logvar, motion, gt, *(t for t in (pmu, plogvar, mask) if t is not None))
        ctx.opt = (pmu is not None, mask is not None)
        ctx.dims = (n, K, nz, D, float(scale))
        ctx.set_materialize_grads(False)
        return kld, div, rec, es_ade, es_fde

    @staticmethod
    def backward(ctx, *g):
        mu, logvar, motion, gt, *rest = ctx.saved_tensors
        pmu, plogvar = (rest.pop(0), rest.pop(0)) if ctx.opt[0] else (None, None)
        mask = rest.pop(0) if ctx.opt[1] else None
        n, K, nz, D, scale = ctx.dims
        g = [None if t is None else t.contiguous().float() for t in g]
        dmu, dlv, dmo = torch.empty_like(mu), torch.empty_like(logvar), torch.empty_like(motion)
        capi.call('sttode_sampler_objective_bwd', mu, logvar, pmu, plogvar, motion, gt, mask, *g, n, K, nz, D, scale, dmu, dlv, dmo,
                  capi.stream_ptr())
        return dmu, dlv, dmo, None, None, None, None, None


def _objective(q, p, motion, gt, fut_mask, scale):
    """The five per-agent terms of sttode_sampler_objective for motion [n,K,Tf,2], gt [n,Tf,2], fut_mask None | [n,Tf] on any device;
    differentiable wrt q.mu, q.logvar and motion."""
    if motion.device.type != 'cuda' or gt.device.type != 'cuda' or q.mu.device.type != 'cuda':
        raise capi.SttodeError('sampler objective runs only on a HIP device (no CPU fallback)')
    f = lambda t: t.contiguous().float()
    n, Tf = motion.shape[0], motion.shape[2] if motion.dim() == 4 else -1
    if motion.dim() != 4 or motion.shape[3] != 2 or tuple(gt.shape) != (n, Tf, 2):
        raise capi.SttodeError(f'sampler objective: motion [n,K,Tf,2] and gt [n,Tf,2] expected, got {tuple(motion.shape)} and {tuple(gt.shape)}')
    mask = None
    if fut_mask is not None:
        mask = f(torch.as_tensor(fut_mask).to(motion.device)).detach()
        if tuple(mask.shape) != (n, Tf):
            raise capi.SttodeError(f'sampler objective: fut_mask [n,Tf] = {(n, Tf)} expected, got {tuple(mask.shape)}')
    return _Objective.apply(f(q.mu), f(q.logvar), f(motion), None if p is None else f(p.mu).detach(),
                            None if p is None else f(p.logvar).detach(), f(gt).detach(), mask, scale)


def _motion_only(fut_motion_orig, infer_dec_motion, fut_mask):
    """The objective's ground-truth terms for callers that have no latent distribution (recon_loss / energy_loss on their own)."""
    from .dist import Normal
    if infer_dec_motion.device.type != 'cuda':
        raise capi.SttodeError('sampler objective runs only on a HIP device (no CPU fallback)')
    n, K = infer_dec_motion.shape[:2]
    zeros = torch.zeros(n * K, 1, device=infer_dec_motion.device)
    return _objective(Normal(mu=zeros, logvar=zeros), None, infer_dec_motion, fut_motion_orig, fut_mask, 1.0)


def recon_loss(fut_motion_orig, infer_dec_motion, fut_mask, weight, _rec=None):
    """samplerloss.py:23-31: mean over agents of min_k sum_t |mask_t (x_k,t - y_t)|^2 -> (loss, loss_unweighted)."""
    if _rec is None:
        _rec = _motion_only(fut_motion_orig, infer_dec_motion, fut_mask)[2]
    uw = _rec.mean()
    return uw * weight, uw


def energy_loss(fut_motion_orig, infer_dec_motion, fut_mask, weight, kind='ade', _es=None):
    """Mean over agents of the energy score of the K samples against the ground truth, on the per-frame mean
    displacement ('ade') or the last frame's ('fde') -> (loss, loss_unweighted)."""
    if kind not in ('ade', 'fde'):
        raise ValueError(f"energy_loss: kind 'ade' | 'fde', got {kind!r}")
    if _es is None:
        _es = _motion_only(fut_motion_orig, infer_dec_motion, fut_mask)[3 if kind == 'ade' else 4]
    uw = _es.mean()
    return uw * weight, uw


class _ObjectiveJoint(torch.autograd.Function):
    """kld [n] and (div, rec, es) [S] = sttode_sampler_objective_joint; backward = sttode_sampler_objective_joint_bwd, one
    summed dmotion.  An output nobody uses reaches the kernel as a NULL upstream gradient (= zero)."""

    @staticmethod
    def forward(ctx, mu, logvar, motion, pmu, plogvar, gt, mask, seg_ptr, scale):
        n, K = motion.shape[:2]
        D = motion[0, 0].numel()
        nz = mu.shape[-1]
        S = seg_ptr.numel() - 1
        dev = mu.device
        kld = torch.empty(n, device=dev)
        div, rec, es = (torch.empty(S, device=dev) for _ in range(3))
        best = torch.empty(S, dtype=torch.int32, device=dev)
        nb = capi.sampler_joint_ws(n, K, S)
        ws = torch.empty((nb + 7) // 8, dtype=torch.float64, device=dev)
        capi.call('sttode_sampler_objective_joint', mu, logvar, pmu, plogvar, motion, gt, mask, seg_ptr, S, n, K, nz, D, float(scale), ws,
                  ws.numel() * 8, kld, div, rec, best, es, capi.stream_ptr())
        ctx.save_for_backward(mu, logvar, motion, gt, seg_ptr, ws, *(t for t in (pmu, plogvar, mask) if t is not None))
        ctx.opt = (pmu is not None, mask is not None)
        ctx.dims = (S, n, K, nz, D, float(scale))
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(best)
        return kld, div, rec, es, best

    @staticmethod
    def backward(ctx, g_kld, g_div, g_rec, g_es, _g_best):
        mu, logvar, motion, gt, seg_ptr, ws, *rest = ctx.saved_tensors
        pmu, plogvar = (rest.pop(0), rest.pop(0)) if ctx.opt[0] else (None, None)
        mask = rest.pop(0) if ctx.opt[1] else None
        S, n, K, nz, D, scale = ctx.dims
        g = [None if t is None else t.contiguous().float() for t in (g_kld, g_div, g_rec, g_es)]
        dmu, dlv, dmo = torch.empty_like(mu), torch.empty_like(logvar), torch.empty_like(motion)
        capi.call('sttode_sampler_objective_joint_bwd', mu, logvar, pmu, plogvar, motion, gt, mask, seg_ptr, S, *g, n, K, nz, D, scale, ws,
                  ws.numel() * 8, dmu, dlv, dmo, capi.stream_ptr())
        return dmu, dlv, dmo, None, None, None, None, None, None


def _segments(seg_ptr, n, device):
    """seg_ptr None (all n agents one segment) | a CSR [S+1] as list, array or tensor -> int32 device tensor."""
    from . import metrics
    if seg_ptr is None:
        seg_ptr = [0, n]
    metrics.check_seg_ptr(seg_ptr, n)
    return metrics.seg_ptr_tensor(seg_ptr, device)


def _objective_joint(q, p, motion, gt, fut_mask, seg_ptr, scale):
    """kld [n] and the joint div, rec, es [S] (and best [S], int32) of sttode_sampler_objective_joint for motion [n,K,Tf,2], gt [n,Tf,2],
    fut_mask None | [n,Tf] on any device, seg_ptr None | CSR [S+1]; differentiable wrt q.mu, q.logvar and motion."""
    if motion.device.type != 'cuda' or gt.device.type != 'cuda' or q.mu.device.type != 'cuda':
        raise capi.SttodeError('joint sampler objective runs only on a HIP device (no CPU fallback)')
    f = lambda t: t.contiguous().float()
    n, Tf = motion.shape[0], motion.shape[2] if motion.dim() == 4 else -1
    if motion.dim() != 4 or motion.shape[3] != 2 or tuple(gt.shape) != (n, Tf, 2):
        raise capi.SttodeError(f'joint sampler objective: motion [n,K,Tf,2] and gt [n,Tf,2] expected, got {tuple(motion.shape)} and {tuple(gt.shape)}')
    mask = None
    if fut_mask is not None:
        mask = f(torch.as_tensor(fut_mask).to(motion.device)).detach()
        if tuple(mask.shape) != (n, Tf):
            raise capi.SttodeError(f'joint sampler objective: fut_mask [n,Tf] = {(n, Tf)} expected, got {tuple(mask.shape)}')
    sp = _segments(seg_ptr, n, motion.device)
    with torch.cuda.device(motion.device):
        return _ObjectiveJoint.apply(f(q.mu), f(q.logvar), f(motion), None if p is None else f(p.mu).detach(),
                                     None if p is None else f(p.logvar).detach(), f(gt).detach(), mask, sp, scale)


def _motion_only_joint(fut_motion_orig, infer_dec_motion, fut_mask, seg_ptr, scale=1.0):
    """The joint terms for callers that have no latent distribution (the stand-alone joint losses)."""
    from .dist import Normal
    if infer_dec_motion.device.type != 'cuda':
        raise capi.SttodeError('joint sampler objective runs only on a HIP device (no CPU fallback)')
    n, K = infer_dec_motion.shape[:2]
    zeros = torch.zeros(n * K, 1, device=infer_dec_motion.device)
    if fut_motion_orig is None:                                    # the diversity term reads no ground truth
        fut_motion_orig = torch.zeros(n, *infer_dec_motion.shape[2:], device=infer_dec_motion.device)
    return _objective_joint(Normal(mu=zeros, logvar=zeros), None, infer_dec_motion, fut_motion_orig, fut_mask, seg_ptr, scale)


def diversity_loss_joint(infer_dec_motion, seg_ptr, weight, scale, _div=None):
    """Mean over the segments of the joint DLow term: exp(-d2_g / scale) over the sample pairs, d2_g the segment's mean squared distance
     -> (loss, loss_unweighted)."""
    if _div is None:
        _div = _motion_only_joint(None, infer_dec_motion, None, seg_ptr, scale)[1]
    uw = _div.sum() / _div.numel()
    return uw * weight, uw


def recon_loss_joint(fut_motion_orig, infer_dec_motion, fut_mask, seg_ptr, weight, _rec=None):
    """sum_g rec_g / n: ONE best sample per segment, its masked squared error summed over the segment's agents (>= the marginal
    recon_loss, equal when the agents' own minima coincide) -> (loss, loss_unweighted)."""
    if _rec is None:
        _rec = _motion_only_joint(fut_motion_orig, infer_dec_motion, fut_mask, seg_ptr)[2]
    uw = _rec.sum() / infer_dec_motion.shape[0]
    return uw * weight, uw


def energy_loss_joint(fut_motion_orig, infer_dec_motion, fut_mask, seg_ptr, weight, _es=None):
    """Mean over the segments of the joint energy score on the scene's RMS displacement -> (loss, loss_unweighted)."""
    if _es is None:
        _es = _motion_only_joint(fut_motion_orig, infer_dec_motion, fut_mask, seg_ptr)[3]
    uw = _es.sum() / _es.numel()
    return uw * weight, uw


def _compute_sampler_loss_joint(args, fut_motion_orig, infer_dec_motion, fut_mask, p_z_dist, q_z_dist_dlow, div_cfg, seg_ptr, recon, energy,
                                energy_weight):
    """compute_sampler_loss(joint=True): one forward call and one backward call for kld + joint diverse (+ joint recon) (+ joint energy)."""
    agent_num = fut_motion_orig.shape[0]
    kld_a, div_g, rec_g, es_g, _ = _objective_joint(q_z_dist_dlow, p_z_dist, infer_dec_motion, fut_motion_orig, fut_mask, seg_ptr,
                                                    div_cfg['scale'])
    kld_loss, _ = compute_z_kld(q_z_dist_dlow, p_z_dist, agent_num, args.kld_min_clamp, args.kld_weight, _kld=kld_a)
    div_loss, _ = diversity_loss_joint(infer_dec_motion, seg_ptr, div_cfg['weight'], div_cfg['scale'], _div=div_g)
    total_loss = kld_loss + div_loss
    loss_dict = {'kld': kld_loss, 'diverse': div_loss, 'recon': 0}
    if recon:
        loss_dict['recon'], _ = recon_loss_joint(fut_motion_orig, infer_dec_motion, fut_mask, seg_ptr, args.recon_weight, _rec=rec_g)
        total_loss = total_loss + loss_dict['recon']
    if energy:
        loss_dict['energy'], _ = energy_loss_joint(fut_motion_orig, infer_dec_motion, fut_mask, seg_ptr, float(energy_weight), _es=es_g)
        total_loss = total_loss + loss_dict['energy']
    return total_loss, loss_dict, dict(loss_dict)


def compute_sampler_loss(args, fut_motion_orig, infer_dec_motion, batch_size, fut_mask, p_z_dist, q_z_dist_dlow, div_cfg, *, recon=False,
                         energy_weight=0.0, energy_kind='ade', joint=False, seg_ptr=None):
    """samplerloss.py:41-58: total = weighted clamped KL + weighted diversity (reconstruction term disabled upstream).
    recon=True adds args.recon_weight * recon_loss (the call upstream comments out; loss_dict['recon']); energy_weight > 0 adds that weight
    times the mean energy score (loss_dict['energy']).  With either on, the whole objective is one sttode_sampler_objective call and one
    backward call; with both off, exactly the calls and the dict of the reference's two-term objective.
    joint=True: the diversity, reconstruction and energy terms in their scene-level forms over the segments of the CSR
    ``seg_ptr`` (list, array or tensor; None: all agents one segment, the training loop's one scene per step); the KL term stays per
    agent; one sttode_sampler_objective_joint call and one backward call.  The joint energy score has one kind ('ade': all frames)."""
    agent_num = fut_motion_orig.shape[0]
    if energy_kind not in ('ade', 'fde'):
        raise ValueError(f"compute_sampler_loss: energy_kind 'ade' | 'fde', got {energy_kind!r}")
    energy = energy_weight is not None and float(energy_weight) > 0.0
    if joint:
        if energy_kind != 'ade':
            raise ValueError("compute_sampler_loss: the joint energy score has one kind, the all-frames RMS form (energy_kind='ade'); "
                             f"got {energy_kind!r} with joint=True")
        return _compute_sampler_loss_joint(args, fut_motion_orig, infer_dec_motion, fut_mask, p_z_dist, q_z_dist_dlow, div_cfg, seg_ptr,
                                           recon, energy, energy_weight)
    if seg_ptr is not None:
        raise ValueError('compute_sampler_loss: seg_ptr is read only with joint=True')
    if not recon and not energy:
        kld_a, div_a = _per_agent(q_z_dist_dlow, p_z_dist, infer_dec_motion, div_cfg['scale'])
    else:
        kld_a, div_a, rec_a, es_ade_a, es_fde_a = _objective(q_z_dist_dlow, p_z_dist, infer_dec_motion, fut_motion_orig, fut_mask,
                                                             div_cfg['scale'])
    kld_loss, _ = compute_z_kld(q_z_dist_dlow, p_z_dist, agent_num, args.kld_min_clamp, args.kld_weight, _kld=kld_a)
    div_loss, _ = diversity_loss(infer_dec_motion, agent_num, div_cfg['weight'], div_cfg['scale'], _div=div_a)
    total_loss = kld_loss + div_loss
    loss_dict = {'kld': kld_loss, 'diverse': div_loss, 'recon': 0}
    if recon:
        loss_dict['recon'], _ = recon_loss(fut_motion_orig, infer_dec_motion, fut_mask, args.recon_weight, _rec=rec_a)
        total_loss = total_loss + loss_dict['recon']
    if energy:
        loss_dict['energy'], _ = energy_loss(fut_motion_orig, infer_dec_motion, fut_mask, float(energy_weight), energy_kind,
                                             _es=es_ade_a if energy_kind == 'ade' else es_fde_a)
        total_loss = total_loss + loss_dict['energy']
    return total_loss, loss_dict, dict(loss_dict)


def compute_sampler_loss_nba(args, fut_motion_orig, infer_dec_motion, batch_size, p_z_dist, q_z_dist_dlow, div_cfg, *, recon=False,
                             energy_weight=0.0, energy_kind='ade', joint=False, seg_len=None):
    """samplerloss.py:60-73.  joint=True: the scene-level terms with one segment per game of ``seg_len`` agents (required; it divides n)."""
    if not joint:
        if seg_len is not None:
            raise ValueError('compute_sampler_loss_nba: seg_len is read only with joint=True')
        return compute_sampler_loss(args, fut_motion_orig, infer_dec_motion, batch_size, None, p_z_dist, q_z_dist_dlow, div_cfg, recon=recon,
                                    energy_weight=energy_weight, energy_kind=energy_kind)
    n = fut_motion_orig.shape[0]
    if seg_len is None or int(seg_len) < 1 or n % int(seg_len) != 0:
        raise ValueError(f'compute_sampler_loss_nba: joint=True needs seg_len (agents per game) dividing n = {n}, got {seg_len!r}')
    return compute_sampler_loss(args, fut_motion_orig, infer_dec_motion, batch_size, None, p_z_dist, q_z_dist_dlow, div_cfg, recon=recon,
                                energy_weight=energy_weight, energy_kind=energy_kind, joint=True,
                                seg_ptr=list(range(0, n + 1, int(seg_len))))
