"""References of the scene-level (joint) best-of-K objective (sttode_loss_objective_joint, sttode_loss_diverse_joint), generic
over the dtype of their inputs as tests/train_ref.py: the kernel-level ``objective_joint`` -- train_ref.objective with the min over K taken
over the segment sums -- and the model-level ``oracle_joint_loss`` -- oracle.sttode_ref.STTODENetRef.forward_loss_tensors from the
oracle's public pieces with the joint term in the place of the marginal one.  The reference has no joint objective; these two are held,
independently of each other and of the kernels, by tests/test_joint_objective.py."""
import torch

import train_ref as R


def segments_of(n, scene_ptr=None, seg_len=None):
    """The segments [(first agent, one past the last)] of the joint entry points' rule: the scenes of a CSR [S + 1], else runs of seg_len
    agents (seg_len divides n)."""
    if scene_ptr is not None:
        ptr = [int(v) for v in scene_ptr]
        assert ptr[0] == 0 and ptr[-1] == n and all(b > a for a, b in zip(ptr[:-1], ptr[1:]))
        return list(zip(ptr[:-1], ptr[1:]))
    assert seg_len >= 1 and n % seg_len == 0
    return [(a, a + seg_len) for a in range(0, n, seg_len)]


def joint_term(d2, segs, per_scene):
    """d2 [n, K] -> (sum_g w_g min_k J_g(k), first argmin [G] (0-based), J [G, K]); J_g(k) = sum_{a in g} d2[a, k]; w_g = 1 / (agents of g)
    where each segment is a scene of its own (``per_scene``: a CSR batch), 1 / n otherwise."""
    n = d2.shape[0]
    J = torch.stack([d2[a:b].sum(0) for a, b in segs])
    mn, idx = J.min(dim=1)                                           # (first minimum; its gradient goes to that sample alone)
    w = torch.tensor([1.0 / (b - a) if per_scene else 1.0 / n for a, b in segs], dtype=d2.dtype)
    return (mn * w).sum(), idx, J


def objective_joint(pred, rec, fut, past, qzp, scene_ptr, seg_len, K1, scale_mse, scale_rec, kl_denom, min_clip):
    """train_ref.objective with the joint term: the same mse, recover and KL terms, and in the diverse slot sum_g w_g J_g(k*_g) over the
    segments of (scene_ptr, seg_len).  -> dict mse, rec, kl, diverse, total (0-d), dpred, drec, dqzp (torch autograd of the total), best [n]
    and seg_best [G] (1..K: the first minimum of the agent's / the segment's J), J [G, K] and d2 [n, K]."""
    n = pred.shape[0]
    assert pred.shape[1] == rec.shape[1] == K1
    P, Rc, Q = (v.detach().clone().requires_grad_(True) for v in (pred, rec, qzp))
    mse = (fut - P[:, 0]).pow(2).sum() * scale_mse
    recover = (past - Rc[:, 0]).pow(2).sum() * scale_rec
    kl = R.scene_kl(Q, scene_ptr, kl_denom).clamp_min(min_clip).sum()
    d2 = (fut[:, None, :] - P[:, 1:]).pow(2).sum(-1)                 # [n, K]
    segs = segments_of(n, scene_ptr, seg_len)
    diverse, idx, J = joint_term(d2, segs, scene_ptr is not None)
    total = ((mse + recover) + kl) + diverse
    total.backward()
    seg_best = (idx + 1).to(torch.int32)
    best = torch.cat([seg_best[g].repeat(b - a) for g, (a, b) in enumerate(segs)])
    return dict(mse=mse.detach(), rec=recover.detach(), kl=kl.detach(), diverse=diverse.detach(), total=total.detach(), dpred=P.grad,
                drec=Rc.grad, dqzp=Q.grad, best=best, seg_best=seg_best, J=J.detach(), d2=d2.detach())


def oracle_joint_loss(ref_net, eps_q, eps_p1, eps_p20, segments):
    """STTODENetRef.forward_loss_tensors (after set_data / set_data_nba) with the joint term: (total, pred, recover, kl, diverse_joint) as
    tensors with their autograd graph, in the dtype of ``ref_net`` and its inputs.  ``segments``: [(first, one past the last)] over the
    call's agents -- [(0, n)] for one scene, the games [(b N, b N + N)] in NBA mode; every segment weighs 1 / n, as the marginal mean."""
    from oracle.sttode_ref import Normal
    m, a = ref_net, ref_net.args
    B, N = m.batch_size, m.agent_num
    pf = m.past_encoder(m.inputs, B, N)
    qz = Normal(params=m.future_encoder(m.inputs_for_posterior, B, N, pf))
    qz_s = qz.rsample(eps_q)
    zeros = torch.zeros(pf.shape[0], a.zdim, dtype=pf.dtype)
    pz = Normal(mu=zeros, logvar=zeros)
    pz.rsample(eps_p1)
    pred, rec = m.decoder(pf, qz_s, m.past_traj, m.cur_location, sample_num=1)
    lp = (m.future_traj - pred).pow(2).sum() / B / pred.shape[1]
    lr = (m.past_traj - rec).pow(2).sum() / B / rec.shape[1]
    lk = (qz.kl(pz).sum() / (B * N)).clamp_min(a.min_clip)
    div, _ = m.decoder(pf.repeat_interleave(20, dim=0), eps_p20, m.past_traj, m.cur_location, sample_num=20, mode='inference')
    d2 = (m.future_traj.unsqueeze(1) - div).pow(2).sum(-1).sum(-1)   # [n, 20]
    ld, _, _ = joint_term(d2, segments, False)
    return lp + lr + lk + ld, lp, lr, lk, ld
