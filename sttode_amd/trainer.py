"""Caller-side training loop over the HIP training step: the reference's ``train()`` (train.py:55-100) and checkpoint
format (train.py:208-213), without the argparse / dataset-path plumbing.

    model = STTODENet(args, device); optimizer = Adam(model.parameters(), lr=args.lr)
    scheduler = StepLR(optimizer, step_size=args.decay_step, gamma=args.decay_gamma)
    for epoch in range(args.num_epochs):
        train_epoch(args, epoch, model, optimizer, scheduler, loader)

``model.forward()`` runs forward + (lazily, inside ``total_loss.backward()``) backward on csrc/train*.hip kernels; the
optimizer is torch's (element-wise parameter update on device tensors).
"""
import torch


def train_epoch(args, epoch, model, optimizer, scheduler, train_loader, log=print, max_iters=None, log_grad_norm=False):
    """One epoch.  NBA: loader yields seq_collate dicts (train.py:59-71); otherwise the per-scene 10-tuples of
    TrajectoryDataset / SDD_Dataset wrapped by DataLoader(batch_size=1) (train.py:72-95).  Returns the list of total losses.
    log_grad_norm: with an optimizer that has ``last_grad_norm`` (sttode_amd.optim.Adam with max_grad_norm / skip_nonfinite), the printed
    lines also carry the last step's global gradient norm and the number of steps the non-finite guard skipped."""
    model.train()
    total_iter_num = len(train_loader)
    losses = []
    for iter_num, batch in enumerate(train_loader):
        if max_iters is not None and iter_num >= max_iters:
            break
        if args.dataset == 'nba':
            model.set_data_nba(batch)
        else:
            batch = list(batch)
            batch.pop()                                            # seq_name
            batch.pop()                                            # frame_idx
            obs_traj, pred_traj_gt, _, _, _, _, obs_loss_mask, pred_loss_mask = [t[0] for t in batch]
            model.set_data(batch, obs_traj, pred_traj_gt, obs_loss_mask, pred_loss_mask)
        total_loss, loss_pred, loss_recover, loss_kl, loss_diverse = model.forward()
        optimizer.zero_grad()
        total_loss.backward()
        optimizer.step()
        losses.append(float(total_loss.detach()))
        if log is not None and iter_num % getattr(args, 'iternum_print', 100) == 0:
            line = ('Epochs: {:02d}/{:02d}| It: {:04d}/{:04d} | Total loss: {:03f}| Loss_pred: {:03f}| Loss_recover: {:03f}| Loss_kl: {:03f}| '
                    'Loss_diverse: {:03f}'.format(epoch, getattr(args, 'num_epochs', 1), iter_num, total_iter_num, losses[-1], loss_pred,
                                                  loss_recover, loss_kl, loss_diverse))
            if log_grad_norm and getattr(optimizer, 'last_grad_norm', None) is not None:
                line += '| Grad norm: {:03f}| Skipped steps: {:d}'.format(float(optimizer.last_grad_norm), optimizer.skipped_steps)
            log(line)
    if scheduler is not None:
        scheduler.step()
    model.step_annealer()
    return losses


def train_sampler_epoch(args, epoch, model, sampler, optimizer, scheduler, train_loader, div_cfg, log=print, max_iters=None, recon=False,
                        energy_weight=0.0, energy_kind='ade', joint=False):
    """One epoch of stage 2, trainsampler.py:124-194: the prediction model stays frozen, ``optimizer`` steps the sampler's parameters
    (trainsampler.py:283) on compute_sampler_loss (samplerloss.py:41-73) through Sampler.forward's autograd path (csrc/train*.hip +
    csrc/sampler.hip).  NBA: loader yields seq_collate dicts; otherwise the per-scene tuples of TrajectoryDataset / SDD_Dataset wrapped by
    DataLoader(batch_size=1).  recon / energy_weight / energy_kind: the opt-in ground-truth terms of compute_sampler_loss,
    handed through; a term that is on joins the printed line.  joint=True: the scene-level forms of the diversity, reconstruction and energy
    terms, the step's scene as one segment, an NBA batch as one segment per game of N agents.  Returns the list of total
    losses."""
    from . import samplerloss
    terms = dict(recon=recon, energy_weight=energy_weight, energy_kind=energy_kind)
    total_iter_num = len(train_loader)
    losses = []
    for iter_num, batch in enumerate(train_loader):
        if max_iters is not None and iter_num >= max_iters:
            break
        model.decoder.train()
        if args.dataset == 'nba':
            model.set_data_nba(batch)
            dec_motion, sampler_dist, vae_dist, _ = sampler.forward(model)
            B, N = batch['past_traj'].shape[:2]
            fut = torch.as_tensor(batch['future_traj'], dtype=torch.float32).to(sampler.device).reshape(B * N, args.future_length, 2)
            total_loss, loss_dict, loss_dict_uw = samplerloss.compute_sampler_loss_nba(
                args, fut, dec_motion.reshape(-1, sampler.nk, args.future_length, 2), 1, vae_dist, sampler_dist, div_cfg, **terms,
                **(dict(joint=True, seg_len=N) if joint else {}))
        else:
            batch = list(batch)
            batch.pop()                                            # seq_name
            batch.pop()                                            # frame_idx
            obs_traj, pred_traj_gt, _, _, _, _, obs_loss_mask, pred_loss_mask = [t[0] for t in batch]
            model.set_data(batch, obs_traj, pred_traj_gt, obs_loss_mask, pred_loss_mask)
            dec_motion, sampler_dist, vae_dist, _ = sampler.forward(model)
            fut = torch.as_tensor(pred_traj_gt, dtype=torch.float32).to(sampler.device).transpose(1, 2)   # [N 2 T] -> [N T 2]
            total_loss, loss_dict, loss_dict_uw = samplerloss.compute_sampler_loss(args, fut, dec_motion, 1, pred_loss_mask, vae_dist,
                                                                                    sampler_dist, div_cfg, **terms,
                                                                                    **(dict(joint=True) if joint else {}))
        optimizer.zero_grad()
        total_loss.backward()
        optimizer.step()
        losses.append(float(total_loss.detach()))
        if log is not None and iter_num % getattr(args, 'iternum_print', 100) == 0:
            log('Epochs: {:02d}/{:02d}| It: {:04d}/{:04d} | Total loss: {:03f}| kld: {:03f}| diverse: {:03f}'.format(
                epoch, getattr(args, 'num_epochs', 1), iter_num, total_iter_num, losses[-1], float(loss_dict['kld']),
                float(loss_dict['diverse'])) + ('| recon: {:03f}'.format(float(loss_dict['recon'].detach())) if recon else '')
                + ('| energy: {:03f}'.format(float(loss_dict['energy'].detach())) if 'energy' in loss_dict else ''))
    if scheduler is not None:
        scheduler.step()
    sampler.step_annealer()
    return losses


def save_checkpoint(path, args, model, optimizer, scheduler, epoch):
    """train.py:208-213 layout: test.py:675-678 loads ``model_cfg`` / ``model_dict`` from it."""
    torch.save({'model_dict': model.state_dict(), 'optimizer': optimizer.state_dict(),
                'scheduler': scheduler.state_dict() if scheduler is not None else None, 'epoch': epoch + 1, 'model_cfg': args}, path)


def rotate_scene_batch(past, future, scene_ptr, theta):
    """Train-mode augmentation of model/STTODE.py:419-426 for a CSR batch of scenes (``STTODENet.set_scene_batch``): scene s is
    rotated by ``theta[s]`` about its own origin (the mean of its agents' last observed positions).  past [n,Tp,2],
    future [n,Tf,2], scene_ptr [S+1], theta [S]; data preparation with torch ops on whatever device the tensors live on."""
    ptr = torch.as_tensor(scene_ptr, dtype=torch.long, device=past.device)
    counts = ptr[1:] - ptr[:-1]
    S = counts.numel()
    sid = torch.repeat_interleave(torch.arange(S, device=past.device), counts)
    orig = torch.zeros(S, 2, dtype=past.dtype, device=past.device).index_add_(0, sid, past[:, -1]) / counts[:, None].to(past.dtype)
    th = torch.as_tensor(theta, dtype=past.dtype, device=past.device)
    c, s = torch.cos(th)[sid], torch.sin(th)[sid]                     # per agent
    o = orig[sid][:, None, :]

    def rot(x):
        d = x - o
        return torch.stack((d[..., 0] * c[:, None] - d[..., 1] * s[:, None], d[..., 0] * s[:, None] + d[..., 1] * c[:, None]), dim=-1) + o
    return rot(past), (rot(future) if future is not None else None)
