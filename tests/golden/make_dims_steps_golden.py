#!/usr/bin/env python3
"""Golden vectors for the TRAINING STEP at the non-default hyper-parameters that tests/golden/dims.npz records on inference() only
(helpers.DIMS_STEP_CASES: num_decompose 1 and 5, past_length 20, future_length 60 and 36, zdim 64, the mixed case).  One ETH scene and one
NBA batch per case through the IMPORTED reference: ``forward()``'s five values, and after ``backward()`` the digest of every parameter
gradient (make_golden.grad_summary) or a ``nograd::`` marker.  Only what the reference writes: inputs and noises are regenerated from
seeds by helpers.dims_case_inputs, weights by the NumPy recipe ``make_weights(seed, **hyper-parameters)``.  dims.npz is not touched.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_dims_steps_golden.py        (authoring container only)
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)


def main():
    from make_golden import NoiseQueue, grad_summary, install_shims
    install_shims()
    from model.STTODE import STTODENet
    from sttode_amd.weights import to_torch_state_dict
    noise = NoiseQueue()
    out = {}
    sys.path.insert(0, os.path.join(os.path.dirname(HERE)))          # tests/helpers.py: the case table, shared with the tests
    from helpers import DIMS_STEP_CASES, dims_case_inputs, dims_case_weights
    for tag in DIMS_STEP_CASES:
        for dataset in ('eth', 'nba'):
            a, inputs, _, (e_q, e_p, e20) = dims_case_inputs(tag, dataset)
            Tp, Tf = a.past_length, a.future_length
            m = STTODENet(a, torch.device('cpu')).eval()
            m.load_state_dict(to_torch_state_dict(dims_case_weights(a)), strict=True)
            k = f'{tag}_{dataset}_'
            m.zero_grad()
            if dataset == 'eth':
                o, p = inputs
                n = o.shape[0]
                m.set_data(None, torch.from_numpy(o), torch.from_numpy(p), torch.ones(n, Tp), torch.ones(n, Tf))
            else:
                m.set_data_nba({kk: (torch.from_numpy(v) if isinstance(v, np.ndarray) else v) for kk, v in inputs.items()})
            noise.push(e_q, e_p, e20)
            vals = m()                                                    # forward(): (total, loss_pred, loss_recover, loss_kl, loss_diverse)
            vals[0].backward()
            out[k + 'losses'] = np.array([float(vals[0].detach())] + [float(v) for v in vals[1:]], np.float64)
            for name, prm in m.named_parameters():
                if prm.grad is None:
                    out[f'{k}nograd::{name}'] = np.int64(1)
                else:
                    out[f'{k}grad::{name}'] = grad_summary(prm.grad)
    assert not noise.q
    path = os.path.join(HERE, 'dims_steps.npz')
    np.savez_compressed(path, **out)
    print('dims_steps.npz bytes:', os.path.getsize(path), 'cases:', len(DIMS_STEP_CASES))


if __name__ == '__main__':
    main()
