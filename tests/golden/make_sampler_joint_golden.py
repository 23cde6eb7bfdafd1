#!/usr/bin/env python3
"""Generate tests/golden/sampler_joint.npz (the scene-level forms of the stage-2 sampler's terms) on the CPU with the
float64 torch restatement tests/sampler_joint_ref.py (the reference project has no joint form; tests/test_sampler_joint.py pins the
restatement against NumPy loops and central differences):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_sampler_joint_golden.py

Per (shape, mask) of sampler_joint_ref.GOLDEN_SEGS / GOLDEN_MASKS, <k.._z.._t.._mask>/...:

  motion [n,K,Tf,2], gt [n,Tf,2]   float32 inputs (sampler_joint_ref.draw; the latents are not stored: kld is sttode_sampler_loss's)
  mask [n,Tf]                      float32 zeros and ones ('ragged' only)
  seg_ptr [S+1]                    int32 CSR of the case's segments
  g_div, g_rec, g_es [S]           float32 upstream gradients
  div, rec, es [S], best [S]       float64 restatement at scale 2 (best: int64), J [S,K] its per-sample sums
  dmotion [n,K,Tf,2]               float64 gradient of sum_g (g_div div + g_rec rec + g_es es) at scale 2
  seed                             the seed whose inputs met sampler_joint_ref.conditions (asserted here and in the tests)"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import sampler_joint_ref as JR                                       # noqa: E402


def main():
    out = {}
    tags = []
    for si, shape in enumerate(JR.SHAPES):
        segs = JR.GOLDEN_SEGS[shape]
        for mk in JR.GOLDEN_MASKS[shape]:
            inp, seed = JR.make_case(shape, segs, mk, 1000 * (si + 1))
            t = JR.tag(shape, mk)
            tags.append(t)
            g = JR.upstream(inp)
            r = JR.objective(*JR.as_torch(inp, torch.float64), 2.0, g={k: g[k] for k in ('div', 'rec', 'es')})
            out[t + '/motion'], out[t + '/gt'], out[t + '/seg_ptr'] = inp['motion'], inp['gt'], inp['seg_ptr']
            if inp['mask'] is not None:
                out[t + '/mask'] = inp['mask']
            for k in ('div', 'rec', 'es'):
                out[t + '/g_' + k] = inp['g'][k]
                out[t + '/' + k] = r[k].numpy()
            out[t + '/best'], out[t + '/J'], out[t + '/dmotion'] = r['best'].numpy(), r['J'].numpy(), r['dmotion'].numpy()
            out[t + '/seed'] = np.int64(seed)
            assert (r['dmu'] == 0).all() and (r['dlogvar'] == 0).all()
    out['cases'] = np.array(tags)
    path = os.path.join(HERE, 'sampler_joint.npz')
    np.savez(path, **out)
    print(path, os.path.getsize(path), 'bytes;', len(tags), 'cases')
    assert os.path.getsize(path) <= os.path.getsize(os.path.join(HERE, 'sampler_objective.npz'))


if __name__ == '__main__':
    main()
