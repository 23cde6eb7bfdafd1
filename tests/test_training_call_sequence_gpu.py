"""The calls one eager training step makes, pinned: forward plus backward with ``train_graphs = False`` on every trunk path
of training.Engine -- the fused trunk launches, the default layer-by-layer walk, the stage program fused and layer by layer with its
chunked deferred weight gradients, the generic widths -- and one stage-2 sampler step.  Per call: the entry point (without its
``sttode_`` prefix), for sttode_tgemm_group, sttode_train_ewise and sttode_twgrad_defer their first integer argument (the bracket and the op
code: where grouping and order live), and which arguments were tensors ('t'), None ('-'), numbers ('.') or host tables ('p'), the stream
left out.  Pointer-valued integers count as numbers; their values are not recorded.

EXPECTED was recorded by running ``sequences`` below against the sttode_amd package of the commit BEFORE the engine's two encoder-layer
forwards, two VJPs, four state dicts, two MLP walks and five attention calls were merged into one each (that tree from ``git archive``,
this file's ``sequences``, on an MI355X on the same built library through STTODE_HIP_LIB; a run on a host without a GPU, with capi.call
replaced by a recorder that launches nothing, gives the same literal -- a step's control flow does not depend on device values): the merge must not change which entry points a step calls, in
which order, in which groups or with which kinds of arguments.  The literal keeps each distinct call once (CALLS) and a step as indices.

Shapes: the smallest that take each branch -- one ETH scene of 3 agents (attention length 1), an NBA batch of 3 x 4 (attention over the
batch, length 3), the generic cases' 6 agents."""
import pytest
import torch

pytestmark = pytest.mark.gpu

_FIRST_INT = ('sttode_tgemm_group', 'sttode_train_ewise', 'sttode_twgrad_defer')
_NO_STREAM = ('sttode_tgemm_group', 'sttode_twgrad_defer', 'sttode_twgrad_flush')


def _kind(a):
    return 't' if isinstance(a, torch.Tensor) else '-' if a is None else '.' if isinstance(a, (int, float)) else 'p'


def sequences(pkg, dev):
    """{case: ['entry [first int] kinds', ...]} of one eager forward plus backward per case, recorded by a pass-through around capi.call.
    ``pkg``: the sttode_amd package under test."""
    from helpers import dims_case_inputs, dims_case_weights, make_args, sampler_args
    from importlib import import_module
    capi, scenes, training, weights = (import_module(f'{pkg.__name__}.{k}') for k in ('capi', 'scenes', 'training', 'weights'))
    calls = []
    real = capi.call

    def recording(name, *args, **kw):
        rec = name[len('sttode_'):]
        if name in _FIRST_INT:
            rec += f' {int(args[0])}'
        calls.append(rec + ' ' + ''.join(_kind(a) for a in (args if name in _NO_STREAM else args[:-1])))
        return real(name, *args, **kw)

    def model(a, w):
        m = pkg.STTODENet(a, dev).eval()
        m.load_state_dict(weights.to_torch_state_dict(w), strict=True)
        m.train_graphs = False
        return m

    def reference_model(ds, Tp, Tf):
        return model(make_args(ds, Tp, Tf), weights.make_weights(1234, past_length=Tp, future_length=Tf))

    def feed(m, ds, Tp, Tf):
        if ds == 'eth':
            ob, pr = scenes.eth_scene(41, obs_len=Tp, pred_len=Tf, n_min=3, n_max=3)
            m.set_data(None, torch.from_numpy(ob), torch.from_numpy(pr))
        else:
            d = scenes.nba_batch(41, 3, N=4, obs_len=Tp, pred_len=Tf)
            m.set_data_nba({k: (torch.from_numpy(v) if hasattr(v, 'shape') else v) for k, v in d.items()})

    def step(m, eps, drop=(None, None)):
        m.zero_grad()
        del calls[:]
        vals = m.forward(eps_q=eps[0], eps_p=eps[1], eps20=eps[2], drop_past=drop[0], drop_future=drop[1])
        vals[0].backward()
        return list(calls)

    def reference_step(ds, Tp, Tf, ode=('euler', 1), fused=True, chunk=None):
        m = reference_model(ds, Tp, Tf)
        m.ode_method, m.ode_steps = ode
        feed(m, ds, Tp, Tf)
        n = m._past.shape[0]
        gen = torch.Generator().manual_seed(17)
        eps = [torch.randn(r, 32, generator=gen) for r in (n, n, n * 20)]
        drop = [(torch.rand(n * T, 64, generator=gen) < 0.9).float() / 0.9 for T in (Tp, Tf)]
        was = training._ode_chunk_stages
        if chunk is not None:
            training._ode_chunk_stages = lambda nst, per_stage: chunk
        try:
            m.forward(eps_q=eps[0], eps_p=eps[1], eps20=eps[2])        # builds the engine, whose switch the case sets
            m._engine.fused_trunk = fused
            return step(m, eps, drop)
        finally:
            training._ode_chunk_stages = was

    def generic_step(tag):
        a, inputs, _, eps = dims_case_inputs(tag, 'eth')
        m = model(a, dims_case_weights(a))
        m.set_data(None, torch.from_numpy(inputs[0]), torch.from_numpy(inputs[1]))
        return step(m, [torch.from_numpy(e) for e in eps])

    def sampler_step():
        m = reference_model('eth', 8, 12)
        smp = pkg.Sampler(sampler_args('eth', 8, 12))
        smp.load_state_dict(weights.to_torch_state_dict(weights.make_sampler_weights()), strict=True)
        smp.set_device(dev)
        smp.train()
        feed(m, 'eth', 8, 12)
        del calls[:]
        dec, q, _, _ = smp.forward(m, mean=True)
        (dec.sum() + q.mu.sum() + q.logvar.sum()).backward()
        return list(calls)

    eth, nba = ('eth', 8, 12), ('nba', 5, 10)
    out = {}
    capi.call = recording
    try:
        out['eth fused'] = reference_step(*eth)
        out['eth layer by layer'] = reference_step(*eth, fused=False)
        out['nba fused'] = reference_step(*nba)
        out['nba layer by layer'] = reference_step(*nba, fused=False)
        out['eth rk4 x1 fused'] = reference_step(*eth, ode=('rk4', 1))
        out['eth rk4 x1 layer by layer'] = reference_step(*eth, ode=('rk4', 1), fused=False)
        out['nba rk4 x2'] = reference_step(*nba, ode=('rk4', 2))
        out['nba rk4 x2 chunks of 3'] = reference_step(*nba, ode=('rk4', 2), chunk=3)
        out['generic hd32'] = generic_step('hd32')
        out['generic nd1'] = generic_step('nd1')
        out['sampler mean'] = sampler_step()
    finally:
        capi.call = real
    torch.cuda.synchronize()
    return out


# the distinct calls of all cases, in the order of their first appearance
CALLS = (
    'frontend_scenes tt.....ttttttt', 'frontend_future tt....tttt', 'tgemm_group 1 .', 'ttrunk_fwd p......', 'tgemm_group 0 .',
    'tlinear t..t..t-.t......', 'train_ewise 5 .ttt--...', 'decoder_inputs tt.t.tt....', 'conv_fwd t.-tttt..', 'gru_seq_fwd tttttt...',
    'rows_copy t.t.....', 'conv_fwd t.ttttt..', 'train_ewise 12 .tttt-...', 'train_ewise 12 .ttt--...',
    'loss_objective_live ttttt--..........tttttt.', 'live_rows_gather p.t..', 'tlinear_bwd t.t.t.t...t..t.t...t.',
    'tlinear_bwd t.t.-.t...t..t.t...t.', 'gru_seq_bwd t.ttttt..', 'twgrad t.t..t.t...t.', 'conv_bwd tttttt..t.', 'train_ewise 14 .tt---...',
    'rows_reduce t.t.....', 'conv_bwd ttt-tt..t.', 'train_ewise 1 .tt---...', 'train_ewise 8 .tttt-...', 'train_ewise 15 .tt---...',
    'train_ewise 13 .tt-tt...', 'ln_bwd ttttttt..t.', 'train_ewise 2 .ttttt...', 'train_ewise 0 .ttt--...', 'twgrad_defer 0 .-.',
    'add_ln_fwd ttttttt..', 'train_ewise 3 .ttt--...', 'frontend_nba t....ttttt', 'frontend_future tt....---t',
    'mhgsa_attn_groups ...t...................', 'twgrad_defer 1 .t.', 'mhgsa_attn_bwd ttt...', 'ttrunk_ode_fwd p..pppppp', 'ode_combine p..',
    'ode_stage_bwd p.', 'tlinear t..t..-t.t......', 'tlinear t..t..--.t......', 'decoder_inputs t-.t.tt....', 'embed_qkv ttttttttttttttt..',
    'post_attn ttttttttttttttt..t..', 'linear_cols t..t..ttt....', 'linear_cols t..-..ttt....', 'sampler_latent tt-.tt...', 'gru_cols ttttttt...',
    'agent_preact ttttttttttt.', 'mlp_block0 ttt.tttt....', 'mlp_block1 tt.tttttt....', 'mlp_cols tt.ttt...', 'train_ewise 14 .t----...',
    'train_ewise 11 .ttt-t...', 'train_ewise 10 .ttt--...',
)
# per case: the step's calls in order, as indices into CALLS
EXPECTED = {
    'eth fused':
        '0 1 2 3 3 4 5 5 6 7 8 5 9 10 2 5 5 4 2 5 5 4 2 5 5 4 11 5 9 2 5 5 4 2 5 5 4 2 5 5 4 2 12 13 4 14 15 2 16 16 4 2 16 16 4 17 17 18 19 16 20 21 '
        '2 16 16 4 2 16 16 4 17 17 22 18 19 16 23 24 22 10 25 16 17 26 2 27 27 4 28 28 2 16 16 4 2 17 17 4 28 28 2 24 29 24 29 4 2 17 17 4 2 17 17 4 '
        '2 17 17 4 2 17 17 4 2 17 17 4 2 17 17 4 2 30 30 4 2 17 17 4 2 19 19 4 31',
    'eth layer by layer':
        '0 1 2 5 5 4 10 10 2 5 5 4 2 30 30 4 2 5 5 4 2 5 5 4 2 5 5 4 2 5 5 4 2 5 5 5 5 4 2 30 30 4 32 32 2 5 5 4 2 5 5 4 32 32 2 33 33 4 5 5 6 7 8 5 '
        '9 10 2 5 5 4 2 5 5 4 2 5 5 4 11 5 9 2 5 5 4 2 5 5 4 2 5 5 4 2 12 13 4 14 15 2 16 16 4 2 16 16 4 17 17 18 19 16 20 21 2 16 16 4 2 16 16 4 17 '
        '17 22 18 19 16 23 24 22 10 25 16 17 26 2 27 27 4 28 28 2 16 16 4 2 17 17 4 28 28 2 24 29 24 29 4 2 17 17 4 2 17 17 4 2 17 17 4 2 17 17 4 2 '
        '17 17 4 2 17 17 4 2 30 30 4 2 17 17 4 2 19 19 4 31',
    'nba fused':
        '34 35 2 3 3 4 36 36 2 3 3 4 5 5 6 7 8 5 9 10 2 5 5 4 2 5 5 4 2 5 5 4 11 5 9 2 5 5 4 2 5 5 4 2 5 5 4 2 12 13 4 14 37 15 2 16 16 4 2 16 16 4 '
        '17 17 18 19 16 20 21 2 16 16 4 2 16 16 4 17 17 22 18 19 16 23 24 22 10 25 16 17 26 2 27 27 4 28 28 2 16 16 4 2 17 17 4 28 28 2 24 29 24 29 4 '
        '2 17 17 4 2 17 17 4 2 17 17 4 38 38 2 17 17 4 2 17 17 4 2 17 17 4 2 30 30 4 2 17 17 4 2 19 19 4 31',
    'nba layer by layer':
        '34 35 2 5 5 4 10 10 2 5 5 4 2 30 30 4 2 5 5 4 2 5 5 4 2 5 5 4 36 36 2 5 5 4 2 5 5 5 5 4 2 30 30 4 32 32 2 5 5 4 2 5 5 4 32 32 2 33 33 4 5 5 '
        '6 7 8 5 9 10 2 5 5 4 2 5 5 4 2 5 5 4 11 5 9 2 5 5 4 2 5 5 4 2 5 5 4 2 12 13 4 14 37 15 2 16 16 4 2 16 16 4 17 17 18 19 16 20 21 2 16 16 4 2 '
        '16 16 4 17 17 22 18 19 16 23 24 22 10 25 16 17 26 2 27 27 4 28 28 2 16 16 4 2 17 17 4 28 28 2 24 29 24 29 4 2 17 17 4 2 17 17 4 2 17 17 4 38 '
        '38 2 17 17 4 2 17 17 4 2 17 17 4 2 30 30 4 2 17 17 4 2 19 19 4 31',
    'eth rk4 x1 fused':
        '0 1 39 5 5 6 7 8 5 9 10 2 5 5 4 2 5 5 4 2 5 5 4 11 5 9 2 5 5 4 2 5 5 4 2 5 5 4 2 12 13 4 14 15 2 16 16 4 2 16 16 4 17 17 18 19 16 20 21 2 16 '
        '16 4 2 16 16 4 17 17 22 18 19 16 23 24 22 10 25 16 17 26 40 41 41 41 41 2 19 19 4 2 19 19 4 2 19 19 4 2 19 19 4 2 19 19 4 22 22 22 22 22 22 '
        '22 22 2 19 19 4 2 17 17 4 2 17 17 4 2 30 30 4 2 17 17 4 2 19 19 4 31',
    'eth rk4 x1 layer by layer':
        '0 1 2 5 5 4 10 10 2 5 5 4 2 30 30 4 2 5 5 4 2 5 5 4 40 2 5 5 4 2 5 5 4 2 5 5 5 5 4 2 30 30 4 32 32 2 5 5 4 2 5 5 4 32 32 40 2 5 5 4 2 5 5 4 '
        '2 5 5 5 5 4 2 30 30 4 32 32 2 5 5 4 2 5 5 4 32 32 40 2 5 5 4 2 5 5 4 2 5 5 5 5 4 2 30 30 4 32 32 2 5 5 4 2 5 5 4 32 32 40 2 5 5 4 2 5 5 4 2 '
        '5 5 5 5 4 2 30 30 4 32 32 2 5 5 4 2 5 5 4 32 32 40 5 5 6 7 8 5 9 10 2 5 5 4 2 5 5 4 2 5 5 4 11 5 9 2 5 5 4 2 5 5 4 2 5 5 4 2 12 13 4 14 15 2 '
        '16 16 4 2 16 16 4 17 17 18 19 16 20 21 2 16 16 4 2 16 16 4 17 17 22 18 19 16 23 24 22 10 25 16 17 26 40 2 5 5 4 2 5 5 4 2 5 5 5 5 4 2 30 30 '
        '4 32 32 2 5 5 4 2 5 5 4 32 32 40 28 28 2 42 42 4 2 43 43 4 2 24 24 4 28 28 2 29 29 4 2 43 43 4 2 43 43 4 2 43 43 4 2 43 43 4 2 5 5 4 2 5 5 4 '
        '2 5 5 5 5 4 2 30 30 4 32 32 2 5 5 4 2 5 5 4 32 32 40 28 28 2 42 42 4 2 43 43 4 2 24 24 4 28 28 2 29 29 4 2 43 43 4 2 43 43 4 2 43 43 4 2 43 '
        '43 4 2 5 5 4 2 5 5 4 2 5 5 5 5 4 2 30 30 4 32 32 2 5 5 4 2 5 5 4 32 32 40 28 28 2 42 42 4 2 43 43 4 2 24 24 4 28 28 2 29 29 4 2 43 43 4 2 43 '
        '43 4 2 43 43 4 2 43 43 4 2 5 5 4 2 5 5 4 2 5 5 5 5 4 2 30 30 4 32 32 2 5 5 4 2 5 5 4 32 32 40 28 28 2 42 42 4 2 43 43 4 2 24 24 4 28 28 2 29 '
        '29 4 2 43 43 4 2 43 43 4 2 43 43 4 2 43 43 4 40 2 19 19 4 2 19 19 4 2 19 19 4 2 19 19 4 2 19 19 4 2 19 19 4 2 17 17 4 2 17 17 4 2 30 30 4 2 '
        '17 17 4 2 19 19 4 31',
    'nba rk4 x2':
        '34 35 2 3 3 4 40 2 5 5 4 36 36 2 5 5 4 2 5 5 5 5 4 2 30 30 4 32 32 2 5 5 4 2 5 5 4 32 32 40 2 5 5 4 36 36 2 5 5 4 2 5 5 5 5 4 2 30 30 4 32 '
        '32 2 5 5 4 2 5 5 4 32 32 40 2 5 5 4 36 36 2 5 5 4 2 5 5 5 5 4 2 30 30 4 32 32 2 5 5 4 2 5 5 4 32 32 40 2 5 5 4 36 36 2 5 5 4 2 5 5 5 5 4 2 '
        '30 30 4 32 32 2 5 5 4 2 5 5 4 32 32 40 2 5 5 4 36 36 2 5 5 4 2 5 5 5 5 4 2 30 30 4 32 32 2 5 5 4 2 5 5 4 32 32 40 2 5 5 4 36 36 2 5 5 4 2 5 '
        '5 5 5 4 2 30 30 4 32 32 2 5 5 4 2 5 5 4 32 32 40 2 5 5 4 36 36 2 5 5 4 2 5 5 5 5 4 2 30 30 4 32 32 2 5 5 4 2 5 5 4 32 32 40 2 5 5 4 36 36 2 '
        '5 5 4 2 5 5 5 5 4 2 30 30 4 32 32 2 5 5 4 2 5 5 4 32 32 40 5 5 6 7 8 5 9 10 2 5 5 4 2 5 5 4 2 5 5 4 11 5 9 2 5 5 4 2 5 5 4 2 5 5 4 2 12 13 4 '
        '14 37 15 2 16 16 4 2 16 16 4 17 17 18 19 16 20 21 2 16 16 4 2 16 16 4 17 17 22 18 19 16 23 24 22 10 25 16 17 26 40 2 5 5 4 36 36 2 5 5 4 2 5 '
        '5 5 5 4 2 30 30 4 32 32 2 5 5 4 2 5 5 4 32 32 40 28 28 2 42 42 4 2 43 43 4 2 24 24 4 28 28 2 29 29 4 2 43 43 4 2 43 43 4 2 43 43 4 38 38 2 '
        '43 43 4 2 5 5 4 36 36 2 5 5 4 2 5 5 5 5 4 2 30 30 4 32 32 2 5 5 4 2 5 5 4 32 32 40 28 28 2 42 42 4 2 43 43 4 2 24 24 4 28 28 2 29 29 4 2 43 '
        '43 4 2 43 43 4 2 43 43 4 38 38 2 43 43 4 2 5 5 4 36 36 2 5 5 4 2 5 5 5 5 4 2 30 30 4 32 32 2 5 5 4 2 5 5 4 32 32 40 28 28 2 42 42 4 2 43 43 '
        '4 2 24 24 4 28 28 2 29 29 4 2 43 43 4 2 43 43 4 2 43 43 4 38 38 2 43 43 4 2 5 5 4 36 36 2 5 5 4 2 5 5 5 5 4 2 30 30 4 32 32 2 5 5 4 2 5 5 4 '
        '32 32 40 28 28 2 42 42 4 2 43 43 4 2 24 24 4 28 28 2 29 29 4 2 43 43 4 2 43 43 4 2 43 43 4 38 38 2 43 43 4 40 2 5 5 4 36 36 2 5 5 4 2 5 5 5 '
        '5 4 2 30 30 4 32 32 2 5 5 4 2 5 5 4 32 32 40 28 28 2 42 42 4 2 43 43 4 2 24 24 4 28 28 2 29 29 4 2 43 43 4 2 43 43 4 2 43 43 4 38 38 2 43 43 '
        '4 2 5 5 4 36 36 2 5 5 4 2 5 5 5 5 4 2 30 30 4 32 32 2 5 5 4 2 5 5 4 32 32 40 28 28 2 42 42 4 2 43 43 4 2 24 24 4 28 28 2 29 29 4 2 43 43 4 2 '
        '43 43 4 2 43 43 4 38 38 2 43 43 4 2 5 5 4 36 36 2 5 5 4 2 5 5 5 5 4 2 30 30 4 32 32 2 5 5 4 2 5 5 4 32 32 40 28 28 2 42 42 4 2 43 43 4 2 24 '
        '24 4 28 28 2 29 29 4 2 43 43 4 2 43 43 4 2 43 43 4 38 38 2 43 43 4 2 5 5 4 36 36 2 5 5 4 2 5 5 5 5 4 2 30 30 4 32 32 2 5 5 4 2 5 5 4 32 32 '
        '40 28 28 2 42 42 4 2 43 43 4 2 24 24 4 28 28 2 29 29 4 2 43 43 4 2 43 43 4 2 43 43 4 38 38 2 43 43 4 40 2 19 19 4 2 19 19 4 2 19 19 4 2 19 '
        '19 4 2 19 19 4 2 19 19 4 2 17 17 4 2 17 17 4 2 30 30 4 2 17 17 4 2 19 19 4 31',
    'nba rk4 x2 chunks of 3':
        '34 35 2 3 3 4 40 2 5 5 4 36 36 2 5 5 4 2 5 5 5 5 4 2 30 30 4 32 32 2 5 5 4 2 5 5 4 32 32 40 2 5 5 4 36 36 2 5 5 4 2 5 5 5 5 4 2 30 30 4 32 '
        '32 2 5 5 4 2 5 5 4 32 32 40 2 5 5 4 36 36 2 5 5 4 2 5 5 5 5 4 2 30 30 4 32 32 2 5 5 4 2 5 5 4 32 32 40 2 5 5 4 36 36 2 5 5 4 2 5 5 5 5 4 2 '
        '30 30 4 32 32 2 5 5 4 2 5 5 4 32 32 40 2 5 5 4 36 36 2 5 5 4 2 5 5 5 5 4 2 30 30 4 32 32 2 5 5 4 2 5 5 4 32 32 40 2 5 5 4 36 36 2 5 5 4 2 5 '
        '5 5 5 4 2 30 30 4 32 32 2 5 5 4 2 5 5 4 32 32 40 2 5 5 4 36 36 2 5 5 4 2 5 5 5 5 4 2 30 30 4 32 32 2 5 5 4 2 5 5 4 32 32 40 2 5 5 4 36 36 2 '
        '5 5 4 2 5 5 5 5 4 2 30 30 4 32 32 2 5 5 4 2 5 5 4 32 32 40 5 5 6 7 8 5 9 10 2 5 5 4 2 5 5 4 2 5 5 4 11 5 9 2 5 5 4 2 5 5 4 2 5 5 4 2 12 13 4 '
        '14 37 15 2 16 16 4 2 16 16 4 17 17 18 19 16 20 21 2 16 16 4 2 16 16 4 17 17 22 18 19 16 23 24 22 10 25 16 17 26 40 2 5 5 4 36 36 2 5 5 4 2 5 '
        '5 5 5 4 2 30 30 4 32 32 2 5 5 4 2 5 5 4 32 32 40 28 28 2 42 42 4 2 43 43 4 2 24 24 4 28 28 2 29 29 4 2 43 43 4 2 43 43 4 2 43 43 4 38 38 2 '
        '43 43 4 2 5 5 4 36 36 2 5 5 4 2 5 5 5 5 4 2 30 30 4 32 32 2 5 5 4 2 5 5 4 32 32 40 28 28 2 42 42 4 2 43 43 4 2 24 24 4 28 28 2 29 29 4 2 43 '
        '43 4 2 43 43 4 2 43 43 4 38 38 2 43 43 4 2 5 5 4 36 36 2 5 5 4 2 5 5 5 5 4 2 30 30 4 32 32 2 5 5 4 2 5 5 4 32 32 40 28 28 2 42 42 4 2 43 43 '
        '4 2 24 24 4 28 28 2 29 29 4 2 43 43 4 2 43 43 4 2 43 43 4 38 38 2 43 43 4 2 19 19 4 2 19 19 4 2 19 19 4 2 19 19 4 2 19 19 4 2 19 19 4 2 5 5 '
        '4 36 36 2 5 5 4 2 5 5 5 5 4 2 30 30 4 32 32 2 5 5 4 2 5 5 4 32 32 40 28 28 2 42 42 4 2 43 43 4 2 24 24 4 28 28 2 29 29 4 2 43 43 4 2 43 43 4 '
        '2 43 43 4 38 38 2 43 43 4 40 2 5 5 4 36 36 2 5 5 4 2 5 5 5 5 4 2 30 30 4 32 32 2 5 5 4 2 5 5 4 32 32 40 28 28 2 42 42 4 2 43 43 4 2 24 24 4 '
        '28 28 2 29 29 4 2 43 43 4 2 43 43 4 2 43 43 4 38 38 2 43 43 4 2 5 5 4 36 36 2 5 5 4 2 5 5 5 5 4 2 30 30 4 32 32 2 5 5 4 2 5 5 4 32 32 40 28 '
        '28 2 42 42 4 2 43 43 4 2 24 24 4 28 28 2 29 29 4 2 43 43 4 2 43 43 4 2 43 43 4 38 38 2 43 43 4 2 19 19 4 2 19 19 4 2 19 19 4 2 19 19 4 2 19 '
        '19 4 2 19 19 4 2 5 5 4 36 36 2 5 5 4 2 5 5 5 5 4 2 30 30 4 32 32 2 5 5 4 2 5 5 4 32 32 40 28 28 2 42 42 4 2 43 43 4 2 24 24 4 28 28 2 29 29 '
        '4 2 43 43 4 2 43 43 4 2 43 43 4 38 38 2 43 43 4 2 5 5 4 36 36 2 5 5 4 2 5 5 5 5 4 2 30 30 4 32 32 2 5 5 4 2 5 5 4 32 32 40 28 28 2 42 42 4 2 '
        '43 43 4 2 24 24 4 28 28 2 29 29 4 2 43 43 4 2 43 43 4 2 43 43 4 38 38 2 43 43 4 40 2 19 19 4 2 19 19 4 2 19 19 4 2 19 19 4 2 19 19 4 2 19 19 '
        '4 2 17 17 4 2 17 17 4 2 30 30 4 2 17 17 4 2 19 19 4 31',
    'generic hd32':
        '0 1 2 5 5 4 10 10 2 5 5 4 2 4 2 5 5 4 2 5 5 4 2 5 5 4 2 5 5 4 2 5 5 5 5 4 2 30 30 4 32 32 2 5 5 4 2 5 5 4 32 32 2 33 33 4 5 5 6 7 8 5 9 10 2 '
        '5 5 4 2 5 5 4 2 5 5 4 11 5 9 2 5 5 4 2 5 5 4 2 5 5 4 2 12 13 4 14 37 15 2 16 16 4 2 16 16 4 17 17 18 19 16 20 21 2 16 16 4 2 16 16 4 17 17 '
        '22 18 19 16 23 24 22 10 25 16 17 26 2 27 27 4 28 28 2 16 16 4 2 17 17 4 28 28 2 24 29 24 29 4 2 17 17 4 2 17 17 4 2 17 17 4 2 17 17 4 2 17 '
        '17 4 2 17 17 4 2 4 2 17 17 4 2 19 19 4 31',
    'generic nd1':
        '0 1 2 3 3 4 5 5 6 44 8 5 9 10 2 5 5 4 2 5 5 4 2 5 5 4 2 12 13 4 14 37 15 2 16 16 4 2 16 16 4 17 17 22 18 19 16 23 22 10 25 16 17 26 2 27 27 '
        '4 28 28 2 16 16 4 2 17 17 4 28 28 2 24 29 24 29 4 2 17 17 4 2 17 17 4 2 17 17 4 2 17 17 4 2 17 17 4 2 17 17 4 2 4 2 17 17 4 2 19 19 4 31',
    'sampler mean':
        '0 45 46 1 45 46 47 48 6 5 5 5 5 5 49 5 50 51 52 50 53 48 54 8 5 9 10 10 10 2 5 5 4 2 5 5 4 2 5 5 4 11 5 9 10 10 5 5 5 2 12 4 42 42 43 18 42 '
        '20 55 2 42 42 4 2 42 42 4 43 43 22 18 42 23 24 22 56 24 17 17 57 17 57 17 19',
}


def test_an_eager_step_makes_the_recorded_calls():
    import sttode_amd
    got = sequences(sttode_amd, torch.device('cuda:0'))
    assert sorted(got) == sorted(EXPECTED)
    for key, indices in EXPECTED.items():
        new, calls = got[key], [CALLS[int(i)] for i in indices.split()]
        first = next((i for i, (a, b) in enumerate(zip(new, calls)) if a != b), min(len(new), len(calls)))
        assert new == calls, f'{key}: {len(new)} calls for {len(calls)} recorded; first difference at call {first}: ' \
                             f'{new[first - 2:first + 3]} for {calls[first - 2:first + 3]}'
