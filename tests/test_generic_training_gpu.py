"""The training step of the GENERIC form (sttode_amd/generic.py, sttode_amd/training.py) at every width ``generic.unsupported_reason``
accepts and tests/test_gpu_parity.py::test_non_default_hyperparameters_training_step_vs_reference leaves out (run on a real MI355X:
``pytest -m gpu``).  Every kernel underneath has a float64 test of its own; what is held here is the host-side composition -- offsets,
leading dimensions, which buffer carries the running sum, which rows are gathered -- against the float64 autograd of the oracle, with that
test's comparison and bound (test_gpu_parity._dims_training_step: err_hip <= max(6 err_fp32_autograd, 5e-4 max|g64|) per parameter, the
five values against the imported reference at rtol 1e-4).  What each case of helpers.DIMS_STEP_CASES is there for:

    nd1       one block: sttode_decoder_inputs with a null second block, prediction / reconstruction summed against zeros, d recover handed
              straight to block 0, 70 parameters with a gradient
    nd5       five blocks: 41 tape tensors (45 without the per-agent GRU) in decoder_live, i.e. a SECOND sttode_live_rows_gather launch
    tp20      past_length 20: the decoder's conv / GRU-sequence / tlinear_bwd chain on tapes [20, m, 384]
    tf60      future_length 60: a 120-column objective, the future trunk at T = 60
    zd64      zdim 64: the cat(pf | z | state) offsets PFW / ST / IN of decoder_inputs, rows_copy, rows_reduce and the dz slice
    tf36_tp8  fused inference, but the layer-by-layer trunk in training (T > 12) on D = 64
    mix       hidden_dim 32, zdim 16, three blocks, short windows: also the batched-scene step and the captured step below

Worst err_hip / max|g64| over the parameters of a step, MEASURED ON AN MI355X (a record, not a bound), beside the oracle's own fp32
autograd on the same graph:

    case        eth: HIP     fp32 autograd      nba: HIP     fp32 autograd
    nd1          8.6e-06     6.2e-06            7.0e-06     1.1e-05
    tp20         6.8e-05     3.5e-05            1.9e-03     1.5e-03
    tf60         1.0e-04     6.8e-05            1.5e-04     5.4e-04
    zd64         1.9e-05     1.0e-05            1.6e-05     6.3e-05
    tf36_tp8     2.7e-05     1.2e-05            5.4e-05     1.2e-04
    mix          7.8e-06     5.0e-06            1.5e-04     1.0e-04
    nd5          2.3e-05     8.9e-06            6.4e-04     1.7e-04
    mix, three scenes in one batch (against the summed per-scene steps):  4.7e-06     5.1e-06

The three backward forms of nd1 / nd3 / nd5 give the figures of their case to two digits (nd3, eth: 4.3e-04 against 5.3e-03).  Before the
lifetime fix in decoder_fwd (see test_operands_of_grouped_launches_outlive_their_group), nd1 eth as the first step of a process: 2.1e-03.
"""
import numpy as np
import pytest
import torch

from helpers import DIMS_GRAD_CASES, DIMS_STEP_CASES, dims_case_args, dims_case_inputs, dims_case_weights
from test_gpu_parity import _dims_grads_vs_float64, _dims_model, _dims_oracle_steps, _dims_training_step, _gpu

pytestmark = pytest.mark.gpu

_ORACLE = {}


def _oracle_steps(tag, dataset, a, inputs, eps):
    """The oracle's fp32 and float64 steps of one case: computed once, shared by the tests below, never modified."""
    key = (tag, dataset)
    if key not in _ORACLE:
        _ORACLE[key] = _dims_oracle_steps(a, dataset, inputs, eps)
    return _ORACLE[key]


def _reference_losses(golden, tag, dataset):
    """The imported reference's five values: tests/golden/dims.npz holds those of DIMS_GRAD_CASES, dims_steps.npz the others."""
    return golden('dims' if tag in DIMS_GRAD_CASES else 'dims_steps')[f'{tag}_{dataset}_losses']


@pytest.mark.parametrize('dataset', ['eth', 'nba'])
@pytest.mark.parametrize('tag', list(DIMS_STEP_CASES))
def test_generic_training_step_vs_reference_and_float64(golden, tag, dataset):
    """(a) forward() + backward() at the widths whose gradients nothing pinned: the five values against the imported reference
    (tests/golden/dims_steps.npz), every parameter gradient against the oracle's float64 autograd, a parameter without a gradient there has
    none here (or exact zeros), as many parameters compared as the float64 oracle gives a gradient (70 / 88 / 106 / 142 for one / two /
    three / five blocks: counted, not assumed), and the no-grad forward() returns the same five values."""
    from sttode_amd import generic
    m, a, inputs, _, eps = _dims_model(tag, dataset)
    assert generic.unsupported_reason(a) is None and m._generic == (tag != 'tf36_tp8')
    ora = _oracle_steps(tag, dataset, a, inputs, eps)
    _, _, checked, worst = _dims_training_step(m, dataset, inputs, eps, _reference_losses(golden, tag, dataset), f'dims_{tag}_{dataset}_', ora)
    assert checked == sum(v is not None for v in ora[True][0].values())       # (one block 70, two 88, three 106, five 142)
    print(f'{tag}_{dataset}: {checked} parameters, worst err_hip / max|g64| {worst:.2e}')


@pytest.mark.parametrize('tag', ['nd1', 'nd3', 'nd5'])
def test_three_backward_forms_at_one_three_and_five_blocks(golden, monkeypatch, tag):
    """(b) The dense backward over all 21 columns per agent, the live-column backward, and the live-column backward with the first block's
    conv + GRU once per agent: each against the float64 oracle on its own (no bound between two forms of the code under test: at these
    widths activations reach 1e3 with cancellation), the five values of the three forms within rtol 1e-6 of one another.  Five blocks: the
    live forms gather 45 / 41 tape tensors, 32 per launch -- sttode_live_rows_gather must have run exactly twice per step, and never in the
    dense form; one and three blocks (5 and 23 tensors): once."""
    from sttode_amd import STTODENet, capi, training
    from sttode_amd.weights import to_torch_state_dict
    a, inputs, _, eps = dims_case_inputs(tag, 'eth')
    ora = _oracle_steps(tag, 'eth', a, inputs, eps)
    ref_losses = _reference_losses(golden, tag, 'eth')
    calls = []
    real_call = capi.call

    def counting_call(name, *args, **kw):
        calls.append(name)
        return real_call(name, *args, **kw)
    monkeypatch.setattr(capi, 'call', counting_call)
    losses = {}
    saved = training._LIVE_COLUMNS, training._AGENT_GRU
    try:
        for live, agent in ((False, False), (True, False), (True, True)):
            training._LIVE_COLUMNS, training._AGENT_GRU = live, agent
            m = STTODENet(a, _gpu()).eval()
            m.load_state_dict(to_torch_state_dict(dims_case_weights(a)), strict=True)
            m.train_graphs = False
            del calls[:]
            losses[(live, agent)], _, checked, _ = _dims_training_step(m, 'eth', inputs, eps, ref_losses, f'dims_{tag}_eth_live{int(live)}_agent{int(agent)}_',
                                                                       ora, no_grad_too=False)
            gathers = calls.count('sttode_live_rows_gather')
            items = (9 * a.num_decompose - (4 if agent else 0)) if live else 0       # tape tensors decoder_live gathers (training.py)
            assert gathers == -(-items // training._GATHER_MAX), (tag, live, agent, gathers)
            assert checked == sum(v is not None for v in ora[True][0].values())
    finally:
        training._LIVE_COLUMNS, training._AGENT_GRU = saved
    if tag == 'nd5':
        assert training._GATHER_MAX == 32                           # (45 and 41 tensors: two launches each, as asserted above)
    for key in ((True, False), (True, True)):
        np.testing.assert_allclose(losses[key], losses[(False, False)], rtol=1e-6)


def test_batched_scene_step_at_a_generic_width_equals_sum_of_oracle_steps():
    """(c) set_scene_batch + forward() + backward() over scenes of 1, 2 and 3 agents at the 'mix' widths (hidden_dim 32, zdim 16, three
    blocks, Tp 6, Tf 9): the objective is the sum of the per-scene objectives (per-scene KL clamp, per-scene mean of the best-of-20 term), so
    the five values equal the sums of the float64 oracle's per-scene steps at rtol 1e-4 and every gradient the sum of its per-scene float64
    gradients, measured by the sum of the fp32 oracle's (the structure of test_batched_scene_training_step_equals_sum_of_per_scene_steps,
    with the oracle in place of the device's own per-scene steps)."""
    from sttode_amd import STTODENet, scenes
    from sttode_amd.weights import to_torch_state_dict
    from test_oracle_golden import _oracle_step
    a = dims_case_args('mix', 'eth')
    Tp, Tf, zd = a.past_length, a.future_length, a.zdim
    assert (Tp, Tf, zd, a.hidden_dim, a.num_decompose) == (6, 9, 16, 32, 3)
    sizes = (1, 2, 3)
    rng = np.random.default_rng(4500)
    sc = [scenes.eth_scene(7400 + i, n_min=n, n_max=n, obs_len=Tp, pred_len=Tf) for i, n in enumerate(sizes)]
    eps = [tuple(rng.standard_normal(s).astype(np.float32) for s in ((n, zd), (n, zd), (n * 20, zd))) for n in sizes]
    sums = {}
    for dbl in (False, True):
        lsum, gsum = np.zeros(5), None
        for inputs, e in zip(sc, eps):
            g, l = _oracle_step(a, 'eth', inputs, e, dbl)
            lsum += np.array(l)
            gsum = g if gsum is None else {k: (v if g[k] is None else g[k] if v is None else v + g[k]) for k, v in gsum.items()}
        sums[dbl] = (gsum, lsum)
    m = STTODENet(a, _gpu()).eval()
    m.load_state_dict(to_torch_state_dict(dims_case_weights(a)), strict=True)
    assert m._generic
    past = np.concatenate([o.transpose(0, 2, 1) for o, _ in sc])
    fut = np.concatenate([p.transpose(0, 2, 1) for _, p in sc])
    ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    cat = [torch.from_numpy(np.concatenate([e[i] for e in eps])) for i in range(3)]
    m.zero_grad()
    m.set_scene_batch(torch.from_numpy(past), torch.from_numpy(fut), torch.from_numpy(ptr))
    out = m.forward(*cat)
    got_l = [float(out[0].detach())] + list(out[1:])
    print('batched mix step:', got_l, 'float64 oracle sum:', list(sums[True][1]))
    np.testing.assert_allclose(got_l, sums[True][1], rtol=1e-4)
    out[0].backward()
    got = {k: (q.grad.detach().clone() if q.grad is not None else None) for k, q in m.named_parameters()}
    checked, worst = _dims_grads_vs_float64(got, sums[False][0], sums[True][0], 'dims_mix_scene_batch_')
    assert checked == sum(v is not None for v in sums[True][0].values())
    print(f'mix scene batch: {checked} parameters, worst err_hip / max|g64| {worst:.2e}')
    with torch.no_grad():                                           # the value path agrees on the batched objective
        m.set_scene_batch(torch.from_numpy(past), torch.from_numpy(fut), torch.from_numpy(ptr))
        v = m.forward(*cat)
    np.testing.assert_allclose([float(v[0])] + list(v[1:]), sums[True][1], rtol=1e-4)


def test_captured_step_at_a_generic_width_replays_the_eager_step(golden):
    """(d) ``train_graphs`` at its default on the 'mix' NBA case: the first forward() / backward() pair runs eagerly, the second, on the same
    inputs and noises, is captured into a graph and replayed.  Both pass the comparison of (a), and the replay gives the eager step's bits
    in the five values and in every gradient."""
    m, a, inputs, _, eps = _dims_model('mix', 'nba')
    ora = _oracle_steps('mix', 'nba', a, inputs, eps)
    ref_losses = _reference_losses(golden, 'mix', 'nba')
    steps = []
    for i in range(2):
        losses, got, checked, _ = _dims_training_step(m, 'nba', inputs, eps, ref_losses, f'dims_mix_nba_captured_step{i}_', ora, no_grad_too=False)
        assert checked == sum(v is not None for v in ora[True][0].values())
        steps.append((losses, got))
        assert len(m._graphs) == i                                  # eager, then one captured step
    assert steps[0][0] == steps[1][0], (steps[0][0], steps[1][0])
    for name, g0 in steps[0][1].items():
        g1 = steps[1][1][name]
        assert (g0 is None) == (g1 is None) and (g0 is None or torch.equal(g0, g1)), name


@pytest.mark.parametrize('tag,dataset', [('nd1', 'eth'), ('nd3', 'eth'), ('mix', 'nba')])
def test_operands_of_grouped_launches_outlive_their_group(golden, monkeypatch, tag, dataset):
    """What Engine.group() queues is launched when the group closes, with raw pointers: a tensor handed to a call inside a group and dropped
    before the group closes leaves its memory to the next allocation inside the group, and two pieces of one launch then share it.  With
    one block, decoder_fwd handed its sums temporaries of zeros: on the first step of a process the reconstruction got the memory of the
    prediction's zeros, and the gradients of the block's conv / GRU / decoder_y were off by up to 2e-3 of max|g| (found by
    test_generic_training_step_vs_reference_and_float64[nd1-eth] as the first test of a process; whether the values show it depends on
    the allocator's state and on timing).  This holds the rule itself, which depends on neither: through a whole forward() + backward(),
    every tensor passed to an entry point inside an open group (its base, for a view) is still referenced when the group closes."""
    import weakref
    from sttode_amd import capi
    m, a, inputs, _, eps = _dims_model(tag, dataset)
    m.train_graphs = False
    real_call = capi.call
    pending, dropped, groups = None, [], 0

    def watching_call(name, *args, **kw):
        nonlocal pending, groups
        if name == 'sttode_tgemm_group':
            if args[0] > 0:
                pending = []
            else:
                if pending is not None:
                    groups += 1
                    dropped.extend((nm, i) for nm, i, ref in pending if ref() is None)
                pending = None
        elif pending is not None:
            for i, t in enumerate(args):
                if isinstance(t, torch.Tensor):
                    pending.append((name, i, weakref.ref(t if t._base is None else t._base)))
        return real_call(name, *args, **kw)
    monkeypatch.setattr(capi, 'call', watching_call)
    try:
        _dims_training_step(m, dataset, inputs, eps, _reference_losses(golden, tag, dataset), f'dims_{tag}_{dataset}_lifetimes_',
                            _oracle_steps(tag, dataset, a, inputs, eps), no_grad_too=False)
    finally:                                                        # (first: it names the cause of whatever the step's values show)
        assert groups >= 6 and not dropped, (groups, sorted(set(dropped)))
