"""CPU: masked attention and the Euclidean dot-product baseline without a GPU.

The plain-torch restatement (tests/attention_ref.py) reproduces the reference's own outputs, weights and gradients recorded in
tests/golden/attention.npz (make_attention_golden.py) -- this pins the yardstick tests/test_attention_gpu.py holds the HIP kernels to --
and the host side of the feature: the two exports and their refusals, the drop-in modules' state_dict and constructor refusals, no CPU
fallback."""
import os

import numpy as np
import pytest
import torch

import attention_ref as AR
from helpers import assert_close, yardstick_close
from test_stack_grads_oracle import decoder_state, digest, encoder_state, fixture_grads, seeded

HERE = os.path.dirname(os.path.abspath(__file__))
PREFIX = 'cross_attn.temporal_attention_before.'
MODES = {'hyp': 0, 'euc': 1}
MODULE_CASES = ['self_none', 'self_rand', 'self_causal', 'kv_none', 'kv_rand', 'kv_causal', 'eq_rand', 'eq_causal', 'lead_lead']
FORWARD_CASES = ['hyp_nanrow', 'euc_nanrow', 'euc_overflow']


@pytest.fixture(scope='module')
def g():
    return np.load(os.path.join(HERE, 'golden', 'attention.npz'))


def attn_state():
    return {k[len(PREFIX):]: v for k, v in decoder_state().items() if k.startswith(PREFIX)}


def case_inputs(g, tag):
    """(inputs, mask | None, G) of a fixture case: inputs and G drawn from the recorded seed, scaled where the case says so."""
    seed = int(g[f'{tag}_seed'])
    scale = np.float32(g[f'{tag}_scale']) if f'{tag}_scale' in g.files else np.float32(1.0)
    inputs = [seeded(seed + 1 + i, sh) * scale for i, sh in enumerate(g[f'{tag}_shapes'])]
    mask = g[f'{tag}_mask'] if f'{tag}_mask' in g.files else None
    return inputs, mask, seeded(seed, g[f'{tag}_out'].shape)


def qkv(xs):
    """The fixture's call form: (query, key, value) with key is value, and all three the same tensor for one input."""
    return (xs[0], xs[0], xs[0]) if len(xs) == 1 else (xs[0], xs[1], xs[1])


def ref_module(mode, double=False):
    m = AR.AttentionRef(mode)
    m.load_state_dict(attn_state(), strict=True)
    return m.double() if double else m


def ref_run(g, tag, mode, double, grads=True):
    """The restatement on a module case -> (out, weights, {param: grad}, [input grads])."""
    m = ref_module(mode, double)
    inputs, mask, G = case_inputs(g, tag)
    xs, G = [torch.from_numpy(x) for x in inputs], torch.from_numpy(G)
    mk = None if mask is None else torch.from_numpy(mask)
    if double:
        xs, G = [x.double() for x in xs], G.double()
    xs = [x.requires_grad_(grads) for x in xs]
    with torch.set_grad_enabled(grads):
        y, w = m(*qkv(xs), attn_mask=mk)
        if grads:
            (y * G).sum().backward()
    if not grads:
        return y.numpy(), w.numpy(), None, None
    return y.detach().numpy(), w.detach().numpy(), {k: p.grad.numpy() for k, p in m.named_parameters()}, [x.grad.numpy() for x in xs]


def check_grads(g, tag, grads, g64, dxs, dx64):
    fix = fixture_grads(g, tag)
    assert sorted(fix) == sorted(grads), (tag, set(fix) ^ set(grads))
    for name, (kind, ref) in fix.items():
        got, r64 = (grads[name], g64[name]) if kind == 'full' else (digest(grads[name]), digest(g64[name]))
        for part in ((slice(None),) if kind == 'full' else (slice(0, 2), slice(2, None))):
            scale = float(np.abs(ref[part]).max()) + 1e-30
            yardstick_close(got[part], ref[part], r64[part], rtol=1e-4, atol=1e-5 * scale, what=f'{tag} grad {name} ({kind})')
    for i, (d, d64) in enumerate(zip(dxs, dx64)):
        ref = g[f'{tag}_dinput::{i}']
        yardstick_close(d, ref, d64, rtol=1e-4, atol=1e-5 * float(np.abs(ref).max()), what=f'{tag} d input {i}')


@pytest.mark.parametrize('case', MODULE_CASES)
@pytest.mark.parametrize('mod', ['hyp', 'euc'])
def test_restatement_reproduces_reference_module_cases(g, mod, case):
    tag = f'{mod}_{case}'
    y, w, grads, dxs = ref_run(g, tag, MODES[mod], False)
    _, _, g64, dx64 = ref_run(g, tag, MODES[mod], True)
    assert_close(y, g[f'{tag}_out'], what=f'{tag} out')
    assert_close(w, g[f'{tag}_w'], rtol=1e-4, atol=1e-6, what=f'{tag} weights')
    check_grads(g, tag, grads, g64, dxs, dx64)


@pytest.mark.parametrize('tag', FORWARD_CASES)
def test_restatement_reproduces_reference_forward_cases(g, tag):
    y, w, _, _ = ref_run(g, tag, MODES[tag[:3]], False, grads=False)
    ref, refw = g[f'{tag}_out'], g[f'{tag}_w']
    assert (np.isnan(y) == np.isnan(ref)).all() and (np.isnan(w) == np.isnan(refw)).all()
    if tag.endswith('nanrow'):
        nan = g[f'{tag}_nan']
        assert nan.any() and not nan.all() and (np.isnan(y) == nan).all()
        assert np.isfinite(y[~nan]).all()
        fin = ~np.isnan(refw)
        assert_close(y[~nan], ref[~nan], what=f'{tag} out')
        assert_close(w[fin], refw[fin], rtol=1e-4, atol=1e-6, what=f'{tag} weights')
    else:
        assert float(g['euc_overflow_maxscore']) > 89.0 and np.isfinite(y).all()      # exp(89) overflows fp32
        assert_close(y, ref, what=f'{tag} out')
        assert_close(w, refw, rtol=1e-4, atol=1e-6, what=f'{tag} weights')


def test_mask_changes_the_reference_output_and_padding_mask_is_absent(g):
    """The facts the drop-ins rely on: attn_mask is live in both reference modules (the masked fixture outputs differ from the unmasked ones
    on the same inputs only through the mask), and a -inf tile leaves the other columns' softmax exact."""
    for mod in ('hyp', 'euc'):
        m = ref_module(MODES[mod])
        inputs, mask, _ = case_inputs(g, f'{mod}_self_rand')
        xs = [torch.from_numpy(x) for x in inputs]
        with torch.no_grad():
            y0 = m(*qkv(xs))[0].numpy()
        assert np.abs(y0 - g[f'{mod}_self_rand_out']).max() > 1e-2
        w = g[f'{mod}_lead_lead_w']
        assert (w[:, [1, 3], :128] == 0).all() and np.allclose(w[:, [1, 3], 128], 1.0)


def stack_layer(tag, double=False):
    m, sd = (AR.DecoderLayerRef(), decoder_state()) if tag == 'edec' else (AR.EncoderLayerRef(), encoder_state())
    m.load_state_dict(sd, strict=True)
    return m.double() if double else m


def stack_run(g, tag, double):
    m = stack_layer(tag, double)
    inputs, _, G = case_inputs(g, tag)
    xs, G = [torch.from_numpy(x) for x in inputs], torch.from_numpy(G)
    if double:
        xs, G = [x.double() for x in xs], G.double()
    xs = [x.requires_grad_(True) for x in xs]
    y = m(*xs)
    (y * G).sum().backward()
    return y.detach().numpy(), {k: p.grad.numpy() for k, p in m.named_parameters()}, [x.grad.numpy() for x in xs]


@pytest.mark.parametrize('tag', ['edec', 'eenc'])
def test_restatement_reproduces_reference_euclidean_stacks(g, tag):
    y, grads, dxs = stack_run(g, tag, False)
    y64, g64, dx64 = stack_run(g, tag, True)
    yardstick_close(y, g[f'{tag}_out'], y64, rtol=1e-5, atol=1e-5, what=f'{tag} out')
    check_grads(g, tag, grads, g64, dxs, dx64)


# ---------------------------------------------------------------------------------------------------------------------------------
# host side
# ---------------------------------------------------------------------------------------------------------------------------------
P = 4096          # a non-NULL operand for calls that must be refused before any pointer is used
FWD_OK = dict(R=P, C=P, V=P, mask=None, ld_mask=0, out=P, wmax=None, wsum=None, wout=None, rows=4, cols=4, Nb=1, s=(64, 64) * 4, rs=1.0, cs=1.0,
              mode=0)
BWD_OK = dict(R=P, C=P, V=P, mask=None, ld_mask=0, dO=P, dR=P, dC=P, dV=P, rows=4, cols=4, Nb=1, s=(64, 64) * 4, rs=1.0, cs=1.0, mode=0)


def fwd_args(**kw):
    a = {**FWD_OK, **kw}
    return (a['R'], a['C'], a['V'], a['mask'], a['ld_mask'], a['out'], a['wmax'], a['wsum'], a['wout'], a['rows'], a['cols'], a['Nb'], *a['s'],
            a['rs'], a['cs'], a['mode'], None)


def bwd_args(**kw):
    a = {**BWD_OK, **kw}
    return (a['R'], a['C'], a['V'], a['mask'], a['ld_mask'], a['dO'], a['dR'], a['dC'], a['dV'], a['rows'], a['cols'], a['Nb'], *a['s'],
            a['rs'], a['cs'], a['mode'], None)


def test_exports_exist_and_abi_version_is_unchanged():
    from sttode_amd import capi
    L = capi.lib()
    assert capi.ABI_VERSION == 15 and L.sttode_abi_version() == 15
    assert hasattr(L, 'sttode_attn_core') and hasattr(L, 'sttode_attn_core_bwd')
    assert len(capi.SIGNATURES['sttode_attn_core']) == len(fwd_args()) and len(capi.SIGNATURES['sttode_attn_core_bwd']) == len(bwd_args())


@pytest.mark.parametrize('bad', [dict(R=None), dict(C=None), dict(V=None), dict(out=None), dict(rows=0), dict(cols=0), dict(Nb=0), dict(rows=-3),
                                 dict(Nb=8192), dict(mode=2), dict(mode=-1), dict(mask=P, ld_mask=3), dict(wout=P),
                                 dict(wout=P, wmax=P), dict(wmax=P)], ids=str)
def test_forward_entry_refuses_before_touching_the_device(bad):
    from sttode_amd import capi
    with pytest.raises(capi.SttodeError, match=r'sttode_attn_core:'):
        capi.call('sttode_attn_core', *fwd_args(**bad))


@pytest.mark.parametrize('bad', [dict(R=None), dict(C=None), dict(V=None), dict(dO=None), dict(dR=None), dict(dC=None), dict(dV=None),
                                 dict(rows=0), dict(cols=0), dict(Nb=0), dict(Nb=8192), dict(mode=2), dict(mode=-1), dict(mask=P, ld_mask=3),
                                 dict(rows=469, cols=469), dict(rows=4, cols=1025), dict(rows=863, cols=1)], ids=str)
def test_backward_entry_refuses_before_touching_the_device(bad):
    from sttode_amd import capi
    with pytest.raises(capi.SttodeError, match=r'sttode_attn_core_bwd:'):
        capi.call('sttode_attn_core_bwd', *bwd_args(**bad))


def test_backward_lds_bound_is_what_the_header_states():
    """rows (2 head_dim + 3) + cols 2 head_dim floats must fit 64 KiB: 468 x 468 is the largest square."""
    assert (468 * 19 + 468 * 16) * 4 <= 65536 < (469 * 19 + 469 * 16) * 4
    src = open(os.path.join(os.path.dirname(HERE), 'include', 'sttode_hip.h')).read()
    assert 'rows = cols <= 468' in src


def test_dropin_state_dict_matches_the_reference(g):
    from sttode_amd import attention
    for mod, cls in (('hyp', attention.Hyp_mhsa), ('euc', attention.MultiheadAttention)):
        m = cls(64, 8)
        sd = m.state_dict()
        assert list(sd) == [str(n) for n in g[f'{mod}_sd_names']]
        for v, sh in zip(sd.values(), g[f'{mod}_sd_shapes']):
            assert list(v.shape) == [int(d) for d in sh[:v.dim()]]
        m.load_state_dict(attn_state(), strict=True)
        # the reference's _reset_parameters: xavier_uniform_ in-projection (bound sqrt(6 / (fan_in + fan_out))), zero biases
        fresh = cls(64, 8)
        bound = (6.0 / (64 + 192)) ** 0.5
        w = fresh.in_proj_weight.detach()
        assert float(w.abs().max()) <= bound and float(w.std()) > 0.4 * bound
        assert not fresh.in_proj_bias.any() and not fresh.out_proj.bias.any()


@pytest.mark.parametrize('kw', [dict(embed_dim=32), dict(embed_dim=128), dict(num_heads=4), dict(dropout=0.1), dict(bias=False),
                                dict(add_bias_kv=True), dict(add_zero_attn=True), dict(kdim=32), dict(vdim=32),
                                dict(sparse_gate_class=object())],
                         ids=lambda kw: ', '.join(kw) if 'sparse_gate_class' in kw else str(kw))   # (no object address in a test id)
def test_dropin_constructor_refusals(kw):
    from sttode_amd import attention
    for cls in (attention.Hyp_mhsa, attention.MultiheadAttention):
        a = {'embed_dim': 64, 'num_heads': 8, **kw}
        with pytest.raises(NotImplementedError):
            cls(**a)
        cls(64, 8, kdim=64, vdim=64)


def test_forward_signature_is_the_reference_signature():
    import inspect
    from sttode_amd import attention
    want = ['self', 'query', 'key', 'value', 'key_padding_mask', 'need_weights', 'attn_mask', 'cross_range', 'interaction_mask', 'seq_mask']
    for cls in (attention.Hyp_mhsa, attention.MultiheadAttention):
        sig = inspect.signature(cls.forward)
        assert list(sig.parameters) == want
        assert sig.parameters['need_weights'].default is True and sig.parameters['cross_range'].default == 0
        assert list(inspect.signature(cls.__init__).parameters) == ['self', 'embed_dim', 'num_heads', 'dropout', 'bias', 'add_bias_kv',
                                                                    'add_zero_attn', 'kdim', 'vdim', 'sparse_gate_class']


def test_no_cpu_fallback_and_mask_validation():
    from sttode_amd import attention, capi, hypertransformer as ht, ops
    x = torch.zeros(3, 2, 64)
    W = (torch.zeros(192, 64), torch.zeros(192), torch.zeros(64, 64), torch.zeros(64))
    mask = torch.zeros(3, 3)
    for f in (lambda: ops.mha(x, x, x, *W), lambda: ops.mha(x, x, x, *W, attn_mask=mask), lambda: ops.mhgsa(x, x, x, *W, attn_mask=mask),
              lambda: attention.Hyp_mhsa(64, 8)(x, x, x), lambda: attention.MultiheadAttention(64, 8)(x, x, x, attn_mask=mask),
              lambda: ht.trainable(attention.MultiheadAttention(64, 8))(x.requires_grad_(True), x, x),
              lambda: ht.TransformerEncoderLayer(64, 8, 64, euclidean=True)(torch.zeros(3, 2, 1, 64))):
        with pytest.raises(capi.SttodeError):
            f()


def test_trainable_learns_the_two_modules_and_euclidean_flag_is_handed_down():
    import copy
    from sttode_amd import attention, hypertransformer as ht
    for cls in (attention.Hyp_mhsa, attention.MultiheadAttention):
        m = cls(64, 8)
        assert m._trainable is False and ht.trainable(m) is m and m._trainable is True
        assert ht.trainable(m, False)._trainable is False
    dec = ht.TransformerDecoderLayer(64, 8, 64, euclidean=True)
    assert dec.self_attn.euclidean and dec.cross_attn.euclidean and ht.TransformerEncoderLayer(64, 8, 64, euclidean=True).self_attn.euclidean
    assert copy.deepcopy(ht.ODEG(dec, 2, 1.0)).layers[1].cross_attn.euclidean
    assert list(dec.state_dict()) == list(ht.TransformerDecoderLayer(64, 8, 64).state_dict())
    assert not ht.TransformerDecoderLayer(64, 8, 64).self_attn.euclidean and not ht.Hypattention(64, 8).euclidean
    with pytest.raises(TypeError):
        ht.Hypattention(64, 8, 0., True, 0, 3, True)                        # keyword-only
