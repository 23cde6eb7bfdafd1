"""The six follow-up entry points of an asynchronous call (csrc/pipeline.hip slot_follow_up: sttode_async_best_of_k, _best_of_k_select,
_joint_select, _kde_nll, _sample_spread, _horizon_metrics) refuse alike, with their own name in front: a bad model or slot, and a slot no
asynchronous call has used.  A refused pass enqueues nothing and writes nothing."""
import ctypes

import pytest
import torch

from helpers import make_args

N, K, TF, S = 2, 2, 2, 1


def _entries(pred, gt, seg_ptr, out):
    """name -> the arguments behind (model, slot) for n = 2, K = 2, Tf = 2 and one segment; ``out(name, dtype, *shape)`` gives an output."""
    f, d, i = torch.float32, torch.float64, torch.int32
    head = (pred, gt, N, K, TF, 1.0)
    return {
        'sttode_async_best_of_k': head + (out('ade', f, N), out('fde', f, N)),
        'sttode_async_best_of_k_select': head + (1.0, seg_ptr, S, out('ade', f, N), out('fde', f, N), out('ia', i, N), out('if', i, N),
                                                 out('miss', torch.uint8, N), out('best', f, N, TF, 2), out('sa', f, S), out('sf', f, S),
                                                 out('sm', i, S)),
        'sttode_async_joint_select': head + (seg_ptr, S, 0.5, out('ja', f, S), out('jf', f, S), out('jia', i, S), out('jif', i, S),
                                             out('col', i, S), out('gcol', i, S)),
        'sttode_async_kde_nll': head + (out('nll', d, N),),
        'sttode_async_sample_spread': head + (1.0,) + tuple(out(w, d, N) for w in ('apd', 'fpd', 'pade', 'dlow', 'ea', 'ef'))
        + (out('ak', f, N, K), out('fk', f, N, K)),
        'sttode_async_horizon_metrics': head + (out('hm', f, N, TF, 2),),
    }


NAMES = sorted(_entries(None, None, None, lambda *a: None))


@pytest.mark.parametrize('name', NAMES)
def test_a_null_model_is_refused_by_name_without_a_device(name):
    from sttode_amd import capi
    L = capi.lib()
    P = ctypes.c_void_p(16)                                            # (never dereferenced: the call is refused first)
    args = [P if a is None else a for a in _entries(None, None, None, lambda *a: None)[name]]
    assert getattr(L, name)(None, 0, *args) != 0
    assert L.sttode_last_error().decode() == name + ': bad model / slot'
    assert getattr(L, name)(None, 8, *args) != 0                       # (slots are 0..7)
    assert L.sttode_last_error().decode() == name + ': bad model / slot'


@pytest.mark.gpu
def test_a_slot_no_asynchronous_call_has_used_is_refused_and_nothing_is_written():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from sttode_amd import STTODENet, capi
    from sttode_amd.weights import make_weights, to_torch_state_dict
    dev = torch.device('cuda:0')
    m = STTODENet(make_args('eth', 8, 12), dev).eval()                 # a model of its own: it has made no asynchronous call
    m.load_state_dict(to_torch_state_dict(make_weights(1234)), strict=True)
    h = m.native().h
    L = capi.lib()
    pred, gt = torch.randn(N, K, TF, 2, device=dev), torch.randn(N, TF, 2, device=dev)
    seg_ptr = torch.tensor([0, N], dtype=torch.int32, device=dev)
    outs = []

    def out(what, dtype, *shape):
        outs.append((what, torch.full(shape, 77, dtype=dtype, device=dev)))
        return outs[-1][1]
    entries = _entries(pred, gt, seg_ptr, out)
    torch.cuda.synchronize()
    for name in NAMES:
        args = [a.data_ptr() if isinstance(a, torch.Tensor) else a for a in entries[name]]
        assert getattr(L, name)(h, 0, *args) != 0, name
        assert L.sttode_last_error().decode() == name + ': no asynchronous call has used this slot'
    torch.cuda.synchronize()
    for what, t in outs:
        assert bool((t == 77).all()), what
