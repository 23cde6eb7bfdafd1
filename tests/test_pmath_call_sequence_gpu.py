"""The calls that pmath's differentiable functions make, pinned: forward plus backward of eight public functions under a
float c, a tensor c with everything requiring grad, a tensor c that alone requires grad, and a tensor c that does not -- the entry points
in order and, per call, which arguments were tensors ('t'), None ('-') or numbers ('.'), the stream left out.  EXPECTED was recorded by
running `sequences` below over the pmath.py of the commit before the Functions' float and tensor backward bodies were merged: which
buffers a backward pass allocates is a function of the curvature's form and of needs_input_grad, and must stay one.

Shapes: the smallest that take every branch -- 5 rows (a partial last block of the 4-rows-per-block kernels), d = 3, P = 3, R = 2, O = 4."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SETTINGS = ('float c', 'tensor c, all grads', 'tensor c, c alone', 'tensor c without grad')


def _ball(gen, *shape):
    x = torch.randn(*shape, generator=gen)
    return 0.6 * x / (1.0 + x.norm(dim=-1, keepdim=True))     # |x| < 0.6: inside the ball for c = 0.7


def sequences(pm, capi, dev):
    """{'function / setting': [(entry, argument kinds), ...]} of forward plus backward, recorded by a pass-through around capi.call."""
    gen = torch.Generator().manual_seed(5)
    functions = {   # name: (function of (c, *tensors), the tensors' shapes)
        'mobius_add': (lambda c, x, y: pm.mobius_add(x, y, c=c), ((5, 3), (5, 3))),
        'dist': (lambda c, x, y: pm.dist(x, y, c=c), ((5, 3), (5, 3))),
        'expmap0': (lambda c, u: pm.expmap0(u, c=c), ((5, 3),)),
        'mobius_matvec': (lambda c, m, x: pm.mobius_matvec(m, x, c=c), ((4, 3), (5, 3))),
        'dist_matrix': (lambda c, x, y: pm.dist_matrix(x, y, c), ((3, 3), (2, 3))),
        '_mobius_addition_batch': (lambda c, x, y: pm._mobius_addition_batch(x, y, c), ((3, 3), (2, 3))),
        '_hyperbolic_softmax': (lambda c, X, A, P: pm._hyperbolic_softmax(X, A, P, c), ((5, 3), (3, 3), (3, 3))),
        'poincare_mean': (lambda c, x: pm.poincare_mean(x, dim=1, c=c, differentiable=True), ((5, 2, 3),)),
    }
    calls = []
    real = capi.call

    def recording(name, *args, **kw):
        calls.append((name, ''.join('t' if isinstance(a, torch.Tensor) else '-' if a is None else '.' for a in args[:-1])))
        return real(name, *args, **kw)

    out = {}
    capi.call = recording
    try:
        for fname, (fn, shapes) in functions.items():
            values = [_ball(gen, *s).to(dev) for s in shapes]
            for setting in SETTINGS:
                tensors = [v.clone().requires_grad_(setting != 'tensor c, c alone') for v in values]
                c = 0.7 if setting == 'float c' else torch.full((1,), 0.7, device=dev).requires_grad_(setting != 'tensor c without grad')
                del calls[:]
                fn(c, *tensors).sum().backward()
                out[fname + ' / ' + setting] = list(calls)
    finally:
        capi.call = real
    torch.cuda.synchronize()
    return out


EXPECTED = {
    'mobius_add / float c': [('sttode_pmath_rowop', '.ttt-...'), ('sttode_pmath_rowop_bwd', '.ttttt...')],
    'mobius_add / tensor c, all grads': [('sttode_pmath_rowop_c', '.ttt-..t'), ('sttode_pmath_rowop_bwd_c', '.ttttt..ttt')],
    'mobius_add / tensor c, c alone': [('sttode_pmath_rowop_c', '.ttt-..t'), ('sttode_pmath_rowop_bwd_c', '.ttt--..ttt')],
    'mobius_add / tensor c without grad': [('sttode_pmath_rowop_c', '.ttt-..t'), ('sttode_pmath_rowop_bwd_c', '.ttttt..ttt')],
    'dist / float c': [('sttode_pmath_rowop', '.ttt-...'), ('sttode_pmath_rowop_bwd', '.ttttt...')],
    'dist / tensor c, all grads': [('sttode_pmath_rowop_c', '.ttt-..t'), ('sttode_pmath_rowop_bwd_c', '.ttttt..ttt')],
    'dist / tensor c, c alone': [('sttode_pmath_rowop_c', '.ttt-..t'), ('sttode_pmath_rowop_bwd_c', '.ttt--..ttt')],
    'dist / tensor c without grad': [('sttode_pmath_rowop_c', '.ttt-..t'), ('sttode_pmath_rowop_bwd_c', '.ttttt..ttt')],
    'expmap0 / float c': [('sttode_pmath_rowop', '.t-t-...'), ('sttode_pmath_rowop_bwd', '.t-tt-...')],
    'expmap0 / tensor c, all grads': [('sttode_pmath_rowop_c', '.t-t-..t'), ('sttode_pmath_rowop_bwd_c', '.t-tt-..ttt')],
    'expmap0 / tensor c, c alone': [('sttode_pmath_rowop_c', '.t-t-..t'), ('sttode_pmath_rowop_bwd_c', '.t-t--..ttt')],
    'expmap0 / tensor c without grad': [('sttode_pmath_rowop_c', '.t-t-..t'), ('sttode_pmath_rowop_bwd_c', '.t-tt-..ttt')],
    'mobius_matvec / float c': [('sttode_pmath_matvec', 'ttttt....'), ('sttode_pmath_matvec_bwd', 'tttttttt....')],
    'mobius_matvec / tensor c, all grads': [('sttode_pmath_matvec_c', 'ttttt...t'), ('sttode_pmath_matvec_bwd_c', 'ttttt-tt...ttt')],
    'mobius_matvec / tensor c, c alone': [('sttode_pmath_matvec_c', 'ttttt...t'), ('sttode_pmath_matvec_bwd_c', 'tttt----...ttt')],
    'mobius_matvec / tensor c without grad': [('sttode_pmath_matvec_c', 'ttttt...t'), ('sttode_pmath_matvec_bwd_c', 'ttttt-tt...ttt')],
    'dist_matrix / float c': [('sttode_pmath_pair', '.tt-t....'), ('sttode_pmath_dist_matrix_bwd', 'ttttt....')],
    'dist_matrix / tensor c, all grads': [('sttode_pmath_pair_c', '.tt-t...t'), ('sttode_pmath_dist_matrix_bwd_c', 'ttttt...ttt')],
    'dist_matrix / tensor c, c alone': [('sttode_pmath_pair_c', '.tt-t...t'), ('sttode_pmath_dist_matrix_bwd_c', 'ttt--...ttt')],
    'dist_matrix / tensor c without grad': [('sttode_pmath_pair_c', '.tt-t...t'), ('sttode_pmath_dist_matrix_bwd_c', 'ttttt...ttt')],
    '_mobius_addition_batch / float c': [('sttode_pmath_pair', '.tt-t....'), ('sttode_pmath_rowop_bwd', '.ttttt...')],
    '_mobius_addition_batch / tensor c, all grads': [('sttode_pmath_pair_c', '.tt-t...t'), ('sttode_pmath_rowop_bwd_c', '.ttttt..ttt')],
    '_mobius_addition_batch / tensor c, c alone': [('sttode_pmath_pair_c', '.tt-t...t'), ('sttode_pmath_rowop_bwd_c', '.ttt--..ttt')],
    '_mobius_addition_batch / tensor c without grad': [('sttode_pmath_pair_c', '.tt-t...t'), ('sttode_pmath_rowop_bwd_c', '.ttttt..ttt')],
    '_hyperbolic_softmax / float c': [('sttode_pmath_pair', '.tttt....'), ('sttode_pmath_hsoftmax_bwd', 'tttttttt....')],
    '_hyperbolic_softmax / tensor c, all grads': [('sttode_pmath_pair_c', '.tttt...t'), ('sttode_pmath_hsoftmax_bwd_c', 'tttttttt...ttt')],
    '_hyperbolic_softmax / tensor c, c alone': [('sttode_pmath_pair_c', '.tttt...t'), ('sttode_pmath_hsoftmax_bwd_c', 'ttttt---...ttt')],
    '_hyperbolic_softmax / tensor c without grad': [('sttode_pmath_pair_c', '.tttt...t'), ('sttode_pmath_hsoftmax_bwd_c', 'tttttttt...ttt')],
    'poincare_mean / float c': [('sttode_pmath_mean_seg', 'tttt--.....-'), ('sttode_pmath_mean_bwd', 'ttttt.....')],
    'poincare_mean / tensor c, all grads': [('sttode_pmath_mean_seg', 'tttt--.....t'), ('sttode_pmath_mean_bwd_c', 'ttttt....ttt')],
    'poincare_mean / tensor c, c alone': [('sttode_pmath_mean_seg', 'tttt--.....t'), ('sttode_pmath_mean_bwd_c', 'tttt-....ttt')],
    'poincare_mean / tensor c without grad': [('sttode_pmath_mean_seg', 'tttt--.....t'), ('sttode_pmath_mean_bwd_c', 'ttttt....ttt')],
}


def test_forward_and_backward_make_the_recorded_calls():
    from sttode_amd import capi, pmath
    got = sequences(pmath, capi, torch.device('cuda:0'))
    assert sorted(got) == sorted(EXPECTED)
    for key, calls in EXPECTED.items():
        assert got[key] == calls, key
