"""CPU tests of the encoder integrators' stage program (sttode_amd/odestages.py): the Butcher tables and their discrete adjoint, applied
to a small float64 function, against oracle.sttode_ref.ode_integrate_ref and torch autograd of it."""
import pytest
import torch

from oracle.sttode_ref import ode_integrate_ref
from sttode_amd import odestages

CASES = [('euler', 1), ('euler', 3), ('rk4', 1), ('rk4', 2), ('rk4_classic', 2), ('rk4', 5)]


def _f():
    g = torch.Generator().manual_seed(3)
    W = torch.randn(6, 6, generator=g, dtype=torch.float64) * 0.3
    b = torch.randn(6, generator=g, dtype=torch.float64) * 0.1

    def f(y):
        return torch.tanh(y @ W.T + b)
    return f


def _comb(terms, dst):
    return sum(c * v for c, v in terms)


@pytest.mark.parametrize('method,steps', CASES)
def test_stage_program_matches_ode_integrate_ref(method, steps):
    f = _f()
    y0 = torch.randn(4, 6, dtype=torch.float64, generator=torch.Generator().manual_seed(5))
    kept = {}

    def comb(terms, dst):
        out = _comb(terms, dst)
        kept[dst] = out
        return out
    got = odestages.integrate(lambda j, Y: f(Y), comb, y0, 1.7, method, steps)
    ref = ode_integrate_ref(f, y0, 1.7, method, steps)
    torch.testing.assert_close(got, ref, rtol=1e-12, atol=1e-12)
    # every stage input is named once (the tape of the training path), and y_T as 'final'
    assert sorted(k for k in kept if isinstance(k, int)) == list(range(steps * odestages.stages(method)))
    assert 'final' in kept


@pytest.mark.parametrize('method,steps', CASES)
def test_stage_adjoint_matches_autograd(method, steps):
    f = _f()
    y0 = torch.randn(4, 6, dtype=torch.float64, generator=torch.Generator().manual_seed(7)).requires_grad_(True)
    w = torch.randn(4, 6, dtype=torch.float64, generator=torch.Generator().manual_seed(8))
    extra = torch.randn(4, 6, dtype=torch.float64, generator=torch.Generator().manual_seed(9))
    (ode_integrate_ref(f, y0, 2.0, method, steps) * w).sum().backward()
    ref = y0.grad.clone() + extra
    Ys = {}

    def comb(terms, dst):
        out = _comb(terms, dst)
        if isinstance(dst, int):
            Ys[dst] = out.detach()
        return out
    with torch.no_grad():
        odestages.integrate(lambda j, Y: f(Y), comb, y0.detach(), 2.0, method, steps)
    order = []

    def vjp(j, kb, close):
        order.append(j)
        Y = Ys[j].clone().requires_grad_(True)
        with torch.enable_grad():
            (gY,) = torch.autograd.grad(f(Y), Y, _comb(kb, None))
        return gY, (None if close is None else _comb([(1.0, gY)] + close, None))
    got = odestages.integrate_adjoint(vjp, w, 2.0, method, steps, extra=[(1.0, extra)])
    torch.testing.assert_close(got, ref, rtol=1e-11, atol=1e-12)
    assert order == list(reversed(range(steps * odestages.stages(method))))      # stages visited in reverse, once each


def test_tables_are_consistent():
    for method, (A, B) in odestages.TABLEAU.items():
        assert len(A) == len(B) == odestages.stages(method)
        assert abs(sum(B) - 1.0) < 1e-15                      # consistency of the scheme
        assert all(len(A[i]) == i for i in range(len(A)))     # explicit: stage i reads k_0 .. k_{i-1}
    with pytest.raises(ValueError):
        odestages.stages('dopri5')
