"""The stage program of the fixed-grid encoder integrators and its discrete adjoint, written once for every user.

``oracle.sttode_ref.ode_integrate_ref`` / ``hypertransformer.ode_integrate`` define the integrators (uniform grid of ``steps`` steps over
[0, t1]); here they are one Butcher tableau each.  Stage i of a step reads Y_i = y + h sum_{j<i} A[i][j] k_j and evaluates k_i = f(Y_i); the
step is y' = y + h sum_i B[i] k_i.

``integrate`` and ``integrate_adjoint`` take the arithmetic as callables, so that the same program drives the training kernels
(training.Engine: one sttode_ttrunk_ode_fwd launch runs the whole forward program, one sttode_ode_stage_bwd launch per stage the
adjoint's combinations together with f's VJP; sttode_ode_combine launches on the layer-by-layer path) and plain torch
(tests/test_ode_stages.py).
The adjoint is discretize-then-optimize: exactly the gradient of the discrete scheme, i.e. what autograd of ode_integrate_ref gives.
"""

TABLEAU = {                     # method -> (A: row i = the coefficients of stage i's input, B: the step's weights)
    'euler': (((),), (1.0,)),
    'rk4': (((), (1 / 3,), (-1 / 3, 1.0), (1.0, -1.0, 1.0)), (1 / 8, 3 / 8, 3 / 8, 1 / 8)),                  # torchdiffeq rk4_alt_step_func
    'rk4_classic': (((), (0.5,), (0.0, 0.5), (0.0, 0.0, 1.0)), (1 / 6, 1 / 3, 1 / 3, 1 / 6)),
}


def stages(method):
    if method not in TABLEAU:
        raise ValueError(f'unknown ODE method {method!r}')
    return len(TABLEAU[method][1])


def integrate(f, comb, y0, t1, method, steps):
    """Forward program.  ``f(j, Y)`` -> k (j = global stage index, n * stages + i); ``comb(terms, dst)`` -> sum of coef * value over
    ``terms`` [(coef, value)]; ``dst`` names the result: stage index j (a stage input, kept for the backward pass), 'final' (y_T) or
    None (a temporary).  Stage 0 of a step reads the step's start state itself, which the previous combination wrote as stage input j."""
    A, B = TABLEAU[method]
    s, h = stages(method), float(t1) / steps
    y = comb([(1.0, y0)], 0)
    for n in range(steps):
        ks = []
        for i in range(s):
            Y = y if i == 0 else comb([(1.0, y)] + [(h * a, k) for a, k in zip(A[i], ks) if a != 0.0], n * s + i)
            ks.append(f(n * s + i, Y))
        y = comb([(1.0, y)] + [(h * b, k) for b, k in zip(B, ks)], 'final' if n == steps - 1 else (n + 1) * s)
    return y


def integrate_adjoint(vjp, ybar, t1, method, steps, extra=()):
    """Reverse program: ``ybar`` = gradient wrt y_T.  Stages are visited in reverse (j descending); ``vjp(j, kb, close)`` gets the terms
    [(coef, value)] whose sum is the gradient of k_j (the stage-combination adjoint: h B[i] ybar + h sum_{l>i} A[l][i] dY_l), and, on a
    step's first stage, ``close``: the terms that, added to the stage's own input gradient, give the gradient wrt the step's start state
    (None otherwise).  It returns (gradient wrt stage input j, that sum or None) -- a caller may form both sums inside one launch.
    ``extra`` [(coef, value)] is added into the returned gradient wrt y_0."""
    A, B = TABLEAU[method]
    s, h = stages(method), float(t1) / steps
    for n in reversed(range(steps)):
        Yb = [None] * s
        for i in reversed(range(s)):
            kb = [(h * B[i], ybar)] + [(h * A[l][i], Yb[l]) for l in range(i + 1, s) if A[l][i] != 0.0]
            close = [(1.0, ybar)] + [(1.0, v) for v in Yb[1:]] + (list(extra) if n == 0 else []) if i == 0 else None
            Yb[i], closed = vjp(n * s + i, kb, close)
        ybar = closed
    return ybar
