"""Shapes and seeded inputs of the float64 tests of the per-agent displacement kernels (tests/test_metric_root_ref.py on the CPU,
tests/test_metric_root_gpu.py on the device).  Inputs follow the draw of tests/golden/make_selection_golden.py: a straight-walk ground
truth, samples with a drift that grows along the horizon, coordinates O(10).  Every case is regenerated from its seed; nothing is stored.

The shapes are the smallest at which a code path changes: n around the four waves of a workgroup; K around the 64 lanes (and, for
sttode_best_of_k only, around a second trip of its k += 64 loop); K Tf around 1024, where best_of_k_kernel / bok_select_kernel stop
staging the distances in LDS, and at 2048, all of horizon_metrics_kernel's LDS array.

Two conditions are asserted on every agent of every case and scale, from the float64 reference alone (see conditions()): the best and the
second-best ADE, and FDE, differ by more than 4 bounds relative, so no index hinges on rounding; every FDE is further than 4 bound_fde
relative from every miss threshold.  A seed that fails one is changed (SEED_SALT); no agent is masked."""
import functools

import numpy as np

import metric_root_ref as R

SCALES = (1.0, 1.7)
THRESHOLDS = (0.5, 1.0, 2.0)
NS = (1, 3, 4, 5)
# (K, Tf): K = 1 | two samples | one lane idle | a full wave | K Tf = 1024, the last LDS case | 1088 and 1025, the first direct reads |
# long frames
SELECT_SHAPES = ((1, 1), (2, 12), (63, 12), (64, 12), (64, 16), (64, 17), (41, 25), (20, 200))
# sttode_best_of_k only: one sample in the second trip | a second trip, LDS | 1024 in two full trips | 1040: two trips and a tail, direct reads
BOK_ONLY_SHAPES = ((65, 12), (100, 10), (128, 8), (130, 8))
# sttode_horizon_metrics: ... | K Tf = 2048 exactly | 2000
HORIZON_SHAPES = ((1, 1), (20, 10), (63, 12), (64, 32), (20, 100))
HORIZON_REFUSED = ((65, 4), (63, 33))                 # K = 65; K Tf = 2079
NONFINITE_SHAPES = ((20, 12), (64, 12))

BOK_CASES = tuple((n, K, Tf) for K, Tf in SELECT_SHAPES + BOK_ONLY_SHAPES for n in NS)
SELECT_CASES = tuple((n, K, Tf) for K, Tf in SELECT_SHAPES for n in NS)
HORIZON_CASES = tuple((n, K, Tf) for K, Tf in HORIZON_SHAPES for n in NS)

# segments: one batch of 200 agents
SEG_CASE = (200, 20, 12)
SEG_CSRS = {
    'sizes_1_63_64_65_7': (0, 1, 64, 128, 193, 200),
    # [0, 10) from a bound below 0 | empty | [10, 150) | [150, 200) from a bound above n | empty: both bounds clamp to n, a1 >= a0
    'empty_and_clamped': (-5, 10, 10, 150, 230, 120),
    'one_segment_of_200': (0, 200),
}

SEED_SALT = {}                                        # (n, K, Tf) -> added to the seed of a case whose first draw failed a condition


def case_id(c):
    return 'n%d-K%d-Tf%d' % c


def _spread(K):
    return 1.5 if K == 1 else (8.0 if K > 40 else 4.0)          # as make_selection_golden.py: FDE near the thresholds


def draw(rng, n, K, Tf, spread):
    """make_selection_golden.py's draw."""
    start, vel = rng.uniform(-5, 5, (n, 1, 2)), rng.normal(0, 0.4, (n, 1, 2))
    gt = start + vel * np.arange(1, Tf + 1)[None, :, None]
    drift = rng.normal(0, spread, (n, K, 1, 2)) * np.linspace(0.3, 1.0, Tf)[None, None, :, None]
    pred = gt[:, None] + drift + rng.normal(0, 0.05 * spread, (n, K, Tf, 2))
    return pred.astype(np.float32), gt.astype(np.float32)


def _gap(v):
    """v [n,K] -> relative gap between the smallest and the second-smallest value per row (inf for K = 1)."""
    if v.shape[1] < 2:
        return np.full(len(v), np.inf)
    d = np.sort(v, axis=1)
    return (d[:, 1] - d[:, 0]) / d[:, 1]


def conditions(n, K, Tf, ref):
    """The two conditions, on every agent; ``ref``: R.best64 of the case at one scale.  Returns the smallest margins for the record."""
    ga, gf = _gap(ref['ade_k']), _gap(ref['fde_k'])
    assert (ga > 4 * R.bound_ade(Tf)).all(), ('ADE gap', (n, K, Tf), ga.min())
    assert (gf > 4 * R.bound_fde).all(), ('FDE gap', (n, K, Tf), gf.min())
    thr = np.array(THRESHOLDS)[None]
    away = np.abs(ref['fde'][:, None] - thr) / np.maximum(ref['fde'][:, None], thr)
    assert (away > 4 * R.bound_fde).all(), ('FDE against a miss threshold', (n, K, Tf), away.min())
    return float(ga.min()), float(gf.min()), float(away.min())


@functools.lru_cache(maxsize=None)
def inputs(n, K, Tf):
    """(pred [n,K,Tf,2], gt [n,Tf,2]) float32 of a case, drawn once and read-only."""
    rng = np.random.default_rng(20261021 + 100003 * n + 1009 * K + Tf + SEED_SALT.get((n, K, Tf), 0))
    pred, gt = draw(rng, n, K, Tf, _spread(K))
    pred.flags.writeable = gt.flags.writeable = False
    return pred, gt


@functools.lru_cache(maxsize=None)
def reference(n, K, Tf, scale):
    """The float64 values of a case at one scale (R.best64's dict plus 'horizon' [n,Tf,2] and the 'margins' of conditions()), computed once,
    shared and read-only.  The conditions are asserted here: no test sees a case that fails one."""
    pred, gt = inputs(n, K, Tf)
    d = R.dist64(pred, gt, scale)
    ak, fk = R.per_sample(d)
    (a, ia), (f, jf) = R.first_min(ak), R.first_min(fk)
    ref = {'ade_k': ak, 'fde_k': fk, 'ade': a, 'fde': f, 'ade_idx': ia, 'fde_idx': jf, 'horizon': R.horizon_from(d)}
    ref['margins'] = conditions(n, K, Tf, ref)
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.flags.writeable = False
    return ref


def all_cases():
    """Every (n, K, Tf) any test uses, once."""
    seen = []
    for c in BOK_CASES + HORIZON_CASES + (SEG_CASE,) + tuple((5, K, Tf) for K, Tf in NONFINITE_SHAPES):
        if c not in seen:
            seen.append(c)
    return seen


def nonfinite_inputs(K, Tf):
    """Five agents: agent 1 has every second sample NaN, beginning with the sample that was its best; agent 3 is all NaN; agents 0, 2 and 4
    are the finite case's.  -> (pred, gt, half: the agent, nan_k: its NaN samples, dead: the all-NaN agent)."""
    pred, gt = inputs(5, K, Tf)
    pred = pred.copy()
    half, dead = 1, 3
    k0 = int(reference(5, K, Tf, 1.0)['ade_idx'][half])
    nan_k = np.arange(k0 % 2, K, 2)
    pred[half, nan_k] = np.nan
    pred[dead] = np.nan
    keep = np.setdiff1d(np.arange(K), nan_k)
    for scale in SCALES:                                  # the conditions, again, on what is left of the half-NaN agent
        ref = R.best64(pred, gt, scale)
        conditions(5, K, Tf, {'ade_k': ref['ade_k'][[half]][:, keep], 'fde_k': ref['fde_k'][[half]][:, keep], 'fde': ref['fde'][[half]]})
    return pred, gt, half, nan_k, dead
