"""GPU tests of Gromov delta-hyperbolicity (csrc/delta.hip, sttode_amd.delta, evaluate.embedding_delta; hyptorch/delta.py): the delta kernel
bitwise against a float32 NumPy restatement of the formula on both paths, both entry points against the reference's outputs in
tests/golden/delta.npz, exact results at n = 4096, the distance kernel (symmetry, accuracy, the idx gather, one launch across tries), and
embedding_delta against batched_delta_hyp over rows gathered through the staged API."""
import numpy as np
import pytest
import torch

from helpers import make_args
from test_delta import delta_f32, dist_f64

pytestmark = pytest.mark.gpu


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    return torch.device('cuda:0')


@pytest.fixture(autouse=True)
def _needs_gpu():
    _gpu()


def _dev_delta(D, symmetric):
    from sttode_amd import delta
    return np.float32(delta.delta_hyp_device(torch.from_numpy(np.ascontiguousarray(D, np.float32)).to(_gpu()), symmetric=symmetric).item())


def _sym_dist(rng, n, d=16):
    """A bitwise-symmetric float32 distance matrix with a zero diagonal (upper triangle mirrored)."""
    D = dist_f64(rng.standard_normal((n, d))).astype(np.float32)
    D = np.triu(D, 1)
    return D + D.T


@pytest.mark.parametrize('n', [1, 2, 3, 63, 64, 65, 127, 129, 255, 257, 1500])
def test_delta_bitwise_against_f32_restatement(n):
    rng = np.random.default_rng(1000 + n)
    D = _sym_dist(rng, n)
    ref = delta_f32(D, chunk=4 if n >= 1000 else 16)
    assert _dev_delta(D, False) == ref
    assert _dev_delta(D, True) == ref
    # the general path on a non-symmetric matrix of the same size
    N = rng.uniform(0.5, 4.0, (n, n)).astype(np.float32)
    if n <= 257:
        assert _dev_delta(N, False) == delta_f32(N)


def test_delta_non_symmetric_fixture(golden):
    from sttode_amd import delta
    g = golden('delta')
    D = g['ns_D']
    got = _dev_delta(D, False)
    assert got == delta_f32(D)
    assert abs(float(got) - g['ns_delta']) <= 2e-6 * D.max()
    assert abs(delta.delta_hyp(D) - g['ns_delta']) <= 2e-6 * D.max()
    assert isinstance(delta.delta_hyp(D), np.float64)


TAGS = ('gauss', 'circle', 'clusters', 'n1', 'n2', 'n3', 'n65')


def test_against_reference_fixtures(golden):
    from sttode_amd import delta
    g = golden('delta')
    dev = _gpu()
    for tag in TAGS:
        X, dref, diam_ref = g['dh_%s_X' % tag], float(g['dh_%s_delta' % tag]), float(g['dh_%s_diam' % tag])
        D64 = dist_f64(X)
        assert abs(delta.delta_hyp(D64) - dref) <= 2e-6 * max(diam_ref, 1.0), tag          # D given (float64 numpy, copied as float32)
        assert abs(delta.delta_hyp(torch.from_numpy(D64).to(dev)) - dref) <= 2e-6 * max(diam_ref, 1.0), tag
        # device distances: one try of the rows as given
        dl, dm = delta.batched_deltas(X, np.arange(len(X))[None])
        dl, dm = float(dl[0]), float(dm[0])
        assert abs(dm - diam_ref) <= 1e-5 * diam_ref, tag
        assert abs(dl - dref) <= 1e-5 * max(diam_ref, 1.0), tag
    # batched_delta_hyp: same seed -> same rows, same values, same RNG state afterwards
    np.random.seed(int(g['bt_seed']))
    m, s = delta.batched_delta_hyp(g['bt_X'], n_tries=4, batch_size=300)
    assert isinstance(m, np.float64) and isinstance(s, np.float64)
    assert abs(m - g['bt_mean']) <= 1e-5 and abs(s - g['bt_std']) <= 1e-5
    assert np.random.rand() == g['bt_next']
    np.random.seed(int(g['bt_seed']))
    m2, s2 = delta.batched_delta_hyp(torch.from_numpy(g['bt_X']).to(dev), n_tries=4, batch_size=300)
    assert (m2, s2) == (m, s)
    # Poincare ball: the general path on pmath.dist_matrix
    c = float(g['pc_c'])
    X = g['pc_X']
    m, s = delta.batched_delta_hyp(X, n_tries=1, batch_size=len(X), metric='poincare', c=c, idx=np.arange(len(X))[None])
    assert abs(m - g['pc_delta'] / g['pc_diam']) <= 1e-4 * g['pc_delta'] / g['pc_diam'] and s == 0.0
    from sttode_amd import pmath
    Xt = torch.from_numpy(X).to(dev)
    dp = delta.delta_hyp(pmath.dist_matrix(Xt, Xt, c))
    assert abs(dp - g['pc_delta']) <= 1e-4 * g['pc_delta']


def test_identical_rows_give_nan_like_the_reference():
    from sttode_amd import delta
    X = np.ones((5, 3), np.float32)
    m, s = delta.batched_delta_hyp(X, n_tries=2, batch_size=4)
    assert np.isnan(m) and np.isnan(s)


def _tree_dist(rng, n):
    """A random tree with integer edge weights 1..8 (node i hangs under a parent < i): exact path lengths, integers exact in float32.
    Nodes after i are never on the path from i to an earlier node j, so d(i, j) = d(parent(i), j) + w(i) for j < i."""
    D = np.zeros((n, n), np.int64)
    for i in range(1, n):
        p, w = int(rng.integers(0, i)), int(rng.integers(1, 9))
        D[i, :i] = D[p, :i] + w
        D[i, p] = w
        D[:i, i] = D[i, :i]
    return D


def test_tree_metric_is_exactly_zero_at_4096():
    rng = np.random.default_rng(77)
    n = 4096
    D = _tree_dist(rng, n)
    assert (D == D.T).all() and D.max() < 2 ** 20
    Df = D.astype(np.float32)
    assert _dev_delta(Df, True) == 0.0
    assert _dev_delta(Df, False) == 0.0


def test_permutation_invariance_at_4096():
    from sttode_amd import delta
    rng = np.random.default_rng(78)
    n = 4096
    X = rng.standard_normal((n, 32)).astype(np.float32)
    perm = np.concatenate([[0], 1 + rng.permutation(n - 1)])             # the base point stays first
    d0, _ = delta.batched_deltas(X, np.arange(n)[None])
    d1, _ = delta.batched_deltas(X, perm[None])
    assert float(d0[0]) == float(d1[0]) and float(d0[0]) > 0


@pytest.mark.parametrize('d', [2, 128, 4096])
def test_distances_symmetric_accurate_and_gathered(d):
    from sttode_amd import delta
    dev = _gpu()
    rng = np.random.default_rng(d)
    rows, n = 700, 300
    X = rng.standard_normal((rows, d)).astype(np.float32)
    idx = rng.integers(0, rows, (2, n))
    Xt = torch.from_numpy(X).to(dev)
    ix = torch.from_numpy(idx.astype(np.int32)).to(dev)
    dist, diam = delta._dist(Xt, ix, 2, n)
    D = dist.cpu().numpy()
    for t in range(2):
        assert np.array_equal(D[t], D[t].T) and (np.diag(D[t]) == 0).all()
        ref = dist_f64(X[idx[t]])
        off = ref > 0
        assert (D[t][~off] == 0).all()                                     # repeated rows: exact zeros off the diagonal too
        assert np.max(np.abs(D[t][off] - ref[off]) / ref[off]) <= 1e-5
        assert float(diam[t]) == D[t].max()
        # the idx gather equals distances of the pre-gathered rows, bitwise
        g, gd = delta._dist(torch.from_numpy(np.ascontiguousarray(X[idx[t]])).to(dev), None, 1, n)
        assert torch.equal(g[0], dist[t]) and float(gd[0]) == float(diam[t])


def test_one_launch_across_tries_equals_one_try_calls():
    from sttode_amd import delta
    rng = np.random.default_rng(5)
    X = rng.standard_normal((2000, 64)).astype(np.float32)
    idx = rng.integers(0, 2000, (10, 400))
    dl, dm = delta.batched_deltas(X, idx)
    dl, dm = dl.cpu().numpy(), dm.cpu().numpy()
    for t in range(10):
        a, b = delta.batched_deltas(X, idx[t:t + 1])
        assert float(a[0]) == dl[t] and float(b[0]) == dm[t]
    # and the whole call against the restatement
    for t in (0, 9):
        D = delta._dist(torch.from_numpy(X).cuda(), torch.from_numpy(idx[t].astype(np.int32)).cuda()[None], 1, 400)[0][0].cpu().numpy()
        assert dl[t] == delta_f32(D)
    m, s = delta.batched_delta_hyp(X, n_tries=10, batch_size=400, idx=idx)
    v = dl.astype(np.float64) / dm.astype(np.float64)
    assert (m, s) == (np.mean(v), np.std(v))


_MODELS = {}


def _model(dataset='eth', Tp=8, Tf=12, hidden_dim=None):
    from sttode_amd import STTODENet
    from sttode_amd.weights import make_weights, to_torch_state_dict
    key = (dataset, Tp, Tf, hidden_dim)
    if key not in _MODELS:
        a = make_args(dataset, Tp, Tf)
        if hidden_dim is not None:
            from helpers import dims_case_weights
            a = a.__class__(**{**vars(a), 'hidden_dim': hidden_dim})
            w = dims_case_weights(a, seed=1234)
        else:
            w = make_weights(1234, past_length=Tp, future_length=Tf)
        m = STTODENet(a, _gpu()).eval()
        m.load_state_dict(to_torch_state_dict(w), strict=True)
        _MODELS[key] = m
    return _MODELS[key]


def _dataset(ids, kind):
    from test_selection_gpu import _dataset as ds
    return ds(ids, kind)


def test_embedding_delta_scenes():
    from sttode_amd import delta
    from sttode_amd.evaluate import embedding_delta
    m = _model('eth')
    ds = _dataset(range(5200, 5330), 'eth')
    n_agents = int(ds.obs_traj.shape[0])
    rows, trajs = [], []
    for s0 in range(0, len(ds), 48):                                       # the staged API, batch by batch
        sb = ds.scene_batch(range(s0, min(s0 + 48, len(ds))))
        m.set_scene_batch(sb.past, sb.future, sb.scene_ptr)
        rows.append(m.encode_history().clone())
        trajs.append((m.past_traj - m.cur_location).reshape(sb.n_agents, -1).clone())
    X = torch.cat(rows)
    assert X.shape == (n_agents, 128)
    np.random.seed(11)
    ref = delta.batched_delta_hyp(X, n_tries=3, batch_size=256)
    np.random.seed(11)
    got = embedding_delta(m, ds, n_tries=3, batch_size=256, scenes_per_call=48)
    assert got == ref and np.isfinite(got[0]) and got[0] > 0
    np.random.seed(12)
    ref_t = delta.batched_delta_hyp(torch.cat(trajs), n_tries=2, batch_size=200)
    np.random.seed(12)
    assert embedding_delta(m, ds, n_tries=2, batch_size=200, scenes_per_call=48, what='past_traj') == ref_t
    assert torch.cat(trajs).shape == (n_agents, 16)


@pytest.mark.parametrize('hidden_dim', [None, 128])
def test_embedding_delta_nba(hidden_dim):
    """NBA loader; hidden_dim 128 takes the generic form (generic.py): encode_history() after set_data_nba works on both forms."""
    from sttode_amd import delta, scenes
    from sttode_amd.evaluate import embedding_delta
    m = _model('nba', 5, 10, hidden_dim)
    assert m._generic == (hidden_dim is not None)
    loader = []
    for i, B in enumerate([16, 16, 9]):
        d = scenes.nba_batch(7700 + i, B, N=11)
        loader.append({'past_traj': torch.from_numpy(d['past_traj']), 'future_traj': torch.from_numpy(d['future_traj'])})
    rows = []
    for data in loader:
        m.set_data_nba(data)
        pf = m.encode_history()
        assert pf.shape[0] == data['past_traj'].shape[0] * 11 and bool(torch.isfinite(pf).all())
        rows.append(pf.clone())
    X = torch.cat(rows)
    assert X.shape[0] == 41 * 11
    np.random.seed(21)
    ref = delta.batched_delta_hyp(X, n_tries=2, batch_size=300)
    np.random.seed(21)
    got = embedding_delta(m, loader, n_tries=2, batch_size=300)
    assert got == ref and np.isfinite(got[0])
