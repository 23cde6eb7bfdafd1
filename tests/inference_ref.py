"""Plain restatements of the inference stages (csrc/frontend.hip, encoder.hip, decoder.hip, chain32.hip), one function per entry point,
for tests/test_inference_ref.py (the CPU pin) and tests/test_inference_kernels_gpu.py.

The torch stages are built from the oracle's own modules (oracle/sttode_ref.py: PastEncoder, its EncoderLayer, DecomposeBlock, Decoder)
loaded with sttode_amd.weights.make_weights(seed) and run in the dtype of the module set: ``nets(...)['f64']`` is the rounding-free yardstick,
``nets(...)['f32']`` torch's own fp32 evaluation of the same graph (how far a correct fp32 kernel may sit from float64).  Every function
returns all the tensors its kernel writes, in the kernel's layout.  The front-end is NumPy: float64, or float32 when given float32
(each value is then one rounding away from what set_data computes).

Case generators at the bottom are shared by both test files: weights by seed, tracks from sttode_amd.scenes, seeded normals where a
stage takes a raw tensor.  Stage inputs that an earlier stage produces are made by the fp32 restatement of that stage, so they have the
magnitudes the kernels see; the float64 reference of a stage is evaluated on those very fp32 values."""
import functools

import numpy as np
import torch
from torch.nn import functional as F

from helpers import make_args

F32, F64 = torch.float32, torch.float64
ATTN_CLAMP = 1e-4                      # core/manifolds/oblique.py:7
ODE_TIME = 12.0                        # model/STTODE.py:195
ODE_METHODS = ('euler', 'rk4', 'rk4_classic')


def tiles_x(Tp):
    return (2 * Tp + 15) // 16


def tiles_y(Tf):
    return (2 * Tf + 15) // 16


# ---------------------------------------------------------------------------------------------------------------------------------------
# module sets
# ---------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def nets(seed=1234, Tp=8, Tf=12, dataset='eth'):
    """{'f32': oracle, 'f64': the same weights in float64, 'sd': the NumPy state_dict the packers take}."""
    from oracle.sttode_ref import STTODENetRef
    from sttode_amd.weights import make_weights, to_torch_state_dict
    sd = make_weights(seed, past_length=Tp, future_length=Tf)
    out = {'sd': sd}
    for k in ('f32', 'f64'):
        m = STTODENetRef(make_args(dataset, Tp, Tf)).eval()
        m.load_state_dict(to_torch_state_dict(sd), strict=True)
        out[k] = m.double() if k == 'f64' else m
        for p in out[k].parameters():
            p.requires_grad_(False)
    return out


def _dt(net):
    return next(net.parameters()).dtype


def _t(a, net):
    """NumPy / torch value -> tensor in the module set's dtype (integers stay integers)."""
    a = torch.as_tensor(np.asarray(a)) if not torch.is_tensor(a) else a
    return a.to(_dt(net)) if a.is_floating_point() else a


# ---------------------------------------------------------------------------------------------------------------------------------------
# front-end (NumPy): set_data for scene batches, set_data_nba, inputs_for_posterior, the train-mode rotation
# ---------------------------------------------------------------------------------------------------------------------------------------
def _seqsum(v, dtype):
    """Sum in index order (what a loop over the agents computes); float64: the order does not matter at the tests' precision."""
    v = np.asarray(v, dtype)
    return np.cumsum(v, axis=0, dtype=dtype)[-1] if dtype == np.float32 else v.sum(axis=0)


def _pad(x2d, width):
    out = np.zeros((x2d.shape[0], width), x2d.dtype)
    out[:, :x2d.shape[1]] = x2d
    return out


def _vel(seq, prev=None):
    """First differences along axis 1; the first one duplicates the second (model/STTODE.py:432-433) unless the frame before is given."""
    v = seq[:, 1:] - seq[:, :-1]
    first = v[:, :1] if prev is None else (seq[:, :1] - prev[:, None, :])
    return np.concatenate([first, v], axis=1)


def frontend_scenes(past, scene_ptr, vel_from_norm, dtype=np.float64):
    """model/STTODE.py:397-461 over the scenes of a CSR.  past [n, Tp, 2] -> dict scene_orig [S, 2], agent_scene [n], xpad [n, 16 TPX],
    enc_in [n, Tp, 4], cur, orig [n, 2], last [n].  vel_from_norm 1: velocities of the normalised track (inference(), :582-583)."""
    past = np.asarray(past, dtype)
    ptr = np.asarray(scene_ptr, np.int64)
    n, Tp = past.shape[0], past.shape[1]
    S = len(ptr) - 1
    so = np.stack([_seqsum(past[ptr[s]:ptr[s + 1], -1], dtype) / dtype(ptr[s + 1] - ptr[s]) for s in range(S)]).astype(dtype)
    ags = np.repeat(np.arange(S), np.diff(ptr)).astype(np.int32)
    orig = so[ags]
    norm = past - orig[:, None, :]
    vel = _vel(norm) if vel_from_norm else _vel(past)
    last = np.zeros(n, np.int32)
    last[ptr[1:] - 1] = 1
    return dict(scene_orig=so, agent_scene=ags, xpad=_pad(norm.reshape(n, 2 * Tp), 16 * tiles_x(Tp)),
                enc_in=np.concatenate([norm, vel], axis=-1), cur=norm[:, -1].copy(), orig=orig, last=last)


def frontend_nba(past, N, dtype=np.float64):
    """model/STTODE.py:463-486: no normalisation, orig = 0, the flag on slot N - 1 (add_category, :199-210)."""
    past = np.asarray(past, dtype)
    n, Tp = past.shape[0], past.shape[1]
    last = (np.arange(n) % N == N - 1).astype(np.int32)
    return dict(xpad=_pad(past.reshape(n, 2 * Tp), 16 * tiles_x(Tp)), enc_in=np.concatenate([past, _vel(past)], axis=-1),
                cur=past[:, -1].copy(), orig=np.zeros((n, 2), dtype), last=last)


def frontend_future(future, past_last, mode, scene_orig=None, agent_scene=None, dtype=np.float64):
    """inputs_for_posterior (model/STTODE.py:430,434,457; 477,481): (future - scene origin, future - the frame before) [n, Tf, 4];
    mode 0 scenes, 1 NBA (origin 0).  The velocities are those of the world track in both modes."""
    fut, pl = np.asarray(future, dtype), np.asarray(past_last, dtype)
    orig = np.asarray(scene_orig, dtype)[np.asarray(agent_scene)] if mode == 0 else np.zeros((fut.shape[0], 2), dtype)
    return np.concatenate([fut - orig[:, None, :], _vel(fut, pl)], axis=-1)


def rotate_scene(past, fut, c, s, dtype=np.float64):
    """rotation_2d_torch about the mean last observed position (model/STTODE.py:6-14,417-426): x' = R (x - o) + o, R = [[c, -s], [s, c]]."""
    past = np.asarray(past, dtype)
    c, s = dtype(c), dtype(s)
    o = _seqsum(past[:, -1], dtype) / dtype(past.shape[0])

    def rot(x):
        d = np.asarray(x, dtype) - o
        return np.stack([(d[..., 0] * c + d[..., 1] * (-s)) + o[0], (d[..., 0] * s + d[..., 1] * c) + o[1]], axis=-1).astype(dtype)
    return rot(past), (rot(fut) if fut is not None else None)


# ---------------------------------------------------------------------------------------------------------------------------------------
# encoder trunk
# ---------------------------------------------------------------------------------------------------------------------------------------
def _layer(trunk):
    return trunk.ODE_Encoder.odeblock.odefunc.layers[0]


def embed_qkv(trunk, enc_in, last):
    """PastEncoder / FutureEncoder up to the packed in-projection (model/STTODE.py:214-223): g [n, 64], qkv [n, 192] (q unscaled).
    ``last`` [n]: the add_category flag of each agent (any subset; the module ties it to the agent's index)."""
    enc_in = _t(enc_in, trunk)
    n, T = enc_in.shape[0], enc_in.shape[1]
    x = trunk.pos_encoder(trunk.input_fc(enc_in)).reshape(n, T * trunk.model_dim)
    cat = torch.zeros(n, 3, dtype=enc_in.dtype)
    cat[:, 2] = _t(last, trunk).to(enc_in.dtype)
    g = trunk.input_fc3(torch.cat([trunk.input_fc2(x), cat], dim=-1))
    mha = _layer(trunk).self_attn.temporal_attention_before
    return dict(g=g, qkv=F.linear(g, mha.in_proj_weight, mha.in_proj_bias))


def attention(R, C, V, rscale=1.0, cscale=1.0, hd=8):
    """out_i = sum_j softmax_j(-acos(clamp(<r_i / |r_i|, c_j / |c_j|>, -1 + 1e-4, 1 - 1e-4))) v_j per (slot, head); R [rows, Nb, 8 hd],
    C, V [cols, Nb, 8 hd].  Self-attention of the model: R = k, C = q with cscale = hd ** -0.5 (the untransposed-score quirk,
    hyptransformerlib.py:261-265).  -> out [rows, Nb, 8 hd], weights [Nb, rows, cols] (mean over the heads), rowsum [Nb, 8, rows]
    (sum_j exp(score): the kernel's softmax has no maximum subtraction, scores lie in [-pi, 0])."""
    rows, Nb = R.shape[0], R.shape[1]
    cols = C.shape[0]
    r = (R * rscale).reshape(rows, Nb, 8, hd)
    c = (C * cscale).reshape(cols, Nb, 8, hd)
    r = r / r.norm(dim=-1, keepdim=True)
    c = c / c.norm(dim=-1, keepdim=True)
    s = -torch.acos(torch.einsum('ibhd,jbhd->bhij', r, c).clamp(-1 + ATTN_CLAMP, 1 - ATTN_CLAMP))
    P = torch.softmax(s, dim=-1)
    out = torch.einsum('bhij,jbhd->ibhd', P, V.reshape(cols, Nb, 8, hd)).reshape(rows, Nb, 8 * hd)
    return dict(out=out, weights=P.mean(dim=1), rowsum=torch.exp(s).sum(-1))


def layer_rhs(trunk, y, attn):
    """f(y) of the encoder's ODE with the attention output of y given: out_proj -> tanh(info) * sigmoid(gate) -> post-LN -> FFN -> post-LN
    (hypertransformer.py:81-83,134-153)."""
    L = _layer(trunk)
    a = L.self_attn.temporal_attention_before.out_proj(attn)
    gate = torch.tanh(L.self_attn.temporal_info(a)) * torch.sigmoid(L.self_attn.temporal_gate(a))
    h = L.norm1(y + gate)
    return L.norm2(h + L.linear2(torch.relu(L.linear1(h))))


def post_attn(trunk, g, attn, ode_time=ODE_TIME):
    """One Euler step of size ode_time, relu, pf = cat(g, .) (ode_demo.py:186-190,223-231; model/STTODE.py:233-235)."""
    g, attn = _t(g, trunk), _t(attn, trunk)
    return torch.cat([g, torch.relu(g + ode_time * layer_rhs(trunk, g, attn))], dim=-1)


def post_attn_rhs(trunk, y, attn):
    return layer_rhs(trunk, _t(y, trunk), _t(attn, trunk))


def value_of(trunk, y):
    """Attention output of a state at attention length 1: the softmax over one key is 1, so it is the value projection."""
    mha = _layer(trunk).self_attn.temporal_attention_before
    return F.linear(y, mha.in_proj_weight[128:], mha.in_proj_bias[128:])


def post_attn_ode(trunk, g, method, steps, ode_time=ODE_TIME):
    """The same layer under a fixed-grid integrator at attention length 1: method 0 Euler, 1 the 3/8 rule (torchdiffeq's fixed-grid rk4),
    2 the classical RK4; ``steps`` uniform steps over [0, ode_time].  -> pf [n, 128] = cat(g, relu(y(T)))."""
    g = _t(g, trunk)
    f = lambda y: layer_rhs(trunk, y, value_of(trunk, y))
    h = ode_time / steps
    y = g
    for _ in range(steps):
        k1 = f(y)
        if method == 0:
            y = y + h * k1
        elif method == 1:
            k2 = f(y + h * k1 / 3)
            k3 = f(y + h * (k2 - k1 / 3))
            k4 = f(y + h * (k1 - k2 + k3))
            y = y + h * (k1 + 3 * (k2 + k3) + k4) / 8
        else:
            k2 = f(y + h * k1 / 2)
            k3 = f(y + h * k2 / 2)
            k4 = f(y + h * k3)
            y = y + h * (k1 + 2 * k2 + 2 * k3 + k4) / 6
    return ode_state_to_pf(g, y)


def ode_state_to_pf(g, y):
    return torch.cat([g, torch.relu(y)], dim=-1)


def past_feature(net, enc_in, last, B, N):
    """The stages composed: embed -> attention over the B scenes of a forward call (slots = the N agents; B = 1: the value itself)
    -> post_attn.  enc_in [B N, Tp, 4] -> pf [B N, 128]."""
    tr = net.past_encoder
    e = embed_qkv(tr, enc_in, last)
    if B == 1:
        attn = e['qkv'][:, 128:]
    else:
        q, k, v = (e['qkv'][:, 64 * i:64 * i + 64].reshape(B, N, 64) for i in range(3))
        attn = attention(k, q, v, 1.0, 8.0 ** -0.5)['out'].reshape(B * N, 64)
    return post_attn(tr, e['g'], attn)


# ---------------------------------------------------------------------------------------------------------------------------------------
# decoder
# ---------------------------------------------------------------------------------------------------------------------------------------
def gru_state(blk, xin, Tp):
    """DecomposeBlock front half (model/STTODE.py:62-69): conv1d(2 -> 32, k 3, pad 1) + relu, GRU(32 -> 96) final state.
    xin [m, >= 2 Tp] flattened (t, c) -> state [m, 96]."""
    xin = _t(xin, blk)
    x = xin[:, :2 * Tp].reshape(-1, Tp, 2)
    e = torch.relu(blk.conv_past(x.transpose(1, 2))).transpose(1, 2)
    return blk.encoder_past(e)[1].squeeze(0)


def agent_preact(dec, pf, state0):
    """Per-agent part of layer 1 of decoder_x / decoder_y of block 0 (k = [pf | state0]) and of decoder_y of block 1 (k = pf), bias
    included: the split of model/STTODE.py:71,74-75 over feat = [pf | z | state]."""
    b0, b1 = dec.decompose[0], dec.decompose[1]
    pf, state0 = _t(pf, dec), _t(state0, dec)
    ps = torch.cat([pf, state0], dim=-1)

    def part(lin, with_state):
        W = lin.weight
        return F.linear(ps, torch.cat([W[:, :128], W[:, 160:]], dim=1), lin.bias) if with_state else F.linear(pf, W[:, :128], lin.bias)
    return dict(A0x=part(b0.decoder_x.layers[0], True), A0y=part(b0.decoder_y.layers[0], True), A1y=part(b1.decoder_y.layers[0], False))


def _mlp_tail(mlp, A, kcols, v, K, width):
    """relu(A[agent] + W1[:, kcols] v) -> relu(layer 2) -> layer 3, zero padded to ``width`` columns; column c belongs to agent c // K."""
    A, v = _t(A, mlp), _t(v, mlp)
    l1, l2, l3 = mlp.layers
    h = torch.relu(A.repeat_interleave(K, dim=0) + v @ l1.weight[:, kcols].T)
    o = l3(torch.relu(l2(h)))
    return F.pad(o, (0, width - o.shape[1]))


def mlp_block0(dec, A0x, A0y, z, xpad, K, Tp, Tf):
    """Block 0's back half (model/STTODE.py:71-75,336-339): dbuf = x_true - x_hat0 [m, 16 TPX], ybuf = y_hat0 [m, 16 NOY]."""
    b0 = dec.decompose[0]
    xh = _mlp_tail(b0.decoder_x, A0x, slice(128, 160), z, K, 16 * tiles_x(Tp))
    xp = _t(xpad, dec)[:, :16 * tiles_x(Tp)]
    return dict(dbuf=xp.repeat_interleave(K, dim=0) - xh, ybuf=_mlp_tail(b0.decoder_y, A0y, slice(128, 160), z, K, 16 * tiles_y(Tf)))


def mlp_block1(dec, A1y, z, state1, ybuf, cur, orig, K, Tf):
    """Block 1's back half and the epilogue (model/STTODE.py:338,343-346,621-622): pred [m, Tf, 2] = ((y_hat0 + y_hat1) + cur) + orig."""
    b1 = dec.decompose[1]
    zs = torch.cat([_t(z, dec), _t(state1, dec)], dim=-1)
    y1 = _mlp_tail(b1.decoder_y, A1y, slice(128, 256), zs, K, 2 * Tf)
    y = (_t(ybuf, dec)[:, :2 * Tf] + y1).reshape(-1, Tf, 2)
    return (y + _t(cur, dec).repeat_interleave(K, dim=0)[:, None, :]) + _t(orig, dec).repeat_interleave(K, dim=0)[:, None, :]


def mlp_cols(mlp, A0, z, state, K, NO):
    """One decoder MLP of a non-first block with k = [z | state] per column, raw output tiles [m, 16 NO]."""
    return _mlp_tail(mlp, A0, slice(128, 256), torch.cat([_t(z, mlp), _t(state, mlp)], dim=-1), K, 16 * NO)


def traj_chain(dec, A0x, A0y, A1y, z, xpad, cur, orig, K, Tp, Tf):
    """The per-trajectory chain of Decoder.forward (model/STTODE.py:320-347): block 0 MLPs -> block 1 conv + GRU -> block 1 decoder_y ->
    epilogue.  -> dict dbuf, ybuf, state1, pred."""
    o = mlp_block0(dec, A0x, A0y, z, xpad, K, Tp, Tf)
    o['state1'] = gru_state(dec.decompose[1], o['dbuf'], Tp)
    o['pred'] = mlp_block1(dec, A1y, z, o['state1'], o['ybuf'], cur, orig, K, Tf)
    return o


def decode(net, pf, z, xpad, cur, orig, K, Tp, Tf):
    """The decoder stages composed from past_feature on: -> dict state0, A0x, A0y, A1y, dbuf, ybuf, state1, pred [n K, Tf, 2]."""
    dec = net.decoder
    o = dict(state0=gru_state(dec.decompose[0], xpad, Tp))
    o.update(agent_preact(dec, pf, o['state0']))
    o.update(traj_chain(dec, o['A0x'], o['A0y'], o['A1y'], z, xpad, cur, orig, K, Tp, Tf))
    return o


def inference_scenes(net, past, scene_ptr, z, K=20):
    """inference() over a batch of independent scenes, stage by stage in the dtype of ``net``: -> dict of every stage's tensors; pred
    [n K, Tf, 2] in world coordinates (row = agent K + k)."""
    a = net.args
    npdt = np.float64 if _dt(net) == F64 else np.float32
    fe = frontend_scenes(past, scene_ptr, 1, npdt)
    pf = past_feature(net, fe['enc_in'], fe['last'], 1, 1)
    o = decode(net, pf, z, fe['xpad'], fe['cur'], fe['orig'], K, a.past_length, a.future_length)
    o.update(fe, pf=pf)
    return o


def inference_nba(net, past, B, N, z, K=20):
    """inference() of one NBA forward call: past [B N, Tp, 2]; attention over the B scenes per agent slot."""
    a = net.args
    fe = frontend_nba(past, N, np.float64 if _dt(net) == F64 else np.float32)
    pf = past_feature(net, fe['enc_in'], fe['last'], B, N)
    o = decode(net, pf, z, fe['xpad'], fe['cur'], fe['orig'], K, a.past_length, a.future_length)
    o.update(fe, pf=pf)
    return o


# ---------------------------------------------------------------------------------------------------------------------------------------
# case generators (fp32 inputs; shared by the CPU pin and the GPU file)
# ---------------------------------------------------------------------------------------------------------------------------------------
def scene_case(sizes, Tp=8, Tf=12, seed=0):
    """A scene batch with exactly ``sizes`` agents per scene: (past [n, Tp, 2], future [n, Tf, 2], scene_ptr [S + 1]) fp32 / int32."""
    from sttode_amd import scenes
    past, fut = [], []
    for i, s in enumerate(sizes):
        o, p = scenes.eth_scene(7000 + 131 * seed + i, Tp, Tf, n_min=s, n_max=s)
        past.append(o.transpose(0, 2, 1))
        fut.append(p.transpose(0, 2, 1))
    return (np.ascontiguousarray(np.concatenate(past)), np.ascontiguousarray(np.concatenate(fut)),
            np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32))


def nba_case(B, N, Tp=5, Tf=10, seed=0):
    """(past [B N, Tp, 2], future [B N, Tf, 2]) of scenes.nba_batch."""
    from sttode_amd import scenes
    d = scenes.nba_batch(900 + seed, B, N=N, obs_len=Tp, pred_len=Tf)
    return (np.ascontiguousarray(d['past_traj'].reshape(B * N, Tp, 2)), np.ascontiguousarray(d['future_traj'].reshape(B * N, Tf, 2)))


def normals(seed, *shape, scale=1.0):
    return (scale * np.random.default_rng(seed).standard_normal(shape)).astype(np.float32)


def last_flags(n, which):
    """'none' | 'all' | 'ragged' (a seeded subset that holds both values whenever n > 1)."""
    if which == 'none':
        return np.zeros(n, np.int32)
    if which == 'all':
        return np.ones(n, np.int32)
    f = (np.random.default_rng(n).random(n) < 0.4).astype(np.int32)
    if n > 1:
        f[0], f[-1] = 0, 1
    return f


@functools.lru_cache(maxsize=None)
def embed_case(n, Tlen, flags, seed=1234):
    """Inputs of sttode_embed_qkv: a trunk for Tlen frames, enc_in [n, Tlen, 4] of a normalised scene, flags [n]."""
    past, _, ptr = scene_case([n], max(Tlen, 2), 12, seed=Tlen)
    fe = frontend_scenes(past, ptr, 1, np.float32)
    return dict(n=n, Tlen=Tlen, enc_in=np.ascontiguousarray(fe['enc_in'][:, :Tlen]), last=last_flags(n, flags), seed=seed)


@functools.lru_cache(maxsize=None)
def trunk_state_case(n, seed=1234):
    """Inputs of the post-attention kernels: g [n, 64] and qkv [n, 192] of a scene through the fp32 embedding."""
    c = embed_case(n, 8, 'ragged', seed)
    with torch.no_grad():
        e = embed_qkv(nets(seed)['f32'].past_encoder, c['enc_in'], c['last'])
    return dict(n=n, g=e['g'].numpy(), qkv=e['qkv'].numpy(), seed=seed)


@functools.lru_cache(maxsize=None)
def decoder_case(n, K, Tp, Tf, seed=1234):
    """Inputs of every decoder kernel for n agents x K samples: xpad [n, 32] (zero beyond 2 Tp), cur, orig, pf, z and, through the fp32
    restatement, state0, A0x / A0y / A1y, dbuf, ybuf, state1."""
    rng = np.random.default_rng(100000 + 1000 * n + 10 * K + Tp + 7 * Tf)
    walk = np.cumsum(rng.normal(0.0, 0.4, (n, Tp, 2)), axis=1) + rng.normal(0.0, 3.0, (n, 1, 2))
    xpad = np.zeros((n, 32), np.float32)
    xpad[:, :2 * Tp] = walk.reshape(n, 2 * Tp)
    pf = rng.standard_normal((n, 128)).astype(np.float32)
    pf[:, 64:] = np.maximum(pf[:, 64:], 0)                   # the ODE half of past_feature is a relu output
    c = dict(n=n, K=K, Tp=Tp, Tf=Tf, seed=seed, xpad=xpad, pf=pf, cur=np.ascontiguousarray(xpad[:, 2 * Tp - 2:2 * Tp]),
             orig=rng.normal(0.0, 5.0, (n, 2)).astype(np.float32), z=rng.standard_normal((n * K, 32)).astype(np.float32))
    with torch.no_grad():
        o = decode(nets(seed, Tp, Tf)['f32'], c['pf'], c['z'], c['xpad'], c['cur'], c['orig'], K, Tp, Tf)
    c.update({k: o[k].numpy() for k in ('state0', 'A0x', 'A0y', 'A1y', 'dbuf', 'ybuf', 'state1')})
    return c
