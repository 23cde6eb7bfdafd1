"""Plain-torch restatement of the attention core (two score modes, optional additive mask) and of the two stand-alone attention
modules, in whatever dtype the operands have (float32 or float64).  Written from the formulas of DESIGN.md §4o:

    mode 0 (geodesic)     s = -acos(clamp(<r^, c^>, -1+1e-4, 1-1e-4)),  r = rscale R, c = cscale C, ^ = / |.|
    mode 1 (dot product)  s = <rscale R, cscale C>
    P = softmax_cols(s + mask),  out = P V,  weights = mean over the 8 heads of P

Operands [len, Nb, 64] (8 heads x 8 dims).  tests/test_attention.py pins these against the reference's own results
(tests/golden/attention.npz); tests/test_attention_gpu.py uses them as the yardstick of the HIP kernels."""
import torch
from torch import nn
from torch.nn import functional as F

LO, HI = -1 + 1e-4, 1 - 1e-4


def core(R, C, V, rs, cs, mode, mask=None):
    """-> (out [rows, Nb, 64], head-averaged weights [Nb, rows, cols]); mask [rows, cols] or None."""
    rows, Nb, _ = R.shape
    cols = C.shape[0]
    r = (R * rs).reshape(rows, Nb, 8, 8)
    c = (C * cs).reshape(cols, Nb, 8, 8)
    if mode == 0:
        r = r / r.norm(dim=-1, keepdim=True)
        c = c / c.norm(dim=-1, keepdim=True)
    s = torch.einsum('rbhd,cbhd->bhrc', r, c)
    if mode == 0:
        s = -torch.acos(s.clamp(LO, HI))
    if mask is not None:
        s = s + mask.to(s.dtype)
    P = torch.softmax(s, dim=-1)
    out = torch.einsum('bhrc,cbhd->rbhd', P, V.reshape(cols, Nb, 8, 8)).reshape(rows, Nb, 64)
    return out, P.mean(dim=1)


def orientation(mode, L, S):
    """(rows are keys?, rscale, cscale): geodesic scores with L == S are used untransposed (rows = keys, columns = queries); every other
    case has rows = queries.  The query side carries head_dim ** -0.5."""
    sc = 8 ** -0.5
    return (True, 1.0, sc) if (mode == 0 and L == S) else (False, sc, 1.0)


def attention(mode, query, key, value, in_w, in_b, out_w, out_b, mask=None):
    """Both modules' forward: packed in-projection, core, out_proj.  -> (out [L, Nb, 64], weights [Nb, L, S])."""
    E = 64
    q = F.linear(query, in_w[:E], in_b[:E])
    k = F.linear(key, in_w[E:2 * E], in_b[E:2 * E])
    v = F.linear(value, in_w[2 * E:], in_b[2 * E:])
    swap, rs, cs = orientation(mode, query.shape[0], key.shape[0])
    o, w = core(k, q, v, rs, cs, mode, mask) if swap else core(q, k, v, rs, cs, mode, mask)
    return F.linear(o, out_w, out_b), w


class AttentionRef(nn.Module):
    """Parameter holder with the reference modules' names; mode 0 = Hyp_mhsa, 1 = MultiheadAttention."""

    def __init__(self, mode):
        super().__init__()
        self.mode = mode
        self.in_proj_weight = nn.Parameter(torch.zeros(192, 64))
        self.in_proj_bias = nn.Parameter(torch.zeros(192))
        self.out_proj = nn.Linear(64, 64)

    def forward(self, query, key, value, attn_mask=None):
        return attention(self.mode, query, key, value, self.in_proj_weight, self.in_proj_bias, self.out_proj.weight, self.out_proj.bias,
                         attn_mask)


class GatedAttentionRef(nn.Module):
    """Hypattention (hypertransformer.py:19-89) around a Euclidean core: attention over [T, N*sample_num, D], then tanh(info) * sigmoid(gate)."""

    def __init__(self):
        super().__init__()
        self.temporal_attention_before = AttentionRef(1)
        self.temporal_info = nn.Linear(64, 64)
        self.temporal_gate = nn.Linear(64, 64)

    def forward(self, q, k, v):
        Lq, A, Sn, D = q.shape
        o, _ = self.temporal_attention_before(q.reshape(Lq, A * Sn, D), k.reshape(k.shape[0], A * Sn, D), v.reshape(v.shape[0], A * Sn, D))
        o = o.reshape(Lq, A, Sn, D)
        return torch.tanh(self.temporal_info(o)) * torch.sigmoid(self.temporal_gate(o))


class EncoderLayerRef(nn.Module):
    """TransformerEncoderLayer (hypertransformer.py:91-153) with Euclidean attention: post-LayerNorm, relu FFN."""

    def __init__(self, ff=256):
        super().__init__()
        self.self_attn = GatedAttentionRef()
        self.linear1, self.linear2 = nn.Linear(64, ff), nn.Linear(ff, 64)
        self.norm1, self.norm2 = nn.LayerNorm(64), nn.LayerNorm(64)

    def forward(self, src):
        src = self.norm1(src + self.self_attn(src, src, src))
        return self.norm2(src + self.linear2(torch.relu(self.linear1(src))))


class DecoderLayerRef(nn.Module):
    """TransformerDecoderLayer (hypertransformer.py:156-236) with Euclidean attention."""

    def __init__(self, ff=256):
        super().__init__()
        self.self_attn, self.cross_attn = GatedAttentionRef(), GatedAttentionRef()
        self.linear1, self.linear2 = nn.Linear(64, ff), nn.Linear(ff, 64)
        self.norm1, self.norm2, self.norm3 = nn.LayerNorm(64), nn.LayerNorm(64), nn.LayerNorm(64)

    def forward(self, tgt, memory):
        tgt = self.norm1(tgt + self.self_attn(tgt, tgt, tgt))
        tgt = self.norm2(tgt + self.cross_attn(tgt, memory, memory))
        return self.norm3(tgt + self.linear2(torch.relu(self.linear1(tgt))))
