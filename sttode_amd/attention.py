"""Stand-alone attention modules on the HIP kernels: drop-ins for the reference's two multi-head attention classes, with the
reference's constructor signature, parameter names, initialisation and call signature:

    MultiheadAttention(embed_dim, num_heads, ...)     transformerlib.py:295-445      dot-product scores (the Euclidean baseline)
    Hyp_mhsa(embed_dim, num_heads, ...)               hyptransformerlib.py:314-454   geodesic scores on the oblique manifold

Both run ``ops.mha`` / ``ops.mhgsa``: embed_dim = 64, num_heads = 8 (the kernels' build); dropout, bias=False, add_bias_kv, add_zero_attn,
kdim / vdim other than embed_dim and a sparse gate raise NotImplementedError at construction.

``attn_mask`` (float32 [L, S]) is added to the scores before the softmax, as in the reference (hyptransformerlib.py:290-292,
transformerlib.py:276-279).  In Hyp_mhsa with L == S the reference uses the scores untransposed (rows = keys, columns = queries) and adds
the mask to that matrix as it stands; so does this.  ``key_padding_mask`` is accepted and IGNORED: in both reference modules the code that
would apply it is commented out (hyptransformerlib.py:270-276, transformerlib.py:258-264), so honouring it would change results.
``cross_range``, ``interaction_mask`` and ``seq_mask`` feed only the sparse gate and are ignored too.

Values only by default; ``hypertransformer.trainable(module)`` switches autograd on (HIP backward, attention weights not differentiable).
"""
import torch
from torch import nn

from . import capi
from .ops import mha, mhgsa


class _Attention(nn.Module):
    _op = None

    def __init__(self, embed_dim, num_heads, dropout=0., bias=True, add_bias_kv=False, add_zero_attn=False, kdim=None, vdim=None,
                 sparse_gate_class=None):
        super().__init__()
        name = type(self).__name__
        if embed_dim != 64 or num_heads != 8:
            raise NotImplementedError(f'{name}: the HIP attention core is built for embed_dim=64, num_heads=8')
        if dropout != 0.:
            raise NotImplementedError(f'{name}: dropout must be 0')
        if not bias or add_bias_kv or add_zero_attn:
            raise NotImplementedError(f'{name}: bias=False, add_bias_kv and add_zero_attn are not built')
        if (kdim is not None and kdim != embed_dim) or (vdim is not None and vdim != embed_dim):
            raise NotImplementedError(f'{name}: kdim and vdim must equal embed_dim')
        if sparse_gate_class is not None:
            raise NotImplementedError(f'{name}: sparse gates are not built')
        self.embed_dim, self.kdim, self.vdim = embed_dim, embed_dim, embed_dim
        self.num_heads, self.dropout, self.head_dim = num_heads, dropout, embed_dim // num_heads
        self.in_proj_weight = nn.Parameter(torch.empty(3 * embed_dim, embed_dim))
        self.in_proj_bias = nn.Parameter(torch.empty(3 * embed_dim))
        self.out_proj = nn.Linear(embed_dim, embed_dim, bias=True)
        self.bias_k = self.bias_v = None
        self.add_zero_attn = False
        self.sparse_attn_gate = None
        self._trainable = False
        self._reset_parameters()

    def _reset_parameters(self):
        nn.init.xavier_uniform_(self.in_proj_weight)
        nn.init.constant_(self.in_proj_bias, 0.)
        nn.init.constant_(self.out_proj.bias, 0.)

    def forward(self, query, key, value, key_padding_mask=None, need_weights=True, attn_mask=None, cross_range=0, interaction_mask=None,
                seq_mask=False):
        """query [L,Nb,64], key / value [S,Nb,64] -> (out [L,Nb,64], head-averaged weights [Nb,L,S] | None).  ``key_padding_mask`` is
        accepted and ignored, as the reference ignores it."""
        if query.device.type != 'cuda':
            raise capi.SttodeError(f'{type(self).__name__} runs only on a HIP device (no CPU fallback)')
        grad = (self._trainable and torch.is_grad_enabled()
                and (any(t.requires_grad for t in (query, key, value)) or any(p.requires_grad for p in self.parameters())))
        return type(self)._op(query, key, value, self.in_proj_weight, self.in_proj_bias, self.out_proj.weight, self.out_proj.bias,
                              num_heads=self.num_heads, need_weights=need_weights, attn_mask=attn_mask, differentiable=grad)


class MultiheadAttention(_Attention):
    """transformerlib.MultiheadAttention: softmax(q k^T / sqrt(head_dim) + attn_mask) v."""
    _op = staticmethod(mha)


class Hyp_mhsa(_Attention):
    """hyptransformerlib.Hyp_mhsa: softmax(-acos(clamp(<q^, k^>)) + attn_mask) v, with the reference's untransposed scores for L == S."""
    _op = staticmethod(mhgsa)
