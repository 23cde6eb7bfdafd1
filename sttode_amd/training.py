"""Training step on the HIP kernels: forward-with-tape and backward of ``STTODENet.forward()``.

Reference: model/STTODE.py:553-568 (objective), :372-395 (losses), :214-236 / :276-300 (encoders), :320-347 / :51-77
(decoder), hypertransformer.py:134-153 + hyptransformerlib.py:191-300 (encoder layer / geodesic attention),
ode_demo.py:188,228 (one Euler step of size 12 + relu); what ``train.py:81-87`` drives through ``total_loss.backward()``.

Every network evaluation, loss and gradient runs in ``csrc/train*.hip`` kernels (generic MFMA linear / weight-gradient
kernels over the row-major nn.Parameter storage, plus the element-wise pieces).  PyTorch only allocates buffers and, via
one ``autograd.Function``, hands the finished gradients to ``.grad`` so that ``optimizer.step()`` works unchanged.
There is no eager / CPU fallback.
"""
import contextlib
import ctypes
import os

import torch

from . import capi, odestages
from .capi import SttodeError

# backward over the decoder columns that carry a gradient (Engine.decoder_live).  False -- over all 21 per agent, as rounds 1-4 -- is a test
# reference only (tests/test_gpu_parity.py::test_live_column_backward_equals_the_dense_backward sets it); part of the graph key
_LIVE_COLUMNS = True
_GATHER_MAX = 32
_K1 = 21                      # decoder columns per agent in forward(): the posterior draw + the 20 prior draws


class _OdeCombine(ctypes.Structure):                 # include/sttode_hip.h SttodeOdeCombine (sttode_ode_combine)
    _fields_ = [('v', ctypes.c_void_p * 6), ('ld', ctypes.c_long * 6), ('c', ctypes.c_float * 6), ('out', ctypes.c_void_p),
                ('ld_out', ctypes.c_long), ('relu_out', ctypes.c_void_p), ('ld_relu', ctypes.c_long), ('mask', ctypes.c_void_p),
                ('ld_mask', ctypes.c_long), ('nterms', ctypes.c_int), ('rows', ctypes.c_int)]


class _OdeProgram(ctypes.Structure):                 # include/sttode_hip.h SttodeOdeProgram (sttode_ttrunk_ode_fwd)
    _fields_ = [('stages', ctypes.c_int), ('steps', ctypes.c_int), ('h', ctypes.c_float), ('a', ctypes.c_float * 16), ('b', ctypes.c_float * 4)]


class _OdeStageBwd(ctypes.Structure):                # include/sttode_hip.h SttodeOdeStageBwd (sttode_ode_stage_bwd)
    _fields_ = [('w', ctypes.c_void_p * 16), ('y', ctypes.c_void_p), ('kb', _OdeCombine), ('dy', ctypes.c_void_p), ('next', _OdeCombine)] + \
               [(k, ctypes.c_void_p) for k in ('attn', 'ao', 'h', 'f1', 'dsum2', 'df1', 'du', 'dv', 'dao', 'dattn', 'ln')] + [('n', ctypes.c_int)]


class _GatherItem(ctypes.Structure):                 # csrc/train_ewise.hip GatherItem (include/sttode_hip.h sttode_live_rows_gather)
    _fields_ = [('src', ctypes.c_void_p), ('dst', ctypes.c_void_p), ('src_plane', ctypes.c_long),
                ('dst_plane', ctypes.c_long), ('row', ctypes.c_int), ('outer', ctypes.c_int)]


EW_MUL, EW_AXPY, EW_GATE_BWD, EW_EULER_FWD, EW_EULER_BWD, EW_RSAMPLE, EW_RELU_BWD, EW_FILL, EW_RSAMPLE_BWD, EW_CUR_ADD = range(10)
EW_TANH_BWD, EW_LATENT_BWD, EW_SUM_CUR, EW_EULER_BWD_CAT, EW_SCALE_ADD, EW_AXPY_ROWS = 10, 11, 12, 13, 14, 15
ACT = {None: 0, 'relu': 1, 'tanh': 2, 'sigmoid': 3}
_ATT = 'ODE_Encoder.odeblock.odefunc.layers.0.'
_SA = _ATT + 'self_attn.temporal_attention_before.'
# A trunk's parameters, role -> name below the trunk's prefix, in the order of capi.TRUNK_PTRS (the fused launch's table): the layers in
# front of the ODE block, then the ODE block's encoder layer in the order of SttodeOdeStageBwd.w[] as well
_FRONT = dict(fc1_w='input_fc.weight', fc1_b='input_fc.bias', pos_w='pos_encoder.fc.weight', pos_b='pos_encoder.fc.bias',
              fc2_w='input_fc2.weight', fc2_b='input_fc2.bias', fc3_w='input_fc3.weight', fc3_b='input_fc3.bias')
_LAYER = dict(inproj_w=_SA + 'in_proj_weight', inproj_b=_SA + 'in_proj_bias', out_w=_SA + 'out_proj.weight', out_b=_SA + 'out_proj.bias',
              info_w=_ATT + 'self_attn.temporal_info.weight', info_b=_ATT + 'self_attn.temporal_info.bias',
              gate_w=_ATT + 'self_attn.temporal_gate.weight', gate_b=_ATT + 'self_attn.temporal_gate.bias',
              ln1_w=_ATT + 'norm1.weight', ln1_b=_ATT + 'norm1.bias', l1_w=_ATT + 'linear1.weight', l1_b=_ATT + 'linear1.bias',
              l2_w=_ATT + 'linear2.weight', l2_b=_ATT + 'linear2.bias', ln2_w=_ATT + 'norm2.weight', ln2_b=_ATT + 'norm2.bias')
assert tuple(_FRONT) + tuple(_LAYER) == capi.TRUNK_PTRS[:24] and len(_LAYER) == 16


# the first block's conv + GRU once per agent.  False -- per trajectory column -- is a test reference only (the same test); part of the graph key
_AGENT_GRU = True
_SCRATCH_BATCH = 32 << 20     # floats (128 MB): split sums of one backward pass at batch sizes (more than 2048 GEMM columns)
_TGEMM_MIN_COLS_BWD = 600     # == TGEMM_MIN_COLS_BWD of csrc/train_gemm.hip: backward products above it take the LDS-tiled GEMM (split sums)
# non-default encoder integrators: cap of the per-stage activation and gradient columns the deferred weight-gradient pass holds at once
_ODE_DW_CAP = int(os.environ.get('STTODE_ODE_DW_CAP_MB', '256')) << 20      # bytes


def _ode_chunk_stages(nst, per_stage):
    """Stages per chunk of the deferred weight-gradient pass: as many as fit under _ODE_DW_CAP (at least one)."""
    return max(1, min(nst, _ODE_DW_CAP // per_stage))


def _ld(t):
    assert t.dim() == 2 and (t.stride(1) == 1 or t.shape[1] == 1), (t.shape, t.stride())
    return t.stride(0)


class Engine:
    """One training step: ``run_forward`` builds the tape and the loss values, ``run_backward`` returns name -> gradient."""

    def __init__(self, net):
        self.net = net
        self.dev = net.device
        self.scratch = torch.empty(4 << 20, dtype=torch.float32, device=self.dev)
        self.red_scratch = None     # split sums of a backward pass's deferred weight-gradient reductions (batch sizes; allocated on first use)
        self.param_grads = True     # False: skip the weight-gradient GEMMs (stage-2 sampler training keeps this net frozen)
        # scene batches: a trunk's forward + tape in one launch.  False -- layer by layer, the only form for T > 12 and D != 64 -- is otherwise
        # a test reference only (tests/test_gpu_parity.py::test_fused_trunk_forward_writes_the_layer_by_layer_tape sets it)
        self.fused_trunk = True
        # dimensions (train.py:37-40 --zdim / --hidden_dim / --num_decompose; 8 heads, ff 1024, conv 32 and GRU 96 are fixed in the reference:
        # model/STTODE.py:23-26,188-189): D model width, HD head width, ZD latent width, PFW = width of past_feature = cat(ftraj_input, ode),
        # ST = column of the GRU state in a decompose block's input cat(pf, z, state), IN = its width
        a = net.args
        self.D, self.ZD, self.NBLK = int(a.hidden_dim), int(a.zdim), int(a.num_decompose)
        self.HD, self.PFW = self.D // 8, 2 * self.D
        self.ST = self.PFW + self.ZD
        self.IN = self.ST + 96

    def begin(self):
        """Start a pass on the engine: the parameters by name as they are now, and the launches bound to the caller's stream."""
        self.P = dict(self.net.named_parameters())
        self._enter()

    def _enter(self):
        """Bind the launches to the caller's current stream (again inside a capture: torch.cuda.graph switches the stream)."""
        self.st = capi.stream_ptr()

    # ---------------------------------------------------------------- primitives
    def new(self, *shape):
        return torch.empty(*shape, dtype=torch.float32, device=self.dev)

    def zeros(self, *shape):
        return torch.zeros(*shape, dtype=torch.float32, device=self.dev)

    def lin(self, X, W, b, act=None, xdiv=1, out=None, cols=None):
        """out[c] = act(W X[c / xdiv] + b); X [rows, J] (row stride free), W [I, J] row-major view."""
        cols = X.shape[0] * xdiv if cols is None else cols
        I, J = W.shape
        assert X.shape[1] == J
        out = self.new(cols, I) if out is None else out
        capi.call('sttode_tlinear', X, _ld(X), xdiv, W, _ld(W), 0, b, None, 0, out, _ld(out), cols, J, I, ACT[act], 0, self.st)
        return out

    def lin_dx(self, dY, W, mask=None, out=None, accumulate=False, in_features=None):
        """dX = (dY W[:, :in_features]) (* (mask > 0));  W [N, K] is the forward weight."""
        cols, N = dY.shape
        K = W.shape[1] if in_features is None else in_features
        out = self.new(cols, K) if out is None else out
        capi.call('sttode_tlinear', dY, _ld(dY), 1, W, _ld(W), 1, None, mask, _ld(mask) if mask is not None else 0, out, _ld(out),
                  cols, N, K, 0, int(accumulate), self.st)
        return out

    def wgrad(self, dY, X, gW, gb, xdiv=1):
        if not self.param_grads:
            return
        cols, N = dY.shape
        K = X.shape[1]
        assert gW.shape[0] == N and gW.shape[1] == K, (gW.shape, N, K)
        capi.call('sttode_twgrad', dY, _ld(dY), X, _ld(X), xdiv, gW, _ld(gW), gb, cols, N, K, self.scratch, self.scratch.numel(), self.st)

    def lin_bwd(self, dY, W, X, gW, gb, mask=None, out=None, accumulate=False, in_features=None):
        """One layer's backward: returns dX = (dY W[:, :in_features]) (* (mask > 0)) (+ out) and accumulates gW += dY^T X,
        gb += sum dY -- one launch at scene sizes (sttode_tlinear_bwd)."""
        if not self.param_grads:
            return self.lin_dx(dY, W, mask=mask, out=out, accumulate=accumulate, in_features=in_features)
        cols, N = dY.shape
        K = W.shape[1]
        Kdx = K if in_features is None else in_features
        out = self.new(cols, Kdx) if out is None else out
        assert X.shape[1] == K and gW.shape[0] == N and gW.shape[1] == K
        capi.call('sttode_tlinear_bwd', dY, _ld(dY), W, _ld(W), mask, _ld(mask) if mask is not None else 0, out, _ld(out), Kdx,
                  int(accumulate), X, _ld(X), 1, gW, _ld(gW), gb, cols, N, K, self.scratch, self.scratch.numel(), self.st)
        return out

    def ew(self, op, p0, p1=None, p2=None, p3=None, p4=None, i0=0, f0=0.0, count=None):
        capi.call('sttode_train_ewise', op, p0, p1, p2, p3, p4, p0.numel() if count is None else count, i0, float(f0), self.st)

    def grad(self, name):
        """Gradient buffer of a parameter: a view into one flat buffer that is zeroed once per step."""
        self.touched.add(name)
        return self.G[name]

    def _grad_views(self):
        # a FRESH flat buffer per backward (one memset): autograd may adopt the returned views as .grad, so they must not
        # alias the next step's buffer
        tot = sum(((v.numel() + 3) // 4) * 4 for v in self.P.values())           # 16-byte aligned sub-buffers
        self.Gflat = torch.zeros(tot, dtype=torch.float32, device=self.dev)
        self.G, off = {}, 0
        for k, v in self.P.items():
            self.G[k] = self.Gflat[off: off + v.numel()].view(v.shape)
            off += ((v.numel() + 3) // 4) * 4
        self.touched = set()

    # ---------------------------------------------------------------- encoder trunk (PastEncoder / FutureEncoder shared part)
    def trunk_fwd(self, pre, enc_in, last, feat, drop_mask):
        """enc_in [n,T,4] -> feat[:, :64] = ftraj_input, feat[:, 64:128] = ODE encoder output.  Returns the tape."""
        return self.trunk_fwd_multi([(pre, enc_in, last, feat, drop_mask)])[0]

    def _trunk_state(self, items, backward=False):
        """The walkers' per-trunk state, one dict per trunk.  Forward items: (pre, enc_in, last, feat, drop), with a fresh tape under 't';
        backward items: (tape, dfeat).  'w': the encoder layer's parameter names by role (_LAYER), 'L' / 'Nb': attention length and slots."""
        net, D = self.net, self.D
        L, Nb = (net.batch_size, net._N) if net._mode == 'nba' else (1, None)
        S = []
        for it in items:
            if backward:
                t, dfeat = it
                assert dfeat.stride(1) == 1 and dfeat.shape[1] >= 2 * D
                s = dict(t=t, pre=t['pre'], n=t['n'], T=t['T'], dfeat=dfeat, L=t['L'], Nb=t['Nb'], Ys=t.get('Ys'))
            else:
                pre, enc_in, last, feat, drop_mask = it
                n, T = enc_in.shape[0], enc_in.shape[1]
                s = dict(t={'n': n, 'T': T, 'pre': pre, 'feat': feat}, pre=pre, n=n, T=T, X0=enc_in.reshape(n * T, 4), last=last, feat=feat,
                         drop=drop_mask, L=L, Nb=Nb if Nb is not None else n)
            s['w'] = {k: s['pre'] + name for k, name in _LAYER.items()}
            S.append(s)
        return S

    def trunk_fwd_multi(self, items):
        """Forward of one or several trunks (past and future encoder: the same layers, separate weights, independent of each other).  Scene
        batches with T <= 12: each trunk is ONE launch (csrc/train_trunk.hip), two of them inside a group one launch together.  Otherwise
        (NBA: attention over the batch) layer by layer, layer i of every trunk inside one group -- one launch at scene sizes."""
        prog = self.ode_program()
        if prog is not None:                                     # a non-default integrator: the stage program (_ode_trunk_fwd)
            return self._ode_trunk_fwd(items, *prog)
        net, D = self.net, self.D
        S = self._trunk_state(items)
        L = S[0]['L']
        pair = lambda: self.group() if len(S) > 1 else contextlib.nullcontext()
        if all(s['T'] <= 12 for s in S) and self.fused_trunk and D == 64:
            if L == 1:
                with pair():
                    return [self._trunk_fwd_fused(s) for s in S]
            # attention over the forward-call batch (the NBA branch): each trunk as TWO launches -- up to the in-projection, then (the attention
            # kernel between) from the attention output on -- instead of twelve layer launches; both trunks of a phase in one launch
            with pair():
                tabs = [self._trunk_fwd_fused(s, phase=1) for s in S]
            for s, (t, src) in zip(S, tabs):
                capi.self_attn_groups(src['qkv'], src['attn'], getattr(net, '_G', 1), L, s['Nb'], D, self.st)
            with pair():
                for s, (t, src) in zip(S, tabs):
                    self._trunk_launch(src, s['n'], s['T'], s['feat'], 2)
            for s, (t, src) in zip(S, tabs):
                t.update(L=L, Nb=s['Nb'], attn=src['attn'])
            return [t for t, _ in tabs]
        self._trunk_pre_layers(S)
        ks, A = self._layer_fwd(S, [s['x'] for s in S], full_qkv=True)
        with self.group():
            for s, a, k in zip(S, A, ks):
                s['ode'] = self.new(s['n'], D)
                self.ew(EW_EULER_FWD, s['ode'], a['xc'], k, f0=net.ODE_TIME)
        out = []
        for s, a in zip(S, A):
            s['feat'][:, D:2 * D] = s['ode']
            t = s['t']
            t.update(X0=s['X0'], posin=s['posin'], tp=s['tp'], drop=s['drop'], h3in=s['h3in'], ode=s['ode'], L=L, Nb=s['Nb'],
                     **{k: a[k] for k in ('xc', 'qkv', 'attn', 'ao', 'tt', 'ss', 'h', 'xh1', 'rs1', 'f1', 'xh2', 'rs2')})
            out.append(t)
        return out

    def _layer_fwd(self, S, Y, keep=None, full_qkv=False):
        """k = f(Y) per trunk: the ODE block's TransformerEncoderLayer (in-projection, geodesic attention -- the value rows alone at attention
        length 1 --, out_proj, tanh * sigmoid gate, add + LN1, FFN, add + LN2).  Layer i of every trunk in one group.  Y [n, D] per trunk,
        row stride free: the in-projection reads it where it is, add + LN1 a contiguous copy ('xc'; Y itself when it is contiguous).
        ``keep``: per trunk, buffers for the activations the weight gradients read (qkv, attn, ao, h, f1).  ``full_qkv``: at attention length
        1 the whole in-projection, not just the value rows the layer reads (the default path's tape carries qkv).  Returns (k per trunk,
        activations per trunk)."""
        P, D, net = self.P, self.D, self.net
        A = [dict(keep[i]) if keep is not None else {} for i in range(len(S))]
        with self.group():
            for s, y, a in zip(S, Y, A):
                W, b = P[s['w']['inproj_w']], P[s['w']['inproj_b']]
                if s['L'] > 1 or full_qkv:
                    a['qkv'] = self.lin(y, W, b, out=a.get('qkv'))
                else:
                    a['attn'] = self.lin(y, W[2 * D:], b[2 * D:], out=a.get('attn'))
        for s, a in zip(S, A):
            if s['L'] > 1:
                a['attn'] = a['attn'] if 'attn' in a else self.new(s['n'], D)
                # (the forward-call batches of a call, set_data_nba with [G,B,N,...]: attention within each)
                capi.self_attn_groups(a['qkv'], a['attn'], getattr(net, '_G', 1), s['L'], s['Nb'], D, self.st)
            elif full_qkv:
                a['attn'] = a['qkv'][:, 2 * D:]                  # softmax over a single key == 1  =>  output == v
        with self.group():
            for s, a in zip(S, A):
                a['ao'] = self.lin(a['attn'], P[s['w']['out_w']], P[s['w']['out_b']], out=a.get('ao'))
        with self.group():                                       # temporal_info and temporal_gate read the same input: four layers, one launch
            for s, a in zip(S, A):
                a['tt'] = self.lin(a['ao'], P[s['w']['info_w']], P[s['w']['info_b']], act='tanh')
                a['ss'] = self.lin(a['ao'], P[s['w']['gate_w']], P[s['w']['gate_b']], act='sigmoid')
        with self.group():
            for s, a in zip(S, A):
                a['gated'] = self.new(s['n'], D)
                self.ew(EW_MUL, a['gated'], a['tt'], a['ss'])
        for s, y, a in zip(S, Y, A):
            n = s['n']
            a['xc'] = y.contiguous()
            a['h'] = a['h'] if 'h' in a else self.new(n, D)
            a['xh1'], a['rs1'] = self.new(n, D), self.new(n)
            capi.call('sttode_add_ln_fwd', a['xc'], a['gated'], P[s['w']['ln1_w']], P[s['w']['ln1_b']], a['h'], a['xh1'], a['rs1'], n, D, self.st)
        with self.group():
            for s, a in zip(S, A):
                a['f1'] = self.lin(a['h'], P[s['w']['l1_w']], P[s['w']['l1_b']], act='relu', out=a.get('f1'))
        with self.group():
            for s, a in zip(S, A):
                a['f2'] = self.lin(a['f1'], P[s['w']['l2_w']], P[s['w']['l2_b']])
        ks = []
        for s, a in zip(S, A):
            n = s['n']
            k, a['xh2'], a['rs2'] = self.new(n, D), self.new(n, D), self.new(n)
            capi.call('sttode_add_ln_fwd', a['h'], a['f2'], P[s['w']['ln2_w']], P[s['w']['ln2_b']], k, a['xh2'], a['rs2'], n, D, self.st)
            ks.append(k)
        return tuple(ks), A

    def _trunk_pre_layers(self, S):
        """Layer by layer up to the ODE block's input (input_fc .. input_fc3, add_category): s['x'] = feat[:, :D] = ftraj_input."""
        P, net, D = self.P, self.net, self.D
        with self.group():
            for s in S:
                s['posin'] = self.new(s['n'] * s['T'], 2 * D)
                self.lin(s['X0'], P[s['pre'] + 'input_fc.weight'], P[s['pre'] + 'input_fc.bias'], out=s['posin'][:, :D])
        for s in S:
            pe = getattr(net, s['pre'][:-1]).pos_encoder.pe
            capi.call('sttode_rows_copy', s['posin'][:, D:], 2 * D, pe, D, s['n'] * s['T'], D, 1, s['T'], self.st)
        with self.group():
            for s in S:
                s['tp'] = self.lin(s['posin'], P[s['pre'] + 'pos_encoder.fc.weight'], P[s['pre'] + 'pos_encoder.fc.bias'])
        with self.group():
            for s in S:
                if s['drop'] is not None:                        # nn.Dropout(0.1) of PositionalAgentEncoding (model/STTODE.py:140,176)
                    self.ew(EW_MUL, s['tp'], s['tp'], s['drop'])
        for s in S:
            s['h3in'] = self.zeros(s['n'], D + 4)
            s['h3in'][:, D + 2] = s['last'].to(torch.float32)   # add_category: [0, 0, 1] for the last agent (model/STTODE.py:199-210)
        with self.group():
            for s in S:
                self.lin(s['tp'].view(s['n'], s['T'] * D), P[s['pre'] + 'input_fc2.weight'], P[s['pre'] + 'input_fc2.bias'], out=s['h3in'][:, :D])
        with self.group():
            for s in S:
                s['x'] = s['feat'][:, :D]
                self.lin(s['h3in'][:, :D + 3], P[s['pre'] + 'input_fc3.weight'], P[s['pre'] + 'input_fc3.bias'], out=s['x'])

    def _trunk_launch(self, src, n, T, feat, phase):
        tbl = (ctypes.c_void_p * len(capi.TRUNK_PTRS))(*[(src[k].data_ptr() if src.get(k) is not None else None) for k in capi.TRUNK_PTRS])
        capi.call('sttode_ttrunk_fwd', tbl, len(capi.TRUNK_PTRS), n, T, feat.stride(0), float(self.net.ODE_TIME), phase, self.st)

    def _trunk_fwd_fused(self, s, phase=0, launch=True):
        """The same forward and the same tape in ONE launch (csrc/train_trunk.hip, attention length 1): the step is bound by the number of
        launches, and a trunk is 21 of them layer by layer.  ``phase=1``: only up to the in-projection (attention over the forward-call batch:
        the caller runs the attention and then phase 2 through _trunk_launch); returns (tape, pointer sources) then."""
        P, net = self.P, self.net
        t, X0, feat, drop_mask = s['t'], s['X0'], s['feat'], s['drop']
        pre, n, T = t['pre'], t['n'], t['T']
        out = dict(posin=self.new(n * T, 128), tp=self.new(n * T, 64), h3in=self.new(n, 68), xc=self.new(n, 64), qkv=self.new(n, 192),
                   ao=self.new(n, 64), tt=self.new(n, 64), ss=self.new(n, 64), h=self.new(n, 64), xh1=self.new(n, 64), rs1=self.new(n),
                   f1=self.new(n, 1024), xh2=self.new(n, 64), rs2=self.new(n), ode=self.new(n, 64))
        src = dict({k: P[pre + name] for k, name in _FRONT.items()}, **{k: P[name] for k, name in s['w'].items()},
                   enc_in=X0, last=s['last'], pe=getattr(net, pre[:-1]).pos_encoder.pe, drop=drop_mask, feat=feat, **out)
        for k, v in src.items():
            assert v is None or v.is_contiguous() or k == 'feat', k
        if phase == 1:
            src['attn'] = self.new(n, 64)
        if launch:                                               # (launch=False: the caller launches the table itself, _ode_trunk_fwd)
            self._trunk_launch(src, n, T, feat, phase)
        t.update(X0=X0, drop=drop_mask, attn=out['qkv'][:, 128:], L=1, Nb=n, **out)
        return (t, src) if phase == 1 else t

    @contextlib.contextmanager
    def group(self):
        """Independent layers issued inside leave as ONE launch (sttode_tgemm_group: up to four per launch, scene sizes and batch sizes).
        What is issued inside is QUEUED with raw pointers and launched when the group closes (or its queue is full): every tensor handed to
        a call inside must stay referenced until then, or the allocator may give its memory to the next tensor allocated inside the group
        (tests/test_generic_training_gpu.py::test_operands_of_grouped_launches_outlive_their_group)."""
        capi.call('sttode_tgemm_group', 1)
        try:
            yield
        except BaseException:
            capi.call('sttode_tgemm_group', -1)
            raise
        capi.call('sttode_tgemm_group', 0)

    def trunk_bwd(self, t, dfeat):
        """dfeat [n,128] (row stride free) = grad wrt cat(ftraj_input, ode_out).  Accumulates parameter grads."""
        self.trunk_bwd_multi([(t, dfeat)])

    def trunk_bwd_multi(self, items):
        """Backward of one or several trunks (the past and the future encoder: the same layers, separate weights, independent of each
        other) walked through TOGETHER: layer i of every trunk is issued inside one group, i.e. one launch -- a one-scene step is bound by
        the number of launches, and the two trunks are 2 x 10 linear-layer backward launches otherwise."""
        if items[0][0].get('ode_prog') is not None:
            return self._ode_trunk_bwd(items)
        D = self.D
        S = self._trunk_state(items, backward=True)
        with self.group():
            for s in S:                                          # dx = dfeat[:, :64] + d, dy = T d, d = dfeat[:, 64:128] * (ode > 0): one piece,
                n = s['n']                                       # reading the strided rows of dfeat (no .contiguous() copies)
                assert s['dfeat'].stride(0) < 65536
                s['dx'], s['dy'] = self.new(n, D), self.new(n, D)
                self.ew(EW_EULER_BWD_CAT, s['dfeat'], s['t']['ode'], None, s['dx'], s['dy'], i0=s['dfeat'].stride(0) | ((D << 16) if D != 64 else 0),
                        f0=self.net.ODE_TIME, count=n * D)
        self._layer_vjp(S, [s['t'] for s in S], [s['dy'] for s in S], into=[s['dx'] for s in S])
        self._trunk_bwd_pre(S)                                   # s['dx'] is now the gradient wrt ftraj_input

    def _layer_vjp(self, S, A, dk, into=None, keep=None):
        """Gradient wrt the layer's input Y of every trunk, given the gradient dk of k = f(Y) and f's activations A (_layer_fwd's, or a tape
        of the default path): LN2, linear2^T, the relu mask, linear1^T, LN1, the gate, temporal_info / temporal_gate^T, out_proj^T, the
        attention and in_proj^T.  The LayerNorm parameter gradients accumulate here.  ``keep`` None: every linear layer's backward is ONE
        launch with its weight gradient (lin_bwd), and the residual dh = dsum2 + W1^T df1 accumulates in place.  ``keep`` given (per
        trunk, the chunk's column buffers): input gradients alone (lin_dx), every linear layer's output gradient written into ``keep`` for
        the deferred weight-gradient pass (_ode_wgrad) -- dsum2 among them, so the residual is a piece of its own.  ``into``: per trunk, a
        buffer the input gradient is ADDED to (the LN1 residual inside the gate's group, then the in-projection's part); None: new buffers.
        Returns the input gradient per trunk."""
        P, g, D = self.P, self.grad, self.D
        assert into is None or keep is None                      # the default path passes ``into``, the stage program ``keep``: never both
        K = keep if keep is not None else [{} for _ in S]

        def back(s, dY, role, X, rows=None, **kw):
            wn, bn = s['w'][role + '_w'], s['w'][role + '_b']
            if keep is not None:
                return self.lin_dx(dY, P[wn] if rows is None else P[wn][rows], **kw)
            if rows is None:
                return self.lin_bwd(dY, P[wn], X, g(wn), g(bn), **kw)
            return self.lin_bwd(dY, P[wn][rows], X, g(wn)[rows], g(bn)[rows], **kw)

        def ln_bwd(s, a, dY, x, rs, role, out):
            capi.call('sttode_ln_bwd', dY, a[x], a[rs], P[s['w'][role + '_w']], out, g(s['w'][role + '_w']), g(s['w'][role + '_b']), s['n'], D,
                      self.scratch, self.scratch.numel(), self.st)
            return out
        for s, a, d, k in zip(S, A, dk, K):
            if keep is None:
                k['dsum2'] = self.new(s['n'], D)
            ln_bwd(s, a, d, 'xh2', 'rs2', 'ln2', k['dsum2'])
        with self.group():
            for s, a, k in zip(S, A, K):
                k['df1'] = back(s, k['dsum2'], 'l2', a['f1'], mask=a['f1'], out=k.get('df1'))
        with self.group():                                       # dh = dsum2 (residual branch of LN2(h + f)) + W1^T df1
            if keep is None:
                dh = [back(s, k['df1'], 'l1', a['h'], out=k['dsum2'], accumulate=True) for s, a, k in zip(S, A, K)]
            else:
                dh = [back(s, k['df1'], 'l1', a['h']) for s, a, k in zip(S, A, K)]
        if keep is not None:                                     # (dsum2 stays as it is for _ode_wgrad)
            with self.group():
                for h, k in zip(dh, K):
                    self.ew(EW_AXPY, h, k['dsum2'], f0=1.0)
        d1 = [ln_bwd(s, a, h, 'xh1', 'rs1', 'ln1', self.new(s['n'], D)) for s, a, h in zip(S, A, dh)]
        dY = d1 if into is None else into                     # (None: the residual branch of LN1(Y + gated) is the buffer itself)
        with self.group():
            for s, a, k, d, dy in zip(S, A, K, d1, dY):
                if into is not None:
                    self.ew(EW_AXPY, dy, d, f0=1.0)              # residual branch of LN1(x + gated)
                if keep is None:
                    k['du'], k['dv'] = self.new(s['n'], D), self.new(s['n'], D)
                self.ew(EW_GATE_BWD, d, a['tt'], a['ss'], k['du'], k['dv'])
        with self.group():
            for s, a, k in zip(S, A, K):
                k['dao'] = back(s, k['du'], 'info', a['ao'], out=k.get('dao'))
        with self.group():
            for s, a, k in zip(S, A, K):
                back(s, k['dv'], 'gate', a['ao'], out=k['dao'], accumulate=True)
        with self.group():
            for s, a, k in zip(S, A, K):
                k['dattn'] = back(s, k['dao'], 'out', a['attn'], out=k.get('dattn'))
        for s, a, k in zip(S, A, K):
            if s['L'] > 1:
                if keep is None:
                    k['dqkv'] = self.new(s['n'], 3 * D)
                capi.call('sttode_mhgsa_attn_bwd', a['qkv'], k['dattn'], k['dqkv'], s['L'], s['Nb'], self.HD, self.st)
        with self.group():
            for s, a, k, dy in zip(S, A, K, dY):
                if s['L'] > 1:
                    back(s, k['dqkv'], 'inproj', a['xc'], out=dy, accumulate=True)
                else:
                    # attention length 1 (scene batches): the softmax over one key is 1, the output is v -- dv = dattn, and the gradients of
                    # q and k are exactly zero (their rows of the in-projection's gradient stay the zeros of the flat buffer)
                    back(s, k['dattn'], 'inproj', a['xc'], rows=slice(2 * D, None), out=dy, accumulate=True)
        return tuple(dY)

    def _trunk_bwd_pre(self, S):
        """Backward of the layers in front of the ODE block (input_fc3 .. input_fc), s['dx'] = gradient wrt ftraj_input."""
        P, g, D = self.P, self.grad, self.D
        with self.group():
            for s in S:
                t, pre = s['t'], s['pre']
                s['dh2'] = self.lin_bwd(s['dx'], P[pre + 'input_fc3.weight'], t['h3in'][:, :D + 3], g(pre + 'input_fc3.weight'), g(pre + 'input_fc3.bias'),
                                        in_features=D)
        with self.group():
            for s in S:
                t, pre, n, T = s['t'], s['pre'], s['n'], s['T']
                s['dtp'] = self.lin_bwd(s['dh2'], P[pre + 'input_fc2.weight'], t['tp'].view(n, T * D), g(pre + 'input_fc2.weight'),
                                        g(pre + 'input_fc2.bias')).view(n * T, D)
        with self.group():
            for s in S:
                if s['t']['drop'] is not None:
                    self.ew(EW_MUL, s['dtp'], s['dtp'], s['t']['drop'])
        with self.group():
            for s in S:
                t, pre = s['t'], s['pre']
                s['dtf'] = self.lin_bwd(s['dtp'], P[pre + 'pos_encoder.fc.weight'], t['posin'], g(pre + 'pos_encoder.fc.weight'),
                                        g(pre + 'pos_encoder.fc.bias'), in_features=D)
        with self.group():
            for s in S:
                self.wgrad(s['dtf'], s['t']['X0'], g(s['pre'] + 'input_fc.weight'), g(s['pre'] + 'input_fc.bias'))

    # ---------------------------------------------------------------- encoder trunk through a non-default integrator
    def ode_program(self):
        """(method, steps) of the model's encoder integrator when it is not the default one Euler step, else None (the default trunk path)."""
        net = self.net
        method, steps = getattr(net, 'ode_method', 'euler'), int(getattr(net, 'ode_steps', 1))
        if (method, steps) == ('euler', 1):
            return None
        if getattr(net, '_generic', False) or self.D != 64:
            raise NotImplementedError('non-default integrators are built for the reference widths (hidden_dim 64, zdim 32, two blocks)')
        odestages.stages(method)
        if steps < 1:
            raise ValueError(f'ode_steps must be positive, got {steps}')
        return method, steps

    def _ode_comb(self, S, terms, dst, mask=None):
        """One sttode_ode_combine launch over the trunks: per trunk sum of coef * value[trunk] for (coef, value) in terms.  dst: stage
        index j (written into the trunk's tape of stage inputs), 'final' (y_T, and relu(y_T) into feat[:, D:2 D]) or None (new buffer)."""
        D = self.D
        jobs = (_OdeCombine * len(S))()
        outs = []
        for si, s in enumerate(S):
            n, j = s['n'], jobs[si]
            if dst is None:
                out = self.new(n, D)
            elif dst == 'final':
                out, relu = s['yT'], s['feat'][:, D:2 * D]
                j.relu_out, j.ld_relu = relu.data_ptr(), _ld(relu)
            else:
                out = s['Ys'][dst * n:(dst + 1) * n]
            for ti, (c, v) in enumerate(terms):
                j.v[ti], j.ld[ti], j.c[ti] = v[si].data_ptr(), _ld(v[si]), c
            if mask is not None:
                j.mask, j.ld_mask = mask[si].data_ptr(), _ld(mask[si])
            j.out, j.ld_out, j.nterms, j.rows = out.data_ptr(), _ld(out), len(terms), n
            outs.append(out)
        capi.call('sttode_ode_combine', jobs, len(S), D, self.st)
        return tuple(outs)

    def _ode_wgrad(self, S, K, c0, c1):
        """The deferred weight-gradient pass of stages c0 .. c1-1: ONE product per layer over all of their columns (stage j's rows of
        every buffer at (j - c0) n .. (j - c0 + 1) n; the in-projection reads the stage inputs where the tape keeps them)."""
        P, g, D = self.P, self.grad, self.D
        rows = [(c1 - c0) * s['n'] for s in S]
        for dy, x, role in (('dsum2', 'f1', 'l2'), ('df1', 'h', 'l1'), ('du', 'ao', 'info'), ('dv', 'ao', 'gate'), ('dao', 'attn', 'out')):
            with self.group():
                for s, k, m in zip(S, K, rows):
                    self.wgrad(k[dy][:m], k[x][:m], g(s['w'][role + '_w']), g(s['w'][role + '_b']))
        for s, k, m in zip(S, K, rows):
            if 'ln' in k:                                       # (the fused dX chain) LayerNorm parameter gradients: column sums of its rows
                for off, role in ((0, 'ln2_w'), (D, 'ln2_b'), (2 * D, 'ln1_w'), (3 * D, 'ln1_b')):
                    capi.call('sttode_rows_reduce', g(s['w'][role]), D, k['ln'][:, off:], 4 * D, 1, D, m, 1, self.st)
        with self.group():
            for s, k, m in zip(S, K, rows):
                Y = s['Ys'][c0 * s['n']:c1 * s['n']]
                gW, gb = g(s['w']['inproj_w']), g(s['w']['inproj_b'])
                if s['L'] > 1:
                    self.wgrad(k['dqkv'][:m], Y, gW, gb)
                else:
                    self.wgrad(k['dattn'][:m], Y, gW[2 * D:], gb[2 * D:])

    def _ode_trunk_fwd(self, items, method, steps):
        """Forward of the trunks through ``steps`` steps of ``method`` (odestages.integrate).  Attention length 1 with T <= 12 (scene
        batches): ONE launch for both trunks whatever the step count (sttode_ttrunk_ode_fwd: the layers in front of the ODE block, then
        the stage loop inside the kernel).  Otherwise the layers in front as in the default path (the fused phase-1 launch when T <= 12),
        then the stage program with f layer by layer, both trunks' layer i in one group.  Tape: the layers in front, and the stage inputs
        Y_j alone ([stages * n, 64] per trunk); the backward pass recomputes f's activations from them."""
        net, D = self.net, self.D
        S = self._trunk_state(items)
        L = S[0]['L']
        nst = steps * odestages.stages(method)
        for s in S:
            s['Ys'], s['yT'] = self.new(nst * s['n'], D), self.new(s['n'], D)
        fused = all(s['T'] <= 12 for s in S) and self.fused_trunk
        if fused and L == 1:
            tabs = [self._trunk_fwd_fused(s, phase=1, launch=False) for s in S]
            ptrs = [(src[k].data_ptr() if src.get(k) is not None else None) for _, src in tabs for k in capi.TRUNK_PTRS]
            A, B = odestages.TABLEAU[method]
            prog = _OdeProgram(stages=len(B), steps=steps, h=float(net.ODE_TIME) / steps)
            for i, row in enumerate(A):
                for j, c in enumerate(row):
                    prog.a[4 * i + j] = c
            for i, c in enumerate(B):
                prog.b[i] = c
            m = len(S)
            capi.call('sttode_ttrunk_ode_fwd', (ctypes.c_void_p * len(ptrs))(*ptrs), len(ptrs), m, (ctypes.c_int * m)(*[s['n'] for s in S]),
                      (ctypes.c_int * m)(*[s['T'] for s in S]), (ctypes.c_long * m)(*[s['feat'].stride(0) for s in S]),
                      (ctypes.c_void_p * m)(*[s['Ys'].data_ptr() for s in S]), (ctypes.c_void_p * m)(*[s['yT'].data_ptr() for s in S]),
                      ctypes.byref(prog), self.st)
        else:
            if fused:                                            # phase 1 of the fused trunk launch, both trunks in one launch
                with (self.group() if len(S) > 1 else contextlib.nullcontext()):
                    tabs = [self._trunk_fwd_fused(s, phase=1) for s in S]
                for s in S:
                    s['y0'] = s['t']['xc']
            else:
                self._trunk_pre_layers(S)
                for s in S:
                    s['y0'] = s['x']
                    s['t'].update(X0=s['X0'], posin=s['posin'], tp=s['tp'], drop=s['drop'], h3in=s['h3in'])
            odestages.integrate(lambda j, Y: self._layer_fwd(S, Y)[0], lambda terms, dst: self._ode_comb(S, terms, dst),
                                tuple(s['y0'] for s in S), net.ODE_TIME, method, steps)
        for s in S:
            s['t'].update(ode_prog=(method, steps), ode_fused=fused and L == 1, Ys=s['Ys'], yT=s['yT'], L=L, Nb=s['Nb'])
        return [s['t'] for s in S]

    def _ode_stage_bwd(self, S, j, kb, close, keep, dY):
        """One sttode_ode_stage_bwd launch for stage j of both trunks: f recomputed, dk from ``kb``, f's VJP into dY, the columns into
        ``keep``; with ``close`` also the gradient wrt the step's start state (returned, per trunk)."""
        P, D = self.P, self.D
        jobs = (_OdeStageBwd * len(S))()
        closed = []
        for si, s in enumerate(S):
            J, n = jobs[si], s['n']
            for wi, name in enumerate(s['w'].values()):         # (the order of _LAYER is the order of w[])
                J.w[wi] = P[name].data_ptr()
            J.y, J.dy, J.n = s['Ys'][j * n:(j + 1) * n].data_ptr(), dY[si].data_ptr(), n
            for ti, (c, v) in enumerate(kb):
                J.kb.v[ti], J.kb.ld[ti], J.kb.c[ti] = v[si].data_ptr(), _ld(v[si]), c
            J.kb.nterms, J.kb.rows = len(kb), n
            if close is not None:
                out = self.new(n, D)
                for ti, (c, v) in enumerate(close):
                    J.next.v[ti], J.next.ld[ti], J.next.c[ti] = v[si].data_ptr(), _ld(v[si]), c
                J.next.nterms, J.next.rows, J.next.out, J.next.ld_out = len(close), n, out.data_ptr(), D
                closed.append(out)
            for k, v in keep[si].items():
                setattr(J, k, v.data_ptr())
        capi.call('sttode_ode_stage_bwd', jobs, len(S), self.st)
        return tuple(closed) if close is not None else None

    def _ode_trunk_bwd(self, items):
        """Backward of _ode_trunk_fwd (odestages.integrate_adjoint): stages in reverse, each one f recomputed from its stage input, its
        VJP, and the stage-combination adjoints -- ONE sttode_ode_stage_bwd launch per stage for both trunks at attention length 1, the
        layer kernels and sttode_ode_combine otherwise; the linear layers' weight gradients in chunks of stages (_ode_wgrad) whose columns
        stay under _ODE_DW_CAP bytes.  Then the layers in front of the ODE block as in the default path."""
        D = self.D
        method, steps = items[0][0]['ode_prog']
        fused = items[0][0]['ode_fused']
        assert all(t['ode_prog'] == (method, steps) and t['ode_fused'] == fused for t, _ in items)
        S = self._trunk_state(items, backward=True)
        acts = ('attn', 'ao', 'h', 'f1')
        width = dict(attn=D, ao=D, h=D, f1=1024, dsum2=D, df1=1024, du=D, dv=D, dao=D, dattn=D, qkv=3 * D, dqkv=3 * D, ln=4 * D)
        names = [acts + ('dsum2', 'df1', 'du', 'dv', 'dao', 'dattn') + (('ln',) if fused else ()) + (('qkv', 'dqkv') if s['L'] > 1 else ())
                 for s in S]
        per_stage = sum(4 * s['n'] * sum(width[k] for k in nm) for s, nm in zip(S, names))
        nst = steps * odestages.stages(method)
        C = _ode_chunk_stages(nst, per_stage)
        K = []

        def vjp(j, kb, close):
            c1 = nst - ((nst - 1 - j) // C) * C
            c0 = max(0, c1 - C)
            if j == c1 - 1:                                     # the chunk's first (highest) stage: its column buffers
                K[:] = [{k: torch.empty((c1 - c0) * s['n'], width[k], dtype=torch.float32, device=self.dev) for k in nm} for s, nm in zip(S, names)]
            keep = [{k: v[(j - c0) * s['n']:(j - c0 + 1) * s['n']] for k, v in kk.items()} for s, kk in zip(S, K)]
            if fused:
                dY = tuple(self.new(s['n'], D) for s in S)
                closed = self._ode_stage_bwd(S, j, kb, close, keep, dY)
            else:
                Y = tuple(s['Ys'][j * s['n']:(j + 1) * s['n']] for s in S)
                _, A = self._layer_fwd(S, Y, keep=[{k: kp[k] for k in kp if k in acts or k == 'qkv'} for kp in keep])
                dY = self._layer_vjp(S, A, self._ode_comb(S, kb, None), keep=keep)
                closed = None if close is None else self._ode_comb(S, [(1.0, dY)] + close, None)
            if j == c0:
                self._ode_wgrad(S, K, c0, c1)
            return dY, closed

        ybar = self._ode_comb(S, [(1.0, tuple(s['dfeat'][:, D:2 * D] for s in S))], None, mask=tuple(s['t']['yT'] for s in S))
        dx = odestages.integrate_adjoint(vjp, ybar, self.net.ODE_TIME, method, steps, extra=[(1.0, tuple(s['dfeat'][:, :D] for s in S))])
        for s, d in zip(S, dx):
            s['dx'] = d
        self._trunk_bwd_pre(S)

    # ---------------------------------------------------------------- decoder (Decoder.forward, model/STTODE.py:320-347)
    def mlp_fwd(self, pres, inp):
        """The three-layer MLPs ``pres`` over the same input (decoder_y alone, or decoder_y and decoder_x of a block: separate weights,
        model/STTODE.py:71-77) layer by layer: at batch sizes the two products of a layer leave as one launch (sttode_tgemm_group); one
        MLP's stay outside any group.  Returns (output, (a1, a2)) per MLP."""
        P = self.P
        xs, acts = [inp] * len(pres), []
        for li, act in ((0, 'relu'), (1, 'relu'), (2, None)):
            with (self.group() if len(pres) > 1 else contextlib.nullcontext()):
                xs = [self.lin(x, P[f'{pre}layers.{li}.weight'], P[f'{pre}layers.{li}.bias'], act=act) for pre, x in zip(pres, xs)]
            acts.append(xs)
        return [(a3, (a1, a2)) for a1, a2, a3 in zip(*acts)]

    def mlp_bwd(self, pres, inp, saved, douts, din):
        """Backward of mlp_fwd: layers 2 and 1 of the MLPs side by side (four products per launch at batch sizes); their layer-0 input
        gradients add into the same ``din``, so those stay launches of their own, in order."""
        P, g = self.P, self.grad
        ds = douts
        for li in (2, 1):
            with (self.group() if len(pres) > 1 else contextlib.nullcontext()):
                nxt = [self.lin_bwd(d, P[f'{pre}layers.{li}.weight'], sv[li - 1], g(f'{pre}layers.{li}.weight'), g(f'{pre}layers.{li}.bias'), mask=sv[li - 1])
                       for pre, sv, d in zip(pres, saved, ds)]
            ds = nxt                                                # (the layer's inputs keep their names until the group has left: see group())
        for i, (pre, d) in enumerate(zip(pres, ds)):
            self.lin_bwd(d, P[pre + 'layers.0.weight'], inp, g(pre + 'layers.0.weight'), g(pre + 'layers.0.bias'), out=din, accumulate=i > 0)

    def block_fwd(self, i, past, K, xhat_prev, pf, z, want_x, inp=None):
        P = self.P
        pre = f'decoder.decompose.{i}.'
        n, Tp = past.shape[0], past.shape[1]
        m = n * K
        # The first block reads x_true - 0: its conv + GRU see the same track for every sample of an agent (model/STTODE.py:329-335, x_hat = 0).
        # Run them ONCE per agent and hand the state to the agent's K columns (the inference path has done so since round 1) -- K = 21 in
        # forward(): a 21 x smaller input projection and GRU sequence; the backward sums the K columns' state gradients first (block_bwd).
        agent = xhat_prev is None and K > 1 and _AGENT_GRU
        mg, Kg = (n, 1) if agent else (m, K)
        x, e = self.new(mg, Tp, 2), self.new(mg * Tp, 32)
        capi.call('sttode_conv_fwd', past, Kg, xhat_prev, P[pre + 'conv_past.weight'], P[pre + 'conv_past.bias'], x, e, mg, Tp, self.st)
        gi = self.lin(e, P[pre + 'encoder_past.weight_ih_l0'], P[pre + 'encoder_past.bias_ih_l0'])       # [mg*Tp, 288], row c*Tp + t
        H = self.new(Tp + 1, mg, 96)                                                                     # H[0] = 0 (written by the launch), H[t+1] = h_t
        tapes = self.new(Tp, mg, 384)
        prefix = inp is None                                                                             # cat(pf_rep, z, state): the prefix may come filled (decoder_fwd)
        IN, ST, PFW, ZD = self.IN, self.ST, self.PFW, self.ZD
        if prefix:
            inp = self.new(m, IN)
        if agent:
            state = self.new(n, 96)
            capi.call('sttode_gru_seq_fwd', gi, P[pre + 'encoder_past.weight_hh_l0'], P[pre + 'encoder_past.bias_hh_l0'], H, tapes,
                      state, 96, n, Tp, self.st)
            capi.call('sttode_rows_copy', inp[:, ST:], IN, state, 96, m, 96, K, n, self.st)              # row c of inp <- state of agent c / K
        else:
            capi.call('sttode_gru_seq_fwd', gi, P[pre + 'encoder_past.weight_hh_l0'], P[pre + 'encoder_past.bias_hh_l0'], H, tapes,
                      inp[:, ST:], IN, m, Tp, self.st)                                                   # all Tp steps, one launch
        if prefix:
            capi.call('sttode_rows_copy', inp, IN, pf, _ld(pf), m, PFW, K, n, self.st)
            capi.call('sttode_rows_copy', inp[:, PFW:], IN, z, _ld(z), m, ZD, 1, m, self.st)
        if want_x:
            (yh, sy), (xh, sx) = self.mlp_fwd([pre + 'decoder_y.', pre + 'decoder_x.'], inp)
        else:
            (yh, sy), (xh, sx) = self.mlp_fwd([pre + 'decoder_y.'], inp)[0], (None, None)
        return dict(pre=pre, m=m, Tp=Tp, K=K, x=x, e=e, H=H, tapes=tapes, inp=inp, yh=yh, sy=sy, xh=xh, sx=sx, agent=agent)

    def block_bwd(self, b, dyh, dxh, need_dx):
        """Returns (din [m, IN], dx [m,Tp,2] | None)."""
        P, g = self.P, self.grad
        pre, m, Tp, K = b['pre'], b['m'], b['Tp'], b['K']
        IN, ST = self.IN, self.ST
        din = self.new(m, IN)
        if dxh is not None:
            self.mlp_bwd([pre + 'decoder_y.', pre + 'decoder_x.'], b['inp'], [b['sy'], b['sx']], [dyh, dxh], din)
        else:
            self.mlp_bwd([pre + 'decoder_y.'], b['inp'], [b['sy']], [dyh], din)
        dstate, lds, mg = din[:, ST:], IN, m
        if b.get('agent'):                                          # conv + GRU ran once per agent: its state gradient is the sum over the agent's columns
            assert not need_dx
            mg = m // K
            dstate, lds = self.new(mg, 96), 96
            capi.call('sttode_rows_reduce', dstate, 96, din[:, ST:], IN, mg, 96, K, 0, self.st)
        dgi = self.new(mg * Tp, 288)
        dgh = self.new(Tp, mg, 288)
        capi.call('sttode_gru_seq_bwd', dstate, lds, b['tapes'], b['H'], P[pre + 'encoder_past.weight_hh_l0'], dgi, dgh, mg, Tp, self.st)
        self.wgrad(dgh.view(Tp * mg, 288), b['H'][:Tp].view(Tp * mg, 96), g(pre + 'encoder_past.weight_hh_l0'), g(pre + 'encoder_past.bias_hh_l0'))
        de = self.lin_bwd(dgi, P[pre + 'encoder_past.weight_ih_l0'], b['e'], g(pre + 'encoder_past.weight_ih_l0'),
                          g(pre + 'encoder_past.bias_ih_l0'), mask=b['e'])
        dx = self.new(mg, Tp, 2) if need_dx else None
        capi.call('sttode_conv_bwd', de, b['x'], P[pre + 'conv_past.weight'], dx, g(pre + 'conv_past.weight'), g(pre + 'conv_past.bias'),
                  mg, Tp, self.scratch, self.scratch.numel(), self.st)
        return din, dx

    def decoder_fwd(self, pf, z, K, past, cur, want_recover, qz_eps=None):
        """Decoder.forward (model/STTODE.py:320-347) over ``num_decompose`` blocks: block i reads x_true - x_hat_{i-1} (x_hat_{-1} = 0) and the
        same cat(pf, z); prediction = sum y_hat_i + cur_location, reconstruction = sum x_hat_i (the last block's decoder_x is needed only for it).
        ``qz_eps`` = (qz [n, zd], eps [n (K - 1), zd]) instead of ``z`` [n K, zd]: the blocks' input prefix cat(pf, z) is written for the
        first TWO blocks by one launch (sttode_decoder_inputs; further blocks copy it) and z is never assembled."""
        n, Tp = past.shape[0], past.shape[1]
        Tf = self.net.args.future_length
        m = n * K
        nb = self.NBLK
        inps = [None] * nb
        if qz_eps is not None:
            inps = [self.new(m, self.IN) for _ in range(nb)]
            capi.call('sttode_decoder_inputs', inps[0], inps[1] if nb > 1 else None, self.IN, pf, _ld(pf), qz_eps[0], qz_eps[1], n, K, self.PFW, self.ZD, self.st)
            for i in range(2, nb):                                  # (further blocks: the same prefix)
                capi.call('sttode_rows_copy', inps[i], self.IN, inps[0], self.IN, m, self.ST, 1, m, self.st)
        blocks, xprev = [], None
        for i in range(nb):
            b = self.block_fwd(i, past, K, xprev, pf, z, want_recover or i + 1 < nb, inp=inps[i])
            blocks.append(b)
            xprev = b['xh']
        pred = self.new(m, 2 * Tf)
        rec = None
        ysum, xsum = blocks[0]['yh'], blocks[0]['xh']
        for b in blocks[1:-1]:                                      # (num_decompose > 2: partial sums of the middle blocks)
            t = self.new(m, 2 * Tf)
            self.ew(EW_SUM_CUR, t, ysum, b['yh'], None, i0=2 * Tf, f0=K)
            ysum = t
            if want_recover:
                t = self.new(m, 2 * Tp)
                self.ew(EW_SUM_CUR, t, xsum, b['xh'], None, i0=2 * Tp, f0=K)
                xsum = t
        # one block: the sums' second operands are zeros.  They are named HERE: a piece issued inside a group is only queued, so a temporary
        # handed to it would be freed before the launch leaves, and `rec`, allocated next, got its memory -- the prediction then read the
        # reconstruction being written by the same launch (seen on the first step of a process, when the allocator has nothing else to give)
        y1, x1 = (blocks[-1]['yh'], blocks[-1]['xh']) if nb > 1 else (self.zeros(m, 2 * Tf), self.zeros(m, 2 * Tp) if want_recover else None)
        with self.group():                                          # two independent pieces: one launch
            self.ew(EW_SUM_CUR, pred, ysum, y1, cur, i0=2 * Tf, f0=K)
            if want_recover:
                rec = self.new(m, 2 * Tp)
                self.ew(EW_SUM_CUR, rec, xsum, x1, None, i0=2 * Tp, f0=K)
        return dict(blocks=blocks, b0=blocks[0], b1=blocks[-1], n=n, K=K, m=m, pred=pred, rec=rec)

    def decoder_live(self, d, best):
        """The decoder's tape reduced to the columns that carry a gradient.  forward() decodes 1 + 20 samples per agent, but the objective
        (model/STTODE.py:553-568) touches sample 0 (mse + recover terms) and, through the min over K of loss_diverse (:390-395), ONE of
        the prior samples per agent; the decoder treats trajectory columns independently (conv, GRU and MLPs per column,
        model/STTODE.py:50-77), so the backward pass of the other 19 columns is exactly zero in every layer and contributes nothing to
        any parameter gradient.  The reference's autograd multiplies through those zeros; here the tape rows of the two live columns per
        agent are gathered (ONE launch, csrc/train_ewise.hip live_rows_gather_kernel) and the backward pass runs over 2 n columns instead of
        21 n -- the same gradient (the reference's own backward() digests: tests/test_gpu_parity.py::test_training_step_vs_reference_*)."""
        n, K1, m2 = d['n'], d['K'], 2 * d['n']
        items, blocks = [], []

        def take(src, row, outer=1):
            m = n * K1
            dst = self.new(outer * m2 * row)
            assert src.is_contiguous() and src.numel() == outer * m * row
            items.append(_GatherItem(src.data_ptr(), dst.data_ptr(), m * row, m2 * row, row, outer))
            return dst
        for b in d['blocks']:
            Tp = b['Tp']
            nb = dict(pre=b['pre'], m=m2, Tp=Tp, K=2, agent=b.get('agent', False))
            if nb['agent']:                                          # conv + GRU ran per agent: their tape has no column dimension
                nb.update(x=b['x'], e=b['e'], H=b['H'], tapes=b['tapes'])
            else:
                nb['x'] = take(b['x'], 2 * Tp).view(m2, Tp, 2)
                nb['e'] = take(b['e'], Tp * 32).view(m2 * Tp, 32)
                nb['H'] = take(b['H'], 96, Tp + 1).view(Tp + 1, m2, 96)
                nb['tapes'] = take(b['tapes'], 384, Tp).view(Tp, m2, 384)
            nb['inp'] = take(b['inp'], self.IN).view(m2, self.IN)
            for key in ('sy', 'sx'):
                nb[key] = tuple(take(t, t.shape[1]).view(m2, t.shape[1]) for t in b[key]) if b[key] is not None else None
            blocks.append(nb)
        for i in range(0, len(items), _GATHER_MAX):
            chunk = items[i:i + _GATHER_MAX]
            table = (_GatherItem * len(chunk))(*chunk)              # (a named object: it must outlive the call that reads it)
            capi.call('sttode_live_rows_gather', table, len(chunk), best, n, K1, self.st)
        return dict(blocks=blocks, b0=blocks[0], b1=blocks[-1], n=n, K=2, m=m2)

    def decoder_bwd(self, d, dpred, drec, dpf, dz, dpf_accumulate=True):
        """Accumulates dpf [n, 2 D] (+=; ``dpf_accumulate=False``: writes it); writes dz [m, zd] if not None.  Returns the gradient of the
        blocks' summed layer-1 input [m, IN] = cat(d pf_rep | d z | d state) (its columns 2 D .. 2 D + zd - 1 are dz)."""
        n, K, m = d['n'], d['K'], d['m']
        blocks = d['blocks']
        # x_{i+1} = x_true - x_hat_i  =>  d x_hat_i = (d recover) - d x_{i+1}; the last block's x_hat only feeds the reconstruction
        dxh, din_sum = drec, None
        for i in range(len(blocks) - 1, -1, -1):
            din, dx = self.block_bwd(blocks[i], dpred, dxh, i > 0)
            if din_sum is None:
                din_sum = din
            else:
                self.ew(EW_AXPY, din, din_sum, f0=1.0)              # (the running sum ends in block 0's buffer, as in rounds 3-4)
                din_sum = din
            if i > 0:
                dxh = dx.view(m, -1)
                self.ew(EW_SCALE_ADD, dxh, drec, f0=-1.0)           # d x_hat_{i-1} = -dx_i (+ drec)
        capi.call('sttode_rows_reduce', dpf, _ld(dpf), din_sum, self.IN, n, self.PFW, K, int(dpf_accumulate), self.st)
        if dz is not None:
            dz.copy_(din_sum[:, self.PFW:self.ST])
        return din_sum

    # ---------------------------------------------------------------- the objective (model/STTODE.py:553-568)
    def prepare_forward(self):
        """The host side of a forward pass, BEFORE a capture begins (_GraphedStep._capture): the parameters by name, and at batch sizes the
        room for a backward pass's deferred split sums -- the engine's own buffer, which must not come from a graph's private pool."""
        self.begin()
        net = self.net
        if net._past.shape[0] * _K1 * net.args.past_length > _TGEMM_MIN_COLS_BWD and self.red_scratch is None:
            self.red_scratch = torch.empty(_SCRATCH_BATCH, dtype=torch.float32, device=self.dev)

    def enqueue_forward(self, eps_q, eps20, drop_past=None, drop_future=None):
        """Enqueues the forward pass (after prepare_forward): the frontend, both trunks together, then the q-net and ONE decoder pass over
        1 + 20 samples per agent -- sample 0 decoded from the posterior draw (pred_traj / recover_traj, model/STTODE.py:553-560),
        samples 1..20 from the prior draws (diverse_pred_traj, :562-566): the two passes of the reference share every weight, so one
        pass over 21 columns per agent halves the launches of the decoder's forward and backward.  Returns the loss values [5]."""
        self._enter()
        net, a, P = self.net, self.net.args, self.P
        B = net.batch_size if net._mode == 'nba' else 1
        N = net.agent_num
        n, Tp, Tf, zd = net._past.shape[0], a.past_length, a.future_length, a.zdim
        mode = 0 if net._mode == 'scenes' else 1
        K1, PFW = _K1, self.PFW
        ws = net._frontend(vel_from_norm=0)
        past = ws['xpad'][:, :2 * Tp].reshape(n, Tp, 2).contiguous()
        fut = (net._future - ws['orig'][:, None, :]).contiguous()
        hcat = self.new(n, 2 * PFW)
        lastpos = net._past[:, -1].contiguous()
        enc_f = self.new(n, Tf, 4)
        capi.call('sttode_frontend_future', net._future, lastpos, n, Tf, mode, net._N or 1, ws.get('scene_orig'),
                  ws.get('agent_scene'), net._scene_ptr if mode == 0 else None, enc_f, self.st)
        tf, tp = self.trunk_fwd_multi([('future_encoder.', enc_f, ws['last'], hcat[:, PFW:], drop_future),    # both trunks together (grouped launches)
                                       ('past_encoder.', ws['enc_in'], ws['last'], hcat[:, :PFW], drop_past)])
        hq = self.lin(hcat, P['future_encoder.out_mlp.affine_layers.0.weight'], P['future_encoder.out_mlp.affine_layers.0.bias'], act='relu')
        qzp = self.lin(hq, P['future_encoder.qz_layer.weight'], P['future_encoder.qz_layer.bias'])
        qz = self.new(n, zd)
        self.ew(EW_RSAMPLE, qz, qzp, eps_q, i0=zd)
        # z per (agent, sample): sample 0 = the posterior draw, samples 1..20 = the prior draws -- read where they are by the launch that
        # fills both blocks' input prefix
        assert zd % 4 == 0 and eps20.is_contiguous() and qz.is_contiguous()
        d = self.decoder_fwd(hcat[:, :PFW], None, K1, past, ws['cur'], True, qz_eps=(qz, eps20))
        losses = self.new(5)                                    # the four terms and their sum
        live = _LIVE_COLUMNS
        KG = 2 if live else K1                                  # columns per agent that carry a gradient (see decoder_live)
        dpred, drec, dqzp = self.new(n * KG, 2 * Tf), self.new(n * KG, 2 * Tp), self.new(n, 2 * zd)
        best = torch.empty(n, dtype=torch.int32, device=self.dev) if live else None
        # several independent scenes in one step (set_scene_batch): the objective is the SUM of the per-scene objectives, i.e. the
        # gradient equals what S reference steps would accumulate (per-scene KL clamp and per-scene mean of the best-of-20 term)
        seg = net._mode == 'scenes' and net._S > 1
        sp, ags, S = (net._scene_ptr, ws['agent_scene'], net._S) if seg else (None, None, 0)
        # what the three objective entries share: the inputs, the sizes and scales, then the values and the gradients they write
        common = (d['pred'], d['rec'], fut, past, qzp, sp, ags, S, n, K1, 2 * Tf, 2 * Tp, zd, 1.0 / (B * Tf), 1.0 / (B * Tp), float(B * N),
                  float(a.min_clip), losses, dpred, drec, dqzp)
        tail = (self.scratch, self.scratch.numel(), self.st)
        if net._diverse_joint():
            # the scene-level best-of-K term: one prior sample per segment -- a scene of the CSR, the one scene, an NBA game --
            # so the gradient still lives in sample 0 plus one prior column per agent and `best` feeds decoder_live as it is
            if not live:
                raise SttodeError("diverse_mode 'joint' is built on the live-column backward pass (its kernel writes the two live gradient "
                                  "rows per agent); _LIVE_COLUMNS = False has no dense joint form")
            capi.call('sttode_loss_objective_joint', *common, best, 0 if seg else net._joint_seg_len(n), None, *tail)
        elif live:
            capi.call('sttode_loss_objective_live', *common, best, *tail)
        else:
            capi.call('sttode_loss_objective', *common, *tail)
        if getattr(self, 'publish', None) is not None:         # a step being captured: the values reach the host from HERE (see _GraphedStep)
            capi.call('sttode_publish_values', losses, 5, *self.publish, self.st)
        self.step_id = getattr(self, 'step_id', 0) + 1
        self.tape = dict(step_id=self.step_id, tp=tp, tf=tf, hcat=hcat, hq=hq, qzp=qzp, eps_q=eps_q, d=d, dpred=dpred,
                         drec=drec, dqzp=dqzp, n=n, zd=zd, K1=K1, best=best)
        # the forward pass's own buffers (a captured step keeps them: _GraphedStep.keep)
        self.V = dict(ws=ws, past=past, fut=fut, hcat=hcat, lastpos=lastpos, enc_f=enc_f, tf=tf, tp=tp, losses=losses)
        # attributes the reference sets (read by callers)
        pr = d['pred'].view(n, K1, Tf, 2)
        net.past_feature = hcat[:, :PFW]
        net.qz_param = qzp
        net.qz_sampled = qz
        net.pred_traj = pr[:, 0]
        net.recover_traj = d['rec'].view(n, K1, Tp, 2)[:, 0]
        net.diverse_pred_traj = pr[:, 1:]
        net.past_traj, net.future_traj, net.cur_location = past, fut, past[:, -1:]
        return losses

    def run_forward(self, eps_q, eps20, drop_past=None, drop_future=None):
        self.prepare_forward()
        return self.enqueue_forward(eps_q, eps20, drop_past, drop_future)

    def enqueue_backward(self):
        """Enqueues the backward pass of the most recent forward: the decoder and the q-net, then both trunks together (disjoint parameters).
        A failure on the way drops the weight-gradient reductions that were deferred so far."""
        try:
            self._enqueue_backward()
        except BaseException:
            capi.call('sttode_twgrad_defer', -1, None, 0)
            raise

    def _enqueue_backward(self):
        T = self.tape
        # The tape (and the flat gradient buffer it fills) belongs to the MOST RECENT eager forward().  backward() of an older loss, or
        # a second backward() of the same loss, would silently differentiate the wrong step: refuse instead.
        if T is None:
            raise SttodeError('training backward: the tape of this forward() was already consumed (backward() called twice, or '
                              'retain_graph reuse); run forward() again')
        self._enter()
        n, zd, K1 = T['n'], T['zd'], T['K1']
        P, g, PFW = self.P, self.grad, self.PFW
        self._grad_views()
        if self.red_scratch is not None:                            # batch sizes: the split weight gradients' reductions as one launch per 16
            capi.call('sttode_twgrad_defer', 1, self.red_scratch, self.red_scratch.numel())
        dpf = self.new(n, PFW)
        d, KG = T['d'], K1
        if T.get('best') is not None:                               # backward over the two columns per agent that carry a gradient
            d, KG = self.decoder_live(T['d'], T['best']), 2
        din = self.decoder_bwd(d, T['dpred'], T['drec'], dpf, None, dpf_accumulate=False)
        dqz = self.new(n, zd)                                       # gradient of the posterior draw = sample 0 of every agent: dz of row a KG
        capi.call('sttode_rows_copy', dqz, zd, din[:, PFW:], KG * self.IN, n, zd, 1, n, self.st)
        dqzp = T['dqzp']                                            # starts as the KL gradient
        self.ew(EW_RSAMPLE_BWD, dqz, T['qzp'], T['eps_q'], dqzp, i0=zd)
        dhq = self.lin_bwd(dqzp, P['future_encoder.qz_layer.weight'], T['hq'], g('future_encoder.qz_layer.weight'),
                           g('future_encoder.qz_layer.bias'), mask=T['hq'])
        dh = self.lin_bwd(dhq, P['future_encoder.out_mlp.affine_layers.0.weight'], T['hcat'], g('future_encoder.out_mlp.affine_layers.0.weight'),
                          g('future_encoder.out_mlp.affine_layers.0.bias'))
        assert dh.stride(1) == 1 and dh.stride(0) < 65536
        self.ew(EW_AXPY_ROWS, dpf, dh, i0=(dh.stride(0) << 16) | PFW, f0=1.0, count=n * PFW)   # dpf += dhcat[:, :2 D] (read where it is)
        self.trunk_bwd_multi([(T['tf'], dh[:, PFW:]), (T['tp'], dpf)])    # both trunks layer by layer, grouped launches
        capi.call('sttode_twgrad_defer', 0, None, 0)                # the pending reductions run here, behind the last gradient
        self.tape = None

    def run_backward(self, gout=None, step_id=None):
        T = self.tape
        if T is not None and step_id is not None and T.get('step_id') != step_id:
            raise SttodeError('training backward: this loss belongs to an earlier forward(); only the most recent forward() of a model '
                              'can be differentiated (its tape was overwritten by the newer forward())')
        self.enqueue_backward()
        if gout is not None:
            self.Gflat.mul_(gout)
        return {k: self.G[k] for k in self.touched}


class _LossFn(torch.autograd.Function):
    """Hands the HIP-computed parameter gradients to autograd: ``total_loss.backward()`` fills ``.grad`` (train.py:83-87).
    The only autograd input is a private scalar anchor (one graph edge instead of one per parameter: the step is host-bound); the
    gradients are written to the parameters' ``.grad`` directly, so ``torch.autograd.grad(total, params)`` is not supported."""

    @staticmethod
    def forward(ctx, total, engine, names, ready, params, anchor):
        ctx.engine, ctx.names, ctx.ready, ctx.params = engine, names, ready, params
        ctx.step_id = engine.tape['step_id'] if (ready is None and engine.tape is not None) else None
        return total.clone()

    @staticmethod
    def backward(ctx, gout):
        if ctx.ready is not None:                                  # graph replay already produced the gradients
            flat, views, state = ctx.ready
            _consume(state)
            flat.mul_(gout)
            G = views
        else:
            G = ctx.engine.run_backward(gout, ctx.step_id)
        _hand_over(G, ctx.names, ctx.params, rotating=ctx.ready is not None)
        return None, None, None, None, None, None


def _consume(state):
    """A graph-replay step hands its gradients over ONCE, through whichever path comes first (the direct one of _LossTensor.backward or
    the autograd node): a second backward() raises like the eager step's consumed tape does, instead of silently doubling ``.grad``."""
    if state['consumed']:
        raise SttodeError('training backward: the tape of this forward() was already consumed (backward() called twice on a '
                          'graph-replayed step); call forward() again')
    state['consumed'] = True


def _hand_over(G, names, params, rotating=False):
    """The gradients of a step become the parameters' ``.grad``: autograd's AccumulateGrad would copy each of the 88 views of the flat
    buffer into a fresh tensor (88 extra kernels per step).  The flat buffer is private to this step, so the views can BE the .grad
    tensors; an existing .grad (gradient accumulation) is added to -- in place when the step's buffer is its own (eager steps), OUT of
    place when it is one of a replayed step's two rotating buffers (the existing .grad may itself be a view of one of them, which a later
    replay overwrites)."""
    for nm, p in zip(names, params):
        g = G.get(nm)
        if g is None or not p.requires_grad:
            continue
        if p.grad is None:
            p.grad = g
        elif rotating:
            p.grad = p.grad + g
        else:
            p.grad.add_(g)


class _LossTensor(torch.Tensor):
    """``total_loss`` as forward() returns it.  ``total_loss.backward()`` (train.py:84) with no arguments hands the gradients over directly
    -- no autograd-engine round trip (thread hand-off, graph traversal: ~0.1 ms of a 1.5 ms step); any other use (a scaled loss, explicit
    ``gradient=``, ``inputs=``, retain_graph) goes through the autograd node the tensor also carries (_LossFn)."""

    def backward(self, gradient=None, retain_graph=None, create_graph=False, inputs=None):
        fast = getattr(self, '_sttode_step', None)
        if fast is None or gradient is not None or inputs is not None or retain_graph or create_graph:
            return super().backward(gradient, retain_graph, create_graph, inputs)
        self._sttode_step = None
        engine, names, ready, params, step_id = fast
        if ready is not None:
            _consume(ready[2])
            G = ready[1]                                           # graph replay already produced the gradients
        else:
            G = engine.run_backward(None, step_id)
        _hand_over(G, names, params, rotating=ready is not None)


_PARKED_GRAPHS = []


class _GraphedStep:
    """One hipGraph per step shape: the ~165 launches of forward-with-tape + backward replayed as a single graph launch
    (the training step is launch-latency-bound at the reference's scene sizes).  Inputs are copied into static buffers,
    the loss values and the flat gradient buffer are static outputs."""

    def __init__(self, eng, net, inputs, drawn=None):
        self.eng, self.net = eng, net
        self.static = {k: (v.clone() if v is not None else None) for k, v in inputs.items()}
        # drawn: name -> (rows, cols, kind) of the random inputs the GRAPH draws itself (torch's generator is graph-safe: a captured
        # normal_() / bernoulli_() reads seed and offset at replay, and replay() advances the offset by the graph's total) -- in the order
        # and with the calls of the eager step, so a seeded run draws the same numbers either way
        self.drawn = drawn or {}
        for k, (rows, cols, kind) in self.drawn.items():
            if kind != 'unused':
                self.static[k] = torch.empty(rows, cols, device=eng.dev)
        self.graph = None

    def __del__(self):
        # torch's CUDAGraph destructor synchronises the device on ROCm; while a stream of the process is being captured that call is refused
        # and the failed check inside a destructor aborts the process (profiles/exp_r05_capture_gc_stress.py: a model collected inside a
        # user's own torch.cuda.graph block).  A graph that dies during a capture is parked instead and released by the next replay.
        try:
            g = getattr(self, 'graph_obj', None)
            if g is not None and torch.cuda.is_current_stream_capturing():
                _PARKED_GRAPHS.append(g)
        except Exception:                                           # (interpreter shutdown: the module's globals may be gone)
            pass

    def _bind(self):
        net, st = self.net, self.static
        net._past, net._future = st['past'], st['future']
        if st['scene_ptr'] is not None:
            net._scene_ptr = st['scene_ptr']

    def _capture(self):
        """The whole step (forward with tape + backward) as ONE hipGraph on one stream.  Measured alternatives: the future trunk as a
        branch of the same graph, or pieces of the step as graphs of their own replayed on two streams -- hipGraphLaunch feeds a
        graph's kernels at about the rate a queue executes small dependent kernels (~5 us each), so neither ran the trunks
        concurrently, and every graph boundary cost 20-60 us of idle queue (7 graphs: ~0.15 ms per step)."""
        eng, st = self.eng, self.static
        eng.prepare_forward()                                       # host side, and the engine's own buffers: outside the capture
        torch.cuda.synchronize()
        # The loss values leave for the host in the MIDDLE of the graph (after the forward half): forward() returns them as Python floats
        # (model/STTODE.py:568), and reading them off the end of the queue (`.tolist()`) left the GPU idle for the whole host side of
        # train.py:61-67 -- zero_grad, backward's hand-over, optimizer.step, the next set_data and draws: 0.21 ms of a 0.81 ms one-scene step
        # (profiles/r05/train_host_window.txt).  One launch publishes them to pinned memory with a sequence count; run() spins on that word.
        self.host_vals = torch.zeros(8, dtype=torch.float32).pin_memory()
        self.host_seq = torch.zeros(2, dtype=torch.int32).pin_memory()
        self.dev_seq = torch.zeros(2, dtype=torch.int32, device=eng.dev)
        self.host_np, self.replays = self.host_vals.numpy(), 0
        self.graph_obj = torch.cuda.CUDAGraph()
        eng.publish = (self.host_vals, self.dev_seq, self.host_seq)
        # No cyclic-collector run inside the capture: the body allocates thousands of Python objects, and a collection it trips may destroy
        # whatever garbage the process holds -- other models' native handles (streams, events), pinned buffers, older graphs -- whose
        # destructors make HIP calls that are not permitted while a stream captures (the runtime aborts the process: seen once a
        # collection happened to fall into _grad_views under capture).  torch.cuda.graph collects on entry; from there to the end: off.
        import gc
        gc_was_on = gc.isenabled()
        gc.disable()
        try:
            with torch.cuda.graph(self.graph_obj):
                for k, (rows, cols, kind) in self.drawn.items():
                    if kind == 'unused':
                        torch.randn(rows, cols, device=eng.dev)     # pz_distribution.rsample(): drawn, never used (model/STTODE.py:525)
                    elif kind == 'bern':
                        st[k].bernoulli_(_DROP_KEEP).div_(_DROP_KEEP)
                    else:
                        st[k].normal_()
                eng.enqueue_forward(st['eps_q'], st['eps20'], st['drop_past'], st['drop_future'])
                eng.enqueue_backward()
        finally:
            eng.publish = None
            if gc_was_on:
                gc.enable()
        self.keep = (eng.V, eng.G, eng.scratch, eng.red_scratch)        # static buffers of the graph
        self.out = (eng.V['losses'], eng.Gflat, {k: eng.G[k] for k in eng.touched})

    def run(self, inputs):
        one_scene = self.graph is not None and self.net._mode == 'scenes' and self.net._S == 1
        for k, v in inputs.items():
            if k == 'scene_ptr' and one_scene:                      # [0, n] for ONE scene of n agents (n is part of the graph's key): copied when captured
                continue
            if v is not None and v is not self.static[k]:           # (random inputs nobody passed in are drawn by the graph itself)
                self.static[k].copy_(v)
        self._bind()
        if _PARKED_GRAPHS:                                          # graphs that died during somebody's capture (see __del__): nothing captures now
            _PARKED_GRAPHS.clear()
        if self.graph is None:
            self._capture()
            self.graph = True
            self.attrs = {k: getattr(self.net, k) for k in ('past_feature', 'qz_param', 'qz_sampled', 'pred_traj', 'recover_traj',
                                                            'diverse_pred_traj', 'past_traj', 'future_traj', 'cur_location')}
        self.graph_obj.replay()
        for k, v in self.attrs.items():
            setattr(self.net, k, v)
        losses, flat, G = self.out
        # .grad must not alias the graph's static output: the step's gradients are copied (ONE D2D copy) into one of TWO persistent flat
        # buffers used in turn, whose per-parameter views are built once -- a fresh clone per step needed 88 slice + view operations, ~0.15 ms
        # of host time on the host-bound one-scene step.  A step's gradients therefore stay valid until the step after the next one runs;
        # gradients that are ACCUMULATED across steps never live in these buffers (_hand_over adds out of place).
        if getattr(self, 'rot', None) is None:
            self.rot, self.rot_i = [], 0
            for _ in range(2):
                buf = torch.empty_like(flat)
                views, off = {}, 0
                for k, v in self.eng.P.items():
                    if k in G:
                        views[k] = buf[off: off + v.numel()].view(v.shape)
                    off += ((v.numel() + 3) // 4) * 4
                self.rot.append((buf, views))
        buf, views = self.rot[self.rot_i]
        self.rot_i ^= 1
        buf.copy_(flat)
        total = losses[4].clone()
        self.replays = (self.replays + 1) & 0xFFFFFFFF
        if capi.lib().sttode_wait_value(self.host_seq.data_ptr(), self.replays, 60.0):
            msg = capi.lib().sttode_last_error().decode()
            torch.cuda.synchronize()
            self.replays = int(self.dev_seq[0].item()) & 0xFFFFFFFF     # whatever did run: the next replay is counted from the device's own count
            raise capi.SttodeError('the replayed step did not publish its loss values: ' + msg)
        return (total, self.host_np[:4].tolist()), (buf, views, {'consumed': False, 'rotating': True})


def _names_params(eng, net):
    """(names, parameters, pointer token) of ``net``, cached on the engine and VALIDATED on every call: each cached Parameter must still
    be the object registered under its name in its module, and each module the one registered in its parent (~130 dict look-ups; walking
    named_parameters() every step costs ~0.1 ms of a 1.3 ms step).  A replaced Parameter or sub-module rebuilds the cache, and the token
    -- a hash of every parameter's storage pointer, part of the hipGraph key -- changes with it, so a captured graph is never replayed
    against parameters it does not hold and ``.grad`` lands on the live objects."""
    cache = getattr(eng, '_names_params', None)
    if cache is not None:
        names, params, token, pslots, mslots = cache
        if all(m._parameters.get(k) is p for m, k, p in pslots) and all(pm._modules.get(k) is m for pm, k, m in mslots):
            return names, params, token
    names, params, pslots, mslots = [], [], [], []
    for mname, mod in net.named_modules():
        if mname:
            parent, _, leaf = mname.rpartition('.')
            mslots.append((net.get_submodule(parent) if parent else net, leaf, mod))
    for name, p in net.named_parameters():
        mname, _, leaf = name.rpartition('.')
        names.append(name)
        params.append(p)
        pslots.append((net.get_submodule(mname) if mname else net, leaf, p))
    token = hash(tuple(p.data_ptr() for p in params))
    eng._names_params = (names, params, token, pslots, mslots)
    return names, params, token


_GRAPH_MAX_AGENTS = int(os.environ.get('STTODE_TRAIN_GRAPH_MAX', '512'))
_DROP_KEEP = 0.9

def training_forward(net, eps_q=None, eps_p=None, eps20=None, drop_past=None, drop_future=None):
    """STTODENet.forward() with autograd support (see module docstring).  Returns the reference's 5-tuple.
    ``net.train_graphs`` (default True): after one eager step per shape the whole step is captured into a hipGraph."""
    a, dev = net.args, net.device
    n = net._past.shape[0]
    eng = getattr(net, '_engine', None)
    if eng is None or eng.dev != dev:
        eng = net._engine = Engine(net)
        net._graphs, net._graph_seen = {}, set()
    names, params, ptr_token = _names_params(eng, net)
    ready = None
    keep = _DROP_KEEP                                               # nn.Dropout(0.1) after the positional fc, both encoders (train mode)
    # random inputs the caller did not pass in, in the order the eager step draws them: (name, rows, cols, kind)
    want = [('eps_q', n, a.zdim, 'normal' if eps_q is None else None), ('eps_p', n, a.zdim, 'unused' if eps_p is None else None),
            ('eps20', n * 20, a.zdim, 'normal' if eps20 is None else None),
            ('drop_past', n * a.past_length, a.hidden_dim, 'bern' if (drop_past is None and net.training) else None),
            ('drop_future', n * a.future_length, a.hidden_dim, 'bern' if (drop_future is None and net.training) else None)]
    drawn = {nm: (r, c, kind) for nm, r, c, kind in want if kind is not None}
    key = (net._mode, n, net._S if net._mode == 'scenes' else net.batch_size, drop_past is not None or net.training,
           drop_future is not None or net.training, tuple(drawn), _LIVE_COLUMNS, _AGENT_GRU,
           ptr_token, params[0].data_ptr(), params[-1].data_ptr(),     # graphs hold raw parameter pointers ...
           float(a.min_clip), float(net.ODE_TIME))            # ... and bake scalar kernel arguments in
    prog = eng.ode_program()                                        # (raises for a non-default integrator at generic widths)
    if prog is not None:                                            # the stage program is part of what a graph holds (the default key is as before)
        key = key + (prog,)
    if net._diverse_joint():                                        # a graph holds ONE objective launch: the two modes never share one (default key as before)
        key = key + ('diverse_joint',)
    # a step is ~170 launches of 5-30 us each and the host needs ~15 us to enqueue one: replay wins as long as the launches are short
    # (one scene: launch-bound; an NBA batch of 32 x 11 agents: 3.5 ms eager for 2.5 ms of kernels)
    graphs = getattr(net, 'train_graphs', os.environ.get('STTODE_TRAIN_GRAPHS', '1') != '0') and net._future is not None and n <= _GRAPH_MAX_AGENTS
    replay = graphs and (key in net._graphs or key in net._graph_seen)

    def given(t):
        return None if t is None else t.to(dev, torch.float32).contiguous()
    if replay:                                                      # the graph draws what is missing (see _GraphedStep)
        eps_q, eps20, drop_past, drop_future = given(eps_q), given(eps20), given(drop_past), given(drop_future)
        inputs = dict(past=net._past, future=net._future, scene_ptr=net._scene_ptr if net._mode == 'scenes' else None,
                      eps_q=eps_q, eps20=eps20, drop_past=drop_past, drop_future=drop_future)
        if key not in net._graphs:
            if len(net._graphs) >= 48:
                net._graphs.clear()
            net._graphs[key] = _GraphedStep(eng, net, inputs, drawn)
        losses, ready = net._graphs[key].run(inputs)
    else:
        def draw(t, name):
            if t is not None or name not in drawn:
                return given(t)
            rows, cols, kind = drawn[name]
            out = torch.empty(rows, cols, device=dev)
            return out.bernoulli_(keep).div_(keep) if kind == 'bern' else out.normal_()
        eps_q = draw(eps_q, 'eps_q')
        if 'eps_p' in drawn:
            torch.randn(n, a.zdim, device=dev)                      # pz_distribution.rsample(): drawn, never used (model/STTODE.py:525)
        eps20 = draw(eps20, 'eps20')
        drop_past, drop_future = draw(drop_past, 'drop_past'), draw(drop_future, 'drop_future')
        if graphs:
            net._graph_seen.add(key)                                # first time: eager (also warms one-time kernel attributes)
    if ready is None:
        losses = eng.run_forward(eps_q, eps20, drop_past, drop_future)
        tot_dev, lv = losses[4], None
    else:
        tot_dev, lv = losses                                        # a replayed step: the four values are on the host already
    if getattr(eng, 'anchor', None) is None:
        eng.anchor = torch.zeros((), device=dev, requires_grad=True)
    total = _LossFn.apply(tot_dev, eng, names, ready, params, eng.anchor).as_subclass(_LossTensor)
    total._sttode_step = (eng, names, ready, params, eng.tape['step_id'] if (ready is None and eng.tape is not None) else None)
    if lv is None:
        lv = losses.tolist()
    return total, lv[0], lv[1], lv[2], lv[3]
