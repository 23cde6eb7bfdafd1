"""``sttode_amd.optim.Adam``: torch.optim.Adam (what train.py:122 constructs) with the step of ALL parameters as ONE HIP launch.

Drop-in: same constructor, same ``state`` layout (``step`` / ``exp_avg`` / ``exp_avg_sq`` per parameter), so ``state_dict()`` /
``load_state_dict()`` round-trip with torch's class and the reference's checkpoints (train.py:188-213) load.  torch's own implementations
walk the model's 88 small tensors -- foreach: ~0.3 ms of host time and a dozen launches per step, fused: three multi_tensor_apply launches
of 41-44 us -- which is 6 % of an NBA-size step and 13 % of a one-scene step of this model (profiles/r05/); the update itself moves 26 MB.
``csrc/train_optim.hip adam_step_kernel`` does it in one launch from a device table of the tensors.  Options the kernel does not implement
(amsgrad, maximize, capturable, differentiable, sparse or non-fp32 / non-contiguous / CPU tensors) take torch's own step.

Opt-in, for the deep unrolled training paths (RK4 / multi-step Euler encoders, GRU BPTT): ``Adam(..., max_grad_norm=c)`` clips the
gradients to the global 2-norm c (torch.nn.utils.clip_grad_norm_'s formula) and ``skip_nonfinite=True`` leaves parameters and moments
untouched by a step whose gradient norm is NaN / Inf (the reference's unused detect_grad_nan, core/utils.py:268-272, superseded).  Both
run on the device over the same table -- per-chunk sums of squares, one workgroup that writes the norm, the clip coefficient, the apply
flag and the step counters to a small state block, and the update reading them -- with no host round trip: torch's clip walks the 88
tensors again with foreach launches, which is the cost this file exists to remove.  A skipped step does not count towards the bias
corrections (as a step a GradScaler skipped).  ``clip_grad_norm_`` below is the stand-alone drop-in for torch's function.

``RiemannianAdam`` and ``RiemannianSGD`` (the end of this file; csrc/manifold.hip) step ``manifolds.ManifoldParameter``s on
their manifolds -- the optimiser that the reference's core/manifolds interface is written for and the reference does not ship.
"""
import ctypes
import math
import struct

import torch

from . import capi

_NORM, _APPLIED, _SKIPPED = 0, 3, 4      # words of the device state block (include/sttode_hip.h: STTODE_GRAD_STATE_WORDS)


def _chunk_rows(ptrs, offs, numels):
    """Rows of the device tensor table (struct AdamItem of csrc/train_optim.hip) and their total of 1024-element chunks."""
    rows, chunk = [], 0
    for (p, m, v), off, n in zip(ptrs, offs, numels):
        rows.append((p, m, v, off // 4, n, chunk))
        chunk += (n + 1023) // 1024
    return rows, chunk


class Adam(torch.optim.Adam):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, max_grad_norm=None, skip_nonfinite=False, **kw):
        kw.pop('fused', None)
        kw.pop('foreach', None)
        if max_grad_norm is not None:
            if isinstance(max_grad_norm, bool) or not isinstance(max_grad_norm, (int, float)) or not 0 < max_grad_norm < math.inf:
                raise ValueError(f'max_grad_norm must be a positive finite number or None, got {max_grad_norm!r}')
            max_grad_norm = float(max_grad_norm)
        # plain attributes, not entries of param_groups: state_dict() stays interchangeable with torch's class
        self.max_grad_norm, self.skip_nonfinite = max_grad_norm, bool(skip_nonfinite)
        self._gstate = None       # the device state block of the guarded step (norm, coef, apply, counters, per-group scalars); None: never used
        self._guard = None        # (plans it was made for, partials, the host array of SttodeGradGroup, total chunks)
        self._skipped_host = 0    # skipped steps already taken out of _t (the device word counts the ones since)
        self._applied0 = 0        # what the device's `applied` word starts from (load_state_dict: the loaded step)
        self._unfolded = False    # a guarded step ran since the device's count of skipped steps was last read
        self._last_norm = None
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, **kw)
        self._plans = None        # per group: (group, params, device table, chunks, rows, gradient offsets from the first one) -- None: (re)build
        self._t = {}              # group index -> steps taken (the per-parameter ``step`` tensors of torch's state are written on demand)
        self._ngrad = None        # per group: how many parameters had a gradient when the plans were built

    @staticmethod
    def _hip_ok(group, ps):
        if group.get('amsgrad') or group.get('maximize') or group.get('capturable') or group.get('differentiable') or not ps:
            return False
        if isinstance(group['lr'], torch.Tensor):
            return False
        dev = ps[0].device
        return dev.type == 'cuda' and all(p.device == dev and p.dtype == torch.float32 and p.is_contiguous() and not p.grad.is_sparse
                                          and p.grad.dtype == torch.float32 and p.grad.is_contiguous() and p.grad.device == dev for p in ps)

    def _build(self):
        """Validate every group once and upload its tensor table; None if any group needs an option the kernel does not implement."""
        plans = []
        self._ngrad = self._grad_counts()
        for gi, group in enumerate(self.param_groups):
            ps = [p for p in group['params'] if p.grad is not None]
            if not ps:
                continue
            if not self._hip_ok(group, ps):
                return None
            steps = set()
            for p in ps:                                          # torch's lazy state initialisation (same keys, same dtypes)
                st = self.state[p]
                if len(st) == 0:
                    st['step'] = torch.tensor(0.0, dtype=torch.float32)
                    st['exp_avg'] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st['exp_avg_sq'] = torch.zeros_like(p, memory_format=torch.preserve_format)
                steps.add(int(st['step']))
            if len(steps) != 1:
                return None                                       # parameters at different step counts (a hand-made state): torch's own step
            self._t.setdefault(gi, steps.pop())
            g0 = ps[0].grad.data_ptr()
            offs = [p.grad.data_ptr() - g0 for p in ps]
            if any(o % 4 for o in offs):
                return None
            rows, chunk = _chunk_rows([(p.data_ptr(), self.state[p]['exp_avg'].data_ptr(), self.state[p]['exp_avg_sq'].data_ptr()) for p in ps],
                                      offs, [p.numel() for p in ps])
            plans.append((gi, group, ps, torch.tensor(rows, dtype=torch.int64).to(ps[0].device), chunk, len(rows), offs,
                          [p.data_ptr() for p in ps]))
        return plans

    def _grad_counts(self):
        return [sum(p.grad is not None for p in group['params']) for group in self.param_groups]

    def _fold_skips(self):
        """Take the steps the device skipped out of the host's counts (reads the device word: synchronises)."""
        if self._unfolded:
            self._unfolded = False
            sk = int(self._gstate.view(torch.int32)[_SKIPPED])
            if sk:
                self._t = {gi: t - sk for gi, t in self._t.items()}
                self._skipped_host += sk
                self._gstate[_SKIPPED].zero_()

    def _sync_steps(self):
        self._fold_skips()                                        # step = applied: a skipped step does not count
        for gi, group, ps, *_ in (self._plans or ()):
            t = float(self._t.get(gi, 0))
            for p in ps:
                self.state[p]['step'] = torch.tensor(t, dtype=torch.float32)

    def state_dict(self):
        self._sync_steps()
        return super().state_dict()

    def load_state_dict(self, sd):
        super().load_state_dict(sd)
        self._plans, self._t, self._guard = None, {}, None
        steps = [int(st['step']) for st in self.state.values() if 'step' in st]
        self._skipped_host, self._applied0, self._unfolded = 0, (steps[0] if steps else 0), False     # the counters start again from the loaded step
        if self._gstate is not None:
            self._gstate.zero_()
            self._gstate.view(torch.int32)[_APPLIED] = self._applied0

    def add_param_group(self, group):
        super().add_param_group(group)
        self._plans = None

    def _guard_buffers(self, plans):
        """What the guarded step needs besides the plans: the state block (made once, it carries the counters), the partial sums and the
        host array of group records.  None: more groups than the finish kernel takes, or groups on several devices."""
        dev = plans[0][2][0].device
        if len(plans) > capi.GRAD_MAX_GROUPS or any(pl[2][0].device != dev for pl in plans):
            return None
        if self._gstate is None or self._gstate.device != dev:
            self._gstate = torch.zeros(capi.GRAD_STATE_WORDS, dtype=torch.float32, device=dev)
            self._gstate.view(torch.int32)[_APPLIED] = self._applied0
        total = sum(pl[4] for pl in plans)
        arr = (capi.GradGroup * len(plans))()
        for r, (gi, group, ps, table, chunks, nrows, offs, pptrs) in zip(arr, plans):
            r.items, r.n, r.chunks = table.data_ptr(), nrows, chunks
        return plans, torch.empty(total, dtype=torch.float32, device=dev), arr, total

    def _step_fallback_guarded(self):
        """The same semantics with torch's own pieces (amsgrad, CPU tensors, ...): clip, then skip the step if the norm is not finite."""
        params = [p for group in self.param_groups for p in group['params'] if p.grad is not None]
        if not params:
            return
        if self.max_grad_norm is not None:
            norm = torch.nn.utils.clip_grad_norm_(params, self.max_grad_norm)
        else:
            norm = torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(p.grad) for p in params]))
        self._last_norm = norm
        if self.skip_nonfinite and not bool(torch.isfinite(norm)):
            self._skipped_host += 1
        else:
            super().step()

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        plans = self._plans
        if plans is not None:
            # the hot path: the gradients must sit where the uploaded table expects them relative to the first one (the training engine
            # hands every step's gradients out as views of ONE flat buffer with a fixed layout) and the parameters where they were
            # (a parameter outside the plans that has a gradient now -- an unfrozen layer -- changes its group's count, a non-contiguous
            # gradient its offset: rebuild)
            try:
                if self._grad_counts() != self._ngrad:
                    plans = None
                for gi, group, ps, table, chunks, nrows, offs, pptrs in plans or ():
                    g0 = ps[0].grad.data_ptr()
                    if ([p.grad.data_ptr() - g0 if p.grad.is_contiguous() else -1 for p in ps] != offs or ps[-1].data_ptr() != pptrs[-1]
                            or ps[0].data_ptr() != pptrs[0]):
                        plans = None
                        break
            except AttributeError:                                # a gradient is None this step
                plans = None
        guarded = self.max_grad_norm is not None or self.skip_nonfinite
        if plans is None:
            self._sync_steps()
            plans = self._plans = self._build()
            self._guard = None
        if guarded and plans and (self._guard is None or self._guard[0] is not plans):
            self._guard = self._guard_buffers(plans)
            if self._guard is None:
                self._sync_steps()
                plans = self._plans = None
        if plans is None:                                         # an option the kernel does not implement: torch's own step throughout
            if guarded:
                self._step_fallback_guarded()
            else:
                super().step()
            self._t = {}                                          # torch advanced the state's step tensors: the next plans read them again
            return loss
        L, st = capi.lib(), capi.stream_ptr()
        if guarded and plans:
            # norm, coefficient and the apply flag on the device, the update reading them: all on the current stream, nothing synchronises
            _, partials, arr, total = self._guard
            state = self._gstate.data_ptr()
            for r, (gi, group, ps, *_) in zip(arr, plans):
                r.gbase, r.lr, (r.beta1, r.beta2) = ps[0].grad.data_ptr(), group['lr'], group['betas']
                r.step = self._t[gi] = self._t.get(gi, 0) + 1     # (the device takes its count of skipped steps off)
            if L.sttode_grad_norm(arr, len(arr), partials.data_ptr(), total, self.max_grad_norm or 0.0, int(self.skip_nonfinite), state, st):
                raise capi.SttodeError('sttode_grad_norm failed: ' + L.sttode_last_error().decode())
            for i, (gi, group, ps, table, chunks, nrows, offs, pptrs) in enumerate(plans):
                b1, b2 = group['betas']
                if L.sttode_adam_step_guarded(table.data_ptr(), nrows, chunks, ps[0].grad.data_ptr(), b1, b2, group['eps'], group['weight_decay'], state, i, st):
                    raise capi.SttodeError('sttode_adam_step_guarded failed: ' + L.sttode_last_error().decode())
            self._last_norm, self._unfolded = self._gstate[_NORM], True
            return loss
        self._fold_skips()                                        # (only after guarded steps, when the options were switched off again)
        for gi, group, ps, table, chunks, nrows, offs, pptrs in plans:
            t = self._t[gi] = self._t.get(gi, 0) + 1
            b1, b2 = group['betas']
            if L.sttode_adam_step(table.data_ptr(), nrows, chunks, ps[0].grad.data_ptr(), group['lr'], b1, b2, group['eps'], group['weight_decay'], t, st):
                raise capi.SttodeError('sttode_adam_step failed: ' + L.sttode_last_error().decode())
        return loss

    @property
    def steps_taken(self):
        self._fold_skips()
        return dict(self._t)

    @property
    def last_grad_norm(self):
        """The global gradient norm of the last guarded step: a 0-dim tensor on the parameters' device (a view of the state block, read
        without synchronising; the next step overwrites it).  None before the first such step."""
        return self._last_norm

    @property
    def skipped_steps(self):
        """How many steps the non-finite guard has skipped (reads the device word: synchronises)."""
        return self._skipped_host + (int(self._gstate.view(torch.int32)[_SKIPPED]) if self._gstate is not None else 0)


_CLIP_PLANS = {}         # gradient layout (device, offsets from the first gradient, sizes) -> uploaded table, partials, state block
_CLIP_PLANS_MAX = 8


def _clip_plan(grads):
    dev = grads[0].device
    if dev.type != 'cuda' or not all(g.device == dev and g.dtype == torch.float32 and not g.is_sparse and g.is_contiguous() for g in grads):
        return None
    g0 = grads[0].data_ptr()
    offs, numels = tuple(g.data_ptr() - g0 for g in grads), tuple(g.numel() for g in grads)
    if any(o % 4 for o in offs) or not all(numels):
        return None
    key = (dev, offs, numels)
    plan = _CLIP_PLANS.get(key)
    if plan is None:
        rows, chunks = _chunk_rows([(0, 0, 0)] * len(grads), offs, numels)
        arr = (capi.GradGroup * 1)()
        table = torch.tensor(rows, dtype=torch.int64).to(dev)
        arr[0].items, arr[0].n, arr[0].chunks = table.data_ptr(), len(rows), chunks
        plan = (table, arr, torch.empty(chunks, dtype=torch.float32, device=dev), torch.zeros(capi.GRAD_STATE_WORDS, dtype=torch.float32, device=dev))
        while len(_CLIP_PLANS) >= _CLIP_PLANS_MAX:
            _CLIP_PLANS.pop(next(iter(_CLIP_PLANS)))
        _CLIP_PLANS[key] = plan
    return plan


@torch.no_grad()
def clip_grad_norm_(parameters, max_norm, norm_type=2.0, error_if_nonfinite=False, foreach=None):
    """torch.nn.utils.clip_grad_norm_ (same signature, same return value: the total norm, on the device) as two HIP launches plus the
    one-workgroup finish over one table of all gradients, instead of a walk over every tensor.  Kernel path: norm_type 2, fp32 contiguous
    CUDA gradients, 0 < max_norm < inf; anything else is torch's own function.  A NaN norm turns the gradients NaN, as in torch."""
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    parameters = list(parameters)
    grads = [p.grad for p in parameters if p.grad is not None]
    max_norm = float(max_norm)
    plan = _clip_plan(grads) if grads and float(norm_type) == 2.0 and 0 < max_norm < math.inf else None
    if plan is None:
        return torch.nn.utils.clip_grad_norm_(parameters, max_norm, norm_type, error_if_nonfinite, foreach)
    table, arr, partials, state = plan
    arr[0].gbase = grads[0].data_ptr()
    with torch.cuda.device(grads[0].device):
        L, st = capi.lib(), capi.stream_ptr()
        if L.sttode_grad_norm(arr, 1, partials.data_ptr(), arr[0].chunks, max_norm, 0, state.data_ptr(), st):
            raise capi.SttodeError('sttode_grad_norm failed: ' + L.sttode_last_error().decode())
        norm = state[_NORM].clone()
        if error_if_nonfinite and not bool(torch.isfinite(norm)):
            raise RuntimeError(f'The total norm of order {norm_type} for gradients from `parameters` is non-finite, so it cannot be clipped. '
                               'To disable this error and scale the gradients by the non-finite norm anyway, set `error_if_nonfinite=False`')
        if L.sttode_grad_scale(table.data_ptr(), arr[0].n, arr[0].chunks, grads[0].data_ptr(), state.data_ptr(), st):
            raise capi.SttodeError('sttode_grad_scale failed: ' + L.sttode_last_error().decode())
    return norm


# ---------------------------------------------------------------------------------------------------------------------------------------
# Riemannian Adam and SGD (csrc/manifold.hip): a ``manifolds.ManifoldParameter`` is stepped ON its manifold -- Riemannian
# gradient, retraction, the momentum transported to the new point -- every manifold parameter of a param group in ONE launch over a device
# table of the tensors (the manner of ``_chunk_rows`` above: one table row per parameter, one wave per row of the parameter, or per two or four short rows).
# ---------------------------------------------------------------------------------------------------------------------------------------
_PLAIN_ROW = 256         # a plain parameter under RiemannianSGD: cut into rows of this many elements (the rule is elementwise)


def _manifold_code(p):
    """(manifold code, c) of a parameter; plain parameters and ManifoldParameters on manifolds.Euclidean are Euclidean."""
    from . import manifolds
    man = getattr(p, 'manifold', None) if isinstance(p, manifolds.ManifoldParameter) else None
    if man is None or isinstance(man, manifolds.Euclidean):
        return None
    if isinstance(man, manifolds.PoincareBall):
        return capi.MANIFOLDS['poincare'], man.c
    if isinstance(man, manifolds.Oblique):
        return capi.MANIFOLDS['oblique'], 1.0
    raise ValueError(f'{type(man).__module__}.{type(man).__qualname__} ({getattr(man, "name", man)!r}) is not a manifold the Riemannian '
                     'optimisers step on: sttode_amd.manifolds.Oblique, PoincareBall or Euclidean')


def _check_tensor(p, what):
    for t, name in ((p, what), (p.grad, 'the gradient of ' + what)):
        if t.is_sparse:
            raise ValueError(f'{name} is sparse: the Riemannian step kernel takes dense tensors')
        if not t.is_cuda:
            raise ValueError(f'{name} is on {t.device}: the Riemannian step runs only on HIP tensors (no CPU fallback)')
        if t.dtype != torch.float32:
            raise ValueError(f'{name} is {t.dtype}: the Riemannian step kernel takes float32')
        if not t.is_contiguous():
            raise ValueError(f'{name} is not contiguous')
    if p.grad.shape != p.shape or p.grad.device != p.device:
        raise ValueError(f'the gradient of {what} does not match it in shape or device')


class _RiemannianOptimizer(torch.optim.Optimizer):
    """What the two rules share: the check of the manifolds, the device table of a group's tensors and the launch."""

    _rule = None

    def add_param_group(self, group):
        if getattr(self, '_plans', None) is not None:
            self._sync_steps()                                    # (the step counts go to the state before the plans that hold them go)
        super().add_param_group(group)
        for p in self.param_groups[-1]['params']:
            _manifold_code(p)                                     # an unknown manifold is refused here, by name
        self._plans = self._sig = self._plain = None

    def load_state_dict(self, sd):
        super().load_state_dict(sd)
        self._plans = self._sig = self._plain = None
        self._loaded()

    def _loaded(self):
        pass

    def _sync_steps(self):
        pass

    def _signature(self):
        return [tuple((p.data_ptr(), p.grad.data_ptr()) for p in group['params'] if p.grad is not None) for group in self.param_groups]

    def _table(self, entries):
        """entries: (parameter, state buffer 1 or None, state buffer 2 or None, manifold code, c, d) -> (device table, wave slots in all).
        A wave steps one row of d > 32 elements, two rows of d <= 32, four rows of d <= 16 (csrc/manifold.hip riem_group)."""
        words, slot0 = [], 0
        for p, m, v, code, c, d in entries:
            rows = (p.numel() + d - 1) // d
            per_wave = 4 if d <= 16 else 2 if d <= 32 else 1
            words.append((p.data_ptr(), m.data_ptr() if m is not None else 0, v.data_ptr() if v is not None else 0, p.grad.data_ptr(), d, rows,
                          slot0, code, struct.unpack('<q', struct.pack('<d', c))[0], p.numel()))
            slot0 += (rows + per_wave - 1) // per_wave
        assert all(len(w) == capi.RIEMANNIAN_ITEM_WORDS for w in words)
        return torch.tensor(words, dtype=torch.int64).to(entries[0][0].device), slot0

    def _launch(self, dev, table, nrows, total, group, t, tstate):
        b1, b2 = group.get('betas', (0.0, 0.0))
        args = (capi.RIEMANNIAN_RULES[self._rule], table, nrows, total, float(group['lr']), float(b1), float(b2), float(group.get('eps', 0.0)),
                float(group['weight_decay']), float(group.get('momentum', 0.0)), t, tstate)
        if dev.index == torch.cuda.current_device():
            capi.call('sttode_riemannian_step', *args, capi.stream_ptr())
        else:
            with torch.cuda.device(dev):
                capi.call('sttode_riemannian_step', *args, capi.stream_ptr())


class RiemannianAdam(_RiemannianOptimizer):
    """Adam on manifolds.  Per row x of a ``ManifoldParameter`` (g: its gradient, t: the step count from 1):
        g += weight_decay x;  r = egrad2rgrad(x, g);  m = beta1 m + (1 - beta1) r;  v = beta2 v + (1 - beta2) inner_x(r, r)
        y = retr(x, -lr (m / (1 - beta1^t)) / (sqrt(v / (1 - beta2^t)) + eps));  m = ptransp(x, y, m);  x = y
    with ONE second moment per row (``exp_avg_sq`` has shape ``x.shape[:-1] + (1,)``).  State keys: ``step``, ``exp_avg``, ``exp_avg_sq``.
    Every manifold parameter of a group is stepped by one launch; plain parameters (and ManifoldParameters on ``manifolds.Euclidean``)
    take ``sttode_amd.optim.Adam``'s own one-launch step and come out bitwise as that class gives them.  A manifold other than Oblique /
    PoincareBall / Euclidean raises ValueError at construction; non-fp32, non-contiguous, sparse-gradient or CPU tensors raise ValueError
    at the first step (no silent slow path).  No ``amsgrad``, ``max_grad_norm`` or ``skip_nonfinite``.

    A step makes no host round trip.  Captured into a HIP graph (``torch.cuda.graph``), the manifold parameters' step count lives on the
    device and a one-thread launch in front of the step advances it, so replays advance the bias corrections as eager steps do; after a
    capture, the next eager step reads the count back (one synchronisation).  Plain parameters' count is a host argument of
    ``optim.Adam``'s launch: capture a step only for groups of manifold parameters."""

    _rule = 'adam'

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0):
        if not 0.0 <= lr < math.inf:
            raise ValueError(f'Invalid learning rate: {lr}')
        if not 0.0 <= eps < math.inf:
            raise ValueError(f'Invalid epsilon value: {eps}')
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError(f'Invalid betas: {betas}')
        if not 0.0 <= weight_decay < math.inf:
            raise ValueError(f'Invalid weight_decay value: {weight_decay}')
        self._t, self._tstate, self._captured = {}, {}, False
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))

    def _loaded(self):
        self._t, self._tstate, self._captured = {}, {}, False

    def _build(self):
        plans, plain_groups = [], []
        for gi, group in enumerate(self.param_groups):
            entries, steps = [], set()
            plain = [p for p in group['params'] if _manifold_code(p) is None]
            if plain:
                plain_groups.append((group, plain))
            for p in group['params']:
                if p.grad is None:
                    continue
                _check_tensor(p, 'a parameter')
                mc = _manifold_code(p)
                if mc is None or not p.numel():
                    continue
                if p.dim() == 0:
                    raise ValueError('a ManifoldParameter needs a last dimension: its rows are the points of the manifold')
                st = self.state[p]
                if len(st) == 0:
                    st['step'] = torch.tensor(0.0, dtype=torch.float32)
                    st['exp_avg'] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                    st['exp_avg_sq'] = torch.zeros(p.shape[:-1] + (1,), dtype=torch.float32, device=p.device)
                for k in ('exp_avg', 'exp_avg_sq'):
                    if not (st[k].is_cuda and st[k].dtype == torch.float32 and st[k].is_contiguous()):
                        raise ValueError(f'the state buffer {k} of a parameter is not a contiguous float32 HIP tensor')
                steps.add(int(st['step']))
                entries.append((p, st['exp_avg'], st['exp_avg_sq'], mc[0], mc[1], p.shape[-1]))
            if not entries:
                continue
            if len(steps) != 1 or len({e[0].device for e in entries}) != 1:
                raise ValueError('the manifold parameters of a param group must share one step count and one device')
            self._t.setdefault(gi, steps.pop())
            dev = entries[0][0].device
            if gi not in self._tstate or self._tstate[gi].device != dev:
                self._tstate[gi] = torch.full((1,), float(self._t[gi]), dtype=torch.float64, device=dev)
            table, total = self._table(entries)
            plans.append((gi, group, [e[0] for e in entries], table, len(entries), total, dev))
        if self._plain is None and plain_groups:
            # the plain parameters' step IS optim.Adam's: one instance over the same state dict, its groups following this class's groups
            self._plain = Adam([dict(params=ps, lr=g['lr'], betas=g['betas'], eps=g['eps'], weight_decay=g['weight_decay']) for g, ps in plain_groups])
            self._plain.state = self.state
            self._plain_of = [g for g, _ in plain_groups]
        return plans

    def _sync_steps(self):
        if self._captured:                                        # replays advanced the device counts behind the host's back
            for gi, ts in self._tstate.items():
                self._t[gi] = int(ts.item())
        for gi, group, ps, *_ in (self._plans or ()):
            t = float(self._t.get(gi, 0))
            for p in ps:
                self.state[p]['step'] = torch.tensor(t, dtype=torch.float32)
        if self._plain is not None:
            self._plain._sync_steps()

    def state_dict(self):
        self._sync_steps()
        return super().state_dict()

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        sig = self._signature()
        if self._plans is None or sig != self._sig:
            self._sync_steps()
            self._plans, self._sig = self._build(), sig
        if self._plain is not None:
            for pg, g in zip(self._plain.param_groups, self._plain_of):
                pg['lr'], pg['betas'], pg['eps'], pg['weight_decay'] = g['lr'], g['betas'], g['eps'], g['weight_decay']
            if any(p.grad is not None for pg in self._plain.param_groups for p in pg['params']):
                self._plain.step()
        capturing = bool(self._plans) and torch.cuda.is_current_stream_capturing()
        if self._captured and not capturing:
            for gi, ts in self._tstate.items():
                self._t[gi] = int(ts.item())
        for gi, group, ps, table, nrows, total, dev in self._plans:
            if capturing:
                self._captured, t = True, 0
            else:
                t = self._t[gi] = self._t[gi] + 1
            self._launch(dev, table, nrows, total, group, t, self._tstate[gi])
        return loss


class RiemannianSGD(_RiemannianOptimizer):
    """SGD with momentum on manifolds.  Per row x of a ``ManifoldParameter`` (g: its gradient):
        g += weight_decay x;  r = egrad2rgrad(x, g);  buf = momentum buf + r (buf starts at zero; momentum 0: buf = r, not kept)
        y = retr(x, -lr buf);  buf = ptransp(x, y, buf);  x = y
    State key: ``momentum_buffer``.  Plain parameters go through the same launch with the Euclidean code, where the rule is elementwise and
    is ``torch.optim.SGD``'s with ``dampening=0, nesterov=False``.  One launch per group, no host round trip, capturable into a HIP graph.
    Manifolds and tensors are refused as by ``RiemannianAdam``."""

    _rule = 'sgd'

    def __init__(self, params, lr, momentum=0, weight_decay=0):
        if not 0.0 <= lr < math.inf:
            raise ValueError(f'Invalid learning rate: {lr}')
        if not 0.0 <= momentum < math.inf:
            raise ValueError(f'Invalid momentum value: {momentum}')
        if not 0.0 <= weight_decay < math.inf:
            raise ValueError(f'Invalid weight_decay value: {weight_decay}')
        super().__init__(params, dict(lr=lr, momentum=momentum, weight_decay=weight_decay))

    def _build(self):
        plans = []
        for gi, group in enumerate(self.param_groups):
            entries = []
            for p in group['params']:
                if p.grad is None:
                    continue
                _check_tensor(p, 'a parameter')
                mc = _manifold_code(p)
                if mc is not None and p.dim() == 0:
                    raise ValueError('a ManifoldParameter needs a last dimension: its rows are the points of the manifold')
                buf = None
                if group['momentum'] != 0:
                    st = self.state[p]
                    if 'momentum_buffer' not in st:
                        st['momentum_buffer'] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                    buf = st['momentum_buffer']
                    if not (buf.is_cuda and buf.dtype == torch.float32 and buf.is_contiguous()):
                        raise ValueError('the momentum_buffer of a parameter is not a contiguous float32 HIP tensor')
                if mc is None:
                    entries.append((p, buf, None, capi.MANIFOLDS['euclidean'], 1.0, _PLAIN_ROW))
                else:
                    entries.append((p, buf, None, mc[0], mc[1], p.shape[-1]))
            entries = [e for e in entries if e[0].numel()]
            if not entries:
                continue
            if len({e[0].device for e in entries}) != 1:
                raise ValueError('the parameters of a param group must be on one device')
            table, total = self._table(entries)
            plans.append((gi, group, [e[0] for e in entries], table, len(entries), total, entries[0][0].device))
        return plans

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        sig = (self._signature(), [g['momentum'] != 0 for g in self.param_groups])
        if self._plans is None or sig != self._sig:
            self._plans, self._sig = self._build(), sig
        for gi, group, ps, table, nrows, total, dev in self._plans:
            self._launch(dev, table, nrows, total, group, 0, None)
        return loss
