"""Latent sets on the device (csrc/latents.hip): how the K latents of an agent are placed.

``draw`` makes, per agent, a set of M = rounds * K points of N(0, I) in zdim dimensions -- a Sobol sequence under a per-agent
randomisation (``scramble='owen'``: nested uniform scrambling by hash, the default; ``'shift'``: a random digital shift; ``None``: the
raw sequence, whose point 0 is z ~ -6.34 in every dimension -- for checks only) or i.i.d. draws (``kind='random'``) -- optionally as
antithetic pairs, with the prior mode as sample 0, and from a truncated prior -- in the layout ``inference(z=)``,
``inference_async(z=)`` and ``inference_reduced(z=)`` take.  ``LatentSource`` wraps it as the ``z_fn`` of the loops of evaluate.py and
as ``STTODENet.latent_source``.  One launch on the caller's stream; no CPU fallback.

Nothing here claims the sets improve accuracy: that needs a trained checkpoint."""
import contextlib
import math
import numbers

import torch

from . import capi

KINDS = {'sobol': 0, 'random': 1}
SCRAMBLES = {None: 0, 'shift': 1, 'owen': 2}
MAX_M, MAX_ZDIM, DIR_BITS = 65536, 1024, 30

_DIRS = {}   # (device, zdim) -> [zdim, 30] int32 on the device


def _check(n, K, zdim, rounds, kind, scramble, seed, antithetic, center, truncate, first_agent):
    """The arguments of draw() as the C entry takes them, or ValueError (nothing is allocated before this passes)."""
    for name, v in (('n', n), ('K', K), ('zdim', zdim), ('rounds', rounds), ('first_agent', first_agent)):
        if isinstance(v, bool) or not isinstance(v, numbers.Integral):
            raise ValueError(f'{name} must be an int, got {v!r}')
    if n < 1 or K < 1 or rounds < 1:
        raise ValueError(f'n, K and rounds must be positive, got n = {n}, K = {K}, rounds = {rounds}')
    if rounds * K > MAX_M:
        raise ValueError(f'M = rounds * K must be <= {MAX_M}, got {rounds * K}')
    if not 1 <= zdim <= MAX_ZDIM:
        raise ValueError(f'zdim must be in [1, {MAX_ZDIM}], got {zdim}')
    if first_agent < 0 or first_agent + n > 1 << 63:
        raise ValueError(f'first_agent must be in [0, 2^63 - n], got {first_agent}')
    if kind not in KINDS:
        raise ValueError(f"kind must be 'sobol' or 'random', got {kind!r}")
    if scramble not in SCRAMBLES:
        raise ValueError(f"scramble must be 'owen', 'shift' or None, got {scramble!r}")
    if seed is not None and (isinstance(seed, bool) or not isinstance(seed, numbers.Integral) or not 0 <= seed < 1 << 64):
        raise ValueError(f'seed must be None or an int in [0, 2^64), got {seed!r}')
    if center and rounds * K < 2:
        raise ValueError('center needs M = rounds * K >= 2')
    t = 0.0 if truncate is None else float(truncate)
    if truncate is not None and not (math.isfinite(t) and t >= 0.01):
        raise ValueError(f'truncate must be None or finite and >= 0.01, got {truncate!r}')
    return KINDS[kind], SCRAMBLES[scramble], int(bool(antithetic)), int(bool(center)), t


def _device(device):
    dev = torch.device('cuda' if device is None and torch.cuda.is_available() else 'cpu' if device is None else device)
    if dev.type != 'cuda':
        raise capi.SttodeError(f'latents.draw runs on the HIP device only, got device {dev} (there is no CPU fallback)')
    return torch.device('cuda', torch.cuda.current_device()) if dev.index is None else dev


def directions(zdim, device):
    """[zdim, 30] int32 on ``device``: the 30-bit direction numbers of torch.quasirandom.SobolEngine(zdim), read at first use and uploaded
    once per (device, zdim)."""
    key = (str(device), int(zdim))
    if key not in _DIRS:
        st = torch.quasirandom.SobolEngine(int(zdim)).sobolstate
        if tuple(st.shape) != (zdim, DIR_BITS) or int(st.min()) < 0 or int(st.max()) >= 1 << DIR_BITS:
            raise capi.SttodeError(f'SobolEngine({zdim}).sobolstate is not [zdim, {DIR_BITS}] of {DIR_BITS}-bit numbers')
        _DIRS[key] = st.to(torch.int32).contiguous().to(device)
    return _DIRS[key]


def draw(n, K, zdim, rounds=1, kind='sobol', scramble='owen', seed=None, antithetic=False, center=False, truncate=None, first_agent=0,
         device=None, return_bits=False):
    """Latent sets for ``n`` agents: ``[n * K, zdim]`` float32 for ``rounds == 1``, else ``[rounds, n * K, zdim]``; row = agent * K + k, and
    set index m of an agent (M = rounds * K points) lives at round m // K, column m % K.

    ``kind``: 'sobol' (``scramble`` 'owen' | 'shift' | None as above) or 'random' (i.i.d., Philox).  ``seed``: 64 bits; None takes 63 bits
    from torch's generator, so a run under ``torch.manual_seed`` is reproducible.  Agent ``first_agent + i`` is randomised by (seed, its
    index) only: its rows do not depend on the batch it is drawn in.  ``antithetic``: the second half of the set mirrors the first
    (z, -z).  ``center``: set index 0 is the zero vector, the prior mode.  ``truncate`` = t >= 0.01: the prior truncated to [-t, t] per
    dimension.  ``return_bits``: also the int32 tensor of the same shape with the 32-bit integer behind every drawn value (0 where none
    was drawn).  Bad arguments raise ValueError before anything is allocated; a CPU device raises SttodeError."""
    ikind, iscr, anti, cen, t = _check(n, K, zdim, rounds, kind, scramble, seed, antithetic, center, truncate, first_agent)
    dev = _device(device)
    n, K, zdim, rounds, first_agent = int(n), int(K), int(zdim), int(rounds), int(first_agent)
    if seed is None:
        seed = int(torch.empty((), dtype=torch.int64).random_()) & 0x7fffffffffffffff
    # (the launch goes to the current device's current stream; entering a device context costs more than the rest of this function)
    with (contextlib.nullcontext() if torch.cuda.current_device() == dev.index else torch.cuda.device(dev)):
        dirs = directions(zdim, dev) if ikind == 0 else None
        z = torch.empty(rounds, n * K, zdim, dtype=torch.float32, device=dev)
        bits = torch.empty(rounds, n * K, zdim, dtype=torch.int32, device=dev) if return_bits else None
        capi.call('sttode_latent_set', z, bits, dirs, n, K, rounds, zdim, first_agent, int(seed), ikind, iscr, anti, cen, t, capi.stream_ptr())
    if rounds == 1:
        z, bits = z[0], (bits[0] if return_bits else None)
    return (z, bits) if return_bits else z


class LatentSource:
    """``src(rows)`` -> ``[rows, zdim]``: ``draw`` behind every ``z_fn=`` of evaluate.py (``options``: the keywords of ``draw`` except n,
    first_agent and return_bits; ``seed=None`` is fixed once, here, from torch's generator).

    ``rows`` must be a multiple of K; n = rows // K agents.  The reduced loops ask z_fn once per round in round order, so calls
    c * rounds .. c * rounds + rounds - 1 return rounds 0 .. rounds - 1 of ONE draw for the same n agents (a changed ``rows`` inside
    such a group raises ValueError): the M = rounds * K samples of an agent are one sequence.  After each group ``first_agent`` advances
    by n, so every agent of a dataset gets its own randomisation whatever scenes_per_call is.  ``draw_rounds(n)`` returns the whole
    ``[rounds, n * K, zdim]`` and advances (not inside an open group); ``reset()`` rewinds to agent 0.  With K = 1 it also serves as
    the ``eps_fn`` of the sampler loops, which ask for ``[rows, nz]``."""

    def __init__(self, K, zdim, rounds=1, **options):
        bad = sorted(set(options) - {'kind', 'scramble', 'seed', 'antithetic', 'center', 'truncate', 'device'})
        if bad:
            raise ValueError(f'LatentSource: unknown options {bad}')
        self.K, self.zdim, self.rounds = K, zdim, rounds
        _check(1, K, zdim, rounds, options.get('kind', 'sobol'), options.get('scramble', 'owen'), options.get('seed'),
               options.get('antithetic', False), options.get('center', False), options.get('truncate'), 0)
        if options.get('seed') is None:
            options['seed'] = int(torch.empty((), dtype=torch.int64).random_()) & 0x7fffffffffffffff
        self.options = options
        self.reset()

    def reset(self):
        self.first_agent, self._group, self._next = 0, None, 0

    def draw_rounds(self, n):
        if self._group is not None:
            raise ValueError(f'LatentSource.draw_rounds inside an open group (round {self._next} of {self.rounds} is next)')
        z = draw(n, self.K, self.zdim, rounds=self.rounds, first_agent=self.first_agent, **self.options)
        self.first_agent += n
        return z if self.rounds > 1 else z[None]

    def __call__(self, rows):
        rows = int(rows)
        if rows < self.K or rows % self.K:
            raise ValueError(f'LatentSource: rows must be a positive multiple of K = {self.K}, got {rows}')
        if self._group is None:
            z = self.draw_rounds(rows // self.K)
            if self.rounds == 1:
                return z[0]
            self._group, self._next = z, 0
        elif rows != self._group.shape[1]:
            raise ValueError(f'LatentSource: rows changed from {self._group.shape[1]} to {rows} inside a group of {self.rounds} rounds '
                             f'(round {self._next} is next)')
        z = self._group[self._next]
        self._next += 1
        if self._next == self.rounds:
            self._group = None
        return z
