"""The tile counts that the kernels pass to ChainStreamT::begin(N) as constants (csrc/chain32.hip: mlp_l12, mlp_l3, gru32_conv, gru32_steps)
against the chunk programs the host packs (sttode_amd.packing).  begin(N) at chunk step p issues the DMA of chunk p + 1 with N pieces per
wave and no look at the program's own count: a constant that is too small loses a tile, one that is too large reads a tile too many
(past the pool's end for its last chunk), and neither shows in the shipped build.  This walk is the kernels' consumption order written
down once more on the host; no GPU."""
import pytest

from sttode_amd import packing
from sttode_amd.weights import make_weights


def _mlp_steps(kh, no, nxt):
    """mlp_l12<KH> then mlp_l3<NO, NEXT>: the constant of every chunk step's begin() (None: the run-time form)."""
    assert (1 + kh + 8) % 3 == 0
    steps = [3] * (16 * ((1 + kh + 8) // 3))                    # every chunk of layers 1 + 2 is followed by three tiles (the last by layer 3's first)
    for i in range(0, 8 * no, 3):
        left = 8 * no - (i + 3)
        steps.append(3 if left >= 3 else left if left > 0 else nxt)
    return steps


def _gru_steps(tp):
    """gru32_steps: per step the conv tile's begin(3), eleven gate chunks begin(3), the last gate chunk begin() (next: a conv tile or the
    next phase)."""
    return ([3] + [3] * 11 + [None]) * tp


def _check(prog, steps, what):
    counts = [int(c) for _, c in prog]
    assert len(steps) == len(counts), (what, len(steps), len(counts))
    for p, n in enumerate(steps):
        if n is not None:
            assert counts[(p + 1) % len(counts)] == n, '%s: chunk step %d passes begin(%d), the program holds %d tiles for chunk %d' % (
                what, p, n, counts[(p + 1) % len(counts)], (p + 1) % len(counts))


@pytest.mark.parametrize('Tp,Tf', [(8, 12), (8, 16), (8, 20), (2, 1), (16, 48), (5, 33), (10, 40), (1, 5)])
def test_chain_program_holds_the_kernels_static_counts(Tp, Tf):
    sd = make_weights(1234, past_length=Tp, future_length=Tf)
    cs = packing.chain_stream(sd, Tp, Tf)
    ny = packing.tiles_y32(Tf)
    # traj_chain_kernel: decoder_x (mlp_l3<1, 3>), decoder_y of block 0 (mlp_l3<NY, 1>: the GRU's conv tile follows), GRU, decoder_y of block 1
    # (mlp_l3<NY, 3>: the program starts again with the next group's decoder_x)
    steps = _mlp_steps(0, 1, 3) + _mlp_steps(0, ny, 1) + _gru_steps(Tp) + _mlp_steps(3, ny, 3)
    _check(cs['prog'], steps, 'chain_stream(%d, %d)' % (Tp, Tf))
    # every tile a chunk names lies inside the pool, the constants included (they equal the program's counts)
    assert all(0 <= f and f + c <= len(cs['pool']) for f, c in cs['prog'])


@pytest.mark.parametrize('Tp', [1, 2, 8, 16])
def test_gru_programs_hold_the_kernels_static_counts(Tp):
    sd = make_weights(1234, past_length=Tp, future_length=12)
    gs = packing.gru32_stream(sd, 0, Tp)
    _check(gs['prog'], _gru_steps(Tp), 'gru32_stream(%d)' % Tp)
    rs = packing.role_stream(sd, Tp)
    for key in ('prog_scenes', 'prog_nba'):                     # the role's program starts with the GRU's; TileFeed takes the rest at run time
        prog = rs[key]
        steps = _gru_steps(Tp) + [None] * (len(prog) - 13 * Tp)
        _check(prog, steps, 'role_stream(%d).%s' % (Tp, key))
