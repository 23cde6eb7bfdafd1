"""The start of a chunk step in the headline kernel, traj_chain_kernel<1, 2, false, true>, read from the built library's gfx950 code object
(no GPU needed).  A chunk step of the weight stream (csrc/chain32.hip ChainStreamT) is  begin() .. 48 MFMAs .. end();  what a wave issues
between the workgroup barrier in end() and the first MFMA behind it is serial issue time that nothing hides, so the step keeps that stretch
to the ring's first fragment reads and the DMA instructions themselves:

  * no scalar load in it: the chunk-program entries are fetched in the middle of a step, never across a fragment wait (scalar loads and LDS
    reads share lgkmcnt, so a scalar load in flight turns every fragment wait into lgkmcnt(0));
  * M0 is written, never read: the LDS-DMA asm is its only user, there is no save / restore around a piece, and two pieces 4 KiB apart
    share one M0 write;
  * where the call site knows the next chunk's tile count the DMA pieces are issued in a straight line (no compare, no branch), and the
    scalar instructions of the stretch are the M0 writes alone: every address was computed in front of the barrier.

The parent commit's figures are in the assertions' comments; the instruction mix itself (MFMAs, scalar-base DMA) stays with test_chain_isa.py."""
import os
import re
import statistics
import subprocess
import tempfile

import pytest

from test_chain_isa import HEADLINE, LIB, _code_object, _tool

RING_DMA = re.compile(r'global_load_lds_dwordx4 v\d+, s\[\d+:\d+\] offset:-4096')   # first piece of a pair: only the weight stream issues it


@pytest.fixture(scope='module')
def kernel():
    objdump, readelf = _tool('llvm-objdump'), _tool('llvm-readelf')
    assert os.path.exists(LIB), 'build the library first (__graft_entry__.build())'
    with tempfile.TemporaryDirectory() as d:
        co = os.path.join(d, 'chain.co')
        with open(co, 'wb') as f:
            f.write(_code_object(HEADLINE))
        asm = subprocess.run([objdump, '-d', '--mcpu=gfx950', '--disassemble-symbols=' + HEADLINE, co],
                             capture_output=True, text=True, check=True).stdout
        notes = subprocess.run([readelf, '--notes', co], capture_output=True, text=True, check=True).stdout
    ins = [m.group(1).strip() for m in re.finditer(r'^\s+([a-z][a-z0-9_]*\b[^/\n]*)', asm, re.M)]   # instruction text without the encoding comment
    i = notes.index('.name:           ' + HEADLINE + '\n')
    entry = notes[notes.rfind('- .agpr_count', 0, i):]
    meta = {k: int(re.search(re.escape(k) + r':\s+(\d+)', entry).group(1)) for k in ('.vgpr_count', '.private_segment_fixed_size')}
    return ins, meta


def _op(s):
    return s.split()[0]


def _stretches(ins):
    """Per s_barrier, in linear order: (index, instructions up to the next v_mfma or s_barrier, whether an MFMA ends it, distance to the next v_mfma)."""
    out = []
    for k, s in enumerate(ins):
        if _op(s) != 's_barrier':
            continue
        j = k + 1
        while j < len(ins) and not _op(ins[j]).startswith('v_mfma') and _op(ins[j]) != 's_barrier':
            j += 1
        m = j
        while m < len(ins) and not _op(ins[m]).startswith('v_mfma'):
            m += 1
        out.append((k, ins[k + 1:j], j < len(ins) and _op(ins[j]).startswith('v_mfma'), m - k - 1))
    return out


def _not_a_chunk_step(seg):
    """The exceptions, by what identifies them.  The top of the kernel, of the group path and of a role read their arguments: a block of
    scalar loads from the kernel-argument segment (s[0:1] at entry, or the pair hipcc copied it to), three or more at different constant
    offsets from ONE base; a step's own fetch is one load, or two, from the program's address at a run-time offset.  The top of the
    group loop draws the next group's ticket from the work queue: the kernel's only global_atomic_add."""
    by_base = {}
    for s in seg:
        m = re.match(r's_load_dword\w* s\S+ (s\[\d+:\d+\]), (0x[0-9a-f]+)$', s)
        if m:
            by_base.setdefault(m.group(1), set()).add(m.group(2))
    return any(len(v) >= 3 for v in by_base.values()) or any(_op(s) == 'global_atomic_add' for s in seg)


def test_no_scalar_load_between_barrier_and_first_mfma(kernel):
    ins, _ = kernel
    st = _stretches(ins)
    assert len(st) == 112                                     # the barriers of the kernel are what they were
    steps = [(k, seg, mf) for k, seg, mf, _ in st if any(RING_DMA.match(s) for s in seg) and not _not_a_chunk_step(seg)]
    # the chunk steps proper, a begin() (ring DMA) behind the barrier: 104 of the 112 barriers in this build (the others: four exempt
    # stretches, the barriers without a begin() behind them); pinned, so that a step that drops out of the check is seen
    assert len(steps) >= 104, len(steps)
    left = [(k, s) for k, seg, _ in steps for s in seg if _op(s).startswith('s_load')]
    assert not left, left                                     # parent: 143 over its 112 barriers
    # ... and in the whole kernel no program load sits right in front of a wait that an MFMA needs (parent: 74 s_load_dwordx2)
    direct = [k for k, seg, mf, _ in st if mf for a, b in zip(seg, seg[1:]) if _op(a) == 's_load_dwordx2' and _op(b) == 's_waitcnt']
    assert not direct, direct


def test_m0_is_written_only_by_the_dma_issue(kernel):
    ins, _ = kernel
    named = [s for s in ins if re.search(r'\bm0\b', s)]
    writes = [s for s in named if re.match(r's_mov_b32 m0, (s\d+|vcc_lo|vcc_hi|ttmp\d+)$', s)]
    assert named and len(writes) == len(named), [s for s in named if s not in writes][:8]   # parent: 348 reads (s_mov_b32 sN, m0) and 696 writes
    dma = sum(_op(s) == 'global_load_lds_dwordx4' for s in ins)
    assert len(writes) <= dma, (len(writes), dma)                                          # parent: 696 for 351
    # every M0 write is directly followed by its wait state and a DMA instruction
    for k, s in enumerate(ins):
        if s in writes:
            assert _op(ins[k + 1]) == 's_nop' and _op(ins[k + 2]) == 'global_load_lds_dwordx4', ins[k:k + 3]
    # nothing else in the kernel needs M0: no s_movrel, LDS-direct, GWS or message instruction
    other = [s for s in ins if _op(s).startswith(('s_movrel', 'v_movrel', 'ds_gws', 's_sendmsg', 'v_interp', 'ds_param', 'ds_direct'))]
    assert not other, other[:4]


def test_static_count_steps_issue_straight_line(kernel):
    ins, _ = kernel
    st = _stretches(ins)
    # a chunk step whose call site knows the next chunk's tile count: ring DMA behind the barrier, no compare and no branch up to the first MFMA
    static = [(k, seg) for k, seg, mf, _ in st if mf and any(RING_DMA.match(s) for s in seg)
              and not any(_op(s).startswith(('s_cmp', 's_cbranch')) for s in seg)]
    # The sources have 67 static sites in this kernel (group path 43: 2 x (3 + 3) block-0 MLPs, 12 + 12 GRU, 4 + 3 block-1 MLP; role GRU 24).
    # Of them the 4 conv tiles branch on their non-zero fragment groups, the 6 MFMA-less steps of step 0 end at a barrier, and 6 stretches
    # at loop tops and phase starts hold the loop's or the phase's own compares in linear order: 51 remain in this build (parent: 0, three
    # branches per step).  Pinned at that: a static site that falls back to the run-time form fails here.
    assert len(static) >= 51, len(static)
    pure = 0
    for k, seg in static:
        ops = [_op(s) for s in seg]
        salu = [s for s in seg if s.startswith('s_') and _op(s) not in ('s_nop', 's_waitcnt')]
        rest = [s for s in salu if not re.match(r's_mov_b32 m0, ', s)]
        # no address arithmetic of the DMA behind the barrier (parent: 12-14 SALU).  At the top of a loop the ring parity is not a constant of
        # the code and the LDS address of the fragment reads is formed from it: one multiply, at most
        assert len(rest) <= 1 and all(_op(s) == 's_mul_i32' for s in rest), (k, rest)
        assert ops.count('global_load_lds_dwordx4') <= 3 and len(salu) - len(rest) <= 3, (k, seg)
        assert not any(o.startswith(('s_load', 'v_readfirstlane', 'v_readlane')) for o in ops), (k, seg)
        pure += not rest
    # M0 writes and nothing else in all of them but the four loop tops with the multiply (pinned at this build's 47)
    assert pure >= 47, pure
    # the steps with nothing but the step itself between barrier and MFMA: 4 fragment reads, <= 3 pieces of M0 write / wait state / DMA, waits
    bare = [seg for _, seg in static if not any(_op(s).startswith('v_') for s in seg)]
    assert len(bare) >= 39, len(bare)                           # (this build's count, pinned; the other 12 hold gate or bias math of their phase)
    for seg in bare:
        ops = [_op(s) for s in seg]
        assert set(ops) <= {'ds_read_b128', 's_mov_b32', 's_nop', 's_waitcnt', 'global_load_lds_dwordx4'}, seg
        assert ops.count('ds_read_b128') in (4, 8) and len(seg) <= 20, seg      # (8: the first tile's fragments and a bias row)


def test_median_distance_barrier_to_mfma(kernel):
    ins, _ = kernel
    d = [m for _, _, _, m in _stretches(ins)]
    assert statistics.median(d) < 44, sorted(d)               # parent: 57; entry load moved in front of the barrier and no M0 restore alone: 44


def test_registers_scratch_and_mfmas(kernel):
    ins, meta = kernel
    assert sum(_op(s).startswith('v_mfma') for s in ins) == 2888
    assert meta['.vgpr_count'] <= 256
    assert meta['.private_segment_fixed_size'] <= 12          # the parent's 12 B per lane


def test_no_other_m0_user_in_any_chain_kernel():
    """ChainStreamT and the gathers are shared by every kernel of the chain's code object (all traj_chain_kernel instantiations, gru32_kernel,
    the Q-net): none of them may name M0 in anything but an s_mov_b32 (the DMA issue's writes; the latency roles' glds16_asm still saves and
    restores around its own pieces) -- an s_movrel, s_set_gpr_idx or LDS-direct instruction would read what the DMA issue left there."""
    objdump = _tool('llvm-objdump')
    with tempfile.TemporaryDirectory() as d:
        co = os.path.join(d, 'chain.co')
        with open(co, 'wb') as f:
            f.write(_code_object(HEADLINE))
        asm = subprocess.run([objdump, '-d', '--mcpu=gfx950', co], capture_output=True, text=True, check=True).stdout
    ins = [m.group(1).strip() for m in re.finditer(r'^\s+([a-z][a-z0-9_]*\b[^/\n]*)', asm, re.M)]
    named = [s for s in ins if re.search(r'\bm0\b', s)]
    other = [s for s in named if not re.match(r's_mov_b32 (m0, (s\d+|vcc_lo|vcc_hi|ttmp\d+)|s\d+, m0)$', s)]
    assert named and not other, other[:8]
    assert not [s for s in ins if _op(s).startswith(('s_movrel', 'v_movrel', 's_set_gpr_idx', 'ds_gws', 'v_interp', 'ds_param', 'ds_direct'))]
