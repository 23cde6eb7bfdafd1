"""Instruction mix of the headline kernel, traj_chain_kernel<1, 2, false, true> (the lagged launch at ETH shapes), read from the built
library's gfx950 code object: no GPU needed.  The weight stream and the gathers issue LDS-DMA in the scalar-base form (one 32-bit lane
offset, the uniform part of the address in SGPRs) and read the chunk program with scalar loads, so the 64-bit per-lane address adds
(v_lshl_add_u64) and the v_readfirstlane_b32 of the LDS-resident program are gone; the MFMAs are exactly the ones they were."""
import os
import re
import shutil
import struct
import subprocess
import tempfile
from collections import Counter

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.environ.get('STTODE_HIP_LIB') or os.path.join(ROOT, 'sttode_amd', 'lib', 'libsttode_hip.so')
HEADLINE = '_Z17traj_chain_kernelILi1ELi2ELb0ELb1EEv9ChainArgs'


def _tool(name):
    for p in (shutil.which(name), os.path.join(os.environ.get('ROCM_PATH', '/opt/rocm'), 'llvm', 'bin', name)):
        if p and os.path.exists(p):
            return p
    pytest.skip(name + ' not found')


def _section(path, want):
    b = open(path, 'rb').read()
    shoff, = struct.unpack_from('<Q', b, 0x28)
    shentsize, shnum, shstrndx = struct.unpack_from('<HHH', b, 0x3A)
    hdr = lambda i: struct.unpack_from('<IIQQQQ', b, shoff + i * shentsize)
    stroff = hdr(shstrndx)[4]
    for i in range(shnum):
        name, _, _, _, off, size = hdr(i)
        if b[stroff + name:b.index(b'\0', stroff + name)] == want:
            return b[off:off + size]
    raise AssertionError('%s has no %s section' % (path, want.decode()))


def _code_object(symbol, arch='gfx950'):
    """The gfx950 code object (clang offload bundles in .hip_fatbin, one per translation unit) that defines `symbol`."""
    fb = _section(LIB, b'.hip_fatbin')
    magic = b'__CLANG_OFFLOAD_BUNDLE__'
    pos = fb.find(magic)
    while pos >= 0:
        n, = struct.unpack_from('<Q', fb, pos + 24)
        q = pos + 32
        for _ in range(n):
            off, size, tl = struct.unpack_from('<QQQ', fb, q)
            triple = fb[q + 24:q + 24 + tl].decode()
            q += 24 + tl
            co = fb[pos + off:pos + off + size]
            if triple.endswith(arch) and symbol.encode() in co:
                return co
        pos = fb.find(magic, pos + 32)
    raise AssertionError('no %s code object defines %s' % (arch, symbol))


@pytest.fixture(scope='module')
def headline():
    objdump, readelf = _tool('llvm-objdump'), _tool('llvm-readelf')
    assert os.path.exists(LIB), 'build the library first (__graft_entry__.build())'
    with tempfile.TemporaryDirectory() as d:
        co = os.path.join(d, 'chain.co')
        with open(co, 'wb') as f:
            f.write(_code_object(HEADLINE))
        asm = subprocess.run([objdump, '-d', '--mcpu=gfx950', '--disassemble-symbols=' + HEADLINE, co],
                             capture_output=True, text=True, check=True).stdout
        notes = subprocess.run([readelf, '--notes', co], capture_output=True, text=True, check=True).stdout
    ops = Counter(m.group(1) for m in re.finditer(r'^\s+([a-z][a-z0-9_]*)\b', asm, re.M))
    # the kernel's entry in the code object metadata: keys are sorted, .name sits between the register / segment counts
    i = notes.index('.name:           ' + HEADLINE + '\n')
    entry = notes[notes.rfind('- .agpr_count', 0, i):]
    meta = {k: int(re.search(re.escape(k) + r':\s+(\d+)', entry).group(1))
            for k in ('.vgpr_count', '.private_segment_fixed_size')}
    return ops, asm, meta


def test_headline_mfmas_unchanged(headline):
    ops, _, _ = headline
    assert ops['v_mfma_f32_32x32x2_f32'] == 2888
    assert sum(v for k, v in ops.items() if k.startswith('v_mfma')) == 2888


def test_headline_dma_uses_scalar_bases(headline):
    ops, asm, _ = headline
    dma = re.findall(r'global_load_lds_dwordx4\s+(\S+)', asm)
    assert dma and all(re.fullmatch(r'v\d+,', a) for a in dma), 'an LDS-DMA with a 64-bit per-lane address is left'
    assert re.search(r'global_load_lds_dwordx4 v\d+, s\[\d+:\d+\] offset:96', asm), 'gather step not folded into the immediate'
    assert ops['v_lshl_add_u64'] <= 128, ops['v_lshl_add_u64']           # 584 with per-lane 64-bit DMA addresses
    assert ops['v_readfirstlane_b32'] <= 16, ops['v_readfirstlane_b32']  # 256 with the chunk program in LDS


def test_headline_registers_and_scratch(headline):
    _, _, meta = headline
    assert meta['.vgpr_count'] <= 256
    assert meta['.private_segment_fixed_size'] <= 32   # scratch per lane never above the 32 B of the per-lane-address form
