"""Device assembly of train_gemm.hip, train_ewise.hip and train_trunk.hip: the parent commit's files against this tree's.
usage: python profiles/gemm_host/kernels.py <parent csrc dir> <this tree's csrc dir>  > profiles/gemm_host/kernels.txt   (no GPU needed)
A kernel is its text from its label to .Lfunc_end, comments dropped, local label numbers (.LBB<n>_) replaced by a constant; its resources
are the .vgpr_count .sgpr_count .group_segment_fixed_size .private_segment_fixed_size of its metadata entry."""
import os
import re
import subprocess
import sys
import tempfile

FILES = ('train_gemm.hip', 'train_ewise.hip', 'train_trunk.hip')
FLAGS = '-O3 -std=c++17 -fPIC --offload-arch=gfx950 -Wall -Wno-unused-function --cuda-device-only -S'
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')


def kernels(csrc, name, tmp):
    out = os.path.join(tmp, name + '.s')
    subprocess.run([HIPCC, *FLAGS.split(), os.path.join(csrc, name), '-o', out], check=True)
    text = open(out).read()
    meta = {}
    for m in re.finditer(r'\.group_segment_fixed_size:\s*(\d+).*?\.name:\s*(\S+).*?\.private_segment_fixed_size:\s*(\d+).*?\.sgpr_count:\s*(\d+)'
                         r'.*?\.vgpr_count:\s*(\d+)', text, re.S):
        meta[m.group(2)] = (int(m.group(5)), int(m.group(4)), int(m.group(1)), int(m.group(3)))
    found = {}
    for k in meta:
        body = text[text.index('\n' + k + ':'):]
        body = body[:body.index('.Lfunc_end')]
        lines = []
        for ln in body.splitlines():
            ln = re.sub(r'\.LBB\d+_', '.LBBn_', ln.split(';')[0]).strip()
            if ln:
                lines.append(ln)
        found[k] = (lines, meta[k])
    return found


def main(parent, new):
    print('# Device assembly of every kernel of train_gemm.hip, train_ewise.hip and train_trunk.hip: the parent commit against this tree.')
    print(f'# hipcc {FLAGS}; a kernel is its text from its label')
    print('# to .Lfunc_end, comments dropped, local label numbers (.LBB<n>_) replaced by a constant.  lines: instructions and labels compared.')
    print('# resources: .vgpr_count .sgpr_count .group_segment_fixed_size .private_segment_fixed_size (this tree; equal to the parent where "same").')
    print('file              lines verdict   vgpr  sgpr    lds  private  kernel')
    same = differ = 0
    removed, added = [], []
    with tempfile.TemporaryDirectory() as ta, tempfile.TemporaryDirectory() as tb:
        for f in FILES:
            a, b = kernels(parent, f, ta), kernels(new, f, tb)
            for k in sorted(a):
                if k not in b:
                    removed.append(k)
                    print('%-16s %6d removed  %5d %5d %6d %8d  %s' % ((f, len(a[k][0])) + a[k][1] + (k,)))
                    continue
                ok = a[k] == b[k]
                same, differ = same + ok, differ + (not ok)
                print('%-16s %6d %-8s %5d %5d %6d %8d  %s' % ((f, len(b[k][0]), 'same' if ok else 'DIFFER') + b[k][1] + (k,)))
            added += [k for k in sorted(b) if k not in a]
    print(f'# verdict: {same} same, {differ} differ; removed: {", ".join(removed) or "none"}; not in the parent: {", ".join(added) or "none"}')
    return 1 if differ or added else 0


if __name__ == '__main__':
    sys.exit(main(sys.argv[1], sys.argv[2]))
