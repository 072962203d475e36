#!/usr/bin/env python3
"""Kernel by kernel, are two builds' device listings the same instructions?  For a refactor that moves or recomposes kernels.

    hipcc -S --cuda-device-only --offload-arch=gfx950 <the build's flags> unit.hip -o unit.s        (each unit of each side)
    tools/isa_diff.py --a parent/*.s --b new/*.s [--show KERNEL]

Cuts every listing at its kernel symbols (.amdhsa_kernel names), so a kernel may sit in another file on the other side.  A body is the
instruction text between the symbol's label and its .Lfunc_end, comments and directives dropped, block labels renumbered in order of
appearance.  Prints, per kernel: identical, or both sides' VGPRs, AGPRs, SGPRs, scratch bytes, LDS bytes, occupancy and instruction count
from the kernel's own metadata; kernels that exist on one side only are listed.  --show prints a unified diff of one kernel's two bodies.
Compares text only.  Exit status 0 when every kernel present on both sides is identical."""
import difflib
import re
import subprocess
import sys


def kernels_of(path):
    """-> {mangled name: (body lines, metadata dict)}"""
    lines = open(path).read().split('\n')
    names = [l.split()[1] for l in lines if l.strip().startswith('.amdhsa_kernel ')]
    out = {}
    for name in names:
        start = next(i for i, l in enumerate(lines) if l.startswith(name + ':'))
        body, meta, labels = [], {}, {}
        i = start + 1
        while not lines[i].startswith('.Lfunc_end'):
            l = lines[i].split(';')[0].strip()
            i += 1
            if not l:
                continue
            m = re.match(r'^(\.LBB\d+_\d+):', l)
            if m:
                labels.setdefault(m.group(1), 'L%d' % len(labels))
                body.append(labels[m.group(1)] + ':')
            elif not l.startswith('.'):
                body.append(l)
        for k in range(len(body)):                      # forward references: labels not yet seen when the branch was read
            body[k] = re.sub(r'\.LBB\d+_\d+', lambda m: labels.get(m.group(0), m.group(0)), body[k])
        meta['instructions'] = sum(1 for l in body if not l.endswith(':'))
        # the summary comments the compiler writes behind the body, then the .amdhsa_ block
        while i < len(lines) and not lines[i].strip().startswith('.end_amdhsa_kernel'):
            l = lines[i].strip()
            i += 1
            m = re.match(r'^; (NumVgprs|NumAgprs|TotalNumSgprs|ScratchSize|Occupancy|LDSByteSize): (\d+)', l)
            if m:
                meta[m.group(1)] = int(m.group(2))
            m = re.match(r'^\.amdhsa_(group_segment_fixed_size|private_segment_fixed_size|next_free_vgpr|next_free_sgpr|accum_offset) (\d+)', l)
            if m:
                meta[m.group(1)] = int(m.group(2))
        out[name] = (body, meta)
    return out


def demangle(names):
    try:
        r = subprocess.run(['c++filt'] + list(names), capture_output=True, text=True, check=True)
        return dict(zip(names, r.stdout.strip().split('\n')))
    except Exception:
        return {n: n for n in names}


COLS = ['NumVgprs', 'NumAgprs', 'TotalNumSgprs', 'ScratchSize', 'LDSByteSize', 'Occupancy', 'instructions']


def main():
    a_files = sys.argv[sys.argv.index('--a') + 1:sys.argv.index('--b')]
    rest = sys.argv[sys.argv.index('--b') + 1:]
    show = rest[rest.index('--show') + 1] if '--show' in rest else None
    b_files = rest[:rest.index('--show')] if show else rest
    A, B = {}, {}
    where = {}
    for files, side, tag in ((a_files, A, 'a'), (b_files, B, 'b')):
        for f in files:
            for k, v in kernels_of(f).items():
                side[k] = v
                where[(tag, k)] = f.split('/')[-1]
    pretty = demangle(sorted(set(A) | set(B)))
    same = diff = 0
    for k in sorted(set(A) | set(B), key=lambda k: pretty[k]):
        if k not in A or k not in B:
            print('ONLY IN %s  %s' % ('A' if k in A else 'B', pretty[k]))
            continue
        (ba, ma), (bb, mb) = A[k], B[k]
        moved = '' if where[('a', k)] == where[('b', k)] else '   [%s -> %s]' % (where[('a', k)], where[('b', k)])
        if ba == bb and all(ma.get(c) == mb.get(c) for c in COLS):
            same += 1
            print('identical  %5d instr  %s%s' % (ma['instructions'], pretty[k].split('(')[0], moved))
        else:
            diff += 1
            print('DIFFERENT  %s%s' % (pretty[k].split('(')[0], moved))
            print('           ' + '  '.join('%s %s|%s' % (c, ma.get(c), mb.get(c)) for c in COLS) + ('' if ba != bb else '  (same text)')
                  + ('  (same counts: the instructions differ in order, registers or block layout)' if all(ma.get(c) == mb.get(c) for c in COLS) else ''))
        if show and show in pretty[k]:
            sys.stdout.write('\n'.join(difflib.unified_diff(ba, bb, 'a', 'b', lineterm='', n=2)) + '\n')
    print('%d kernels identical, %d different' % (same, diff))
    return 0 if diff == 0 else 1


if __name__ == '__main__':
    sys.exit(main())
