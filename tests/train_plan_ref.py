"""The training step's GEMM launch rules as the launchers held them BEFORE csrc/cmdgen_train_plan.h existed: a transcription of
cmdgen_wgrad_group, cmdgen_sgemm and cmdgen_dgrad_split of csrc/kernels_train.hip at commit 5f4a7d7 (the line numbers below are that file's), statement by
statement - the split-K arithmetic is written out once per kernel because it was.  And the way to ask the planners on the CPU
(tests/train_plan_check.cpp, compiled once per process)."""
import atexit
import functools
import os
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# TrainTune's defaults at 5f4a7d7 (csrc/cmdgen_dev.h:265-275)
TUNE = dict(wgrad_split=-1, wgrad_tile=0, wgrad_k128=131072, wgrad_split_wgs128=384, wgrad_split_wgs64=512, wgrad_wgs=768, dgrad_mt=0)
TUNE_KEYS = tuple(TUNE)
GROUP, SPLIT64, SPLIT128 = 0, 1, 2


def shape(M, N, lddy_mod4=0, ldx_mod4=0, aligned=1, xs=0):
    return (M, N, lddy_mod4, ldx_mod4, aligned, xs)


def wgrad(shapes, K, bf16, split3, force3, tune):
    """-> (kernel, pieces, xs, grid x, grid y, grid z, kchunk, zsplit)                                  kernels_train.hip:582-655"""
    n = len(shapes)
    xs = any(s[5] != 0 for s in shapes)                                                                  # :584-585
    tm = max([1] + [(s[0] + 63) // 64 for s in shapes])                                                  # :586-587
    tn = max([1] + [(s[1] + 63) // 64 for s in shapes])
    env3 = tune['wgrad_split']                                                                           # :589
    tile64 = tune['wgrad_tile'] == 64                                                                    # :590
    ok64, ok128 = True, not tile64                                                                       # :591
    for M, N, lddy4, ldx4, aligned, _ in shapes:                                                         # :592-596
        ok64 = ok64 and M % 64 == 0 and N % 64 == 0 and lddy4 == 0 and ldx4 == 0 and bool(aligned)
        ok128 = ok128 and M % 128 == 0 and N % 128 == 0
    ok128 = ok128 and ok64                                                                               # :597
    tiles128 = sum((s[0] // 128) * (s[1] // 128) for s in shapes)                                        # :603-604
    three = (not bf16) and (force3 or (split3 and env3 != 0 and ok64))                                   # :605
    sp = ok64 and (bf16 or three)                                                                        # :606
    sp128 = sp and ok128 and (force3 or env3 == 1 or (K >= 65536 if bf16 else K * tiles128 >= tune['wgrad_k128']))     # :607
    pieces = 1 if bf16 else 3            # the template argument each ladder picks (:619-622, :636-639, :651-654)
    if sp128:                                                                                            # :608-624
        tm = max([1] + [s[0] // 128 for s in shapes])
        tn = max([1] + [s[1] // 128 for s in shapes])
        tiles = sum((s[0] // 128) * (s[1] // 128) for s in shapes)
        zsplit = (tune['wgrad_split_wgs128'] + tiles - 1) // tiles
        zsplit = max(1, min(zsplit, (K + 127) // 128))
        kchunk = ((K + zsplit - 1) // zsplit + 31) // 32 * 32
        zsplit = (K + kchunk - 1) // kchunk
        return (SPLIT128, pieces, int(xs), tn, tm, n * zsplit, kchunk, zsplit)
    if sp:                                                                                               # :625-641
        tm = max([1] + [s[0] // 64 for s in shapes])
        tn = max([1] + [s[1] // 64 for s in shapes])
        zsplit = (tune['wgrad_split_wgs64'] + tm * tn * n - 1) // (tm * tn * n)
        zsplit = max(1, min(zsplit, (K + 127) // 128))
        kchunk = ((K + zsplit - 1) // zsplit + 63) // 64 * 64
        zsplit = (K + kchunk - 1) // kchunk
        return (SPLIT64, pieces, int(xs), tn, tm, n * zsplit, kchunk, zsplit)
    zsplit = (tune['wgrad_wgs'] + tm * tn * n - 1) // (tm * tn * n)                                      # :643-650
    zsplit = max(1, min(zsplit, (K + 127) // 128))
    kchunk = ((K + zsplit - 1) // zsplit + 63) // 64 * 64
    zsplit = (K + kchunk - 1) // kchunk
    return (GROUP, pieces, int(xs), tn, tm, n * zsplit, kchunk, zsplit)


def sgemm(ta, tb, M, N, K, a_vec, b_vec, split_k, bf16, epi):
    """-> (kt, grid x, grid y, grid z, kchunk, z, epi passed, slot)                                     kernels_train.hip:696-728"""
    tiles = ((N + 63) // 64) * ((M + 63) // 64)                                                          # :700
    if split_k == 0:                                                                                     # :701-706
        split_k = (1024 + tiles - 1) // tiles
        split_k = max(1, min(split_k, (K + 127) // 128))
    kchunk, z = K, 1                                                                                     # :707
    if split_k > 1:                                                                                      # :708-711
        kchunk = ((K + split_k - 1) // split_k + 63) // 64 * 64
        z = (K + kchunk - 1) // kchunk
    grid = ((N + 63) // 64, (M + 63) // 64, z)                                                           # :713
    fat = grid[0] * grid[1] * grid[2] < 1024                                                             # :717
    kt = 64 if fat else 32                                                                               # :720
    # :718-724: k_sgemm_bf16 / k_sgemm <KT, TA, TB, VECA, VECB>; the planner numbers the 64 instantiations by those six bits
    slot = (32 if bf16 else 0) | (16 if kt == 64 else 0) | (8 if ta else 0) | (4 if tb else 0) | (2 if a_vec else 0) | (1 if b_vec else 0)
    return (kt,) + grid + (kchunk, z, 0 if z > 1 else epi, slot)                                         # :718 (z > 1 ? 0 : epi)


def dgrad(M, tune, force_mt):
    """-> rows per tile                                                                                  kernels_train.hip:971-972"""
    mt = tune['dgrad_mt']
    big = force_mt == 64 if force_mt else (mt == 64 if mt else M >= 24576)
    return 64 if big else 32


@functools.lru_cache(maxsize=None)
def check_exe():
    """tests/train_plan_check.cpp as plain host C++ (-x c++: no HIP header is on the include path of a C++ compile)."""
    d = tempfile.mkdtemp(prefix='train_plan_check_')
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    exe = os.path.join(d, 'train_plan_check')
    r = subprocess.run(['/opt/rocm/bin/hipcc', '-x', 'c++', '-std=c++17', '-O1', '-Wall', '-Werror', '-I' + os.path.join(ROOT, 'cmdgen_amd', 'csrc'),
                        os.path.join(ROOT, 'tests', 'train_plan_check.cpp'), '-o', exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return exe


def run_planner(cases):
    """cases: [('wgrad', tune, shapes, K, bf16, split3, force3) | ('sgemm', ta, tb, M, N, K, a_vec, b_vec, split_k, bf16, epi) | ('dgrad', tune, M, force_mt)]
    -> one tuple of ints per case, as the planner answers it."""
    lines, cur = [], None
    for c in cases:
        if c[0] in ('wgrad', 'dgrad') and c[1] is not cur:
            cur = c[1]
            lines.append('tune ' + ' '.join(str(cur[k]) for k in TUNE_KEYS))
        if c[0] == 'wgrad':
            _, _, shapes, K, bf16, split3, force3 = c
            lines.append('wgrad %d %d %d %d %d %s' % (K, bf16, split3, force3, len(shapes), ' '.join(' '.join(map(str, s)) for s in shapes)))
        elif c[0] == 'sgemm':
            lines.append('sgemm ' + ' '.join(str(int(v)) for v in c[1:]))
        else:
            lines.append('dgrad %d %d' % (c[2], c[3]))
    r = subprocess.run([check_exe()], input='\n'.join(lines) + '\n', capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    out = [tuple(int(v) for v in ln.split()) for ln in r.stdout.strip().split('\n')]
    assert len(out) == len(cases)
    return out


def reference(c):
    if c[0] == 'wgrad':
        return wgrad(c[2], c[3], bool(c[4]), bool(c[5]), bool(c[6]), c[1])
    if c[0] == 'sgemm':
        return sgemm(*c[1:])
    return (dgrad(c[2], c[1], c[3]),)
