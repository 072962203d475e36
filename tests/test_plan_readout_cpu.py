"""The launch planner (csrc/cmdgen_plan.h) compiled on the host, as tests/plan_check.cpp is: how the option "readout_in_coord" resolves, and that the
17 launch keys recorded in tests/golden/plan_table.npz do not depend on it."""
import functools
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_RECORDED = 17


@functools.lru_cache(maxsize=None)
def exe():
    out = os.path.join(tempfile.mkdtemp(prefix='plan_readout_'), 'plan_readout_check')
    r = subprocess.run(['/opt/rocm/bin/hipcc', '-x', 'c++', '-std=c++17', '-O1', '-Wall', '-Werror', '-I' + os.path.join(ROOT, 'cmdgen_amd', 'csrc'),
                        os.path.join(ROOT, 'tests', 'plan_readout_check.cpp'), '-o', out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return out


def plan(cases):
    """cases: [dict(H, L, S, dyn, joint, no_cutoff, n_cus, split, packs, training, B, nph, npk, opts)] -> [len(cases), 18]"""
    base = dict(H=256, L=5, S=1, dyn=33, joint=0, no_cutoff=0, n_cus=256, split=1, packs=1, training=0, B=64, nph=15, npk=44, opts={})
    lines = []
    for c in cases:
        c = dict(base, **c)
        lines.append('%d %d %d %d %d %d %d %d %d %d %d %d %d %d %s' % (
            c['H'], c['L'], c['S'], c['dyn'], c['joint'], c['no_cutoff'], c['n_cus'], c['split'], c['packs'], c['training'], c['B'], c['nph'],
            c['npk'], len(c['opts']), ' '.join(f'{k} {v}' for k, v in c['opts'].items())))
    r = subprocess.run([exe()], input='\n'.join(lines) + '\n', capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    return np.array([ln.split() for ln in r.stdout.strip().split('\n')], dtype=np.int64).reshape(len(cases), N_RECORDED + 1)


def readout(**case):
    return int(plan([case])[0, N_RECORDED])


SMALL = {'node_mt': 16, 'node64': 0, 'coord_mt': 32}          # what the small layouts of the GPU test force: the 32-row full-K coordinate tile


def test_where_readout_in_coord_resolves():
    # the headline (64 C-alpha pockets) and 32 pockets: on when unset and when 1, off when 0
    for B in (64, 32):
        assert readout(B=B) == 1 and readout(B=B, opts={'readout_in_coord': 1}) == 1 and readout(B=B, opts={'readout_in_coord': 0}) == 0
    # the three-piece engine: where its coordinate list runs on the 32-row full-K tile (at 32 pockets it stays on 16-row tiles)
    assert readout(opts={'half_engine': 0}) == 1 and readout(B=32, opts={'half_engine': 0, 'readout_in_coord': 1}) == 0
    # 256 pockets: the coordinate list runs on 128-row tiles - off whatever the option says
    for v in ({}, {'readout_in_coord': 1}):
        assert readout(B=256, opts=v) == 0
        # the joint model, several GCLs per block, the fp32 engine, other widths, the training forward, a sample of more than 128 nodes
        assert readout(joint=1, opts=v) == 0
        assert readout(S=2, opts=v) == 0
        assert readout(split=0, opts=v) == 0
        for H in (64, 128, 512):
            assert readout(H=H, opts=v) == 0
        assert readout(training=1, opts=v) == 0
        assert readout(npk=366, opts=dict(v, coord_mt=32)) == 0
        # embedding_out^T must fit the coordinate tile's third of the LDS
        assert readout(dyn=40, opts=v) == 1 and readout(dyn=41, opts=v) == 0 and readout(dyn=0, opts=v) == 0
    # small layouts on the forced launches: wherever the launches allow it
    for lay in (dict(B=1, nph=8), dict(B=3, nph=5), dict(B=20, nph=3)):
        assert readout(opts=dict(SMALL, readout_in_coord=1), **lay) == 1
        assert readout(opts=dict(SMALL, readout_in_coord=0), **lay) == 0
    # ... and not on 16-row coordinate tiles (the fp32 instruction's generic tile)
    assert readout(B=2, nph=8, opts={'readout_in_coord': 1}) == 0
    # one block: the only coordinate launch is the last one
    assert readout(L=1) == 1


def test_recorded_launch_keys_do_not_depend_on_the_option():
    layouts = [dict(B=64), dict(B=32), dict(B=256), dict(B=20, nph=3), dict(B=2, nph=8), dict(B=64, npk=366), dict(B=64, joint=1), dict(B=64, S=2),
               dict(B=64, opts={'half_engine': 0}), dict(B=64, split=0), dict(B=64, H=128), dict(B=64, training=1), dict(B=3, nph=5, opts=SMALL)]
    for lay in layouts:
        o = lay.get('opts', {})
        got = plan([dict(lay, opts=dict(o)), dict(lay, opts=dict(o, readout_in_coord=0)), dict(lay, opts=dict(o, readout_in_coord=1)), dict(lay, dyn=0, opts=dict(o))])
        for k in (1, 2, 3):
            assert (got[k, :N_RECORDED] == got[0, :N_RECORDED]).all(), lay
        assert got[1, N_RECORDED] == 0 and got[3, N_RECORDED] == 0
