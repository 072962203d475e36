"""The launch planner (csrc/cmdgen_plan.h) compiled on the host, as tests/plan_check.cpp is: how the option "embed_mfma" resolves, and that the 17
launch keys recorded in tests/golden/plan_table.npz do not depend on it (test_planner_reproduces_the_recorded_launch_table replays the whole table
with the option unset; here a handful of layouts with it set to 0, to 1 and unset)."""
import functools
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_RECORDED = 17


@functools.lru_cache(maxsize=None)
def exe():
    out = os.path.join(tempfile.mkdtemp(prefix='plan_options_'), 'plan_options_check')
    r = subprocess.run(['/opt/rocm/bin/hipcc', '-x', 'c++', '-std=c++17', '-O1', '-Wall', '-Werror', '-I' + os.path.join(ROOT, 'cmdgen_amd', 'csrc'),
                        os.path.join(ROOT, 'tests', 'plan_options_check.cpp'), '-o', out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return out


def plan(cases):
    """cases: [dict(H, L, S, joint, no_cutoff, n_cus, split, packs, training, embed_pack, B, nph, npk, opts)] -> [len(cases), 18]"""
    base = dict(H=256, L=5, S=1, joint=0, no_cutoff=0, n_cus=256, split=1, packs=1, training=0, embed_pack=1, B=64, nph=15, npk=44, opts={})
    lines = []
    for c in cases:
        c = dict(base, **c)
        lines.append('%d %d %d %d %d %d %d %d %d %d %d %d %d %d %s' % (
            c['H'], c['L'], c['S'], c['joint'], c['no_cutoff'], c['n_cus'], c['split'], c['packs'], c['training'], c['embed_pack'], c['B'], c['nph'],
            c['npk'], len(c['opts']), ' '.join(f'{k} {v}' for k, v in c['opts'].items())))
    r = subprocess.run([exe()], input='\n'.join(lines) + '\n', capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    return np.array([ln.split() for ln in r.stdout.strip().split('\n')], dtype=np.int64).reshape(len(cases), N_RECORDED + 1)


def embed_mfma(**case):
    return int(plan([case])[0, N_RECORDED])


def test_where_embed_mfma_resolves():
    # the headline (64 C-alpha pockets, H = 256): on when unset and when 1, off when 0
    assert embed_mfma() == 1
    assert embed_mfma(opts={'embed_mfma': 1}) == 1
    assert embed_mfma(opts={'embed_mfma': 0}) == 0
    assert embed_mfma(opts={'embed_mfma': 1, 'half_engine': 0}) == 1 and embed_mfma(split=0) == 1       # the tile's two products are fp32 on every engine
    # its packs do not exist (other encoder sizes, or before cmdgen_finalize_weights); other widths; the training forward - whatever the option says
    for v in ({}, {'embed_mfma': 1}):
        assert embed_mfma(embed_pack=0, opts=v) == 0
        assert embed_mfma(packs=0, embed_pack=0, opts=v) == 0
        for H in (64, 128, 512):
            assert embed_mfma(H=H, opts=v) == 0
        assert embed_mfma(training=1, opts=v) == 0
        assert embed_mfma(training=1, B=2, nph=8, opts=v) == 0
    # no 16-row embedding tile anywhere: the joint model at a size whose node tiles are larger, embed_mt forced to 32 beside 32-row node tiles
    assert embed_mfma(B=256, joint=1) == 0
    assert embed_mfma(B=256, opts={'embed_mt': 32}) == 0
    assert embed_mfma(B=256) == 1                       # (inside a chain k_write_embed's phar tiles are 16 rows at every batch size)
    # unset: from 30 full-path tiles, where every measured run was faster; 1: wherever the form exists
    assert embed_mfma(B=32) == 1 and embed_mfma(B=31) == 0 and embed_mfma(B=20, nph=3) == 0 and embed_mfma(B=2, nph=8) == 0
    assert embed_mfma(B=20, nph=3, opts={'embed_mfma': 1}) == 1 and embed_mfma(B=2, nph=8, opts={'embed_mfma': 1}) == 1
    assert embed_mfma(B=1, nph=1, opts={'embed_mfma': 1}) == 1


def test_recorded_launch_keys_do_not_depend_on_the_option():
    layouts = [dict(B=64), dict(B=32), dict(B=256), dict(B=20, nph=3), dict(B=2, nph=8), dict(B=64, npk=366), dict(B=64, joint=1), dict(B=64, S=2),
               dict(B=64, opts={'half_engine': 0}), dict(B=64, split=0), dict(B=64, H=128), dict(B=64, training=1), dict(B=3, nph=5, opts={'node_mt': 16, 'node64': 0, 'coord_mt': 32})]
    for lay in layouts:
        o = lay.get('opts', {})
        got = plan([dict(lay, opts=dict(o)), dict(lay, opts=dict(o, embed_mfma=0)), dict(lay, opts=dict(o, embed_mfma=1))])
        assert (got[1, :N_RECORDED] == got[0, :N_RECORDED]).all() and (got[2, :N_RECORDED] == got[0, :N_RECORDED]).all(), lay
        assert got[1, N_RECORDED] == 0
