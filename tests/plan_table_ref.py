"""The recorded launch table (tests/golden/plan_table.npz, written by tools/dump_plan_table.py from the library as it was BEFORE the launch
planner, csrc/cmdgen_plan.h) and the two ways to replay it: through the planner on the CPU (tests/plan_check.cpp, compiled once per process)
and through Handle.query on the GPU."""
import atexit
import functools
import os
import shutil
import subprocess
import sys
import tempfile
from dataclasses import replace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from dump_plan_table import IN_COLS, OPTION_KEYS, QUERY_KEYS  # noqa: E402  (the table's columns, defined where it is written)

N_IN = len(IN_COLS)


@functools.lru_cache(maxsize=None)
def table():
    z = np.load(os.path.join(ROOT, 'tests', 'golden', 'plan_table.npz'))
    ptr = z['lay_ptr']
    layouts = [(z['lay_nph'][ptr[i]:ptr[i + 1]].astype(np.int64), z['lay_npk'][ptr[i]:ptr[i + 1]].astype(np.int64)) for i in range(len(ptr) - 1)]
    return dict(rows=z['rows'], layouts=layouts, n_cus=int(z['n_cus'][0]))


def options_of(row):
    """{option: value} a row of the table sets."""
    he, key, val = (int(row[IN_COLS.index(c)]) for c in ('half_engine_opt', 'opt_key', 'opt_value'))
    opts = {'half_engine': he} if he >= 0 else {}
    if key >= 0:
        opts[OPTION_KEYS[key]] = val
    return opts


@functools.lru_cache(maxsize=None)
def plan_check_exe():
    """tests/plan_check.cpp as plain host C++ (-x c++: no HIP header is on the include path of a C++ compile)."""
    d = tempfile.mkdtemp(prefix='plan_check_')
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    exe = os.path.join(d, 'plan_check')
    r = subprocess.run(['/opt/rocm/bin/hipcc', '-x', 'c++', '-std=c++17', '-O1', '-Wall', '-Werror', '-I' + os.path.join(ROOT, 'cmdgen_amd', 'csrc'),
                        os.path.join(ROOT, 'tests', 'plan_check.cpp'), '-o', exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return exe


# what plan_check prints behind the query keys: the kernel enums and engines (cmdgen_plan.h's order) and the rest the launchers / the training step read
EXTRA_KEYS = ('msg', 'node', 'coord', 'msg_eng', 'node_eng', 'coord_eng', 'e128_grid', 'embed_mt', 'write_embed', 'reads_frag', 'fwd_half', 'node_half')
MSG = dict(tiles=0, fullk32=1, e128=2)
NODE = dict(tiles=0, node16w=1, node32p=2, node64=3, node64e=4, node64d=5)
COORD = dict(tiles=0, fullk32=1, fullk32_proj=2, e128=3)
ENG = dict(fp32=0, bf3=1, half=2)


def run_planner(layouts, plans, extra=False):
    """layouts: [(nph, npk)]; plans: [dict(H, L, S, joint, sin, no_cutoff, n_cus, gemm_split, layout, opts, packs=1, training=0, E=0, Ec=0)]
    -> [len(plans), len(QUERY_KEYS)], with extra=True also the EXTRA_KEYS columns."""
    lines = ['layout %d %s %s' % (len(a), ' '.join(map(str, a)), ' '.join(map(str, b))) for a, b in layouts]
    for p in plans:
        opts = p.get('opts', {})
        lines.append('plan %d %d %d %d %d %d %d %d %d %d %d %d %d %d %s' % (
            p['H'], p['L'], p['S'], p['joint'], p['sin'], p['no_cutoff'], p['n_cus'], p['gemm_split'], p.get('packs', 1), p.get('training', 0), p.get('E', 0),
            p.get('Ec', 0), p['layout'], len(opts),
            ' '.join(f'{k} {v}' for k, v in opts.items())))
    r = subprocess.run([plan_check_exe()], input='\n'.join(lines) + '\n', capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    out = np.array([ln.split() for ln in r.stdout.strip().split('\n')], dtype=np.int64).reshape(len(plans), len(QUERY_KEYS) + len(EXTRA_KEYS))
    return out if extra else out[:, :len(QUERY_KEYS)]


def table_plans():
    t = table()
    cols = {c: i for i, c in enumerate(IN_COLS)}
    return [dict(H=int(r[cols['H']]), L=int(r[cols['L']]), S=int(r[cols['S']]), joint=int(r[cols['joint']]), sin=int(r[cols['sin']]),
                 no_cutoff=int(r[cols['no_cutoff']]), n_cus=t['n_cus'], gemm_split=int(r[cols['gemm_split_mode']]), layout=int(r[cols['layout']]),
                 opts=options_of(r)) for r in t['rows']]


def describe(row):
    return dict(zip(IN_COLS, (int(v) for v in row[:N_IN])))


def replay_on_gpu():
    """[rows, len(QUERY_KEYS)]: Handle.query of every row's keys - one handle per config, weights from make_state_dict, no kernel launched."""
    from bench import bounded_config
    from cmdgen_amd import hip_backend
    from cmdgen_amd.synthetic import make_state_dict
    t = table()
    rows, layouts = t['rows'], t['layouts']
    got = np.zeros((len(rows), len(QUERY_KEYS)), dtype=np.int64)
    configs = sorted({tuple(int(v) for v in r[:6]) for r in rows})
    for H, L, S, joint, sin, no_cutoff in configs:
        cfg = replace(bounded_config(20, 1000), hidden_nf=H, n_layers=L, inv_sublayers=S, update_pocket_coords=bool(joint), sin_embedding=bool(sin),
                      edge_cutoff=None if no_cutoff else 6.0)
        idx = [i for i, r in enumerate(rows) if tuple(int(v) for v in r[:6]) == (H, L, S, joint, sin, no_cutoff)]
        h = hip_backend.Handle(cfg.as_dict(), 0)
        h.load_state_dict(make_state_dict(cfg, seed=0))
        h.set_layout(*layouts[max((int(rows[i][N_IN - 1]) for i in idx), key=lambda k: int(sum(layouts[k][0]) + sum(layouts[k][1])))])     # the workspaces grow once
        split, opts = None, {}
        for i in idx:
            r = rows[i]
            if not sin and int(r[6]) != split:
                split = int(r[6])
                h.set_gemm_mode(bool(split))
            want = options_of(r)
            if want != opts:
                for k in opts:
                    if k not in want:
                        h.set_option(k, None)
                for k, v in want.items():
                    if opts.get(k) != v:
                        h.set_option(k, v)
                opts = want
            h.set_layout(*layouts[int(r[N_IN - 1])])
            got[i] = [int(h.query(k)) for k in QUERY_KEYS]
        h.close()
    return got
