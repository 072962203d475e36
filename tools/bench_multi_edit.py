#!/usr/bin/env python3
"""Cost of the multi-pocket edit chain: one op of cmdgen_multi_edit_chain against one op of cmdgen_multi_pocket_chain on the same layout
(the same evaluations; one per-member launch per op in both), from the prior at resamplings = jump_length = 1 - without marks (the
multi-pocket chain's arithmetic through the edit chain's step kernel) and with the first quarter of every group's rows held in both column
groups (step B runs) - on one handle, graphs on, alternating repetitions; C-alpha pockets of bench.py's model (shipped architecture,
bounded weights).  Prints one JSON line per shape: ms per chain and us per op, median over the repetitions, and the differences.

    python tools/bench_multi_edit.py [--K 1000] [--reps 5] [--shapes 64x2,20x3] [--n_phar 15]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cmdgen_amd import hip_backend  # noqa: E402
from cmdgen_amd.synthetic import make_state_dict, make_pockets  # noqa: E402
from bench import bounded_config  # noqa: E402


def one_shape(h, G, M, a):
    B = G * M
    pb = make_pockets(B, 'CA', ragged=True, first_index=7000)
    nl = np.full(B, a.n_phar, dtype=np.int64)  # the members of a group share their point count
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    px, poh = dev(pb.x), dev(pb.one_hot)
    h.set_layout(nl, pb.size)
    w = np.full(B, 1.0 / M, dtype=np.float32)
    nu = G * a.n_phar
    rng = np.random.default_rng(1)
    kx = dev((rng.normal(size=(nu, 3)) * 2.5).astype(np.float32))
    koh = dev(np.eye(8, dtype=np.float32)[rng.integers(0, 8, size=nu)])
    none = dev(np.zeros(nu, np.float32))
    quarter = dev((np.arange(nu) % a.n_phar < max(1, a.n_phar // 4)).astype(np.float32))
    runs = {'multi': lambda: h.multi_pocket_chain(px, poh, [M] * G, w, a.K, seed=1),
            'edit_no_marks': lambda: h.multi_edit_chain(px, poh, [M] * G, w, kx, koh, none, none, a.K, seed=1),
            'edit_marks': lambda: h.multi_edit_chain(px, poh, [M] * G, w, kx, koh, quarter, quarter, a.K, seed=1)}
    for f in runs.values():                     # warm-up: graph capture, buffers
        f()
    torch.cuda.synchronize()
    times = {k: [] for k in runs}
    status = {}
    for _ in range(a.reps):
        for k, f in runs.items():
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            times[k].append(1e3 * (time.perf_counter() - t0))
            status[k] = h.chain_status()
    res = {'K': a.K, 'groups': G, 'members': M, 'pockets': B, 'n_phar': a.n_phar, 'reps': a.reps}
    for k, v in times.items():
        ms = float(np.median(v))
        res[f'{k}_ms'] = round(ms, 2)
        res[f'{k}_us_per_op'] = round(1e3 * ms / a.K, 3)
        res[f'{k}_spread_us_per_op'] = round(1e3 * (max(v) - min(v)) / a.K, 3)
        res[f'{k}_status_clean'] = bool(status[k]['max_rel_com_error'] < 1e-2 and status[k]['nan_resets'] == 0)
    res['edit_no_marks_minus_multi_us_per_op'] = round(res['edit_no_marks_us_per_op'] - res['multi_us_per_op'], 3)
    res['edit_marks_minus_multi_us_per_op'] = round(res['edit_marks_us_per_op'] - res['multi_us_per_op'], 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--K', type=int, default=1000)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--shapes', default='64x2,20x3', help='groups x members, comma separated')
    ap.add_argument('--n_phar', type=int, default=15)
    a = ap.parse_args()
    cfg = bounded_config(20, 1000)             # bench.py's workload: shipped architecture, bounded coordinates
    h = hip_backend.Handle(cfg.as_dict(), 0)
    h.load_state_dict(make_state_dict(cfg, seed=0))
    for shape in a.shapes.split(','):
        G, M = (int(v) for v in shape.split('x'))
        print(json.dumps(one_shape(h, G, M, a)), flush=True)
    h.close()


if __name__ == '__main__':
    main()
