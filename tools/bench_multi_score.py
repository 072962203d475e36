#!/usr/bin/env python3
"""Cost of the multi-pocket scoring chain: one level of cmdgen_multi_score_chain (group rows only, and with the member rows) against
one level of cmdgen_score_chain on the same member layout with the group's rows given to every member (the same evaluations, one
per-member launch per level in both: the difference is the step kernel's), and against one op of cmdgen_multi_pocket_chain - on one
handle, graphs on, alternating repetitions; C-alpha pockets of bench.py's model (shipped architecture, bounded weights); the levels are
t = T .. 1 (K = T = 1000: the diffusion part of the bound itself).  Prints one JSON line per shape: ms per chain and us per op, median
over the repetitions, spread = max - min, and the differences.

    python tools/bench_multi_score.py [--K 1000] [--reps 5] [--shapes 64x2,20x3] [--n_phar 15]
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


def one_shape(h, G, M, a, T):
    B = G * M
    pb = make_pockets(B, 'CA', ragged=True, first_index=7000)
    nl = np.full(B, a.n_phar, dtype=np.int64)  # the members of a group share their point count
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    px, poh = dev(pb.x), dev(pb.one_hot)
    h.set_layout(nl, pb.size)
    w = np.full(B, 1.0 / M, dtype=np.float32)
    nu = G * a.n_phar
    rng = np.random.default_rng(1)
    x = (rng.normal(size=(nu, 3)) * 2.5).astype(np.float32)
    oh = np.eye(8, dtype=np.float32)[rng.integers(0, 8, size=nu)]
    urow = (np.repeat(np.arange(G), M)[:, None] * a.n_phar + np.arange(a.n_phar)[None, :]).reshape(-1)     # the group's rows, once per member
    kx, koh, mx, moh = dev(x), dev(oh), dev(x[urow]), dev(oh[urow])
    levels = (np.arange(a.K, dtype=np.int32)[::-1] + 1) * (T // a.K)
    runs = {'score': lambda: h.score_chain(mx, moh, px, poh, levels, seed=1),
            'multi_score': lambda: h.multi_score_chain(kx, koh, px, poh, [M] * G, w, levels, seed=1),
            'multi_score_members': lambda: h.multi_score_chain(kx, koh, px, poh, [M] * G, w, levels, seed=1, want_members=True),
            'multi': lambda: h.multi_pocket_chain(px, poh, [M] * G, w, a.K, seed=1)}
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
    for k in ('multi_score', 'multi_score_members'):
        res[f'{k}_minus_score_us_per_op'] = round(res[f'{k}_us_per_op'] - res['score_us_per_op'], 3)
        res[f'{k}_minus_multi_us_per_op'] = round(res[f'{k}_us_per_op'] - res['multi_us_per_op'], 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--K', type=int, default=1000)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--shapes', default='64x2,20x3', help='groups x members, comma separated')
    ap.add_argument('--n_phar', type=int, default=15)
    a = ap.parse_args()
    cfg = bounded_config(20, 1000)             # bench.py's workload: shipped architecture, bounded coordinates
    if cfg.timesteps % a.K:
        raise SystemExit(f'--K must divide T = {cfg.timesteps}')
    h = hip_backend.Handle(cfg.as_dict(), 0)
    h.load_state_dict(make_state_dict(cfg, seed=0))
    for shape in a.shapes.split(','):
        G, M = (int(v) for v in shape.split('x'))
        print(json.dumps(one_shape(h, G, M, a, cfg.timesteps)), flush=True)
    h.close()


if __name__ == '__main__':
    main()
