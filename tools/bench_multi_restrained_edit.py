#!/usr/bin/env python3
"""Cost of the restrained multi-pocket edit chain: one guided op of cmdgen_multi_restrained_edit_chain against one op of
cmdgen_multi_edit_chain on the same layout (the same evaluations over the G x M member samples, the same plan from the prior at
resamplings = jump_length = 1, the first three points of every group held; the plain op is one per-member launch, the guided op that launch
and, in front of it, one per-group launch that computes the displacement) - with the clash term on and four restraints per group (a position
on a free point, a distance window from a held to a free point and two exclusion spheres), and with scale = 0 (both launches, nothing added)
- on one handle, graphs on, alternating repetitions; C-alpha pockets of bench.py's model (shipped architecture, bounded weights), a different
pocket for every member.  Prints one JSON line per shape (and appends it to --out): ms per chain and us per op, median over the repetitions,
and the ratio of a guided op to a plain one.

    python tools/bench_multi_restrained_edit.py [--K 1000] [--reps 5] [--shapes 32x2,20x3] [--n_phar 15] [--out FILE]
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
from cmdgen_amd import restraints as rs  # noqa: E402
from cmdgen_amd.synthetic import make_state_dict, make_pockets  # noqa: E402
from bench import bounded_config  # noqa: E402

N_HELD = 3


def one_shape(h, G, M, a):
    B = G * M
    pb = make_pockets(B, 'CA', n_phar=a.n_phar)                # the headline's pockets, one per member
    nl = np.full(B, a.n_phar, dtype=np.int64)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    px, poh = dev(pb.x), dev(pb.one_hot)
    h.set_layout(nl, pb.size)
    sizes, w = [M] * G, np.full(B, 1.0 / M, dtype=np.float32)
    rng = np.random.default_rng(1)
    nu = G * a.n_phar
    coms = np.stack([pb.x[pb.mask == g * M].mean(0) for g in range(G)])
    given_x = (np.repeat(coms, a.n_phar, axis=0) + rng.normal(size=(nu, 3)) * 2.5).astype(np.float32)
    given_oh = np.eye(8, dtype=np.float32)[rng.integers(0, 8, size=nu)]
    held = (np.arange(nu) % a.n_phar < N_HELD).astype(np.float32)
    given = [dev(v) for v in (given_x, given_oh, held, held)]
    restraints = []
    for g in range(G):
        at = lambda: tuple(float(v) for v in coms[g] + rng.uniform(-3.0, 3.0, size=3))
        restraints += [{'kind': 'position', 'sample': g, 'point': N_HELD, 'center': at(), 'radius': 1.5, 'k': 1.0},
                       {'kind': 'distance', 'sample': g, 'points': (0, N_HELD + 1), 'lo': 5.0, 'hi': 7.0, 'k': 1.0},
                       {'kind': 'exclusion', 'sample': g, 'center': at(), 'radius': 3.0, 'k': 0.5},
                       {'kind': 'exclusion', 'sample': g, 'center': at(), 'radius': 3.0, 'k': 0.5}]
    rec = rs.records(restraints, np.full(G, a.n_phar, dtype=np.int64))
    guided = lambda scale: h.multi_restrained_edit_chain(px, poh, sizes, w, *given, a.K, restraints=rec, clash_radius=3.0, clash_k=1.0,
                                                         scale=scale, seed=1)
    runs = {'multi_edit': lambda: h.multi_edit_chain(px, poh, sizes, w, *given, a.K, seed=1),
            'multi_restrained_edit_scale0': lambda: guided(0.0),
            'multi_restrained_edit': lambda: guided(1.0)}
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
    res = {'K': a.K, 'groups': G, 'members': M, 'n_phar': a.n_phar, 'held_per_group': N_HELD, 'restraints_per_group': 4, 'clash': True,
           'reps': a.reps}
    for k, v in times.items():
        ms = float(np.median(v))
        res[f'{k}_ms'] = round(ms, 2)
        res[f'{k}_us_per_op'] = round(1e3 * ms / a.K, 3)
        res[f'{k}_spread_us_per_op'] = round(1e3 * (max(v) - min(v)) / a.K, 3)
        res[f'{k}_status_clean'] = bool(status[k]['max_rel_com_error'] < 1e-2 and status[k]['nan_resets'] == 0)
    res['guided_minus_plain_us_per_op'] = round(res['multi_restrained_edit_us_per_op'] - res['multi_edit_us_per_op'], 3)
    res['scale0_minus_plain_us_per_op'] = round(res['multi_restrained_edit_scale0_us_per_op'] - res['multi_edit_us_per_op'], 3)
    res['multi_restrained_edit_over_multi_edit'] = round(res['multi_restrained_edit_us_per_op'] / res['multi_edit_us_per_op'], 4)
    res['multi_restrained_edit_scale0_over_multi_edit'] = round(res['multi_restrained_edit_scale0_us_per_op'] / res['multi_edit_us_per_op'], 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--K', type=int, default=1000)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--shapes', default='32x2,20x3', help='groups x members per batch, comma separated')
    ap.add_argument('--n_phar', type=int, default=15)
    ap.add_argument('--out', default=None, help='append the JSON lines to this file')
    a = ap.parse_args()
    cfg = bounded_config(20, 1000)             # bench.py's workload: shipped architecture, bounded coordinates
    h = hip_backend.Handle(cfg.as_dict(), 0)
    h.load_state_dict(make_state_dict(cfg, seed=0))
    for shape in a.shapes.split(','):
        G, M = (int(v) for v in shape.split('x'))
        line = json.dumps(one_shape(h, G, M, a))
        print(line, flush=True)
        if a.out:
            with open(a.out, 'a') as f:
                f.write(line + '\n')
    h.close()


if __name__ == '__main__':
    main()
