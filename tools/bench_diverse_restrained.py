#!/usr/bin/env python3
"""Cost of the restrained diverse chain: one op of cmdgen_diverse_restrained_chain (three per-sample launches: frame, pair, the step with both
terms) beside one op of cmdgen_diverse_chain, of cmdgen_restrained_chain and of cmdgen_sample_chain on the same layout - on one handle, graphs
on, alternating repetitions; C-alpha pockets of bench.py's model (shipped architecture, bounded weights), tools/bench_restrained.py's restraint
set (four records per sample, the clash term on) and tools/bench_diverse.py's sets.  Where the library's plan says readout_in_coord = 1 (reported
in every line) the plain and the restrained chain run without k_readout and the two chains with sets keep it, as in tools/bench_diverse.py.  Prints
one JSON line per shape: ms per chain and us per op, median over the repetitions, and the expectation it is there to confirm or refute - a
combined op costs about a diverse op plus the restrained op's increment over a plain op, since it launches what the diverse op launches.

    python tools/bench_diverse_restrained.py [--K 1000] [--reps 5] [--out profiles/diverse_restrained_cost.jsonl]
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

SHAPES = ((64, 15, [16] * 4), (256, 15, [16] * 16), (20, 3, [20]))       # pockets, points per sample, sets; the last is the reference driver's


def one_shape(h, B, n_phar, sets, a):
    pb = make_pockets(B, 'CA', n_phar=n_phar)                  # the headline's pockets
    nl = np.full(B, n_phar, dtype=np.int64)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    px, poh = dev(pb.x), dev(pb.one_hot)
    h.set_layout(nl, pb.size)
    rng = np.random.default_rng(1)
    restraints = []
    for b in range(B):                                         # tools/bench_restrained.py's set
        com = pb.x[pb.mask == b].mean(0)
        at = lambda: tuple(float(v) for v in com + rng.uniform(-3.0, 3.0, size=3))
        restraints += [{'kind': 'position', 'sample': b, 'point': 0, 'center': at(), 'radius': 1.5, 'k': 1.0},
                       {'kind': 'distance', 'sample': b, 'points': (0, 1), 'lo': 5.0, 'hi': 7.0, 'k': 1.0},
                       {'kind': 'exclusion', 'sample': b, 'center': at(), 'radius': 3.0, 'k': 0.5},
                       {'kind': 'exclusion', 'sample': b, 'center': at(), 'radius': 3.0, 'k': 0.5}]
    rec = rs.records(restraints, nl)
    guide = dict(clash_radius=3.0, clash_k=1.0, scale=1.0)
    runs = {'plain': lambda: h.sample_chain(px, poh, a.K, seed=1),
            'restrained': lambda: h.restrained_chain(px, poh, a.K, rec, seed=1, **guide),
            'diverse': lambda: h.diverse_chain(px, poh, a.K, sets, strength=1.0, width=2.0, seed=1),
            'diverse_restrained': lambda: h.diverse_restrained_chain(px, poh, a.K, sets, rec, strength=1.0, width=2.0, seed=1, **guide)}
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
    res = {'K': a.K, 'pockets': B, 'n_phar': n_phar, 'sets': len(sets), 'rows_per_set': int(max(sets)) * n_phar, 'restraints_per_sample': 4,
           'clash': True, 'reps': a.reps, 'readout_in_coord': h.query('readout_in_coord')}
    for k, v in times.items():
        ms = float(np.median(v))
        res[f'{k}_ms'] = round(ms, 2)
        res[f'{k}_us_per_op'] = round(1e3 * ms / a.K, 3)
        res[f'{k}_spread_us_per_op'] = round(1e3 * (max(v) - min(v)) / a.K, 3)
        res[f'{k}_status_clean'] = bool(status[k]['max_rel_com_error'] < 1e-2 and status[k]['nan_resets'] == 0)
    us = lambda k: res[f'{k}_us_per_op']
    res['expected_us_per_op'] = round(us('diverse') + us('restrained') - us('plain'), 3)
    res['measured_over_expected'] = round(us('diverse_restrained') / res['expected_us_per_op'], 4)
    res['diverse_restrained_over_plain'] = round(us('diverse_restrained') / us('plain'), 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--K', type=int, default=1000)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=None, help='also append the JSON lines to this file')
    a = ap.parse_args()
    cfg = bounded_config(20, 1000)             # bench.py's workload: shipped architecture, bounded coordinates
    h = hip_backend.Handle(cfg.as_dict(), 0)
    h.load_state_dict(make_state_dict(cfg, seed=0))
    for B, n_phar, sets in SHAPES:
        line = json.dumps(one_shape(h, B, n_phar, sets, a))
        print(line, flush=True)
        if a.out:
            with open(a.out, 'a') as f:
                f.write(line + '\n')
    h.close()


if __name__ == '__main__':
    main()
