#!/usr/bin/env python3
"""Cost of editing under restraints: cmdgen_restrained_edit_chain beside cmdgen_edit_chain and cmdgen_restrained_chain at the shapes of the
tests' `mixed` and `large` cases (tests/restrained_edit_cases.py: 8 ragged C-alpha pockets with 1-8 points, and 3 samples of which one has a
140-atom pocket - the 1024-thread step), on one handle in one process, from the prior, no jumps, K ops; bench.py's model (shipped architecture,
bounded weights).  The guided chains carry the cases' restraints (a position, a distance window, an exclusion sphere per sample) and the clash
term; the edit chains hold the first half of every sample's points.

Prints one JSON line per shape: us per op = chain time / K, median over the alternating repetitions (graphs on), for the edit chain, the
restrained edit chain with scale = 0 (the edit chain's arithmetic through the new step kernel), the restrained edit chain guided, and the
restrained chain guided.  For the step kernels' own times run it under `rocprofv3 --kernel-trace --stats` with --eager --K 50 --reps 1:
k_inpaint_step_count, k_restrained_step_count and k_restrained_edit_step_count are one dispatch per op.

    python tools/bench_restrained_edit.py [--K 200] [--reps 5] [--eager]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from cmdgen_amd import hip_backend  # noqa: E402
from cmdgen_amd import restraints as rs  # noqa: E402
from cmdgen_amd.synthetic import make_state_dict  # noqa: E402
from bench import bounded_config  # noqa: E402
import restrained_edit_cases as ec  # noqa: E402


def one_shape(h, case, a):
    pb = ec.pockets(case)
    phar = ec.phar_dict(case, pb)
    fx, fh = ec.marks(case)
    rec = rs.records(ec.restraints_of(case, pb), case.nph)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    px, poh, phx, phoh, dfx, dfh = dev(pb.x), dev(pb.one_hot), phar['x'].cuda(), phar['one_hot'].cuda(), dev(fx), dev(fh)
    h.set_layout(pb.num_nodes_phar, pb.size)
    g = not a.eager
    guide = dict(restraints=rec, clash_radius=ec.CLASH[0], clash_k=ec.CLASH[1], max_shift=ec.MAX_SHIFT)
    runs = {'edit': lambda: h.edit_chain(px, poh, phx, phoh, dfx, dfh, a.K, seed=1, use_graph=g),
            'restrained_edit_scale0': lambda: h.restrained_edit_chain(px, poh, phx, phoh, dfx, dfh, a.K, scale=0.0, seed=1, use_graph=g, **guide),
            'restrained_edit': lambda: h.restrained_edit_chain(px, poh, phx, phoh, dfx, dfh, a.K, scale=1.0, seed=1, use_graph=g, **guide),
            'restrained': lambda: h.restrained_chain(px, poh, a.K, scale=1.0, seed=1, use_graph=g, **guide)}
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
    res = {'shape': case.name, 'K': a.K, 'samples': len(case.nph), 'max_nodes': int((pb.size + pb.num_nodes_phar).max()), 'reps': a.reps,
           'graphs': g, 'readout_in_coord': h.query('readout_in_coord')}
    for k, v in times.items():
        ms = float(np.median(v))
        res[f'{k}_us_per_op'] = round(1e3 * ms / a.K, 2)
        res[f'{k}_spread_us_per_op'] = round(1e3 * (max(v) - min(v)) / a.K, 2)
        res[f'{k}_status_clean'] = bool(status[k]['max_rel_com_error'] < 1e-2 and status[k]['nan_resets'] == 0)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--K', type=int, default=200)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--eager', action='store_true', help='no graphs: every op a dispatch of its own (for a kernel trace)')
    a = ap.parse_args()
    cfg = bounded_config(20, 1000)
    h = hip_backend.Handle(cfg.as_dict(), 0)
    h.load_state_dict(make_state_dict(cfg, seed=0))
    for case in (ec.MIXED, ec.LARGE):
        print(json.dumps(one_shape(h, case, a)), flush=True)
    h.close()


if __name__ == '__main__':
    main()
