#!/usr/bin/env python3
"""Cost of the diverse chain: one guided op of cmdgen_diverse_chain (three per-sample launches: frame, pair, step) against the same chain with
strength = 0 (its frame and pair launches return at once) and one op of cmdgen_sample_chain on the same layout - on one handle, graphs on,
alternating repetitions; C-alpha pockets of bench.py's model (shipped architecture, bounded weights).  Each batch size runs with one set per 16
samples and with a single set; the reference driver's shape (20 copies x 3 points, one set) closes the list.  Prints one JSON line per shape:
ms per chain and us per op, median over the repetitions, and the ratios to a plain op.

    python tools/bench_diverse.py [--K 1000] [--reps 5] [--shapes 64,256] [--n_phar 15] [--out profiles/diverse_cost.jsonl]
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


def one_shape(h, B, n_phar, sets, a):
    pb = make_pockets(B, 'CA', n_phar=n_phar)                  # the headline's pockets
    nl = np.full(B, n_phar, dtype=np.int64)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    px, poh = dev(pb.x), dev(pb.one_hot)
    h.set_layout(nl, pb.size)
    runs = {'plain': lambda: h.sample_chain(px, poh, a.K, seed=1),
            'diverse_strength0': lambda: h.diverse_chain(px, poh, a.K, sets, strength=0.0, seed=1),
            'diverse': lambda: h.diverse_chain(px, poh, a.K, sets, strength=1.0, width=2.0, seed=1)}
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
    res = {'K': a.K, 'pockets': B, 'n_phar': n_phar, 'sets': len(sets), 'rows_per_set': int(max(sets)) * n_phar, 'reps': a.reps,
           'readout_in_coord': h.query('readout_in_coord')}
    for k, v in times.items():
        ms = float(np.median(v))
        res[f'{k}_ms'] = round(ms, 2)
        res[f'{k}_us_per_op'] = round(1e3 * ms / a.K, 3)
        res[f'{k}_spread_us_per_op'] = round(1e3 * (max(v) - min(v)) / a.K, 3)
        res[f'{k}_status_clean'] = bool(status[k]['max_rel_com_error'] < 1e-2 and status[k]['nan_resets'] == 0)
    res['diverse_over_plain'] = round(res['diverse_us_per_op'] / res['plain_us_per_op'], 4)
    res['diverse_strength0_over_plain'] = round(res['diverse_strength0_us_per_op'] / res['plain_us_per_op'], 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--K', type=int, default=1000)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--shapes', default='64,256', help='pockets per batch, comma separated')
    ap.add_argument('--n_phar', type=int, default=15)
    ap.add_argument('--out', default=None, help='also append the JSON lines to this file')
    a = ap.parse_args()
    cfg = bounded_config(20, 1000)             # bench.py's workload: shipped architecture, bounded coordinates
    h = hip_backend.Handle(cfg.as_dict(), 0)
    h.load_state_dict(make_state_dict(cfg, seed=0))
    shapes = []
    for B in (int(s) for s in a.shapes.split(',') if s):
        shapes += [(B, a.n_phar, [16] * (B // 16) + ([B % 16] if B % 16 else [])), (B, a.n_phar, [B])]
    shapes.append((20, 3, [20]))               # the reference driver's: 20 copies of one pocket, 3 points each
    for B, n_phar, sets in shapes:
        line = json.dumps(one_shape(h, B, n_phar, sets, a))
        print(line, flush=True)
        if a.out:
            with open(a.out, 'a') as f:
                f.write(line + '\n')
    h.close()


if __name__ == '__main__':
    main()
