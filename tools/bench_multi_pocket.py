#!/usr/bin/env python3
"""Cost of the multi-pocket chain: cmdgen_multi_pocket_chain over G groups of M members against cmdgen_sample_chain over the same
G x M pockets as independent samples - the same layout, hence the same evaluations and one per-sample launch per step - on one handle,
graphs on, alternating repetitions; C-alpha pockets of bench.py's model (shipped architecture, bounded weights).
Prints one JSON line (ms per chain and per step, median over the repetitions, and the ratio).

    python tools/bench_multi_pocket.py [--K 1000] [--reps 3] [--groups 32] [--members 2] [--n_phar 15]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--K', type=int, default=1000)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--groups', type=int, default=32)
    ap.add_argument('--members', type=int, default=2)
    ap.add_argument('--n_phar', type=int, default=15)
    a = ap.parse_args()
    cfg = bounded_config(20, 1000)             # bench.py's workload: shipped architecture, bounded coordinates
    h = hip_backend.Handle(cfg.as_dict(), 0)
    h.load_state_dict(make_state_dict(cfg, seed=0))
    G, M = a.groups, a.members
    B = G * M
    pb = make_pockets(B, 'CA', ragged=True, first_index=7000)
    nl = np.full(B, a.n_phar, dtype=np.int64)  # the members of a group share their point count
    px, poh = torch.from_numpy(pb.x).cuda(), torch.from_numpy(pb.one_hot).cuda()
    h.set_layout(nl, pb.size)
    w = np.full(B, 1.0 / M, dtype=np.float32)
    runs = {'sample': lambda: h.sample_chain(px, poh, a.K, seed=1),
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
    res = {'K': a.K, 'groups': G, 'members': M, 'pockets': B, 'n_phar': a.n_phar}
    for k, v in times.items():
        ms = float(np.median(v))
        res[f'{k}_ms'] = round(ms, 2)
        res[f'{k}_ms_per_step'] = round(ms / a.K, 5)
        res[f'{k}_status_clean'] = bool(status[k]['max_rel_com_error'] < 1e-2 and status[k]['nan_resets'] == 0)
    res['multi_over_sample'] = round(res['multi_ms'] / res['sample_ms'], 4)
    h.close()
    print(json.dumps(res))


if __name__ == '__main__':
    main()
