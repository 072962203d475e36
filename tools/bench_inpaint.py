#!/usr/bin/env python3
"""Cost of conditional inpainting: cmdgen_inpaint_chain (resamplings = jump_length = 1, a quarter of every sample's points
fixed) against cmdgen_sample_chain on the same handle, layout and seed, K denoising steps, graphs on, alternating
repetitions; 64 and 256 C-alpha pockets of bench.py's model (shipped architecture, bounded weights).  Also reports the ops of an r = 10 schedule.
Prints one JSON line (ms per chain and per denoising step, median over the repetitions).

    python tools/bench_inpaint.py [--K 1000] [--reps 3] [--batches 64,256]
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
    ap.add_argument('--batches', default='64,256')
    a = ap.parse_args()
    cfg = bounded_config(20, 1000)             # bench.py's workload: shipped architecture, bounded coordinates
    h = hip_backend.Handle(cfg.as_dict(), 0)
    h.load_state_dict(make_state_dict(cfg, seed=0))
    res = {'K': a.K, 'r10_ops': h.inpaint_plan(a.K, 10, 1)[0], 'r10_j10_ops': h.inpaint_plan(a.K, 10, 10)[0]}
    for B in [int(b) for b in a.batches.split(',')]:
        pb = make_pockets(B, 'CA', ragged=True, first_index=7000)
        nl = pb.num_nodes_phar
        pm = np.repeat(np.arange(B), nl)
        local = np.arange(len(pm)) - np.concatenate([[0], np.cumsum(nl)[:-1]])[pm]
        fixed = torch.from_numpy((local < np.maximum(1, nl[pm] // 4)).astype(np.float32)).cuda()
        com = np.stack([pb.x[pb.mask == b].mean(0) for b in range(B)])
        rng = np.random.default_rng(0)
        phx = torch.from_numpy((com[pm] + rng.normal(size=(len(pm), 3)) * 2.5).astype(np.float32)).cuda()
        phoh = torch.from_numpy(np.eye(8, dtype=np.float32)[rng.integers(0, 8, size=len(pm))]).cuda()
        px, poh = torch.from_numpy(pb.x).cuda(), torch.from_numpy(pb.one_hot).cuda()
        h.set_layout(nl, pb.size)
        runs = {'sample': lambda: h.sample_chain(px, poh, a.K, seed=1),
                'inpaint': lambda: h.inpaint_chain(px, poh, phx, phoh, fixed, a.K, seed=1)}
        for f in runs.values():                 # warm-up: graph capture, buffers
            f()
        torch.cuda.synchronize()
        times = {k: [] for k in runs}
        for _ in range(a.reps):
            for k, f in runs.items():
                t0 = time.perf_counter()
                f()
                torch.cuda.synchronize()
                times[k].append(1e3 * (time.perf_counter() - t0))
        st = h.chain_status()
        for k, v in times.items():
            ms = float(np.median(v))
            res[f'b{B}_{k}_ms'] = round(ms, 2)
            res[f'b{B}_{k}_ms_per_step'] = round(ms / (a.K + 1), 4)
        res[f'b{B}_inpaint_over_sample'] = round(res[f'b{B}_inpaint_ms'] / res[f'b{B}_sample_ms'], 4)
        res[f'b{B}_inpaint_status_clean'] = bool(st['max_rel_com_error'] < 1e-2 and st['nan_resets'] == 0)
    h.close()
    print(json.dumps(res))


if __name__ == '__main__':
    main()
