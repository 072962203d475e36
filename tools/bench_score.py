#!/usr/bin/env python3
"""Cost of scoring: cmdgen_score_chain with K + 1 levels against cmdgen_sample_chain with K steps (the same K + 1 evaluations and one
per-sample launch per step) on the same handle and layout, graphs on, alternating repetitions; 64 and 256 C-alpha pockets of bench.py's
model (shipped architecture, bounded weights).  Once, at a small K, the host loop a user had before: ConditionalDDPM.forward(t_int=t)
per level in eval mode (two evaluations per level and a few hundred small tensor operations).
Prints one JSON line (ms per chain and per evaluation, median over the repetitions).

    python tools/bench_score.py [--K 1000] [--reps 3] [--batches 64,256] [--host_K 20]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cmdgen_amd import hip_backend, scoring  # noqa: E402
from cmdgen_amd.synthetic import make_state_dict, make_pockets  # noqa: E402
from bench import bounded_config  # noqa: E402


def host_loop_model(cfg, sd):
    from cmdgen_amd.equivariant_diffusion.dynamics import EGNNDynamics
    from cmdgen_amd.equivariant_diffusion.conditional_model import ConditionalDDPM
    dyn = EGNNDynamics(phar_nf=cfg.phar_nf, residue_nf=cfg.residue_nf, n_dims=3, joint_nf=cfg.joint_nf, hidden_nf=cfg.hidden_nf,
                       n_layers=cfg.n_layers, attention=True, tanh=True, norm_constant=1, inv_sublayers=1, sin_embedding=False,
                       normalization_factor=100, aggregation_method='sum', edge_cutoff=6.0, update_pocket_coords=False)
    ddpm = ConditionalDDPM(dynamics=dyn, phar_nf=cfg.phar_nf, residue_nf=cfg.residue_nf, n_dims=3, timesteps=cfg.timesteps,
                           noise_schedule=cfg.noise_schedule, noise_precision=cfg.noise_precision, loss_type='l2',
                           norm_values=list(cfg.norm_values), size_histogram=np.ones((40, 80)))
    ddpm.load_state_dict({k[len('ddpm.'):]: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return ddpm.cuda().eval()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--K', type=int, default=1000)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--batches', default='64,256')
    ap.add_argument('--host_K', type=int, default=20)
    a = ap.parse_args()
    cfg = bounded_config(20, 1000)             # bench.py's workload: shipped architecture, bounded coordinates
    sd = make_state_dict(cfg, seed=0)
    h = hip_backend.Handle(cfg.as_dict(), 0)
    h.load_state_dict(sd)
    levels = scoring.level_list(cfg.timesteps, a.K)
    res = {'K': a.K, 'levels': len(levels)}
    for B in [int(b) for b in a.batches.split(',')]:
        pb = make_pockets(B, 'CA', ragged=True, first_index=7000)
        nl = pb.num_nodes_phar
        pm = np.repeat(np.arange(B), nl)
        com = np.stack([pb.x[pb.mask == b].mean(0) for b in range(B)])
        rng = np.random.default_rng(0)
        phx = torch.from_numpy((com[pm] + rng.normal(size=(len(pm), 3)) * 2.5).astype(np.float32)).cuda()
        phoh = torch.from_numpy(np.eye(8, dtype=np.float32)[rng.integers(0, 8, size=len(pm))]).cuda()
        px, poh = torch.from_numpy(pb.x).cuda(), torch.from_numpy(pb.one_hot).cuda()
        h.set_layout(nl, pb.size)
        runs = {'sample': lambda: h.sample_chain(px, poh, a.K, seed=1),
                'score': lambda: h.score_chain(phx, phoh, px, poh, levels, seed=1)}
        for f in runs.values():                 # warm-up: graph capture, buffers
            f()
        torch.cuda.synchronize()
        times = {k: [] for k in runs}
        edges = {}
        for _ in range(a.reps):
            for k, f in runs.items():
                c0 = h.counters()
                t0 = time.perf_counter()
                f()
                torch.cuda.synchronize()
                times[k].append(1e3 * (time.perf_counter() - t0))
                c1 = h.counters()              # the two chains evaluate different geometries: their edge lists differ in length
                edges[k] = (c1['edges'] - c0['edges']) / max(c1['evaluations'] - c0['evaluations'], 1) / B
        st = h.chain_status()
        for k, v in times.items():
            ms = float(np.median(v))
            res[f'b{B}_{k}_ms'] = round(ms, 2)
            res[f'b{B}_{k}_ms_per_eval'] = round(ms / (a.K + 1), 4)
            res[f'b{B}_{k}_edges_per_pocket_eval'] = round(edges[k], 1)
        res[f'b{B}_score_over_sample'] = round(res[f'b{B}_score_ms'] / res[f'b{B}_sample_ms'], 4)
        res[f'b{B}_score_status_clean'] = bool(st['max_rel_com_error'] < 1e-2 and st['nan_resets'] == 0)
        if B == int(a.batches.split(',')[0]) and a.host_K > 0:
            # the host loop: one eval-mode forward per level (each re-does the t = 0 pass), then the same levels on the device
            ddpm = host_loop_model(cfg, sd)
            dev = lambda v: torch.from_numpy(np.ascontiguousarray(v)).cuda()
            phar = {'x': phx, 'one_hot': phoh, 'size': dev(nl), 'mask': dev(pm)}
            pocket = {'x': px, 'one_hot': poh, 'size': dev(pb.size), 'mask': dev(pb.mask)}
            lv = scoring.level_list(cfg.timesteps, a.host_K)[:-1]

            def host_loop():
                tot = 0.0
                for t in lv:
                    terms = ddpm.forward(phar, pocket, t_int=torch.full((B, 1), float(t)))
                    tot = tot + terms[1]
                return tot
            host_loop()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            host_loop()
            torch.cuda.synchronize()
            host_ms = 1e3 * (time.perf_counter() - t0)
            ddpm.score(phar, pocket, timesteps=a.host_K, seed=1)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ddpm.score(phar, pocket, timesteps=a.host_K, seed=1)
            torch.cuda.synchronize()
            dev_ms = 1e3 * (time.perf_counter() - t0)
            res.update({'host_K': a.host_K, f'b{B}_host_loop_ms': round(host_ms, 2), f'b{B}_host_loop_ms_per_level': round(host_ms / a.host_K, 3),
                        f'b{B}_score_call_ms': round(dev_ms, 2), f'b{B}_host_loop_over_score_call': round(host_ms / dev_ms, 2)})
            h.set_layout(nl, pb.size)
    h.close()
    print(json.dumps(res))


if __name__ == '__main__':
    main()
