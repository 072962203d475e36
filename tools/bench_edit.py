#!/usr/bin/env python3
"""Cost of the column-group merge: one inpainting or one edit chain at the benchmark's size (bench.py: 64 C-alpha pockets, the
bounded model, K = 1000 steps, graph mode), a quarter of each sample's rows marked.  Prints one JSON line (seconds per chain:
every repetition and their mean).  For an A/B record run it in alternation from two checkouts (--tree imports the package of
another one, e.g. the parent commit's, which has no edit chain: --chain inpaint only):

    python tools/bench_edit.py --chain inpaint [--tree ../parent] [--batch 64] [--timesteps 1000] [--reps 3]
    python tools/bench_edit.py --chain edit          # types-only marks
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--chain', choices=['inpaint', 'edit'], required=True)
    ap.add_argument('--tree', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    help='checkout whose cmdgen_amd (and bench.py) is measured; default: this one')
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--timesteps', type=int, default=1000)
    ap.add_argument('--reps', type=int, default=3)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    from bench import bounded_config
    from cmdgen_amd import hip_backend
    from cmdgen_amd.synthetic import make_state_dict, make_pockets

    dev = torch.device('cuda', 0)
    K = a.timesteps
    cfg = bounded_config(20, K)
    h = hip_backend.Handle(cfg.as_dict(), 0)
    h.load_state_dict(make_state_dict(cfg, seed=0))
    pb = make_pockets(a.batch, 'CA', n_phar=15)
    h.set_layout(pb.num_nodes_phar, pb.size)
    nl = pb.num_nodes_phar
    pm = np.repeat(np.arange(len(nl)), nl)
    rng = np.random.default_rng(1)
    com = np.stack([pb.x[pb.mask == b].mean(0) for b in range(len(nl))])
    to = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dev)
    phar_x = to(com[pm] + rng.normal(size=(len(pm), 3)) * 2.5)
    phar_oh = to(np.eye(cfg.phar_nf)[rng.integers(0, cfg.phar_nf, size=len(pm))])
    first = np.concatenate([[0], np.cumsum(nl)[:-1]])
    marked = to((np.arange(len(pm)) - first[pm]) < np.maximum(1, nl[pm] // 4))
    px, poh = to(pb.x), to(pb.one_hot)
    if a.chain == 'inpaint':
        run = lambda seed: h.inpaint_chain(px, poh, phar_x, phar_oh, marked, K, seed=seed, use_graph=True)
    else:
        run = lambda seed: h.edit_chain(px, poh, phar_x, phar_oh, torch.zeros_like(marked), marked, K, seed=seed, use_graph=True)
    run(0)                                   # prepares the slot and captures the graph
    torch.cuda.synchronize()
    secs = []
    for r in range(a.reps):
        t0 = time.perf_counter()
        run(1 + r)
        torch.cuda.synchronize()
        secs.append(time.perf_counter() - t0)
    st = h.chain_status()
    print(json.dumps({'metric': 'seconds_per_chain', 'chain': a.chain, 'tree': os.path.abspath(a.tree), 'batch': a.batch, 'timesteps': K,
                      'marked_rows': int(marked.sum().item()), 'phar_rows': int(len(pm)), 'seconds': [round(s, 5) for s in secs],
                      'mean_s': float(np.mean(secs)), 'nan_resets': int(st['nan_resets'])}))


if __name__ == '__main__':
    main()
