#!/usr/bin/env python3
"""Cost of the input gradients: forward + cmdgen_train_backward_inputs against forward + cmdgen_train_backward at the training
benchmark's size (tools/bench_train.py: 64 C-alpha complexes, shipped hyper-parameters), same handle, same batch, alternating
blocks of repetitions.  Prints one JSON line (ms per forward + backward, median over the blocks).

    python tools/bench_backward_inputs.py [--batch 64] [--reps 20] [--blocks 5]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bench_train as bt  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--blocks', type=int, default=5)
    a = ap.parse_args()
    dev = torch.device('cuda', 0)
    cfg, model, tr = bt.build_trainer(a.batch, 'CA', 'fp32', dev, pipelined=False)
    batch = bt.synthetic_batch(a.batch, 9100, dev)
    tr.loss_and_grad(batch)                     # sets the layout and sizes every buffer
    h, fused = tr.h, tr._last_fused
    z, q, t = fused['z_t'], fused['xh_pocket'], fused['tab'][10].contiguous()
    d_eps = fused['d_eps']
    grad = torch.zeros_like(tr.theta)
    dxp, dxq, dt = torch.empty_like(z), torch.empty_like(q), torch.empty_like(t)

    def plain():
        h.train_forward(tr.theta, z, q, t)
        h.train_backward(d_eps, grad)

    def inputs():
        h.train_forward(tr.theta, z, q, t)
        h.train_backward_inputs(d_eps, grad, None, dxp, dxq, dt)

    def timed(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.reps

    res = {'plain': [], 'inputs': []}
    for _ in range(a.blocks):
        res['plain'].append(timed(plain))
        res['inputs'].append(timed(inputs))
    med = {k: float(np.median(v)) for k, v in res.items()}
    print(json.dumps({'metric': 'forward_plus_backward_ms', 'batch': a.batch,
                      'plain_ms': med['plain'], 'inputs_ms': med['inputs'], 'ratio': med['inputs'] / med['plain'],
                      'blocks': {k: [round(x, 4) for x in v] for k, v in res.items()}}))


if __name__ == '__main__':
    main()
