#!/usr/bin/env python
"""Parent against change for the training step, one process per measurement so that two builds of the library can alternate on one device
(profiles/train_plan_refactor.txt).  TREE is a checkout with its library built (python __graft_entry__.py).
  ab_train_step.py grad TREE OUT.npz N      loss_and_grad on the batch of test_training_step_options_leave_the_gradient_where_it_is, fp32 and bf16
                                            operands, N calls each: losses and flat gradients
  ab_train_step.py time TREE TAG            bench.py's training-step record of TREE: one JSON line with train_ms_fp32 and train_ms_bf16_operands
  ab_train_step.py compare NEW.npz PARENT.npz PARENT.npz [...]
                                            tensor by tensor, NEW against the parent runs, with the parents' own run-to-run difference as the yardstick
                                            (the first two parent files alone, and all of them)"""
import json
import os
import sys


def grad(tree, out, nruns):
    tree = os.path.abspath(tree)
    from argparse import Namespace

    sys.path.insert(0, tree)
    sys.path.insert(0, os.path.join(tree, 'tools'))
    import numpy as np
    import torch
    import cmdgen_amd
    assert os.path.abspath(cmdgen_amd.__file__).startswith(tree), cmdgen_amd.__file__
    from cmdgen_amd.lightning_modules import PharPocketDDPM
    from cmdgen_amd.training import HipTrainer
    from cmdgen_amd.synthetic import ModelConfig, make_state_dict
    import bench_train as bt

    L = 2
    cfg = ModelConfig(n_layers=L)
    hp = dict(outdir='out', dataset='crossdock', datadir='data', batch_size=24, lr=1e-3,
              egnn_params=Namespace(device='cuda', edge_cutoff=6.0, joint_nf=32, hidden_nf=256, n_layers=L, attention=True, tanh=True,
                                    norm_constant=1, inv_sublayers=1, sin_embedding=False, aggregation_method='sum', normalization_factor=100),
              diffusion_params=Namespace(diffusion_steps=500, diffusion_noise_schedule='polynomial_2', diffusion_noise_precision=1e-5,
                                         diffusion_loss_type='l2', normalize_factors=[1, 4]),
              num_workers=0, augment_noise=0, augment_rotation=False, clip_grad=True, eval_epochs=50,
              eval_params=Namespace(n_eval_samples=100, eval_batch_size=100), mode='pocket_conditioning',
              node_histogram=np.ones((30, 500)), pocket_representation='CA')
    res = {}
    for gemm in ('fp32', 'bf16'):
        model = PharPocketDDPM(**hp)
        model.load_state_dict({k: torch.from_numpy(v) for k, v in make_state_dict(cfg, seed=0).items()}, strict=True)
        tr = HipTrainer(model.cuda(), gemm_dtype=gemm)
        batch = bt.synthetic_batch(24, 7300, torch.device('cuda', 0))
        gen = torch.Generator().manual_seed(14)
        t_int = torch.randint(0, 501, (24, 1), generator=gen).float()
        eps = [torch.randn((int(batch['num_phar_atoms'].sum()), 11), generator=gen).cuda()]
        for r in range(nruns):
            loss, _, _ = tr.loss_and_grad(batch, t_int=t_int, eps=eps)
            torch.cuda.synchronize()
            res[f'{gemm}_loss_{r}'] = np.array(float(loss), dtype=np.float64)
            res[f'{gemm}_grad_{r}'] = tr.grad.detach().cpu().numpy().copy()
        if gemm == 'fp32':
            names, offs = [], []
            for name, p in tr.dyn.named_parameters():
                off, cnt = tr.h.param_offset(name)
                names.append(name); offs.append((off, cnt))
            res['names'] = np.array(names); res['offs'] = np.array(offs, dtype=np.int64)
        del tr, model
    np.savez(out, **res)
    print('wrote', out)


def time(tree, tag):
    tree = os.path.abspath(tree)

    os.chdir(tree)
    sys.path.insert(0, tree)
    import torch
    import cmdgen_amd
    assert os.path.abspath(cmdgen_amd.__file__).startswith(tree), cmdgen_amd.__file__
    import bench
    assert os.path.abspath(bench.__file__).startswith(tree), bench.__file__

    dev = torch.device('cuda', 0)
    stream = torch.cuda.Stream(dev)
    with torch.cuda.stream(stream):
        ts = bench.training_step_record(dev)
    print(json.dumps({'build': tag, 'train_ms_fp32': round(ts['fp32_results']['ms_per_step'], 3),
                      'train_ms_bf16_operands': round(ts['bf16_gemm_operands']['ms_per_step'], 3),
                      'launches_per_step': ts['fp32_results'].get('launches_per_step')}), flush=True)


def compare(new, parents):
    import numpy as np

    nw = np.load(new)
    par = [np.load(f) for f in parents]
    pa, pb = par[0], par[1]
    names, offs = pa['names'], pa['offs']
    ok_loss = True
    for gemm in ('fp32', 'bf16'):
        for r in (0, 1):
            if f'{gemm}_loss_{r}' not in pa.files:
                continue
            lp = [float(z[f'{gemm}_loss_{r}']) for z in par]
            ln = float(nw[f'{gemm}_loss_{r}'])
            print(f'[{gemm}, call {r} of the process] loss: parent runs {lp}  this build {ln!r}  parent runs identical: {len(set(lp)) == 1}  this build identical: {ln == lp[0]}')
            ok_loss = ok_loss and (ln == lp[0] or len(set(lp)) > 1)
            gp = [z[f'{gemm}_grad_{r}'] for z in par]
            gn = nw[f'{gemm}_grad_{r}']
            two_det = two_det_same = two_noisy = two_within = 0
            cl_det = cl_det_same = cl_noisy = cl_within = 0
            worst = (0.0, '')
            for name, (off, cnt) in zip(names, offs):
                p = [g[off:off + cnt] for g in gp]
                n = gn[off:off + cnt]
                scale = max(float(np.abs(p[0]).max()), 1e-30)
                # the issue's check: this build against a parent run, no more than the parent's two runs differ
                d_par2 = float(np.abs(p[0] - p[1]).max())
                d_new2 = min(float(np.abs(n - p[0]).max()), float(np.abs(n - p[1]).max()))
                if d_par2 == 0.0:
                    two_det += 1; two_det_same += d_new2 == 0.0
                else:
                    two_noisy += 1; two_within += d_new2 <= d_par2
                # against all parent runs: the nearest parent run, against the widest pair of parent runs
                d_par = max(float(np.abs(p[i] - p[j]).max()) for i in range(len(p)) for j in range(i))
                d_new = min(float(np.abs(n - q).max()) for q in p)
                if d_par == 0.0:
                    cl_det += 1; cl_det_same += d_new == 0.0
                    if d_new != 0.0:
                        print(f'   identical in all {len(p)} parent runs, differs here: {name} {d_new:.3e} (scale {scale:.3e})')
                else:
                    cl_noisy += 1; cl_within += d_new <= d_par
                    if d_new / d_par > worst[0]:
                        worst = (d_new / d_par, f'{name}: parent {d_par:.3e} this build {d_new:.3e} scale {scale:.3e} (this build, relative: {d_new / scale:.2e})')
            print(f'   two parent runs: {len(names)} tensors; identical in both {two_det}, of those identical here {two_det_same}; differing {two_noisy}, of those this build within their difference {two_within}')
            print(f'   {len(p)} parent runs: identical in all {cl_det}, of those identical here {cl_det_same}; differing {cl_noisy}, of those this build within the widest parent pair {cl_within}')
            print(f'   largest (this build - nearest parent run) / (widest parent pair): {worst[0]:.2f}  {worst[1]}')
    print('loss identical wherever the parent runs agree:', ok_loss)


if __name__ == '__main__':
    cmd, args = sys.argv[1], sys.argv[2:]
    if cmd == 'grad':
        grad(args[0], args[1], int(args[2]))
    elif cmd == 'time':
        time(args[0], args[1])
    elif cmd == 'compare':
        compare(args[0], args[1:])
    else:
        sys.exit(__doc__)
