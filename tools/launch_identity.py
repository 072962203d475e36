#!/usr/bin/env python3
"""Which kernels a workload launches, with which grid, block and LDS size: the A/B of a change that must not move any of them.

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT/<side>/<workload> -- python3 tools/launch_identity.py run <workload> [--root TREE]
    python3 tools/launch_identity.py compare OUT/<sideA> OUT/<sideB>

Workloads: cond<B> (one eager K = 5 conditional chain on B ragged C-alpha pockets, tests/rule_sweep_ref.py's layouts), joint<B> (the joint
model's inpainting chain, K = 5, uniform 44 + 15 pockets), train_fp32 / train_bf16 (one HipTrainer.training_step on 64 complexes).
--root imports the package (and tools/bench_train.py) from another checkout with its own built library.  `compare` folds each trace into
(kernel name, grid, workgroup, LDS bytes, scratch bytes) -> launches and prints every workload's table, or the difference."""
import collections
import csv
import glob
import os
import sys

K = 5


def run(workload, root):
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(root, 'tools'))
    import numpy as np
    import torch
    import cmdgen_amd  # noqa: F401
    from cmdgen_amd import hip_backend
    from cmdgen_amd.synthetic import ModelConfig, make_pockets, make_state_dict
    d = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()  # noqa: E731
    if workload.startswith('train_'):
        import bench_train
        dev = torch.device('cuda', 0)
        cfg, model, tr = bench_train.build_trainer(64, 'CA', workload[6:], dev, pipelined=False)
        torch.manual_seed(0)
        print(workload, float(tr.training_step(bench_train.synthetic_batch(64, 50000, dev))['loss']))
        return
    joint = workload.startswith('joint')
    B = int(workload[5 if joint else 4:])
    cfg = ModelConfig(residue_nf=20, timesteps=1000, noise_precision=0.1, norm_values=(1.0, 0.25), update_pocket_coords=joint)    # bench.py's bounded_config
    h = hip_backend.Handle(cfg.as_dict(), 0)
    h.load_state_dict(make_state_dict(cfg, seed=0))
    pb = make_pockets(B, 'CA') if joint else make_pockets(B, 'CA', ragged=True, first_index=7000)
    h.set_layout(pb.num_nodes_phar, pb.size)
    if joint:
        Nl, Np = int(pb.num_nodes_phar.sum()), len(pb.mask)
        h.joint_chain(K, phar=(torch.zeros(Nl, 3).cuda(), torch.zeros(Nl, 8).cuda()), pocket=(d(pb.x), d(pb.one_hot)), phar_fixed=torch.zeros(Nl).cuda(),
                      pocket_fixed=torch.ones(Np).cuda(), seed=1, pocket_ids=pb.pocket_index, use_graph=False)
    else:
        h.sample_chain(d(pb.x), d(pb.one_hot), K, seed=1, use_graph=False)
    torch.cuda.synchronize()
    print(workload, h.chain_status(), {k: h.query(k) for k in ('node_mt', 'edge_mt', 'coord_mt', 'edge_grid', 'coord_grid', 'node64', 'node16w', 'proj_in_coord', 'e128_fused')})


def fold(side):
    out = {}
    for wl in sorted(os.listdir(side)):
        files = glob.glob(os.path.join(side, wl, '**', '*kernel_trace.csv'), recursive=True)
        assert len(files) == 1, (side, wl, files)
        c = collections.Counter()
        for r in csv.DictReader(open(files[0])):
            dim = lambda n: 'x'.join(r[n + '_' + a] for a in 'XYZ') if n + '_X' in r else r[n]  # noqa: E731  (older rocprofv3: one column)
            c[(r['Kernel_Name'], dim('Grid_Size'), dim('Workgroup_Size'), int(r.get('LDS_Block_Size', r.get('Group_Segment_Size', -1))),
               int(r.get('Scratch_Size', r.get('Private_Segment_Size', -1))))] += 1
        out[wl] = c
    return out


def compare(a, b):
    fa, fb = fold(a), fold(b)
    assert fa.keys() == fb.keys(), (sorted(fa), sorted(fb))
    same = True
    for wl in fa:
        ca, cb = fa[wl], fb[wl]
        print('--- %s: %d launches of %d (kernel, grid, workgroup, LDS, scratch) forms in %s, %d of %d in %s: %s'
              % (wl, sum(ca.values()), len(ca), a, sum(cb.values()), len(cb), b, 'IDENTICAL' if ca == cb else 'DIFFERENT'))
        for k in sorted(set(ca) | set(cb), key=lambda k: (k[0].startswith('void at::') or 'at::native' in k[0], k)):
            if ca[k] != cb[k]:
                same = False
                print('  DIFF %4d | %4d  grid %-14s wg %-9s LDS %6d scratch %4d  %s' % ((ca[k], cb[k]) + k[1:] + (k[0][:150],)))
            elif 'at::native' not in k[0] and 'rocprim' not in k[0]:
                print('  %4d  grid %-14s wg %-9s LDS %6d scratch %4d  %s' % ((ca[k],) + k[1:] + (k[0][:150],)))
    print('ALL IDENTICAL' if same else 'NOT IDENTICAL')
    return 0 if same else 1


if __name__ == '__main__':
    if sys.argv[1] == 'run':
        root = sys.argv[sys.argv.index('--root') + 1] if '--root' in sys.argv else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        run(sys.argv[2], os.path.abspath(root))
    else:
        sys.exit(compare(sys.argv[2], sys.argv[3]))
