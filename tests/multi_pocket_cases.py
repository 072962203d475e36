"""Cases, inputs and reference results of the multi-pocket chain tests (test_hip_multi_pocket.py on the GPU, test_multi_pocket_cpu.py
without one).  The reference is multi_pocket_ref.multi_pocket_chain, live, fp32 on the CPU, computed once per case and shared.

Inputs: ragged C-alpha pockets of cmdgen_amd/synthetic.py, a different one for every member (each drawn round the origin, so the pockets
of a group overlap in one common frame), 1-8 phar points per group, non-uniform weights, K = 5 steps on injected noise.  A group with a
pair within multi_pocket_ref.MARGIN of the radius graph's cutoff at any reference evaluation is left out of a comparison (the graph is a
hard threshold); first_index below is chosen so that at most CHAIN_CAP of a case's groups are - test_multi_pocket_cpu.py asserts it."""
from collections import namedtuple

import numpy as np
import torch

import multi_pocket_ref as mp
from bench import bounded_config
from cmdgen_amd.synthetic import PocketBatch, make_pockets, make_state_dict
from oracle import ref_cpu

K = 5
Case = namedtuple('Case', 'name group_sizes nph first_index big_member')

# groups of 1, 2 and 3 members in one batch (the ragged C-level case), one group with a single phar point
MIXED = Case('mixed', (1, 2, 3, 2, 1, 3, 2, 1, 2, 3), (4, 1, 8, 3, 6, 2, 7, 5, 8, 3), 9100, None)
# one member above 128 nodes: the 1024-thread step, its loops on their second trip
LARGE = Case('large', (2, 1, 2), (8, 5, 3), 9200, 0)
# M = 2 everywhere: the other engines, captured against eager, run to run
PAIRS = Case('pairs', (2, 2, 2), (6, 3, 8), 9300, None)
CASES = {c.name: c for c in (MIXED, LARGE, PAIRS)}


def config():
    return bounded_config(20, 1000)


_SD, _PARAMS, _REF = [], [], {}


def state_dict():
    if not _SD:
        _SD.append(make_state_dict(config(), seed=0))
    return _SD[0]


def params():
    if not _PARAMS:
        _PARAMS.append(ref_cpu.to_torch_params(state_dict()))
    return _PARAMS[0]


def member_pockets(case):
    """PocketBatch of the B member samples (num_nodes_phar: the group's count on every member)."""
    B = int(sum(case.group_sizes))
    pb = make_pockets(B, 'CA', ragged=True, first_index=case.first_index)
    xs, hs = np.split(pb.x, np.cumsum(pb.size)[:-1]), np.split(pb.one_hot, np.cumsum(pb.size)[:-1])
    if case.big_member is not None:
        big = make_pockets(1, 'CA', n_pocket_nodes=140, radius=16.0, first_index=case.first_index + 500)
        xs[case.big_member], hs[case.big_member] = big.x, big.one_hot
    size = np.asarray([len(x) for x in xs], dtype=np.int64)
    return PocketBatch(x=np.concatenate(xs), one_hot=np.concatenate(hs), size=size, mask=np.repeat(np.arange(B, dtype=np.int64), size),
                       num_nodes_phar=np.repeat(np.asarray(case.nph, dtype=np.int64), case.group_sizes),
                       pocket_index=np.arange(case.first_index, case.first_index + B, dtype=np.int64))


def weights_of(case):
    """[B] float32, non-uniform, every group's normalised in float64."""
    rng = np.random.Generator(np.random.PCG64(case.first_index))
    out = []
    for m in case.group_sizes:
        w = rng.uniform(0.2, 1.0, size=m)
        out.append((w / w.sum()).astype(np.float32))
    return np.concatenate(out)


def noise_of(case):
    return torch.randn((K + 2, int(sum(case.nph)), 11), generator=torch.Generator().manual_seed(case.first_index))


def pocket_dict(pb):
    return {'x': torch.from_numpy(pb.x), 'one_hot': torch.from_numpy(pb.one_hot), 'size': torch.from_numpy(pb.size),
            'mask': torch.from_numpy(pb.mask)}


def reference(case):
    """dict(pb, weights, noise, groups, want, want_pocket, z_steps, pocket_steps, margins [K + 1, B], keep [G]) - computed once."""
    if case.name not in _REF:
        torch.set_num_threads(min(16, max(1, torch.get_num_threads())))
        pb, w, noise = member_pockets(case), weights_of(case), noise_of(case)
        tape = iter(noise)
        with torch.no_grad():
            want, want_p, um, _, zs, ps, margins = mp.multi_pocket_chain(
                params(), config().as_dict(), pocket_dict(pb), case.group_sizes, case.nph, w, timesteps=K,
                noise=lambda shape: next(tape), return_steps=True)
        groups = mp.Groups(case.group_sizes, case.nph)
        _REF[case.name] = dict(pb=pb, weights=w, noise=noise, groups=groups, want=want.numpy(), want_pocket=want_p.numpy(),
                               z_steps=zs.numpy(), pocket_steps=ps.numpy(), margins=margins, keep=mp.kept_groups(margins, groups),
                               unique_mask=um.numpy())
    return _REF[case.name]
