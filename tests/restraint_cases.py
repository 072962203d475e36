"""Cases, inputs and reference results of the restrained chain's tests (test_hip_restraint.py on the GPU, test_restraint_cpu.py without one).
The reference is restraint_ref.restrained_chain, live, fp32 on the CPU, computed once per case and shared - guided, and unguided (scale = 0)
on the same draws.

Inputs as multi_pocket_cases.py makes them: bounded_config(20, 1000), seed-0 weights, ragged C-alpha pockets of cmdgen_amd/synthetic.py, K = 5
ops on injected noise.  A sample with a pair within MARGIN of the radius graph's cutoff at any reference evaluation (guided or unguided) is left
out of a comparison; first_index is chosen so that at most CHAIN_CAP of a case's samples are - test_restraint_cpu.py asserts it.

SCALE and MAX_SHIFT: DESIGN.md, "Restrained sampling", says how they were picked."""
from collections import namedtuple

import numpy as np
import torch

import restraint_ref as rr
from multi_pocket_ref import MARGIN, CHAIN_CAP                    # noqa: F401  (1e-4 A, 0.20)
from bench import bounded_config
from cmdgen_amd import restraints as rs
from cmdgen_amd.synthetic import PocketBatch, make_pockets, make_state_dict
from oracle import ref_cpu

K = 5
SCALE = 1.0
MAX_SHIFT = rs.DEFAULT_MAX_SHIFT
CLASH = (3.0, 1.0)                # r_c in A (C-alpha atoms sit ~3.8 A apart), k_c
Case = namedtuple('Case', 'name nph first_index big_sample bare_sample')

# 8 samples of 1-8 points: every kind, sample 1 a single point (position and exclusion only), sample 4 without a restraint of its own
MIXED = Case('mixed', (4, 1, 8, 3, 6, 2, 7, 5), 9140, None, 4)
# one sample above 128 nodes: the 1024-thread step, its loops on their second trip
LARGE = Case('large', (8, 5, 3), 9200, 0, None)
CASES = {c.name: c for c in (MIXED, LARGE)}


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


def pockets(case):
    B = len(case.nph)
    pb = make_pockets(B, 'CA', ragged=True, first_index=case.first_index)
    xs, hs = np.split(pb.x, np.cumsum(pb.size)[:-1]), np.split(pb.one_hot, np.cumsum(pb.size)[:-1])
    if case.big_sample is not None:
        big = make_pockets(1, 'CA', n_pocket_nodes=140, radius=16.0, first_index=case.first_index + 500)
        xs[case.big_sample], hs[case.big_sample] = big.x, big.one_hot
    size = np.asarray([len(x) for x in xs], dtype=np.int64)
    return PocketBatch(x=np.concatenate(xs), one_hot=np.concatenate(hs), size=size, mask=np.repeat(np.arange(B, dtype=np.int64), size),
                       num_nodes_phar=np.asarray(case.nph, dtype=np.int64),
                       pocket_index=np.arange(case.first_index, case.first_index + B, dtype=np.int64))


def restraints_of(case, pb=None):
    """The case's list of restraint dicts: per sample (but the bare one) a position restraint on point 0, an exclusion sphere at the pocket's
    centre and, from two points on, a distance window between points 0 and 1; centres in the pocket's frame."""
    pb = pockets(case) if pb is None else pb
    rng = np.random.Generator(np.random.PCG64(case.first_index))
    out = []
    for b, nl in enumerate(case.nph):
        com = pb.x[pb.mask == b].mean(0)
        spot = com + rng.uniform(-3.0, 3.0, size=3)
        if b == case.bare_sample:
            continue
        out.append({'kind': 'position', 'sample': b, 'point': 0, 'center': tuple(float(v) for v in spot), 'radius': 1.5, 'k': 1.0})
        if nl >= 2:
            out.append({'kind': 'distance', 'sample': b, 'points': (0, 1), 'lo': 5.0, 'hi': 7.0, 'k': 1.0})
        out.append({'kind': 'exclusion', 'sample': b, 'center': tuple(float(v) for v in com), 'radius': 3.0, 'k': 0.5})
    return out


def noise_of(case):
    return torch.randn((K + 2, int(sum(case.nph)), 11), generator=torch.Generator().manual_seed(case.first_index))


def pocket_dict(pb):
    return {'x': torch.from_numpy(pb.x), 'one_hot': torch.from_numpy(pb.one_hot), 'size': torch.from_numpy(pb.size),
            'mask': torch.from_numpy(pb.mask)}


def run_ref(case, pb, rec, noise, scale, clash=CLASH, guide_below=1.0):
    tape = iter(noise)
    with torch.no_grad():
        return rr.restrained_chain(params(), config().as_dict(), pocket_dict(pb), case.nph, rec, clash_r=clash[0], clash_k=clash[1], scale=scale,
                                   max_shift=MAX_SHIFT, guide_below=guide_below, timesteps=K, noise=lambda shape: next(tape))


def reference(case):
    """dict(pb, restraints, rec, noise, guided, unguided (restraint_ref's dicts, scale = SCALE and 0), keep [B]) - computed once."""
    if case.name not in _REF:
        torch.set_num_threads(min(16, max(1, torch.get_num_threads())))
        pb, noise = pockets(case), noise_of(case)
        restraints = restraints_of(case, pb)
        rec = rs.records(restraints, case.nph)
        guided, unguided = run_ref(case, pb, rec, noise, SCALE), run_ref(case, pb, rec, noise, 0.0)
        keep = np.minimum(guided['margins'].min(axis=0), unguided['margins'].min(axis=0)) >= MARGIN
        _REF[case.name] = dict(pb=pb, restraints=restraints, rec=rec, noise=noise, guided=guided, unguided=unguided, keep=keep)
    return _REF[case.name]
