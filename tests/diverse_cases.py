"""Cases, inputs and reference results of the diverse chain's tests (test_hip_diverse.py on the GPU, test_diverse_cpu.py without one).  The
reference is diverse_ref.diverse_chain, live, fp32 on the CPU, computed once per case and run and shared - guided, and unguided (strength = 0)
on the same draws.

Inputs as restraint_cases.py makes them: bounded_config(20, 1000), seed-0 weights, ragged C-alpha pockets of cmdgen_amd/synthetic.py - ONE pocket
per set, repeated for every member of the set ("the draws for one pocket") - and injected noise.

Leave-out rule.  The term couples the members of a set, so a set with ANY member within MARGIN of the radius graph's cutoff, at any evaluation of
the guided or the unguided reference, is left out whole.  At most CHAIN_CAP of a case's sets may be left out, and none is for the committed
inputs: first_index is chosen that way, and test_diverse_cpu.py asserts both."""
from collections import namedtuple

import numpy as np
import torch

import diverse_ref as dr
from chain_ref import CHAIN_CAP, MARGIN                            # noqa: F401  (0.20, 1e-4 A)
from bench import bounded_config
from cmdgen_amd.synthetic import PocketBatch, make_pockets, make_state_dict
from oracle import ref_cpu

STRENGTH, WIDTH, MAX_SHIFT = 1.0, 2.0, 1.0
CLIP_SHIFT = 0.02                 # the max_shift of the run that exercises the clip
Case = namedtuple('Case', 'name sets nph K first_index big_set')

# four sets, one of a single member; members of a set with different numbers of points, one of them a single point
MIXED = Case('mixed', (4, 1, 3, 2), (4, 6, 3, 5, 2, 8, 1, 7, 5, 5), 5, 9350, None)
# set 0 on a pocket of 140 nodes: samples 0 and 1 have 148 and 145 nodes and the 1024-thread step runs
LARGE = Case('large', (2, 2), (8, 5, 3, 4), 5, 9440, 0)
# set 0 has 288 rows: more than the pair kernel's tile of 256 rows, so its loop takes a second trip
WIDE = Case('wide', (36, 1), (8,) * 36 + (3,), 2, 9730, None)
CASES = {c.name: c for c in (MIXED, LARGE, WIDE)}


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
    """One pocket per set, repeated set_size times; pocket_index = first_index + arange(B)."""
    S, B = len(case.sets), int(sum(case.sets))
    pb = make_pockets(S, 'CA', ragged=True, first_index=case.first_index)
    xs, hs = np.split(pb.x, np.cumsum(pb.size)[:-1]), np.split(pb.one_hot, np.cumsum(pb.size)[:-1])
    if case.big_set is not None:
        big = make_pockets(1, 'CA', n_pocket_nodes=140, radius=16.0, first_index=case.first_index + 500)
        xs[case.big_set], hs[case.big_set] = big.x, big.one_hot
    set_of = np.repeat(np.arange(S), case.sets)
    xs, hs = [xs[s] for s in set_of], [hs[s] for s in set_of]
    size = np.asarray([len(x) for x in xs], dtype=np.int64)
    return PocketBatch(x=np.concatenate(xs), one_hot=np.concatenate(hs), size=size, mask=np.repeat(np.arange(B, dtype=np.int64), size),
                       num_nodes_phar=np.asarray(case.nph, dtype=np.int64),
                       pocket_index=np.arange(case.first_index, case.first_index + B, dtype=np.int64))


def noise_of(case):
    return torch.randn((case.K + 2, int(sum(case.nph)), 11), generator=torch.Generator().manual_seed(case.first_index))


def pocket_dict(pb):
    return {'x': torch.from_numpy(pb.x), 'one_hot': torch.from_numpy(pb.one_hot), 'size': torch.from_numpy(pb.size),
            'mask': torch.from_numpy(pb.mask)}


def run_ref(case, pb, noise, strength=STRENGTH, max_shift=MAX_SHIFT, guide_below=1.0, sets=None):
    tape = iter(noise)
    with torch.no_grad():
        return dr.diverse_chain(params(), config().as_dict(), pocket_dict(pb), case.nph, case.sets if sets is None else sets, strength=strength,
                                width=WIDTH, max_shift=max_shift, guide_below=guide_below, timesteps=case.K, noise=lambda shape: next(tape))


def kept_sets(case, *runs):
    """[S] bool: the sets none of whose members has a pair within MARGIN of the cutoff at any evaluation of any of the runs."""
    ok = np.minimum.reduce([r['margins'].min(axis=0) for r in runs]) >= MARGIN
    first = np.concatenate([[0], np.cumsum(case.sets)[:-1]])
    return np.array([ok[f:f + m].all() for f, m in zip(first, case.sets)])


def reference(case, clipped=False):
    """dict(pb, noise, guided, unguided (diverse_ref's dicts, strength = STRENGTH and 0), keep [S], keep_samples [B]) - computed once.
    clipped: the guided run with max_shift = CLIP_SHIFT."""
    key = (case.name, clipped)
    if key not in _REF:
        torch.set_num_threads(min(16, max(1, torch.get_num_threads())))
        if clipped:
            base = reference(case)
            pb, noise, unguided = base['pb'], base['noise'], base['unguided']
            guided = run_ref(case, pb, noise, max_shift=CLIP_SHIFT)
        else:
            pb, noise = pockets(case), noise_of(case)
            guided, unguided = run_ref(case, pb, noise), run_ref(case, pb, noise, strength=0.0)
        keep = kept_sets(case, guided, unguided)
        _REF[key] = dict(pb=pb, noise=noise, guided=guided, unguided=unguided, keep=keep, keep_samples=np.repeat(keep, case.sets))
    return _REF[key]
