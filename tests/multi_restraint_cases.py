"""Cases, inputs and reference results of the restrained multi-pocket chain's tests (test_hip_multi_restraint.py on the GPU,
test_multi_restraint_cpu.py without one).  The reference is multi_restraint_ref.multi_restrained_chain, live, fp32 on the CPU, computed once
per case and shared - guided, and unguided (scale = 0) on the same draws.

Inputs as multi_pocket_cases.py makes them: bounded_config(20, 1000), seed-0 weights, ragged C-alpha pockets of cmdgen_amd/synthetic.py, a
different one for every member (each drawn round the origin, so the pockets of a group overlap in one common frame), non-uniform weights,
K = 5 ops on injected noise [K + 2][Nu][11].  The restraints follow restraint_cases.py, per GROUP: a position restraint on point 0, an
exclusion sphere and, from two points on, a distance window; centres in the common frame; the clash term against every member's atoms.

A group with a pair within MARGIN of the radius graph's cutoff at any reference evaluation (guided or unguided) is left out of a comparison.
first_index, the centres and the windows below were chosen here, on the CPU, so that the reference alone leaves out at most CHAIN_CAP of a
case's groups and the guidance bites (a clipped and an unclipped displacement, a clash term from a member other than the first) -
test_multi_restraint_cpu.py asserts both."""
from collections import namedtuple

import numpy as np
import torch

import multi_pocket_cases as mc
import multi_restraint_ref as mr
from multi_restraint_ref import MARGIN, CHAIN_CAP                 # noqa: F401  (1e-4 A, 0.20)
from cmdgen_amd import restraints as rs

K = mc.K
SCALE = 1.0
MAX_SHIFT = rs.DEFAULT_MAX_SHIFT
CLASH = (3.0, 1.0)                # r_c in A (C-alpha atoms sit ~3.8 A apart), k_c
Case = namedtuple('Case', 'name group_sizes nph first_index big_member bare_group')

# groups of 1, 2 and 3 members, group 1 a single point (position and exclusion only), group 4 without a record of its own
MIXED = Case('mixed', (1, 2, 3, 2, 1, 3, 2, 1, 2, 3), (4, 1, 8, 3, 6, 2, 7, 5, 8, 3), 9100, None, 4)
# one member above 128 nodes: the 1024-thread path, its loops on their second trip
LARGE = Case('large', (2, 1, 2), (8, 5, 3), 9200, 0, None)
# M = 2 everywhere: the other engines, the effect
PAIRS = Case('pairs', (2, 2, 2), (6, 3, 8), 9300, None, None)
CASES = {c.name: c for c in (MIXED, LARGE, PAIRS)}

config, state_dict, params, pocket_dict = mc.config, mc.state_dict, mc.params, mc.pocket_dict
member_pockets, weights_of, noise_of = mc.member_pockets, mc.weights_of, mc.noise_of
_REF = {}


def restraints_of(case, pb=None):
    """The case's list of restraint dicts, 'sample' the GROUP: per group (but the bare one) a position restraint on point 0 near the centre
    of the group's first pocket, an exclusion sphere at the centre of all its pockets and, from two points on, a distance window between
    points 0 and 1."""
    pb = member_pockets(case) if pb is None else pb
    gr = mr.Groups(case.group_sizes, case.nph)
    rng = np.random.Generator(np.random.PCG64(case.first_index))
    out = []
    for g, nl in enumerate(case.nph):
        members = np.arange(gr.first[g], gr.first[g] + gr.sizes[g])
        com_first = pb.x[pb.mask == members[0]].mean(0)
        com_all = pb.x[np.isin(pb.mask, members)].mean(0)
        spot = com_first + rng.uniform(-3.0, 3.0, size=3)
        if g == case.bare_group:
            continue
        out.append({'kind': 'position', 'sample': g, 'point': 0, 'center': tuple(float(v) for v in spot), 'radius': 1.5, 'k': 1.0})
        if nl >= 2:
            out.append({'kind': 'distance', 'sample': g, 'points': (0, 1), 'lo': 5.0, 'hi': 7.0, 'k': 1.0})
        out.append({'kind': 'exclusion', 'sample': g, 'center': tuple(float(v) for v in com_all), 'radius': 3.0, 'k': 0.5})
    return out


def run_ref(case, pb, w, rec, noise, scale, clash=CLASH, guide_below=1.0):
    tape = iter(noise)
    with torch.no_grad():
        return mr.multi_restrained_chain(params(), config().as_dict(), pocket_dict(pb), case.group_sizes, case.nph, w, rec, clash_r=clash[0],
                                         clash_k=clash[1], scale=scale, max_shift=MAX_SHIFT, guide_below=guide_below, timesteps=K,
                                         noise=lambda shape: next(tape))


def reference(case):
    """dict(pb, weights, restraints, rec, noise, groups, guided, unguided (multi_restraint_ref's dicts, scale = SCALE and 0), keep [G]) -
    computed once."""
    if case.name not in _REF:
        torch.set_num_threads(min(16, max(1, torch.get_num_threads())))
        pb, w, noise = member_pockets(case), weights_of(case), noise_of(case)
        restraints = restraints_of(case, pb)
        rec = rs.records(restraints, case.nph)
        groups = mr.Groups(case.group_sizes, case.nph)
        guided, unguided = run_ref(case, pb, w, rec, noise, SCALE), run_ref(case, pb, w, rec, noise, 0.0)
        keep = mr.kept_groups(guided['margins'], groups) & mr.kept_groups(unguided['margins'], groups)
        _REF[case.name] = dict(pb=pb, weights=w, restraints=restraints, rec=rec, noise=noise, groups=groups, guided=guided, unguided=unguided,
                               keep=keep)
    return _REF[case.name]
