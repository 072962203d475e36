"""Cases, inputs and reference results of the restrained edit chain's tests (test_hip_restrained_edit.py on the GPU,
test_restrained_edit_cpu.py without one).  The reference is restrained_edit_ref.restrained_edit, live, fp32 on the CPU, computed once per case
and shared - guided, and unguided (scale = 0) on the same draws.

Inputs in the style of restraint_cases.py: bounded_config(20, 1000), seed-0 weights, ragged C-alpha pockets of cmdgen_amd/synthetic.py, injected
noise; the given points lie round the pocket's centre.  A sample with a pair within MARGIN of the radius graph's cutoff at any reference
evaluation (guided or unguided) is left out of a comparison; first_index is chosen on the CPU so that at most CHAIN_CAP of a case's samples are
- test_restrained_edit_cpu.py asserts it on the reference alone.

Marks: per sample the first ceil(n / 2) points have x and types held ('b'), except sample 2 (no mark) and sample 3 (types only, 'h').  The
smallest shapes that reach every branch: a single-point sample (its only point held), a pocket of more atoms than the 64 lanes that walk them,
a sample above 128 nodes (the 1024-thread step), samples that merge and one that does not, ops that jump back."""
import math
from collections import namedtuple

import numpy as np
import torch

import restrained_edit_ref as rer
import restraint_cases as rc
from edit_ref import edit_plan
from multi_pocket_ref import MARGIN, CHAIN_CAP                    # noqa: F401  (1e-4 A, 0.20)
from cmdgen_amd import restraints as rs

SCALE = rc.SCALE
MAX_SHIFT = rc.MAX_SHIFT
CLASH = (3.0, 1.0)
Case = namedtuple('Case', 'name nph first_index big_sample K start r j no_mark types_only bare')

NPH = (4, 1, 8, 3, 6, 2, 7, 5)
# 8 samples, from the prior, no jumps: sample 1 a single (held) point, 2 without a mark, 3 with types held only, 4 without a restraint of its own
MIXED = Case('mixed', NPH, 9300, None, 6, 6, 1, 1, 2, 3, 4)
# the same batch part-way (k_edit_start) with resampling and jumps back (op C)
JUMPS = Case('jumps', NPH, 9300, None, 6, 4, 2, 2, 2, 3, 4)
# one sample above 128 nodes (a 140-atom pocket): the 1024-thread step, the pocket loops on their third trip; sample 1 without a mark
LARGE = Case('large', (8, 5, 3), 9400, 0, 5, 5, 1, 1, 1, None, None)
CASES = {c.name: c for c in (MIXED, JUMPS, LARGE)}
# the samples of MIXED on which the guided reference must end with less energy than the unguided one (same draws): every restrained sample
# with a free point - sample 1 has none, sample 4 only the clash term (it has free points and stays in)
EFFECT_SAMPLES = (0, 2, 3, 4, 5, 6, 7)

config, state_dict, params, pocket_dict = rc.config, rc.state_dict, rc.params, rc.pocket_dict


def pockets(case):
    return rc.pockets(rc.Case(case.name, case.nph, case.first_index, case.big_sample, None))


def marks(case):
    """(fix_x, fix_h) float32 [Nl]."""
    fx, fh = [], []
    for b, n in enumerate(case.nph):
        held = np.arange(n) < math.ceil(n / 2)
        fx.append(held & (b != case.no_mark) & (b != case.types_only))
        fh.append(held & (b != case.no_mark))
    return np.concatenate(fx).astype(np.float32), np.concatenate(fh).astype(np.float32)


def phar_dict(case, pb=None):
    """The given rows: points within a few A of the pocket's centre, in the pocket's frame."""
    pb = pockets(case) if pb is None else pb
    rng = np.random.Generator(np.random.PCG64(case.first_index + 1))
    nph = np.asarray(case.nph, dtype=np.int64)
    pm = np.repeat(np.arange(len(nph)), nph)
    com = np.stack([pb.x[pb.mask == b].mean(0) for b in range(len(nph))])
    x = (com[pm] + rng.normal(size=(len(pm), 3)) * 2.5).astype(np.float32)
    oh = np.eye(8, dtype=np.float32)[rng.integers(0, 8, size=len(pm))]
    return {'x': torch.from_numpy(x), 'one_hot': torch.from_numpy(oh), 'size': torch.from_numpy(nph), 'mask': torch.from_numpy(pm)}


def restraints_of(case, pb=None):
    """Per sample (but the bare one): a position restraint on its first free point, a distance window between point 0 (held, where the sample
    holds x) and its last free point, an exclusion sphere at the pocket's centre; centres in the pocket's frame."""
    pb = pockets(case) if pb is None else pb
    rng = np.random.Generator(np.random.PCG64(case.first_index))
    fx = np.split(marks(case)[0], np.cumsum(case.nph)[:-1])
    out = []
    for b, nl in enumerate(case.nph):
        com = pb.x[pb.mask == b].mean(0)
        spot = com + rng.uniform(-3.0, 3.0, size=3)
        if b == case.bare:
            continue
        free = [i for i in range(nl) if fx[b][i] == 0]
        if free:
            out.append({'kind': 'position', 'sample': b, 'point': free[0], 'center': tuple(float(v) for v in spot), 'radius': 1.5, 'k': 1.0})
            if free[-1] != 0:
                out.append({'kind': 'distance', 'sample': b, 'points': (0, free[-1]), 'lo': 5.0, 'hi': 7.0, 'k': 1.0})
        out.append({'kind': 'exclusion', 'sample': b, 'center': tuple(float(v) for v in com), 'radius': 3.0, 'k': 0.5})
    return out


def plan(case):
    """(n_steps, n_draws, n_jumps)"""
    return edit_plan(case.r, case.j, case.K, case.start)


def noise_of(case):
    return torch.randn((plan(case)[1], int(sum(case.nph)), 11), generator=torch.Generator().manual_seed(case.first_index + 7 * case.start))


def run_ref(case, pb, rec, noise, scale, clash=CLASH, guide_below=1.0, marked=True, probe=None, **over):
    tape = iter(noise)
    fx, fh = marks(case)
    if not marked:
        fx, fh = np.zeros_like(fx), np.zeros_like(fh)
    kw = dict(start=case.start, resamplings=case.r, jump_length=case.j, timesteps=case.K)
    kw.update(over)
    with torch.no_grad():
        out = rer.restrained_edit(params(), config().as_dict(), phar_dict(case, pb), pocket_dict(pb), fx, fh, rec, clash_r=clash[0],
                                  clash_k=clash[1], scale=scale, max_shift=MAX_SHIFT, guide_below=guide_below,
                                  noise=lambda shape: next(tape), probe=probe, **kw)
    assert next(tape, None) is None                      # every planned draw was used
    return out


_REF = {}


def reference(case):
    """dict(pb, phar, fx, fh, restraints, rec, noise, guided, unguided (restrained_edit_ref's dicts, scale = SCALE and 0), keep [B]) - computed
    once."""
    if case.name not in _REF:
        torch.set_num_threads(min(16, max(1, torch.get_num_threads())))
        pb, noise = pockets(case), noise_of(case)
        restraints = restraints_of(case, pb)
        rec = rs.records(restraints, case.nph)
        guided, unguided = run_ref(case, pb, rec, noise, SCALE), run_ref(case, pb, rec, noise, 0.0)
        keep = np.minimum(guided['margins'].min(axis=0), unguided['margins'].min(axis=0)) >= MARGIN
        fx, fh = marks(case)
        _REF[case.name] = dict(pb=pb, phar=phar_dict(case, pb), fx=fx, fh=fh, restraints=restraints, rec=rec, noise=noise, guided=guided,
                               unguided=unguided, keep=keep)
    return _REF[case.name]

