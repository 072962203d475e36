"""Cases, inputs and reference results of the restrained diverse chain's tests (test_hip_diverse_restrained.py on the GPU,
test_diverse_restrained_cpu.py without one).  The reference is diverse_restrained_ref.diverse_restrained_chain, live, fp32 on the CPU, computed
once per case and run and shared: both terms, restraints only (strength = 0), overlap only (scale = 0) and neither, all on the same draws.

Inputs as diverse_cases.py makes them (its pockets(): bounded_config(20, 1000), seed-0 weights, ONE ragged C-alpha pocket per set, repeated for
every member) with restraints in restraint_cases.restraints_of's style on the samples `restrained`, injected noise and K = 5.

  mixed   with the clash term off every branch of the mean runs in one batch: both terms (samples 0-3, 5, 6), the restraint term alone (sample 4,
          the single-member set 1), the overlap term alone (sample 7, which has no restraint, and the bare set 3), neither (sample 10, the bare
          single-member set 4).  Also run with the clash term on (every sample is touched then) and with both max_shifts at CLIP_SHIFT.
  large   set 0 on a pocket of 140 nodes: the 1024-thread block and the loops' second trips; restraints on every sample, clash on.

Leave-out rule.  The overlap term couples the members of a set, so a set with ANY member within MARGIN of the radius graph's cutoff, at any
evaluation of any of the four reference runs (of a variant: those four and the variant's own run), is left out whole.  At most CHAIN_CAP of a
case's sets may be left out, and none is for the committed inputs: first_index is chosen that way, and test_diverse_restrained_cpu.py asserts
both."""
from collections import namedtuple

import numpy as np
import torch

import diverse_cases as dc
import diverse_restrained_ref as drr
import restraint_cases as rc
from chain_ref import CHAIN_CAP, MARGIN                            # noqa: F401  (0.20, 1e-4 A)
from cmdgen_amd import restraints as rs

K = 5
SCALE, MAX_SHIFT, CLASH, NO_CLASH = rc.SCALE, rc.MAX_SHIFT, rc.CLASH, (0.0, 0.0)      # the restraint side: restraint_cases'
STRENGTH, WIDTH, DIVERSE_MAX_SHIFT = dc.STRENGTH, dc.WIDTH, dc.MAX_SHIFT              # the overlap side: diverse_cases'
CLIP_SHIFT = dc.CLIP_SHIFT            # both max_shifts of the run that exercises the clips
# (bare_sample: restraints_of's field - no sample is skipped there; `restrained` picks the samples that keep theirs)
Case = namedtuple('Case', 'name sets nph K first_index big_set restrained clash bare_sample')

MIXED = Case('mixed', (4, 1, 3, 2, 1), (4, 6, 3, 5, 2, 8, 1, 7, 5, 5, 3), K, 9350, None, tuple(range(7)), NO_CLASH, None)
LARGE = Case('large', (2, 2), (8, 5, 3, 4), K, 9440, 0, tuple(range(4)), CLASH, None)
CASES = {c.name: c for c in (MIXED, LARGE)}
VARIANTS = {'clash': dict(clash=CLASH), 'clipped': dict(max_shift=CLIP_SHIFT, diverse_max_shift=CLIP_SHIFT)}     # of `mixed`

config, state_dict, params, pockets, noise_of, pocket_dict = dc.config, dc.state_dict, dc.params, dc.pockets, dc.noise_of, dc.pocket_dict
_REF = {}


def restraints_of(case, pb):
    """restraint_cases.restraints_of's list (a position restraint on point 0, an exclusion sphere at the pocket's centre and, from two points on,
    a distance window between points 0 and 1) for the samples case.restrained."""
    return [r for r in rc.restraints_of(case, pb) if r['sample'] in case.restrained]


def first_of_set(case):
    return np.concatenate([[0], np.cumsum(case.sets)[:-1]])


def run_ref(case, pb, rec, noise, scale=SCALE, strength=STRENGTH, clash=None, max_shift=MAX_SHIFT, diverse_max_shift=DIVERSE_MAX_SHIFT,
            guide_below=1.0, diverse_guide_below=1.0, sets=None):
    clash = case.clash if clash is None else clash
    tape = iter(noise)
    with torch.no_grad():
        return drr.diverse_restrained_chain(params(), config().as_dict(), pocket_dict(pb), case.nph, case.sets if sets is None else sets, rec,
                                            clash_r=clash[0], clash_k=clash[1], scale=scale, max_shift=max_shift, guide_below=guide_below,
                                            strength=strength, width=WIDTH, diverse_max_shift=diverse_max_shift,
                                            diverse_guide_below=diverse_guide_below, timesteps=case.K, noise=lambda shape: next(tape))


def kept_sets(case, *runs):
    """[S] bool: the sets none of whose members has a pair within MARGIN of the cutoff at any evaluation of any of the runs."""
    return dc.kept_sets(case, *runs)


def reference(case, variant=None):
    """dict(pb, restraints, rec, noise, both, restrained, diverse, neither (diverse_restrained_ref's dicts: both terms, strength = 0, scale = 0,
    both zero), keep [S], keep_samples [B], touched [B] (a restraint or the clash term touches the sample), coupled [B] (its set has several
    members)) - computed once.  variant: a key of VARIANTS - `both` is then that run (the other three are the case's own: they take no part in
    the variant's comparison but in its leave-out rule)."""
    key = (case.name, variant)
    if key not in _REF:
        torch.set_num_threads(min(16, max(1, torch.get_num_threads())))
        if variant is None:
            pb, noise = pockets(case), noise_of(case)
            restraints = restraints_of(case, pb)
            rec = rs.records(restraints, case.nph)
            runs = dict(both=run_ref(case, pb, rec, noise), restrained=run_ref(case, pb, rec, noise, strength=0.0),
                        diverse=run_ref(case, pb, rec, noise, scale=0.0), neither=run_ref(case, pb, rec, noise, scale=0.0, strength=0.0))
            keep = kept_sets(case, *runs.values())
            clash_r = case.clash[0]
        else:
            base = reference(case)
            pb, noise, restraints, rec = (base[k] for k in ('pb', 'noise', 'restraints', 'rec'))
            runs = dict(base, both=run_ref(case, pb, rec, noise, **VARIANTS[variant]))
            runs = {k: runs[k] for k in ('both', 'restrained', 'diverse', 'neither')}
            keep = kept_sets(case, *runs.values()) & base['keep']
            clash_r = VARIANTS[variant].get('clash', case.clash)[0]
        touched = np.isin(np.arange(len(case.nph)), [r['sample'] for r in restraints]) | (clash_r > 0)
        _REF[key] = dict(pb=pb, restraints=restraints, rec=rec, noise=noise, **runs, keep=keep, keep_samples=np.repeat(keep, case.sets),
                         touched=touched, coupled=np.repeat(np.asarray(case.sets) > 1, case.sets))
    return _REF[key]
