"""Cases, inputs and reference results of the restrained multi-pocket edit chain's tests (test_hip_multi_restrained_edit.py on the GPU,
test_multi_restrained_edit_cpu.py without one).  The reference is multi_restrained_edit_ref.multi_restrained_edit, live, fp32 on the CPU,
computed once per run and shared - guided, and unguided (scale = 0) on the same draws.

Everything is composed from what exists: multi_edit_cases' batches (MIXED: groups of 1, 2 and 3 members, 1-8 given points, every kind of
mark; LARGE: one member above 128 nodes; and multi_pocket_cases.PAIRS with marks of its own, M = 2 everywhere), their member pockets,
weights, given rows and injected noise [n_draws][Nu][11], K = 6; and
multi_restraint_cases.restraints_of's recipe per GROUP - a position restraint on point 0, from two points on a distance window between
points 0 and 1, an exclusion sphere, the clash term against every member's atoms.  In MIXED group 3 (no mark) has no record, and group 2
('b-hx----') has its distance window between the held point 0 and the free point 1.

A group with a pair within MARGIN of the radius graph's cutoff at any reference evaluation (guided or unguided) is left out of a comparison;
at most CHAIN_CAP of a case's groups may be - test_multi_restrained_edit_cpu.py asserts it on the reference alone, together with the bite of
the guidance (a clipped and an unclipped displacement, a clash term from a member other than the first, a guided op with a held-free distance
record)."""
from collections import namedtuple

import numpy as np
import torch

import multi_edit_cases as mec
import multi_pocket_cases as mc
import multi_restrained_edit_ref as mre
import multi_restraint_cases as mrc
from multi_restrained_edit_ref import MARGIN, CHAIN_CAP           # noqa: F401  (1e-4 A, 0.20)
from cmdgen_amd import restraints as rs

K = mec.K
SCALE = mrc.SCALE
MAX_SHIFT = mrc.MAX_SHIFT
CLASH = mrc.CLASH                 # (3.0, 1.0)
Case = namedtuple('Case', mc.Case._fields + ('bare_group',))

MIXED = Case(*mec.MIXED, 3)       # marks 'hh--', 'x', 'b-hx----', '---', 'xxx---', 'hh'; group 3 without a record
LARGE = Case(*mec.LARGE, None)    # one member above 128 nodes: the 1024-thread path of both launches
PAIRS = Case(*mc.PAIRS, None)     # M = 2 everywhere (multi_pocket_cases' batch): the other engines
MARKS = dict(mec.MARKS, pairs=('b-x---', 'h--', 'xh------'))
CASES = {c.name: c for c in (MIXED, LARGE, PAIRS)}
HELD_FREE_GROUP = 2               # of MIXED: its distance record joins point 0 (x held) to point 1 (free)

Run = mec.Run
# from the prior with resampling and jumps; part-way (the second init kernel) with the same schedule rules; the large member from the prior
RUNS = (Run('mixed', 6, 2, 2), Run('mixed', 3, 2, 2), Run('large', 6, 1, 1))
ENGINE_RUN = Run('pairs', 6, 2, 2)
run_id = mec.run_id

config, state_dict, params, pocket_dict = mc.config, mc.state_dict, mc.params, mc.pocket_dict
member_pockets, weights_of = mc.member_pockets, mc.weights_of
_REF = {}


def given_rows(case):
    """(phar_x [Nu,3], phar_one_hot [Nu,8], fix_x [Nu], fix_h [Nu]) float32: multi_edit_cases.given_rows' recipe (its values for its cases)."""
    if case.name in mec.MARKS:
        return mec.given_rows(mec.CASES[case.name])
    rng = np.random.Generator(np.random.PCG64(case.first_index + 1))
    nu = int(sum(case.nph))
    x = (rng.normal(size=(nu, 3)) * 2.5).astype(np.float32)
    oh = np.eye(8, dtype=np.float32)[rng.integers(0, 8, size=nu)]
    marks = ''.join(MARKS[case.name])
    assert len(marks) == nu and [len(m) for m in MARKS[case.name]] == list(case.nph)
    return x, oh, np.array([c in 'xb' for c in marks], dtype=np.float32), np.array([c in 'hb' for c in marks], dtype=np.float32)


def phar_dict(case):
    x, oh, _, _ = given_rows(case)
    nph = np.asarray(case.nph, dtype=np.int64)
    return {'x': torch.from_numpy(x), 'one_hot': torch.from_numpy(oh), 'size': torch.from_numpy(nph),
            'mask': torch.from_numpy(np.repeat(np.arange(len(nph)), nph))}


def noise_of(run):
    """[n_draws][Nu][11], multi_edit_cases.noise_of's draws"""
    case = CASES[run.case]
    return torch.randn((plan(run)[1], int(sum(case.nph)), 11), generator=torch.Generator().manual_seed(case.first_index + 7 * run.start))


def plan(run):
    """(n_steps, n_draws, n_jumps)"""
    return mre.edit_plan(run.r, run.j, K, run.start)


def restraints_of(case, pb=None):
    """multi_restraint_cases.restraints_of's list for the case's groups, 'sample' the GROUP."""
    return mrc.restraints_of(case, member_pockets(case) if pb is None else pb)


def run_ref(run, pb, w, rec, noise, scale, clash=CLASH, guide_below=1.0, marked=True):
    case = CASES[run.case]
    _, _, fx, fh = given_rows(case)
    if not marked:
        fx, fh = np.zeros_like(fx), np.zeros_like(fh)
    tape = iter(noise)
    with torch.no_grad():
        out = mre.multi_restrained_edit(params(), config().as_dict(), phar_dict(case), pocket_dict(pb), case.group_sizes, w, fx, fh, rec,
                                        clash_r=clash[0], clash_k=clash[1], scale=scale, max_shift=MAX_SHIFT, guide_below=guide_below,
                                        start=run.start, resamplings=run.r, jump_length=run.j, timesteps=K, noise=lambda shape: next(tape))
    assert next(tape, None) is None                      # every planned draw was used
    return out


def reference(run):
    """dict(pb, weights, restraints, rec, noise, groups, guided, unguided (multi_restrained_edit_ref's dicts, scale = SCALE and 0), keep [G]) -
    computed once per run."""
    if run not in _REF:
        torch.set_num_threads(min(16, max(1, torch.get_num_threads())))
        case = CASES[run.case]
        pb, w, noise = member_pockets(case), weights_of(case), noise_of(run)
        restraints = restraints_of(case, pb)
        rec = rs.records(restraints, case.nph)
        groups = mre.Groups(case.group_sizes, case.nph)
        guided, unguided = run_ref(run, pb, w, rec, noise, SCALE), run_ref(run, pb, w, rec, noise, 0.0)
        keep = mre.kept_groups(guided['margins'], groups) & mre.kept_groups(unguided['margins'], groups)
        _REF[run] = dict(pb=pb, weights=w, restraints=restraints, rec=rec, noise=noise, groups=groups, guided=guided, unguided=unguided,
                         keep=keep)
    return _REF[run]
