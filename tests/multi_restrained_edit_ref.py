"""CPU model of the restrained multi-pocket edit chain (ConditionalDDPM.edit_restrained_given_pockets, cmdgen_multi_restrained_edit_chain;
INTEGRATION.md, "Editing under restraints for several pockets"), built only from oracle.ref_cpu primitives in torch fp32: the multi-pocket
edit chain's op sequence over the MEMBER samples (every member of a group holds a copy of the group's latent; the known rows, the marks and
the draws hold one copy of the rows per group; ops A, B and C of the edit plan) with the guidance term of csrc/kernels_restrain.hip added to
the mean of op A, once per GROUP:
  - a restraint belongs to a group (rec['sample'] is the group index), its centres lie in the common frame of the group's pockets;
  - xhat of a row whose x columns are not held comes from the combined eps the step itself uses; a row whose x columns ARE held enters at its
    given position moved into the current frame, n_x K_i.x + shift_g;
  - the frame shift is the group's FIRST member's, its pocket as it stands at the op's input (step B keeps its own offset);
  - the clash term sums over the atoms of EVERY member, unweighted; a point's terms are summed in the definition's order;
  - every member's copy of the latent gets the same displacement, on the rows whose x is not held only; op C and the decode are not guided.
Given the same draws it reproduces, bit for bit, multi_edit_ref.multi_edit_chain with scale = 0 or with no record and r_c = 0,
restrained_edit_ref.restrained_edit with every group of one member, and multi_restraint_ref.multi_restrained_chain with no mark, start =
timesteps and resamplings = jump_length = 1 (the B draws are then read and not used) - test_multi_restrained_edit_cpu.py asserts all three.

It is chain_ref.run_chain with the groups, the edit and the guide parts."""
import numpy as np
import torch

from chain_ref import (CHAIN_CAP, DISTANCE, MARGIN, Groups, _norm, edit_plan, energy_terms, kept_groups, pair_margins,      # noqa: F401
                       run_chain, touched_samples)
from multi_restraint_ref import other_member_clash

KEYS = ('xh_phar', 'xh_pocket', 'phar_mask', 'pocket_mask', 'z_steps', 'pocket_steps', 'margins', 'op_energy', 'energy', 'max_violation',
        'kind_violation', 'clipped', 'unclipped', 'other_member_clash', 'held_record_ops')


def held_record_op(a, rec, clash_r, scale, guide_below):
    """A test's diagnostic, no part of the chain: whether at one op - `a` is what run_chain hands its probe - a guided group has a distance
    record that joins a held-x row to a free row."""
    um, fx, G = a['pm'], a['fx'], len(a['first'])
    nph = torch.bincount(um, minlength=G)
    ubase = torch.cumsum(nph, 0) - nph
    held_free = torch.zeros(G, dtype=torch.bool)                       # groups with a distance record between a held-x and a free row
    for r in rec:
        if int(r['kind']) == DISTANCE:
            g = int(r['sample'])
            if bool(fx[ubase[g] + int(r['i'])]) != bool(fx[ubase[g] + int(r['j'])]):
                held_free[g] = True
    guided = torch.from_numpy(touched_samples(rec, G, clash_r)) & (a['t'][a['first']][:, 0] <= guide_below) & (scale > 0)       # [G]
    return bool((guided & held_free).any())


def multi_restrained_edit(p, cfg, phar, pocket, group_sizes, weights, fix_x, fix_h, rec, clash_r=0.0, clash_k=0.0, scale=1.0, max_shift=1.0,
                          guide_below=1.0, start=None, resamplings=1, jump_length=1, timesteps=None, noise=None, checks=True):
    """phar: dict(x [Nu,3], one_hot [Nu,P], size [G]) one copy of the rows per group, in the pockets' common frame; pocket: dict(x, one_hot,
    size [B], mask) of the member samples; weights [B]; fix_x, fix_h [Nu]; rec: the record array of cmdgen_amd.restraints.records called with
    the per-GROUP point counts; noise(shape) supplies each draw of shape (Nu, 3 + P) in the edit plan's call order.
    -> dict(xh_phar [Nu, 3+P], xh_pocket [Np, 3+R], phar_mask [Nu] (group ids), pocket_mask, z_steps [n_steps, Nu, 3+P], pocket_steps
    [n_steps, Np, 3], margins [n_steps + 1, B] (A), op_energy [n_steps, G], energy [G], max_violation [G], kind_violation [n_steps, 4],
    clipped, unclipped: counts of displacements that were and were not clipped (per unique free row and op), other_member_clash [n_steps]:
    the largest clash violation (A) against an atom of a member other than its group's first, held_record_ops: how many guided ops had a
    distance record that joins a held-x row to a free row of a guided group)."""
    other_v, held_v = [], []

    def probe(op, a):
        other_v.append(other_member_clash(a, clash_r, cfg['norm_values'][0], cfg['n_dims']))
        held_v.append(held_record_op(a, rec, clash_r, scale, guide_below))

    groups = dict(group_sizes=group_sizes, weights=weights)
    edit = dict(fix_x=fix_x, fix_h=fix_h, start=start, resamplings=resamplings, jump_length=jump_length)
    guide = dict(rec=rec, clash_r=clash_r, clash_k=clash_k, scale=scale, max_shift=max_shift, guide_below=guide_below)
    o = run_chain(p, cfg, pocket, phar=phar, groups=groups, edit=edit, guide=guide, timesteps=timesteps, noise=noise, checks=checks, probe=probe)
    o.update(other_member_clash=np.asarray(other_v), held_record_ops=sum(held_v))
    return {k: o[k] for k in KEYS}
