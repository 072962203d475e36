"""CPU model of the restrained multi-pocket chain (ConditionalDDPM.sample_restrained_given_pockets, cmdgen_multi_restrained_chain;
INTEGRATION.md, "Restraints on the shared latent"), built only from oracle.ref_cpu primitives in torch fp32: the multi-pocket chain's op
sequence over the MEMBER samples (every member of a group holds a copy of the group's latent, the members' eps rows are combined by the
group's weights before every op) with the guidance term of csrc/kernels_restrain.hip added to the mean of every posterior op, once per
GROUP:
  - a restraint belongs to a group (rec['sample'] is the group index), its centres lie in the common frame of the group's pockets;
  - xhat comes from the combined eps the step itself uses;
  - the frame shift is the group's FIRST member's, its pocket as it stands at the op's input;
  - the clash term sums over the atoms of EVERY member, unweighted; a point's terms are summed in the definition's order - position,
    distance and exclusion terms in list order, then the members, ascending, each member's atoms in index order;
  - every member's copy of the latent gets the same displacement.
With no record and r_c = 0, or with scale = 0, it reproduces multi_pocket_ref.multi_pocket_chain bit for bit; with every group of one
member it reproduces restraint_ref.restrained_chain bit for bit (test_multi_restraint_cpu.py asserts both).

It is chain_ref.run_chain with the groups and the guide parts."""
import numpy as np
import torch

from chain_ref import CHAIN_CAP, MARGIN, Groups, _norm, energy_terms, kept_groups, op_terms, pair_margins, run_chain, touched_samples      # noqa: F401

KEYS = ('xh_phar', 'xh_pocket', 'phar_mask', 'pocket_mask', 'z_steps', 'pocket_steps', 'margins', 'op_energy', 'energy', 'max_violation',
        'kind_violation', 'clipped', 'unclipped', 'other_member_clash')


def other_member_clash(a, clash_r, n_x, nd):
    """A test's diagnostic, no part of the chain: the largest clash violation (A) of one op - `a` is what run_chain hands its probe - against
    an atom of a member other than its group's first.  Does a member other than the first bite?"""
    if not clash_r > 0:
        return 0.0
    terms_in = {k: v for k, v in a.items() if k != 't'}
    # the op's xhat, by the loop's own steps 1 and 2 a second time; with no record and r_c = 0 energy_terms pushes no term (both of its loops
    # are empty: `for r in rec`, `if clash_r > 0`) and returns zeros
    xhat = op_terms(rec=(), clash_r=0.0, clash_k=0.0, n_x=n_x, nd=nd, **terms_in)[0]
    q, um, qg = n_x * a['P'][:, :nd], a['pm'], a['qg']
    other = a['first'][qg] != a['qm']                                  # [Np] atoms of a member that is not its group's first
    vo = 0.0
    for k in range(len(a['first'])):
        pts, atoms = xhat[um == k], q[other & (qg == k)]
        if len(pts) and len(atoms):
            dist = _norm((pts[:, None, :] - atoms[None, :, :]).reshape(-1, 3))
            vo = max(vo, float(torch.clamp(clash_r - dist, min=0).max()))
    return vo


def multi_restrained_chain(p, cfg, pocket, group_sizes, num_nodes_phar, weights, rec, clash_r=0.0, clash_k=0.0, scale=1.0, max_shift=1.0,
                           guide_below=1.0, timesteps=None, noise=None, checks=True):
    """pocket: dict(x, one_hot, size [B], mask) of the member samples; weights [B]; rec: the record array of cmdgen_amd.restraints.records
    called with the per-GROUP point counts; noise(shape) supplies each of the K + 2 draws of shape (Nu, 3 + P).
    -> dict(xh_phar [Nu, 3+P], xh_pocket [Np, 3+R], phar_mask [Nu] (group ids), pocket_mask, z_steps [K, Nu, 3+P], pocket_steps [K, Np, 3],
    margins [K + 1, B] (A), op_energy [K, G], energy [G], max_violation [G], kind_violation [K, 4], clipped, unclipped: counts of
    displacements (per unique row and op), other_member_clash [K]: the largest clash violation (A) against an atom of a member other than its
    group's first)."""
    other_v = []
    groups = dict(group_sizes=group_sizes, weights=weights)
    guide = dict(rec=rec, clash_r=clash_r, clash_k=clash_k, scale=scale, max_shift=max_shift, guide_below=guide_below)
    o = run_chain(p, cfg, pocket, num_nodes_phar=num_nodes_phar, groups=groups, guide=guide, timesteps=timesteps, noise=noise, checks=checks,
                  probe=lambda op, a: other_v.append(other_member_clash(a, clash_r, cfg['norm_values'][0], cfg['n_dims'])))
    o['other_member_clash'] = np.asarray(other_v)
    return {k: o[k] for k in KEYS}
