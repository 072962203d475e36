"""CPU model of editing under restraints (ConditionalDDPM.edit_restrained, cmdgen_restrained_edit_chain; INTEGRATION.md, "Editing under
restraints"), built only from oracle.ref_cpu primitives and restraint_ref.energy_terms in torch fp32: edit_ref.cond_edit's op sequence with the
guidance of restraint_ref.restrained_chain in op A.  A row whose x columns are held enters the energy at its given position moved into the
current frame and receives no displacement.

Given the same draws it reproduces edit_ref.cond_edit bit for bit with scale = 0 or without restraints, and restraint_ref.restrained_chain bit
for bit without marks, from the prior and without jumps (the B draws are then read and not used).

It is chain_ref.run_chain with the edit and the guide parts."""
from chain_ref import op_terms, run_chain                          # noqa: F401  (op_terms: the tests look at single ops with it)

KEYS = ('xh_phar', 'xh_pocket', 'phar_mask', 'pocket_mask', 'z_steps', 'pocket_steps', 'known_steps', 'margins', 'op_energy', 'energy',
        'max_violation', 'kind_violation')


def restrained_edit(p, cfg, phar, pocket, fix_x, fix_h, rec, clash_r=0.0, clash_k=0.0, scale=1.0, max_shift=1.0, guide_below=1.0, start=None,
                    resamplings=1, jump_length=1, timesteps=None, noise=None, checks=True, probe=None):
    """-> dict(xh_phar, xh_pocket, phar_mask, pocket_mask, z_steps [n_steps, Nl, 3+P], pocket_steps [n_steps, Np, 3], margins [n_steps + 1, B]
    (A, one row per evaluation), op_energy [n_steps, B], energy [B], max_violation [B], kind_violation [n_steps, 4], known_steps [n_steps, Nl, 3]:
    the x of the noised known rows in the frame of the saved step - what the x-held rows of z_steps are, up to rounding).  noise(shape) supplies
    each draw in call order.
    probe(op index, dict of the op's inputs): called before the guidance of every op (tests look at single ops through it)."""
    edit = dict(fix_x=fix_x, fix_h=fix_h, start=start, resamplings=resamplings, jump_length=jump_length)
    guide = dict(rec=rec, clash_r=clash_r, clash_k=clash_k, scale=scale, max_shift=max_shift, guide_below=guide_below)
    o = run_chain(p, cfg, pocket, phar=phar, edit=edit, guide=guide, timesteps=timesteps, noise=noise, checks=checks, probe=probe)
    return {k: o[k] for k in KEYS}
