"""CPU model of ConditionalDDPM.edit (the edit chain; INTEGRATION.md, "Editing a given pharmacophore"), built only from
oracle.ref_cpu primitives: cond_inpaint_ref.cond_inpaint's op sequence with one mask per column group and a start level, so
with both masks equal and start = timesteps it reproduces cond_inpaint bit for bit given the same draws.

It is chain_ref.run_chain with the edit part alone."""
from chain_ref import edit_plan, run_chain                         # noqa: F401  (edit_plan: imported from here by the tests)


def cond_edit(p, cfg, phar, pocket, fix_x, fix_h, start=None, resamplings=1, jump_length=1, timesteps=None, noise=None,
              return_steps=False, checks=True):
    """-> (xh_phar, xh_pocket, phar_mask, pocket_mask[, z_steps, pocket_steps]); noise(shape) supplies each draw in call order."""
    edit = dict(fix_x=fix_x, fix_h=fix_h, start=start, resamplings=resamplings, jump_length=jump_length)
    o = run_chain(p, cfg, pocket, phar=phar, edit=edit, timesteps=timesteps, noise=noise, checks=checks, record_margins=False)
    out = (o['xh_phar'], o['xh_pocket'], o['phar_mask'], o['pocket_mask'])
    return out + (o['z_steps'], o['pocket_steps']) if return_steps else out
