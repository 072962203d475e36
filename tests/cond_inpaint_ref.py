"""CPU model of ConditionalDDPM.inpaint (the conditional RePaint loop; INTEGRATION.md, "Pharmacophore-constrained
sampling"), built only from oracle.ref_cpu primitives: the same op sequence as ref_cpu.sample_given_pocket, so a chain
without fixed rows and with resamplings = jump_length = 1 reproduces it bit for bit given the same draws.

It is chain_ref.run_chain with the edit part alone: one row mask for both column groups, from the prior."""
from chain_ref import inpaint_plan, run_chain                      # noqa: F401  (inpaint_plan: imported from here by the tests)


def cond_inpaint(p, cfg, phar, pocket, phar_fixed, resamplings=1, jump_length=1, timesteps=None, noise=None,
                 return_steps=False, checks=True):
    """-> (xh_phar, xh_pocket, phar_mask, pocket_mask[, z_steps, pocket_steps]); noise(shape) supplies each draw in call order."""
    edit = dict(fix_x=phar_fixed, fix_h=phar_fixed, start=None, resamplings=resamplings, jump_length=jump_length)
    o = run_chain(p, cfg, pocket, phar=phar, edit=edit, timesteps=timesteps, noise=noise, checks=checks, record_margins=False)
    out = (o['xh_phar'], o['xh_pocket'], o['phar_mask'], o['pocket_mask'])
    return out + (o['z_steps'], o['pocket_steps']) if return_steps else out
