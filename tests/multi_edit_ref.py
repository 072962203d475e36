"""CPU model of the multi-pocket edit chain (ConditionalDDPM.edit_given_pockets, cmdgen_multi_edit_chain; INTEGRATION.md, "Holding or
editing given points for several pockets"), built only from oracle.ref_cpu primitives: multi_pocket_ref.multi_pocket_chain's grouping
and eps combination with edit_ref.cond_edit's op sequence.  Every member of a group holds a copy of the group's latent; the known
rows, the marks and the draws hold ONE copy of the rows per group (Nu rows).  The pocket offset of step B is the GROUP's: the shift of
the group's first member's pocket, com(P_first) - com(P0_first), used by every member.

With groups of one member it reproduces edit_ref.cond_edit, and with no mark, start = timesteps and resamplings = jump_length = 1
multi_pocket_ref.multi_pocket_chain, both bit for bit given the same draws.

It is chain_ref.run_chain with the groups and the edit parts."""
from chain_ref import run_chain


def multi_edit_chain(p, cfg, phar, pocket, group_sizes, weights, fix_x, fix_h, start=None, resamplings=1, jump_length=1,
                     timesteps=None, noise=None, return_steps=False, checks=True):
    """phar: dict(x [Nu,3], one_hot [Nu,P], size [G]) one copy of the rows per group, in the pockets' common frame; pocket:
    dict(x, one_hot, size [B], mask) of the member samples; weights [B]; fix_x, fix_h [Nu]; noise(shape) supplies each draw of shape
    (Nu, 3 + P) in edit_ref.cond_edit's call order.
    -> (xh_phar [Nu, 3+P], xh_pocket [Np, 3+R], unique phar mask [Nu], pocket mask[, z_steps [n_steps, Nu, 3+P], pocket_steps
    [n_steps, Np, 3], margins [n_steps + 1, B]])."""
    edit = dict(fix_x=fix_x, fix_h=fix_h, start=start, resamplings=resamplings, jump_length=jump_length)
    o = run_chain(p, cfg, pocket, phar=phar, groups=dict(group_sizes=group_sizes, weights=weights), edit=edit, timesteps=timesteps,
                  noise=noise, checks=checks, record_margins=return_steps)
    out = (o['xh_phar'], o['xh_pocket'], o['phar_mask'], o['pocket_mask'])
    return out + (o['z_steps'], o['pocket_steps'], o['margins']) if return_steps else out
