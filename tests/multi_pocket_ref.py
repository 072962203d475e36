"""CPU model of the multi-pocket chain (ConditionalDDPM.sample_given_pockets, cmdgen_multi_pocket_chain; INTEGRATION.md, "One
pharmacophore for several pockets"), built only from oracle.ref_cpu primitives: ref_cpu.sample_given_pocket's op sequence over the
MEMBER samples of the batch, every member of a group holding a copy of the group's latent, with the members' eps rows combined by
the group's weights before every op.  With groups of one member it reproduces ref_cpu.sample_given_pocket bit for bit given the
same draws.

Layout.  The batch has B = sum_g M_g member samples; group g is the consecutive members first[g] .. first[g] + M_g - 1, all with
num_nodes_phar[g] phar rows.  Draws, z_steps and the phar output hold ONE copy of the rows per group (Nu = sum_g num_nodes_phar[g]).

It is chain_ref.run_chain with the groups part alone.
"""
from chain_ref import CHAIN_CAP, CUTOFF, MARGIN, Groups, kept_groups, pair_margins, run_chain      # noqa: F401  (imported from here)


def multi_pocket_chain(p, cfg, pocket, group_sizes, num_nodes_phar, weights, timesteps=None, noise=None, return_steps=False,
                       checks=True):
    """pocket: dict(x, one_hot, size [B], mask) of the member samples; weights [B] (one per member; every group's sum to 1);
    noise(shape) supplies each of the K + 2 draws of shape (Nu, 3 + P).
    -> (xh_phar [Nu, 3+P], xh_pocket [Np, 3+R], unique phar mask [Nu] (group ids), pocket mask[, z_steps [K, Nu, 3+P],
    pocket_steps [K, Np, 3], margins [K + 1, B]])."""
    o = run_chain(p, cfg, pocket, num_nodes_phar=num_nodes_phar, groups=dict(group_sizes=group_sizes, weights=weights), timesteps=timesteps,
                  noise=noise, checks=checks, record_margins=return_steps)
    out = (o['xh_phar'], o['xh_pocket'], o['phar_mask'], o['pocket_mask'])
    return out + (o['z_steps'], o['pocket_steps'], o['margins']) if return_steps else out
