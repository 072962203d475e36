"""CPU model of the multi-pocket chain (ConditionalDDPM.sample_given_pockets, cmdgen_multi_pocket_chain; INTEGRATION.md, "One
pharmacophore for several pockets"), built only from oracle.ref_cpu primitives: ref_cpu.sample_given_pocket's op sequence over the
MEMBER samples of the batch, every member of a group holding a copy of the group's latent, with the members' eps rows combined by
the group's weights before every op.  With groups of one member it reproduces ref_cpu.sample_given_pocket bit for bit given the
same draws.

Layout.  The batch has B = sum_g M_g member samples; group g is the consecutive members first[g] .. first[g] + M_g - 1, all with
num_nodes_phar[g] phar rows.  Draws, z_steps and the phar output hold ONE copy of the rows per group (Nu = sum_g num_nodes_phar[g]).
"""
import numpy as np
import torch

from oracle import ref_cpu
from oracle.ref_cpu import FLOAT, INT

CUTOFF = 6.0
MARGIN = 1e-4          # A: a group with a pair closer than this to the cutoff at any evaluation may be left out of a comparison
CHAIN_CAP = 0.20       # ... but at most this share of a case's groups


class Groups:
    """Index tables of a grouping: group_sizes [G], num_nodes_phar [G] (per group)."""
    def __init__(self, group_sizes, num_nodes_phar):
        self.sizes = np.asarray(group_sizes, dtype=np.int64)
        self.nph = np.asarray(num_nodes_phar, dtype=np.int64)
        assert self.sizes.ndim == 1 and self.sizes.shape == self.nph.shape and (self.sizes >= 1).all()
        self.G, self.B, self.max_m = len(self.sizes), int(self.sizes.sum()), int(self.sizes.max())
        self.first = np.concatenate([[0], np.cumsum(self.sizes)[:-1]])
        self.group_of = np.repeat(np.arange(self.G), self.sizes)                       # [B] group of a member
        self.member_nph = self.nph[self.group_of]                                       # [B] phar rows of a member
        self.Nu, self.Nl = int(self.nph.sum()), int(self.member_nph.sum())
        ubase = np.concatenate([[0], np.cumsum(self.nph)[:-1]])
        pbase = np.concatenate([[0], np.cumsum(self.member_nph)[:-1]])
        local = np.arange(self.Nl) - np.repeat(pbase, self.member_nph)
        self.phar_mask = torch.from_numpy(np.repeat(np.arange(self.B), self.member_nph))          # [Nl] member of a member row
        self.unique_mask = torch.from_numpy(np.repeat(np.arange(self.G), self.nph))               # [Nu] group of a unique row
        self.urow = torch.from_numpy(ubase[self.group_of][self.phar_mask.numpy()] + local)        # [Nl] unique row of a member row
        # rows_of[j]: (unique rows, member rows, member) of the j-th member of every group that has one
        self.rows_of = []
        for j in range(self.max_m):
            gs = np.flatnonzero(self.sizes > j)
            members = self.first[gs] + j
            mrows = np.concatenate([pbase[b] + np.arange(self.member_nph[b]) for b in members]).astype(np.int64)
            urows = np.concatenate([ubase[g] + np.arange(self.nph[g]) for g in gs]).astype(np.int64)
            self.rows_of.append((torch.from_numpy(urows), torch.from_numpy(mrows), torch.from_numpy(np.repeat(members, self.nph[gs]))))

    def combine(self, rows, w):
        """sum_m w_m rows_m with m ascending, the first term not added to a zero: member rows [Nl, C] -> unique rows [Nu, C]."""
        u, r, b = self.rows_of[0]
        out = w[b][:, None] * rows[r]
        for u, r, b in self.rows_of[1:]:
            out[u] = out[u] + w[b][:, None] * rows[r]
        return out

    def combine_members(self, per_member, w):
        """The same sum over one row per member: [B, C] -> [G, C]."""
        f = torch.from_numpy(self.first)
        out = w[f][:, None] * per_member[f]
        for j in range(1, self.max_m):
            gs = torch.from_numpy(np.flatnonzero(self.sizes > j))
            out[gs] = out[gs] + w[f[gs] + j][:, None] * per_member[f[gs] + j]
        return out

    def first_rows(self):
        """[Nu] the member rows of every group's first member: the group's copy of the latent that is reported."""
        return self.rows_of[0][1]


def pair_margins(x_phar, x_pocket, phar_mask, pocket_mask, cutoff=CUTOFF):
    """[B] float64: per member sample the smallest | ||x_i - x_j|| - cutoff | over its pairs i < j."""
    pm, qm = np.asarray(phar_mask), np.asarray(pocket_mask)
    xp, xq = np.asarray(x_phar, dtype=np.float64), np.asarray(x_pocket, dtype=np.float64)
    B = int(max(pm.max(initial=-1), qm.max(initial=-1))) + 1
    out = np.full(B, np.inf)
    for b in range(B):
        p = np.concatenate([xp[pm == b], xq[qm == b]])
        if len(p) > 1:
            d = np.sqrt(((p[:, None, :] - p[None, :, :]) ** 2).sum(-1))
            out[b] = np.abs(d[np.triu_indices(len(p), k=1)] - cutoff).min()
    return out


def kept_groups(margins, groups):
    """[G] bool: the groups none of whose members has a pair within MARGIN of the cutoff at any evaluation (margins [evaluations, B])."""
    ok = np.asarray(margins).min(axis=0) >= MARGIN
    return np.array([ok[f:f + m].all() for f, m in zip(groups.first, groups.sizes)])


def multi_pocket_chain(p, cfg, pocket, group_sizes, num_nodes_phar, weights, timesteps=None, noise=None, return_steps=False,
                       checks=True):
    """pocket: dict(x, one_hot, size [B], mask) of the member samples; weights [B] (one per member; every group's sum to 1);
    noise(shape) supplies each of the K + 2 draws of shape (Nu, 3 + P).
    -> (xh_phar [Nu, 3+P], xh_pocket [Np, 3+R], unique phar mask [Nu] (group ids), pocket mask[, z_steps [K, Nu, 3+P],
    pocket_steps [K, Np, 3], margins [K + 1, B]])."""
    T, nd, pnf = cfg['timesteps'], cfg['n_dims'], cfg['phar_nf']
    nv, nb = cfg['norm_values'], cfg['norm_biases']
    assert not cfg.get('no_com_projection', False) and not cfg.get('update_pocket_coords', False)
    table = ref_cpu.gamma_source(p)
    timesteps = T if timesteps is None else timesteps
    gr = Groups(group_sizes, num_nodes_phar)
    B = gr.B
    assert len(pocket['size']) == B
    w = torch.as_tensor(weights).to(FLOAT).reshape(-1)
    assert len(w) == B
    draw = noise if noise is not None else (lambda shape: torch.randn(shape))
    pm, qm, urow = gr.phar_mask, pocket['mask'].to(INT), gr.urow
    shape = (gr.Nu, nd + pnf)
    # normalize, en_diffusion.py:874-889
    px = pocket['x'].to(FLOAT) / nv[0]
    xh0_pocket = torch.cat([px, (pocket['one_hot'].float() - nb[1]) / nv[1]], dim=1)
    # init: c = sum_m w_m com(P_m); every member's copy is [c, 0] + the group's draw, then the projection per member
    c = gr.combine_members(ref_cpu.scatter_mean(px, qm, B), w)                               # [G, 3]
    mu_phar = torch.cat((c, torch.zeros((gr.G, pnf))), dim=1)[torch.from_numpy(gr.group_of)][pm]
    sigma = torch.ones_like(pocket['size']).unsqueeze(1)
    z, P = ref_cpu.sample_normal_zero_com(mu_phar, xh0_pocket, sigma, pm, qm, draw(shape)[urow], nd)
    if checks:
        ref_cpu.assert_mean_zero_with_mask(z[:, :nd], pm)
    z_steps, p_steps, margins = [], [], []

    # The members are evaluated SLOT by slot: call j holds the j-th member of every group that has one, as one ordinary batch.  With
    # groups of one member the only call is ref_cpu.sample_given_pocket's own, and the first members of all groups form the batch a
    # single chain on the first pockets evaluates - so both reductions hold bit for bit (the oracle's matrix products round a
    # sample's rows differently in the last bit when the batch around it changes).
    slots = []
    for j, (u, r, b) in enumerate(gr.rows_of):
        members = torch.from_numpy(gr.first[gr.sizes > j] + j)
        renum = torch.full((B,), -1, dtype=INT)
        renum[members] = torch.arange(len(members))
        qrows = torch.nonzero(renum[qm] >= 0).reshape(-1)
        slots.append((r, members, renum[pm[r]], qrows, renum[qm[qrows]]))

    def eps_bar(t_array):
        """the members' evaluations combined per group, on every member's rows; the NaN guard is batch-wide"""
        if return_steps:
            margins.append(pair_margins(z[:, :nd], P[:, :nd], pm, qm, cfg['edge_cutoff']) * nv[0])     # (the graph is built on normalised x)
        eps = torch.empty_like(z)
        reset = False
        for r, members, pm_j, qrows, qm_j in slots:
            eps[r], _ = ref_cpu.dynamics_forward(p, cfg, z[r], P[qrows], t_array[members], pm_j, qm_j)
            # dynamics_forward zeroes the velocities of its whole call when one is NaN (dynamics.py:129-131): all exactly zero then
            reset = reset or (len(r) > 0 and not bool(eps[r][:, :nd].any()))
        if reset:
            eps[:, :nd] = 0.0
        return gr.combine(eps, w)[urow]

    for s in reversed(range(0, timesteps)):
        s_array = torch.full((B, 1), fill_value=s)
        t_array = s_array + 1
        s_array = s_array / timesteps
        t_array = t_array / timesteps
        gamma_s = ref_cpu.gamma_lookup(table, s_array, T)
        gamma_t = ref_cpu.gamma_lookup(table, t_array, T)
        sigma2_ts, sigma_ts, alpha_ts = ref_cpu.sigma_and_alpha_t_given_s(gamma_t, gamma_s)
        sigma_s, sigma_t = ref_cpu.sigma_of(gamma_s), ref_cpu.sigma_of(gamma_t)
        mu = z / alpha_ts[pm] - (sigma2_ts / alpha_ts / sigma_t)[pm] * eps_bar(t_array)
        sig = sigma_ts * sigma_s / sigma_t
        zt_old = z
        z, P = ref_cpu.sample_normal_zero_com(mu, P, sig, pm, qm, draw(shape)[urow], nd)
        if checks:
            ref_cpu.assert_mean_zero_with_mask(zt_old[:, :nd], pm)
        if return_steps:
            z_steps.append(z[gr.first_rows()].clone())
            p_steps.append(P[:, :nd].clone())
    # decode, as ref_cpu.sample_given_pocket
    t_zeros = torch.zeros((B, 1))
    gamma_0 = ref_cpu.gamma_lookup(table, t_zeros, T)
    sigma_x = torch.exp(-(-0.5 * gamma_0))
    net_out = eps_bar(t_zeros)
    sigma_0, alpha_0 = ref_cpu.sigma_of(gamma_0), ref_cpu.alpha_of(gamma_0)
    mu_x = 1. / alpha_0[pm] * (z - sigma_0[pm] * net_out)
    xh_phar, xh_pocket = ref_cpu.sample_normal_zero_com(mu_x, P, sigma_x, pm, qm, draw(shape)[urow], nd)
    x_phar = xh_phar[:, :nd] * nv[0]
    h_phar = torch.nn.functional.one_hot(torch.argmax(z[:, nd:] * nv[1] + nb[1], dim=1), pnf)
    x_pocket = xh_pocket[:, :nd] * nv[0]
    h_pocket = xh_pocket[:, nd:] * nv[1] + nb[1]
    if checks:
        ref_cpu.assert_mean_zero_with_mask(x_phar, pm)
    if ref_cpu.scatter_add(x_phar, pm).abs().max().item() > 5e-2:                            # batch-wide, as the single chain
        x_phar, x_pocket = ref_cpu.remove_mean_batch(x_phar, x_pocket, pm, qm)
    fr = gr.first_rows()
    out = (torch.cat([x_phar, h_phar.to(FLOAT)], dim=1)[fr], torch.cat([x_pocket, h_pocket], dim=1), gr.unique_mask, qm)
    if return_steps:
        return out + (torch.stack(z_steps), torch.stack(p_steps), np.stack(margins))
    return out
