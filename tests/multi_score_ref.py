"""CPU model of the multi-pocket scoring chain (ConditionalDDPM.score_given_pockets, cmdgen_multi_score_chain), composed from the
oracle's pieces: score_ref.score_levels' per-level arithmetic over the MEMBER samples of multi_pocket_ref.Groups, every member
holding a copy of its group's clean rows and draws, with the members' eps rows combined by Groups.combine before the group's sums.

Level k of group g (normalised space, everything centred on the centre of mass of the group's phar rows):
    z_k = alpha xh0_g + sigma eps_k, remove_mean_batch per member;  eps_m = dynamics(z_k, P_m, t / T) over the B members as one batch;
    eps_bar = sum_m w_m eps_m;  group sums over (eps_k - eps_bar)^2, member sums over (eps_k - eps_m)^2.
With groups of one this IS score_ref.score_levels, bit for bit: the evaluation is the same call on the same batch and w = 1.

The categorical term of the t = 0 level is given twice.  'log_ph' is the model's: sum of log p(h | z_0) * one_hot, the weight being
the NORMALISED one-hot un-normalised again, (h - b) / v * v + b - conditional_model.py:81 on the dict that normalize() has rewritten
in place (:203), the expression of the oracle's own joint model (ref_cpu's cat_logp).  'log_ph_oracle' is score_ref.score_levels'
expression, which un-normalises the RAW one-hot (ref_cpu.ddpm_forward's l0_terms) and so carries a factor norm_values[1]: it equals
the model's only where norm_values[1] = 1 or the term is 0 (as it is, exactly, in the G21 vectors).  The exact reduction to
score_ref.score_levels holds for 'log_ph_oracle'; the device is compared with 'log_ph'.
"""
import numpy as np
import torch

import multi_pocket_ref as mp
from oracle.ref_cpu import (FLOAT, INT, alpha_of, dynamics_forward, gamma_lookup, gamma_source, remove_mean_batch, sigma_of,
                            _cdf_std_gauss, _sum_except_batch)

BAND = 1e-4            # A: a (level, group) entry with a pair of any member closer than this to the cutoff may be left out
CAP = 0.02             # ... but at most this share of a case's entries (the scoring tests' cap)


def member_inputs(groups, phar_x, phar_onehot, noise=None):
    """The [Nu] rows of the groups (and the [n_levels, Nu, C] draws) gathered onto the member layout: the phar dict a single
    scoring chain over the B members takes, and its draws."""
    urow = groups.urow
    phar = {'x': torch.as_tensor(phar_x)[urow], 'one_hot': torch.as_tensor(phar_onehot)[urow],
            'size': torch.from_numpy(groups.member_nph), 'mask': groups.phar_mask}
    return (phar, torch.as_tensor(noise)[:, urow]) if noise is not None else phar


def score_levels(p, cfg, groups, phar_x, phar_onehot, pocket, weights, t_levels, noise):
    """groups: multi_pocket_ref.Groups; phar_x [Nu, 3], phar_onehot [Nu, P] raw rows, one copy per group; pocket: dict(x, one_hot,
    size [B], mask) of the member samples; weights [B]; noise [n_levels, Nu, 3 + P].
    -> dict: group / member: dicts of err, err_x, log_ph, log_ph_oracle, netmax [n_levels, G] / [n_levels, B] (a group's netmax is the largest over
    its members); kl_sums [G, 2]; z [n_levels, Nl, 3 + P] and pocket_x [n_levels, Np, 3] of the members; margins [n_levels, B] in A;
    keep [n_levels, G]."""
    T, nd, nv, nb = cfg['timesteps'], cfg['n_dims'], cfg['norm_values'], cfg['norm_biases']
    gr = groups
    B, G = gr.B, gr.G
    table = gamma_source(p)
    w = torch.as_tensor(weights).to(FLOAT).reshape(-1)
    assert len(w) == B and len(pocket['size']) == B
    phar = member_inputs(gr, phar_x, phar_onehot)
    pm, qm, um = gr.phar_mask.to(INT), pocket['mask'].to(INT), gr.unique_mask.to(INT)
    # score_ref.score_levels' preparation on the member layout: every member centres on its own copy of the group's rows
    x_l = phar['x'].to(FLOAT) / nv[0]
    h_l = (phar['one_hot'].float() - nb[1]) / nv[1]
    x_p = pocket['x'].to(FLOAT) / nv[0]
    h_p = (pocket['one_hot'].float() - nb[1]) / nv[1]
    xh0_l, xh0_p = torch.cat([x_l, h_l], dim=1), torch.cat([x_p, h_p], dim=1)
    a, b = remove_mean_batch(xh0_l[:, :nd], xh0_p[:, :nd], pm, qm)
    xh0_l, xh0_p = torch.cat([a, xh0_l[:, nd:]], dim=1), torch.cat([b, xh0_p[:, nd:]], dim=1)
    fr = gr.first_rows()
    first = torch.from_numpy(gr.first)
    names = ('err', 'err_x', 'log_ph', 'log_ph_oracle', 'netmax')
    out_g, out_m = {k: [] for k in names}, {k: [] for k in names}
    zs, pxs, margins = [], [], []
    for t_i, eps_u in zip(t_levels, noise):
        eps_u = torch.as_tensor(eps_u)
        eps = eps_u[gr.urow]
        t = torch.full((B, 1), float(t_i)) / T
        gamma_t = gamma_lookup(table, t, T)
        z = alpha_of(gamma_t)[pm] * xh0_l + sigma_of(gamma_t)[pm] * eps
        zx, px = remove_mean_batch(z[:, :nd], xh0_p[:, :nd], pm, qm)
        z, xp = torch.cat([zx, z[:, nd:]], dim=1), torch.cat([px, xh0_p[:, nd:]], dim=1)
        net, _ = dynamics_forward(p, cfg, z, xp, t, pm, qm)            # one batch: its NaN reset is batch-wide
        bar = gr.combine(net, w)                                        # [Nu, C]
        out_m['err'].append(_sum_except_batch((eps - net) ** 2, pm, B))
        out_m['err_x'].append(_sum_except_batch((eps[:, :nd] - net[:, :nd]) ** 2, pm, B))
        out_g['err'].append(_sum_except_batch((eps_u - bar) ** 2, um, G))
        out_g['err_x'].append(_sum_except_batch((eps_u[:, :nd] - bar[:, :nd]) ** 2, um, G))
        if t_i == 0:                                                    # l0_terms, as score_ref.score_levels
            sigma_0_cat = sigma_of(gamma_t) * nv[1]
            onehot = phar['one_hot'].float() * nv[1] + nb[1]
            c = z[:, nd:] * nv[1] + nb[1] - 1
            logp = torch.log(_cdf_std_gauss((c + 0.5) / sigma_0_cat[pm]) - _cdf_std_gauss((c - 0.5) / sigma_0_cat[pm]) + 1e-10)
            logp = logp - torch.logsumexp(logp, dim=1, keepdim=True)
            lph_oracle = _sum_except_batch(logp * onehot, pm, B)
            lph = _sum_except_batch(logp * (h_l * nv[1] + nb[1]), pm, B)    # the model's weight: the one-hot itself
        else:
            lph = lph_oracle = torch.zeros(B)
        for name, v in (('log_ph', lph), ('log_ph_oracle', lph_oracle)):
            out_m[name].append(v)
            out_g[name].append(v[first])                                # z and the rows are the group's: every member's value is the same
        nmax = torch.stack([net[pm == i].abs().max() for i in range(B)])
        out_m['netmax'].append(nmax)
        out_g['netmax'].append(torch.stack([nmax[f:f + m].max() for f, m in zip(gr.first, gr.sizes)]))
        zs.append(z)
        pxs.append(px)
        margins.append(mp.pair_margins(z[:, :nd], px, pm, qm, cfg['edge_cutoff']) * nv[0])
    gamma_T = gamma_lookup(table, torch.ones((B, 1)), T)
    mu_T = alpha_of(gamma_T)[pm] * xh0_l
    kl_m = torch.stack([_sum_except_batch(mu_T[:, :nd] ** 2, pm, B), _sum_except_batch(mu_T[:, nd:] ** 2, pm, B)], dim=1)
    margins = np.stack(margins)
    keep = np.stack([[margins[k, f:f + m].min() >= BAND for f, m in zip(gr.first, gr.sizes)] for k in range(len(margins))])
    return {'group': {k: torch.stack(v) for k, v in out_g.items()}, 'member': {k: torch.stack(v) for k, v in out_m.items()},
            'kl_sums': kl_m[first], 'member_kl_sums': kl_m, 'z': torch.stack(zs), 'pocket_x': torch.stack(pxs), 'margins': margins,
            'keep': keep, 'first_rows': fr}
