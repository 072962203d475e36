"""CPU model of the multi-pocket edit chain (ConditionalDDPM.edit_given_pockets, cmdgen_multi_edit_chain; INTEGRATION.md, "Holding or
editing given points for several pockets"), built only from oracle.ref_cpu primitives: multi_pocket_ref.multi_pocket_chain's grouping
and eps combination with edit_ref.cond_edit's op sequence.  Every member of a group holds a copy of the group's latent; the known
rows, the marks and the draws hold ONE copy of the rows per group (Nu rows).  The pocket offset of step B is the GROUP's: the shift of
the group's first member's pocket, com(P_first) - com(P0_first), used by every member.

With groups of one member it reproduces edit_ref.cond_edit, and with no mark, start = timesteps and resamplings = jump_length = 1
multi_pocket_ref.multi_pocket_chain, both bit for bit given the same draws."""
import numpy as np
import torch

from oracle import ref_cpu
from oracle.ref_cpu import FLOAT, INT
from edit_ref import edit_plan
from multi_pocket_ref import Groups, pair_margins


def multi_edit_chain(p, cfg, phar, pocket, group_sizes, weights, fix_x, fix_h, start=None, resamplings=1, jump_length=1,
                     timesteps=None, noise=None, return_steps=False, checks=True):
    """phar: dict(x [Nu,3], one_hot [Nu,P], size [G]) one copy of the rows per group, in the pockets' common frame; pocket:
    dict(x, one_hot, size [B], mask) of the member samples; weights [B]; fix_x, fix_h [Nu]; noise(shape) supplies each draw of shape
    (Nu, 3 + P) in edit_ref.cond_edit's call order.
    -> (xh_phar [Nu, 3+P], xh_pocket [Np, 3+R], unique phar mask [Nu], pocket mask[, z_steps [n_steps, Nu, 3+P], pocket_steps
    [n_steps, Np, 3], margins [n_steps + 1, B]])."""
    T, nd, pnf = cfg['timesteps'], cfg['n_dims'], cfg['phar_nf']
    nv, nb = cfg['norm_values'], cfg['norm_biases']
    assert not cfg.get('no_com_projection', False) and not cfg.get('update_pocket_coords', False)
    table = ref_cpu.gamma_source(p)
    timesteps = T if timesteps is None else timesteps
    start = timesteps if start is None else start
    edit_plan(resamplings, jump_length, timesteps, start)           # the range check
    gr = Groups(group_sizes, np.asarray(phar['size']).reshape(-1))
    B = gr.B
    assert len(pocket['size']) == B
    w = torch.as_tensor(weights).to(FLOAT).reshape(-1)
    assert len(w) == B
    draw = noise if noise is not None else (lambda shape: torch.randn(shape))
    pm, qm, urow = gr.phar_mask, pocket['mask'].to(INT), gr.urow
    group_of = torch.from_numpy(gr.group_of)
    first_of = torch.from_numpy(gr.first)[group_of]                 # [B] the first member of a member's group
    shape = (gr.Nu, nd + pnf)
    # normalize (en_diffusion.py:874-889), both inputs; the known rows and the marks on every member's rows
    px = pocket['x'].to(FLOAT) / nv[0]
    xh0_pocket = torch.cat([px, (pocket['one_hot'].float() - nb[1]) / nv[1]], dim=1)
    known = torch.cat([phar['x'].to(FLOAT) / nv[0], (phar['one_hot'].float() - nb[1]) / nv[1]], dim=1)[urow]
    fx = (torch.as_tensor(fix_x).to(FLOAT).reshape(-1) != 0)[urow]
    fh = (torch.as_tensor(fix_h).to(FLOAT).reshape(-1) != 0)[urow]
    col_fixed = torch.cat([fx[:, None].expand(-1, nd), fh[:, None].expand(-1, pnf)], dim=1)
    has_mark = torch.zeros(B, dtype=torch.bool)
    has_mark[pm[fx | fh]] = True
    rows_m, rows_q = has_mark[pm], has_mark[qm]
    if start == timesteps:
        # from the prior, as multi_pocket_ref.multi_pocket_chain
        c = gr.combine_members(ref_cpu.scatter_mean(px, qm, B), w)
        mu_phar = torch.cat((c, torch.zeros((gr.G, pnf))), dim=1)[group_of][pm]
        sigma = torch.ones_like(pocket['size']).unsqueeze(1)
        z, P = ref_cpu.sample_normal_zero_com(mu_phar, xh0_pocket, sigma, pm, qm, draw(shape)[urow], nd)
    else:
        # part-way, as edit_ref.cond_edit: every member's pocket centred on the centre of mass of the group's given rows
        xh0, P0c = known.clone(), xh0_pocket.clone()
        xh0[:, :nd], P0c[:, :nd] = ref_cpu.remove_mean_batch(known[:, :nd], xh0_pocket[:, :nd], pm, qm)
        gamma_t = ref_cpu.gamma_lookup(table, torch.full((B, 1), fill_value=start) / timesteps, T)
        z = ref_cpu.alpha_of(gamma_t)[pm] * xh0 + ref_cpu.sigma_of(gamma_t)[pm] * draw(shape)[urow]
        P = P0c.clone()
        z[:, :nd], P[:, :nd] = ref_cpu.remove_mean_batch(z[:, :nd], P0c[:, :nd], pm, qm)
    if checks:
        ref_cpu.assert_mean_zero_with_mask(z[:, :nd], pm)
    com0 = ref_cpu.scatter_mean(px, qm, B)
    z_steps, p_steps, margins = [], [], []

    # the members are evaluated slot by slot, as in multi_pocket_ref.multi_pocket_chain (which says why)
    slots = []
    for j, (u, r, b) in enumerate(gr.rows_of):
        members = torch.from_numpy(gr.first[gr.sizes > j] + j)
        renum = torch.full((B,), -1, dtype=INT)
        renum[members] = torch.arange(len(members))
        qrows = torch.nonzero(renum[qm] >= 0).reshape(-1)
        slots.append((r, members, renum[pm[r]], qrows, renum[qm[qrows]]))

    def eps_bar(t_array):
        if return_steps:
            margins.append(pair_margins(z[:, :nd], P[:, :nd], pm, qm, cfg['edge_cutoff']) * nv[0])
        eps = torch.empty_like(z)
        reset = False
        for r, members, pm_j, qrows, qm_j in slots:
            eps[r], _ = ref_cpu.dynamics_forward(p, cfg, z[r], P[qrows], t_array[members], pm_j, qm_j)
            reset = reset or (len(r) > 0 and not bool(eps[r][:, :nd].any()))
        if reset:
            eps[:, :nd] = 0.0
        return gr.combine(eps, w)[urow]

    schedule = ref_cpu.get_repaint_schedule(resamplings, jump_length, start)
    s = start - 1
    for i, n_denoise_steps in enumerate(schedule):
        for j in range(n_denoise_steps):
            s_array = torch.full((B, 1), fill_value=s)
            t_array = s_array + 1
            s_array = s_array / timesteps
            t_array = t_array / timesteps
            # A: the posterior step on eps_bar
            gamma_s = ref_cpu.gamma_lookup(table, s_array, T)
            gamma_t = ref_cpu.gamma_lookup(table, t_array, T)
            sigma2_ts, sigma_ts, alpha_ts = ref_cpu.sigma_and_alpha_t_given_s(gamma_t, gamma_s)
            sigma_s, sigma_t = ref_cpu.sigma_of(gamma_s), ref_cpu.sigma_of(gamma_t)
            mu = z / alpha_ts[pm] - (sigma2_ts / alpha_ts / sigma_t)[pm] * eps_bar(t_array)
            sig = sigma_ts * sigma_s / sigma_t
            if checks:
                ref_cpu.assert_mean_zero_with_mask(z[:, :nd], pm)
            z_u, P_u = ref_cpu.sample_normal_zero_com(mu, P, sig, pm, qm, draw(shape)[urow], nd)
            # B: the noised known rows, moved by the GROUP's offset (its first member's pocket shift), replace the held column groups
            eps_b = draw(shape)[urow]
            alpha_s = ref_cpu.alpha_of(gamma_s)
            z_k = alpha_s[pm] * known + sigma_s[pm] * eps_b
            off = (ref_cpu.scatter_mean(P_u[:, :nd], qm, B) - com0)[first_of]
            z_k[:, :nd] = z_k[:, :nd] + off[pm]
            z_m = torch.where(col_fixed, z_k, z_u)
            P_m = P_u.clone()
            z_m[:, :nd], P_m[:, :nd] = ref_cpu.remove_mean_batch(z_m[:, :nd], P_u[:, :nd], pm, qm)
            z = torch.where(rows_m[:, None], z_m, z_u)          # groups without a mark skip the merge
            P = torch.where(rows_q[:, None], P_m, P_u)
            if return_steps:
                z_steps.append(z[gr.first_rows()].clone())
                p_steps.append(P[:, :nd].clone())
            # C: jump back
            if j == n_denoise_steps - 1 and i < len(schedule) - 1:
                t = s + jump_length
                gamma_t2 = ref_cpu.gamma_lookup(table, torch.full((B, 1), fill_value=t) / timesteps, T)
                _, sigma_ts2, alpha_ts2 = ref_cpu.sigma_and_alpha_t_given_s(gamma_t2, gamma_s)
                z, P = ref_cpu.sample_normal_zero_com(alpha_ts2[pm] * z, P, sigma_ts2, pm, qm, draw(shape)[urow], nd)
                s = t
            s -= 1
    # decode, as multi_pocket_ref.multi_pocket_chain
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
    if ref_cpu.scatter_add(x_phar, pm).abs().max().item() > 5e-2:
        x_phar, x_pocket = ref_cpu.remove_mean_batch(x_phar, x_pocket, pm, qm)
    fr = gr.first_rows()
    out = (torch.cat([x_phar, h_phar.to(FLOAT)], dim=1)[fr], torch.cat([x_pocket, h_pocket], dim=1), gr.unique_mask, qm)
    if return_steps:
        return out + (torch.stack(z_steps), torch.stack(p_steps), np.stack(margins))
    return out
