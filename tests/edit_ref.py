"""CPU model of ConditionalDDPM.edit (the edit chain; INTEGRATION.md, "Editing a given pharmacophore"), built only from
oracle.ref_cpu primitives: cond_inpaint_ref.cond_inpaint's op sequence with one mask per column group and a start level, so
with both masks equal and start = timesteps it reproduces cond_inpaint bit for bit given the same draws."""
import torch

from oracle import ref_cpu
from oracle.ref_cpu import FLOAT, INT


def edit_plan(resamplings, jump_length, timesteps, start=None):
    """(ops, draws, jumps) of a chain that starts at level `start`: draw 0, per op A and B (and C before a jump back), the
    decode draw - n_draws = 2 + 2 n_steps + n_jumps for the schedule actually walked."""
    start = timesteps if start is None else start
    if not 1 <= start <= timesteps:
        raise ValueError(f'start={start} must be in [1, timesteps={timesteps}]')
    schedule = ref_cpu.get_repaint_schedule(resamplings, jump_length, start)
    n_steps, n_jumps = sum(schedule), len(schedule) - 1
    return n_steps, 2 + 2 * n_steps + n_jumps, n_jumps


def cond_edit(p, cfg, phar, pocket, fix_x, fix_h, start=None, resamplings=1, jump_length=1, timesteps=None, noise=None,
              return_steps=False, checks=True):
    """-> (xh_phar, xh_pocket, phar_mask, pocket_mask[, z_steps, pocket_steps]); noise(shape) supplies each draw in call order."""
    T, nd, pnf = cfg['timesteps'], cfg['n_dims'], cfg['phar_nf']
    nv, nb = cfg['norm_values'], cfg['norm_biases']
    table = ref_cpu.gamma_source(p)
    timesteps = T if timesteps is None else timesteps
    start = timesteps if start is None else start
    edit_plan(resamplings, jump_length, timesteps, start)           # the range check
    draw = noise if noise is not None else (lambda shape: torch.randn(shape))
    B = len(pocket['size'])
    pm, qm = phar['mask'].to(INT), pocket['mask'].to(INT)
    # normalize (en_diffusion.py:874-889), both inputs
    px = pocket['x'].to(FLOAT) / nv[0]
    xh0_pocket = torch.cat([px, (pocket['one_hot'].float() - nb[1]) / nv[1]], dim=1)
    known = torch.cat([phar['x'].to(FLOAT) / nv[0], (phar['one_hot'].float() - nb[1]) / nv[1]], dim=1)
    fx = torch.as_tensor(fix_x).to(FLOAT).reshape(-1) != 0
    fh = torch.as_tensor(fix_h).to(FLOAT).reshape(-1) != 0
    col_fixed = torch.cat([fx[:, None].expand(-1, nd), fh[:, None].expand(-1, pnf)], dim=1)
    has_mark = torch.zeros(B, dtype=torch.bool)
    has_mark[pm[fx | fh]] = True
    rows_m, rows_q = has_mark[pm], has_mark[qm]
    shape = (len(pm), nd + pnf)
    if start == timesteps:
        # from the prior, as ref_cpu.sample_given_pocket
        mu_phar = torch.cat((ref_cpu.scatter_mean(px, qm), torch.zeros((B, pnf))), dim=1)[pm]
        sigma = torch.ones_like(pocket['size']).unsqueeze(1)
        z, P = ref_cpu.sample_normal_zero_com(mu_phar, xh0_pocket, sigma, pm, qm, draw(shape), nd)
    else:
        # part-way: q(z_start | x) of the given rows, as ConditionalDDPM.forward (conditional_model.py:235-243, :158-179)
        xh0, P0c = known.clone(), xh0_pocket.clone()
        xh0[:, :nd], P0c[:, :nd] = ref_cpu.remove_mean_batch(known[:, :nd], xh0_pocket[:, :nd], pm, qm)
        gamma_t = ref_cpu.gamma_lookup(table, torch.full((B, 1), fill_value=start) / timesteps, T)
        z = ref_cpu.alpha_of(gamma_t)[pm] * xh0 + ref_cpu.sigma_of(gamma_t)[pm] * draw(shape)
        P = P0c.clone()
        z[:, :nd], P[:, :nd] = ref_cpu.remove_mean_batch(z[:, :nd], P0c[:, :nd], pm, qm)
    if checks:
        ref_cpu.assert_mean_zero_with_mask(z[:, :nd], pm)
    com0 = ref_cpu.scatter_mean(px, qm, B)
    schedule = ref_cpu.get_repaint_schedule(resamplings, jump_length, start)
    z_steps, p_steps = [], []
    s = start - 1
    for i, n_denoise_steps in enumerate(schedule):
        for j in range(n_denoise_steps):
            s_array = torch.full((B, 1), fill_value=s)
            t_array = s_array + 1
            s_array = s_array / timesteps
            t_array = t_array / timesteps
            # A: sample_p_zs_given_zt, as in ref_cpu.sample_given_pocket
            gamma_s = ref_cpu.gamma_lookup(table, s_array, T)
            gamma_t = ref_cpu.gamma_lookup(table, t_array, T)
            sigma2_ts, sigma_ts, alpha_ts = ref_cpu.sigma_and_alpha_t_given_s(gamma_t, gamma_s)
            sigma_s, sigma_t = ref_cpu.sigma_of(gamma_s), ref_cpu.sigma_of(gamma_t)
            eps_t, _ = ref_cpu.dynamics_forward(p, cfg, z, P, t_array, pm, qm)
            mu = z / alpha_ts[pm] - (sigma2_ts / alpha_ts / sigma_t)[pm] * eps_t
            sig = sigma_ts * sigma_s / sigma_t
            if checks:
                ref_cpu.assert_mean_zero_with_mask(z[:, :nd], pm)
            z_u, P_u = ref_cpu.sample_normal_zero_com(mu, P, sig, pm, qm, draw(shape), nd)
            # B: the noised known rows in the current frame replace the held column groups, then the projection
            eps_b = draw(shape)
            alpha_s = ref_cpu.alpha_of(gamma_s)
            z_k = alpha_s[pm] * known + sigma_s[pm] * eps_b
            z_k[:, :nd] = z_k[:, :nd] + (ref_cpu.scatter_mean(P_u[:, :nd], qm, B) - com0)[pm]
            z_m = torch.where(col_fixed, z_k, z_u)
            P_m = P_u.clone()
            z_m[:, :nd], P_m[:, :nd] = ref_cpu.remove_mean_batch(z_m[:, :nd], P_u[:, :nd], pm, qm)
            z = torch.where(rows_m[:, None], z_m, z_u)          # samples without a mark skip the merge
            P = torch.where(rows_q[:, None], P_m, P_u)
            if return_steps:
                z_steps.append(z.clone())
                p_steps.append(P[:, :nd].clone())
            # C: jump back (sample_p_zt_given_zs, conditional_model.py:330-340)
            if j == n_denoise_steps - 1 and i < len(schedule) - 1:
                t = s + jump_length
                gamma_t2 = ref_cpu.gamma_lookup(table, torch.full((B, 1), fill_value=t) / timesteps, T)
                _, sigma_ts2, alpha_ts2 = ref_cpu.sigma_and_alpha_t_given_s(gamma_t2, gamma_s)
                z, P = ref_cpu.sample_normal_zero_com(alpha_ts2[pm] * z, P, sigma_ts2, pm, qm, draw(shape), nd)
                s = t
            s -= 1
    # decode, as ref_cpu.sample_given_pocket
    t_zeros = torch.zeros((B, 1))
    gamma_0 = ref_cpu.gamma_lookup(table, t_zeros, T)
    sigma_x = torch.exp(-(-0.5 * gamma_0))
    net_out, _ = ref_cpu.dynamics_forward(p, cfg, z, P, t_zeros, pm, qm)
    sigma_0, alpha_0 = ref_cpu.sigma_of(gamma_0), ref_cpu.alpha_of(gamma_0)
    mu_x = 1. / alpha_0[pm] * (z - sigma_0[pm] * net_out)
    xh_phar, xh_pocket = ref_cpu.sample_normal_zero_com(mu_x, P, sigma_x, pm, qm, draw(shape), nd)
    x_phar = xh_phar[:, :nd] * nv[0]
    h_phar = torch.nn.functional.one_hot(torch.argmax(z[:, nd:] * nv[1] + nb[1], dim=1), pnf)
    x_pocket = xh_pocket[:, :nd] * nv[0]
    h_pocket = xh_pocket[:, nd:] * nv[1] + nb[1]
    if checks:
        ref_cpu.assert_mean_zero_with_mask(x_phar, pm)
    if ref_cpu.scatter_add(x_phar, pm).abs().max().item() > 5e-2:
        x_phar, x_pocket = ref_cpu.remove_mean_batch(x_phar, x_pocket, pm, qm)
    out = (torch.cat([x_phar, h_phar.to(FLOAT)], dim=1), torch.cat([x_pocket, h_pocket], dim=1), pm, qm)
    if return_steps:
        return out + (torch.stack(z_steps), torch.stack(p_steps))
    return out
