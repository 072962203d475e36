"""CPU model of editing under restraints (ConditionalDDPM.edit_restrained, cmdgen_restrained_edit_chain; INTEGRATION.md, "Editing under
restraints"), built only from oracle.ref_cpu primitives and restraint_ref.energy_terms in torch fp32: edit_ref.cond_edit's op sequence with the
guidance of restraint_ref.restrained_chain in op A.  A row whose x columns are held enters the energy at its given position moved into the
current frame and receives no displacement.

Given the same draws it reproduces edit_ref.cond_edit bit for bit with scale = 0 or without restraints, and restraint_ref.restrained_chain bit
for bit without marks, from the prior and without jumps (the B draws are then read and not used)."""
import numpy as np
import torch

from multi_pocket_ref import pair_margins
from oracle import ref_cpu
from oracle.ref_cpu import FLOAT, INT
from restraint_ref import _norm, energy_terms, touched_samples


def op_terms(z, P, eps_t, known, fx, sigma_t, alpha_t, com_in, pm, qm, rec, clash_r, clash_k, n_x, nd):
    """Steps 1-3 of one op: -> (xhat [Nl, 3] (A), shift [B, 3] (A), E [B], g [Nl, 3], largest violation per kind [4]).  z, P: the op's input;
    eps_t: the network's output; known: the normalised given rows; fx [Nl] bool: the rows whose x columns are held."""
    B = com_in.shape[0]
    shift = n_x * (ref_cpu.scatter_mean(P[:, :nd], qm, B) - com_in)                               # 2.
    xhat = n_x * (z[:, :nd] - sigma_t[pm] * eps_t[:, :nd]) / alpha_t[pm]                           # 1. free rows
    held = n_x * known[:, :nd] + shift[pm]                                                         #    held rows: the given position in this frame
    xhat = torch.where(fx[:, None], held, xhat)
    E, g, _, vk = energy_terms(xhat, n_x * P[:, :nd], shift, pm, qm, rec, clash_r, clash_k)        # 3.
    return xhat, shift, E, g, vk


def restrained_edit(p, cfg, phar, pocket, fix_x, fix_h, rec, clash_r=0.0, clash_k=0.0, scale=1.0, max_shift=1.0, guide_below=1.0, start=None,
                    resamplings=1, jump_length=1, timesteps=None, noise=None, checks=True, probe=None):
    """-> dict(xh_phar, xh_pocket, phar_mask, pocket_mask, z_steps [n_steps, Nl, 3+P], pocket_steps [n_steps, Np, 3], margins [n_steps + 1, B]
    (A, one row per evaluation), op_energy [n_steps, B], energy [B], max_violation [B], kind_violation [n_steps, 4], known_steps [n_steps, Nl, 3]:
    the x of the noised known rows in the frame of the saved step - what the x-held rows of z_steps are, up to rounding).  noise(shape) supplies
    each draw in call order.
    probe(op index, dict of the op's inputs): called before the guidance of every op (tests look at single ops through it)."""
    T, nd, pnf = cfg['timesteps'], cfg['n_dims'], cfg['phar_nf']
    nv, nb = cfg['norm_values'], cfg['norm_biases']
    assert not cfg.get('no_com_projection', False) and not cfg.get('update_pocket_coords', False)
    table = ref_cpu.gamma_source(p)
    timesteps = T if timesteps is None else timesteps
    start = timesteps if start is None else start
    if not 1 <= start <= timesteps:
        raise ValueError(f'start={start} must be in [1, timesteps={timesteps}]')
    draw = noise if noise is not None else (lambda shape: torch.randn(shape))
    B = len(pocket['size'])
    n_x = nv[0]
    pm, qm = phar['mask'].to(INT), pocket['mask'].to(INT)
    px = pocket['x'].to(FLOAT) / n_x
    xh0_pocket = torch.cat([px, (pocket['one_hot'].float() - nb[1]) / nv[1]], dim=1)
    known = torch.cat([phar['x'].to(FLOAT) / n_x, (phar['one_hot'].float() - nb[1]) / nv[1]], dim=1)
    fx = torch.as_tensor(fix_x).to(FLOAT).reshape(-1) != 0
    fh = torch.as_tensor(fix_h).to(FLOAT).reshape(-1) != 0
    col_fixed = torch.cat([fx[:, None].expand(-1, nd), fh[:, None].expand(-1, pnf)], dim=1)
    has_mark = torch.zeros(B, dtype=torch.bool)
    has_mark[pm[fx | fh]] = True
    rows_m, rows_q = has_mark[pm], has_mark[qm]
    shape = (len(pm), nd + pnf)
    com_in = ref_cpu.scatter_mean(px, qm, B)                                     # com(P_in.x / n_x) = edit_ref's com0
    if start == timesteps:
        mu_phar = torch.cat((ref_cpu.scatter_mean(px, qm), torch.zeros((B, pnf))), dim=1)[pm]
        sigma = torch.ones_like(pocket['size']).unsqueeze(1)
        z, P = ref_cpu.sample_normal_zero_com(mu_phar, xh0_pocket, sigma, pm, qm, draw(shape), nd)
    else:
        xh0, P0c = known.clone(), xh0_pocket.clone()
        xh0[:, :nd], P0c[:, :nd] = ref_cpu.remove_mean_batch(known[:, :nd], xh0_pocket[:, :nd], pm, qm)
        gamma_t = ref_cpu.gamma_lookup(table, torch.full((B, 1), fill_value=start) / timesteps, T)
        z = ref_cpu.alpha_of(gamma_t)[pm] * xh0 + ref_cpu.sigma_of(gamma_t)[pm] * draw(shape)
        P = P0c.clone()
        z[:, :nd], P[:, :nd] = ref_cpu.remove_mean_batch(z[:, :nd], P0c[:, :nd], pm, qm)
    if checks:
        ref_cpu.assert_mean_zero_with_mask(z[:, :nd], pm)
    touched = torch.from_numpy(touched_samples(rec, B, clash_r))
    any_touched = bool(touched.any())
    schedule = ref_cpu.get_repaint_schedule(resamplings, jump_length, start)
    z_steps, p_steps, k_steps, margins, op_energy, kind_v = [], [], [], [], [], []
    op = 0
    s = start - 1
    for i, n_denoise_steps in enumerate(schedule):
        for j in range(n_denoise_steps):
            s_array = torch.full((B, 1), fill_value=s)
            t_array = s_array + 1
            s_array = s_array / timesteps
            t_array = t_array / timesteps
            # A: sample_p_zs_given_zt with the guidance term in its mean
            gamma_s = ref_cpu.gamma_lookup(table, s_array, T)
            gamma_t = ref_cpu.gamma_lookup(table, t_array, T)
            sigma2_ts, sigma_ts, alpha_ts = ref_cpu.sigma_and_alpha_t_given_s(gamma_t, gamma_s)
            sigma_s, sigma_t = ref_cpu.sigma_of(gamma_s), ref_cpu.sigma_of(gamma_t)
            alpha_t = ref_cpu.alpha_of(gamma_t)
            margins.append(pair_margins(z[:, :nd], P[:, :nd], pm, qm, cfg['edge_cutoff']) * n_x)
            eps_t, _ = ref_cpu.dynamics_forward(p, cfg, z, P, t_array, pm, qm)
            mu = z / alpha_ts[pm] - (sigma2_ts / alpha_ts / sigma_t)[pm] * eps_t
            sig = sigma_ts * sigma_s / sigma_t
            E = torch.zeros(B)
            vk = torch.zeros(4)
            if probe is not None:
                probe(op, dict(z=z, P=P, eps_t=eps_t, known=known, fx=fx, sigma_t=sigma_t, alpha_t=alpha_t, com_in=com_in, pm=pm, qm=qm))
            if any_touched:
                _, _, E, g, vk = op_terms(z, P, eps_t, known, fx, sigma_t, alpha_t, com_in, pm, qm, rec, clash_r, clash_k, n_x, nd)
                var = (n_x * sig) ** 2
                d = -scale * var[pm] * g                                                           # 4.
                length = _norm(d)
                over = length > max_shift
                d = torch.where(over[:, None], d * (max_shift / length.clamp(min=1e-30))[:, None], d)
                active = touched[pm] & (t_array[pm][:, 0] <= guide_below) & (scale > 0) & ~fx       # a held row gets nothing added
                rows = torch.nonzero(active).reshape(-1)
                if len(rows):
                    mu[rows, :nd] = mu[rows, :nd] + d[rows] / n_x                                  # 5.
            op_energy.append(E)
            kind_v.append(vk)
            if checks:
                ref_cpu.assert_mean_zero_with_mask(z[:, :nd], pm)
            z_u, P_u = ref_cpu.sample_normal_zero_com(mu, P, sig, pm, qm, draw(shape), nd)
            # B: as edit_ref.cond_edit
            eps_b = draw(shape)
            alpha_s = ref_cpu.alpha_of(gamma_s)
            z_k = alpha_s[pm] * known + sigma_s[pm] * eps_b
            z_k[:, :nd] = z_k[:, :nd] + (ref_cpu.scatter_mean(P_u[:, :nd], qm, B) - com_in)[pm]
            z_m = torch.where(col_fixed, z_k, z_u)
            P_m = P_u.clone()
            z_m[:, :nd], P_m[:, :nd] = ref_cpu.remove_mean_batch(z_m[:, :nd], P_u[:, :nd], pm, qm)
            z = torch.where(rows_m[:, None], z_m, z_u)
            P = torch.where(rows_q[:, None], P_m, P_u)
            z_steps.append(z.clone())
            p_steps.append(P[:, :nd].clone())
            # the noised known rows in the frame of the saved step (what the held rows of z are, up to rounding)
            k_steps.append(z_k[:, :nd] - (ref_cpu.scatter_mean(P_u[:, :nd], qm, B) - ref_cpu.scatter_mean(P[:, :nd], qm, B))[pm])
            # C: jump back, not guided
            if j == n_denoise_steps - 1 and i < len(schedule) - 1:
                t = s + jump_length
                gamma_t2 = ref_cpu.gamma_lookup(table, torch.full((B, 1), fill_value=t) / timesteps, T)
                _, sigma_ts2, alpha_ts2 = ref_cpu.sigma_and_alpha_t_given_s(gamma_t2, gamma_s)
                z, P = ref_cpu.sample_normal_zero_com(alpha_ts2[pm] * z, P, sigma_ts2, pm, qm, draw(shape), nd)
                s = t
            s -= 1
            op += 1
    # decode, not guided
    t_zeros = torch.zeros((B, 1))
    gamma_0 = ref_cpu.gamma_lookup(table, t_zeros, T)
    sigma_x = torch.exp(-(-0.5 * gamma_0))
    margins.append(pair_margins(z[:, :nd], P[:, :nd], pm, qm, cfg['edge_cutoff']) * n_x)
    net_out, _ = ref_cpu.dynamics_forward(p, cfg, z, P, t_zeros, pm, qm)
    sigma_0, alpha_0 = ref_cpu.sigma_of(gamma_0), ref_cpu.alpha_of(gamma_0)
    mu_x = 1. / alpha_0[pm] * (z - sigma_0[pm] * net_out)
    xh_phar, xh_pocket = ref_cpu.sample_normal_zero_com(mu_x, P, sigma_x, pm, qm, draw(shape), nd)
    x_phar = xh_phar[:, :nd] * n_x
    h_phar = torch.nn.functional.one_hot(torch.argmax(z[:, nd:] * nv[1] + nb[1], dim=1), pnf)
    x_pocket = xh_pocket[:, :nd] * n_x
    h_pocket = xh_pocket[:, nd:] * nv[1] + nb[1]
    if checks:
        ref_cpu.assert_mean_zero_with_mask(x_phar, pm)
    if ref_cpu.scatter_add(x_phar, pm).abs().max().item() > 5e-2:
        x_phar, x_pocket = ref_cpu.remove_mean_batch(x_phar, x_pocket, pm, qm)
    # the diagnostics of the returned sample (held points at their returned positions): shift from the returned pocket
    shift = ref_cpu.scatter_mean(x_pocket, qm, B) - n_x * com_in
    E_fin, _, v_fin, _ = energy_terms(x_phar, x_pocket, shift, pm, qm, rec, clash_r, clash_k)
    return dict(xh_phar=torch.cat([x_phar, h_phar.to(FLOAT)], dim=1), xh_pocket=torch.cat([x_pocket, h_pocket], dim=1), phar_mask=pm,
                pocket_mask=qm, z_steps=torch.stack(z_steps), pocket_steps=torch.stack(p_steps), known_steps=torch.stack(k_steps),
                margins=np.stack(margins), op_energy=torch.stack(op_energy), energy=E_fin, max_violation=v_fin,
                kind_violation=torch.stack(kind_v))
