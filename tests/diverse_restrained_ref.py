"""CPU model of diverse sampling under restraints (ConditionalDDPM.sample_diverse_restrained, cmdgen_diverse_restrained_chain; INTEGRATION.md,
"Diverse sampling under restraints"), built only from oracle.ref_cpu primitives in torch fp32: diverse_ref.diverse_chain's loop - which is
ref_cpu.sample_given_pocket's op sequence - with the restraint term (chain_ref.op_terms: steps 1-4 of csrc/kernels_restrain.hip's header) added
to the mean of op A in front of the overlap term (diverse_ref.overlap_terms: steps 1-3 of csrc/kernels_diverse.hip's header):

    mu.x_i = ((z.x_i / coef.x - coef.y e_i) + d^r_i / n_x) + d^v_i / n_x,

each addition made only on the rows where its term is active.  Both terms are taken at the same denoised estimate; each keeps the scalars of its
own chain.  The term functions are the parents', called, not copied.  With strength = 0 (or diverse_guide_below = 0, or sets of one) the loop
reproduces restraint_ref.restrained_chain bit for bit on the same draws; with scale = 0 (or no record and no clash) diverse_ref.diverse_chain."""
import numpy as np
import torch

from chain_ref import _norm, energy_terms, op_terms, pair_margins, touched_samples
from diverse_ref import overlap_terms, set_tables
from oracle import ref_cpu
from oracle.ref_cpu import FLOAT, INT


def diverse_restrained_chain(p, cfg, pocket, num_nodes_phar, set_sizes, rec, clash_r=0.0, clash_k=0.0, scale=1.0, max_shift=1.0,
                             guide_below=1.0, strength=1.0, width=2.0, diverse_max_shift=1.0, diverse_guide_below=1.0, timesteps=None,
                             noise=None, checks=True):
    """pocket: dict(x, one_hot, size [B], mask); rec: the record array of cmdgen_amd.restraints.records; noise(shape) supplies each draw in
    call order: draw 0, one per op, the decode draw.
    -> dict(xh_phar, xh_pocket, phar_mask, pocket_mask, z_steps [K, Nl, 3+P], pocket_steps [K, Np, 3], margins [K + 1, B] (A, one row per
    evaluation), op_energy [K, B], energy [B], max_violation [B], op_overlap [K, B], overlap [B], clipped, total (the restraint term's
    displacements capped and made), diverse_clipped, diverse_total (the overlap term's))."""
    T, nd, pnf = cfg['timesteps'], cfg['n_dims'], cfg['phar_nf']
    nv, nb = cfg['norm_values'], cfg['norm_biases']
    n_x = nv[0]
    assert not cfg.get('no_com_projection', False) and not cfg.get('update_pocket_coords', False)
    table = ref_cpu.gamma_source(p)
    timesteps = T if timesteps is None else timesteps
    draw = noise if noise is not None else (lambda shape: torch.randn(shape))
    qm = pocket['mask'].to(INT)
    B = len(pocket['size'])
    pm = torch.repeat_interleave(torch.arange(B), torch.as_tensor(num_nodes_phar).to(INT))
    _, M = set_tables(set_sizes, B)
    coupled = (M > 1)[pm]                                                              # [Nl] rows of a set of at least two
    touched = torch.from_numpy(touched_samples(rec, B, clash_r))                       # [B] samples a restraint (or the clash term) touches
    any_touched = bool(touched.any())
    shape = (len(pm), nd + pnf)
    # normalize (en_diffusion.py:874-889)
    px = pocket['x'].to(FLOAT) / n_x
    xh0_pocket = torch.cat([px, (pocket['one_hot'].float() - nb[1]) / nv[1]], dim=1)
    com0 = ref_cpu.scatter_mean(px, qm, B)                                             # com(P_in.x / n_x)
    # init: from the prior, as ref_cpu.sample_given_pocket
    mu_phar = torch.cat((com0, torch.zeros((B, pnf))), dim=1)[pm]
    sigma = torch.ones_like(pocket['size']).unsqueeze(1)
    z, P = ref_cpu.sample_normal_zero_com(mu_phar, xh0_pocket, sigma, pm, qm, draw(shape), nd)
    if checks:
        ref_cpu.assert_mean_zero_with_mask(z[:, :nd], pm)
    margins = []

    def evaluate(t_array):
        margins.append(pair_margins(z[:, :nd], P[:, :nd], pm, qm, cfg['edge_cutoff']) * n_x)   # (the graph is built on normalised x)
        return ref_cpu.dynamics_forward(p, cfg, z, P, t_array, pm, qm)[0]                       # (its x columns are zero when the NaN guard reset)

    def capped(d, cap):
        length = _norm(d)
        over = length > cap
        return torch.where(over[:, None], d * (cap / length.clamp(min=1e-30))[:, None], d), over

    z_steps, p_steps, op_energy, op_overlap = [], [], [], []
    clipped = total = d_clipped = d_total = 0
    for s in reversed(range(0, timesteps)):
        s_array = torch.full((B, 1), fill_value=s)
        t_array = s_array + 1
        s_array = s_array / timesteps
        t_array = t_array / timesteps
        # A: sample_p_zs_given_zt, as in ref_cpu.sample_given_pocket, with both terms in its mean
        gamma_s = ref_cpu.gamma_lookup(table, s_array, T)
        gamma_t = ref_cpu.gamma_lookup(table, t_array, T)
        sigma2_ts, sigma_ts, alpha_ts = ref_cpu.sigma_and_alpha_t_given_s(gamma_t, gamma_s)
        sigma_s, sigma_t = ref_cpu.sigma_of(gamma_s), ref_cpu.sigma_of(gamma_t)
        eps_t = evaluate(t_array)
        mu = z / alpha_ts[pm] - (sigma2_ts / alpha_ts / sigma_t)[pm] * eps_t
        sig = sigma_ts * sigma_s / sigma_t
        alpha_t = ref_cpu.alpha_of(gamma_t)
        var = (n_x * sig) ** 2
        # 1. the restraint term: chain_ref.run_chain's guide part, ungrouped and without held rows
        E = torch.zeros(B)
        if any_touched:
            _, _, E, g, _ = op_terms(z, P, eps_t, None, torch.zeros(len(pm), dtype=torch.bool), sigma_t, alpha_t, com0, pm, qm, rec, clash_r,
                                     clash_k, n_x, nd)
            d, over = capped(-scale * var[pm] * g, max_shift)
            active = touched[pm] & (t_array[pm][:, 0] <= guide_below) & (scale > 0)
            clipped += int((over & active).sum())
            total += int(active.sum())
            rows = torch.nonzero(active).reshape(-1)
            if len(rows):
                mu[rows, :nd] = mu[rows, :nd] + d[rows] / n_x                                   # (nothing is added to any other row)
        op_energy.append(E)
        # 2. the overlap term: diverse_ref.diverse_chain's, at the same estimate
        xhat = n_x * (z[:, :nd] - sigma_t[pm] * eps_t[:, :nd]) / alpha_t[pm]
        shift = n_x * (ref_cpu.scatter_mean(P[:, :nd], qm, B) - com0)
        _, ov, g, _ = overlap_terms(xhat - shift[pm], pm, set_sizes, strength, width)
        op_overlap.append(ov)
        d, over = capped(-var[pm] * g, diverse_max_shift)
        active = coupled & (t_array[pm][:, 0] <= diverse_guide_below) & (strength > 0)
        d_clipped += int((over & active).sum())
        d_total += int(active.sum())
        rows = torch.nonzero(active).reshape(-1)
        if len(rows):
            mu[rows, :nd] = mu[rows, :nd] + d[rows] / n_x                                       # 3. behind the restraint term's addition
        if checks:
            ref_cpu.assert_mean_zero_with_mask(z[:, :nd], pm)
        z, P = ref_cpu.sample_normal_zero_com(mu, P, sig, pm, qm, draw(shape), nd)
        z_steps.append(z.clone())
        p_steps.append(P[:, :nd].clone())

    # decode, not guided: as ref_cpu.sample_given_pocket
    t_zeros = torch.zeros((B, 1))
    gamma_0 = ref_cpu.gamma_lookup(table, t_zeros, T)
    sigma_x = torch.exp(-(-0.5 * gamma_0))
    net_out = evaluate(t_zeros)
    sigma_0, alpha_0 = ref_cpu.sigma_of(gamma_0), ref_cpu.alpha_of(gamma_0)
    mu_x = 1. / alpha_0[pm] * (z - sigma_0[pm] * net_out)
    xh_phar, xh_pocket = ref_cpu.sample_normal_zero_com(mu_x, P, sigma_x, pm, qm, draw(shape), nd)
    x_phar = xh_phar[:, :nd] * n_x
    h_phar = torch.nn.functional.one_hot(torch.argmax(z[:, nd:] * nv[1] + nb[1], dim=1), pnf)
    x_pocket = xh_pocket[:, :nd] * n_x
    h_pocket = xh_pocket[:, nd:] * nv[1] + nb[1]
    if checks:
        ref_cpu.assert_mean_zero_with_mask(x_phar, pm)
    if ref_cpu.scatter_add(x_phar, pm).abs().max().item() > 5e-2:                                # batch-wide
        x_phar, x_pocket = ref_cpu.remove_mean_batch(x_phar, x_pocket, pm, qm)
    # both reports on the returned rows, each sample in its caller's frame: shift from its returned pocket
    shift = ref_cpu.scatter_mean(x_pocket, qm, B) - n_x * com0
    E_fin, _, v_fin, _ = energy_terms(x_phar, x_pocket, shift, pm, qm, rec, clash_r, clash_k)
    _, overlap, _, _ = overlap_terms(x_phar - shift[pm], pm, set_sizes, strength, width)
    return dict(xh_phar=torch.cat([x_phar, h_phar.to(FLOAT)], dim=1), xh_pocket=torch.cat([x_pocket, h_pocket], dim=1), phar_mask=pm,
                pocket_mask=qm, z_steps=torch.stack(z_steps), pocket_steps=torch.stack(p_steps), margins=np.stack(margins),
                op_energy=torch.stack(op_energy), energy=E_fin, max_violation=v_fin, op_overlap=torch.stack(op_overlap), overlap=overlap,
                clipped=clipped, total=total, diverse_clipped=d_clipped, diverse_total=d_total)
