"""CPU model of diverse sampling (ConditionalDDPM.sample_diverse, cmdgen_diverse_chain; INTEGRATION.md, "Diverse sampling"), built only from
oracle.ref_cpu primitives in torch fp32: ref_cpu.sample_given_pocket's op sequence with the term of csrc/kernels_diverse.hip (steps 1-4 of its
header) added to the mean of every posterior op.  With strength = 0, or with every set of one member, it reproduces chain_ref.run_chain's plain
path bit for bit given the same draws.

chain_ref.run_chain has no hook in the mean, so the loop below is its plain path (no groups, no edit, no guide) line for line, with steps 1-4 in
op A.  The sets are given as set_sizes [S]: runs of consecutive samples."""
import numpy as np
import torch

from chain_ref import pair_margins
from oracle import ref_cpu
from oracle.ref_cpu import FLOAT, INT


def set_tables(set_sizes, B):
    """-> (set_of [B] the set of a sample, M [B] the size of a sample's set) as int64 tensors."""
    sizes = np.asarray(set_sizes, dtype=np.int64).reshape(-1)
    assert (sizes >= 1).all() and int(sizes.sum()) == B, (sizes, B)
    return torch.from_numpy(np.repeat(np.arange(len(sizes)), sizes)), torch.from_numpy(np.repeat(sizes, sizes))


def overlap_terms(y, pm, set_sizes, strength, width):
    """Step 2 at the points y [Nl, 3] (A, each sample in its caller's frame), any float dtype; pm [Nl] the sample of a row.
    -> (o [Nl] a point's share, overlap [B], g [Nl, 3] = dE / dy, E [S] the sets' energies)."""
    B = int(np.asarray(set_sizes).sum())
    set_of, M = set_tables(set_sizes, B)
    S = len(np.asarray(set_sizes).reshape(-1))
    o, g = torch.zeros(len(pm), dtype=y.dtype), torch.zeros((len(pm), 3), dtype=y.dtype)
    E = torch.zeros(S, dtype=y.dtype)
    row_set = set_of[pm]
    for s in range(S):
        rows = torch.nonzero(row_set == s).reshape(-1)
        m = int(M[pm[rows[0]]]) if len(rows) else 1
        if m < 2 or len(rows) == 0:
            continue
        ys = y[rows]
        diff = ys[:, None, :] - ys[None, :, :]                                         # [R, R, 3]: y_ai - y_bj
        other = (pm[rows][:, None] != pm[rows][None, :]).to(y.dtype)                     # b != a
        e = torch.exp(-(diff ** 2).sum(-1) / (2.0 * width * width)) * other
        o[rows] = e.sum(1) / (m - 1)
        g[rows] = -(strength / ((m - 1) * width * width)) * (e[:, :, None] * diff).sum(1)
        E[s] = strength / (m - 1) * 0.5 * e.sum()                                       # every pair a < b once
    overlap = ref_cpu.scatter_add(o, pm, B)
    return o, overlap, g, E


def diverse_chain(p, cfg, pocket, num_nodes_phar, set_sizes, strength=1.0, width=2.0, max_shift=1.0, guide_below=1.0, timesteps=None,
                  noise=None, checks=True):
    """pocket: dict(x, one_hot, size [B], mask); noise(shape) supplies each draw in call order: draw 0, one per op, the decode draw.
    -> dict(xh_phar, xh_pocket, z_steps [K, Nl, 3+P], pocket_steps [K, Np, 3], margins [K + 1, B] (A, one row per evaluation), op_overlap
    [K, B], overlap [B], clipped, total: displacements capped and displacements made)."""
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

    z_steps, p_steps, op_overlap = [], [], []
    clipped = total = 0
    for s in reversed(range(0, timesteps)):
        s_array = torch.full((B, 1), fill_value=s)
        t_array = s_array + 1
        s_array = s_array / timesteps
        t_array = t_array / timesteps
        # A: sample_p_zs_given_zt, as in ref_cpu.sample_given_pocket, with the term in its mean
        gamma_s = ref_cpu.gamma_lookup(table, s_array, T)
        gamma_t = ref_cpu.gamma_lookup(table, t_array, T)
        sigma2_ts, sigma_ts, alpha_ts = ref_cpu.sigma_and_alpha_t_given_s(gamma_t, gamma_s)
        sigma_s, sigma_t = ref_cpu.sigma_of(gamma_s), ref_cpu.sigma_of(gamma_t)
        eps_t = evaluate(t_array)
        mu = z / alpha_ts[pm] - (sigma2_ts / alpha_ts / sigma_t)[pm] * eps_t
        sig = sigma_ts * sigma_s / sigma_t
        alpha_t = ref_cpu.alpha_of(gamma_t)
        xhat = n_x * (z[:, :nd] - sigma_t[pm] * eps_t[:, :nd]) / alpha_t[pm]                    # 1.
        shift = n_x * (ref_cpu.scatter_mean(P[:, :nd], qm, B) - com0)
        y = xhat - shift[pm]
        _, ov, g, _ = overlap_terms(y, pm, set_sizes, strength, width)                          # 2.
        op_overlap.append(ov)
        var = (n_x * sig) ** 2
        d = -var[pm] * g                                                                        # 3.
        length = torch.sqrt((d ** 2).sum(dim=1))
        over = length > max_shift
        d = torch.where(over[:, None], d * (max_shift / length.clamp(min=1e-30))[:, None], d)
        active = coupled & (t_array[pm][:, 0] <= guide_below) & (strength > 0)
        clipped += int((over & active).sum())
        total += int(active.sum())
        rows = torch.nonzero(active).reshape(-1)
        if len(rows):
            mu[rows, :nd] = mu[rows, :nd] + d[rows] / n_x                                       # 4.  (nothing is added to any other row)
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
    # the overlap of the returned rows, each sample in its caller's frame: shift from its returned pocket
    shift = ref_cpu.scatter_mean(x_pocket, qm, B) - n_x * com0
    _, overlap, _, _ = overlap_terms(x_phar - shift[pm], pm, set_sizes, strength, width)
    return dict(xh_phar=torch.cat([x_phar, h_phar.to(FLOAT)], dim=1), xh_pocket=torch.cat([x_pocket, h_pocket], dim=1), phar_mask=pm,
                pocket_mask=qm, z_steps=torch.stack(z_steps), pocket_steps=torch.stack(p_steps), margins=np.stack(margins),
                op_overlap=torch.stack(op_overlap), overlap=overlap, clipped=clipped, total=total)
