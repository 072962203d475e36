"""Golden vectors for ConditionalDDPM.inpaint (G20): the reference has no conditional RePaint loop, so this script composes
the reference's own ConditionalDDPM methods (sample_normal_zero_com, sample_p_zs_given_zt, alpha / sigma / gamma with its
sample_gaussian, remove_mean_batch, sample_p_zt_given_zs, sample_p_xh_given_z0) into the loop INTEGRATION.md specifies,
importing the real reference (/root/reference/DiffPhar) in the build container.  Writes tests/golden/g20_cond_inpaint.npz.

    python tests/golden/make_golden_cond_inpaint.py

Fixtures hold inputs, every raw Gaussian draw (in call order), the cutoff margins and the outputs - never weights (those
are regenerated from the seed by cmdgen_amd/synthetic.py) and never reference source.
"""
import contextlib
import io
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import HIST, build_reference_ddpm, import_reference, pockets_to_torch  # noqa: E402

from cmdgen_amd.synthetic import ModelConfig, make_pockets, min_cutoff_margin  # noqa: E402


def instrument(ddpm, nseed):
    draws, margins = [], []
    gen = torch.Generator().manual_seed(nseed)

    def rec_gauss(size, device):
        n = torch.randn(size, generator=gen)
        draws.append(n.numpy().copy())
        return n
    ddpm.sample_gaussian = rec_gauss
    orig_edges = type(ddpm.dynamics).get_edges.__get__(ddpm.dynamics)

    def rec_edges(mask, x):
        margins.append(min_cutoff_margin(x.numpy(), mask.numpy(), 6.0))
        return orig_edges(mask, x)
    ddpm.dynamics.get_edges = rec_edges
    return draws, margins


def scatter_mean(x, idx, n):
    tot = torch.zeros((n, x.shape[1])).index_add_(0, idx, x)
    cnt = torch.zeros(n).index_add_(0, idx, torch.ones(len(idx))).clamp(min=1)
    return tot / cnt[:, None]


def cond_inpaint(ddpm, phar, pocket, phar_fixed, resamplings, jump_length, timesteps):
    """The conditional RePaint loop on the reference's methods.  -> out_phar, out_pocket, z_steps, pocket_steps."""
    nd = ddpm.n_dims
    phar, pocket = dict(phar), dict(pocket)
    phar, pocket = ddpm.normalize(phar=phar, pocket=pocket)
    pm, qm = phar['mask'], pocket['mask']
    B = len(pocket['size'])
    known = torch.cat([phar['x'], phar['one_hot']], dim=1)
    xh0_pocket = torch.cat([pocket['x'], pocket['one_hot']], dim=1)
    fixed = torch.as_tensor(phar_fixed).bool().view(-1)
    has_fixed = torch.zeros(B, dtype=torch.bool).index_fill_(0, pm[fixed], True) if bool(fixed.any()) else torch.zeros(B, dtype=torch.bool)
    rows_m, rows_q = has_fixed[pm], has_fixed[qm]
    # init, as sample_given_pocket (conditional_model.py:402-420)
    mu_x = scatter_mean(pocket['x'], qm, B)
    mu = torch.cat((mu_x, torch.zeros((B, ddpm.phar_nf))), dim=1)[pm]
    sigma = torch.ones_like(pocket['size']).unsqueeze(1)
    z, P = ddpm.sample_normal_zero_com(mu, xh0_pocket, sigma, pm, qm)
    com0 = scatter_mean(xh0_pocket[:, :nd], qm, B)
    schedule = ddpm.get_repaint_schedule(resamplings, jump_length, timesteps)
    z_steps, p_steps = [], []
    s = timesteps - 1
    for i, n_denoise_steps in enumerate(schedule):
        for j in range(n_denoise_steps):
            s_array = torch.full((B, 1), fill_value=s)
            t_array = s_array + 1
            s_array = s_array / timesteps
            t_array = t_array / timesteps
            z_u, P_u = ddpm.sample_p_zs_given_zt(s_array, t_array, z, P, pm, qm)                       # draw A
            gamma_s = ddpm.gamma(s_array)
            alpha_s, sigma_s = ddpm.alpha(gamma_s, z_u), ddpm.sigma(gamma_s, z_u)
            eps_b = ddpm.sample_gaussian(size=(len(pm), nd + ddpm.phar_nf), device=pm.device)          # draw B
            z_k = alpha_s[pm] * known + sigma_s[pm] * eps_b
            z_k[:, :nd] = z_k[:, :nd] + (scatter_mean(P_u[:, :nd], qm, B) - com0)[pm]
            z_m = torch.where(fixed[:, None], z_k, z_u)
            zx, px = ddpm.remove_mean_batch(z_m[:, :nd], P_u[:, :nd], pm, qm)
            z_m[:, :nd] = zx
            P_m = P_u.clone()
            P_m[:, :nd] = px
            z = torch.where(rows_m[:, None], z_m, z_u)              # a sample without fixed rows skips the merge
            P = torch.where(rows_q[:, None], P_m, P_u)
            z_steps.append(z.numpy().copy())
            p_steps.append(P[:, :nd].numpy().copy())
            if j == n_denoise_steps - 1 and i < len(schedule) - 1:
                t = s + jump_length
                gamma_t = ddpm.gamma(torch.full((B, 1), fill_value=t) / timesteps)
                z, P = ddpm.sample_p_zt_given_zs(z, P, pm, qm, gamma_t, gamma_s)                        # draw C
                s = t
            s -= 1
    x_phar, h_phar, x_pocket, h_pocket = ddpm.sample_p_xh_given_z0(z, P, pm, qm, B)                    # decode draw
    ddpm.assert_mean_zero_with_mask(x_phar, pm)
    x = torch.zeros((B, nd)).index_add_(0, pm, x_phar)
    if float(x.abs().max()) > 5e-2:
        x_phar, x_pocket = ddpm.remove_mean_batch(x_phar, x_pocket, pm, qm)
    return (torch.cat([x_phar, h_phar.float()], 1).numpy(), torch.cat([x_pocket, h_pocket], 1).numpy(),
            np.stack(z_steps), np.stack(p_steps))


def main():
    mods = import_reference()
    g = {}
    # name, hidden_nf, n_layers, B, K, resamplings, jump_length, seed
    cases = [('h64_K12_r1j1', 64, 2, 3, 12, 1, 1, 201),
             ('h64_K8_r2j1', 64, 2, 3, 8, 2, 1, 202),
             ('h64_K9_r3j2', 64, 2, 3, 9, 3, 2, 203),
             ('h256_K5_r2j2', 256, 5, 3, 5, 2, 2, 204)]
    for name, H, L, B, K, R_, J_, seed in cases:
        cfg = ModelConfig(hidden_nf=H, n_layers=L, timesteps=500)
        ddpm, _ = build_reference_ddpm(mods, cfg, seed, 1.0, HIST)
        first, nseed = 100 * seed, seed
        while True:
            pb = make_pockets(B, 'CA', ragged=True, n_phar=7, first_index=first)
            nl = pb.num_nodes_phar
            pmask = np.repeat(np.arange(B), nl)
            rng = np.random.Generator(np.random.PCG64(first))
            com = np.stack([pb.x[pb.mask == b].mean(0) for b in range(B)])
            phar_x = (com[pmask] + rng.normal(size=(len(pmask), 3)) * 2.5).astype(np.float32)
            phar_oh = np.eye(8, dtype=np.float32)[rng.integers(0, 8, size=len(pmask))]
            # sample 0: some rows fixed, sample 1: none, sample 2: all
            fixed = np.zeros(len(pmask), dtype=np.float32)
            r0 = np.nonzero(pmask == 0)[0]
            fixed[r0[:max(1, len(r0) // 3)]] = 1.0
            fixed[pmask == 2] = 1.0
            draws, margins = instrument(ddpm, nseed)
            phar = {'x': torch.from_numpy(phar_x.copy()), 'one_hot': torch.from_numpy(phar_oh.copy()),
                    'size': torch.from_numpy(nl.copy()), 'mask': torch.from_numpy(pmask.copy())}
            with torch.no_grad(), contextlib.redirect_stdout(io.StringIO()):
                xh_phar, xh_pocket, z_steps, p_steps = cond_inpaint(ddpm, phar, pockets_to_torch(pb), fixed, R_, J_, K)
            if min(margins) > 2e-3:
                break
            first += 1000
            nseed += 1000
        n_steps = len(z_steps)
        assert len(draws) == 2 + 2 * n_steps + (len(ddpm.get_repaint_schedule(R_, J_, K)) - 1)
        g[f'{name}/meta'] = np.asarray([H, L, B, 20, seed, K, R_, J_, first], dtype=np.int64)
        g[f'{name}/phar_x'], g[f'{name}/phar_one_hot'], g[f'{name}/phar_fixed'] = phar_x, phar_oh, fixed
        g[f'{name}/noise'] = np.stack(draws).astype(np.float32)
        g[f'{name}/margins'] = np.asarray(margins, dtype=np.float32)
        g[f'{name}/xh_phar'], g[f'{name}/xh_pocket'] = xh_phar, xh_pocket
        g[f'{name}/z_steps'], g[f'{name}/pocket_steps'] = z_steps, p_steps
        print(name, 'first', first, 'draws', len(draws), 'ops', n_steps, 'min margin', min(margins))
    np.savez_compressed(os.path.join(HERE, 'g20_cond_inpaint.npz'), **g)
    print('wrote g20_cond_inpaint.npz', os.path.getsize(os.path.join(HERE, 'g20_cond_inpaint.npz')), 'bytes')


if __name__ == '__main__':
    main()
