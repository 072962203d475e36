"""Golden vectors for ConditionalDDPM.edit (G22): the reference has no loop that edits a given pharmacophore, so this script
composes the reference's own ConditionalDDPM methods (normalize, remove_mean_batch, noised_representation,
sample_normal_zero_com, sample_p_zs_given_zt, alpha / sigma / gamma with its sample_gaussian, sample_p_zt_given_zs,
sample_p_xh_given_z0, get_repaint_schedule) into the loop INTEGRATION.md specifies, importing the real reference in the build
container.  Writes tests/golden/g22_edit.npz.

    python tests/golden/make_golden_edit.py

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
from make_golden_cond_inpaint import instrument, scatter_mean  # noqa: E402

from cmdgen_amd.synthetic import ModelConfig, make_pockets  # noqa: E402


def cond_edit(ddpm, phar, pocket, fix_x, fix_h, start, resamplings, jump_length, timesteps):
    """The edit loop on the reference's methods.  -> out_phar, out_pocket, z_steps, pocket_steps."""
    nd = ddpm.n_dims
    phar, pocket = dict(phar), dict(pocket)
    phar, pocket = ddpm.normalize(phar=phar, pocket=pocket)
    pm, qm = phar['mask'], pocket['mask']
    B = len(pocket['size'])
    known = torch.cat([phar['x'], phar['one_hot']], dim=1)
    xh0_pocket = torch.cat([pocket['x'], pocket['one_hot']], dim=1)
    fx, fh = torch.as_tensor(fix_x).bool().view(-1), torch.as_tensor(fix_h).bool().view(-1)
    col_fixed = torch.cat([fx[:, None].expand(-1, nd), fh[:, None].expand(-1, ddpm.phar_nf)], dim=1)
    marked = fx | fh
    has_mark = torch.zeros(B, dtype=torch.bool)
    if bool(marked.any()):
        has_mark.index_fill_(0, pm[marked], True)
    rows_m, rows_q = has_mark[pm], has_mark[qm]
    com0 = scatter_mean(xh0_pocket[:, :nd], qm, B)
    if start == timesteps:
        # from the prior, as sample_given_pocket (conditional_model.py:402-420)
        mu_x = scatter_mean(pocket['x'], qm, B)
        mu = torch.cat((mu_x, torch.zeros((B, ddpm.phar_nf))), dim=1)[pm]
        sigma = torch.ones_like(pocket['size']).unsqueeze(1)
        z, P = ddpm.sample_normal_zero_com(mu, xh0_pocket, sigma, pm, qm)
    else:
        # part-way, as forward (conditional_model.py:235-243): centre on the phar centre of mass, then q(z_start | x)
        xh0 = known.clone()
        P0c = xh0_pocket.clone()
        xh0[:, :nd], P0c[:, :nd] = ddpm.remove_mean_batch(xh0[:, :nd], P0c[:, :nd], pm, qm)
        gamma_t = ddpm.inflate_batch_array(ddpm.gamma(torch.full((B, 1), fill_value=start) / timesteps), phar['x'])
        z, P, _ = ddpm.noised_representation(xh0, P0c, pm, qm, gamma_t)
        ddpm.assert_mean_zero_with_mask(z[:, :nd], pm)
    schedule = ddpm.get_repaint_schedule(resamplings, jump_length, start)
    z_steps, p_steps = [], []
    s = start - 1
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
            z_m = torch.where(col_fixed, z_k, z_u)                  # per column group
            zx, px = ddpm.remove_mean_batch(z_m[:, :nd], P_u[:, :nd], pm, qm)
            z_m[:, :nd] = zx
            P_m = P_u.clone()
            P_m[:, :nd] = px
            z = torch.where(rows_m[:, None], z_m, z_u)              # a sample without a mark skips the merge
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


def masks_for(kind, pmask, B):
    """(fix_x, fix_h) float [Nl] of a case's mask pattern; samples are 0 .. B-1."""
    fx, fh = np.zeros(len(pmask), np.float32), np.zeros(len(pmask), np.float32)
    rows = [np.nonzero(pmask == b)[0] for b in range(B)]
    if kind == 'holds':            # 0: types only, 1: coordinates only, 2: x / h / both / neither by row, 3: no mark
        fh[rows[0]] = 1.0
        fx[rows[1]] = 1.0
        fx[rows[2][0::4]] = 1.0
        fh[rows[2][1::4]] = 1.0
        fx[rows[2][2::4]] = 1.0
        fh[rows[2][2::4]] = 1.0
    elif kind == 'mixed':          # 0: a third of the rows types only, 1: no mark, 2: x / h / both / neither by row
        fh[rows[0][:max(1, len(rows[0]) // 3)]] = 1.0
        fx[rows[2][0::4]] = 1.0
        fh[rows[2][1::4]] = 1.0
        fx[rows[2][2::4]] = 1.0
        fh[rows[2][2::4]] = 1.0
    else:
        assert kind == 'none'
    return fx, fh


def main():
    mods = import_reference()
    g = {}
    # name, hidden_nf, n_layers, B, K, start, resamplings, jump_length, mask pattern, seed
    cases = [('h64_K12_s12_holds', 64, 2, 4, 12, 12, 1, 1, 'holds', 221),
             ('h64_K12_s7_none', 64, 2, 3, 12, 7, 1, 1, 'none', 222),
             ('h64_K10_s6_mixed_r2j1', 64, 2, 3, 10, 6, 2, 1, 'mixed', 223),
             ('h64_K9_s9_mixed_r3j2', 64, 2, 3, 9, 9, 3, 2, 'mixed', 224),
             ('h256_K6_s4_holds_r2j2', 256, 5, 4, 6, 4, 2, 2, 'holds', 225)]
    for name, H, L, B, K, S, R_, J_, kind, seed in cases:
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
            fix_x, fix_h = masks_for(kind, pmask, B)
            draws, margins = instrument(ddpm, nseed)
            phar = {'x': torch.from_numpy(phar_x.copy()), 'one_hot': torch.from_numpy(phar_oh.copy()),
                    'size': torch.from_numpy(nl.copy()), 'mask': torch.from_numpy(pmask.copy())}
            with torch.no_grad(), contextlib.redirect_stdout(io.StringIO()):
                xh_phar, xh_pocket, z_steps, p_steps = cond_edit(ddpm, phar, pockets_to_torch(pb), fix_x, fix_h, S, R_, J_, K)
            if min(margins) > 2e-3:
                break
            first += 1000
            nseed += 1000
        n_steps = len(z_steps)
        assert len(draws) == 2 + 2 * n_steps + (len(ddpm.get_repaint_schedule(R_, J_, S)) - 1)
        g[f'{name}/meta'] = np.asarray([H, L, B, 20, seed, K, R_, J_, first, S], dtype=np.int64)
        g[f'{name}/phar_x'], g[f'{name}/phar_one_hot'] = phar_x, phar_oh
        g[f'{name}/fix_x'], g[f'{name}/fix_h'] = fix_x, fix_h
        g[f'{name}/noise'] = np.stack(draws).astype(np.float32)
        g[f'{name}/margins'] = np.asarray(margins, dtype=np.float32)
        g[f'{name}/xh_phar'], g[f'{name}/xh_pocket'] = xh_phar, xh_pocket
        g[f'{name}/z_steps'], g[f'{name}/pocket_steps'] = z_steps, p_steps
        print(name, 'first', first, 'draws', len(draws), 'ops', n_steps, 'min margin', min(margins))
    np.savez_compressed(os.path.join(HERE, 'g22_edit.npz'), **g)
    print('wrote g22_edit.npz', os.path.getsize(os.path.join(HERE, 'g22_edit.npz')), 'bytes')


if __name__ == '__main__':
    main()
