"""Host side of ConditionalDDPM.score: the level list, the per-level scalars and the assembly of the per-sample NLL from the raw sums
cmdgen_score_chain returns (include/cmdgen_hip.h).  Everything here is numpy on a few hundred scalars, in the reference's fp32 op
sequence (``training.per_sample_table`` evaluates the schedule; conditional_model.py:206-320, lightning_modules.py:211-229); only the sum
over the levels is taken in float64.

The quantity: with the levels t_k = (k + 1) T / K, k = 0 .. K-1, each with a Gaussian draw of its own,
    loss_t[b] = (T / K) sum_k -0.5 w_k error_k[b],        w_k = 1 - SNR(gamma(t_k - 1/T) - gamma(t_k)),
plus the t = 0 level (loss_0_x, loss_0_h), the constants and the prior KL term.  K = T is the diffusion part of the variational bound
itself; K < T is the reference's one-draw estimator (validation_step: one random t times T) on a fixed grid.
"""
from __future__ import annotations

from typing import Dict

import numpy as np

from .training import per_sample_table

SC_ERR, SC_ERR_X, SC_LOG_PH, SC_RESET = 0, 1, 2, 3        # columns of cmdgen_score_chain's level terms


def level_list(T: int, K: int) -> np.ndarray:
    """int32 [K + 1]: t_k = (k + 1) T / K for k < K, then the t = 0 level.  K must divide T."""
    T, K = int(T), int(K)
    if K < 1 or K > T or T % K != 0:
        raise ValueError(f'timesteps={K} must be a divisor of T = {T} (the levels are t_k = (k + 1) T / timesteps)')
    return np.concatenate([(np.arange(K, dtype=np.int64) + 1) * (T // K), [0]]).astype(np.int32)


def level_table(gamma, T: int, n_dims: int, norm_values, t_levels) -> Dict[str, np.ndarray]:
    """fp32 [n_levels] alpha, sigma and w (the reference's SNR_weight) of every level, and alpha_T / sigma_T, from the schedule's
    lookup table [T + 1] with the reference's own torch ops on the host (en_diffusion.py:859-867, conditional_model.py:206-221), so
    that they equal its values bit for bit."""
    import torch
    g = torch.from_numpy(np.ascontiguousarray(gamma, dtype=np.float32))
    rows = []
    # one level at a time on a single-sample batch, as EnVariationalDiffusion.step_table does: torch's element-wise kernels round a
    # short tensor (the reference's [B, 1] arrays) and a long one differently in the last bit
    for t_i in list(np.asarray(t_levels).reshape(-1)) + [T]:
        t_int = torch.full((1, 1), float(t_i))
        s, t = (t_int - 1) / T, t_int / T
        gamma_s, gamma_t = g[torch.round(s * T).long()], g[torch.round(t * T).long()]   # s = -1/T wraps to gamma[T], as the reference's lookup
        rows.append([torch.sqrt(torch.sigmoid(-gamma_t)).item(), torch.sqrt(torch.sigmoid(gamma_t)).item(),
                     (1 - torch.exp(-(gamma_s - gamma_t))).item()])
    rows = np.asarray(rows, dtype=np.float32)
    return {'alpha': rows[:-1, 0].copy(), 'sigma': rows[:-1, 1].copy(), 'w': rows[:-1, 2].copy(),
            'alpha_T': rows[-1, 0].copy(), 'sigma_T': rows[-1, 1].copy()}


def level_coef(tab: Dict[str, np.ndarray], repeats: int = 1) -> np.ndarray:
    """The `level_coef_host` argument of cmdgen_score_chain: (alpha, sigma) of the level list `repeats` times over, then of t = T."""
    rows = np.stack([np.tile(tab['alpha'], repeats), np.tile(tab['sigma'], repeats)], axis=1)
    return np.ascontiguousarray(np.concatenate([rows, [[tab['alpha_T'], tab['sigma_T']]]]).astype(np.float32))


def assemble(level_terms, kl_sums, gamma, log_pn, T: int, n_dims: int, norm_values, t_levels, n_phar, n_pocket) -> Dict[str, np.ndarray]:
    """level_terms [R, n_levels, B, >= 3] raw sums of R evaluations of the level list, kl_sums [B, 2] -> the per-sample terms (fp32):
    nll, loss_t, loss_0_x, loss_0_h (means over the R repeats) and their per-repeat values '<name>_repeats' [R, B], the weighted
    level terms 'level_terms' [R, n_levels, B] (-0.5 (T / K) w_k error_k; loss_0_x + loss_0_h at a t = 0 level), and the scalars of
    (n_phar, n_pocket): neg_log_const_0, kl_prior, delta_log_px, log_pN.  The list must hold t = 0 exactly once (the level_list form)."""
    f32 = np.float32
    lt = np.asarray(level_terms, dtype=f32)
    if lt.ndim == 3:
        lt = lt[None]
    R, nlev, B = lt.shape[:3]
    t_levels = np.asarray(t_levels).reshape(-1)
    assert len(t_levels) == nlev
    zero = t_levels == 0
    assert int(zero.sum()) == 1, 'the level list holds the t = 0 level exactly once'
    K = nlev - 1
    tab = level_table(gamma, T, n_dims, norm_values, t_levels)
    n_phar, n_pocket = np.asarray(n_phar, dtype=np.int64), np.asarray(n_pocket, dtype=np.int64)
    con = per_sample_table(gamma, log_pn, T, n_dims, norm_values, np.full(B, T, dtype=f32), n_phar, n_pocket).numpy()
    neg_log_const, delta_log_px, log_pN, sig_T = con[6], con[7], con[8], con[5]
    # kl_prior (conditional_model.py:20-56): gaussian_KL(|mu_T|^2, sigma_T, 1, d) for the features (d = 1) and the positions (d = (n - 1) n_dims)
    sub = ((n_phar - 1) * n_dims).astype(f32)
    kl = np.asarray(kl_sums, dtype=f32)
    one = f32(1)
    lg = np.log(one / sig_T, dtype=f32)
    kl_h = (lg + f32(0.5) * (sig_T ** 2 + kl[:, 1]) / one ** 2 - f32(0.5)).astype(f32)
    kl_x = (sub * lg + f32(0.5) * (sub * sig_T ** 2 + kl[:, 0]) / one ** 2 - f32(0.5) * sub).astype(f32)
    kl_prior = (kl_x + kl_h).astype(f32)
    # loss_t = -T 0.5 SNR_weight error_t of one level, times 1 / K (lightning_modules.py:206-212)
    scale = f32(-(float(T) / K) * 0.5) if K else f32(0)
    weighted = np.zeros((R, nlev, B), dtype=f32)
    weighted[:, ~zero] = (scale * tab['w'][~zero])[None, :, None] * lt[..., SC_ERR][:, ~zero]
    loss_0_x = (f32(0.5) * lt[..., SC_ERR_X][:, zero])[:, 0]                  # -(-0.5 sum (eps - net)^2 over x)
    loss_0_h = (-lt[..., SC_LOG_PH][:, zero])[:, 0]
    weighted[:, zero] = (loss_0_x + loss_0_h)[:, None]
    loss_t = weighted[:, ~zero].astype(np.float64).sum(1).astype(f32)        # [R, B]
    loss_0 = ((loss_0_x + f32(0)) + loss_0_h + neg_log_const[None]).astype(f32)
    nll = (((loss_t + loss_0) + kl_prior[None]) - delta_log_px[None] - log_pN[None]).astype(f32)
    mean = lambda v: v.astype(np.float64).mean(0).astype(f32)
    out = {'nll': mean(nll), 'loss_t': mean(loss_t), 'loss_0_x': mean(loss_0_x), 'loss_0_h': mean(loss_0_h),
           'neg_log_const_0': neg_log_const.astype(f32), 'kl_prior': kl_prior, 'delta_log_px': delta_log_px.astype(f32),
           'log_pN': log_pN.astype(f32),
           'nll_repeats': nll, 'loss_t_repeats': loss_t, 'loss_0_x_repeats': loss_0_x, 'loss_0_h_repeats': loss_0_h,
           'level_terms': weighted, 't_levels': t_levels.astype(np.int64)}
    return out


def assemble_groups(group_terms, member_terms, kl_sums, weights, gamma, log_pn, T: int, n_dims: int, norm_values, t_levels, n_phar,
                    n_pocket) -> Dict[str, np.ndarray]:
    """The assembly for groups of pockets that share one pharmacophore (cmdgen_multi_score_chain; ConditionalDDPM.score_given_pockets).
    group_terms [R, n_levels, G, >= 3], member_terms [R, n_levels, G, M, >= 3] or None, kl_sums [G, 2], weights float32 [G, M]
    (normalised), n_phar [G], n_pocket [G, M] -> ``assemble``'s dict per group [G] on the group's raw sums, with
        log_pN = sum_m w_m log p(N_phar | N_pocket_m)        (the geometric mixture's term; float64 sum of the fp32 per-member values)
    and nll taken with it; every other scalar depends on the group's rows alone.  With member_terms also 'member_nll',
    'member_loss_t', 'member_loss_0_x', 'member_log_pN' [G, M] and 'member_level_terms' [R, n_levels, G, M]: ``assemble`` on member m's
    columns with the group's kl_sums and that member's pocket size."""
    f32 = np.float32
    gt = np.asarray(group_terms, dtype=f32)
    if gt.ndim == 3:
        gt = gt[None]
    w = np.asarray(weights, dtype=f32)
    n_phar, n_pocket = np.asarray(n_phar, dtype=np.int64), np.asarray(n_pocket, dtype=np.int64)
    G, M = w.shape
    assert gt.shape[2] == G and n_pocket.shape == (G, M) and n_phar.shape == (G,)
    per_m = lambda terms, m: assemble(terms, kl_sums, gamma, log_pn, T, n_dims, norm_values, t_levels, n_phar, n_pocket[:, m])
    out = per_m(gt, 0)
    # log p(N_phar | N_pocket_m) by ``assemble``'s expression, per member [G, M]
    log_pN_m = np.stack([per_sample_table(gamma, log_pn, T, n_dims, norm_values, np.full(G, T, dtype=f32), n_phar, n_pocket[:, m]).numpy()[8]
                         for m in range(M)], axis=1).astype(f32)
    log_pN = (w.astype(np.float64) * log_pN_m.astype(np.float64)).sum(1).astype(f32)
    # ``assemble``'s nll with the group's log_pN in place of the first member's
    loss_0 = ((out['loss_0_x_repeats'] + f32(0)) + out['loss_0_h_repeats'] + out['neg_log_const_0'][None]).astype(f32)
    nll = (((out['loss_t_repeats'] + loss_0) + out['kl_prior'][None]) - out['delta_log_px'][None] - log_pN[None]).astype(f32)
    out['log_pN'], out['nll_repeats'] = log_pN, nll
    out['nll'] = nll.astype(np.float64).mean(0).astype(f32)
    if member_terms is not None:
        mt = np.asarray(member_terms, dtype=f32)
        if mt.ndim == 4:
            mt = mt[None]
        assert mt.shape[2:4] == (G, M)
        mem = [per_m(mt[:, :, :, m], m) for m in range(M)]
        for k in ('nll', 'loss_t', 'loss_0_x', 'log_pN'):
            out['member_' + k] = np.stack([o[k] for o in mem], axis=1)
        out['member_level_terms'] = np.stack([o['level_terms'] for o in mem], axis=3)
    return out
