"""CPU model of the restrained multi-pocket edit chain (ConditionalDDPM.edit_restrained_given_pockets, cmdgen_multi_restrained_edit_chain;
INTEGRATION.md, "Editing under restraints for several pockets"), built only from oracle.ref_cpu primitives in torch fp32: the multi-pocket
edit chain's op sequence over the MEMBER samples (every member of a group holds a copy of the group's latent; the known rows, the marks and
the draws hold one copy of the rows per group; ops A, B and C of the edit plan) with the guidance term of csrc/kernels_restrain.hip added to
the mean of op A, once per GROUP:
  - a restraint belongs to a group (rec['sample'] is the group index), its centres lie in the common frame of the group's pockets;
  - xhat of a row whose x columns are not held comes from the combined eps the step itself uses; a row whose x columns ARE held enters at its
    given position moved into the current frame, n_x K_i.x + shift_g;
  - the frame shift is the group's FIRST member's, its pocket as it stands at the op's input (step B keeps its own offset);
  - the clash term sums over the atoms of EVERY member, unweighted; a point's terms are summed in the definition's order;
  - every member's copy of the latent gets the same displacement, on the rows whose x is not held only; op C and the decode are not guided.
Given the same draws it reproduces, bit for bit, multi_edit_ref.multi_edit_chain with scale = 0 or with no record and r_c = 0,
restrained_edit_ref.restrained_edit with every group of one member, and multi_restraint_ref.multi_restrained_chain with no mark, start =
timesteps and resamplings = jump_length = 1 (the B draws are then read and not used) - test_multi_restrained_edit_cpu.py asserts all three.

Why this module has a loop of its own: chain_ref.run_chain refuses `groups` together with `guide`, and chain_ref.py is a yardstick that
does not move.  So the loop below repeats run_chain's grouped edit branch (slot-by-slot evaluation, Groups.combine, ops B and C) and
multi_restraint_ref's per-group guidance with op_terms' held rows, composed from the parts chain_ref exports (Groups, energy_terms,
touched_samples, pair_margins, kept_groups, edit_plan) and oracle.ref_cpu.  The duplication is the price of not moving a yardstick."""
import numpy as np
import torch

from chain_ref import (CHAIN_CAP, DISTANCE, MARGIN, Groups, _norm, edit_plan, energy_terms, kept_groups, pair_margins,      # noqa: F401
                       touched_samples)
from oracle import ref_cpu
from oracle.ref_cpu import FLOAT, INT

KEYS = ('xh_phar', 'xh_pocket', 'phar_mask', 'pocket_mask', 'z_steps', 'pocket_steps', 'margins', 'op_energy', 'energy', 'max_violation',
        'kind_violation', 'clipped', 'unclipped', 'other_member_clash', 'held_record_ops')


def multi_restrained_edit(p, cfg, phar, pocket, group_sizes, weights, fix_x, fix_h, rec, clash_r=0.0, clash_k=0.0, scale=1.0, max_shift=1.0,
                          guide_below=1.0, start=None, resamplings=1, jump_length=1, timesteps=None, noise=None, checks=True):
    """phar: dict(x [Nu,3], one_hot [Nu,P], size [G]) one copy of the rows per group, in the pockets' common frame; pocket: dict(x, one_hot,
    size [B], mask) of the member samples; weights [B]; fix_x, fix_h [Nu]; rec: the record array of cmdgen_amd.restraints.records called with
    the per-GROUP point counts; noise(shape) supplies each draw of shape (Nu, 3 + P) in the edit plan's call order.
    -> dict(xh_phar [Nu, 3+P], xh_pocket [Np, 3+R], phar_mask [Nu] (group ids), pocket_mask, z_steps [n_steps, Nu, 3+P], pocket_steps
    [n_steps, Np, 3], margins [n_steps + 1, B] (A), op_energy [n_steps, G], energy [G], max_violation [G], kind_violation [n_steps, 4],
    clipped, unclipped: counts of displacements that were and were not clipped (per unique free row and op), other_member_clash [n_steps]:
    the largest clash violation (A) against an atom of a member other than its group's first, held_record_ops: how many guided ops had a
    distance record that joins a held-x row to a free row of a guided group)."""
    T, nd, pnf = cfg['timesteps'], cfg['n_dims'], cfg['phar_nf']
    nv, nb = cfg['norm_values'], cfg['norm_biases']
    n_x = nv[0]
    assert not cfg.get('no_com_projection', False) and not cfg.get('update_pocket_coords', False)
    table = ref_cpu.gamma_source(p)
    timesteps = T if timesteps is None else timesteps
    start = timesteps if start is None else start
    edit_plan(resamplings, jump_length, timesteps, start)           # the range check
    draw = noise if noise is not None else (lambda shape: torch.randn(shape))

    qm = pocket['mask'].to(INT)
    gr = Groups(group_sizes, np.asarray(phar['size']).reshape(-1))
    B, G = gr.B, gr.G
    assert len(pocket['size']) == B
    w = torch.as_tensor(weights).to(FLOAT).reshape(-1)
    assert len(w) == B
    pm, um = gr.phar_mask, gr.unique_mask
    group_of = torch.from_numpy(gr.group_of)
    first = torch.from_numpy(gr.first)                                # [G] the first member of a group: the guidance frame is its pocket's
    offset_of = first[group_of]                                        # [B] ... and so is the offset of step B
    qg = group_of[qm]                                                  # [Np] group of a pocket atom: members ascending, atoms in index order
    spread, report = (lambda rows: rows[gr.urow]), (lambda rows: rows[gr.first_rows()])
    shape = (gr.Nu, nd + pnf)
    px = pocket['x'].to(FLOAT) / n_x
    xh0_pocket = torch.cat([px, (pocket['one_hot'].float() - nb[1]) / nv[1]], dim=1)
    com0 = ref_cpu.scatter_mean(px, qm, B)                            # com(P_in.x / n_x)
    known_u = torch.cat([phar['x'].to(FLOAT) / n_x, (phar['one_hot'].float() - nb[1]) / nv[1]], dim=1)       # [Nu]
    fx_u = torch.as_tensor(fix_x).to(FLOAT).reshape(-1) != 0           # [Nu] the rows whose x columns are held
    known, fx = spread(known_u), spread(fx_u)
    fh = spread(torch.as_tensor(fix_h).to(FLOAT).reshape(-1) != 0)
    col_fixed = torch.cat([fx[:, None].expand(-1, nd), fh[:, None].expand(-1, pnf)], dim=1)
    has_mark = torch.zeros(B, dtype=torch.bool)
    has_mark[pm[fx | fh]] = True
    rows_m, rows_q = has_mark[pm], has_mark[qm]
    touched = torch.from_numpy(touched_samples(rec, G, clash_r))       # [G]
    any_touched = bool(touched.any())
    other = (torch.arange(B) != first[group_of])[qm]                   # [Np] atoms of a member that is not its group's first
    ubase = np.concatenate([[0], np.cumsum(gr.nph)[:-1]])
    held_free = torch.zeros(G, dtype=torch.bool)                       # groups with a distance record between a held-x and a free row
    for r in rec:
        if int(r['kind']) == DISTANCE:
            g_ = int(r['sample'])
            if bool(fx_u[ubase[g_] + int(r['i'])]) != bool(fx_u[ubase[g_] + int(r['j'])]):
                held_free[g_] = True

    # init
    if start == timesteps:
        # from the prior: c = sum_m w_m com(P_m), every member's copy is [c, 0] + the group's draw
        c = gr.combine_members(com0, w)[group_of]
        mu_phar = torch.cat((c, torch.zeros((B, pnf))), dim=1)[pm]
        sigma = torch.ones_like(pocket['size']).unsqueeze(1)
        z, P = ref_cpu.sample_normal_zero_com(mu_phar, xh0_pocket, sigma, pm, qm, spread(draw(shape)), nd)
    else:
        # part-way: q(z_start | x) of the given rows, every member's pocket centred on the centre of mass of the group's given rows
        xh0, P0c = known.clone(), xh0_pocket.clone()
        xh0[:, :nd], P0c[:, :nd] = ref_cpu.remove_mean_batch(known[:, :nd], xh0_pocket[:, :nd], pm, qm)
        gamma_t = ref_cpu.gamma_lookup(table, torch.full((B, 1), fill_value=start) / timesteps, T)
        z = ref_cpu.alpha_of(gamma_t)[pm] * xh0 + ref_cpu.sigma_of(gamma_t)[pm] * spread(draw(shape))
        P = P0c.clone()
        z[:, :nd], P[:, :nd] = ref_cpu.remove_mean_batch(z[:, :nd], P0c[:, :nd], pm, qm)
    if checks:
        ref_cpu.assert_mean_zero_with_mask(z[:, :nd], pm)

    # evaluation, slot by slot: call j holds the j-th member of every group that has one, as one ordinary batch (chain_ref.run_chain)
    slots = []
    for j, (u, r, b) in enumerate(gr.rows_of):
        members = torch.from_numpy(gr.first[gr.sizes > j] + j)
        renum = torch.full((B,), -1, dtype=INT)
        renum[members] = torch.arange(len(members))
        qrows = torch.nonzero(renum[qm] >= 0).reshape(-1)
        slots.append((r, members, renum[pm[r]], qrows, renum[qm[qrows]]))
    margins = []

    def evaluate(t_array):
        """the members' eps combined per group, one copy of the rows per group [Nu] (the NaN guard is batch-wide)"""
        margins.append(pair_margins(z[:, :nd], P[:, :nd], pm, qm, cfg['edge_cutoff']) * n_x)
        eps = torch.empty_like(z)
        reset = False
        for r, members, pm_j, qrows, qm_j in slots:
            eps[r], _ = ref_cpu.dynamics_forward(p, cfg, z[r], P[qrows], t_array[members], pm_j, qm_j)
            reset = reset or (len(r) > 0 and not bool(eps[r][:, :nd].any()))
        if reset:
            eps[:, :nd] = 0.0
        return gr.combine(eps, w)

    schedule = ref_cpu.get_repaint_schedule(resamplings, jump_length, start)
    z_steps, p_steps, op_energy, kind_v, other_v = [], [], [], [], []
    clipped = unclipped = held_record_ops = 0
    s = start - 1
    for i, n_denoise_steps in enumerate(schedule):
        for j in range(n_denoise_steps):
            s_array = torch.full((B, 1), fill_value=s)
            t_array = s_array + 1
            s_array = s_array / timesteps
            t_array = t_array / timesteps
            # A: sample_p_zs_given_zt on the combined eps, with the group's guidance term in its mean
            gamma_s = ref_cpu.gamma_lookup(table, s_array, T)
            gamma_t = ref_cpu.gamma_lookup(table, t_array, T)
            sigma2_ts, sigma_ts, alpha_ts = ref_cpu.sigma_and_alpha_t_given_s(gamma_t, gamma_s)
            sigma_s, sigma_t = ref_cpu.sigma_of(gamma_s), ref_cpu.sigma_of(gamma_t)
            ebar = evaluate(t_array)                                   # [Nu]
            eps_t = spread(ebar)
            mu = z / alpha_ts[pm] - (sigma2_ts / alpha_ts / sigma_t)[pm] * eps_t
            sig = sigma_ts * sigma_s / sigma_t
            alpha_t = ref_cpu.alpha_of(gamma_t)
            E, vk, vo = torch.zeros(G), torch.zeros(4), 0.0
            if any_touched:
                z_u = report(z)                                        # the first member's copy of the latent
                shift = (n_x * (ref_cpu.scatter_mean(P[:, :nd], qm, B) - com0))[first]                  # 2. the first member's
                xhat = n_x * (z_u[:, :nd] - sigma_t[first][um] * ebar[:, :nd]) / alpha_t[first][um]     # 1. free rows
                held = n_x * known_u[:, :nd] + shift[um]                                                #    held rows: the given position in this frame
                xhat = torch.where(fx_u[:, None], held, xhat)
                q = n_x * P[:, :nd]
                E, g, _, vk = energy_terms(xhat, q, shift, um, qg, rec, clash_r, clash_k)               # 3. every member's atoms
                if clash_r > 0:                                        # diagnostic only: does a member other than the first bite?
                    for k in range(G):
                        pts, atoms = xhat[um == k], q[other & (qg == k)]
                        if len(pts) and len(atoms):
                            dist = _norm((pts[:, None, :] - atoms[None, :, :]).reshape(-1, 3))
                            vo = max(vo, float(torch.clamp(clash_r - dist, min=0).max()))
                var = (n_x * sig[first]) ** 2
                d = -scale * var[um] * g                               # 4.
                length = _norm(d)
                over = length > max_shift
                d = torch.where(over[:, None], d * (max_shift / length.clamp(min=1e-30))[:, None], d)
                guided = touched & (t_array[first][:, 0] <= guide_below) & (scale > 0)                  # [G]
                active = guided[um] & ~fx_u                            # a held row gets nothing added
                clipped += int((over & active).sum())
                unclipped += int((~over & active & (length > 0)).sum())
                held_record_ops += int(bool((guided & held_free).any()))
                d_m, active_m = spread(d), spread(active)              # every member's copy gets the same displacement
                rows = torch.nonzero(active_m).reshape(-1)
                if len(rows):
                    mu[rows, :nd] = mu[rows, :nd] + d_m[rows] / n_x    # 5.
            op_energy.append(E)
            kind_v.append(vk)
            other_v.append(vo)
            if checks:
                ref_cpu.assert_mean_zero_with_mask(z[:, :nd], pm)
            z, P = ref_cpu.sample_normal_zero_com(mu, P, sig, pm, qm, spread(draw(shape)), nd)
            # B: the noised known rows in the current frame (moved by the GROUP's pocket shift, its first member's) replace the held column
            # groups, then the projection
            z_u2, P_u = z, P
            eps_b = spread(draw(shape))
            alpha_s = ref_cpu.alpha_of(gamma_s)
            z_k = alpha_s[pm] * known + sigma_s[pm] * eps_b
            z_k[:, :nd] = z_k[:, :nd] + (ref_cpu.scatter_mean(P_u[:, :nd], qm, B) - com0)[offset_of][pm]
            z_m = torch.where(col_fixed, z_k, z_u2)
            P_m = P_u.clone()
            z_m[:, :nd], P_m[:, :nd] = ref_cpu.remove_mean_batch(z_m[:, :nd], P_u[:, :nd], pm, qm)
            z = torch.where(rows_m[:, None], z_m, z_u2)                # groups without a mark skip the merge
            P = torch.where(rows_q[:, None], P_m, P_u)
            z_steps.append(report(z).clone())
            p_steps.append(P[:, :nd].clone())
            # C: jump back (sample_p_zt_given_zs), not guided
            if j == n_denoise_steps - 1 and i < len(schedule) - 1:
                t = s + jump_length
                gamma_t2 = ref_cpu.gamma_lookup(table, torch.full((B, 1), fill_value=t) / timesteps, T)
                _, sigma_ts2, alpha_ts2 = ref_cpu.sigma_and_alpha_t_given_s(gamma_t2, gamma_s)
                z, P = ref_cpu.sample_normal_zero_com(alpha_ts2[pm] * z, P, sigma_ts2, pm, qm, spread(draw(shape)), nd)
                s = t
            s -= 1

    # decode, not guided: as ref_cpu.sample_given_pocket on the combined eps
    t_zeros = torch.zeros((B, 1))
    gamma_0 = ref_cpu.gamma_lookup(table, t_zeros, T)
    sigma_x = torch.exp(-(-0.5 * gamma_0))
    net_out = spread(evaluate(t_zeros))
    sigma_0, alpha_0 = ref_cpu.sigma_of(gamma_0), ref_cpu.alpha_of(gamma_0)
    mu_x = 1. / alpha_0[pm] * (z - sigma_0[pm] * net_out)
    xh_phar, xh_pocket = ref_cpu.sample_normal_zero_com(mu_x, P, sigma_x, pm, qm, spread(draw(shape)), nd)
    x_phar = xh_phar[:, :nd] * n_x
    h_phar = torch.nn.functional.one_hot(torch.argmax(z[:, nd:] * nv[1] + nb[1], dim=1), pnf)
    x_pocket = xh_pocket[:, :nd] * n_x
    h_pocket = xh_pocket[:, nd:] * nv[1] + nb[1]
    if checks:
        ref_cpu.assert_mean_zero_with_mask(x_phar, pm)
    if ref_cpu.scatter_add(x_phar, pm).abs().max().item() > 5e-2:                                # batch-wide
        x_phar, x_pocket = ref_cpu.remove_mean_batch(x_phar, x_pocket, pm, qm)
    # the diagnostics of the returned rows (held points at their returned positions) against every member's returned pocket: shift from the
    # first member's returned pocket
    shift = (ref_cpu.scatter_mean(x_pocket, qm, B) - n_x * com0)[first]
    E_fin, _, v_fin, _ = energy_terms(report(x_phar), x_pocket, shift, um, qg, rec, clash_r, clash_k)
    return dict(xh_phar=report(torch.cat([x_phar, h_phar.to(FLOAT)], dim=1)), xh_pocket=torch.cat([x_pocket, h_pocket], dim=1),
                phar_mask=um, pocket_mask=qm, z_steps=torch.stack(z_steps), pocket_steps=torch.stack(p_steps), margins=np.stack(margins),
                op_energy=torch.stack(op_energy), kind_violation=torch.stack(kind_v), energy=E_fin, max_violation=v_fin, clipped=clipped,
                unclipped=unclipped, other_member_clash=np.asarray(other_v), held_record_ops=held_record_ops)
