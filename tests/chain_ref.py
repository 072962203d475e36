"""The CPU yardstick of every derived sampling chain, composed the way the device side composes them: ONE chain loop (run_chain: init, the
ops walked by ref_cpu.get_repaint_schedule, the decode) built only from oracle.ref_cpu primitives in torch fp32, and three optional parts -
`groups` (the device's GroupTab), `edit` (InpaintBuf) and `guide` (RestrainBuf).  With no part it is ref_cpu.sample_given_pocket's op sequence,
bit for bit given the same draws.  What a chain IS - layout, frames, what reduces to what - is said in the docstring of its adapter module
(cond_inpaint_ref, edit_ref, multi_pocket_ref, multi_edit_ref, restraint_ref, restrained_edit_ref, multi_restraint_ref,
multi_restrained_edit_ref); the tables and terms the parts need
(Groups, pair_margins, energy_terms, the plans) live here and are imported back by those modules."""
import numpy as np
import torch

from oracle import ref_cpu
from oracle.ref_cpu import FLOAT, INT

CUTOFF = 6.0
MARGIN = 1e-4          # A: a group with a pair closer than this to the cutoff at any evaluation may be left out of a comparison
CHAIN_CAP = 0.20       # ... but at most this share of a case's groups
POSITION, DISTANCE, EXCLUSION, CLASH = 0, 1, 2, 3
KIND_NAMES = ('position', 'distance', 'exclusion', 'clash')
TINY = 1e-12           # A: a term whose distance is below this contributes the zero vector


# ---------------------------------------------------------------------------------------------------------------------------------------
# groups
# ---------------------------------------------------------------------------------------------------------------------------------------
class Groups:
    """Index tables of a grouping: group_sizes [G], num_nodes_phar [G] (per group)."""
    def __init__(self, group_sizes, num_nodes_phar):
        self.sizes = np.asarray(group_sizes, dtype=np.int64)
        self.nph = np.asarray(num_nodes_phar, dtype=np.int64)
        assert self.sizes.ndim == 1 and self.sizes.shape == self.nph.shape and (self.sizes >= 1).all()
        self.G, self.B, self.max_m = len(self.sizes), int(self.sizes.sum()), int(self.sizes.max())
        self.first = np.concatenate([[0], np.cumsum(self.sizes)[:-1]])
        self.group_of = np.repeat(np.arange(self.G), self.sizes)                       # [B] group of a member
        self.member_nph = self.nph[self.group_of]                                       # [B] phar rows of a member
        self.Nu, self.Nl = int(self.nph.sum()), int(self.member_nph.sum())
        ubase = np.concatenate([[0], np.cumsum(self.nph)[:-1]])
        pbase = np.concatenate([[0], np.cumsum(self.member_nph)[:-1]])
        local = np.arange(self.Nl) - np.repeat(pbase, self.member_nph)
        self.phar_mask = torch.from_numpy(np.repeat(np.arange(self.B), self.member_nph))          # [Nl] member of a member row
        self.unique_mask = torch.from_numpy(np.repeat(np.arange(self.G), self.nph))               # [Nu] group of a unique row
        self.urow = torch.from_numpy(ubase[self.group_of][self.phar_mask.numpy()] + local)        # [Nl] unique row of a member row
        # rows_of[j]: (unique rows, member rows, member) of the j-th member of every group that has one
        self.rows_of = []
        for j in range(self.max_m):
            gs = np.flatnonzero(self.sizes > j)
            members = self.first[gs] + j
            mrows = np.concatenate([pbase[b] + np.arange(self.member_nph[b]) for b in members]).astype(np.int64)
            urows = np.concatenate([ubase[g] + np.arange(self.nph[g]) for g in gs]).astype(np.int64)
            self.rows_of.append((torch.from_numpy(urows), torch.from_numpy(mrows), torch.from_numpy(np.repeat(members, self.nph[gs]))))

    def combine(self, rows, w):
        """sum_m w_m rows_m with m ascending, the first term not added to a zero: member rows [Nl, C] -> unique rows [Nu, C]."""
        u, r, b = self.rows_of[0]
        out = w[b][:, None] * rows[r]
        for u, r, b in self.rows_of[1:]:
            out[u] = out[u] + w[b][:, None] * rows[r]
        return out

    def combine_members(self, per_member, w):
        """The same sum over one row per member: [B, C] -> [G, C]."""
        f = torch.from_numpy(self.first)
        out = w[f][:, None] * per_member[f]
        for j in range(1, self.max_m):
            gs = torch.from_numpy(np.flatnonzero(self.sizes > j))
            out[gs] = out[gs] + w[f[gs] + j][:, None] * per_member[f[gs] + j]
        return out

    def first_rows(self):
        """[Nu] the member rows of every group's first member: the group's copy of the latent that is reported."""
        return self.rows_of[0][1]


def pair_margins(x_phar, x_pocket, phar_mask, pocket_mask, cutoff=CUTOFF):
    """[B] float64: per member sample the smallest | ||x_i - x_j|| - cutoff | over its pairs i < j."""
    pm, qm = np.asarray(phar_mask), np.asarray(pocket_mask)
    xp, xq = np.asarray(x_phar, dtype=np.float64), np.asarray(x_pocket, dtype=np.float64)
    B = int(max(pm.max(initial=-1), qm.max(initial=-1))) + 1
    out = np.full(B, np.inf)
    for b in range(B):
        p = np.concatenate([xp[pm == b], xq[qm == b]])
        if len(p) > 1:
            d = np.sqrt(((p[:, None, :] - p[None, :, :]) ** 2).sum(-1))
            out[b] = np.abs(d[np.triu_indices(len(p), k=1)] - cutoff).min()
    return out


def kept_groups(margins, groups):
    """[G] bool: the groups none of whose members has a pair within MARGIN of the cutoff at any evaluation (margins [evaluations, B])."""
    ok = np.asarray(margins).min(axis=0) >= MARGIN
    return np.array([ok[f:f + m].all() for f, m in zip(groups.first, groups.sizes)])


# ---------------------------------------------------------------------------------------------------------------------------------------
# edit
# ---------------------------------------------------------------------------------------------------------------------------------------
def edit_plan(resamplings, jump_length, timesteps, start=None):
    """(ops, draws, jumps) of a chain that starts at level `start`: draw 0, per op A and B (and C before a jump back), the
    decode draw - n_draws = 2 + 2 n_steps + n_jumps for the schedule actually walked."""
    start = timesteps if start is None else start
    if not 1 <= start <= timesteps:
        raise ValueError(f'start={start} must be in [1, timesteps={timesteps}]')
    schedule = ref_cpu.get_repaint_schedule(resamplings, jump_length, start)
    n_steps, n_jumps = sum(schedule), len(schedule) - 1
    return n_steps, 2 + 2 * n_steps + n_jumps, n_jumps


def inpaint_plan(resamplings, jump_length, timesteps):
    """(ops, draws, jumps) of a chain from the prior."""
    return edit_plan(resamplings, jump_length, timesteps)


# ---------------------------------------------------------------------------------------------------------------------------------------
# guide
# ---------------------------------------------------------------------------------------------------------------------------------------
def _norm(diff):
    return torch.sqrt((diff ** 2).sum(dim=1))


def energy_terms(xhat, q, shift, pm, qm, rec, clash_r, clash_k):
    """The energy of step 3 at the points xhat [Nl, 3] (A) with pocket atoms q [Np, 3] (A) and the frame shift [B, 3], any float dtype.
    rec: the record array of cmdgen_amd.restraints.records (kind, sample, i, j, c, a, b, k).  A point's gradient terms are summed in the
    definition's order - position, distance and exclusion terms in list order, then pocket atoms in index order - by one index_add_ over the
    term list (ref_cpu.scatter_add walks it in order).
    -> (E [B], g [Nl, 3] = dE / dxhat, largest violation [B], largest violation per kind [4])."""
    dt = xhat.dtype
    B, Nl = shift.shape[0], xhat.shape[0]
    nph = torch.bincount(pm, minlength=B)
    pbase = torch.cumsum(nph, 0) - nph
    # one entry per (term, point it acts on): the gradient row, the energy (on one of a distance term's two ends only), the violation
    t_row, t_g, t_e, t_v, t_kind = [], [], [], [], []

    def push(rows, diff, dist, v, sign, k, count, kind):
        coef = torch.where(dist >= TINY, sign * (k * v) / dist.clamp(min=TINY), torch.zeros_like(dist))
        t_row.append(rows); t_g.append(coef[:, None] * diff); t_v.append(v)
        t_e.append(0.5 * k * (v * v) if count else torch.zeros_like(v))
        t_kind.append(torch.full_like(rows, kind))

    for r in rec:                                                        # list order
        b, k = int(r['sample']), float(r['k'])
        if int(r['kind']) == DISTANCE:
            i, j = int(pbase[b]) + int(r['i']), int(pbase[b]) + int(r['j'])
            diff = (xhat[i] - xhat[j])[None, :]
            dist = _norm(diff)
            lo, hi = float(r['a']), float(r['b'])
            v = torch.clamp(torch.maximum(lo - dist, dist - hi), min=0)
            sign = torch.where(dist < lo, -torch.ones_like(dist), torch.ones_like(dist))
            push(torch.tensor([i]), diff, dist, v, sign, k, True, DISTANCE)
            push(torch.tensor([j]), -diff, dist, v, sign, k, False, DISTANCE)
            continue
        centre = torch.as_tensor(np.asarray(r['c'], dtype=np.float32)).to(dt) + shift[b]
        if int(r['kind']) == POSITION:
            rows = torch.tensor([int(pbase[b]) + int(r['i'])])
            diff = xhat[rows] - centre
            dist = _norm(diff)
            push(rows, diff, dist, torch.clamp(dist - float(r['a']), min=0), torch.ones_like(dist), k, True, POSITION)
        else:
            rows = int(pbase[b]) + torch.arange(int(nph[b]))
            diff = xhat[rows] - centre
            dist = _norm(diff)
            push(rows, diff, dist, torch.clamp(float(r['a']) - dist, min=0), -torch.ones_like(dist), k, True, EXCLUSION)
    if clash_r > 0:                                                      # then the pocket atoms in index order, point by point
        for b in range(B):
            rows, atoms = torch.nonzero(pm == b).reshape(-1), torch.nonzero(qm == b).reshape(-1)
            if len(rows) == 0 or len(atoms) == 0:
                continue
            diff = (xhat[rows][:, None, :] - q[atoms][None, :, :]).reshape(-1, 3)
            dist = _norm(diff)
            push(rows.repeat_interleave(len(atoms)), diff, dist, torch.clamp(clash_r - dist, min=0), -torch.ones_like(dist), float(clash_k),
                 True, CLASH)
    E, g = torch.zeros(B, dtype=dt), torch.zeros((Nl, 3), dtype=dt)
    vmax, vkind = torch.zeros(B, dtype=dt), torch.zeros(4, dtype=dt)
    if t_row:
        rows, kinds, v = torch.cat(t_row), torch.cat(t_kind), torch.cat(t_v)
        g = ref_cpu.scatter_add(torch.cat(t_g), rows, Nl)
        E = ref_cpu.scatter_add(torch.cat(t_e), pm[rows], B)
        for b in range(B):
            sel = pm[rows] == b
            if bool(sel.any()):
                vmax[b] = v[sel].max()
        for kd in range(4):
            if bool((kinds == kd).any()):
                vkind[kd] = v[kinds == kd].max()
    return E, g, vmax, vkind


def touched_samples(rec, B, clash_r):
    t = np.zeros(B, dtype=bool)
    if clash_r > 0:
        t[:] = True
    for r in rec:
        t[int(r['sample'])] = True
    return t


def op_terms(z, P, eps_t, known, fx, sigma_t, alpha_t, com_in, pm, qm, rec, clash_r, clash_k, n_x, nd, first=None, qg=None):
    """Steps 1-3 of one op: -> (xhat [rows, 3] (A), shift [owners, 3] (A), E [owners], g [rows, 3], largest violation per kind [4]).  z, P: the
    op's input; eps_t: the network's output; known: the normalised given rows (None: no row is given); fx [rows] bool: the rows whose x columns
    are held.  A restraint's OWNER is a sample, or grouped a group: z, eps_t, known and fx then hold one copy of the rows per group, pm is the
    group of a row, first [G] the member whose pocket gives a group its frame and qg [Np] the group of a pocket atom (qm stays its member).
    Ungrouped both default to the identities."""
    B = com_in.shape[0]
    first = torch.arange(B) if first is None else first
    qg = qm if qg is None else qg
    shift = (n_x * (ref_cpu.scatter_mean(P[:, :nd], qm, B) - com_in))[first]                      # 2. the owner's first member's
    xhat = n_x * (z[:, :nd] - sigma_t[first][pm] * eps_t[:, :nd]) / alpha_t[first][pm]            # 1. free rows
    if known is not None:
        held = n_x * known[:, :nd] + shift[pm]                                                     #    held rows: the given position in this frame
        xhat = torch.where(fx[:, None], held, xhat)
    E, g, _, vk = energy_terms(xhat, n_x * P[:, :nd], shift, pm, qg, rec, clash_r, clash_k)        # 3. every member's atoms
    return xhat, shift, E, g, vk


# ---------------------------------------------------------------------------------------------------------------------------------------
# the loop
# ---------------------------------------------------------------------------------------------------------------------------------------
def run_chain(p, cfg, pocket, phar=None, num_nodes_phar=None, groups=None, edit=None, guide=None, timesteps=None, noise=None, checks=True,
              probe=None, record_margins=True):
    """pocket: dict(x, one_hot, size [B], mask) of the samples; the phar rows come from `phar` (dict(x, one_hot, mask), the given rows of an
    edit) or from num_nodes_phar.  noise(shape) supplies each draw in call order: draw 0, per op A (and B with an edit part, and C before a
    jump back), the decode draw.  The parts, all optional:
      groups = dict(group_sizes [G], weights [B]): the samples are the MEMBERS of groups that share one latent; phar (with size [G]) or
        num_nodes_phar [G], the draws and the reported rows hold one copy of the rows per group.
      edit = dict(fix_x, fix_h [rows], start, resamplings, jump_length): op B and the jumps; start < timesteps begins at q(z_start | given rows).
        Without it there is no op B and no B draw, and the schedule is get_repaint_schedule(1, 1, K) == [K].
      guide = dict(rec, clash_r, clash_k, scale, max_shift, guide_below): steps 1-5 of csrc/kernels_restrain.hip's header in op A, once per
        OWNER of a restraint - a sample, or with groups a group (rec['sample'] is then the group index): its rows are the reported copy, its
        frame its first member's pocket, its clash atoms every member's, and every member's copy gets the same displacement.  probe(op index,
        dict of op_terms' inputs in the owner view, and the op's t [B, 1]) is called before them.
    -> dict(xh_phar, xh_pocket, phar_mask, pocket_mask, z_steps [n_steps, rows, 3+P], pocket_steps [n_steps, Np, 3], margins [n_steps + 1, B]
    (A, one row per evaluation; None unless recorded), known_steps [n_steps, rows, 3] (edit), op_energy [n_steps, B], kind_violation
    [n_steps, 4], energy [B], max_violation [B], clipped, unclipped: counts of displacements per reported row and op (guide; grouped, [B]
    reads [G]: one entry per owner)."""
    T, nd, pnf = cfg['timesteps'], cfg['n_dims'], cfg['phar_nf']
    nv, nb = cfg['norm_values'], cfg['norm_biases']
    n_x = nv[0]
    if groups is not None or guide is not None:                     # grouping and guidance are defined for this configuration only
        assert not cfg.get('no_com_projection', False) and not cfg.get('update_pocket_coords', False)
    table = ref_cpu.gamma_source(p)
    timesteps = T if timesteps is None else timesteps
    start, resamplings, jump_length = timesteps, 1, 1
    if edit is not None:
        start = timesteps if edit['start'] is None else edit['start']
        resamplings, jump_length = edit['resamplings'], edit['jump_length']
    edit_plan(resamplings, jump_length, timesteps, start)           # the range check
    draw = noise if noise is not None else (lambda shape: torch.randn(shape))

    # inputs.  spread: one copy of the rows per group -> every member's rows; report: back.  Ungrouped, both are the identity.
    qm = pocket['mask'].to(INT)
    if groups is None:
        gr, B = None, len(pocket['size'])
        pm = phar['mask'].to(INT) if phar is not None else torch.repeat_interleave(torch.arange(B), torch.as_tensor(num_nodes_phar).to(INT))
        n_rows, out_mask, offset_of = len(pm), pm, torch.arange(B)
        spread = report = lambda rows: rows
        um, qg, first, n_own = pm, qm, torch.arange(B), B           # the owner view of the guide part: a sample owns its restraints
    else:
        gr = Groups(groups['group_sizes'], np.asarray(phar['size']).reshape(-1) if phar is not None else num_nodes_phar)
        B = gr.B
        assert len(pocket['size']) == B
        w = torch.as_tensor(groups['weights']).to(FLOAT).reshape(-1)
        assert len(w) == B
        pm, n_rows, out_mask = gr.phar_mask, gr.Nu, gr.unique_mask
        group_of = torch.from_numpy(gr.group_of)
        offset_of = torch.from_numpy(gr.first)[group_of]            # [B] the first member of a member's group: its pocket shift is the group's
        spread, report = (lambda rows: rows[gr.urow]), (lambda rows: rows[gr.first_rows()])
        # ... a GROUP owns them: owner of a reported row, of a pocket atom (members ascending, atoms in index order), the member whose frame it uses
        um, qg, first, n_own = gr.unique_mask, group_of[qm], torch.from_numpy(gr.first), gr.G
    shape = (n_rows, nd + pnf)
    # normalize (en_diffusion.py:874-889)
    px = pocket['x'].to(FLOAT) / n_x
    xh0_pocket = torch.cat([px, (pocket['one_hot'].float() - nb[1]) / nv[1]], dim=1)
    com0 = ref_cpu.scatter_mean(px, qm, B)                          # com(P_in.x / n_x)
    known_u, fx_u = None, torch.zeros(n_rows, dtype=torch.bool)    # (_u: one copy of the rows per group, before spread)
    if edit is not None:
        known_u = torch.cat([phar['x'].to(FLOAT) / n_x, (phar['one_hot'].float() - nb[1]) / nv[1]], dim=1)
        fx_u = torch.as_tensor(edit['fix_x']).to(FLOAT).reshape(-1) != 0
        known, fx = spread(known_u), spread(fx_u)
        fh = spread(torch.as_tensor(edit['fix_h']).to(FLOAT).reshape(-1) != 0)
        col_fixed = torch.cat([fx[:, None].expand(-1, nd), fh[:, None].expand(-1, pnf)], dim=1)
        has_mark = torch.zeros(B, dtype=torch.bool)
        has_mark[pm[fx | fh]] = True
        rows_m, rows_q = has_mark[pm], has_mark[qm]
    if guide is not None:
        rec, clash_r, clash_k, scale, max_shift = (guide[k] for k in ('rec', 'clash_r', 'clash_k', 'scale', 'max_shift'))
        touched = torch.from_numpy(touched_samples(rec, n_own, clash_r))   # [owners]
        any_touched = bool(touched.any())

    # init
    if start == timesteps:
        # from the prior, as ref_cpu.sample_given_pocket; grouped, c = sum_m w_m com(P_m) and every member's copy is [c, 0] + the group's draw
        c = com0 if gr is None else gr.combine_members(com0, w)[group_of]
        mu_phar = torch.cat((c, torch.zeros((B, pnf))), dim=1)[pm]
        sigma = torch.ones_like(pocket['size']).unsqueeze(1)
        z, P = ref_cpu.sample_normal_zero_com(mu_phar, xh0_pocket, sigma, pm, qm, spread(draw(shape)), nd)
    else:
        # part-way: q(z_start | x) of the given rows, as ConditionalDDPM.forward (conditional_model.py:235-243, :158-179); grouped, every
        # member's pocket centred on the centre of mass of the group's given rows
        xh0, P0c = known.clone(), xh0_pocket.clone()
        xh0[:, :nd], P0c[:, :nd] = ref_cpu.remove_mean_batch(known[:, :nd], xh0_pocket[:, :nd], pm, qm)
        gamma_t = ref_cpu.gamma_lookup(table, torch.full((B, 1), fill_value=start) / timesteps, T)
        z = ref_cpu.alpha_of(gamma_t)[pm] * xh0 + ref_cpu.sigma_of(gamma_t)[pm] * spread(draw(shape))
        P = P0c.clone()
        z[:, :nd], P[:, :nd] = ref_cpu.remove_mean_batch(z[:, :nd], P0c[:, :nd], pm, qm)
    if checks:
        ref_cpu.assert_mean_zero_with_mask(z[:, :nd], pm)

    # evaluation.  Grouped, the members are evaluated SLOT by slot: call j holds the j-th member of every group that has one, as one ordinary
    # batch.  With groups of one member the only call is ref_cpu.sample_given_pocket's own, and the first members of all groups form the batch
    # a single chain on the first pockets evaluates - so both reductions hold bit for bit (the oracle's matrix products round a sample's rows
    # differently in the last bit when the batch around it changes).
    slots = []
    for j, (u, r, b) in enumerate(gr.rows_of if gr is not None else ()):
        members = torch.from_numpy(gr.first[gr.sizes > j] + j)
        renum = torch.full((B,), -1, dtype=INT)
        renum[members] = torch.arange(len(members))
        qrows = torch.nonzero(renum[qm] >= 0).reshape(-1)
        slots.append((r, members, renum[pm[r]], qrows, renum[qm[qrows]]))
    margins = []

    def evaluate(t_array):
        """eps on every row of z: the network's, or grouped the members' combined per group (the NaN guard is batch-wide)"""
        if record_margins:
            margins.append(pair_margins(z[:, :nd], P[:, :nd], pm, qm, cfg['edge_cutoff']) * n_x)   # (the graph is built on normalised x)
        if gr is None:
            return ref_cpu.dynamics_forward(p, cfg, z, P, t_array, pm, qm)[0]  # (its x columns are zero when the NaN guard reset)
        eps = torch.empty_like(z)
        reset = False
        for r, members, pm_j, qrows, qm_j in slots:
            eps[r], _ = ref_cpu.dynamics_forward(p, cfg, z[r], P[qrows], t_array[members], pm_j, qm_j)
            # dynamics_forward zeroes the velocities of its whole call when one is NaN (dynamics.py:129-131): all exactly zero then
            reset = reset or (len(r) > 0 and not bool(eps[r][:, :nd].any()))
        if reset:
            eps[:, :nd] = 0.0
        return spread(gr.combine(eps, w))

    schedule = ref_cpu.get_repaint_schedule(resamplings, jump_length, start)
    z_steps, p_steps, k_steps, op_energy, kind_v = [], [], [], [], []
    clipped = unclipped = 0
    s = start - 1
    for i, n_denoise_steps in enumerate(schedule):
        for j in range(n_denoise_steps):
            s_array = torch.full((B, 1), fill_value=s)
            t_array = s_array + 1
            s_array = s_array / timesteps
            t_array = t_array / timesteps
            # A: sample_p_zs_given_zt, as in ref_cpu.sample_given_pocket, with the guidance term in its mean
            gamma_s = ref_cpu.gamma_lookup(table, s_array, T)
            gamma_t = ref_cpu.gamma_lookup(table, t_array, T)
            sigma2_ts, sigma_ts, alpha_ts = ref_cpu.sigma_and_alpha_t_given_s(gamma_t, gamma_s)
            sigma_s, sigma_t = ref_cpu.sigma_of(gamma_s), ref_cpu.sigma_of(gamma_t)
            eps_t = evaluate(t_array)
            mu = z / alpha_ts[pm] - (sigma2_ts / alpha_ts / sigma_t)[pm] * eps_t
            sig = sigma_ts * sigma_s / sigma_t
            if guide is not None:
                alpha_t = ref_cpu.alpha_of(gamma_t)
                E, vk = torch.zeros(n_own), torch.zeros(4)
                terms_in = dict(z=report(z), P=P, eps_t=report(eps_t), known=known_u, fx=fx_u, sigma_t=sigma_t, alpha_t=alpha_t, com_in=com0,
                                pm=um, qm=qm, first=first, qg=qg)
                if probe is not None:
                    probe(len(op_energy), dict(terms_in, t=t_array))
                if any_touched:
                    _, _, E, g, vk = op_terms(rec=rec, clash_r=clash_r, clash_k=clash_k, n_x=n_x, nd=nd, **terms_in)          # 1. - 3.
                    var = (n_x * sig[first]) ** 2
                    d = -scale * var[um] * g                                                       # 4.
                    length = _norm(d)
                    over = length > max_shift
                    d = torch.where(over[:, None], d * (max_shift / length.clamp(min=1e-30))[:, None], d)
                    active = touched[um] & (t_array[first][um][:, 0] <= guide['guide_below']) & (scale > 0) & ~fx_u   # a held row gets nothing added
                    clipped += int((over & active).sum())
                    unclipped += int((~over & active & (length > 0)).sum())
                    d_m = spread(d)                                                                # every member's copy gets the same displacement
                    rows = torch.nonzero(spread(active)).reshape(-1)
                    if len(rows):
                        mu[rows, :nd] = mu[rows, :nd] + d_m[rows] / n_x                            # 5.
                op_energy.append(E)
                kind_v.append(vk)
            if checks:
                ref_cpu.assert_mean_zero_with_mask(z[:, :nd], pm)
            z, P = ref_cpu.sample_normal_zero_com(mu, P, sig, pm, qm, spread(draw(shape)), nd)
            if edit is not None:
                # B: the noised known rows in the current frame (moved by the sample's pocket shift; grouped, by the GROUP's, its first
                # member's) replace the held column groups, then the projection
                z_u, P_u = z, P
                eps_b = spread(draw(shape))
                alpha_s = ref_cpu.alpha_of(gamma_s)
                z_k = alpha_s[pm] * known + sigma_s[pm] * eps_b
                z_k[:, :nd] = z_k[:, :nd] + (ref_cpu.scatter_mean(P_u[:, :nd], qm, B) - com0)[offset_of][pm]
                z_m = torch.where(col_fixed, z_k, z_u)
                P_m = P_u.clone()
                z_m[:, :nd], P_m[:, :nd] = ref_cpu.remove_mean_batch(z_m[:, :nd], P_u[:, :nd], pm, qm)
                z = torch.where(rows_m[:, None], z_m, z_u)          # samples (groups) without a mark skip the merge
                P = torch.where(rows_q[:, None], P_m, P_u)
                # the noised known rows in the frame of the saved step (what the held rows of z are, up to rounding)
                k_steps.append(report(z_k[:, :nd] - (ref_cpu.scatter_mean(P_u[:, :nd], qm, B) - ref_cpu.scatter_mean(P[:, :nd], qm, B))[pm]))
            z_steps.append(report(z).clone())
            p_steps.append(P[:, :nd].clone())
            # C: jump back (sample_p_zt_given_zs, conditional_model.py:330-340), not guided
            if j == n_denoise_steps - 1 and i < len(schedule) - 1:
                t = s + jump_length
                gamma_t2 = ref_cpu.gamma_lookup(table, torch.full((B, 1), fill_value=t) / timesteps, T)
                _, sigma_ts2, alpha_ts2 = ref_cpu.sigma_and_alpha_t_given_s(gamma_t2, gamma_s)
                z, P = ref_cpu.sample_normal_zero_com(alpha_ts2[pm] * z, P, sigma_ts2, pm, qm, spread(draw(shape)), nd)
                s = t
            s -= 1

    # decode, not guided: as ref_cpu.sample_given_pocket
    t_zeros = torch.zeros((B, 1))
    gamma_0 = ref_cpu.gamma_lookup(table, t_zeros, T)
    sigma_x = torch.exp(-(-0.5 * gamma_0))
    net_out = evaluate(t_zeros)
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
    out = dict(xh_phar=report(torch.cat([x_phar, h_phar.to(FLOAT)], dim=1)), xh_pocket=torch.cat([x_pocket, h_pocket], dim=1),
               phar_mask=out_mask, pocket_mask=qm, z_steps=torch.stack(z_steps), pocket_steps=torch.stack(p_steps),
               margins=np.stack(margins) if record_margins else None, known_steps=torch.stack(k_steps) if edit is not None else None)
    if guide is not None:
        # the diagnostics of the returned rows (held points at their returned positions) against every member's returned pocket: shift from
        # the owner's first member's returned pocket
        shift = (ref_cpu.scatter_mean(x_pocket, qm, B) - n_x * com0)[first]
        E_fin, _, v_fin, _ = energy_terms(report(x_phar), x_pocket, shift, um, qg, rec, clash_r, clash_k)
        out.update(op_energy=torch.stack(op_energy), kind_violation=torch.stack(kind_v), energy=E_fin, max_violation=v_fin, clipped=clipped,
                   unclipped=unclipped)
    return out
