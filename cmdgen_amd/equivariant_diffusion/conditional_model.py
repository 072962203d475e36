"""ConditionalDDPM: pocket fixed, only pharmacophore nodes diffuse
(counterpart of conditional_model.py:12-475).

``sample_given_pocket`` is the hot path: the whole ancestral chain (init noise, K posterior
steps with one network evaluation each, final decode, drift fix) runs inside
libcmdgen_hip.so with the step captured as a hipGraph; the host only prepares the per-step
scalar table and reads the deferred checks afterwards.
"""
from __future__ import annotations

import math
from types import SimpleNamespace

import numpy as np
import torch

from .en_diffusion import EnVariationalDiffusion, fresh_seed, no_grad_unless_differentiable
from .. import utils


class ConditionalDDPM(EnVariationalDiffusion):
    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        assert not self.dynamics.update_pocket_coords
        self.use_hip_graph = True
        self.last_chain_status = None

    # ---- reference entry points that were already stubs there
    def sample_normal(self, *args):
        raise NotImplementedError('Has been replaced by sample_normal_zero_com()')

    def sample_combined_position_feature_noise(self, *args):
        raise NotImplementedError('Use sample_normal_zero_com() instead.')

    def sample(self, *args):
        raise NotImplementedError('Conditional model does not support sampling without given pocket.')

    # ---- loss terms (conditional_model.py:20-106, :158-320): the network evaluation runs in the HIP library.  By default
    # they are VALUES (no autograd graph): training.HipTrainer trains with the activation-saving forward (``_net``) plus the
    # library's own backward pass and the analytic gradient of these terms.  With the dynamics in differentiable mode
    # (EGNNDynamics.set_differentiable) and grad mode on they are built with autograd, as in the reference.
    def noised_representation(self, xh_phar, xh0_pocket, phar_mask, pocket_mask, gamma_t, eps=None):
        alpha_t, sigma_t = self.alpha(gamma_t, xh_phar), self.sigma(gamma_t, xh_phar)
        eps_phar = self.sample_gaussian((len(phar_mask), self.n_dims + self.phar_nf), phar_mask.device) \
            if eps is None else eps
        z_t = alpha_t[phar_mask] * xh_phar + sigma_t[phar_mask] * eps_phar
        nd = self.n_dims
        zx, px = self.remove_mean_batch(z_t[:, :nd], xh0_pocket[:, :nd], phar_mask, pocket_mask)
        return torch.cat([zx, z_t[:, nd:]], 1), torch.cat([px, xh0_pocket[:, nd:]], 1), eps_phar

    def kl_prior(self, xh_phar, mask_phar, num_nodes):
        B, nd = len(num_nodes), self.n_dims
        ones = torch.ones((B, 1), device=xh_phar.device)
        gamma_T = self.gamma(ones)
        mu_T = self.alpha(gamma_T, xh_phar)[mask_phar] * xh_phar
        sigma_T = self.sigma(gamma_T, mu_T).squeeze()
        one = torch.ones_like(sigma_T)
        kl_h = self.gaussian_KL(self.sum_except_batch(mu_T[:, nd:] ** 2, mask_phar, B), sigma_T, one, d=1)
        kl_x = self.gaussian_KL(self.sum_except_batch(mu_T[:, :nd] ** 2, mask_phar, B), sigma_T, one,
                                self.subspace_dimensionality(num_nodes))
        return kl_x + kl_h

    def log_pxh_given_z0_without_constants(self, phar, z_0_phar, eps_phar, net_out_phar, gamma_0, epsilon=1e-10):
        nd, B = self.n_dims, len(phar['size'])
        sigma_0_cat = self.sigma(gamma_0, target_tensor=z_0_phar) * self.norm_values[1]
        log_px = -0.5 * self.sum_except_batch((eps_phar[:, :nd] - net_out_phar[:, :nd]) ** 2, phar['mask'], B)
        phar_onehot = phar['one_hot'] * self.norm_values[1] + self.norm_biases[1]
        centered = z_0_phar[:, nd:] * self.norm_values[1] + self.norm_biases[1] - 1
        log_ph = torch.log(self.cdf_standard_gaussian((centered + 0.5) / sigma_0_cat[phar['mask']])
                           - self.cdf_standard_gaussian((centered - 0.5) / sigma_0_cat[phar['mask']]) + epsilon)
        log_ph = log_ph - torch.logsumexp(log_ph, dim=1, keepdim=True)
        return log_px, self.sum_except_batch(log_ph * phar_onehot, phar['mask'], B)

    def log_pN(self, N_phar, N_pocket):
        return self.size_distribution.log_prob_n1_given_n2(N_phar, N_pocket)

    @no_grad_unless_differentiable
    def forward(self, phar, pocket, return_info=False, t_int=None, eps=None, _net=None):
        """The 12 loss terms (+ info) of conditional_model.py:198-320 - VALUES (no autograd graph) unless the dynamics are in
        differentiable mode and grad mode is on (then with autograd, as in the reference).

        t_int [B,1] and eps (list of the Gaussian draws, one per noised_representation call) may be
        supplied for reproducibility; otherwise they are drawn like the reference does.  ``_net`` replaces the
        network evaluation (training.HipTrainer passes the activation-saving training forward); the tensors the
        analytic loss gradient needs are left in ``self._last_train_ctx``."""
        phar, pocket = dict(phar), dict(pocket)
        phar, pocket = self.normalize(phar, pocket)
        B, nd, dev = len(phar['size']), self.n_dims, phar['x'].device
        delta_log_px = self.delta_log_px(phar['size'])
        if t_int is None:
            t_int = torch.randint(0 if self.training else 1, self.T + 1, size=(B, 1), device=dev).float()
        t_int = t_int.to(dev).float()
        s_int = t_int - 1
        t_is_zero = (t_int == 0).float()
        s, t = s_int / self.T, t_int / self.T
        gamma_s = self.inflate_batch_array(self.gamma(s), phar['x'])
        gamma_t = self.inflate_batch_array(self.gamma(t), phar['x'])
        xh0_phar = torch.cat([phar['x'], phar['one_hot']], dim=1)
        xh0_pocket = torch.cat([pocket['x'], pocket['one_hot']], dim=1)
        cx, cp = self.remove_mean_batch(xh0_phar[:, :nd], xh0_pocket[:, :nd], phar['mask'], pocket['mask'])
        xh0_phar = torch.cat([cx, xh0_phar[:, nd:]], 1)
        xh0_pocket = torch.cat([cp, xh0_pocket[:, nd:]], 1)
        draws = iter(eps) if eps is not None else None
        nxt = (lambda: next(draws).to(dev)) if draws is not None else (lambda: None)
        z_t, xh_pocket, eps_t = self.noised_representation(xh0_phar, xh0_pocket, phar['mask'], pocket['mask'],
                                                           gamma_t, nxt())
        net_out, _ = (_net or self.dynamics)(z_t, xh_pocket, t, phar['mask'], pocket['mask'])
        xh_phar_hat = self.xh_given_zt_and_epsilon(z_t, net_out, gamma_t, phar['mask'])
        error_t = self.sum_except_batch((eps_t - net_out) ** 2, phar['mask'], B)
        SNR_weight = (1 - self.SNR(gamma_s - gamma_t)).squeeze(1)
        assert error_t.size() == SNR_weight.size()
        self._last_train_ctx = {'eps_t': eps_t, 'net_out': net_out, 't_is_zero': t_is_zero, 'SNR_weight': SNR_weight}
        neg_log_constants = -self.log_constants_p_x_given_z0(n_nodes=phar['size'], device=dev)
        kl_prior = self.kl_prior(xh0_phar, phar['mask'], phar['size'])
        if self.training:
            lpx, lph = self.log_pxh_given_z0_without_constants(phar, z_t, eps_t, net_out, gamma_t)
            loss_0_x, loss_0_h = -lpx * t_is_zero.squeeze(), -lph * t_is_zero.squeeze()
            error_t = error_t * (1 - t_is_zero).squeeze()
        else:
            t_zeros = torch.zeros_like(s)
            gamma_0 = self.inflate_batch_array(self.gamma(t_zeros), phar['x'])
            z_0, xh_pocket0, eps_0 = self.noised_representation(xh0_phar, xh0_pocket, phar['mask'], pocket['mask'],
                                                                gamma_0, nxt())
            net_out_0, _ = self.dynamics(z_0, xh_pocket0, t_zeros, phar['mask'], pocket['mask'])
            lpx, lph = self.log_pxh_given_z0_without_constants(phar, z_0, eps_0, net_out_0, gamma_0)
            loss_0_x, loss_0_h = -lpx, -lph
        log_pN = self.log_pN(phar['size'], pocket['size'])
        cnt = self._seg_sum(torch.ones(len(phar['mask']), device=dev), phar['mask'], B).clamp(min=1)
        info = {'eps_hat_phar_x': (self._seg_sum(net_out[:, :nd].abs().mean(1), phar['mask'], B) / cnt).mean(),
                'eps_hat_phar_h': (self._seg_sum(net_out[:, nd:].abs().mean(1), phar['mask'], B) / cnt).mean()}
        terms = (delta_log_px, error_t, torch.tensor(0.0), SNR_weight, loss_0_x, torch.tensor(0.0), loss_0_h,
                 neg_log_constants, kl_prior, log_pN, t_int.squeeze(), xh_phar_hat)
        return (*terms, info) if return_info else terms

    @classmethod
    def remove_mean_batch(cls, x_phar, x_pocket, phar_indices, pocket_indices):
        """Subtract the phar centre of mass from both node sets (conditional_model.py:467-475)."""
        n = int(phar_indices.max()) + 1 if phar_indices.numel() else 0
        tot = torch.zeros((n, x_phar.size(1)), dtype=x_phar.dtype, device=x_phar.device).index_add_(0, phar_indices, x_phar)
        cnt = torch.zeros(n, dtype=x_phar.dtype, device=x_phar.device).index_add_(
            0, phar_indices, torch.ones(len(phar_indices), dtype=x_phar.dtype, device=x_phar.device)).clamp(min=1)
        mean = tot / cnt[:, None]
        return x_phar - mean[phar_indices], x_pocket - mean[pocket_indices]

    @torch.no_grad()
    def sample_given_pocket(self, pocket, num_nodes_phar, return_frames=1, timesteps=None,
                            noise=None, seed=None, pocket_ids=None):
        """Draw samples given pockets (conditional_model.py:388-465).

        Reference arguments: pocket dict(x, one_hot, size, mask), num_nodes_phar [B],
        return_frames, timesteps.  Extensions (keyword-only in spirit):
          noise      [K+2, Nl, 3+phar_nf] Gaussian draws to inject (parity / reproducibility);
          seed       Philox seed for on-device draws (default: a fresh one per call from torch's global generator);
          pocket_ids global pocket indices so a shard draws the same noise as the full batch.
        Returns (xh_phar, xh_pocket, phar_mask, pocket_mask) like the reference; with
        return_frames > 1 the first two carry a leading frame axis.
        """
        timesteps = self._checked_frames(timesteps, return_frames)
        ps = self._one_pocket(pocket)
        nph = self._prior_sizes(num_nodes_phar, ps)
        return self._run_chain('sample_chain', ps, nph, timesteps, return_frames=return_frames, noise=noise, seed=seed, ids=pocket_ids)

    # ---- what the chain methods below share
    def _checked_frames(self, timesteps, return_frames):
        timesteps = self.T if timesteps is None else timesteps
        assert 0 < return_frames <= timesteps
        assert timesteps % return_frames == 0
        return timesteps

    @staticmethod
    def _check_mask_order(mask, what):
        if mask.numel() > 1 and bool((mask[1:] < mask[:-1]).any()):
            raise ValueError(f'{what} must be ascending and contiguous')

    # The pocket side of an entry - one pocket per sample, or a group of pockets per sample - is what the run and the epilogue need of it:
    # n owners (samples or groups), sizes, device, layout(nph) for set_layout, args (the leading arguments of the Handle's chain method), ids
    # (the name of its Philox-id keyword), split (xh_pocket back per pocket) and masks (as the entry returns them).
    def _one_pocket(self, pocket, masks='pocket mask'):
        """The pocket side of the single-pocket entries (masks: what the mask is called in the refusal)."""
        self._check_mask_order(pocket['mask'], masks)
        sizes = pocket['size'].detach().to('cpu', torch.int64).numpy()
        f32 = lambda t: t.detach().to(torch.float32).contiguous()
        return SimpleNamespace(grouped=False, n=len(sizes), sizes=sizes, device=pocket['x'].device, layout=lambda nph: (nph, sizes),
                               args=(f32(pocket['x']), f32(pocket['one_hot'])), ids='pocket_ids', split=lambda xh_pocket: xh_pocket,
                               masks=pocket['mask'])

    def _pocket_groups(self, pockets, weights):
        """The pocket side of the *_given_pockets entries: M pocket dicts batched over the same G groups, in the member layout."""
        pockets, M, G = self._checked_pockets(pockets)
        w = self.group_weights(weights, G, M)
        sizes, rows, px, poh = self._member_layout(pockets, M, G)
        return SimpleNamespace(grouped=True, n=G, M=M, w=w, sizes=sizes, device=pockets[0]['x'].device,
                               layout=lambda nph: (np.repeat(nph, M), sizes.reshape(-1)), args=(px, poh, [M] * G, w.reshape(-1)), ids='group_ids',
                               split=lambda xh_pocket: [xh_pocket[..., r, :] for r in rows], masks=[q['mask'] for q in pockets])

    @staticmethod
    def _prior_sizes(num_nodes_phar, ps):
        """num_nodes_phar of an entry that starts from the prior, one per owner of the pocket side -> host int64 array."""
        nph = torch.as_tensor(num_nodes_phar).detach().to('cpu', torch.int64).numpy()
        if not ps.grouped:
            assert len(nph) == ps.n
            return nph
        if len(nph.reshape(-1)) != ps.n:
            raise ValueError(f'num_nodes_phar has {len(nph.reshape(-1))} entries for {ps.n} groups')
        return nph.reshape(-1)

    def _given_sizes(self, phar, ps):
        """The sizes of a GIVEN pharmacophore, batched over the owners of the pocket side with a sorted mask -> host int64 array.  (Per
        group its rows are checked here; per sample the Handle checks them.)"""
        nph = phar['size'].detach().to('cpu', torch.int64).numpy().reshape(-1)
        if len(nph) != ps.n:
            raise ValueError(f'phar has {len(nph)} samples, pocket {ps.n}')
        self._check_mask_order(phar['mask'], 'batch masks')
        if ps.grouped:
            self._check_phar_rows(phar, int(nph.sum()))
        return nph

    def _given_rows(self, phar, ps, fix_coords, fix_types):
        """The given side of the edit entries -> (nph, the device tensors the Handle takes behind the pocket side's: x, one_hot, fix_x, fix_h)."""
        nph = self._given_sizes(phar, ps)
        f32 = lambda t: t.detach().to(ps.device, torch.float32).contiguous()
        masks = [self._row_mask(v, name, int(nph.sum()), ps.device) for v, name in ((fix_coords, 'fix_coords'), (fix_types, 'fix_types'))]
        return nph, (f32(phar['x']), f32(phar['one_hot']), *masks)

    @staticmethod
    def _guide_kw(restraints, nph, clash, scale, max_shift, guide_below, owner='sample'):
        """The guidance arguments of the restrained entries, checked -> (the records, the scalar keyword arguments of the Handle's
        restrained chains).  owner: what a restraint's 'sample' is called in the refusals ('group' where the records belong to the groups)."""
        from .. import restraints as rs
        rec = rs.records(restraints, nph, owner=owner)
        clash_r, clash_k = rs.clash_pair(clash)
        scale, max_shift, guide_below = rs.check_scalars(scale, rs.DEFAULT_MAX_SHIFT if max_shift is None else max_shift, guide_below)
        return rec, dict(clash_radius=clash_r, clash_k=clash_k, scale=scale, max_shift=max_shift, guide_below=guide_below)

    def _run_chain(self, method, ps, nph, timesteps, *, given=(), plan=None, behind=(), steer=None, info=None, frames=(1, 1), return_frames=1,
                   noise, seed, ids):
        """What the sampling entries share once their arguments are checked: prepare the handle, run the Handle's `method` on the pocket
        side ps, finish, split the pockets back.  given: the device tensors of _given_rows, with plan: dict(start, resamplings,
        jump_length) as that method takes them (the noise must cover the plan's draws); steer: the keyword arguments of a guided or diverse
        chain (behind: what a from-prior one takes by position behind timesteps, its records or set sizes), with info: the names
        _finish_with_info reports its side outputs under; frames: (resamplings, jump_length) of the frame schedule.
        -> (xh_phar, xh_pocket as ps splits it, phar_mask, ps.masks) and the info dict, if any."""
        edit_plan = None if plan is None else (plan.get('start', timesteps), plan['resamplings'], plan['jump_length'])
        h, phar_mask, noise, seed = self._prepare_sample(nph, ps.layout(nph), ps.device, timesteps, noise, seed, steer is not None, edit_plan)
        kw = {**(plan or {}), **(steer or {}), 'noise': noise, 'seed': seed, ps.ids: ids, 'want_steps': return_frames > 1,
              'use_graph': self.use_hip_graph}
        run = lambda: getattr(h, method)(*ps.args, *given, timesteps, *behind, **kw)
        # frames: idx = s*return_frames//timesteps for steps with (s*return_frames) % timesteps == 0
        # (conditional_model.py:439-442); frame 0 is overwritten by the final sample (:460-461).
        frame_of_step = self.inpaint_frames(*frames, timesteps, return_frames)
        if info is None:
            out = self._finish_chain(h, run, frame_of_step, return_frames)
            return out[0], ps.split(out[1]), phar_mask, ps.masks
        out, info = self._finish_with_info(h, run, frame_of_step, return_frames, info)
        return out[0], ps.split(out[1]), phar_mask, ps.masks, info

    def _prepare_sample(self, nph, layout, device, timesteps, noise, seed, guide=False, plan=None):
        """The sample family's preparation once the arguments are checked: the learned schedule, the handle with `layout` (num_phar and
        num_pocket of every sample of the device layout), the step table (guide: and the guide table), the phar mask of nph (one entry per
        sample or group), the noise on the device and a seed.  plan: (start, resamplings, jump_length) of an edit chain, whose draws the
        noise must cover.  -> (h, phar_mask, noise, seed)."""
        self.refresh_learned_schedule()
        h = self.dynamics.hip_handle()
        h.set_layout(*layout)
        h.set_step_table(timesteps, self.step_table(timesteps))
        if guide:
            h.set_guide_table(timesteps, self.guide_table(timesteps))
        if noise is not None:
            noise = noise.detach().to(device, torch.float32).contiguous()
        if plan is not None:
            n_steps, n_draws = h.edit_plan(timesteps, *plan)
            if noise is not None and (noise.dim() != 3 or noise.shape[0] < n_draws):
                raise ValueError(f'noise has shape {tuple(noise.shape)}: this schedule needs {n_draws} draws of '
                                 f'[{int(nph.sum())}, {3 + self.phar_nf}]')
        if seed is None:
            seed = fresh_seed()
        return h, utils.num_nodes_to_batch_mask(len(nph), torch.as_tensor(nph), device), noise, seed

    def _checked_start(self, timesteps, start):
        """edit's timesteps and start level, checked -> (timesteps, start) as ints."""
        timesteps = self.T if timesteps is None else int(timesteps)
        start = timesteps if start is None else start
        if int(start) != start or not 1 <= int(start) <= timesteps:
            raise ValueError(f'start={start} must be an integer level in [1, timesteps={timesteps}]')
        return timesteps, int(start)

    def _check_phar_rows(self, phar, n_phar):
        if tuple(phar['x'].shape) != (n_phar, self.n_dims) or tuple(phar['one_hot'].shape) != (n_phar, self.phar_nf):
            raise ValueError(f"phar x / one_hot have shapes {tuple(phar['x'].shape)} / {tuple(phar['one_hot'].shape)}: expected "
                             f'[{n_phar}, {self.n_dims}] / [{n_phar}, {self.phar_nf}] (sum(size) rows)')

    ENERGY_INFO = ('energy', 'max_violation', 'op_energy')          # of the restrained chains: energy [owners, 2], op_energy
    OVERLAP_INFO = ('overlap', 'op_overlap')                        # of the diverse chain: overlap [B], op_overlap

    def _finish_with_info(self, h, run, frame_of_step, return_frames, names):
        """_finish_chain for a chain with side outputs, whose run() returns (xh_phar, xh_pocket, z_steps) and then one pair (per owner,
        per op and owner) for every steering part.  names: the info key of every column of the per-owner output (one name: of the output
        itself), then the per-op output's - or, for a chain with several parts, a tuple of such tuples, one per pair.
        -> (_finish_chain's result, the info dict - the per-op entries only with return_frames > 1)."""
        extra = []

        def run3():
            out = run()
            extra[:] = out[3:]
            return out[:3]

        out = self._finish_chain(h, run3, frame_of_step, return_frames)
        info = {}
        for pair, (*cols, per_op) in enumerate(names if isinstance(names[0], tuple) else (names,)):
            per_owner, per_op_out = extra[2 * pair], extra[2 * pair + 1]
            info.update({cols[0]: per_owner} if len(cols) == 1 else {name: per_owner[:, c].clone() for c, name in enumerate(cols)})
            if return_frames > 1:
                info[per_op] = per_op_out
        return out, info

    def _level_noise(self, noise, R, K, n_phar, device):
        """The injected draws of a scoring call (None: device draws) as float32 [R (K + 1), n_phar, 3+P] on `device`, checked."""
        if noise is None:
            return None
        noise, ld = noise.detach().to(device, torch.float32).contiguous(), self.n_dims + self.phar_nf
        if noise.dim() == 4:
            noise = noise.reshape(-1, noise.shape[2], noise.shape[3])
        if tuple(noise.shape) != (R * (K + 1), n_phar, ld):
            raise ValueError(f'noise has shape {tuple(noise.shape)}: {R} x {K + 1} levels need [{R * (K + 1)}, {n_phar}, {ld}]')
        return noise

    @torch.no_grad()
    def sample_restrained(self, pocket, num_nodes_phar, restraints, clash=None, scale=1.0, max_shift=None, guide_below=1.0,
                          return_frames=1, timesteps=None, noise=None, seed=None, pocket_ids=None):
        """sample_given_pocket BIASED toward a geometric query: the same chain (ops, draws, Philox counters) with a guidance term in
        the mean of every posterior op - the gradient of a restraint energy at the denoised estimate, times the op's posterior variance
        (cmdgen_restrained_chain; the header of csrc/kernels_restrain.hip defines every term).  The whole chain runs on the device.

        restraints: list of dicts (cmdgen_amd/restraints.py), centres in the frame of pocket['x'], lengths in Angstrom:
          {'kind': 'position', 'sample': b, 'point': i, 'center': (x, y, z), 'radius': r, 'k': k}
          {'kind': 'distance', 'sample': b, 'points': (i, j), 'lo': lo, 'hi': hi, 'k': k}
          {'kind': 'exclusion', 'sample': b, 'center': (x, y, z), 'radius': r, 'k': k}
        clash: None, a radius, or (radius, k): no point within the radius of a pocket atom, for every sample.  scale multiplies the
        guidance (0: sample_given_pocket, bit for bit); max_shift (A, default restraints.DEFAULT_MAX_SHIFT) caps a point's
        displacement per op; ops with t / T > guide_below are not guided.  The other arguments as sample_given_pocket.
        Returns sample_given_pocket's tuple plus {'energy': [B], 'max_violation': [B]} of the returned sample (and 'op_energy'
        [timesteps, B], the energy at every op's denoised estimate, when return_frames > 1)."""
        timesteps = self._checked_frames(timesteps, return_frames)
        ps = self._one_pocket(pocket)
        nph = self._prior_sizes(num_nodes_phar, ps)
        rec, steer = self._guide_kw(restraints, nph, clash, scale, max_shift, guide_below)
        return self._run_chain('restrained_chain', ps, nph, timesteps, behind=(rec,), steer=steer, info=self.ENERGY_INFO, return_frames=return_frames,
                               noise=noise, seed=seed, ids=pocket_ids)

    @torch.no_grad()
    def sample_diverse(self, pocket, num_nodes_phar, set_sizes, strength=1.0, width=2.0, max_shift=None, guide_below=1.0,
                       return_frames=1, timesteps=None, noise=None, seed=None, pocket_ids=None):
        """sample_given_pocket with the samples drawn for one pocket PUSHED APART: the same chain (ops, draws, Philox counters) with a
        term in the mean of every posterior op that couples the samples of a set - the gradient of their Gaussian overlap at the denoised
        estimates, times the op's posterior variance: particle guidance (cmdgen_diverse_chain; the header of csrc/kernels_diverse.hip
        defines every term).  The whole chain runs on the device, on one handle: a set is never split.

        set_sizes: the batch partitioned into sets of consecutive samples, "the draws for one pocket" (a set's pockets are normally
        copies of one pocket, given in one frame; that is not checked, and the members' numbers of points differ freely).  strength
        (dimensionless; 0: sample_given_pocket, bit for bit) and width (A) shape the overlap exp(-r^2 / (2 width^2)) between points of
        different samples of a set; max_shift (A, default restraints.DEFAULT_MAX_SHIFT) caps a point's displacement per op; ops with
        t / T > guide_below are not guided.  The other arguments as sample_given_pocket.
        Returns sample_given_pocket's tuple plus {'overlap': [B]}, the mean overlap of every returned sample with the others of its set
        (0 for a set of one) - and 'op_overlap' [timesteps, B], the same at every op's denoised estimate, when return_frames > 1."""
        from .. import restraints as rs
        timesteps = self._checked_frames(timesteps, return_frames)
        ps = self._one_pocket(pocket)
        nph = self._prior_sizes(num_nodes_phar, ps)
        sets = rs.check_set_sizes(set_sizes, nph)
        strength, width, max_shift, guide_below = rs.check_diverse_scalars(strength, width, rs.DEFAULT_MAX_SHIFT if max_shift is None else max_shift,
                                                                           guide_below)
        steer = dict(strength=strength, width=width, max_shift=max_shift, guide_below=guide_below)
        return self._run_chain('diverse_chain', ps, nph, timesteps, behind=(sets,), steer=steer, info=self.OVERLAP_INFO, return_frames=return_frames,
                               noise=noise, seed=seed, ids=pocket_ids)

    @torch.no_grad()
    def sample_diverse_restrained(self, pocket, num_nodes_phar, set_sizes, restraints, clash=None, scale=1.0, strength=1.0, width=2.0,
                                  max_shift=None, guide_below=1.0, diverse_max_shift=None, diverse_guide_below=None, return_frames=1,
                                  timesteps=None, noise=None, seed=None, pocket_ids=None):
        """sample_diverse UNDER sample_restrained's restraints: different samples for one pocket that all keep a geometric query.  The same
        chain (ops, draws, Philox counters) with both terms in the mean of every posterior op, both taken at the op's denoised estimate:
        first the restraint term of sample_restrained, then the overlap term of sample_diverse, each with the definition and the scalars of
        its own method (cmdgen_diverse_restrained_chain; the header of k_diverse_restrained_step_count in csrc/kernels_restrain.hip).  The
        whole chain runs on the device, on one handle.

        set_sizes, strength and width as sample_diverse; restraints, clash and scale as sample_restrained.  max_shift and guide_below
        belong to the restraint term; the overlap term has its own diverse_max_shift and diverse_guide_below (None: the restraint
        side's values).  strength = 0 is sample_restrained and scale = 0 is sample_diverse, bit for bit.
        Returns sample_given_pocket's tuple plus {'energy': [B], 'max_violation': [B], 'overlap': [B]} of the returned sample (and
        'op_energy', 'op_overlap' [timesteps, B] at every op's denoised estimate when return_frames > 1)."""
        from .. import restraints as rs
        timesteps = self._checked_frames(timesteps, return_frames)
        ps = self._one_pocket(pocket)
        nph = self._prior_sizes(num_nodes_phar, ps)
        rec, steer = self._guide_kw(restraints, nph, clash, scale, max_shift, guide_below)
        sets = rs.check_set_sizes(set_sizes, nph)
        strength, width, diverse_max_shift, diverse_guide_below = rs.check_diverse_scalars(
            strength, width, steer['max_shift'] if diverse_max_shift is None else diverse_max_shift,
            steer['guide_below'] if diverse_guide_below is None else diverse_guide_below)
        steer.update(strength=strength, width=width, diverse_max_shift=diverse_max_shift, diverse_guide_below=diverse_guide_below)
        return self._run_chain('diverse_restrained_chain', ps, nph, timesteps, behind=(sets, rec), steer=steer,
                               info=(self.ENERGY_INFO, self.OVERLAP_INFO), return_frames=return_frames, noise=noise, seed=seed, ids=pocket_ids)

    @staticmethod
    def group_weights(weights, n_groups, n_members):
        """weights None (uniform), [M] or [G, M] -> float32 numpy [G, M], every row normalised to sum 1 in float64."""
        if weights is None:
            w = np.ones((n_groups, n_members), dtype=np.float64)
        else:
            w = np.asarray(torch.as_tensor(weights).detach().cpu().numpy(), dtype=np.float64)
            if w.shape == (n_members,):
                w = np.broadcast_to(w, (n_groups, n_members)).copy()
            elif w.shape != (n_groups, n_members):
                raise ValueError(f'weights has shape {tuple(w.shape)}: expected [{n_members}] (one per pocket) or '
                                 f'[{n_groups}, {n_members}] (per group and pocket)')
        if not np.isfinite(w).all() or (w < 0).any():
            raise ValueError('weights must be finite and >= 0')
        tot = w.sum(axis=1, keepdims=True)
        if (tot <= 0).any():
            raise ValueError('the weights of a group sum to zero')
        return (w / tot).astype(np.float32)

    @torch.no_grad()
    def sample_given_pockets(self, pockets, num_nodes_phar, weights=None, return_frames=1, timesteps=None,
                             noise=None, seed=None, group_ids=None):
        """Draw ONE pharmacophore per group of pockets (dual-target design, or an ensemble of conformations of one receptor): one
        chain whose latent is shared by the group's pockets.  At every step the eps-predictions of the pocket contexts are combined
        with the weights - the score of the weighted geometric mixture of the per-pocket distributions - and the step is
        sample_given_pocket's otherwise; the shared latent stays centre-of-mass free and every pocket carries its own translated copy
        (cmdgen_multi_pocket_chain: its header gives the ops, the draw layout and the Philox counters).

        pockets: list of M pocket dicts (x, one_hot, size [G], mask) as sample_given_pocket takes one, each batched over the same G
        groups: group g samples one pharmacophore for pockets[0] .. pockets[M-1] of g.  The pockets of a group must be given in ONE
        common frame - superposing the structures is the caller's business; sizes and compositions differ freely.
        num_nodes_phar [G]; weights None (uniform), [M] or [G, M], >= 0, normalised per group in float64 and cast to float32;
        noise [K+2, Nu, 3+phar_nf] (one draw per group and op, Nu = sum(num_nodes_phar)); seed as in sample_given_pocket; group_ids
        [G] global group ids of the Philox draws.  With M = 1 this is sample_given_pocket, bit for bit.
        Returns (xh_phar [Nu, 3+P], [xh_pocket_m], phar_mask, [pocket_mask_m]); with return_frames > 1 the tensors carry the leading
        frame axis of sample_given_pocket."""
        ps = self._pocket_groups(pockets, weights)
        nph = self._prior_sizes(num_nodes_phar, ps)
        timesteps = self._checked_frames(timesteps, return_frames)
        return self._run_chain('multi_pocket_chain', ps, nph, timesteps, return_frames=return_frames, noise=noise, seed=seed, ids=group_ids)

    @torch.no_grad()
    def sample_restrained_given_pockets(self, pockets, num_nodes_phar, restraints, weights=None, clash=None, scale=1.0, max_shift=None,
                                        guide_below=1.0, return_frames=1, timesteps=None, noise=None, seed=None, group_ids=None):
        """sample_given_pockets BIASED toward a geometric query, sample_restrained's guidance on the latent the group's pockets share
        (cmdgen_multi_restrained_chain; the header of csrc/kernels_restrain.hip defines every term): "one pharmacophore for both kinases,
        a donor at the shared hinge position, a hydrophobe 5-7 A from it, off the atoms of EITHER pocket".

        pockets, num_nodes_phar [G], weights, noise, seed and group_ids as sample_given_pockets.  restraints: the dicts of
        sample_restrained, each naming its GROUP under 'sample'; point indices are rows of the group's pharmacophore, centres lie in the
        common frame the group's pockets are given in.  The guidance is computed once per group: the frame shift follows the group's
        FIRST pocket, the clash term (clash: None, a radius, or (radius, k)) sums over the atoms of EVERY pocket of the group, unweighted.
        scale, max_shift and guide_below as sample_restrained (scale = 0: sample_given_pockets, bit for bit).
        Returns sample_given_pockets' tuple plus {'energy': [G], 'max_violation': [G]} of the returned sample against all its pockets
        (and 'op_energy' [timesteps, G] when return_frames > 1)."""
        ps = self._pocket_groups(pockets, weights)
        nph = self._prior_sizes(num_nodes_phar, ps)
        timesteps = self._checked_frames(timesteps, return_frames)
        rec, steer = self._guide_kw(restraints, nph, clash, scale, max_shift, guide_below)  # per group: 'sample' is the group index
        return self._run_chain('multi_restrained_chain', ps, nph, timesteps, behind=(rec,), steer=steer, info=self.ENERGY_INFO,
                               return_frames=return_frames, noise=noise, seed=seed, ids=group_ids)

    @staticmethod
    def _checked_pockets(pockets):
        """The pocket dicts of sample_given_pockets / edit_given_pockets as a list, with M (pockets per group) and G (groups)."""
        pockets = list(pockets)
        if not pockets:
            raise ValueError('pockets is empty: expected a list of pocket dicts')
        M, G = len(pockets), len(pockets[0]['size'])
        if M > 8:
            raise ValueError(f'{M} pockets per group: the multi-pocket chain takes at most 8')
        for m, q in enumerate(pockets):
            if len(q['size']) != G:
                raise ValueError(f"pockets[{m}] holds {len(q['size'])} groups, pockets[0] {G}: every dict is batched over the same groups")
            ConditionalDDPM._check_mask_order(q['mask'], 'pocket mask')
        return pockets, M, G

    def _member_layout(self, pockets, M, G):
        """The member layout of the multi-pocket chains: sample g * M + m is pocket m of group g.  -> (sizes [G, M], per m its rows in
        the member layout, pocket x and one_hot of all members in that layout)."""
        device = pockets[0]['x'].device
        sizes = np.stack([q['size'].detach().to('cpu', torch.int64).numpy() for q in pockets], axis=1)       # [G, M]
        base = np.concatenate([[0], np.cumsum(sizes.reshape(-1))])                                           # [G * M + 1] first row of every member
        rows = []                                                                                            # per m: its rows in the member layout
        for m, q in enumerate(pockets):
            start = np.concatenate([[0], np.cumsum(sizes[:, m])[:-1]])
            g_of = np.repeat(np.arange(G), sizes[:, m])
            rows.append(torch.from_numpy(base[g_of * M + m] + np.arange(len(g_of)) - start[g_of]).to(device))
        n_rows = int(base[-1])
        f32 = lambda t: t.detach().to(device, torch.float32)
        px = torch.empty((n_rows, self.n_dims), dtype=torch.float32, device=device)
        poh = torch.empty((n_rows, self.residue_nf), dtype=torch.float32, device=device)
        for r, q in zip(rows, pockets):
            if len(q['x']) != len(r):
                raise ValueError("a pocket's x does not have sum(size) rows")
            px[r], poh[r] = f32(q['x']), f32(q['one_hot'])
        return sizes, rows, px, poh

    @torch.no_grad()
    def inpaint(self, phar, pocket, phar_fixed, resamplings=1, jump_length=1, return_frames=1, timesteps=None,
                noise=None, seed=None, pocket_ids=None):
        """Sample given pockets while holding some pharmacophore points: RePaint (the joint model's loop,
        en_diffusion.py:672-831) on this model's own steps.  An op of get_repaint_schedule(resamplings, jump_length,
        timesteps) is sample_p_zs_given_zt, then the given rows noised to the op's s by q(z_s | x) and moved into the
        current frame by the pocket's shift replace the fixed rows, then the phar COM projection; before a jump back,
        sample_p_zt_given_zs re-noises.  The frame is the one of sample_given_pocket (phar COM at zero, the pocket a
        translated copy); both inputs are normalised here (unlike the joint model's inpaint, quirk Q14).
        The whole chain runs on the device (cmdgen_inpaint_chain; its header gives the op and the draw layout).

        phar: dict(x [Nl,3], one_hot [Nl,P], size [B], mask [Nl]) - only rows with phar_fixed set are read;
        pocket: as in sample_given_pocket; phar_fixed: [Nl] or [Nl,1] floats or bools.
        noise [n_draws, Nl, 3+P] (Handle.inpaint_plan), seed and pocket_ids as in sample_given_pocket.
        Returns (xh_phar, xh_pocket, phar_mask, pocket_mask) like sample_given_pocket; with return_frames > 1
        (jump_length 1 only) the frames are the states at the end of each resample cycle, frame 0 the final sample.
        """
        timesteps = self._checked_frames(timesteps, return_frames)
        if return_frames > 1 and jump_length != 1:
            raise ValueError('return_frames > 1 is only implemented for jump_length=1 (as in the joint model\'s inpaint)')
        ps = self._one_pocket(pocket, masks='batch masks')
        nph = self._given_sizes(phar, ps)
        n_phar = int(nph.sum())
        fixed = torch.as_tensor(phar_fixed).detach().to(ps.device, torch.float32)
        if fixed.dim() == 2 and fixed.shape[1] == 1:
            fixed = fixed[:, 0]
        if fixed.dim() != 1 or fixed.numel() != n_phar:
            raise ValueError(f'phar_fixed has shape {tuple(torch.as_tensor(phar_fixed).shape)}: expected [{n_phar}] or [{n_phar}, 1]')
        f32 = lambda t: t.detach().to(ps.device, torch.float32).contiguous()
        return self._run_chain('inpaint_chain', ps, nph, timesteps, given=(f32(phar['x']), f32(phar['one_hot']), fixed.contiguous()),
                               plan=dict(resamplings=resamplings, jump_length=jump_length), frames=(resamplings, jump_length),
                               return_frames=return_frames, noise=noise, seed=seed, ids=pocket_ids)

    def _row_mask(self, value, name, n_phar, device):
        """A per-row mask argument ([Nl] or [Nl,1], bools or floats; None: no row) as float [Nl] on `device`."""
        if value is None:
            return torch.zeros(n_phar, dtype=torch.float32, device=device)
        m = torch.as_tensor(value).detach()
        shape = tuple(m.shape)
        if m.dim() == 2 and m.shape[1] == 1:
            m = m[:, 0]
        if m.dim() != 1 or m.numel() != n_phar:
            raise ValueError(f'{name} has shape {shape}: expected [{n_phar}] or [{n_phar}, 1]')
        return (m != 0).to(device, torch.float32).contiguous()

    @torch.no_grad()
    def edit(self, phar, pocket, fix_coords=None, fix_types=None, start=None, resamplings=1, jump_length=1, timesteps=None,
             noise=None, seed=None, pocket_ids=None):
        """Modify a GIVEN pharmacophore in its pocket: ``inpaint`` with a mask per column group and a start level.

        fix_coords / fix_types ([Nl] or [Nl,1], bools or floats; None: nothing held) hold a row's position / its feature type at
        the noised copy of the given row, independently: types held and coordinates free re-places the points, the reverse
        re-types them; both marked is ``inpaint``'s fixed row.  ``start`` in 1 .. timesteps is the level the chain begins at:
        None or timesteps is the prior (z_T around the pocket centre, as sample_given_pocket); below it the chain begins at
        q(z_start | phar) as ``forward`` forms it (both node sets centred on the phar centre of mass, noised_representation) and
        walks s = start-1 .. 0 with get_repaint_schedule(resamplings, jump_length, start) - then every row of phar is read.
        The whole chain runs on the device (cmdgen_edit_chain; its header gives the ops, the draw layout and the Philox
        counters).  noise [n_draws, Nl, 3+P] (Handle.edit_plan), seed and pocket_ids as in sample_given_pocket.
        Returns (xh_phar, xh_pocket, phar_mask, pocket_mask) like sample_given_pocket."""
        timesteps, start = self._checked_start(timesteps, start)
        ps = self._one_pocket(pocket, masks='batch masks')
        nph, given = self._given_rows(phar, ps, fix_coords, fix_types)
        return self._run_chain('edit_chain', ps, nph, timesteps, given=given,
                               plan=dict(start=start, resamplings=resamplings, jump_length=jump_length), noise=noise, seed=seed, ids=pocket_ids)

    @torch.no_grad()
    def edit_restrained(self, phar, pocket, restraints, fix_coords=None, fix_types=None, start=None, resamplings=1, jump_length=1,
                        clash=None, scale=1.0, max_shift=None, guide_below=1.0, timesteps=None, noise=None, seed=None, pocket_ids=None):
        """``edit`` STEERED by ``sample_restrained``'s geometric query: keep some given points and grow or re-place the others under
        position, distance, exclusion and clash terms.  The chain is ``edit``'s (the same start, ops, draws, Philox counters, merge, jumps
        and decode) with the guidance term of ``sample_restrained`` in the posterior op (op A) of every op; the jump-back op and the decode
        are not guided (cmdgen_restrained_edit_chain; the header of k_restrained_edit_step_count in csrc/kernels_restrain.hip defines it).
        A point whose coordinates are held enters the restraint energy at its GIVEN position (moved into the chain's frame) and is not
        displaced, so a distance window between a held and a free point pulls the free one toward the true held position; a point with
        only its type held is steered like a free one.

        phar, pocket, fix_coords, fix_types, start, resamplings, jump_length, timesteps, noise, seed, pocket_ids as ``edit``; restraints
        (list of dicts, centres in the frame of pocket['x']), clash, scale, max_shift, guide_below as ``sample_restrained``.  With no
        restraint and no clash term, or scale = 0, the result is ``edit``'s bit for bit.
        Returns (xh_phar, xh_pocket, phar_mask, pocket_mask, {'energy': [B], 'max_violation': [B]}): the energy and the largest violation
        (A) of the returned sample, held points included at their returned positions."""
        timesteps, start = self._checked_start(timesteps, start)
        ps = self._one_pocket(pocket, masks='batch masks')
        nph, given = self._given_rows(phar, ps, fix_coords, fix_types)
        rec, steer = self._guide_kw(restraints, nph, clash, scale, max_shift, guide_below)
        return self._run_chain('restrained_edit_chain', ps, nph, timesteps, given=given,
                               plan=dict(start=start, resamplings=resamplings, jump_length=jump_length), steer=dict(steer, restraints=rec),
                               info=self.ENERGY_INFO, noise=noise, seed=seed, ids=pocket_ids)

    @torch.no_grad()
    def edit_given_pockets(self, phar, pockets, fix_coords=None, fix_types=None, start=None, resamplings=1, jump_length=1,
                           weights=None, timesteps=None, noise=None, seed=None, group_ids=None):
        """Hold or edit GIVEN points while drawing one pharmacophore per group of pockets: ``edit``'s ops on the shared latent of
        ``sample_given_pockets`` - a dual-target design around a known anchor, a pharmacophore that fits one target adapted to a
        second one (start below timesteps), points re-typed or re-placed against an ensemble of conformations.

        phar: dict(x [Nu,3], one_hot [Nu,P], size [G], mask [Nu]) batched over the G groups, in the pockets' common frame; pockets,
        weights and group_ids as in sample_given_pockets; fix_coords, fix_types, start, resamplings and jump_length as in edit (masks
        [Nu] or [Nu,1]); noise [n_draws, Nu, 3+P] (Handle.edit_plan), one draw per group, op and role.  The offset that moves the
        given rows into the chain's frame is the group's: the shift of its first pocket, which every pocket of the group shares.
        The whole chain runs on the device (cmdgen_multi_edit_chain; its header gives the ops, the offset and the Philox counters).
        With one pocket this is edit, and with nothing held from the prior at resamplings = jump_length = 1 sample_given_pockets,
        both bit for bit.  Returns what sample_given_pockets returns: (xh_phar [Nu, 3+P], [xh_pocket_m], phar_mask, [pocket_mask_m])."""
        ps = self._pocket_groups(pockets, weights)
        timesteps, start = self._checked_start(timesteps, start)
        nph, given = self._given_rows(phar, ps, fix_coords, fix_types)
        return self._run_chain('multi_edit_chain', ps, nph, timesteps, given=given,
                               plan=dict(start=start, resamplings=resamplings, jump_length=jump_length), noise=noise, seed=seed, ids=group_ids)

    @torch.no_grad()
    def edit_restrained_given_pockets(self, phar, pockets, restraints, fix_coords=None, fix_types=None, start=None, resamplings=1,
                                      jump_length=1, weights=None, clash=None, scale=1.0, max_shift=None, guide_below=1.0, timesteps=None,
                                      noise=None, seed=None, group_ids=None):
        """``edit_given_pockets`` STEERED by ``sample_restrained_given_pockets``' geometric query - all three modifiers at once: keep the
        points known from one target, grow or re-place the others for every pocket of the group under position, distance, exclusion and
        clash terms.  The chain is ``edit_given_pockets``' (the same start, ops, draws, Philox counters, merge, jumps and decode) with the
        guidance of ``sample_restrained_given_pockets`` in the posterior op (op A) of every op, once per group; the jump-back op and the
        decode are not guided (cmdgen_multi_restrained_edit_chain; the header of k_multi_edit_guide in csrc/kernels_restrain.hip defines
        it).  A point whose coordinates are held enters the group's restraint energy at its GIVEN position (moved into the chain's frame by
        the shift of the group's first pocket) and is not displaced; a point with only its type held is steered like a free one.

        phar, pockets, fix_coords, fix_types, start, resamplings, jump_length, weights, timesteps, noise, seed and group_ids as
        ``edit_given_pockets``; restraints (the dicts name their GROUP under 'sample', centres in the pockets' common frame), clash,
        scale, max_shift and guide_below as ``sample_restrained_given_pockets``.  With no restraint and no clash term, or scale = 0, the
        result is ``edit_given_pockets``' bit for bit; with one pocket it is ``edit_restrained``'s.
        Returns (xh_phar [Nu, 3+P], [xh_pocket_m], phar_mask, [pocket_mask_m], {'energy': [G], 'max_violation': [G]}): the energy and the
        largest violation (A) of the returned sample against all its pockets, held points included at their returned positions."""
        ps = self._pocket_groups(pockets, weights)
        timesteps, start = self._checked_start(timesteps, start)
        nph, given = self._given_rows(phar, ps, fix_coords, fix_types)
        rec, steer = self._guide_kw(restraints, nph, clash, scale, max_shift, guide_below, owner='group')  # per group: 'sample' is the group index
        return self._run_chain('multi_restrained_edit_chain', ps, nph, timesteps, given=given,
                               plan=dict(start=start, resamplings=resamplings, jump_length=jump_length), steer=dict(steer, restraints=rec),
                               info=self.ENERGY_INFO, noise=noise, seed=seed, ids=group_ids)

    @torch.no_grad()
    def score(self, phar, pocket, timesteps=None, repeats=1, noise=None, seed=None, pocket_ids=None, return_levels=False):
        """How likely the model finds a GIVEN pharmacophore in its pocket: the per-sample negative log-likelihood bound of
        ``forward`` in eval mode (conditional_model.py:198-320 with lightning_modules.py:211-229), but over a fixed grid of
        noise levels instead of one random t - the whole level loop runs on the device (cmdgen_score_chain).

        Levels t_k = (k + 1) T / timesteps, k = 0 .. timesteps-1 (``timesteps`` must divide T; default T), each with a draw of
        its own, plus the t = 0 level:  loss_t = (T / timesteps) sum_k -0.5 w_k error_k.  timesteps = T is the diffusion part of
        the variational bound itself; smaller values are the reference's estimator on a fixed grid (cmdgen_amd/scoring.py).
        ``repeats`` evaluates the list that many times with distinct draws and returns the means (and '<name>_repeats' [R, B]).

        phar / pocket: dict(x, one_hot, size, mask) as ``forward`` takes them (raw; not modified).
        noise [repeats * (timesteps + 1), Nl, 3+phar_nf] (or [repeats, timesteps + 1, Nl, 3+phar_nf]) Gaussian draws to inject: row
        r (timesteps + 1) + k is level k of repeat r, the last row of a repeat the t = 0 level; seed / pocket_ids as in
        sample_given_pocket (the draws of a pocket do not depend on how a batch is sharded).
        -> dict of per-sample tensors [B]: nll, loss_t, loss_0_x, loss_0_h, neg_log_const_0, kl_prior, delta_log_px, log_pN; with
        return_levels also t_levels [timesteps + 1], level_terms [R, timesteps + 1, B], the weighted terms (the loss profile over t), and
        level_sums [R, timesteps + 1, B, 4], the raw sums of cmdgen_score_chain (error over all / the x columns, log p(h | z_0), reset flag).
        A level whose evaluation the NaN guard reset is reported (warning) and makes nll NaN for the whole batch: the reference
        resets batch-wide, and a reset is never summed in silently."""
        return self._score_with('score', self._one_pocket(pocket, masks='batch masks'), phar, timesteps, repeats, noise, seed, pocket_ids,
                                return_levels)

    @torch.no_grad()
    def score_given_pockets(self, phar, pockets, weights=None, timesteps=None, repeats=1, noise=None, seed=None, group_ids=None,
                            return_levels=False, return_members=False):
        """How likely the model finds a GIVEN pharmacophore under SEVERAL pockets at once: ``score`` for the sampler that
        ``sample_given_pockets`` runs, whose denoiser is eps_bar = sum_m w_m eps_m - the bound that ranks what sample_given_pockets or
        edit_given_pockets drew, or compares a known pharmacophore across target and anti-target.  (The sum of per-pocket ``score``s is
        not this quantity: the error of the combined prediction is not the sum of the members' errors.)

        phar: dict(x [Nu,3], one_hot [Nu,P], size [G], mask [Nu]) batched over the G groups, in the pockets' common frame; pockets,
        weights and group_ids as in sample_given_pockets; timesteps, repeats, seed and the NaN-reset warning as in score; noise
        [repeats * (timesteps + 1), Nu, 3+P] (or [repeats, timesteps + 1, Nu, 3+P]): ONE draw per group and level.  The whole level
        loop runs on the device (cmdgen_multi_score_chain; its header gives the definition and the Philox counters).  With one pocket
        this is score, bit for bit.
        -> score's dict per group [G]; log_pN = sum_m w_m log p(N_phar | N_pocket_m), the geometric mixture's term.  With
        return_members also member_nll, member_loss_t, member_loss_0_x, member_log_pN [G, M]: every pocket's own score on the SAME
        draws (what score gives for that pocket with the group's draws).  With return_levels also t_levels, level_terms
        [R, timesteps + 1, G], level_sums [R, timesteps + 1, G, 4] and, with return_members, member_level_sums [R, timesteps + 1, G, M, 4]."""
        return self._score_with('score_given_pockets', self._pocket_groups(pockets, weights), phar, timesteps, repeats, noise, seed, group_ids,
                                return_levels, return_members)

    def _score_with(self, entry, ps, phar, timesteps, repeats, noise, seed, ids, return_levels, return_members=False):
        """What score and score_given_pockets share: the level grid, the draws, the Handle's scoring chain on the pocket side ps, the
        assembly of the terms and the NaN-reset report (entry: the name it is reported under)."""
        from .. import scoring
        K = self.T if timesteps is None else int(timesteps)
        levels = scoring.level_list(self.T, K)                        # ValueError when K does not divide T
        R = int(repeats)
        if R < 1:
            raise ValueError(f'repeats={repeats} must be >= 1')
        nph = self._given_sizes(phar, ps)
        f32 = lambda t: t.detach().to(ps.device, torch.float32).contiguous()
        noise = self._level_noise(noise, R, K, int(nph.sum()), ps.device)
        self.refresh_learned_schedule()
        gamma = np.asarray(self.gamma_table_host(), dtype=np.float32)
        log_pn = self.size_distribution._table(1, torch.device('cpu')).detach().to(torch.float32).numpy()
        tab = scoring.level_table(gamma, self.T, self.n_dims, self.norm_values, levels)
        h = self.dynamics.hip_handle()
        h.set_layout(*ps.layout(nph))
        if seed is None:
            seed = fresh_seed()
        args = (f32(phar['x']), f32(phar['one_hot']), *ps.args)
        kw = {'noise': noise, 'seed': seed, ps.ids: ids, 'use_graph': self.use_hip_graph, **({'want_members': return_members} if ps.grouped else {})}
        run = lambda: getattr(h, 'multi_score_chain' if ps.grouped else 'score_chain')(*args, np.tile(levels, R),
                                                                                        level_coef=scoring.level_coef(tab, R), **kw)
        (terms, *members, kl), st = h.run_range_guarded(run, h.chain_status)
        self.last_chain_status = st
        assert st['max_rel_com_error'] < 1e-2, f"Mean is not zero, relative_error {st['max_rel_com_error']}"
        terms = terms.cpu().numpy().reshape(R, K + 1, ps.n, -1)
        shared = (gamma, log_pn, self.T, self.n_dims, self.norm_values, levels, nph, ps.sizes)
        if ps.grouped:
            members = members[0].cpu().numpy().reshape(R, K + 1, ps.n, ps.M, -1) if members[0] is not None else None
            out = scoring.assemble_groups(terms, members, kl.cpu().numpy(), ps.w, *shared)
        else:
            members, out = None, scoring.assemble(terms, kl.cpu().numpy(), *shared)
        reset = terms[..., scoring.SC_RESET].max(axis=2) > 0             # [R, K + 1]
        if st['nan_resets'] or reset.any():
            import warnings
            bad = sorted({int(levels[k]) for k in np.nonzero(reset.any(axis=0))[0]})
            warnings.warn(f'{entry}: the NaN guard reset the network output at {int(reset.sum())} level evaluation(s) (t = {bad}): '
                          'the reference resets the whole batch there, so nll is NaN for this batch', RuntimeWarning, stacklevel=3)
            out['nll'] = np.full_like(out['nll'], np.nan)
            out['nll_repeats'][reset.any(axis=1)] = np.nan
            if members is not None:
                out['member_nll'] = np.full_like(out['member_nll'], np.nan)
        keep = ['nll', 'loss_t', 'loss_0_x', 'loss_0_h', 'neg_log_const_0', 'kl_prior', 'delta_log_px', 'log_pN']
        keep += [k for k in out if k.endswith('_repeats')]
        if return_members:
            keep += ['member_nll', 'member_loss_t', 'member_loss_0_x', 'member_log_pN']
        if return_levels:
            out['level_sums'] = terms                                       # the raw sums (include/cmdgen_hip.h: CMDGEN_SC_COLS columns)
            keep += ['t_levels', 'level_terms', 'level_sums']
            if return_members:
                out['member_level_sums'] = members
                keep += ['member_level_sums']
        return {k: torch.from_numpy(np.ascontiguousarray(out[k])).to(ps.device) for k in keep}

    def _chain_frame(self, h, z_steps, step, xh_phar, xh_pocket):
        """The frame of the state after op `step`: unnormalize_z (:897-906) of z and of the pocket the op left; the
        pocket's features are fixed."""
        zs, ps = z_steps[step], h.last_pocket_steps[step]
        nd = self.n_dims
        return (torch.cat([zs[:, :nd] * self.norm_values[0], zs[:, nd:] * self.norm_values[1] + self.norm_biases[1]], dim=1),
                torch.cat([ps * self.norm_values[0], xh_pocket[:, nd:]], dim=1))


class SimpleConditionalDDPM(ConditionalDDPM):
    """The same model without the subspace trick (conditional_model.py:481-525): the context (pocket) is
    centred once and samples are not projected to the COM-free subspace; translation equivariance comes from
    evaluating everything in the pocket-centred frame."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.dynamics.attach_diffusion(self.T, self.gamma_table_host(), self.norm_values,
                                       self.norm_biases, no_com_projection=True)

    def subspace_dimensionality(self, input_size):
        return input_size * self.n_dims

    @classmethod
    def remove_mean_batch(cls, x_phar, x_pocket, phar_indices, pocket_indices):
        return x_phar, x_pocket

    @staticmethod
    def _pocket_com(pocket):
        n = len(pocket['size'])
        x, m = pocket['x'], pocket['mask']
        tot = torch.zeros((n, x.size(1)), dtype=x.dtype, device=x.device).index_add_(0, m, x)
        cnt = torch.zeros(n, dtype=x.dtype, device=x.device).index_add_(
            0, m, torch.ones(len(m), dtype=x.dtype, device=x.device)).clamp(min=1)
        return tot / cnt[:, None]

    @no_grad_unless_differentiable
    def forward(self, phar, pocket, return_info=False, t_int=None, eps=None, _net=None):
        phar, pocket = dict(phar), dict(pocket)
        com = self._pocket_com(pocket)
        phar['x'] = phar['x'] - com[phar['mask']]
        pocket['x'] = pocket['x'] - com[pocket['mask']]
        return super().forward(phar, pocket, return_info, t_int=t_int, eps=eps, _net=_net)

    # sample_given_pocket: the library centres the pocket itself when no_com_projection is set

    def inpaint(self, *args, **kwargs):
        raise NotImplementedError('inpainting is not implemented for SimpleConditionalDDPM (no centre-of-mass projection); '
                                  'use ConditionalDDPM')

    def edit(self, *args, **kwargs):
        raise NotImplementedError('edit is not implemented for SimpleConditionalDDPM (no centre-of-mass projection); '
                                  'use ConditionalDDPM')

    def score(self, *args, **kwargs):
        raise NotImplementedError('score is not implemented for SimpleConditionalDDPM (the scoring chain projects every level to the '
                                  'centre-of-mass-free subspace); use ConditionalDDPM')

    def sample_given_pockets(self, *args, **kwargs):
        raise NotImplementedError('sample_given_pockets is not implemented for SimpleConditionalDDPM (no centre-of-mass projection: the '
                                  'shared latent has no frame of its own); use ConditionalDDPM')

    def sample_restrained(self, *args, **kwargs):
        raise NotImplementedError('sample_restrained is not implemented for SimpleConditionalDDPM (no centre-of-mass projection: the '
                                  'guidance frame follows the projections); use ConditionalDDPM')

    def sample_diverse_restrained(self, *args, **kwargs):
        raise NotImplementedError('sample_diverse_restrained is not implemented for SimpleConditionalDDPM (no centre-of-mass projection: '
                                  'both terms compare positions in a frame that follows the projections)')

    def sample_diverse(self, *args, **kwargs):
        raise NotImplementedError('sample_diverse is not implemented for SimpleConditionalDDPM (no centre-of-mass projection: the '
                                  'frame in which the samples of a set are compared follows the projections); use ConditionalDDPM')

    def sample_restrained_given_pockets(self, *args, **kwargs):
        raise NotImplementedError('sample_restrained_given_pockets is not implemented for SimpleConditionalDDPM (no centre-of-mass '
                                  'projection: the shared latent has no frame of its own for the guidance to follow); use ConditionalDDPM')

    def edit_restrained(self, *args, **kwargs):
        raise NotImplementedError('edit_restrained is not implemented for SimpleConditionalDDPM (no centre-of-mass projection: the '
                                  'edit chain and the guidance frame follow the projections); use ConditionalDDPM')

    def edit_given_pockets(self, *args, **kwargs):
        raise NotImplementedError('edit_given_pockets is not implemented for SimpleConditionalDDPM (no centre-of-mass projection: the '
                                  'shared latent has no frame of its own); use ConditionalDDPM')

    def edit_restrained_given_pockets(self, *args, **kwargs):
        raise NotImplementedError('edit_restrained_given_pockets is not implemented for SimpleConditionalDDPM (no centre-of-mass '
                                  'projection: the shared latent has no frame of its own for the edit chain and the guidance to '
                                  'follow); use ConditionalDDPM')

    def score_given_pockets(self, *args, **kwargs):
        raise NotImplementedError('score_given_pockets is not implemented for SimpleConditionalDDPM (the scoring chain projects every '
                                  'level to the centre-of-mass-free subspace); use ConditionalDDPM')
