"""PharPocketDDPM: the module callers import (counterpart of lightning_modules.py:30-568).

Same constructor arguments, checkpoint format (Lightning 1.8.5 ``.ckpt``: ``state_dict`` with
``ddpm.`` keys + ``hyper_parameters``), ``generate_phars`` and sampling entry points - without
a pytorch_lightning / BioPython / RDKit dependency.  Everything numerical on the sampling
path runs in libcmdgen_hip.so.  Training plumbing (Lightning hooks, W&B, dataloaders) is out
of scope.
"""
from __future__ import annotations

import argparse
import math
from argparse import Namespace
from typing import Optional

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from .constants import dataset_params, FLOAT_TYPE, INT_TYPE
from .equivariant_diffusion.dynamics import EGNNDynamics
from .equivariant_diffusion.en_diffusion import EnVariationalDiffusion
from .equivariant_diffusion.conditional_model import ConditionalDDPM, SimpleConditionalDDPM
from . import utils


def _scatter_mean(src, index, n):
    tot = torch.zeros((n,) + tuple(src.shape[1:]), dtype=src.dtype, device=src.device).index_add_(0, index, src)
    cnt = torch.zeros(n, dtype=src.dtype, device=src.device).index_add_(
        0, index, torch.ones(len(index), dtype=src.dtype, device=src.device)).clamp(min=1)
    return tot / cnt.view((-1,) + (1,) * (src.dim() - 1))


class PharPocketDDPM(nn.Module):
    def __init__(self, outdir, dataset, datadir, batch_size, lr, egnn_params: Namespace, diffusion_params,
                 num_workers, augment_noise, augment_rotation, clip_grad, eval_epochs, eval_params, mode,
                 node_histogram, pocket_representation='CA'):
        super().__init__()
        self.hparams = dict(outdir=outdir, dataset=dataset, datadir=datadir, batch_size=batch_size, lr=lr,
                            egnn_params=egnn_params, diffusion_params=diffusion_params, num_workers=num_workers,
                            augment_noise=augment_noise, augment_rotation=augment_rotation, clip_grad=clip_grad,
                            eval_epochs=eval_epochs, eval_params=eval_params, mode=mode,
                            node_histogram=node_histogram, pocket_representation=pocket_representation)
        ddpm_models = {'joint': EnVariationalDiffusion, 'pocket_conditioning': ConditionalDDPM,
                       'pocket_conditioning_simple': SimpleConditionalDDPM}
        assert mode in ddpm_models
        self.mode = mode
        assert pocket_representation in {'CA', 'full-atom'}
        self.pocket_representation = pocket_representation
        self.dataset_name, self.datadir, self.outdir = dataset, datadir, outdir
        self.batch_size = batch_size
        ep = vars(eval_params) if isinstance(eval_params, Namespace) else dict(eval_params or {})
        self.eval_batch_size = ep.get('eval_batch_size', batch_size)
        self.lr = lr
        self.loss_type = diffusion_params.diffusion_loss_type
        self.eval_epochs, self.eval_params = eval_epochs, eval_params
        self.num_workers, self.augment_noise, self.augment_rotation = num_workers, augment_noise, augment_rotation
        self.dataset_info = dataset_params[dataset]
        self.T = diffusion_params.diffusion_steps
        self.clip_grad = clip_grad
        if clip_grad:
            self.gradnorm_queue = utils.Queue()
            self.gradnorm_queue.add(3000)       # large value that will be flushed (lightning_modules.py:78-80)
        self.phar_type_encoder = self.dataset_info['phar_encoder']
        self.phar_type_decoder = self.dataset_info['phar_decoder']
        ca = self.pocket_representation == 'CA'
        self.pocket_type_encoder = self.dataset_info['aa_encoder' if ca else 'atom_encoder']
        self.pocket_type_decoder = self.dataset_info['aa_decoder' if ca else 'atom_decoder']
        self.phar_nf = len(self.phar_type_decoder)
        self.aa_nf = len(self.pocket_type_decoder)
        self.x_dims = 3
        net_dynamics = EGNNDynamics(
            phar_nf=self.phar_nf, residue_nf=self.aa_nf, n_dims=self.x_dims, joint_nf=egnn_params.joint_nf,
            device='cpu', hidden_nf=egnn_params.hidden_nf, act_fn=torch.nn.SiLU(), n_layers=egnn_params.n_layers,
            attention=egnn_params.attention, tanh=egnn_params.tanh, norm_constant=egnn_params.norm_constant,
            inv_sublayers=egnn_params.inv_sublayers, sin_embedding=egnn_params.sin_embedding,
            normalization_factor=egnn_params.normalization_factor,
            aggregation_method=egnn_params.aggregation_method,
            edge_cutoff=egnn_params.__dict__.get('edge_cutoff'), update_pocket_coords=(self.mode == 'joint'))
        self.ddpm = ddpm_models[self.mode](
            dynamics=net_dynamics, phar_nf=self.phar_nf, residue_nf=self.aa_nf, n_dims=self.x_dims,
            timesteps=diffusion_params.diffusion_steps,
            noise_schedule=diffusion_params.diffusion_noise_schedule,
            noise_precision=diffusion_params.diffusion_noise_precision,
            loss_type=diffusion_params.diffusion_loss_type,
            norm_values=diffusion_params.normalize_factors, size_histogram=node_histogram)

    # ------------------------------------------------------------------ Lightning-free plumbing
    @property
    def device(self):
        return next(self.parameters()).device

    @classmethod
    def load_from_checkpoint(cls, checkpoint_path, map_location=None, trust_checkpoint: bool = False, **overrides):
        """Read a Lightning-format checkpoint (generate_phars.py:32, test.py:73): a pickled dict with
        'state_dict' and 'hyper_parameters' (every constructor argument, incl. argparse.Namespace)."""
        if trust_checkpoint:
            ckpt = torch.load(checkpoint_path, map_location=map_location, weights_only=False)
        else:
            import numpy.core.multiarray as _ncm
            import pathlib
            # the reference passes outdir as a pathlib.Path (train.py:64-66), so real checkpoints carry one
            safe = [argparse.Namespace, np.ndarray, np.dtype, _ncm._reconstruct, _ncm.scalar,
                    pathlib.PosixPath, pathlib.PurePosixPath, pathlib.Path, pathlib.PurePath]
            try:
                safe += [type(np.dtype(np.float64)), type(np.dtype(np.int64)), type(np.dtype(np.float32))]
            except Exception:
                pass
            with torch.serialization.safe_globals(safe):
                ckpt = torch.load(checkpoint_path, map_location=map_location, weights_only=True)
        hp = dict(ckpt['hyper_parameters'])
        hp.update(overrides)
        for k in ('egnn_params', 'diffusion_params', 'eval_params'):
            if isinstance(hp.get(k), dict):
                hp[k] = Namespace(**hp[k])
        model = cls(**hp)
        model.load_state_dict(ckpt['state_dict'], strict=True)
        return model

    def save_checkpoint(self, path):
        torch.save({'state_dict': self.state_dict(), 'hyper_parameters': dict(self.hparams)}, path)

    def get_phar_and_pocket(self, data):
        phar = {'x': data['phar_coords'].to(self.device, FLOAT_TYPE),
                'one_hot': data['phar_one_hot'].to(self.device, FLOAT_TYPE),
                'size': data['num_phar_atoms'].to(self.device, INT_TYPE),
                'mask': data['phar_mask'].to(self.device, INT_TYPE)}
        pocket = {'x': data['pocket_c_alpha'].to(self.device, FLOAT_TYPE),
                  'one_hot': data['pocket_one_hot'].to(self.device, FLOAT_TYPE),
                  'size': data['num_pocket_nodes'].to(self.device, INT_TYPE),
                  'mask': data['pocket_mask'].to(self.device, INT_TYPE)}
        return phar, pocket

    def set_differentiable(self, on: bool = True):
        """Opt in to autograd (default off): with it on, `nll, _ = model(data); nll.mean().backward()` leaves the reference's
        gradients in the dynamics' .grad - the reference's training_step with any torch optimizer (cmdgen_amd.autograd)."""
        self.ddpm.set_differentiable(on)
        return self

    def forward(self, data, t_int=None, eps=None, _net=None):
        """-> (nll [B], info) as lightning_modules.py:188-239.  By default loss VALUES (evaluation / monitoring, no
        autograd graph): training.HipTrainer drives the optimizer with the HIP library's own backward pass
        (cmdgen_train_forward / cmdgen_train_backward) and the analytic gradient of this loss.  After
        set_differentiable(True), in grad mode, nll carries a graph and nll.mean().backward() fills the .grads."""
        phar, pocket = self.get_phar_and_pocket(data)
        delta_log_px, error_t_phar, error_t_pocket, SNR_weight, loss_0_x_phar, loss_0_x_pocket, loss_0_h, \
            neg_log_const_0, kl_prior, log_pN, t_int_, xh_phar_hat, info = \
            self.ddpm(phar, pocket, return_info=True, t_int=t_int, eps=eps, **({'_net': _net} if _net is not None else {}))
        dev = error_t_phar.device
        error_t_pocket, loss_0_x_pocket = error_t_pocket.to(dev), loss_0_x_pocket.to(dev)
        if self.loss_type == 'l2' and self.training:
            error_t_phar = error_t_phar / ((self.x_dims + self.ddpm.phar_nf) * phar['size'])
            error_t_pocket = error_t_pocket / ((self.x_dims + self.ddpm.residue_nf) * pocket['size'])
            loss_t = 0.5 * (error_t_phar + error_t_pocket)
            loss_0 = loss_0_x_phar / (self.x_dims * phar['size']) + loss_0_x_pocket / (self.x_dims * pocket['size']) \
                + loss_0_h
        else:
            loss_t = -self.T * 0.5 * SNR_weight * (error_t_phar + error_t_pocket)
            loss_0 = loss_0_x_phar + loss_0_x_pocket + loss_0_h + neg_log_const_0
        nll = loss_t + loss_0 + kl_prior
        if not (self.loss_type == 'l2' and self.training):
            nll = nll - delta_log_px - log_pN        # normalisation on x; conditional -> joint nll
        info['error_t_phar'] = error_t_phar.mean(0)
        info['error_t_pocket'] = error_t_pocket.mean(0)
        info['SNR_weight'] = SNR_weight.mean(0)
        info['loss_0'] = loss_0.mean(0)
        info['kl_prior'] = kl_prior.mean(0)
        info['delta_log_px'] = delta_log_px.mean(0)
        info['neg_log_const_0'] = neg_log_const_0.mean(0)
        info['log_pN'] = log_pN.mean(0)
        return nll, info

    def setup(self, stage=None):
        """Datasets from <datadir>/{train,val,test}.npz (lightning_modules.py:145-155)."""
        from pathlib import Path
        from .dataset import ProcessedLigandPharPocketDataset
        if stage == 'fit':
            self.train_dataset = ProcessedLigandPharPocketDataset(Path(self.datadir, 'train.npz'))
            self.val_dataset = ProcessedLigandPharPocketDataset(Path(self.datadir, 'val.npz'))
        elif stage == 'test':
            self.test_dataset = ProcessedLigandPharPocketDataset(Path(self.datadir, 'test.npz'))
        else:
            raise NotImplementedError

    @torch.no_grad()
    def sample_given_pocket_dataset(self, n_samples, dataset, batch_size=None, timesteps=None, **kw):
        """Sampling loop of sample_and_analyze_given_pocket (lightning_modules.py:337-373): cycles through the
        dataset in batches, draws the phar-node counts from the size prior and samples; returns per-sample
        (coords, types, reference phar coords).  The RDKit / KL analysis that follows in the reference
        (analysis/metrics.py) is out of scope."""
        batch_size = self.batch_size if batch_size is None else batch_size
        batch_size = min(batch_size, n_samples)
        phars = []
        for i in range(math.ceil(n_samples / batch_size)):
            n_b = min(batch_size, n_samples - len(phars))
            batch = dataset.collate_fn([dataset[(i * batch_size + j) % len(dataset)] for j in range(n_b)])
            phar, pocket = self.get_phar_and_pocket(batch)
            num_nodes_phar = self.ddpm.size_distribution.sample_conditional(n1=None, n2=pocket['size'])
            xh_phar, xh_pocket, phar_mask, _ = self.ddpm.sample_given_pocket(pocket, num_nodes_phar,
                                                                            timesteps=timesteps, **kw)
            x = xh_phar[:, :self.x_dims].detach().cpu()
            t = xh_phar[:, self.x_dims:].argmax(1).detach().cpu()
            pm = phar_mask.cpu()
            phars.extend(zip(utils.batch_to_list(x, pm), utils.batch_to_list(t, pm),
                             utils.batch_to_list(phar['x'].cpu(), phar['mask'].cpu())))
        return phars

    # ------------------------------------------------------------------ validation sampling
    @staticmethod
    def _type_kl(hist_dict, mapping, sample_types):
        """KL(p || q) of the dataset's type histogram p against the sampled types q with the reference's smoothing
        (analysis/metrics.py:12-34, CategoricalDistribution.kl_divergence; -1 when there is no histogram)."""
        if hist_dict is None:
            return -1
        p = np.zeros(len(mapping))
        for k, v in hist_dict.items():
            p[mapping[k]] = v
        p = p / p.sum()
        q = np.bincount(np.asarray(sample_types, dtype=np.int64), minlength=len(mapping)).astype(np.float64)
        q = q / q.sum()
        with np.errstate(divide='ignore', invalid='ignore'):
            return float(-np.sum(p * np.log(q / p + 1e-10)))

    @torch.no_grad()
    def sample_and_analyze_given_pocket(self, n_samples, dataset=None, batch_size=None, timesteps=None, **kw):
        """Sample n_samples pharmacophores for pockets of `dataset` and compare type statistics with the training
        data (lightning_modules.py:337-382 + analyze_sample :307-334): KL divergence of the sampled phar types and of
        the pocket types the sampler returns.  The commented-out stability / RDKit parts of the reference are not
        reproduced."""
        batch_size = self.batch_size if batch_size is None else batch_size
        batch_size = min(batch_size, n_samples)
        phar_types, aa_types, done = [], [], 0
        for i in range(math.ceil(n_samples / batch_size)):
            n_b = min(batch_size, n_samples - done)
            batch = dataset.collate_fn([dataset[(i * batch_size + j) % len(dataset)] for j in range(n_b)])
            phar, pocket = self.get_phar_and_pocket(batch)
            num_nodes_phar = self.ddpm.size_distribution.sample_conditional(n1=None, n2=pocket['size'])
            if type(self.ddpm) == EnVariationalDiffusion:
                xh_phar, xh_pocket, _, _ = self.ddpm.sample(n_b, num_nodes_phar, pocket['size'], timesteps=timesteps,
                                                            device=self.device, **kw)
            else:
                xh_phar, xh_pocket, _, _ = self.ddpm.sample_given_pocket(pocket, num_nodes_phar, timesteps=timesteps, **kw)
            phar_types.extend(xh_phar[:, self.x_dims:].argmax(1).detach().cpu().tolist())
            aa_types.extend(xh_pocket[:, self.x_dims:].argmax(1).detach().cpu().tolist())
            done += n_b
        ca = self.pocket_representation == 'CA'
        out = {'kl_div_atom_types': self._type_kl(self.dataset_info.get('phar_hist'), self.dataset_info['phar_encoder'], phar_types),
               'kl_div_residue_types': self._type_kl(self.dataset_info.get('aa_hist') if ca else None,
                                                     self.dataset_info['aa_encoder'] if ca else {}, aa_types)}
        print('kl_div_atom_types:', out['kl_div_atom_types'])
        print('kl_div_residue_types:', out['kl_div_residue_types'])
        return out

    # ------------------------------------------------------------------ sampling entry points
    @torch.no_grad()
    def sample_given_batch(self, batch, timesteps=None, **kw):
        """Sampling half of sample_and_analyze_given_pocket (lightning_modules.py:352-373): one collated
        batch dict -> (x list, type list per sample).  The RDKit-based analysis is out of scope."""
        phar, pocket = self.get_phar_and_pocket(batch)
        num_nodes_phar = self.ddpm.size_distribution.sample_conditional(n1=None, n2=pocket['size'])
        xh_phar, xh_pocket, phar_mask, _ = self.ddpm.sample_given_pocket(pocket, num_nodes_phar,
                                                                        timesteps=timesteps, **kw)
        x = xh_phar[:, :self.x_dims].detach().cpu()
        phar_type = xh_phar[:, self.x_dims:].argmax(1).detach().cpu()
        pm = phar_mask.cpu()
        return list(zip(utils.batch_to_list(x, pm), utils.batch_to_list(phar_type, pm)))

    def _pdb_pocket(self, pdb_file, n_samples, pocket_ids, ref_ligand):
        """The pocket of a PDB file (residues '<chain>:<resi>' or those around ref_ligand), repeated n_samples times as a
        batch dict (lightning_modules.py:400-441)."""
        pdb_struct = utils.parse_pdb(pdb_file)
        if pocket_ids is not None:
            residues = [pdb_struct[x.split(':')[0]][(' ', int(x.split(':')[1]), ' ')] for x in pocket_ids]
        else:
            residues = utils.get_pocket_from_ligand(pdb_struct, ref_ligand)
        if self.pocket_representation == 'CA':
            pocket_coord = torch.tensor(np.array([res['CA'].get_coord() for res in residues]),
                                        device=self.device, dtype=FLOAT_TYPE)
            pocket_types = torch.tensor([self.pocket_type_encoder[utils.three_to_one(res.get_resname())]
                                         for res in residues], device=self.device)
        else:
            atoms = [a for res in residues for a in res.get_atoms()
                     if (a.element.capitalize() in self.pocket_type_encoder or a.element != 'H')]
            pocket_coord = torch.tensor(np.array([a.get_coord() for a in atoms]), device=self.device, dtype=FLOAT_TYPE)
            pocket_types = torch.tensor([self.pocket_type_encoder[a.element.capitalize()] for a in atoms],
                                        device=self.device)     # KeyError for unknown non-H elements (Q12)
        pocket_one_hot = F.one_hot(pocket_types, num_classes=len(self.pocket_type_encoder))
        pocket_size = torch.tensor([len(pocket_coord)] * n_samples, device=self.device, dtype=INT_TYPE)
        pocket_mask = torch.repeat_interleave(torch.arange(n_samples, device=self.device, dtype=INT_TYPE),
                                              len(pocket_coord))
        pocket = {'x': pocket_coord.repeat(n_samples, 1), 'one_hot': pocket_one_hot.repeat(n_samples, 1),
                  'size': pocket_size, 'mask': pocket_mask}
        return pocket

    # ---- the parts the PDB-level entries below are composed of
    def _pocket_request(self, caller, pdb_files, pocket_ids, ref_ligands, many=False):
        """The pocket(s) an entry names, checked before any file is read: one PDB file with pocket_ids or ref_ligand, or (many) a list of
        files with one entry of either per file.  caller: the entry's name for the refusal of another model than the conditional one
        (None: the entry runs on any model, or refuses on its own).  -> load(n_samples): the pocket batch dicts, one per file."""
        assert (pocket_ids is None) ^ (ref_ligands is None)
        if many:
            pdb_files = list(pdb_files)
            if len(pocket_ids if pocket_ids is not None else ref_ligands) != len(pdb_files):
                raise ValueError(f'{len(pdb_files)} pdb_files need {len(pdb_files)} entries of pocket_ids or ref_ligands (one per file)')
        else:
            pdb_files, pocket_ids, ref_ligands = [pdb_files], [pocket_ids], [ref_ligands]
        if caller is not None and not isinstance(self.ddpm, ConditionalDDPM):
            raise NotImplementedError(f'{caller} needs the conditional model (mode pocket_conditioning)')
        return lambda n_samples: [self._pdb_pocket(f, n_samples, pocket_ids[m] if pocket_ids is not None else None,
                                                   ref_ligands[m] if ref_ligands is not None else None) for m, f in enumerate(pdb_files)]

    def _num_nodes(self, num_nodes_phar, pocket, n_samples, at_least=0):
        """Points per sample: by default the size prior given `pocket` (the first one of several), raised to at_least; a given scalar holds
        for every sample.  -> INT_TYPE [n_samples] on the device."""
        if num_nodes_phar is None:
            num_nodes_phar = self.ddpm.size_distribution.sample_conditional(n1=None, n2=pocket['size'])
            num_nodes_phar = torch.as_tensor(num_nodes_phar, device=self.device).clamp(min=at_least)
        else:
            num_nodes_phar = torch.as_tensor(num_nodes_phar, device=self.device).reshape(-1)
            if num_nodes_phar.numel() == 1:
                num_nodes_phar = num_nodes_phar.expand(n_samples)
        return num_nodes_phar.to(INT_TYPE)

    @staticmethod
    def _restraints_for_all(restraints):
        """Restraints given ONCE, without 'sample', and applied to every sample.  -> (the rows they name: a lower bound of num_nodes_phar,
        per_sample(num_nodes_phar, n_samples): the checked list for the sampler, every dict once per sample)."""
        from . import restraints as rs
        restraints = list(restraints)
        for n, r in enumerate(restraints):
            if isinstance(r, dict) and 'sample' in r:
                raise ValueError(f"restraints[{n}] = {r!r}: restraints are given once, without 'sample', and applied to every sample")
        named = [int(v) for r in restraints if isinstance(r, dict)
                 for v in ([r['point']] if 'point' in r else list(r.get('points', ()))) if isinstance(v, (int, np.integer))]

        def per_sample(num_nodes_phar, n_samples):
            nph = num_nodes_phar.cpu().numpy()
            for b in range(n_samples):
                rs.records(restraints, nph, sample=b)                       # (names the entry of the caller's list)
            return [dict(r, sample=b) for b in range(n_samples) for r in restraints]
        return max(named, default=0) + 1, per_sample

    def _moved_back(self, first, n_samples, sample, pocket_too=False):
        """sample() -> a ConditionalDDPM entry's tuple for `first`, the pocket as given (of several: the first one, every pocket was
        translated by the same vector).  Moves the points back to the original pocket position by that pocket's shift (pocket_too: and
        the pocket the sampler returned).  -> (xh_phar, phar_mask, what the entry returned behind its four: [] or [info])."""
        pocket_com_before = _scatter_mean(first['x'], first['mask'], n_samples)
        xh_phar, xh_pocket, phar_mask, pocket_mask, *info = sample()
        if isinstance(xh_pocket, list):
            xh_pocket, pocket_mask = xh_pocket[0], pocket_mask[0]
        pocket_com_after = _scatter_mean(xh_pocket[:, :self.x_dims], pocket_mask, n_samples)
        if pocket_too:
            xh_pocket[:, :self.x_dims] += (pocket_com_before - pocket_com_after)[pocket_mask]
        xh_phar[:, :self.x_dims] += (pocket_com_before - pocket_com_after)[phar_mask]
        return xh_phar, phar_mask, info

    def _molecule_dict(self, xh_phar, phar_mask):
        """generate_phars' output format.  Quirk Q9 kept: the counter restarts for every sample and advances per POINT, so 'Molecule_k'
        collects the k-th point of all samples, grouped by predicted type."""
        phar_mask = phar_mask.cpu()
        x = xh_phar[:, :self.x_dims].detach().cpu()
        phar_type = xh_phar[:, self.x_dims:].argmax(1).detach().cpu()
        phar_to_coords = {}
        for coords_batch, types in zip(utils.batch_to_list(x, phar_mask), utils.batch_to_list(phar_type, phar_mask)):
            names = [self.dataset_info['phar_decoder'][int(t)] for t in types]
            for k, (name, coords) in enumerate(zip(names, coords_batch), start=1):
                phar_to_coords.setdefault(f'Molecule_{k}', {}).setdefault(name, []).append(coords)
        return phar_to_coords

    def generate_phars(self, pdb_file, n_samples, pocket_ids=None, ref_ligand=None, num_nodes_phar=None,
                       sanitize=False, largest_frag=False, relax_iter=0, timesteps=None, **kwargs):
        """Generate pharmacophore point clouds inside a pocket (lightning_modules.py:385-541).

        pocket_ids: residues as '<chain>:<resi>'; ref_ligand: '<chain>:<resi>' alternative.
        sanitize / largest_frag / relax_iter and the inpainting kwargs are accepted and have no
        effect in conditional mode, as in the reference (quirk Q10); in mode 'joint' the kwargs
        (resamplings, jump_length) go to EnVariationalDiffusion.inpaint (lightning_modules.py:466-486)."""
        load = self._pocket_request(None, pdb_file, pocket_ids, ref_ligand)
        sampler_kw = {k: kwargs.pop(k) for k in ('noise', 'seed') if k in kwargs}
        pocket, = load(n_samples)
        if num_nodes_phar is None:
            num_nodes_phar = self._num_nodes(None, pocket, n_samples)
        if type(self.ddpm) == EnVariationalDiffusion:
            # inpainting: every pocket node is fixed, every phar node is generated (lightning_modules.py:466-486)
            num_nodes_phar = torch.as_tensor(num_nodes_phar, device=self.device)
            phar_mask = utils.num_nodes_to_batch_mask(len(num_nodes_phar), num_nodes_phar, self.device)
            phar = {'x': torch.zeros((len(phar_mask), self.x_dims), device=self.device, dtype=FLOAT_TYPE),
                    'one_hot': torch.zeros((len(phar_mask), self.phar_nf), device=self.device, dtype=FLOAT_TYPE),
                    'size': num_nodes_phar, 'mask': phar_mask}
            phar_mask_fixed = torch.zeros(len(phar_mask), device=self.device)
            pocket_mask_fixed = torch.ones(len(pocket['mask']), device=self.device)
            sample = lambda: self.ddpm.inpaint(phar, pocket, phar_mask_fixed, pocket_mask_fixed, timesteps=timesteps, **sampler_kw, **kwargs)
        elif isinstance(self.ddpm, ConditionalDDPM):
            sample = lambda: self.ddpm.sample_given_pocket(pocket, num_nodes_phar, timesteps=timesteps, **sampler_kw)
        else:
            raise NotImplementedError
        xh_phar, phar_mask, _ = self._moved_back(pocket, n_samples, sample, pocket_too=True)
        return self._molecule_dict(xh_phar, phar_mask)

    def generate_phars_multi(self, pdb_files, n_samples, pocket_ids=None, ref_ligands=None, num_nodes_phar=None, weights=None,
                             timesteps=None, **kwargs):
        """Generate pharmacophore point clouds for SEVERAL pockets at once - the two targets of a dual-target design, or
        conformations of one receptor (ConditionalDDPM.sample_given_pockets): every sample is one point cloud drawn from a chain
        that sees all the pockets.

        pdb_files: one PDB file per pocket.  The files must ALREADY be superposed into one common frame; nothing here aligns
        them (the reference's get_phar/point_dultarget*.py scripts superpose their two point clouds with a Kabsch step AFTER
        sampling each target alone - do that step on the structures first).  pocket_ids: per file a list of residues
        '<chain>:<resi>', or ref_ligands: per file a '<chain>:<resi>' ligand, as generate_phars takes one of them.
        num_nodes_phar: points per sample, default the size prior given the FIRST pocket.  weights: None (uniform) or one
        weight per file, >= 0 (normalised to sum 1).  seed / noise go to the sampler.  Everything is moved back by the first
        pocket's shift, so the points come out in the common frame.  -> the phar_to_coords dict of generate_phars."""
        load = self._pocket_request('generate_phars_multi', pdb_files, pocket_ids, ref_ligands, many=True)
        sampler_kw = {k: kwargs.pop(k) for k in ('noise', 'seed', 'group_ids') if k in kwargs}
        pockets = load(n_samples)
        if num_nodes_phar is None:
            num_nodes_phar = self._num_nodes(None, pockets[0], n_samples)
        xh_phar, phar_mask, _ = self._moved_back(pockets[0], n_samples, lambda: self.ddpm.sample_given_pockets(
            pockets, num_nodes_phar, weights=weights, timesteps=timesteps, **sampler_kw))
        return self._molecule_dict(xh_phar, phar_mask)

    @torch.no_grad()
    def generate_phars_restrained(self, pdb_file, n_samples, restraints, pocket_ids=None, ref_ligand=None, num_nodes_phar=None,
                                  clash=None, scale=1.0, max_shift=None, guide_below=1.0, timesteps=None, seed=None, noise=None):
        """Generate pharmacophores inside a pocket BIASED toward a geometric query (ConditionalDDPM.sample_restrained): "a feature
        within 1.5 A of this spot", "two features 5 to 7 A apart", "nothing inside this excluded volume", "no point on a pocket atom".

        restraints: the dicts of cmdgen_amd/restraints.py WITHOUT 'sample', given once in the PDB's frame and applied to every one of
        the n_samples copies; a point index names a row of every sample.  clash: None, a radius, or (radius, k).  num_nodes_phar:
        points per sample, default the size prior given the pocket, at least as many as the restraints name.  scale, max_shift,
        guide_below as sample_restrained; the pocket and the move back to its position as generate_phars.
        -> (one point list per sample, [(type name, (x, y, z))] in the PDB's frame - edit_phars' format, the ``candidates`` of
        score_phars - and {'energy': [n_samples], 'max_violation': [n_samples]} of the returned samples, to filter on)."""
        load = self._pocket_request('generate_phars_restrained', pdb_file, pocket_ids, ref_ligand)
        at_least, per_sample = self._restraints_for_all(restraints)
        pocket, = load(n_samples)
        num_nodes_phar = self._num_nodes(num_nodes_phar, pocket, n_samples, at_least)
        restraints = per_sample(num_nodes_phar, n_samples)
        xh_phar, _, info = self._moved_back(pocket, n_samples, lambda: self.ddpm.sample_restrained(
            pocket, num_nodes_phar, restraints, clash=clash, scale=scale, max_shift=max_shift, guide_below=guide_below, timesteps=timesteps,
            seed=seed, noise=noise))
        return self._point_lists(xh_phar, {'size': num_nodes_phar}), info[0]

    @torch.no_grad()
    def generate_phars_diverse(self, pdb_file, n_samples, pocket_ids=None, ref_ligand=None, num_nodes_phar=None, strength=1.0, width=2.0,
                               max_shift=None, guide_below=1.0, timesteps=None, seed=None, noise=None):
        """Generate n_samples DIFFERENT pharmacophores inside a pocket (ConditionalDDPM.sample_diverse): the n_samples copies of the
        pocket form one set, and at every denoising step each sample is pushed away from the others where their points overlap.

        strength (0: independent draws, generate_phars' chain), width (A), max_shift and guide_below as sample_diverse.  The pocket,
        num_nodes_phar (default the size prior given the pocket) and the move back to the pocket's position as generate_phars_restrained.
        -> (one point list per sample, [(type name, (x, y, z))] in the PDB's frame - edit_phars' format, the ``candidates`` of
        score_phars - and {'overlap': [n_samples]}, the mean overlap of every returned sample with the others, to rank on)."""
        load = self._pocket_request('generate_phars_diverse', pdb_file, pocket_ids, ref_ligand)
        pocket, = load(n_samples)
        num_nodes_phar = self._num_nodes(num_nodes_phar, pocket, n_samples)
        xh_phar, _, info = self._moved_back(pocket, n_samples, lambda: self.ddpm.sample_diverse(
            pocket, num_nodes_phar, [n_samples], strength=strength, width=width, max_shift=max_shift, guide_below=guide_below,
            timesteps=timesteps, seed=seed, noise=noise))
        return self._point_lists(xh_phar, {'size': num_nodes_phar}), info[0]

    @torch.no_grad()
    def generate_phars_diverse_restrained(self, pdb_file, n_samples, restraints, pocket_ids=None, ref_ligand=None, num_nodes_phar=None,
                                          clash=None, scale=1.0, strength=1.0, width=2.0, max_shift=None, guide_below=1.0,
                                          diverse_max_shift=None, diverse_guide_below=None, timesteps=None, seed=None, noise=None):
        """Generate n_samples DIFFERENT pharmacophores inside a pocket that ALL keep a geometric query
        (ConditionalDDPM.sample_diverse_restrained): generate_phars_restrained's restraints and generate_phars_diverse's push in one chain.

        restraints: the dicts of cmdgen_amd/restraints.py WITHOUT 'sample', given once in the PDB's frame and applied to every one of the
        n_samples copies, which form one set.  clash, scale, max_shift, guide_below as generate_phars_restrained; strength (0:
        generate_phars_restrained's chain) and width as generate_phars_diverse, with diverse_max_shift and diverse_guide_below of the
        overlap term's own (None: the restraint side's values).  The pocket, num_nodes_phar and the move back as generate_phars_restrained.
        -> (one point list per sample, [(type name, (x, y, z))] in the PDB's frame, and {'energy': [n_samples], 'max_violation':
        [n_samples], 'overlap': [n_samples]} of the returned samples, to filter and rank on)."""
        load = self._pocket_request('generate_phars_diverse_restrained', pdb_file, pocket_ids, ref_ligand)
        at_least, per_sample = self._restraints_for_all(restraints)
        pocket, = load(n_samples)
        num_nodes_phar = self._num_nodes(num_nodes_phar, pocket, n_samples, at_least)
        restraints = per_sample(num_nodes_phar, n_samples)
        xh_phar, _, info = self._moved_back(pocket, n_samples, lambda: self.ddpm.sample_diverse_restrained(
            pocket, num_nodes_phar, [n_samples], restraints, clash=clash, scale=scale, strength=strength, width=width, max_shift=max_shift,
            guide_below=guide_below, diverse_max_shift=diverse_max_shift, diverse_guide_below=diverse_guide_below, timesteps=timesteps,
            seed=seed, noise=noise))
        return self._point_lists(xh_phar, {'size': num_nodes_phar}), info[0]

    @torch.no_grad()
    def generate_phars_multi_restrained(self, pdb_files, n_samples, restraints, pocket_ids=None, ref_ligands=None, num_nodes_phar=None,
                                        weights=None, clash=None, scale=1.0, max_shift=None, guide_below=1.0, timesteps=None, seed=None,
                                        noise=None, group_ids=None):
        """generate_phars_multi BIASED toward a geometric query (ConditionalDDPM.sample_restrained_given_pockets): one pharmacophore per
        sample for SEVERAL pockets - "a donor at the shared hinge position, a hydrophobe 5-7 A from it, off the atoms of either pocket".

        pdb_files, pocket_ids / ref_ligands, num_nodes_phar and weights as generate_phars_multi: the files ALREADY superposed into one
        common frame.  restraints: the dicts of cmdgen_amd/restraints.py WITHOUT 'sample', given once in that common frame and applied to
        every one of the n_samples copies; clash (None, a radius, or (radius, k)) holds against the atoms of every pocket.  scale,
        max_shift, guide_below as sample_restrained.  Everything is moved back by the FIRST pocket's shift - the frame the guidance itself
        follows - so the points come out in the frame the centres were given in.
        -> (one point list per sample, [(type name, (x, y, z))], and {'energy': [n_samples], 'max_violation': [n_samples]})."""
        load = self._pocket_request('generate_phars_multi_restrained', pdb_files, pocket_ids, ref_ligands, many=True)
        at_least, per_sample = self._restraints_for_all(restraints)
        pockets = load(n_samples)
        num_nodes_phar = self._num_nodes(num_nodes_phar, pockets[0], n_samples, at_least)
        restraints = per_sample(num_nodes_phar, n_samples)
        sampler_kw = {} if group_ids is None else {'group_ids': group_ids}
        xh_phar, _, info = self._moved_back(pockets[0], n_samples, lambda: self.ddpm.sample_restrained_given_pockets(
            pockets, num_nodes_phar, restraints, weights=weights, clash=clash, scale=scale, max_shift=max_shift, guide_below=guide_below,
            timesteps=timesteps, seed=seed, noise=noise, **sampler_kw))
        return self._point_lists(xh_phar, {'size': num_nodes_phar}), info[0]

    def _phar_with_given_rows(self, points, arg, n_samples, num_nodes_phar, pocket, at_least=0):
        """The phar batch of inpaint_phars / edit_phars: `points` = [(type name, (x, y, z))] are the first rows of every sample, the
        other rows zero.  num_nodes_phar: points per sample, default the size prior given the pocket, at least len(points) (and at_least,
        the rows a caller's restraints name).  -> (phar dict, the indices of the given rows, sample by sample)."""
        n_fix = len(points)
        decoder = list(self.dataset_info['phar_decoder'])
        for name, _ in points:
            if name not in decoder:
                raise ValueError(f'unknown pharmacophore type {name!r}: expected one of {decoder}')
        num_nodes_phar = self._num_nodes(num_nodes_phar, pocket, n_samples, at_least=max(n_fix, at_least))
        if bool((num_nodes_phar < n_fix).any()):
            raise ValueError(f'num_nodes_phar must be at least len({arg}) = {n_fix}')
        phar_mask = utils.num_nodes_to_batch_mask(n_samples, num_nodes_phar, self.device)
        first = torch.cumsum(num_nodes_phar, 0) - num_nodes_phar                 # first row of every sample
        rows = (first[:, None] + torch.arange(n_fix, device=self.device)[None, :]).reshape(-1)
        fx = torch.tensor([list(map(float, xyz)) for _, xyz in points], device=self.device, dtype=FLOAT_TYPE).reshape(n_fix, 3)
        ft = torch.tensor([decoder.index(name) for name, _ in points], device=self.device, dtype=torch.int64)
        x = torch.zeros((len(phar_mask), self.x_dims), device=self.device, dtype=FLOAT_TYPE)
        one_hot = torch.zeros((len(phar_mask), self.phar_nf), device=self.device, dtype=FLOAT_TYPE)
        x[rows] = fx.repeat(n_samples, 1)
        one_hot[rows] = F.one_hot(ft, self.phar_nf).to(FLOAT_TYPE).repeat(n_samples, 1)
        return {'x': x, 'one_hot': one_hot, 'size': num_nodes_phar, 'mask': phar_mask}, rows

    def inpaint_phars(self, pdb_file, n_samples, fixed_phars, pocket_ids=None, ref_ligand=None, num_nodes_phar=None,
                      timesteps=None, resamplings=1, jump_length=1, seed=None):
        """Generate pharmacophores inside a pocket around given points (ConditionalDDPM.inpaint).

        fixed_phars: [(type name of dataset_info['phar_decoder'], (x, y, z) in Angstrom in the PDB's frame)]; they are the
        first rows of every sample.  num_nodes_phar: points per sample, default the size prior given the pocket, at least
        len(fixed_phars).  The pocket, the output format and the move back to the pocket's position are generate_phars'."""
        load = self._pocket_request('inpaint_phars', pdb_file, pocket_ids, ref_ligand)
        pocket, = load(n_samples)
        phar, rows = self._phar_with_given_rows(fixed_phars, 'fixed_phars', n_samples, num_nodes_phar, pocket)
        fixed = torch.zeros(len(phar['mask']), device=self.device, dtype=FLOAT_TYPE)
        fixed[rows] = 1.0
        xh_phar, phar_mask, _ = self._moved_back(pocket, n_samples, lambda: self.ddpm.inpaint(
            phar, pocket, fixed, resamplings=resamplings, jump_length=jump_length, timesteps=timesteps, seed=seed), pocket_too=True)
        return self._molecule_dict(xh_phar, phar_mask)

    KEEP = {'types': (False, True), 'coords': (True, False), 'both': (True, True), 'none': (False, False)}

    @torch.no_grad()
    def edit_phars(self, pdb_file, n_samples, phars, keep='types', strength=None, num_nodes_phar=None, pocket_ids=None,
                   ref_ligand=None, timesteps=None, resamplings=1, jump_length=1, seed=None):
        """Modify a given pharmacophore inside a pocket (ConditionalDDPM.edit): n_samples variants of it.

        phars: [(type name of dataset_info['phar_decoder'], (x, y, z) in Angstrom in the PDB's frame)], the first rows of every
        sample.  keep: what a given point holds - 'types' (the points are re-placed), 'coords' (they are re-typed), 'both' (as
        inpaint_phars) or 'none' - one word for all points or one per point.  strength in (0, 1]: how far the input is noised
        before the chain walks back, start = max(1, round(strength * timesteps)); None: from the prior.  num_nodes_phar adds
        free rows as in inpaint_phars (default: the size prior; with strength < 1 the given points only); with strength < 1 extra
        free rows are refused (there is nothing to noise for those rows).
        -> one point list per sample, [(type name, (x, y, z))] back in the PDB's frame: the ``candidates`` of score_phars."""
        load = self._pocket_request('edit_phars', pdb_file, pocket_ids, ref_ligand)
        keeps, start = self._edit_keeps_and_start(phars, keep, strength, timesteps)
        pocket, = load(n_samples)
        phar, fix_x, fix_h = self._edit_phar_and_masks(phars, keeps, start, strength, timesteps, n_samples, num_nodes_phar, pocket)
        xh_phar, _, _ = self._moved_back(pocket, n_samples, lambda: self.ddpm.edit(
            phar, pocket, fix_coords=fix_x, fix_types=fix_h, start=start, resamplings=resamplings, jump_length=jump_length,
            timesteps=timesteps, seed=seed))
        return self._point_lists(xh_phar, phar)

    @torch.no_grad()
    def edit_phars_restrained(self, pdb_file, n_samples, phars, restraints, keep='both', strength=None, clash=None, num_nodes_phar=None,
                              pocket_ids=None, ref_ligand=None, scale=1.0, max_shift=None, guide_below=1.0, timesteps=None,
                              resamplings=1, jump_length=1, seed=None):
        """edit_phars STEERED by a geometric query (ConditionalDDPM.edit_restrained): "keep these three points of the known
        pharmacophore and grow two more, 5 to 7 A from point 0, inside this sub-pocket, off the pocket atoms".

        phars, keep, strength, num_nodes_phar, resamplings, jump_length as edit_phars (keep defaults to 'both': the given points
        stay); restraints, clash, scale, max_shift, guide_below as generate_phars_restrained: the dicts of cmdgen_amd/restraints.py
        WITHOUT 'sample', given once in the PDB's frame, and every one of the n_samples copies gets the list.  A point index names a
        row of every sample: rows 0 .. len(phars) - 1 are the given points, the rows behind them the free ones.  A given point whose
        coordinates are kept enters the query at its given position and is not moved by it.
        -> (one point list per sample in the PDB's frame, {'energy': [n_samples], 'max_violation': [n_samples]} of the returned
        samples, to filter on)."""
        load = self._pocket_request('edit_phars_restrained', pdb_file, pocket_ids, ref_ligand)
        at_least, per_sample = self._restraints_for_all(restraints)
        keeps, start = self._edit_keeps_and_start(phars, keep, strength, timesteps)
        pocket, = load(n_samples)
        phar, fix_x, fix_h = self._edit_phar_and_masks(phars, keeps, start, strength, timesteps, n_samples, num_nodes_phar, pocket, at_least)
        restraints = per_sample(phar['size'], n_samples)
        xh_phar, _, info = self._moved_back(pocket, n_samples, lambda: self.ddpm.edit_restrained(
            phar, pocket, restraints, fix_coords=fix_x, fix_types=fix_h, start=start, resamplings=resamplings, jump_length=jump_length,
            clash=clash, scale=scale, max_shift=max_shift, guide_below=guide_below, timesteps=timesteps, seed=seed))
        return self._point_lists(xh_phar, phar), info[0]

    def _edit_keeps_and_start(self, phars, keep, strength, timesteps):
        """edit_phars' argument rules: -> (what every given point holds, the start level or None for the prior)."""
        n_given = len(phars)
        if n_given < 1:
            raise ValueError('phars needs at least one point')
        keeps = [keep] * n_given if isinstance(keep, str) else list(keep)
        if len(keeps) != n_given or any(k not in self.KEEP for k in keeps):
            raise ValueError(f'keep must be one of {sorted(self.KEEP)}, or one of these per point ({n_given}): got {keep!r}')
        T = self.ddpm.T if timesteps is None else int(timesteps)
        start = None
        if strength is not None:
            if not 0.0 < float(strength) <= 1.0:
                raise ValueError(f'strength={strength} must be in (0, 1]')
            start = max(1, int(round(float(strength) * T)))
        return keeps, start

    def _edit_phar_and_masks(self, phars, keeps, start, strength, timesteps, n_samples, num_nodes_phar, pocket, at_least=0):
        """-> (the phar batch with the given points as the first rows of every sample, fix_x, fix_h); pocket: the one the size prior
        is conditioned on; at_least: the rows the restraints name, which the size prior's draw is raised to."""
        n_given = len(phars)
        T = self.ddpm.T if timesteps is None else int(timesteps)
        if start is not None and start < T and num_nodes_phar is None:
            num_nodes_phar = n_given                                    # part-way: the given points only (no size prior)
        phar, rows = self._phar_with_given_rows(phars, 'phars', n_samples, num_nodes_phar, pocket, at_least)
        if start is not None and start < T and bool((phar['size'] > n_given).any()):
            raise ValueError(f'strength={strength} < 1 noises the given points; the extra free rows of num_nodes_phar have nothing to '
                             'noise: use strength=None (or 1), or num_nodes_phar = len(phars)')
        fix_x = torch.zeros(len(phar['mask']), device=self.device, dtype=FLOAT_TYPE)
        fix_h = torch.zeros_like(fix_x)
        fix_x[rows] = torch.tensor([float(self.KEEP[k][0]) for k in keeps], device=self.device).repeat(n_samples)
        fix_h[rows] = torch.tensor([float(self.KEEP[k][1]) for k in keeps], device=self.device).repeat(n_samples)
        return phar, fix_x, fix_h

    def _point_lists(self, xh_phar, phar):
        """One point list per sample, [(type name, (x, y, z))], rows in their given order (utils.batch_to_list goes through an
        unstable argsort, which may permute a sample's rows)."""
        decoder = list(self.dataset_info['phar_decoder'])
        x = xh_phar[:, :self.x_dims].detach().cpu()
        phar_type = xh_phar[:, self.x_dims:].argmax(1).detach().cpu()
        sizes = phar['size'].cpu().tolist()
        return [[(decoder[int(t)], tuple(float(v) for v in c)) for t, c in zip(types, coords)]
                for coords, types in zip(torch.split(x, sizes), torch.split(phar_type, sizes))]

    @torch.no_grad()
    def edit_phars_multi(self, pdb_files, n_samples, phars, keep='types', strength=None, num_nodes_phar=None, pocket_ids=None,
                         ref_ligands=None, weights=None, timesteps=None, resamplings=1, jump_length=1, seed=None):
        """edit_phars for SEVERAL pockets at once (ConditionalDDPM.edit_given_pockets): n_samples variants of a given pharmacophore,
        each drawn from a chain that sees all the pockets - a dual-target design around known anchor points, or a pharmacophore of
        one target adapted to a second (strength < 1).

        pdb_files, pocket_ids / ref_ligands and weights as generate_phars_multi takes them: one entry per pocket, the files ALREADY
        superposed into one common frame.  phars: [(type name, (x, y, z))] in that common frame; keep, strength and num_nodes_phar
        follow edit_phars' rules (the size prior is conditioned on the FIRST pocket; with strength < 1 the given points only).
        The result is moved back by the first pocket's shift.  -> edit_phars' point list per sample; keep='both' from the prior is
        the multi-pocket inpaint_phars."""
        load = self._pocket_request('edit_phars_multi', pdb_files, pocket_ids, ref_ligands, many=True)
        keeps, start = self._edit_keeps_and_start(phars, keep, strength, timesteps)
        pockets = load(n_samples)
        phar, fix_x, fix_h = self._edit_phar_and_masks(phars, keeps, start, strength, timesteps, n_samples, num_nodes_phar, pockets[0])
        xh_phar, _, _ = self._moved_back(pockets[0], n_samples, lambda: self.ddpm.edit_given_pockets(
            phar, pockets, fix_coords=fix_x, fix_types=fix_h, start=start, resamplings=resamplings, jump_length=jump_length,
            weights=weights, timesteps=timesteps, seed=seed))
        return self._point_lists(xh_phar, phar)

    @torch.no_grad()
    def edit_phars_multi_restrained(self, pdb_files, n_samples, phars, restraints, keep='both', strength=None, clash=None,
                                    num_nodes_phar=None, pocket_ids=None, ref_ligands=None, weights=None, scale=1.0, max_shift=None,
                                    guide_below=1.0, timesteps=None, resamplings=1, jump_length=1, seed=None):
        """edit_phars_multi STEERED by a geometric query (ConditionalDDPM.edit_restrained_given_pockets): "keep the three points known from
        kinase A and grow two more for kinases A and B together - a hydrophobe 5 to 7 A from the held donor, one point inside the
        sub-pocket only B has, none within 3 A of an atom of either pocket".

        pdb_files, pocket_ids / ref_ligands, weights, phars, keep, strength, num_nodes_phar, resamplings and jump_length as
        edit_phars_multi (keep defaults to 'both': the given points stay); restraints, clash, scale, max_shift and guide_below as
        generate_phars_multi_restrained: the dicts of cmdgen_amd/restraints.py WITHOUT 'sample', given once in the common frame, and every
        one of the n_samples copies gets the list; clash holds against the atoms of every pocket.  A point index names a row of every
        sample: rows 0 .. len(phars) - 1 are the given points, the rows behind them the free ones.  Everything is moved back by the FIRST
        pocket's shift - the frame the guidance itself follows.
        -> (one point list per sample in the common frame, {'energy': [n_samples], 'max_violation': [n_samples]} of the returned samples)."""
        load = self._pocket_request('edit_phars_multi_restrained', pdb_files, pocket_ids, ref_ligands, many=True)
        at_least, per_sample = self._restraints_for_all(restraints)
        keeps, start = self._edit_keeps_and_start(phars, keep, strength, timesteps)
        pockets = load(n_samples)
        phar, fix_x, fix_h = self._edit_phar_and_masks(phars, keeps, start, strength, timesteps, n_samples, num_nodes_phar, pockets[0], at_least)
        restraints = per_sample(phar['size'], n_samples)
        xh_phar, _, info = self._moved_back(pockets[0], n_samples, lambda: self.ddpm.edit_restrained_given_pockets(
            phar, pockets, restraints, fix_coords=fix_x, fix_types=fix_h, start=start, resamplings=resamplings, jump_length=jump_length,
            weights=weights, clash=clash, scale=scale, max_shift=max_shift, guide_below=guide_below, timesteps=timesteps, seed=seed))
        return self._point_lists(xh_phar, phar), info[0]

    # ------------------------------------------------------------------ scoring
    def _score_model(self):
        if not isinstance(self.ddpm, ConditionalDDPM):
            raise NotImplementedError('scoring needs the conditional model (mode pocket_conditioning): the joint model\'s loss has the '
                                      'pocket\'s own terms')
        return self.ddpm

    @torch.no_grad()
    def score(self, data, timesteps=None, repeats=1, noise=None, seed=None, pocket_ids=None, return_levels=False):
        """ConditionalDDPM.score of a collated batch, as ``forward(data)`` takes it: the per-sample NLL bound over a fixed grid of
        noise levels, evaluated on the device.  -> the dict of per-sample tensors ConditionalDDPM.score returns."""
        ddpm = self._score_model()
        phar, pocket = self.get_phar_and_pocket(data)
        return ddpm.score(phar, pocket, timesteps=timesteps, repeats=repeats, noise=noise, seed=seed, pocket_ids=pocket_ids,
                          return_levels=return_levels)

    def _candidate_batch(self, candidates):
        """The phar batch of score_phars / score_phars_multi: one sample per candidate point list, checked."""
        decoder = list(self.dataset_info['phar_decoder'])
        if len(candidates) < 1:
            raise ValueError('no candidates')
        for cand in candidates:
            if len(cand) < 1:
                raise ValueError('a candidate needs at least one point')
            for name, _ in cand:
                if name not in decoder:
                    raise ValueError(f'unknown pharmacophore type {name!r}: expected one of {decoder}')
        n = len(candidates)
        sizes = torch.tensor([len(c) for c in candidates], device=self.device, dtype=INT_TYPE)
        x = torch.tensor([list(map(float, xyz)) for c in candidates for _, xyz in c], device=self.device, dtype=FLOAT_TYPE).reshape(-1, 3)
        types = torch.tensor([decoder.index(name) for c in candidates for name, _ in c], device=self.device, dtype=torch.int64)
        return {'x': x, 'one_hot': F.one_hot(types, self.phar_nf).to(FLOAT_TYPE), 'size': sizes,
                'mask': utils.num_nodes_to_batch_mask(n, sizes, self.device)}

    @torch.no_grad()
    def score_phars(self, pdb_file, candidates, pocket_ids=None, ref_ligand=None, timesteps=None, repeats=1, seed=None):
        """Score candidate pharmacophores in the pocket of a PDB file (ConditionalDDPM.score): lower nll = the model finds the
        candidate more likely there.

        candidates: a list of point lists [(type name of dataset_info['phar_decoder'], (x, y, z) in Angstrom in the PDB's frame), ...];
        every candidate gets a copy of the pocket (pocket_ids / ref_ligand as in generate_phars) and is one sample of the batch.
        -> the dict of ConditionalDDPM.score, entry i of every tensor belonging to candidates[i].  Sample i draws with global pocket
        id i, so with the same seed a candidate's draws depend on its position in the list only.
        The return value of generate_phars cannot be scored: its 'Molecule_k' groups the k-th point of ALL samples (quirk Q9), not
        the points of one sample.  To rank generated samples go through ddpm.sample_given_pocket -> ddpm.score."""
        load = self._pocket_request(None, pdb_file, pocket_ids, ref_ligand)
        ddpm = self._score_model()
        phar = self._candidate_batch(candidates)
        pocket, = load(len(candidates))
        return ddpm.score(phar, pocket, timesteps=timesteps, repeats=repeats, seed=seed)

    @torch.no_grad()
    def score_phars_multi(self, pdb_files, candidates, pocket_ids=None, ref_ligands=None, weights=None, timesteps=None, repeats=1,
                          seed=None, return_members=False):
        """score_phars against SEVERAL pockets at once (ConditionalDDPM.score_given_pockets): how likely the model finds each
        candidate under all the pockets together - to rank what generate_phars_multi or edit_phars_multi drew, or to compare a
        known pharmacophore across a target and an anti-target (return_members gives every pocket's own score on the same draws).

        pdb_files, pocket_ids / ref_ligands and weights as generate_phars_multi takes them: one entry per pocket, the files ALREADY
        superposed into one common frame.  candidates as score_phars takes them, in that common frame; every candidate is one group
        and candidate i draws with global group id i.  -> the dict of ConditionalDDPM.score_given_pockets, entry i of every tensor
        belonging to candidates[i]."""
        load = self._pocket_request(None, pdb_files, pocket_ids, ref_ligands, many=True)
        ddpm = self._score_model()
        phar = self._candidate_batch(candidates)
        return ddpm.score_given_pockets(phar, load(len(candidates)), weights=weights, timesteps=timesteps, repeats=repeats, seed=seed,
                                        return_members=return_members)
