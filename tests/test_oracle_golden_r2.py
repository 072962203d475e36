"""CPU suite, round-2 goldens (tests/golden/make_golden_r2.py, captured from the real reference):
G5 per-block intermediates, G7 generate_phars bookkeeping, G12 the full-atom shape of BASELINE configs[4],
G13 chains in a regime where an ABSOLUTE 1e-4 RMS bound is meaningful.  They pin the oracle (and, for G7, the
host layer); tests/test_hip_parity_r2.py then checks the HIP path against the same vectors."""
import os

import numpy as np
import pytest
import torch

from helpers import (GOLDEN, G7_RUNS, _hparams, assert_same_result, g7_select, load_golden, cases_of, NoiseTape, rms, bounded_case, fullsize_chain_case, g5_case,
                     dynamics_case, pocket_dict)
from oracle import ref_cpu
from cmdgen_amd.synthetic import ModelConfig, make_state_dict, make_pockets


def test_g5_per_block_intermediates():
    """m_ij, e_ij, agg (egnn_new.py:31-58), trans and its segment sum (:87-104), (h, x) per block (:141-156)."""
    g = load_golden('g5_blocks.npz')
    cfg, sd, inp = g5_case(g)
    p = ref_cpu.to_torch_params(sd)
    trace = {}
    with torch.no_grad():
        eps_phar, eps_pocket = ref_cpu.dynamics_forward(
            p, cfg.as_dict(), torch.from_numpy(inp['xh_phar']), torch.from_numpy(inp['xh_pocket']), torch.from_numpy(inp['t']),
            torch.from_numpy(inp['mask_phar']), torch.from_numpy(inp['mask_pocket']), trace=trace)
    assert np.array_equal(np.stack([trace['row'].numpy(), trace['col'].numpy()]), g['edges'])
    nl = len(inp['mask_phar'])
    row = trace['row'].numpy()
    for b in range(cfg.n_layers):
        for ours, theirs in (('mij', 'm_ij'), ('edge_feat', 'e_ij'), ('agg', 'agg'), ('trans', 'trans'), ('h_block', 'h'),
                             ('x_block', 'x')):
            got, want = trace[ours][b].numpy(), g[f'block{b}/{theirs}']
            assert got.shape == want.shape
            assert np.abs(got - want).max() <= 2e-6 * max(1.0, np.abs(want).max()), (b, theirs)
        # the coordinate aggregate the reference adds (before the update mask): segment sum of trans / 100
        xs = np.zeros_like(g[f'block{b}/x_agg'])
        np.add.at(xs, row, trace['trans'][b].numpy() / cfg.normalization_factor)
        assert np.abs(xs - g[f'block{b}/x_agg']).max() <= 1e-6 * max(1.0, np.abs(g[f'block{b}/x_agg']).max())
        assert np.array_equal(trace['x_block'][b].numpy()[nl:], inp['xh_pocket'][:, :3])     # pocket rows never move
    assert np.abs(eps_phar.numpy() - g['eps_phar']).max() <= 2e-6 * max(1.0, np.abs(g['eps_phar']).max())


def test_g12_fullsize_dynamics_forward():
    """One EGNNDynamics.forward at Np=366 / Nl=15 per sample (dynamics.py:141-147 on 381-node samples)."""
    g = load_golden('g12_fullsize.npz')
    cfg, sd, inp = dynamics_case(g, 'dyn_fa366_b2')
    p = ref_cpu.to_torch_params(sd)
    trace = {}
    with torch.no_grad():
        eps_phar, _ = ref_cpu.dynamics_forward(
            p, cfg.as_dict(), torch.from_numpy(inp['xh_phar']), torch.from_numpy(inp['xh_pocket']), torch.from_numpy(inp['t']),
            torch.from_numpy(inp['mask_phar']), torch.from_numpy(inp['mask_pocket']), trace=trace)
    assert np.array_equal(np.stack([trace['row'].numpy(), trace['col'].numpy()]), g['dyn_fa366_b2/edges'])
    assert g['dyn_fa366_b2/edges'].shape[1] > 20000                 # ~13k edges per sample
    want = g['dyn_fa366_b2/eps_phar']
    assert np.abs(eps_phar.numpy() - want).max() <= 2e-6 * max(1.0, np.abs(want).max())


def _run_chain(cfg, sd, pb, K, noise, return_chain=False):
    p = ref_cpu.to_torch_params(sd)
    tape = NoiseTape(noise)
    with torch.no_grad():
        out = ref_cpu.sample_given_pocket(p, cfg.as_dict(), pocket_dict(pb), pb.num_nodes_phar, timesteps=K, noise=tape,
                                          return_chain=return_chain)
    assert tape.i == K + 2
    return out


def test_g12_fullsize_chain():
    g = load_golden('g12_fullsize.npz')
    name = 'chain_fa366_K5'
    cfg, sd, pb, K = fullsize_chain_case(g, name)
    xh_phar, xh_pocket, phar_mask, _, chain = _run_chain(cfg, sd, pb, K, g[name + '/noise'], return_chain=True)
    want = g[name + '/xh_phar']
    assert np.array_equal(phar_mask.numpy(), g[name + '/phar_mask'])
    assert rms(xh_phar[:, :3].numpy(), want[:, :3]) < 1e-4 * max(1.0, np.abs(want[:, :3]).max())
    assert np.array_equal(xh_phar[:, 3:].numpy(), want[:, 3:])
    for k in range(K):
        zs = g[name + '/z_steps'][k]
        assert np.abs(chain[k + 1].numpy() - zs).max() < 1e-4 * max(1.0, np.abs(zs).max())


@pytest.mark.parametrize('name', cases_of(load_golden('g13_bounded.npz')))
def test_g13_bounded_chain_absolute_tolerance(name):
    """north_star: 'sampled coords within 1e-4 RMS of reference' - ABSOLUTE, in a regime where that is above fp32
    resolution: |x| <= 17 A for the whole chain (ulp 2e-6).  K=50 strided and the full K=T=500 chain."""
    g = load_golden('g13_bounded.npz')
    cfg, sd, pb, K = bounded_case(g, name)
    assert float(g[name + '/max_abs_x']) < 30.0
    xh_phar, xh_pocket, phar_mask, _ = _run_chain(cfg, sd, pb, K, g[name + '/noise'])
    want = g[name + '/xh_phar']
    assert np.array_equal(phar_mask.numpy(), g[name + '/phar_mask'])
    assert rms(xh_phar[:, :3].numpy(), want[:, :3]) < 1e-4                           # absolute Angstrom
    assert np.array_equal(xh_phar[:, 3:].numpy(), want[:, 3:])                       # one-hot types exact
    assert rms(xh_pocket[:, :3].numpy(), g[name + '/xh_pocket'][:, :3]) < 1e-4


def test_g15_shipped_schedule_chain_per_step():
    """The oracle against the REAL reference's K = T = 500 chain under the SHIPPED schedule (noise_precision 1e-5, norm_values [1, 4]; G15,
    make_golden_r4.py): per-step z at every 50-step checkpoint and the final x within a few fp32 spacings of the values' magnitude
    (the coordinates inflate to hundreds of A), types exact - the [1, 4] scaling and the 1/alpha_ts growth pinned step by step."""
    from oracle import ref_cpu
    g = load_golden('g15_shipped_schedule_chain.npz')
    name = 'ca_b8_KT500_shipped'
    H, L, B, R, seed, K, T, first, nseed, window = [int(v) for v in g[name + '/meta']]
    cfg = ModelConfig(hidden_nf=H, n_layers=L, residue_nf=R, timesteps=T, noise_precision=float(g[name + '/noise_precision']),
                      norm_values=tuple(float(v) for v in g[name + '/norm_values']))
    sd = make_state_dict(cfg, seed=seed, coord_gain=float(g[name + '/coord_gain']))
    pb = make_pockets(B, 'CA', n_phar=15, first_index=first)
    gen = torch.Generator().manual_seed(nseed)
    draw = lambda shape: torch.randn(shape, generator=gen)
    pocket = {'x': torch.from_numpy(pb.x), 'one_hot': torch.from_numpy(pb.one_hot), 'size': torch.from_numpy(pb.size), 'mask': torch.from_numpy(pb.mask)}
    with torch.no_grad():
        xh_phar, _, _, _, chain = ref_cpu.sample_given_pocket(ref_cpu.to_torch_params(sd), cfg.as_dict(), pocket, pb.num_nodes_phar,
                                                               timesteps=K, noise=draw, return_chain=True)
    ulp = lambda v: float(2.0 ** (np.floor(np.log2(float(v))) - 23))
    for i, s in enumerate(g[name + '/ckpt_steps']):
        z, ref = chain[int(s)].numpy().astype(np.float64), g[name + '/ckpt_z'][i].astype(np.float64)
        for lo, hi in ((0, 3), (3, 11)):
            u = ulp(np.abs(ref[:, lo:hi]).max())
            assert np.sqrt(((z[:, lo:hi] - ref[:, lo:hi]) ** 2).mean()) <= 4.0 * u, (int(s), lo)
    want = g[name + '/xh_phar']
    assert np.array_equal(xh_phar[:, 3:].numpy(), want[:, 3:])
    assert rms(xh_phar[:, :3].numpy(), want[:, :3]) <= 4.0 * ulp(np.abs(want[:, :3]).max())


# ------------------------------------------------------------------------------------------------ G7


@pytest.mark.parametrize('tag,rep,sel', G7_RUNS)
def test_g7_generate_phars_bookkeeping_matches_reference(tag, rep, sel, monkeypatch):
    """PharPocketDDPM.generate_phars (lightning_modules.py:385-541) around the sampler: our PDB reader + pocket
    selection + tensor construction hand the sampler exactly what the reference (driven by a fake Bio structure
    holding the same atoms) handed its own; replaying the reference sampler's outputs through ours gives the
    reference's returned dict (COM restore, Q9 grouping)."""
    from cmdgen_amd.lightning_modules import PharPocketDDPM
    g = load_golden('g7_generate.npz')
    H, L = [int(v) for v in g[('ca' if rep == 'CA' else 'fa') + '/meta'][:2]]
    model = PharPocketDDPM(**_hparams(rep, H, L))
    seen = {}

    def replay(pocket, num_nodes_phar, timesteps=None, **kw):
        seen['pocket'] = {k: v.clone() for k, v in pocket.items()}
        seen['timesteps'] = timesteps
        nph = torch.as_tensor(num_nodes_phar)
        pm = torch.repeat_interleave(torch.arange(len(nph)), nph)
        return (torch.from_numpy(g[tag + '/sampler_xh_phar'].copy()), torch.from_numpy(g[tag + '/sampler_xh_pocket'].copy()),
                pm, pocket['mask'])
    monkeypatch.setattr(model.ddpm, 'sample_given_pocket', replay)
    nph = g[tag + '/num_nodes_phar']
    out = model.generate_phars(os.path.join(GOLDEN, 'g7_pocket.pdb'), len(nph), num_nodes_phar=torch.from_numpy(nph),
                               timesteps=int(g[tag + '/K']), **g7_select(g, tag, sel))
    p = seen['pocket']
    assert np.array_equal(p['x'].numpy(), g[tag + '/pocket_x'])                       # bit-equal fp32 coordinates
    assert np.array_equal(p['one_hot'].numpy().astype(np.int64), g[tag + '/pocket_one_hot'])
    assert np.array_equal(p['size'].numpy(), g[tag + '/pocket_size']) and p['size'].dtype == torch.int64
    assert np.array_equal(p['mask'].numpy(), g[tag + '/pocket_mask'])
    assert seen['timesteps'] == int(g[tag + '/K'])
    assert_same_result(out, str(g[tag + '/result_json']), atol=1e-6)


def test_g7_pocket_selection_quirks():
    from cmdgen_amd import utils
    g = load_golden('g7_generate.npz')
    m = utils.parse_pdb(os.path.join(GOLDEN, 'g7_pocket.pdb'))
    for tag, lig in (('ca_lig', 'B:501'), ('ca_pep', 'B:601')):
        got = [f'{r.get_resname()}{r.id[1]}' for r in utils.get_pocket_from_ligand(m, lig)]
        assert got == [str(s) for s in g[tag + '/selected']]
    assert 'ALA601' in [str(s) for s in g['ca_pep/selected']]         # Q11: a peptide ligand is part of its own pocket
    assert not any(s.startswith('LIG') or s.startswith('HOH') for s in map(str, g['ca_lig/selected']))


def test_g7_full_atom_unknown_element_raises_like_reference():
    from cmdgen_amd.lightning_modules import PharPocketDDPM
    g = load_golden('g7_generate.npz')
    assert str(g['fa_unknown/error']) == "KeyError:'Se'"
    model = PharPocketDDPM(**_hparams('full-atom', 64, 2))
    with pytest.raises(KeyError) as ei:
        model.generate_phars(os.path.join(GOLDEN, 'g7_pocket.pdb'), 1, pocket_ids=['A:28', 'A:29'],
                             num_nodes_phar=torch.tensor([3]), timesteps=2)
    assert ei.value.args[0] == 'Se'
