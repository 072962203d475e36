"""ConditionalDDPM.edit on the CPU: the oracle-built model of the edit chain (edit_ref) against the G22 vectors composed from
the reference's own methods (tests/golden/make_golden_edit.py), its reduction to the inpainting model, the draw plan, and the
argument checks and refusals that need no device."""
import numpy as np
import pytest
import torch

from helpers import load_golden, cases_of, cfg_from_meta, NoiseTape
from cond_inpaint_ref import cond_inpaint, inpaint_plan
from edit_ref import cond_edit, edit_plan
from helpers import bare_inputs as _inputs, bare_model as _model, g20, g20_oracle_case as g20_case, pocket_dict as pocket_of
from oracle import ref_cpu
from cmdgen_amd.synthetic import make_state_dict, make_pockets

G22 = load_golden('g22_edit.npz')


def g22_case(name):
    """-> cfg, oracle params, pocket batch, phar dict, (fix_x, fix_h), (K, start, resamplings, jump_length)."""
    H, L, B, R, seed, K, r, j, first, start = [int(v) for v in G22[name + '/meta']]
    cfg = cfg_from_meta(H, L, R)
    p = ref_cpu.to_torch_params(make_state_dict(cfg, seed=seed, coord_gain=1.0))
    pb = make_pockets(B, 'CA', ragged=True, n_phar=7, first_index=first)
    phar = {'x': torch.from_numpy(G22[name + '/phar_x']), 'one_hot': torch.from_numpy(G22[name + '/phar_one_hot']),
            'size': torch.from_numpy(pb.num_nodes_phar), 'mask': torch.from_numpy(np.repeat(np.arange(B), pb.num_nodes_phar))}
    return cfg, p, pb, phar, (G22[name + '/fix_x'], G22[name + '/fix_h']), (K, start, r, j)


def test_g22_covers_the_specified_cases():
    names = cases_of(G22)
    seen = set()
    for n in names:
        H, L, B, R, seed, K, r, j, first, start = [int(v) for v in G22[n + '/meta']]
        assert 3 <= B <= 4 and K <= 12 and 1 <= start <= K
        assert float(G22[n + '/margins'].min()) > 2e-3
        fx, fh = G22[n + '/fix_x'] != 0, G22[n + '/fix_h'] != 0
        pm = np.repeat(np.arange(B), make_pockets(B, 'CA', ragged=True, n_phar=7, first_index=first).num_nodes_phar)
        for b in range(B):
            x, h = fx[pm == b], fh[pm == b]
            if h.all() and not x.any():
                seen.add('types only')
            if x.all() and not h.any():
                seen.add('coordinates only')
            if (x & ~h).any() and (h & ~x).any() and (x & h).any() and (~x & ~h).any():
                seen.add('mixed')
            if not x.any() and not h.any():
                seen.add('unmarked')
        marks = bool(fx.any() or fh.any())
        if start < K:
            seen.add('part-way with marks' if marks else 'part-way without marks')
        if r > 1 and j > 1:
            seen.add('resampling with jumps')
        if H == 256:
            seen.add('hidden 256')
    assert seen == {'types only', 'coordinates only', 'mixed', 'unmarked', 'part-way with marks', 'part-way without marks',
                    'resampling with jumps', 'hidden 256'}


@pytest.mark.parametrize('name', cases_of(G22))
def test_oracle_model_reproduces_g22(name):
    """The bounds test_cond_inpaint_cpu.py applies to G20: 1e-5 of the scale, types exact."""
    cfg, p, pb, phar, (fx, fh), (K, start, r, j) = g22_case(name)
    tape = NoiseTape(G22[name + '/noise'])
    with torch.no_grad():
        xh_phar, xh_pocket, pm, _, z_steps, p_steps = cond_edit(p, cfg.as_dict(), phar, pocket_of(pb), fx, fh, start, r, j, K,
                                                                noise=tape, return_steps=True)
    assert tape.i == len(G22[name + '/noise']) == edit_plan(r, j, K, start)[1]
    assert len(z_steps) == edit_plan(r, j, K, start)[0]
    want = G22[name + '/xh_phar']
    scale = max(1.0, float(np.abs(want[:, :3]).max()))
    assert float(np.abs(xh_phar[:, :3].numpy() - want[:, :3]).max()) <= 1e-5 * scale
    assert np.array_equal(xh_phar[:, 3:].numpy(), want[:, 3:])
    wq = G22[name + '/xh_pocket']
    assert float(np.abs(xh_pocket.numpy() - wq).max()) <= 1e-5 * max(1.0, float(np.abs(wq).max()))
    zs, ps = G22[name + '/z_steps'], G22[name + '/pocket_steps']
    assert z_steps.shape == zs.shape and p_steps.shape == ps.shape
    assert float(np.abs(z_steps.numpy() - zs).max()) <= 1e-5 * max(1.0, float(np.abs(zs).max()))
    assert float(np.abs(p_steps.numpy() - ps).max()) <= 1e-5 * max(1.0, float(np.abs(ps).max()))


def test_held_parts_of_g22_come_out_as_given():
    """What the two masks are for: a row held in h keeps its type, a row held in x ends where it was given (pocket frame)."""
    for name in cases_of(G22):
        _, _, pb, phar, (fx, fh), _ = g22_case(name)
        fx, fh = fx != 0, fh != 0
        pm = phar['mask'].numpy()
        out, outq = G22[name + '/xh_phar'], G22[name + '/xh_pocket']
        B = len(pb.size)
        shift = np.stack([pb.x[pb.mask == b].mean(0) - outq[pb.mask == b, :3].mean(0) for b in range(B)])
        back = out[:, :3] + shift[pm]
        if fx.any():
            assert np.abs(back[fx] - phar['x'].numpy()[fx]).max() < 0.1
        assert np.array_equal(out[fh, 3:], phar['one_hot'].numpy()[fh])


@pytest.mark.parametrize('name', ['h64_K12_r1j1', 'h64_K8_r2j1', 'h64_K9_r3j2'])
def test_equal_masks_from_the_prior_equal_the_inpainting_model_bit_for_bit(name):
    cfg, p, pb, phar, fixed, (K, r, j) = g20_case(name)
    assert (r, j) in {(1, 1), (2, 1), (3, 2)}
    G20 = g20()
    noise = G20[name + '/noise']
    with torch.no_grad():
        a = cond_edit(p, cfg.as_dict(), phar, pocket_of(pb), fixed, fixed, K, r, j, K, noise=NoiseTape(noise), return_steps=True)
        b = cond_inpaint(p, cfg.as_dict(), phar, pocket_of(pb), fixed, r, j, K, noise=NoiseTape(noise), return_steps=True)
    assert len(a) == len(b) == 6
    for u, v in zip(a, b):
        assert torch.equal(u, v)


@pytest.mark.parametrize('K,start', [(1, 1), (2, 1), (7, 3), (50, 50), (50, 20), (500, 125)])
@pytest.mark.parametrize('r,j', [(1, 1), (2, 1), (3, 2), (10, 10), (4, 3), (2, 20)])
def test_plan_counts(K, start, r, j):
    n_steps, n_draws, n_jumps = edit_plan(r, j, K, start)
    sched = ref_cpu.get_repaint_schedule(r, j, start)
    assert n_steps == sum(sched) and n_jumps == len(sched) - 1
    assert n_draws == 2 + 2 * n_steps + n_jumps
    assert n_steps == start + n_jumps * j            # start steps down plus jump_length steps again for every jump back
    if start == K:
        assert (n_steps, n_draws, n_jumps) == inpaint_plan(r, j, K)


def test_plan_of_every_g22_case():
    for name in cases_of(G22):
        K, r, j, start = (int(G22[name + '/meta'][i]) for i in (5, 6, 7, 9))
        n_steps, n_draws, n_jumps = edit_plan(r, j, K, start)
        assert n_draws == 2 + 2 * n_steps + n_jumps == len(G22[name + '/noise'])
        assert n_steps == len(G22[name + '/z_steps']) == len(G22[name + '/pocket_steps'])


def test_argument_checks_without_a_device():
    from cmdgen_amd.equivariant_diffusion.conditional_model import ConditionalDDPM, SimpleConditionalDDPM
    from cmdgen_amd.equivariant_diffusion.en_diffusion import EnVariationalDiffusion
    phar, pocket = _inputs()
    m = _model(ConditionalDDPM)
    with pytest.raises(ValueError, match='fix_coords'):
        m.edit(phar, pocket, fix_coords=torch.ones(4), timesteps=10)
    with pytest.raises(ValueError, match='fix_types'):
        m.edit(phar, pocket, fix_types=torch.ones(5, 2), timesteps=10)
    with pytest.raises(ValueError, match='fix_types'):
        m.edit(phar, pocket, fix_coords=torch.ones(5, 1, dtype=torch.bool), fix_types=torch.ones(6), timesteps=10)
    for bad in (0, 11, -1, 2.5):
        with pytest.raises(ValueError, match='start'):
            m.edit(phar, pocket, fix_types=torch.ones(5), start=bad, timesteps=10)
    with pytest.raises(ValueError, match='start'):
        edit_plan(1, 1, 10, 11)
    with pytest.raises(NotImplementedError, match='SimpleConditionalDDPM'):
        _model(SimpleConditionalDDPM).edit(phar, pocket, fix_types=torch.ones(5), timesteps=10)
    with pytest.raises(NotImplementedError, match='joint'):
        EnVariationalDiffusion.edit(m, phar, pocket)


def test_edit_phars_builds_the_masks_and_keeps_the_row_order():
    """PharPocketDDPM.edit_phars up to the chain and back (the chain replaced by the identity): the given points are the first rows of
    every sample with the masks `keep` asks for, come back in their given order (also in a sample of more than 16 rows, where an
    unstable sort would permute them) in the pocket's frame, and the argument checks raise before the chain is called."""
    import os
    from helpers import GOLDEN
    from cmdgen_amd.lightning_modules import PharPocketDDPM
    from helpers import _hparams
    model = PharPocketDDPM(**_hparams('CA', 64, 2))
    names = list(model.dataset_info['phar_decoder'])
    pdb, ids = os.path.join(GOLDEN, 'g7_pocket.pdb'), [f'A:{i}' for i in range(1, 30)]
    phars = [(names[1], (9.0, 2.0, -15.0)), (names[3], (11.5, 4.0, -13.0)), (names[1], (7.0, 5.0, -12.0))]
    seen = {}

    def identity(phar, pocket, **kw):
        seen.update(kw, phar=phar)
        return (torch.cat([phar['x'], phar['one_hot']], 1), torch.cat([pocket['x'] + 3.0, pocket['one_hot'].float()], 1),
                phar['mask'], pocket['mask'])
    model.ddpm.edit = identity
    out = model.edit_phars(pdb, 3, phars, keep=['types', 'coords', 'both'], num_nodes_phar=torch.tensor([3, 20, 5]), pocket_ids=ids,
                           timesteps=50, seed=5)
    assert [len(s) for s in out] == [3, 20, 5] and seen['start'] is None
    first = [0, 3, 23]
    for b, sample in enumerate(out):
        assert [n for n, _ in sample[:3]] == [n for n, _ in phars]
        for (_, xyz), (_, got) in zip(phars, sample):                      # moved back by the pocket's shift (-3)
            assert np.allclose(np.asarray(got), np.asarray(xyz) - 3.0, atol=1e-5)
        assert seen['fix_coords'][first[b]:first[b] + 3].tolist() == [0.0, 1.0, 1.0]
        assert seen['fix_types'][first[b]:first[b] + 3].tolist() == [1.0, 0.0, 1.0]
    assert float(seen['fix_coords'].sum()) == 6.0 and float(seen['fix_types'].sum()) == 6.0
    model.edit_phars(pdb, 2, phars, keep='none', strength=0.4, pocket_ids=ids, timesteps=50, seed=5)
    assert seen['start'] == 20
    model.edit_phars(pdb, 2, phars, keep='none', strength=0.001, pocket_ids=ids, timesteps=50, seed=5)
    assert seen['start'] == 1
    model.ddpm.edit = None                                              # the checks below raise before the chain
    with pytest.raises(ValueError, match='strength'):
        model.edit_phars(pdb, 2, phars, strength=0.5, num_nodes_phar=5, pocket_ids=ids, timesteps=50)
    with pytest.raises(ValueError, match='strength'):
        model.edit_phars(pdb, 2, phars, strength=1.5, pocket_ids=ids, timesteps=50)
    with pytest.raises(ValueError, match='keep'):
        model.edit_phars(pdb, 2, phars, keep=['types', 'coords'], pocket_ids=ids, timesteps=50)
    with pytest.raises(ValueError, match='unknown pharmacophore type'):
        model.edit_phars(pdb, 2, [('Nope', (0.0, 0.0, 0.0))], pocket_ids=ids, timesteps=50)


def test_edit_entries_are_bound():
    from cmdgen_amd import hip_backend
    lib = hip_backend.load_library()
    assert lib.cmdgen_edit_chain.argtypes is not None and lib.cmdgen_edit_plan.argtypes is not None
    assert hasattr(hip_backend.Handle, 'edit_chain') and hasattr(hip_backend.Handle, 'edit_plan')
    names = [s[0] for s in hip_backend.SYMBOLS]
    assert 'cmdgen_edit_chain' in names and 'cmdgen_edit_plan' in names
