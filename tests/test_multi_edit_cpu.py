"""The multi-pocket edit chain on the CPU: the oracle-built model (multi_edit_ref) against its two parents where they must coincide
(edit_ref.cond_edit with groups of one, multi_pocket_ref.multi_pocket_chain with nothing held from the prior), the leave-out cap of
the GPU cases, held rows on the reference alone, the argument checks of ConditionalDDPM.edit_given_pockets and
PharPocketDDPM.edit_phars_multi that need no device, and the new entry's binding."""
import ctypes
import os
from dataclasses import replace

import numpy as np
import pytest
import torch

import multi_edit_cases as mec
import multi_edit_ref as me
import multi_pocket_cases as mc
import multi_pocket_ref as mp
from edit_ref import cond_edit, edit_plan
from helpers import NoiseTape, GOLDEN
from oracle import ref_cpu
from cmdgen_amd.synthetic import make_pockets, make_state_dict
from helpers import small, sub_pockets

K = 6


def _given(nph, seed, mark_every=2):
    rng = np.random.default_rng(seed)
    nl = int(np.sum(nph))
    pm = np.repeat(np.arange(len(nph)), nph)
    phar = {'x': torch.from_numpy((rng.normal(size=(nl, 3)) * 2.5).astype(np.float32)),
            'one_hot': torch.from_numpy(np.eye(8, dtype=np.float32)[rng.integers(0, 8, size=nl)]),
            'size': torch.from_numpy(np.asarray(nph, dtype=np.int64)), 'mask': torch.from_numpy(pm)}
    fx = (np.arange(nl) % mark_every == 0).astype(np.float32)
    fh = (np.arange(nl) % 3 == 0).astype(np.float32)
    return phar, fx, fh


@pytest.mark.parametrize('start,r,j', [(6, 1, 1), (6, 2, 2), (3, 1, 1), (3, 2, 1)])
def test_groups_of_one_are_the_edit_model_exactly(start, r, j):
    cfg, p = small()
    pb = make_pockets(4, 'CA', ragged=True, first_index=9400)
    nph = np.minimum(pb.num_nodes_phar, 8)
    phar, fx, fh = _given(nph, 1)
    fx[phar['mask'].numpy() == 2] = 0.0                         # one sample without a mark: it skips step B
    fh[phar['mask'].numpy() == 2] = 0.0
    n_draws = edit_plan(r, j, K, start)[1]
    noise = np.random.default_rng(2).normal(size=(n_draws, int(nph.sum()), 11)).astype(np.float32)
    pocket = sub_pockets(pb, range(4))
    with torch.no_grad():
        want = cond_edit(p, cfg.as_dict(), phar, pocket, fx, fh, start, r, j, K, noise=NoiseTape(noise), return_steps=True)
        got = me.multi_edit_chain(p, cfg.as_dict(), phar, pocket, [1, 1, 1, 1], np.ones(4, np.float32), fx, fh, start, r, j, K,
                                  noise=NoiseTape(noise), return_steps=True)
    assert torch.equal(got[4], want[4]) and torch.equal(got[5], want[5])          # z and the pocket after every op
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def test_no_marks_from_the_prior_are_the_multi_pocket_model_exactly():
    cfg, p = small()
    pb = make_pockets(5, 'CA', ragged=True, first_index=9430)
    sizes, nph = [2, 1, 2], np.array([5, 8, 3])
    w = np.array([0.3, 0.7, 1.0, 0.6, 0.4], np.float32)
    phar, _, _ = _given(nph, 3)
    zero = np.zeros(int(nph.sum()), np.float32)
    noise = np.random.default_rng(4).normal(size=(K + 2, int(nph.sum()), 11)).astype(np.float32)
    # the edit plan at (1, 1) draws A and B per op: the multi-pocket chain's K + 2 draws sit in rows 0, 1, 3, 5, .., and the last
    n_draws = edit_plan(1, 1, K, K)[1]
    spread = np.random.default_rng(5).normal(size=(n_draws, int(nph.sum()), 11)).astype(np.float32)
    spread[[0] + [1 + 2 * i for i in range(K)] + [n_draws - 1]] = noise
    pocket = sub_pockets(pb, range(5))
    with torch.no_grad():
        want = mp.multi_pocket_chain(p, cfg.as_dict(), pocket, sizes, nph, w, timesteps=K, noise=NoiseTape(noise), return_steps=True)
        got = me.multi_edit_chain(p, cfg.as_dict(), phar, pocket, sizes, w, zero, zero, K, 1, 1, K, noise=NoiseTape(spread),
                                  return_steps=True)
    assert len(got) == len(want) == 7
    for u, v in zip(got[:6], want[:6]):
        assert torch.equal(torch.as_tensor(u), torch.as_tensor(v))
    assert np.array_equal(got[6], want[6])


@pytest.mark.parametrize('run', mec.RUNS, ids=mec.run_id)
def test_the_committed_cases_stay_within_the_cap(run):
    """On the reference alone: at most CHAIN_CAP of a case's groups come within MARGIN of the cutoff at any reference evaluation (the
    first_index of multi_edit_cases.py is chosen here, on the CPU, so that this holds), and the cases are the ones the GPU tests name."""
    r = mec.reference(run)
    gr, case = r['groups'], mec.CASES[run.case]
    n_steps = edit_plan(run.r, run.j, mec.K, run.start)[0]
    n_out = int((~r['keep']).sum())
    print(f'\n[{mec.run_id(run)}] left out {n_out} of {gr.G} groups, smallest margin {r["margins"].min():.2e} A over {n_steps + 1} evaluations')
    assert r['margins'].shape == (n_steps + 1, gr.B)
    assert n_out <= mp.CHAIN_CAP * gr.G
    assert r['z_steps'].shape == (n_steps, gr.Nu, 11) and r['pocket_steps'].shape == (n_steps, len(r['pb'].x), 3)
    marks = mec.MARKS[run.case]
    if run.case == 'mixed':
        assert case.group_sizes == (1, 2, 3, 2, 1, 3) and min(case.nph) == 1 and max(case.nph) == 8
        assert any(set(m) == {'-'} for m in marks)                                  # a group without a mark: the skip-B path
        assert any(set(m) <= {'h', '-'} and 'h' in m for m in marks) and any(set(m) <= {'x', '-'} and 'x' in m for m in marks)
        assert any('b-' in m for m in marks)                                        # both marks on one row, none on the next
    else:
        assert max(r['pb'].num_nodes_phar + r['pb'].size) > 128
    # held types come back exactly in the reference's own result
    _, oh, _, fh = mec.given_rows(case)
    keep_rows = r['keep'][r['unique_mask']]
    held = (fh != 0) & keep_rows
    assert np.array_equal(r['want'][held, 3:], oh[held])


_HOLD = {}


def hold_reference():
    """The held-rows case on the CPU model: K = 100 on torch's generator, once."""
    if not _HOLD:
        hc = mec.hold_case()
        cfg = mec.hold_config()
        p = ref_cpu.to_torch_params(make_state_dict(cfg, seed=0))
        case = hc['case']
        nph = np.asarray(case.nph, dtype=np.int64)
        phar = {'x': torch.from_numpy(hc['phar_x']), 'one_hot': torch.from_numpy(hc['phar_oh']), 'size': torch.from_numpy(nph),
                'mask': torch.from_numpy(hc['unique_mask'])}
        torch.set_num_threads(min(16, max(1, torch.get_num_threads())))
        torch.manual_seed(hc['seed'])
        with torch.no_grad():
            out = me.multi_edit_chain(p, cfg.as_dict(), phar, mc.pocket_dict(hc['pb']), hc['sizes'], hc['weights'],
                                      hc['coords_only'].astype(np.float32), hc['types_only'].astype(np.float32), timesteps=mec.HOLD_K)
        _HOLD.update(hc=hc, xh_phar=out[0].numpy(), xh_pocket=out[1].numpy())
    return _HOLD


def test_held_rows_on_the_reference_alone():
    """test_hip_edit.py's test_types_hold_and_coordinates_hold for groups of two pockets with non-uniform weights, on the CPU model:
    held types come back exactly, held coordinates moved back by the FIRST pocket's shift sit within that test's 0.1 A - so the bound
    is the reference's property before the GPU test uses it."""
    h = hold_reference()
    hc = h['hc']
    assert set(hc['sizes']) == {2} and len(set(np.round(hc['weights'], 3))) > 2
    assert hc['types_only'].any() and hc['coords_only'].any()
    err = mec.held_errors(hc, h['xh_phar'], h['xh_pocket'])
    print(f'\n[held rows, reference] coords-only max err {err[hc["coords_only"]].max():.4f} A (bound {mec.HOLD_BOUND}); '
          f'types-only max err {err[hc["types_only"]].max():.3f} A')
    assert np.array_equal(h['xh_phar'][hc['types_only'], 3:], hc['phar_oh'][hc['types_only']])
    assert err[hc['coords_only']].max() < mec.HOLD_BOUND


def test_argument_checks_without_a_device():
    from helpers import bare_model as _model
    from cmdgen_amd.equivariant_diffusion.conditional_model import ConditionalDDPM, SimpleConditionalDDPM
    from cmdgen_amd.equivariant_diffusion.en_diffusion import EnVariationalDiffusion

    def pocket(sizes):
        n = int(sum(sizes))
        return {'x': torch.randn(n, 3), 'one_hot': torch.zeros(n, 20), 'size': torch.tensor(sizes),
                'mask': torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))}
    m = _model(ConditionalDDPM)
    m.dynamics.hip_handle = None                             # every check below raises before a handle is asked for
    a, b = pocket([3, 4]), pocket([5, 2])
    phar = {'x': torch.zeros(5, 3), 'one_hot': torch.zeros(5, 8), 'size': torch.tensor([2, 3]), 'mask': torch.tensor([0, 0, 1, 1, 1])}
    with pytest.raises(ValueError, match='pockets is empty'):
        m.edit_given_pockets(phar, [], timesteps=10)
    with pytest.raises(ValueError, match='at most 8'):
        m.edit_given_pockets(phar, [a] * 9, timesteps=10)
    with pytest.raises(ValueError, match='same groups'):
        m.edit_given_pockets(phar, [a, pocket([3, 4, 2])], timesteps=10)
    unsorted = dict(b, mask=torch.tensor([1, 1, 0, 0, 0, 0, 0]))
    with pytest.raises(ValueError, match='ascending'):
        m.edit_given_pockets(phar, [a, unsorted], timesteps=10)
    with pytest.raises(ValueError, match='ascending'):
        m.edit_given_pockets(dict(phar, mask=torch.tensor([1, 1, 1, 0, 0])), [a, b], timesteps=10)
    with pytest.raises(ValueError, match='phar has 3 samples, pocket 2'):
        m.edit_given_pockets(dict(phar, size=torch.tensor([2, 2, 1])), [a, b], timesteps=10)
    for bad in (0, 11, -1, 2.5):
        with pytest.raises(ValueError, match='start'):
            m.edit_given_pockets(phar, [a, b], fix_types=torch.ones(5), start=bad, timesteps=10)
    with pytest.raises(ValueError, match='weights has shape'):
        m.edit_given_pockets(phar, [a, b], weights=[1.0, 2.0, 3.0], timesteps=10)
    with pytest.raises(ValueError, match='>= 0'):
        m.edit_given_pockets(phar, [a, b], weights=[1.5, -0.5], timesteps=10)
    with pytest.raises(ValueError, match='sum to zero'):
        m.edit_given_pockets(phar, [a, b], weights=[[1.0, 1.0], [0.0, 0.0]], timesteps=10)
    with pytest.raises(ValueError, match='fix_coords'):
        m.edit_given_pockets(phar, [a, b], fix_coords=torch.ones(4), timesteps=10)
    with pytest.raises(ValueError, match='fix_types'):
        m.edit_given_pockets(phar, [a, b], fix_types=torch.ones(5, 2), timesteps=10)
    with pytest.raises(ValueError, match=r'sum\(size\) rows'):
        m.edit_given_pockets(dict(phar, x=torch.zeros(4, 3)), [a, b], timesteps=10)
    with pytest.raises(NotImplementedError, match='SimpleConditionalDDPM'):
        _model(SimpleConditionalDDPM).edit_given_pockets(phar, [a, b], timesteps=10)
    with pytest.raises(NotImplementedError, match='joint'):
        EnVariationalDiffusion.edit_given_pockets(m, phar, [a, b])


def test_edit_phars_multi_builds_the_masks_and_moves_back_by_the_first_pocket():
    """PharPocketDDPM.edit_phars_multi up to the chain and back (the chain replaced by the identity, every pocket moved by its own
    vector): the given points are the first rows with the masks `keep` asks for, the result comes back by the FIRST pocket's shift,
    strength sets the start level, and the argument checks raise before the chain is called."""
    from cmdgen_amd.lightning_modules import PharPocketDDPM
    from helpers import _hparams
    model = PharPocketDDPM(**_hparams('CA', 64, 2))
    names = list(model.dataset_info['phar_decoder'])
    pdb, ids = os.path.join(GOLDEN, 'g7_pocket.pdb'), [f'A:{i}' for i in range(1, 30)]
    phars = [(names[1], (9.0, 2.0, -15.0)), (names[3], (11.5, 4.0, -13.0)), (names[1], (7.0, 5.0, -12.0))]
    seen = {}

    def identity(phar, pockets, **kw):
        seen.update(kw, phar=phar, n_pockets=len(pockets))
        return (torch.cat([phar['x'], phar['one_hot']], 1),
                [torch.cat([q['x'] + 3.0 * (m + 1), q['one_hot'].float()], 1) for m, q in enumerate(pockets)],
                phar['mask'], [q['mask'] for q in pockets])
    model.ddpm.edit_given_pockets = identity
    out = model.edit_phars_multi([pdb, pdb], 3, phars, keep=['types', 'coords', 'both'], num_nodes_phar=torch.tensor([3, 20, 5]),
                                 pocket_ids=[ids, ids], weights=[0.5, 0.5], timesteps=50, seed=5)
    assert [len(s) for s in out] == [3, 20, 5] and seen['start'] is None and seen['n_pockets'] == 2 and seen['weights'] == [0.5, 0.5]
    first = [0, 3, 23]
    for b, sample in enumerate(out):
        assert [n for n, _ in sample[:3]] == [n for n, _ in phars]
        for (_, xyz), (_, got) in zip(phars, sample):                      # moved back by the first pocket's shift (-3), not the second's
            assert np.allclose(np.asarray(got), np.asarray(xyz) - 3.0, atol=1e-5)
        assert seen['fix_coords'][first[b]:first[b] + 3].tolist() == [0.0, 1.0, 1.0]
        assert seen['fix_types'][first[b]:first[b] + 3].tolist() == [1.0, 0.0, 1.0]
    out = model.edit_phars_multi([pdb, pdb], 2, phars, keep='none', strength=0.4, pocket_ids=[ids, ids], timesteps=50, seed=5)
    assert seen['start'] == 20 and [len(s) for s in out] == [3, 3]          # part-way: the given points only
    model.ddpm.edit_given_pockets = None                                    # the checks below raise before the chain
    with pytest.raises(ValueError, match='one per file'):
        model.edit_phars_multi([pdb, pdb], 2, phars, pocket_ids=[ids], timesteps=50)
    with pytest.raises(ValueError, match='strength'):
        model.edit_phars_multi([pdb, pdb], 2, phars, strength=0.5, num_nodes_phar=5, pocket_ids=[ids, ids], timesteps=50)
    with pytest.raises(ValueError, match='strength'):
        model.edit_phars_multi([pdb, pdb], 2, phars, strength=1.5, pocket_ids=[ids, ids], timesteps=50)
    with pytest.raises(ValueError, match='keep'):
        model.edit_phars_multi([pdb, pdb], 2, phars, keep=['types', 'coords'], pocket_ids=[ids, ids], timesteps=50)
    with pytest.raises(ValueError, match='unknown pharmacophore type'):
        model.edit_phars_multi([pdb, pdb], 2, [('Nope', (0.0, 0.0, 0.0))], pocket_ids=[ids, ids], timesteps=50)


def test_the_new_entry_is_bound():
    from cmdgen_amd import hip_backend
    lib = hip_backend.load_library()
    sig = dict((s[0], s) for s in hip_backend.SYMBOLS)['cmdgen_multi_edit_chain']
    multi, edit = (dict((s[0], s) for s in hip_backend.SYMBOLS)[n][2] for n in ('cmdgen_multi_pocket_chain', 'cmdgen_edit_chain'))
    assert sig[1] is ctypes.c_int and len(sig[2]) == 24
    # the multi-pocket chain's arguments with the edit chain's rows, masks, start, plan and draw count in their places
    assert sig[2][:6] == multi[:6] and sig[2][6:10] == edit[3:7] and sig[2][10:14] == edit[7:11] and sig[2][14:17] == edit[11:14]
    assert sig[2][17:] == multi[9:]
    assert lib.cmdgen_multi_edit_chain.argtypes == sig[2] and lib.cmdgen_multi_edit_chain.restype is ctypes.c_int
    assert hasattr(hip_backend.Handle, 'multi_edit_chain')
    with open(os.path.join(os.path.dirname(GOLDEN), '..', 'include', 'cmdgen_hip.h')) as f:
        assert 'int cmdgen_multi_edit_chain(cmdgen_handle* h' in f.read()
