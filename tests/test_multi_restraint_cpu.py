"""The restrained multi-pocket chain on the CPU: the leave-out cap and the bite of the GPU cases on the reference alone, the oracle-built
model (multi_restraint_ref) against its two parents where they must coincide (multi_pocket_ref with nothing guided, restraint_ref with
groups of one), the effect on the model's own result, the argument checks of ConditionalDDPM.sample_restrained_given_pockets and
PharPocketDDPM.generate_phars_multi_restrained that need no device, and the new entry's binding."""
import ctypes
import os

import numpy as np
import pytest
import torch

import multi_pocket_cases as mc
import multi_restraint_cases as mrc
import multi_restraint_ref as mr
import restraint_cases as rc
from helpers import GOLDEN
from cmdgen_amd import restraints as rs


@pytest.mark.parametrize('case', [mrc.MIXED, mrc.LARGE, mrc.PAIRS], ids=lambda c: c.name)
def test_the_committed_cases_stay_within_the_cap_and_the_guidance_bites(case):
    """On the reference alone: at most CHAIN_CAP of a case's groups come within MARGIN of the cutoff at any reference evaluation, guided or
    unguided; the guidance clips at least one displacement and leaves one unclipped; a member other than the first contributes a clash term."""
    r = mrc.reference(case)
    gr, g = r['groups'], r['guided']
    n_out = int((~r['keep']).sum())
    print(f'\n[{case.name}] left out {n_out} of {gr.G} groups, smallest margin {min(g["margins"].min(), r["unguided"]["margins"].min()):.2e} A; '
          f'clipped {g["clipped"]}, unclipped {g["unclipped"]}; largest clash violation against a later member per op {g["other_member_clash"]}')
    assert g['margins'].shape == (mrc.K + 1, gr.B) and g['op_energy'].shape == (mrc.K, gr.G) and g['energy'].shape == (gr.G,)
    assert g['z_steps'].shape == (mrc.K, gr.Nu, 11) and g['pocket_steps'].shape == (mrc.K, len(r['pb'].x), 3)
    assert n_out <= mrc.CHAIN_CAP * gr.G
    assert g['clipped'] >= 1 and g['unclipped'] >= 1
    assert g['other_member_clash'].max() > 0
    kinds = {int(k) for k in r['rec']['kind']}
    if case.name == 'mixed':
        assert set(case.group_sizes) == {1, 2, 3} and min(case.nph) == 1 and kinds == {0, 1, 2}
        assert case.bare_group not in {int(s) for s in r['rec']['sample']}             # a group no record touches
        assert all(float(v) > 0 for v in g['kind_violation'].max(dim=0).values)        # every kind and the clash term act
    if case.name == 'large':
        assert max(r['pb'].num_nodes_phar + r['pb'].size) > 128
    if case.name == 'pairs':
        assert set(case.group_sizes) == {2}


@pytest.mark.parametrize('case', [mrc.MIXED, mrc.PAIRS], ids=lambda c: c.name)
def test_without_guidance_it_is_the_multi_pocket_model_exactly(case):
    """scale = 0 with the records and the clash term present, and no record with r_c = 0: multi_pocket_ref's outputs, steps and margins."""
    r, want = mrc.reference(case), mc.reference(getattr(mc, case.name.upper()))
    none = mrc.run_ref(case, r['pb'], r['weights'], rs.records([], case.nph), r['noise'], mrc.SCALE, clash=(0.0, 0.0))
    for got in (r['unguided'], none):
        assert np.array_equal(got['xh_phar'].numpy(), want['want']) and np.array_equal(got['xh_pocket'].numpy(), want['want_pocket'])
        assert np.array_equal(got['z_steps'].numpy(), want['z_steps']) and np.array_equal(got['pocket_steps'].numpy(), want['pocket_steps'])
        assert np.array_equal(got['margins'], want['margins'])
    assert float(r['unguided']['energy'].sum()) > 0 and not none['energy'].any() and not none['op_energy'].any()
    assert not np.array_equal(r['guided']['xh_phar'].numpy(), want['want'])              # ... and the guidance is not a no-op here


def test_groups_of_one_are_the_restrained_model_exactly():
    """Every M_g = 1 on restraint_cases' mixed batch: restraint_ref's outputs, steps, energies and op energies."""
    case = rc.MIXED
    r = rc.reference(case)
    B = len(case.nph)
    tape = iter(r['noise'])
    with torch.no_grad():
        got = mr.multi_restrained_chain(rc.params(), rc.config().as_dict(), rc.pocket_dict(r['pb']), [1] * B, case.nph, np.ones(B, np.float32),
                                        r['rec'], clash_r=rc.CLASH[0], clash_k=rc.CLASH[1], scale=rc.SCALE, max_shift=rc.MAX_SHIFT,
                                        timesteps=rc.K, noise=lambda shape: next(tape))
    want = r['guided']
    for k in ('xh_phar', 'xh_pocket', 'phar_mask', 'pocket_mask', 'z_steps', 'pocket_steps', 'op_energy', 'energy', 'max_violation',
              'kind_violation'):
        assert torch.equal(got[k], want[k]), k
    assert np.array_equal(got['margins'], want['margins'])
    assert (got['clipped'], got['unclipped']) == (want['clipped'], want['unclipped']) and want['clipped'] > 0
    assert not got['other_member_clash'].any()


@pytest.mark.parametrize('case', [mrc.MIXED, mrc.LARGE, mrc.PAIRS], ids=lambda c: c.name)
def test_guidance_lowers_the_final_energy(case):
    r = mrc.reference(case)
    g, u = r['guided']['energy'].numpy(), r['unguided']['energy'].numpy()
    print(f'\n[{case.name}] final energy per group unguided {u}\n         guided   {g}')
    assert float(g.sum()) < float(u.sum())


def _pocket(sizes):
    n = int(sum(sizes))
    return {'x': torch.randn(n, 3), 'one_hot': torch.zeros(n, 20), 'size': torch.tensor(sizes),
            'mask': torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))}


def test_argument_checks_without_a_device():
    from helpers import bare_model as _model
    from cmdgen_amd.equivariant_diffusion.conditional_model import ConditionalDDPM, SimpleConditionalDDPM
    from cmdgen_amd.equivariant_diffusion.en_diffusion import EnVariationalDiffusion
    m = _model(ConditionalDDPM)
    m.dynamics.hip_handle = None                             # every check below raises before a handle is asked for
    a, b = _pocket([3, 4]), _pocket([5, 2])
    pos = {'kind': 'position', 'sample': 0, 'point': 0, 'center': (0, 0, 0), 'radius': 1, 'k': 1}
    with pytest.raises(ValueError, match='pockets is empty'):
        m.sample_restrained_given_pockets([], [2, 3], [pos], timesteps=10)
    with pytest.raises(ValueError, match='at most 8'):
        m.sample_restrained_given_pockets([a] * 9, [2, 3], [pos], timesteps=10)
    with pytest.raises(ValueError, match='same groups'):
        m.sample_restrained_given_pockets([a, _pocket([3, 4, 2])], [2, 3], [pos], timesteps=10)
    with pytest.raises(ValueError, match='3 entries for 2 groups'):
        m.sample_restrained_given_pockets([a, b], [2, 3, 1], [pos], timesteps=10)
    with pytest.raises(ValueError, match='weights has shape'):
        m.sample_restrained_given_pockets([a, b], [2, 3], [pos], weights=[1.0, 2.0, 3.0], timesteps=10)
    with pytest.raises(ValueError, match=r'restraints\[0\].*sample 2'):                  # a group index >= G
        m.sample_restrained_given_pockets([a, b], [2, 3], [dict(pos, sample=2)], timesteps=10)
    with pytest.raises(ValueError, match=r'restraints\[1\].*point 2: sample 0 has 2 points'):   # a point >= n_phar of the GROUP
        m.sample_restrained_given_pockets([a, b], [2, 3], [pos, dict(pos, point=2)], timesteps=10)
    with pytest.raises(ValueError, match='i == j'):
        m.sample_restrained_given_pockets([a, b], [2, 3], [{'kind': 'distance', 'sample': 1, 'points': (1, 1), 'lo': 1, 'hi': 2, 'k': 1}],
                                          timesteps=10)
    with pytest.raises(ValueError, match='lo=3.0 > hi=2.0'):
        m.sample_restrained_given_pockets([a, b], [2, 3], [{'kind': 'distance', 'sample': 1, 'points': (0, 1), 'lo': 3, 'hi': 2, 'k': 1}],
                                          timesteps=10)
    with pytest.raises(ValueError, match='clash'):
        m.sample_restrained_given_pockets([a, b], [2, 3], [pos], clash=-1.0, timesteps=10)
    with pytest.raises(ValueError, match='max_shift'):
        m.sample_restrained_given_pockets([a, b], [2, 3], [pos], max_shift=0.0, timesteps=10)
    with pytest.raises(ValueError, match='scale'):
        m.sample_restrained_given_pockets([a, b], [2, 3], [pos], scale=-1.0, timesteps=10)
    with pytest.raises(ValueError, match='guide_below'):
        m.sample_restrained_given_pockets([a, b], [2, 3], [pos], guide_below=1.5, timesteps=10)
    with pytest.raises(NotImplementedError, match='SimpleConditionalDDPM'):
        _model(SimpleConditionalDDPM).sample_restrained_given_pockets([a, b], [2, 3], [pos], timesteps=10)
    with pytest.raises(NotImplementedError, match='joint model'):
        EnVariationalDiffusion.sample_restrained_given_pockets(m, [a, b], [2, 3], [pos])


def test_the_records_are_made_with_the_group_counts_and_both_tables_are_supplied():
    """sample_restrained_given_pockets up to the chain call, on a stand-in handle: restraints.records sees the per-GROUP counts (a point
    valid for the group but not for a member index passes), the layout is the member layout, and the step and the guide table are set."""
    from helpers import bare_model as _model
    from cmdgen_amd.equivariant_diffusion.conditional_model import ConditionalDDPM
    m = _model(ConditionalDDPM)
    seen = {}

    class Stop(Exception):
        pass

    class Handle:
        def set_layout(self, nph, sizes):
            seen['layout'] = (list(nph), list(sizes))

        def set_step_table(self, K, tab):
            seen['step'] = (K, np.asarray(tab).shape)

        def set_guide_table(self, K, tab):
            seen['guide'] = (K, np.asarray(tab).shape)

        def multi_restrained_chain(self, px, poh, sizes, w, K, rec, **kw):
            seen.update(kw, sizes=list(sizes), w=np.asarray(w), K=K, rec=rec, rows=len(px))
            raise Stop

        def run_range_guarded(self, run, status):
            return run(), None

        chain_status = None
    m.dynamics.hip_handle = lambda: Handle()
    m.refresh_learned_schedule = lambda: None
    a, b = _pocket([3, 4]), _pocket([5, 2])
    query = [{'kind': 'position', 'sample': 1, 'point': 4, 'center': (1, 2, 3), 'radius': 1.5, 'k': 1},
             {'kind': 'exclusion', 'sample': 0, 'center': (0, 0, 0), 'radius': 2, 'k': 0.5}]
    with pytest.raises(Stop):
        m.sample_restrained_given_pockets([a, b], [2, 5], query, weights=[3.0, 1.0], clash=(3.0, 2.0), scale=0.5, max_shift=0.7, guide_below=0.8,
                                          timesteps=10, seed=4, group_ids=[7, 9])
    assert seen['layout'] == ([2, 2, 5, 5], [3, 5, 4, 2]) and seen['sizes'] == [2, 2] and seen['rows'] == 14
    assert seen['step'] == (10, (11, 4)) and seen['guide'] == (10, (10, 2))
    assert np.allclose(seen['w'], [0.75, 0.25, 0.75, 0.25])
    assert seen['rec']['sample'].tolist() == [1, 0] and seen['rec']['i'].tolist() == [4, 0]
    assert (seen['clash_radius'], seen['clash_k'], seen['scale'], seen['max_shift'], seen['guide_below']) == (3.0, 2.0, 0.5, 0.7, 0.8)
    assert seen['seed'] == 4 and seen['group_ids'] == [7, 9] and seen['want_steps'] is False


def test_generate_phars_multi_restrained_moves_back_by_the_first_pocket():
    """PharPocketDDPM.generate_phars_multi_restrained up to the chain and back (the chain replaced by an identity that returns given points
    and moves every pocket by its own vector): every copy gets the list under its own group index, the centres stay where the caller put
    them, the result comes back by the FIRST pocket's shift, and the argument checks raise before the chain is called."""
    from cmdgen_amd.lightning_modules import PharPocketDDPM
    from helpers import _hparams
    model = PharPocketDDPM(**_hparams('CA', 64, 2))
    pdb, ids = os.path.join(GOLDEN, 'g7_pocket.pdb'), [f'A:{i}' for i in range(1, 30)]
    spot = (9.0, 2.0, -15.0)
    query = [{'kind': 'position', 'point': 0, 'center': spot, 'radius': 1.5, 'k': 1.0},
             {'kind': 'distance', 'points': (0, 1), 'lo': 5.0, 'hi': 7.0, 'k': 1.0}]
    seen = {}

    def identity(pockets, num_nodes_phar, restraints, **kw):
        seen.update(kw, restraints=restraints, n_pockets=len(pockets), nph=num_nodes_phar.tolist())
        n = int(num_nodes_phar.sum())
        pm = torch.repeat_interleave(torch.arange(len(num_nodes_phar)), num_nodes_phar)
        x = torch.tensor(spot).repeat(n, 1) + 3.0                                         # the chain's frame: the first pocket's, moved by +3
        return (torch.cat([x, torch.eye(model.phar_nf)[torch.zeros(n, dtype=torch.long)]], 1),
                [torch.cat([q['x'] + 3.0 * (m + 1), q['one_hot'].float()], 1) for m, q in enumerate(pockets)],
                pm, [q['mask'] for q in pockets], {'energy': torch.zeros(len(num_nodes_phar)), 'max_violation': torch.zeros(len(num_nodes_phar))})
    model.ddpm.sample_restrained_given_pockets = identity
    out, info = model.generate_phars_multi_restrained([pdb, pdb], 3, query, pocket_ids=[ids, ids], num_nodes_phar=torch.tensor([4, 7, 3]),
                                                      weights=[0.5, 0.5], clash=3.0, scale=0.5, timesteps=50, seed=5)
    assert [len(s) for s in out] == [4, 7, 3] and seen['n_pockets'] == 2 and seen['nph'] == [4, 7, 3] and seen['weights'] == [0.5, 0.5]
    assert (seen['clash'], seen['scale'], seen['seed'], seen['timesteps']) == (3.0, 0.5, 5, 50)
    assert [q['sample'] for q in seen['restraints']] == [0, 0, 1, 1, 2, 2]                 # every copy gets the list
    assert all(q['center'] == spot for q in seen['restraints'] if q['kind'] == 'position')  # ... its centres unmoved
    for sample in out:                                                                     # back by the first pocket's +3, not the second's +6
        for _, xyz in sample:
            assert np.allclose(np.asarray(xyz), np.asarray(spot), atol=1e-4)
    assert tuple(info['energy'].shape) == (3,)
    model.ddpm.sample_restrained_given_pockets = None                                      # the checks below raise before the chain
    with pytest.raises(ValueError, match='one per file'):
        model.generate_phars_multi_restrained([pdb, pdb], 2, query, pocket_ids=[ids], timesteps=50)
    with pytest.raises(ValueError, match=r"restraints\[0\].*without 'sample'"):
        model.generate_phars_multi_restrained([pdb, pdb], 2, [dict(query[0], sample=0)], pocket_ids=[ids, ids], timesteps=50)
    with pytest.raises(ValueError, match=r'restraints\[1\].*point 1'):
        model.generate_phars_multi_restrained([pdb, pdb], 2, query, pocket_ids=[ids, ids], num_nodes_phar=torch.tensor([4, 1]), timesteps=50)


def test_the_new_entry_is_bound():
    from cmdgen_amd import hip_backend
    lib = hip_backend.load_library()
    table = dict((s[0], s) for s in hip_backend.SYMBOLS)
    sig, multi, restrained = table['cmdgen_multi_restrained_chain'], table['cmdgen_multi_pocket_chain'][2], table['cmdgen_restrained_chain'][2]
    assert sig[1] is ctypes.c_int and len(sig[2]) == 25
    # the multi-pocket chain's leading arguments, the restrained chain's restraint arguments, the multi-pocket chain's tail, the two energies
    assert sig[2][:7] == multi[:7] and sig[2][7:14] == restrained[4:11] and sig[2][14:21] == multi[7:14]
    assert sig[2][21:23] == restrained[18:20] and sig[2][23:] == multi[14:] == restrained[20:]
    assert lib.cmdgen_multi_restrained_chain.argtypes == sig[2] and lib.cmdgen_multi_restrained_chain.restype is ctypes.c_int
    assert hasattr(hip_backend.Handle, 'multi_restrained_chain')
    with open(os.path.join(os.path.dirname(GOLDEN), '..', 'include', 'cmdgen_hip.h')) as f:
        assert 'int cmdgen_multi_restrained_chain(cmdgen_handle* h' in f.read()
