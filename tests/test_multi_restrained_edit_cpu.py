"""The restrained multi-pocket edit chain on the CPU: the leave-out cap and the bite of the GPU runs on the reference alone, the oracle-built
model (multi_restrained_edit_ref) against its three parents where they must coincide (multi_edit_ref with nothing guided,
restrained_edit_ref with groups of one, multi_restraint_ref without marks from the prior), the effect on the model's own result, the
argument checks of ConditionalDDPM.edit_restrained_given_pockets and PharPocketDDPM.edit_phars_multi_restrained that need no device, and
the new entry's binding."""
import ctypes
import os

import numpy as np
import pytest
import torch

import multi_edit_cases as mec
import multi_restrained_edit_cases as xc
import multi_restrained_edit_ref as mre
import multi_restraint_cases as mrc
import restrained_edit_cases as ec
from helpers import GOLDEN
from cmdgen_amd import restraints as rs


@pytest.mark.parametrize('run', xc.RUNS + (xc.ENGINE_RUN,), ids=xc.run_id)
def test_the_committed_runs_stay_within_the_cap_and_the_guidance_bites(run):
    """On the reference alone, for every run: at most CHAIN_CAP of the case's groups come within MARGIN of the cutoff at any reference
    evaluation, guided or unguided; the guidance leaves a displacement unclipped, a member other than the first contributes a clash term,
    and a guided op has a distance record that joins a held-x row to a free row.  A displacement is clipped in every run that starts from
    the prior: max_shift = 1 A binds where the posterior variance is large, at the high levels a run from start = 3 of 6 never visits."""
    r = xc.reference(run)
    case = xc.CASES[run.case]
    gr, g = r['groups'], r['guided']
    n_steps = xc.plan(run)[0]
    n_out = int((~r['keep']).sum())
    print(f'\n[{xc.run_id(run)}] left out {n_out} of {gr.G} groups, smallest margin '
          f'{min(g["margins"].min(), r["unguided"]["margins"].min()):.2e} A; clipped {g["clipped"]}, unclipped {g["unclipped"]}; largest clash '
          f'violation against a later member per op {g["other_member_clash"]}; guided ops with a held-free distance record '
          f'{g["held_record_ops"]} of {n_steps}')
    assert g['margins'].shape == (n_steps + 1, gr.B) and g['op_energy'].shape == (n_steps, gr.G) and g['energy'].shape == (gr.G,)
    assert g['z_steps'].shape == (n_steps, gr.Nu, 11) and g['pocket_steps'].shape == (n_steps, len(r['pb'].x), 3)
    assert r['noise'].shape == (xc.plan(run)[1], gr.Nu, 11)
    assert n_out <= xc.CHAIN_CAP * gr.G
    assert g['unclipped'] >= 1
    if run.start == xc.K:
        assert g['clipped'] >= 1
    assert g['other_member_clash'].max() > 0
    assert g['held_record_ops'] >= 1
    if run.case == 'mixed':
        assert set(case.group_sizes) == {1, 2, 3} and min(case.nph) == 1 and {int(k) for k in r['rec']['kind']} == {0, 1, 2}
        assert case.bare_group not in {int(s) for s in r['rec']['sample']}             # a group no record touches
        _, _, fx, _ = xc.given_rows(case)
        base = int(np.cumsum(case.nph)[xc.HELD_FREE_GROUP - 1])
        q = [q for q in r['rec'] if int(q['kind']) == 1 and int(q['sample']) == xc.HELD_FREE_GROUP]
        assert len(q) == 1 and (int(q[0]['i']), int(q[0]['j'])) == (0, 1) and fx[base] == 1 and fx[base + 1] == 0
        assert all(float(v) > 0 for v in g['kind_violation'].max(dim=0).values)        # every kind and the clash term act
    if run.case == 'large':
        assert max(r['pb'].num_nodes_phar + r['pb'].size) > 128                        # the 1024-thread path
    if run.case == 'pairs':
        assert set(case.group_sizes) == {2}


def test_the_clipped_and_unclipped_counts_cover_the_mixed_case():
    """Over MIXED's two runs together there is a clipped and an unclipped displacement (the run from the prior has both)."""
    runs = [r for r in xc.RUNS if r.case == 'mixed']
    assert sum(xc.reference(r)['guided']['clipped'] for r in runs) >= 1 and sum(xc.reference(r)['guided']['unclipped'] for r in runs) >= 1


@pytest.mark.parametrize('run', xc.RUNS, ids=xc.run_id)
def test_without_guidance_it_is_the_multi_edit_model_exactly(run):
    """scale = 0 with the records and the clash term present, and no record with r_c = 0: multi_edit_ref's outputs, steps and margins."""
    r, want = xc.reference(run), mec.reference(run)
    case = xc.CASES[run.case]
    none = xc.run_ref(run, r['pb'], r['weights'], rs.records([], case.nph), r['noise'], xc.SCALE, clash=(0.0, 0.0))
    for got in (r['unguided'], none):
        assert np.array_equal(got['xh_phar'].numpy(), want['want']) and np.array_equal(got['xh_pocket'].numpy(), want['want_pocket'])
        assert np.array_equal(got['z_steps'].numpy(), want['z_steps']) and np.array_equal(got['pocket_steps'].numpy(), want['pocket_steps'])
        assert np.array_equal(got['margins'], want['margins'])
    assert float(r['unguided']['energy'].sum()) > 0 and not none['energy'].any() and not none['op_energy'].any()
    assert not np.array_equal(r['guided']['xh_phar'].numpy(), want['want'])              # ... and the guidance is not a no-op here


@pytest.mark.parametrize('case', [ec.MIXED, ec.JUMPS], ids=lambda c: c.name)
def test_groups_of_one_are_the_restrained_edit_model_exactly(case):
    """Every M_g = 1 on restrained_edit_cases' batches (from the prior, and part-way with jumps): restrained_edit_ref's outputs, steps,
    energies and op energies."""
    r = ec.reference(case)
    B = len(case.nph)
    tape = iter(r['noise'])
    with torch.no_grad():
        got = mre.multi_restrained_edit(ec.params(), ec.config().as_dict(), r['phar'], ec.pocket_dict(r['pb']), [1] * B, np.ones(B, np.float32),
                                        r['fx'], r['fh'], r['rec'], clash_r=ec.CLASH[0], clash_k=ec.CLASH[1], scale=ec.SCALE,
                                        max_shift=ec.MAX_SHIFT, start=case.start, resamplings=case.r, jump_length=case.j, timesteps=case.K,
                                        noise=lambda shape: next(tape))
    assert next(tape, None) is None
    want = r['guided']
    for k in ('xh_phar', 'xh_pocket', 'phar_mask', 'pocket_mask', 'z_steps', 'pocket_steps', 'op_energy', 'energy', 'max_violation',
              'kind_violation'):
        assert torch.equal(got[k], want[k]), k
    assert np.array_equal(got['margins'], want['margins'])
    assert float(want['op_energy'].abs().max()) > 0 and not got['other_member_clash'].any()
    assert not torch.equal(got['xh_phar'], r['unguided']['xh_phar'])


@pytest.mark.parametrize('case', [mrc.PAIRS, mrc.MIXED], ids=lambda c: c.name)
def test_without_marks_from_the_prior_it_is_the_multi_restraint_model_exactly(case):
    """No mark in either mask, start = timesteps, r = j = 1: the draws are z_T, (A, B) per op and the decode; the restrained multi-pocket
    model reads z_T, the A rows and the decode, the B rows are read and not used."""
    r = mrc.reference(case)
    Kc, nu = mrc.K, int(sum(case.nph))
    n_draws = 2 + 2 * Kc
    gen = torch.Generator().manual_seed(5)
    noise = torch.randn((n_draws, nu, 11), generator=gen)
    noise[[0] + [1 + 2 * i for i in range(Kc)] + [n_draws - 1]] = r['noise']
    phar = {'x': torch.randn((nu, 3), generator=gen) * 2.5, 'one_hot': torch.eye(8)[torch.randint(0, 8, (nu,), generator=gen)],
            'size': torch.tensor(case.nph)}
    zero = np.zeros(nu, np.float32)
    tape = iter(noise)
    with torch.no_grad():
        got = mre.multi_restrained_edit(mrc.params(), mrc.config().as_dict(), phar, mrc.pocket_dict(r['pb']), case.group_sizes, r['weights'],
                                        zero, zero, r['rec'], clash_r=mrc.CLASH[0], clash_k=mrc.CLASH[1], scale=mrc.SCALE,
                                        max_shift=mrc.MAX_SHIFT, timesteps=Kc, noise=lambda shape: next(tape))
    assert next(tape, None) is None
    want = r['guided']
    for k in ('xh_phar', 'xh_pocket', 'phar_mask', 'pocket_mask', 'z_steps', 'pocket_steps', 'op_energy', 'energy', 'max_violation',
              'kind_violation'):
        assert torch.equal(got[k], want[k]), k
    assert np.array_equal(got['margins'], want['margins']) and np.array_equal(got['other_member_clash'], want['other_member_clash'])
    assert (got['clipped'], got['unclipped']) == (want['clipped'], want['unclipped']) and got['held_record_ops'] == 0


@pytest.mark.parametrize('run', [r for r in xc.RUNS if r.case == 'mixed'], ids=xc.run_id)
def test_guidance_lowers_the_final_energy_of_the_touched_groups(run):
    """With the clash term on every group of MIXED is touched: their guided energies sum below the unguided ones on the same draws (a group
    whose every x is held gets no displacement, so the sum, not every group, is what the guidance lowers)."""
    r = xc.reference(run)
    case = xc.CASES[run.case]
    touched = mre.touched_samples(r['rec'], len(case.nph), xc.CLASH[0])
    g, u = r['guided']['energy'].numpy(), r['unguided']['energy'].numpy()
    print(f'\n[{xc.run_id(run)}] final energy per group unguided {u}\n         guided   {g}')
    assert touched.all() and float(g[touched].sum()) < float(u[touched].sum())
    _, _, fx, _ = xc.given_rows(case)
    all_held = [k for k, f in enumerate(np.split(fx, np.cumsum(case.nph)[:-1])) if f.all()]
    assert all_held == [1] and g[1] == u[1]                                             # the single held point: nothing to steer


# ------------------------------------------------------------------------------------------------ the Python surface (no device)
def _pocket(sizes):
    n = int(sum(sizes))
    return {'x': torch.randn(n, 3), 'one_hot': torch.zeros(n, 20), 'size': torch.tensor(sizes),
            'mask': torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))}


def _phar(nph):
    n = int(sum(nph))
    return {'x': torch.randn(n, 3), 'one_hot': torch.eye(8)[torch.zeros(n, dtype=torch.long)], 'size': torch.tensor(nph),
            'mask': torch.repeat_interleave(torch.arange(len(nph)), torch.tensor(nph))}


def test_argument_checks_without_a_device_and_the_restraint_checks_name_the_group():
    from helpers import bare_model as _model
    from cmdgen_amd.equivariant_diffusion.conditional_model import ConditionalDDPM
    m = _model(ConditionalDDPM)
    m.dynamics.hip_handle = None                             # every check below raises before a handle is asked for
    a, b, phar = _pocket([3, 4]), _pocket([5, 2]), _phar([2, 3])
    pos = {'kind': 'position', 'sample': 0, 'point': 0, 'center': (0, 0, 0), 'radius': 1, 'k': 1}
    with pytest.raises(ValueError, match='pockets is empty'):
        m.edit_restrained_given_pockets(phar, [], [pos], timesteps=10)
    with pytest.raises(ValueError, match='at most 8'):
        m.edit_restrained_given_pockets(phar, [a] * 9, [pos], timesteps=10)
    with pytest.raises(ValueError, match='same groups'):
        m.edit_restrained_given_pockets(phar, [a, _pocket([3, 4, 2])], [pos], timesteps=10)
    with pytest.raises(ValueError, match='phar has 3 samples, pocket 2'):
        m.edit_restrained_given_pockets(_phar([2, 3, 1]), [a, b], [pos], timesteps=10)
    with pytest.raises(ValueError, match='weights has shape'):
        m.edit_restrained_given_pockets(phar, [a, b], [pos], weights=[1.0, 2.0, 3.0], timesteps=10)
    with pytest.raises(ValueError, match='fix_coords'):
        m.edit_restrained_given_pockets(phar, [a, b], [pos], fix_coords=torch.ones(4), timesteps=10)
    with pytest.raises(ValueError, match='fix_types'):
        m.edit_restrained_given_pockets(phar, [a, b], [pos], fix_types=torch.ones(5, 2), timesteps=10)
    for bad in (0, 11, 2.5):
        with pytest.raises(ValueError, match='start'):
            m.edit_restrained_given_pockets(phar, [a, b], [pos], start=bad, timesteps=10)
    with pytest.raises(ValueError, match=r'restraints\[0\].*group 2 outside the batch of 2 groups'):     # a group index >= G
        m.edit_restrained_given_pockets(phar, [a, b], [dict(pos, sample=2)], timesteps=10)
    with pytest.raises(ValueError, match=r'restraints\[1\].*point 2: group 0 has 2 points'):             # a point >= n_phar of the GROUP
        m.edit_restrained_given_pockets(phar, [a, b], [pos, dict(pos, point=2)], timesteps=10)
    with pytest.raises(ValueError, match='group 1 has more than 256 restraints'):
        m.edit_restrained_given_pockets(phar, [a, b], [dict(pos, sample=1)] * 257, timesteps=10)
    with pytest.raises(ValueError, match='i == j'):
        m.edit_restrained_given_pockets(phar, [a, b], [{'kind': 'distance', 'sample': 1, 'points': (1, 1), 'lo': 1, 'hi': 2, 'k': 1}],
                                        timesteps=10)
    with pytest.raises(ValueError, match='clash'):
        m.edit_restrained_given_pockets(phar, [a, b], [pos], clash=-1.0, timesteps=10)
    with pytest.raises(ValueError, match='max_shift'):
        m.edit_restrained_given_pockets(phar, [a, b], [pos], max_shift=0.0, timesteps=10)
    with pytest.raises(ValueError, match='scale'):
        m.edit_restrained_given_pockets(phar, [a, b], [pos], scale=-1.0, timesteps=10)
    with pytest.raises(ValueError, match='guide_below'):
        m.edit_restrained_given_pockets(phar, [a, b], [pos], guide_below=1.5, timesteps=10)
    # the messages of the other entry points keep saying "sample"
    with pytest.raises(ValueError, match=r'restraints\[0\].*sample 2 outside the batch of 2 samples'):
        rs.records([dict(pos, sample=2)], [2, 3])


def test_the_wrappers_refuse_the_joint_and_the_simple_model():
    from helpers import bare_model as _model
    from cmdgen_amd.equivariant_diffusion.conditional_model import ConditionalDDPM, SimpleConditionalDDPM
    from cmdgen_amd.equivariant_diffusion.en_diffusion import EnVariationalDiffusion
    a, b, phar = _pocket([3, 4]), _pocket([5, 2]), _phar([2, 3])
    pos = {'kind': 'position', 'sample': 0, 'point': 0, 'center': (0, 0, 0), 'radius': 1, 'k': 1}
    with pytest.raises(NotImplementedError, match='edit_restrained_given_pockets is not implemented for SimpleConditionalDDPM'):
        _model(SimpleConditionalDDPM).edit_restrained_given_pockets(phar, [a, b], [pos], timesteps=10)
    with pytest.raises(NotImplementedError, match='edit_restrained_given_pockets is not implemented for the joint model'):
        EnVariationalDiffusion.edit_restrained_given_pockets(_model(ConditionalDDPM), phar, [a, b], [pos])


def test_the_records_are_made_with_the_group_counts_and_the_chain_gets_every_argument():
    """edit_restrained_given_pockets up to the chain call, on a stand-in handle: restraints.records sees the per-GROUP counts, the layout is
    the member layout, the given rows and marks hold one copy per group, and the step and the guide table are set."""
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

        def edit_plan(self, K, start, r, j):
            seen['plan'] = (K, start, r, j)
            return mre.edit_plan(r, j, K, start)[:2]

        def multi_restrained_edit_chain(self, px, poh, sizes, w, phx, phoh, fx, fh, K, **kw):
            seen.update(kw, sizes=list(sizes), w=np.asarray(w), K=K, rows=len(px), given=(tuple(phx.shape), tuple(phoh.shape)),
                        fx=fx.tolist(), fh=fh.tolist())
            raise Stop

        def run_range_guarded(self, run, status):
            return run(), None

        chain_status = None
    m.dynamics.hip_handle = lambda: Handle()
    m.refresh_learned_schedule = lambda: None
    a, b, phar = _pocket([3, 4]), _pocket([5, 2]), _phar([2, 5])
    query = [{'kind': 'position', 'sample': 1, 'point': 4, 'center': (1, 2, 3), 'radius': 1.5, 'k': 1},
             {'kind': 'exclusion', 'sample': 0, 'center': (0, 0, 0), 'radius': 2, 'k': 0.5}]
    fix = torch.tensor([1, 0, 1, 1, 0, 0, 0])
    with pytest.raises(Stop):
        m.edit_restrained_given_pockets(phar, [a, b], query, fix_coords=fix, fix_types=1 - fix, start=6, resamplings=2, jump_length=2,
                                        weights=[3.0, 1.0], clash=(3.0, 2.0), scale=0.5, max_shift=0.7, guide_below=0.8, timesteps=10, seed=4,
                                        group_ids=[7, 9])
    assert seen['layout'] == ([2, 2, 5, 5], [3, 5, 4, 2]) and seen['sizes'] == [2, 2] and seen['rows'] == 14
    assert seen['step'] == (10, (11, 4)) and seen['guide'] == (10, (10, 2)) and seen['plan'] == (10, 6, 2, 2)
    assert seen['given'] == ((7, 3), (7, 8)) and seen['fx'] == [1, 0, 1, 1, 0, 0, 0] and seen['fh'] == [0, 1, 0, 0, 1, 1, 1]
    assert np.allclose(seen['w'], [0.75, 0.25, 0.75, 0.25])
    assert seen['restraints']['sample'].tolist() == [1, 0] and seen['restraints']['i'].tolist() == [4, 0]
    assert (seen['clash_radius'], seen['clash_k'], seen['scale'], seen['max_shift'], seen['guide_below']) == (3.0, 2.0, 0.5, 0.7, 0.8)
    assert (seen['start'], seen['resamplings'], seen['jump_length'], seen['seed'], seen['group_ids']) == (6, 2, 2, 4, [7, 9])


def test_edit_phars_multi_restrained_moves_back_by_the_first_pocket():
    """PharPocketDDPM.edit_phars_multi_restrained up to the chain and back (the chain replaced by an identity that returns the given rows and
    moves every pocket by its own vector): the masks of keep, every copy gets the list under its own group index, the result comes back by
    the FIRST pocket's shift, and the argument checks raise before the chain is called."""
    from cmdgen_amd.lightning_modules import PharPocketDDPM
    from helpers import _hparams
    model = PharPocketDDPM(**_hparams('CA', 64, 2))
    names = list(model.dataset_info['phar_decoder'])
    pdb, ids = os.path.join(GOLDEN, 'g7_pocket.pdb'), [f'A:{i}' for i in range(1, 30)]
    phars = [(names[1], (9.0, 2.0, -15.0)), (names[3], (11.5, 4.0, -13.0)), (names[1], (7.0, 5.0, -12.0))]
    query = [{'kind': 'distance', 'points': (0, 3), 'lo': 5.0, 'hi': 7.0, 'k': 1.0},
             {'kind': 'position', 'point': 4, 'center': (10.0, 3.0, -14.0), 'radius': 2.0, 'k': 1.0}]
    seen = {}

    def identity(phar, pockets, restraints, **kw):
        seen.update(kw, phar=phar, restraints=restraints, n_pockets=len(pockets))
        G = len(phar['size'])
        return (torch.cat([phar['x'] + 3.0, phar['one_hot']], 1),                         # the chain's frame: the first pocket's, moved by +3
                [torch.cat([q['x'] + 3.0 * (m + 1), q['one_hot'].float()], 1) for m, q in enumerate(pockets)],
                phar['mask'], [q['mask'] for q in pockets], {'energy': torch.zeros(G), 'max_violation': torch.zeros(G)})
    model.ddpm.edit_restrained_given_pockets = identity
    out, info = model.edit_phars_multi_restrained([pdb, pdb], 3, phars, query, clash=3.0, num_nodes_phar=5, pocket_ids=[ids, ids],
                                                  weights=[0.5, 0.5], scale=0.5, timesteps=50, seed=5)
    assert [len(s) for s in out] == [5, 5, 5] and seen['n_pockets'] == 2 and seen['start'] is None and set(info) == {'energy', 'max_violation'}
    assert (seen['clash'], seen['scale'], seen['seed'], seen['timesteps'], seen['weights']) == (3.0, 0.5, 5, 50, [0.5, 0.5])
    assert [r['sample'] for r in seen['restraints']] == [0, 0, 1, 1, 2, 2]                # every copy gets the list
    assert all(dict(r, sample=None) == dict(q, sample=None) for r, q in zip(seen['restraints'], query * 3))
    assert seen['fix_coords'].tolist() == [1.0, 1.0, 1.0, 0.0, 0.0] * 3 and seen['fix_types'].tolist() == [1.0, 1.0, 1.0, 0.0, 0.0] * 3
    for sample in out:                                                                    # back by the first pocket's +3, not the second's +6
        for (_, xyz), (_, got) in zip(phars, sample):
            assert np.allclose(np.asarray(got), np.asarray(xyz), atol=1e-4)
    out, _ = model.edit_phars_multi_restrained([pdb, pdb], 4, phars, query, pocket_ids=[ids, ids], timesteps=50, seed=5)
    assert all(len(s) >= 5 for s in out)                                                  # from the prior: at least the rows the query names
    model.ddpm.edit_restrained_given_pockets = None                                       # the checks below raise before the chain
    with pytest.raises(ValueError, match='one per file'):
        model.edit_phars_multi_restrained([pdb, pdb], 2, phars, query, pocket_ids=[ids], timesteps=50)
    with pytest.raises(ValueError, match=r"restraints\[0\].*without 'sample'"):
        model.edit_phars_multi_restrained([pdb, pdb], 2, phars, [dict(query[0], sample=0)], num_nodes_phar=5, pocket_ids=[ids, ids], timesteps=50)
    with pytest.raises(ValueError, match=r'restraints\[1\].*point 4'):
        model.edit_phars_multi_restrained([pdb, pdb], 2, phars, query, num_nodes_phar=4, pocket_ids=[ids, ids], timesteps=50)
    with pytest.raises(ValueError, match='strength'):
        model.edit_phars_multi_restrained([pdb, pdb], 2, phars, query, strength=0.5, num_nodes_phar=5, pocket_ids=[ids, ids], timesteps=50)
    with pytest.raises(ValueError, match='keep'):
        model.edit_phars_multi_restrained([pdb, pdb], 2, phars, query, keep=['types'], pocket_ids=[ids, ids], timesteps=50)


def test_the_new_entry_is_bound_and_exported():
    from cmdgen_amd import hip_backend
    lib = hip_backend.load_library()
    table = dict((s[0], s) for s in hip_backend.SYMBOLS)
    sig, medit, mrest = table['cmdgen_multi_restrained_edit_chain'], table['cmdgen_multi_edit_chain'][2], table['cmdgen_multi_restrained_chain'][2]
    assert sig[1] is ctypes.c_int and len(sig[2]) == 33
    # the multi-pocket edit chain's arguments up to pocket_steps_out, the restraint arguments, the two energies, use_graph and the stream
    assert sig[2][:22] == medit[:22] and sig[2][22:29] == mrest[7:14] and sig[2][29:31] == mrest[21:23] and sig[2][31:] == medit[22:]
    assert lib.cmdgen_multi_restrained_edit_chain.argtypes == sig[2] and lib.cmdgen_multi_restrained_edit_chain.restype is ctypes.c_int
    assert hasattr(hip_backend.Handle, 'multi_restrained_edit_chain')
    with open(os.path.join(os.path.dirname(GOLDEN), '..', 'include', 'cmdgen_hip.h')) as f:
        assert 'int cmdgen_multi_restrained_edit_chain(cmdgen_handle* h' in f.read()
