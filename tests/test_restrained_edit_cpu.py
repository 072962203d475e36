"""Editing under restraints on the CPU: the premises of the GPU cases on the oracle-built model alone (restrained_edit_ref) - the leave-out
cap, every term kind, a held-free distance term and a held row with energy - the model's reductions to edit_ref.cond_edit and to
restraint_ref.restrained_chain bit for bit, the held rows' estimate, the effect of the guidance, the step kernel's LDS plan, and the argument
checks of the Python entry points that need no device."""
import atexit
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import restrained_edit_cases as ec
import restrained_edit_ref as rer
import restraint_ref as rr
from edit_ref import cond_edit
from cmdgen_amd import restraints as rs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = [ec.MIXED, ec.JUMPS, ec.LARGE]


@pytest.mark.parametrize('case', ALL, ids=lambda c: c.name)
def test_at_most_a_fifth_of_a_case_is_left_out(case):
    r = ec.reference(case)
    left_out = int((~r['keep']).sum())
    print(f"\n[{case.name}] smallest cutoff margin per sample (A): guided {r['guided']['margins'].min(axis=0)}, unguided "
          f"{r['unguided']['margins'].min(axis=0)}; left out {left_out} of {len(case.nph)}")
    assert left_out <= ec.CHAIN_CAP * len(case.nph)
    n_steps, n_draws, n_jumps = ec.plan(case)
    assert r['guided']['z_steps'].shape[0] == n_steps and r['guided']['margins'].shape == (n_steps + 1, len(case.nph))
    if case.big_sample is not None:
        assert int(r['pb'].size[case.big_sample] + case.nph[case.big_sample]) > 128       # the 1024-thread step
        assert int(r['pb'].size[case.big_sample]) > 128                                   # the pocket loops past their second trip
    if case.name == 'jumps':
        assert n_jumps >= 1 and case.start < case.K
    else:
        assert n_jumps == 0 and case.start == case.K


def test_the_mixed_case_exercises_every_term_and_both_kinds_of_rows():
    case = ec.MIXED
    r = ec.reference(case)
    g = r['guided']
    fx, fh = torch.from_numpy(r['fx']) != 0, torch.from_numpy(r['fh']) != 0
    pm = g['phar_mask']
    nph = torch.tensor(case.nph)
    pbase = torch.cumsum(nph, 0) - nph
    assert {int(q['kind']) for q in r['rec']} == {rr.POSITION, rr.DISTANCE, rr.EXCLUSION} and ec.CLASH[0] > 0
    assert case.nph[1] == 1 and bool(fx[pbase[1]])                                      # the single point is held
    assert not bool((fx | fh)[pm == case.no_mark].any())                                # a sample without a mark
    assert bool(fh[pm == case.types_only].any()) and not bool(fx[pm == case.types_only].any())
    assert case.bare not in {int(q['sample']) for q in r['rec']} and bool(fx[pm == case.bare].any())
    worst = g['kind_violation'].max(dim=0).values
    print('\nlargest violation at any op, per kind (A):', dict(zip(rr.KIND_NAMES, worst.tolist())))
    assert bool((worst > 0).all())
    # a violated distance term between an x-held and a free row, and a held row with energy of its own, at some op
    seen = dict(held_free=0.0, held_energy=0.0)

    def probe(op, a):
        n_x = ec.config().as_dict()['norm_values'][0]
        xhat, shift, E, _, _ = rer.op_terms(a['z'], a['P'], a['eps_t'], a['known'], a['fx'], a['sigma_t'], a['alpha_t'], a['com_in'], a['pm'],
                                            a['qm'], r['rec'], ec.CLASH[0], ec.CLASH[1], n_x, 3)
        for q in r['rec']:
            if int(q['kind']) != rr.DISTANCE:
                continue
            i, j = int(pbase[int(q['sample'])]) + int(q['i']), int(pbase[int(q['sample'])]) + int(q['j'])
            if bool(a['fx'][i]) != bool(a['fx'][j]):
                d = float((xhat[i] - xhat[j]).norm())
                seen['held_free'] = max(seen['held_free'], float(q['a']) - d, d - float(q['b']))
        q_atoms = n_x * a['P'][:, :3]
        for i in torch.nonzero(a['fx']).reshape(-1).tolist():                           # the exclusion and clash terms of the held rows
            b = int(a['pm'][i])
            e = 0.0
            for q in r['rec']:
                if int(q['kind']) == rr.EXCLUSION and int(q['sample']) == b:
                    dist = float((xhat[i] - (torch.from_numpy(q['c'].copy()) + shift[b])).norm())
                    e += 0.5 * float(q['k']) * max(0.0, float(q['a']) - dist) ** 2
            dist = (xhat[i][None, :] - q_atoms[a['qm'] == b]).norm(dim=1)
            e += float((0.5 * ec.CLASH[1] * torch.clamp(ec.CLASH[0] - dist, min=0) ** 2).sum())
            seen['held_energy'] = max(seen['held_energy'], e)

    ec.run_ref(case, r['pb'], r['rec'], r['noise'], ec.SCALE, probe=probe)
    print('largest violation of a held-free distance term (A):', seen['held_free'], '; largest energy of a held row (exclusion and clash terms):',
          seen['held_energy'])
    assert seen['held_free'] > 0 and seen['held_energy'] > 0
    x, x0 = g['xh_phar'][:, :3], r['unguided']['xh_phar'][:, :3]
    assert float((x - x0).abs().max()) > 100 * 1e-4 * max(1.0, float(x0.abs().max()))   # the guidance is far above the parity bound


def _same(got, want):
    assert torch.equal(got['xh_phar'], want[0]) and torch.equal(got['xh_pocket'], want[1])
    assert torch.equal(got['z_steps'], want[4]) and torch.equal(got['pocket_steps'], want[5])


@pytest.mark.parametrize('case', ALL, ids=lambda c: c.name)
@pytest.mark.parametrize('form', ['scale0', 'no_restraints'])
def test_without_guidance_the_model_is_the_edit_model_bit_for_bit(case, form):
    r = ec.reference(case)
    tape = iter(r['noise'])
    with torch.no_grad():
        want = cond_edit(ec.params(), ec.config().as_dict(), r['phar'], ec.pocket_dict(r['pb']), r['fx'], r['fh'], start=case.start,
                         resamplings=case.r, jump_length=case.j, timesteps=case.K, noise=lambda shape: next(tape), return_steps=True)
    if form == 'scale0':
        got = r['unguided']
    else:
        got = ec.run_ref(case, r['pb'], rs.records([], case.nph), r['noise'], ec.SCALE, clash=(0.0, 0.0))
        assert float(got['op_energy'].abs().max()) == 0.0 and float(got['energy'].abs().max()) == 0.0
    _same(got, want)


@pytest.mark.parametrize('case', [ec.MIXED, ec.LARGE], ids=lambda c: c.name)
def test_without_marks_the_model_is_the_restrained_model_bit_for_bit(case):
    """From the prior and without jumps the draws are z_T, (A, B) per op and the decode: the restrained chain reads z_T, the A rows, the decode."""
    r = ec.reference(case)
    n_steps = ec.plan(case)[0]
    assert n_steps == case.K
    got = ec.run_ref(case, r['pb'], r['rec'], r['noise'], ec.SCALE, marked=False)
    rows = [0] + [1 + 2 * i for i in range(n_steps)] + [len(r['noise']) - 1]
    tape = iter(r['noise'][rows])
    with torch.no_grad():
        want = rr.restrained_chain(ec.params(), ec.config().as_dict(), ec.pocket_dict(r['pb']), case.nph, r['rec'], clash_r=ec.CLASH[0],
                                   clash_k=ec.CLASH[1], scale=ec.SCALE, max_shift=ec.MAX_SHIFT, timesteps=case.K,
                                   noise=lambda shape: next(tape))
    for key in ('xh_phar', 'xh_pocket', 'z_steps', 'pocket_steps', 'op_energy', 'energy', 'max_violation'):
        assert torch.equal(got[key], want[key]), key
    assert np.array_equal(got['margins'], want['margins'])
    assert float(want['op_energy'].abs().max()) > 0


def test_a_held_row_enters_the_energy_at_its_given_position():
    case = ec.MIXED
    r = ec.reference(case)
    n_x = ec.config().as_dict()['norm_values'][0]
    ops = []

    def probe(op, a):
        args = (a['P'], a['eps_t'], a['known'], a['fx'], a['sigma_t'], a['alpha_t'], a['com_in'], a['pm'], a['qm'], r['rec'], ec.CLASH[0],
                ec.CLASH[1], n_x, 3)
        xhat, shift, E, g, _ = rer.op_terms(a['z'], *args)
        held = a['fx']
        assert int(held.sum()) > 0
        assert torch.equal(xhat[held], n_x * a['known'][held, :3] + shift[a['pm']][held])
        z2 = a['z'].clone()
        z2[held] += torch.randn((int(held.sum()), z2.shape[1]), generator=torch.Generator().manual_seed(op))
        xhat2, _, E2, g2, _ = rer.op_terms(z2, *args)
        assert torch.equal(E2, E) and torch.equal(g2, g) and torch.equal(xhat2, xhat)
        z3 = a['z'].clone()
        z3[~held, :3] += 0.5                                       # (while a free row's z does move the energy)
        ops.append(bool((rer.op_terms(z3, *args)[2] != E).any()))

    g = ec.run_ref(case, r['pb'], r['rec'], r['noise'], ec.SCALE, probe=probe)
    assert len(ops) == ec.plan(case)[0] and any(ops)
    assert torch.equal(g['op_energy'], r['guided']['op_energy'])
    # and the held rows of every saved step are the noised known rows in that step's frame
    fx = torch.from_numpy(r['fx']) != 0
    err = float((g['z_steps'][:, fx, :3] - g['known_steps'][:, fx]).abs().max())
    print(f'\nheld rows of z_steps against the noised known rows: max |dx| {err:.2e}')
    assert err <= 1e-5 * max(1.0, float(g['z_steps'][:, :, :3].abs().max()))


def test_the_guided_reference_ends_with_less_energy():
    r = ec.reference(ec.MIXED)
    g, u = r['guided']['energy'], r['unguided']['energy']
    print('\nE of the returned samples, unguided:', u.tolist(), '\n                        guided:', g.tolist())
    touched = rr.touched_samples(r['rec'], len(ec.MIXED.nph), ec.CLASH[0])
    fx = np.split(r['fx'], np.cumsum(ec.MIXED.nph)[:-1])
    with_free = [b for b in range(len(ec.MIXED.nph)) if touched[b] and (fx[b] == 0).any()]
    assert tuple(with_free) == ec.EFFECT_SAMPLES                         # every restrained sample that has a free point
    for b in ec.EFFECT_SAMPLES:
        assert float(g[b]) <= float(u[b]), b
    assert float(g.sum()) < float(u.sum())


def test_step_lds_plan_at_its_boundary_sizes():
    """plan_restrained_edit_step_lds against its restatement: per node a float4 position and a degree, z (3 + P floats) per row, then xhat, d
    (3 floats each) and e (1 float); the parent's has the velocity (3 floats) besides.  The largest sample that fits 64 KiB and the first
    that does not."""
    d = tempfile.mkdtemp(prefix='redit_lds_')
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    exe = os.path.join(d, 'lds_check')
    c = subprocess.run(['/opt/rocm/bin/hipcc', '-x', 'c++', '-std=c++17', '-O1', '-Wall', '-Werror', '-I' + os.path.join(ROOT, 'cmdgen_amd', 'csrc'),
                        os.path.join(ROOT, 'tests', 'restrained_edit_lds_check.cpp'), '-o', exe], capture_output=True, text=True)
    assert c.returncode == 0, c.stderr[-2000:]
    P = 8
    per_node = 16 + 4 + 4 * (3 + P) + 4 * 7
    fits = 65536 // per_node
    sizes = [1, 2, 128, 129, 148, fits, fits + 1, 1024]
    out = subprocess.run([exe], input=''.join(f'{n} {P}\n' for n in sizes), capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr[-2000:]
    got = np.array([ln.split() for ln in out.stdout.strip().split('\n')], dtype=np.int64)
    assert got.shape == (len(sizes), 3) and bool((got[:, 2] == 65536).all())
    for n, (edit, plain, cap) in zip(sizes, got):
        assert edit == n * per_node and plain == n * (per_node + 12), n
    assert got[sizes.index(fits), 0] <= 65536 < got[sizes.index(fits + 1), 0]
    assert got[sizes.index(148), 0] <= 65536                              # the `large` case's sample fits


# ------------------------------------------------------------------------------------------------ the Python surface (no device)
GOOD = {'kind': 'position', 'sample': 1, 'point': 2, 'center': (1.0, 2.0, 3.0), 'radius': 1.5, 'k': 1.0}


def test_argument_checks_without_a_device():
    from helpers import bare_inputs as _inputs, bare_model as _model
    from cmdgen_amd.equivariant_diffusion.conditional_model import ConditionalDDPM, SimpleConditionalDDPM
    from cmdgen_amd.equivariant_diffusion.en_diffusion import EnVariationalDiffusion
    phar, pocket = _inputs()                                              # samples of 2 and 3 points
    m = _model(ConditionalDDPM)
    for bad, match in ((dict(GOOD, kind='angle'), 'unknown kind'), (dict(GOOD, sample=2), 'sample 2 outside'),
                       (dict(GOOD, point=3), 'point 3: sample 1 has 3 points'), (dict(GOOD, radius=-1.0), 'radius'),
                       (dict(GOOD, k=float('nan')), 'k='), (dict(GOOD, lo=1.0), 'not understood'),
                       ({'kind': 'distance', 'sample': 0, 'points': (1, 1), 'lo': 1.0, 'hi': 2.0, 'k': 1.0}, 'i == j'),
                       ({'kind': 'distance', 'sample': 0, 'points': (0, 1), 'lo': 3.0, 'hi': 2.0, 'k': 1.0}, 'lo=3.0 > hi=2.0')):
        with pytest.raises(ValueError, match=match) as e:
            m.edit_restrained(phar, pocket, [GOOD, bad], fix_coords=torch.ones(5), timesteps=10)
        assert 'restraints[1]' in str(e.value)
    with pytest.raises(ValueError, match='fix_coords'):
        m.edit_restrained(phar, pocket, [GOOD], fix_coords=torch.ones(4), timesteps=10)
    with pytest.raises(ValueError, match='fix_types'):
        m.edit_restrained(phar, pocket, [GOOD], fix_types=torch.ones(5, 2), timesteps=10)
    for bad in (0, 11, -1, 2.5):
        with pytest.raises(ValueError, match='start'):
            m.edit_restrained(phar, pocket, [GOOD], fix_types=torch.ones(5), start=bad, timesteps=10)
    for bad in (-1.0, float('nan')):
        with pytest.raises(ValueError, match='scale'):
            m.edit_restrained(phar, pocket, [GOOD], scale=bad, timesteps=10)
    for bad in (0.0, -1.0):
        with pytest.raises(ValueError, match='max_shift'):
            m.edit_restrained(phar, pocket, [GOOD], max_shift=bad, timesteps=10)
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError, match='guide_below'):
            m.edit_restrained(phar, pocket, [GOOD], guide_below=bad, timesteps=10)
    with pytest.raises(ValueError, match='clash'):
        m.edit_restrained(phar, pocket, [GOOD], clash=(3.0, -1.0), timesteps=10)
    with pytest.raises(NotImplementedError, match='SimpleConditionalDDPM'):
        _model(SimpleConditionalDDPM).edit_restrained(phar, pocket, [GOOD], timesteps=10)
    with pytest.raises(NotImplementedError, match='joint'):
        EnVariationalDiffusion.edit_restrained(m, phar, pocket, [GOOD])


def test_edit_phars_restrained_builds_the_masks_and_gives_every_copy_the_list():
    """PharPocketDDPM.edit_phars_restrained up to the chain and back (the chain replaced by the identity)."""
    from helpers import GOLDEN
    from cmdgen_amd.lightning_modules import PharPocketDDPM
    from helpers import _hparams
    model = PharPocketDDPM(**_hparams('CA', 64, 2))
    names = list(model.dataset_info['phar_decoder'])
    pdb, ids = os.path.join(GOLDEN, 'g7_pocket.pdb'), [f'A:{i}' for i in range(1, 30)]
    phars = [(names[1], (9.0, 2.0, -15.0)), (names[3], (11.5, 4.0, -13.0)), (names[1], (7.0, 5.0, -12.0))]
    query = [{'kind': 'distance', 'points': (0, 3), 'lo': 5.0, 'hi': 7.0, 'k': 1.0},
             {'kind': 'position', 'point': 4, 'center': (10.0, 3.0, -14.0), 'radius': 2.0, 'k': 1.0}]
    seen = {}

    def identity(phar, pocket, restraints, **kw):
        seen.update(kw, phar=phar, restraints=restraints)
        B = len(phar['size'])
        return (torch.cat([phar['x'], phar['one_hot']], 1), torch.cat([pocket['x'] + 3.0, pocket['one_hot'].float()], 1),
                phar['mask'], pocket['mask'], {'energy': torch.zeros(B), 'max_violation': torch.zeros(B)})
    model.ddpm.edit_restrained = identity
    out, info = model.edit_phars_restrained(pdb, 3, phars, query, clash=3.0, num_nodes_phar=5, pocket_ids=ids, timesteps=50, seed=5)
    assert [len(s) for s in out] == [5, 5, 5] and seen['start'] is None and seen['clash'] == 3.0 and set(info) == {'energy', 'max_violation'}
    assert [r['sample'] for r in seen['restraints']] == [0, 0, 1, 1, 2, 2]
    assert all(dict(r, sample=None) == dict(q, sample=None) for r, q in zip(seen['restraints'], query * 3))
    assert seen['fix_coords'].tolist() == [1.0, 1.0, 1.0, 0.0, 0.0] * 3 and seen['fix_types'].tolist() == [1.0, 1.0, 1.0, 0.0, 0.0] * 3
    for sample in out:
        for (_, xyz), (_, got) in zip(phars, sample):                      # moved back by the pocket's shift (-3)
            assert np.allclose(np.asarray(got), np.asarray(xyz) - 3.0, atol=1e-5)
    # default sizes from the prior: at least the rows the query names
    out, _ = model.edit_phars_restrained(pdb, 4, phars, query, pocket_ids=ids, timesteps=50, seed=5)
    assert all(len(s) >= 5 for s in out)
    model.ddpm.edit_restrained = None                                       # the checks below raise before the chain
    with pytest.raises(ValueError, match="without 'sample'"):
        model.edit_phars_restrained(pdb, 2, phars, [dict(query[0], sample=0)], num_nodes_phar=5, pocket_ids=ids, timesteps=50)
    with pytest.raises(ValueError, match=r'restraints\[1\].*point 4'):
        model.edit_phars_restrained(pdb, 2, phars, query, num_nodes_phar=4, pocket_ids=ids, timesteps=50)
    with pytest.raises(ValueError, match='strength'):
        model.edit_phars_restrained(pdb, 2, phars, query, strength=0.5, num_nodes_phar=5, pocket_ids=ids, timesteps=50)
    with pytest.raises(ValueError, match='keep'):
        model.edit_phars_restrained(pdb, 2, phars, query, keep=['types'], pocket_ids=ids, timesteps=50)


def test_the_entry_is_bound_and_declared_once():
    from cmdgen_amd import hip_backend
    lib = hip_backend.load_library()
    assert lib.cmdgen_restrained_edit_chain.argtypes is not None and len(lib.cmdgen_restrained_edit_chain.argtypes) == 30
    assert hasattr(hip_backend.Handle, 'restrained_edit_chain')
    assert 'cmdgen_restrained_edit_chain' in [s[0] for s in hip_backend.SYMBOLS]
