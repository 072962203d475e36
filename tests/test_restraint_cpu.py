"""The restrained chain on the CPU: the premises of the GPU cases on the oracle-built model alone (restraint_ref) - the leave-out cap, every
restraint kind violated at some op, clipped and unclipped displacements, a guided result far from the unguided one - the reduction to
ref_cpu.sample_given_pocket, the gradient against finite differences of the energy, and the argument checks of the Python entry points
that need no device."""
import numpy as np
import pytest
import torch

import restraint_cases as rc
import restraint_ref as rr
from helpers import NoiseTape
from oracle import ref_cpu
from cmdgen_amd import restraints as rs

PARITY = 1e-4          # the GPU comparison's bound, relative to max(1, max|x|)


@pytest.mark.parametrize('case', [rc.MIXED, rc.LARGE], ids=lambda c: c.name)
def test_at_most_a_fifth_of_a_case_is_left_out(case):
    r = rc.reference(case)
    left_out = int((~r['keep']).sum())
    print(f"\n[{case.name}] smallest cutoff margin per sample (A): guided {r['guided']['margins'].min(axis=0)}, unguided "
          f"{r['unguided']['margins'].min(axis=0)}; left out {left_out} of {len(case.nph)}")
    assert left_out <= rc.CHAIN_CAP * len(case.nph)
    if case.big_sample is not None:
        assert int(r['pb'].size[case.big_sample] + case.nph[case.big_sample]) > 128       # the 1024-thread step


def test_the_mixed_case_exercises_every_term():
    case = rc.MIXED
    r = rc.reference(case)
    g, u = r['guided'], r['unguided']
    kinds = {int(q['kind']) for q in r['rec']}
    assert kinds == {rr.POSITION, rr.DISTANCE, rr.EXCLUSION} and rc.CLASH[0] > 0
    single = [q for q in r['rec'] if case.nph[int(q['sample'])] == 1]
    assert {int(q['kind']) for q in single} == {rr.POSITION, rr.EXCLUSION}
    assert case.bare_sample not in {int(q['sample']) for q in r['rec']}
    worst = g['kind_violation'].max(dim=0).values
    print('\nlargest violation at any op, per kind (A):', dict(zip(rr.KIND_NAMES, worst.tolist())), '; displacements clipped',
          g['clipped'], 'unclipped', g['unclipped'])
    assert bool((worst > 0).all())
    assert g['clipped'] >= 1 and g['unclipped'] >= 1
    x, x0 = g['xh_phar'][:, :3], u['xh_phar'][:, :3]
    apart = float((x - x0).abs().max())
    bound = PARITY * max(1.0, float(x0.abs().max()))
    print(f'guided against unguided, same draws: max |dx| {apart:.3f} A = {apart / bound:.0f} x the parity bound; E {u["energy"].sum():.2f} -> '
          f'{g["energy"].sum():.2f}')
    assert apart > 100 * bound
    keep = r['keep']
    assert bool((g['energy'][keep] < u['energy'][keep]).all())           # the GPU effect test's premise


@pytest.mark.parametrize('with_scale_zero', [False, True])
def test_without_guidance_the_model_is_the_oracle_chain_bit_for_bit(with_scale_zero):
    case = rc.MIXED
    pb, noise = rc.pockets(case), rc.noise_of(case)
    rec = rs.records(rc.restraints_of(case, pb), case.nph) if with_scale_zero else rs.records([], case.nph)
    with torch.no_grad():
        want = ref_cpu.sample_given_pocket(rc.params(), rc.config().as_dict(), rc.pocket_dict(pb), case.nph, timesteps=rc.K,
                                           noise=NoiseTape(noise.numpy()), return_chain=True)
    got = rc.run_ref(case, pb, rec, noise, 0.0 if with_scale_zero else rc.SCALE, clash=rc.CLASH if with_scale_zero else (0.0, 0.0))
    assert torch.equal(got['xh_phar'], want[0]) and torch.equal(got['xh_pocket'], want[1])
    assert torch.equal(got['z_steps'], torch.stack(want[4][1:]))
    if not with_scale_zero:
        assert float(got['op_energy'].abs().max()) == 0.0 and float(got['energy'].abs().max()) == 0.0


def _fd_setup():
    g = torch.Generator().manual_seed(5)
    pm = torch.tensor([0, 0, 0, 1, 1])
    qm = torch.tensor([0] * 6 + [1] * 4)
    xhat = torch.randn((5, 3), generator=g, dtype=torch.float64) * 2.0
    q = torch.randn((10, 3), generator=g, dtype=torch.float64) * 2.0
    shift = torch.randn((2, 3), generator=g, dtype=torch.float64)
    return pm, qm, xhat, q, shift


FD_CASES = {
    'position': ([{'kind': 'position', 'sample': 0, 'point': 1, 'center': (0.5, -0.3, 0.2), 'radius': 0.4, 'k': 1.3},
                  {'kind': 'position', 'sample': 1, 'point': 0, 'center': (3.0, 1.0, -2.0), 'radius': 1.0, 'k': 0.7}], 0.0),
    'distance': ([{'kind': 'distance', 'sample': 0, 'points': (0, 2), 'lo': 9.0, 'hi': 11.0, 'k': 0.9},      # below lo
                  {'kind': 'distance', 'sample': 1, 'points': (1, 0), 'lo': 0.1, 'hi': 0.5, 'k': 1.1}], 0.0),    # above hi
    'exclusion': ([{'kind': 'exclusion', 'sample': 0, 'center': (0.0, 0.0, 0.0), 'radius': 6.0, 'k': 0.8},
                   {'kind': 'exclusion', 'sample': 1, 'center': (1.0, 0.0, -1.0), 'radius': 5.0, 'k': 1.5}], 0.0),
    'clash': ([], 4.0),
}


@pytest.mark.parametrize('kind', sorted(FD_CASES))
def test_gradient_matches_finite_differences_of_the_energy(kind):
    """g = dE / dxhat in float64: central differences with h = 1e-6 A agree to 1e-6 relative to the largest gradient component (the energy is
    quadratic in the violation and smooth away from v = 0 and dist = 0; the inputs keep every active term away from both)."""
    restraints, clash_r = FD_CASES[kind]
    pm, qm, xhat, q, shift = _fd_setup()
    rec = rs.records(restraints, [3, 2])
    E, g, vmax, vkind = rr.energy_terms(xhat, q, shift, pm, qm, rec, clash_r, 1.2)
    assert float(E.sum()) > 0 and float(vkind[rr.KIND_NAMES.index(kind)]) > 0
    h = 1e-6
    fd = torch.zeros_like(g)
    for i in range(xhat.shape[0]):
        for k in range(3):
            xp, xm = xhat.clone(), xhat.clone()
            xp[i, k] += h
            xm[i, k] -= h
            fd[i, k] = (rr.energy_terms(xp, q, shift, pm, qm, rec, clash_r, 1.2)[0].sum() -
                        rr.energy_terms(xm, q, shift, pm, qm, rec, clash_r, 1.2)[0].sum()) / (2 * h)
    err = float((fd - g).abs().max())
    print(f'\n[{kind}] max |g| {float(g.abs().max()):.3f}, max |fd - g| {err:.2e}')
    assert err <= 1e-6 * max(1.0, float(g.abs().max()))


def test_a_term_at_zero_distance_contributes_no_gradient():
    pm, qm = torch.tensor([0]), torch.tensor([0])
    x = torch.zeros((1, 3), dtype=torch.float64)
    rec = rs.records([{'kind': 'exclusion', 'sample': 0, 'center': (0.0, 0.0, 0.0), 'radius': 2.0, 'k': 1.0}], [1])
    E, g, vmax, _ = rr.energy_terms(x, x.clone(), torch.zeros((1, 3), dtype=torch.float64), pm, qm, rec, 1.0, 1.0)
    assert float(g.abs().max()) == 0.0 and float(E[0]) == 0.5 * 4.0 + 0.5 * 1.0 and float(vmax[0]) == 2.0


# ------------------------------------------------------------------------------------------------ validation (no device)
GOOD = {'position': {'kind': 'position', 'sample': 1, 'point': 2, 'center': (1.0, 2.0, 3.0), 'radius': 1.5, 'k': 1.0},
        'distance': {'kind': 'distance', 'sample': 0, 'points': (0, 1), 'lo': 5.0, 'hi': 7.0, 'k': 1.0},
        'exclusion': {'kind': 'exclusion', 'sample': 1, 'center': (0.0, 0.0, 0.0), 'radius': 3.0, 'k': 0.5}}
NPH = [2, 3]


def test_records_of_a_valid_list():
    rec = rs.records([GOOD['position'], GOOD['distance'], GOOD['exclusion']], NPH)
    assert rec.dtype.itemsize == 40 and list(rec['kind']) == [0, 1, 2] and list(rec['sample']) == [1, 0, 1]
    assert (rec['i'][0], rec['a'][0]) == (2, 1.5) and tuple(rec['c'][0]) == (1.0, 2.0, 3.0)
    assert (rec['i'][1], rec['j'][1], rec['a'][1], rec['b'][1]) == (0, 1, 5.0, 7.0)
    one = rs.records([{k: v for k, v in GOOD['exclusion'].items() if k != 'sample'}], NPH, sample=0)
    assert int(one['sample'][0]) == 0


@pytest.mark.parametrize('kind,change,match', [
    ('position', {'kind': 'angle'}, 'unknown kind'),
    ('position', {'sample': 2}, 'sample 2 outside'),
    ('position', {'sample': -1}, 'outside'),
    ('position', {'point': 3}, 'point 3: sample 1 has 3 points'),
    ('position', {'point': -1}, 'point -1'),
    ('position', {'point': 1.5}, 'not an integer'),
    ('position', {'radius': -0.1}, 'radius'),
    ('position', {'radius': float('nan')}, 'radius'),
    ('position', {'k': -1.0}, 'k='),
    ('position', {'k': float('inf')}, 'k='),
    ('position', {'center': (0.0, 1.0)}, 'center'),
    ('position', {'center': (0.0, 1.0, float('nan'))}, 'center'),
    ('position', {'lo': 1.0}, 'not understood'),
    ('distance', {'points': (1, 1)}, 'i == j'),
    ('distance', {'points': (0, 2)}, 'point 2: sample 0 has 2 points'),
    ('distance', {'points': (0,)}, 'pair'),
    ('distance', {'lo': 8.0}, 'lo=8.0 > hi=7.0'),
    ('distance', {'lo': -1.0}, 'lo'),
    ('distance', {'hi': float('inf')}, 'hi'),
    ('exclusion', {'radius': -2.0}, 'radius'),
    ('exclusion', {'k': float('nan')}, 'k='),
])
def test_a_bad_restraint_is_refused_by_name(kind, change, match):
    bad = dict(GOOD[kind], **change)
    with pytest.raises(ValueError, match=match) as e:
        rs.records([GOOD['exclusion'], bad], NPH)
    assert 'restraints[1]' in str(e.value)


def test_missing_keys_the_cap_and_the_scalars_are_refused():
    with pytest.raises(ValueError, match="missing \\['radius'\\]"):
        rs.records([{k: v for k, v in GOOD['position'].items() if k != 'radius'}], NPH)
    with pytest.raises(ValueError, match="expected a dict with a 'kind'"):
        rs.records([('position', 0)], NPH)
    with pytest.raises(ValueError, match=f'more than {rs.MAX_RESTRAINTS} restraints'):
        rs.records([GOOD['exclusion']] * (rs.MAX_RESTRAINTS + 1), NPH)
    assert len(rs.records([GOOD['exclusion']] * rs.MAX_RESTRAINTS, NPH)) == rs.MAX_RESTRAINTS >= 256
    for bad in (-1.0, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='scale'):
            rs.check_scalars(bad, 1.0, 1.0)
    for bad in (0.0, -1.0, float('nan')):
        with pytest.raises(ValueError, match='max_shift'):
            rs.check_scalars(1.0, bad, 1.0)
    for bad in (-0.1, 1.1, float('nan')):
        with pytest.raises(ValueError, match='guide_below'):
            rs.check_scalars(1.0, 1.0, bad)
    assert rs.check_scalars(0, 2, 0) == (0.0, 2.0, 0.0)
    for bad in (-1.0, (3.0, -1.0), (float('nan'), 1.0)):
        with pytest.raises(ValueError, match='clash'):
            rs.clash_pair(bad)
    assert rs.clash_pair(None) == (0.0, 0.0) and rs.clash_pair(3) == (3.0, rs.DEFAULT_CLASH_K) and rs.clash_pair((3.0, 0.5)) == (3.0, 0.5)
