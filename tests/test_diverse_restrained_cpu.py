"""Diverse sampling under restraints on the CPU: the premises of the GPU cases on the oracle-built model alone (diverse_restrained_ref) - no set
left out, both terms acting and each clip capping some displacements and not others, the combined run differing from both parents, the two effect
conditions - the reductions of the model to its two parents bit for bit, the new symbol, and the wrappers' argument checks that need no device."""
import ctypes
import os

import numpy as np
import pytest
import torch

import diverse_cases as dc
import diverse_restrained_cases as drc
import restraint_ref as rr
from helpers import GOLDEN, _hparams, bare_model

CHAIN = ('xh_phar', 'xh_pocket', 'z_steps', 'pocket_steps')
RUNS = ('both', 'restrained', 'diverse', 'neither')


# ------------------------------------------------------------------------------------------------ the cases' premises
@pytest.mark.parametrize('case,variant', [(drc.MIXED, None), (drc.MIXED, 'clash'), (drc.MIXED, 'clipped'), (drc.LARGE, None)],
                         ids=['mixed', 'mixed-clash', 'mixed-clipped', 'large'])
def test_no_set_of_the_committed_inputs_is_left_out(case, variant):
    r = drc.reference(case, variant)
    b = r['both']
    left_out = int((~r['keep']).sum())
    print(f"\n[{case.name} {variant or ''}] smallest cutoff margin (A): " + ', '.join(f"{k} {r[k]['margins'].min():.2e}" for k in RUNS) +
          f"; left out {left_out} of {len(case.sets)} sets; restraint displacements capped {b['clipped']} of {b['total']}, overlap displacements "
          f"{b['diverse_clipped']} of {b['diverse_total']}")
    assert left_out <= drc.CHAIN_CAP * len(case.sets)
    assert left_out == 0                                               # the committed inputs: first_index was chosen for this
    assert b['total'] > 0 and b['diverse_total'] > 0                   # both terms act
    if case.big_set is not None:
        assert int((r['pb'].size + r['pb'].num_nodes_phar).max()) > 128        # the 1024-thread step
    if variant == 'clipped':
        assert 0 < b['clipped'] < b['total'] and 0 < b['diverse_clipped'] < b['diverse_total']       # some capped and some not, on both sides
    if variant is None and case is drc.MIXED:
        # with the clash term off every branch of the mean is taken in the one batch
        t, c = r['touched'], r['coupled']
        assert [int(v.sum()) for v in (t & c, t & ~c, ~t & c, ~t & ~c)] == [6, 1, 3, 1]
        assert (t & ~c).tolist().index(True) == 4 and (~t & ~c).tolist().index(True) == 10 and (~t & c)[7]


@pytest.mark.parametrize('case', [drc.MIXED, drc.LARGE], ids=lambda c: c.name)
def test_the_combined_run_differs_from_both_parents(case):
    r = drc.reference(case)
    for parent in ('restrained', 'diverse', 'neither'):
        assert not torch.equal(r['both']['z_steps'][0], r[parent]['z_steps'][0]), parent
        assert not torch.equal(r['both']['xh_phar'], r[parent]['xh_phar']), parent


def test_both_terms_take_effect_together():
    """Conditions on the chosen inputs of `mixed`: under both terms the coupled sets overlap less than under the restraints alone, and the
    touched samples violate their restraints less than under the overlap term alone."""
    r = drc.reference(drc.MIXED)
    c, t = r['coupled'], r['touched']
    ov = {k: float(r[k]['overlap'].numpy()[c].sum()) for k in RUNS}
    en = {k: float(r[k]['energy'].numpy()[t].sum()) for k in RUNS}
    print(f'\n[mixed] summed overlap of the coupled sets {ov}\n        summed energy of the touched samples {en}')
    assert ov['both'] < ov['restrained'] and en['both'] < en['diverse']


# ------------------------------------------------------------------------------------------------ the reductions
@pytest.mark.parametrize('case', [drc.MIXED, drc.LARGE], ids=lambda c: c.name)
def test_without_the_overlap_term_the_model_is_the_restrained_chain_bit_for_bit(case):
    r = drc.reference(case)
    pb, noise, rec = r['pb'], r['noise'], r['rec']
    tape = iter(noise)
    with torch.no_grad():
        want = rr.restrained_chain(drc.params(), drc.config().as_dict(), drc.pocket_dict(pb), case.nph, rec, clash_r=case.clash[0],
                                   clash_k=case.clash[1], scale=drc.SCALE, max_shift=drc.MAX_SHIFT, timesteps=case.K,
                                   noise=lambda shape: next(tape))
    runs = {'strength-zero': r['restrained'], 'sets-of-one': drc.run_ref(case, pb, rec, noise, sets=(1,) * len(case.nph)),
            'diverse-guide-below-zero': drc.run_ref(case, pb, rec, noise, diverse_guide_below=0.0)}
    for how, got in runs.items():
        for k in CHAIN + ('energy', 'max_violation', 'op_energy'):
            assert torch.equal(got[k], want[k]), (how, k)
    assert float(r['restrained']['overlap'].max()) > 0 and not runs['sets-of-one']['overlap'].any()     # still reported where defined


@pytest.mark.parametrize('case', [drc.MIXED, drc.LARGE], ids=lambda c: c.name)
def test_without_the_restraint_term_the_model_is_the_diverse_chain_bit_for_bit(case):
    r = drc.reference(case)
    pb, noise, rec = r['pb'], r['noise'], r['rec']
    want = dc.run_ref(case, pb, noise, strength=drc.STRENGTH, max_shift=drc.DIVERSE_MAX_SHIFT)
    runs = {'scale-zero': r['diverse'], 'nothing-touched': drc.run_ref(case, pb, rec[:0], noise, clash=drc.NO_CLASH)}
    for how, got in runs.items():
        for k in CHAIN + ('overlap', 'op_overlap'):
            assert torch.equal(got[k], want[k]), (how, k)
    assert float(r['diverse']['energy'].max()) > 0 and not runs['nothing-touched']['energy'].any()
    plain = dc.run_ref(case, pb, noise, strength=0.0)
    for k in CHAIN:
        assert torch.equal(r['neither'][k], plain[k]), k


# ------------------------------------------------------------------------------------------------ the ABI and the Python-side checks
def test_the_new_entry_is_bound():
    from cmdgen_amd import hip_backend
    lib = hip_backend.load_library()
    table = dict((s[0], s) for s in hip_backend.SYMBOLS)
    sig, restrained, diverse = (table['cmdgen_' + n] for n in ('diverse_restrained_chain', 'restrained_chain', 'diverse_chain'))
    assert sig[1] is ctypes.c_int and len(sig[2]) == 30
    # the restrained chain's arguments up to guide_below, the diverse chain's partition and scalars, the draws and the four outputs, the
    # restrained chain's two side outputs, the diverse chain's two, the tail
    assert sig[2][:11] == restrained[2][:11] and sig[2][11:17] == diverse[2][4:10] and sig[2][17:24] == restrained[2][11:18]
    assert sig[2][24:26] == restrained[2][18:20] and sig[2][26:28] == diverse[2][17:19] and sig[2][28:] == restrained[2][20:]
    assert lib.cmdgen_diverse_restrained_chain.argtypes == sig[2] and lib.cmdgen_diverse_restrained_chain.restype is ctypes.c_int
    assert hasattr(hip_backend.Handle, 'diverse_restrained_chain')
    with open(os.path.join(os.path.dirname(GOLDEN), '..', 'include', 'cmdgen_hip.h')) as f:
        hdr = f.read()
    at = hdr.index('int cmdgen_diverse_restrained_chain(cmdgen_handle* h')
    decl = ' '.join(hdr[at:hdr.index(';', at)].split())
    for piece in ('const cmdgen_restraint* restraints_host, int64_t n_restraints, float clash_radius, float clash_k, float scale, float max_shift, '
                  'float guide_below, int64_t n_sets, const int64_t* set_size_host, float strength, float width, float diverse_max_shift, '
                  'float diverse_guide_below, const float* noise, uint64_t seed', 'float* energy_out', 'float* op_energy_out', 'float* overlap_out',
                  'float* op_overlap_out', 'int32_t use_graph, cmdgen_stream stream)'):
        assert piece in decl, piece
    assert decl.index('energy_out') < decl.index('op_energy_out') < decl.index('float* overlap_out') < decl.index('op_overlap_out')


def _never(*a, **kw):
    raise AssertionError('the chain was reached')


def test_sample_diverse_restrained_checks_its_arguments_before_the_chain():
    from cmdgen_amd.equivariant_diffusion.conditional_model import ConditionalDDPM
    case = drc.MIXED
    r = drc.reference(case)
    pb = r['pb']
    ddpm = bare_model(ConditionalDDPM)
    ddpm._run_chain = _never
    pocket = drc.pocket_dict(pb)
    call = lambda sets=case.sets, restraints=r['restraints'], **kw: ddpm.sample_diverse_restrained(pocket, case.nph, sets, restraints,
                                                                                                 timesteps=case.K, **kw)
    with pytest.raises(ValueError, match='set_sizes sums to 9'):
        call(sets=(4, 5))
    with pytest.raises(ValueError, match='at least one sample'):
        call(sets=(11, 0))
    for name, bad, match in (('scale', -1.0, 'scale'), ('max_shift', 0.0, 'max_shift'), ('guide_below', 1.5, 'guide_below'),
                             ('strength', -1.0, 'strength'), ('width', 0.0, 'width'), ('diverse_max_shift', -2.0, 'max_shift'),
                             ('diverse_guide_below', float('nan'), 'guide_below')):
        with pytest.raises(ValueError, match=match):
            call(**{name: bad})
    with pytest.raises(ValueError, match='point 9'):
        call(restraints=[{'kind': 'position', 'sample': 0, 'point': 9, 'center': (0, 0, 0), 'radius': 1.0, 'k': 1.0}])
    # None on the overlap side takes the restraint side's values
    seen = {}
    ddpm._run_chain = lambda method, ps, nph, timesteps, **kw: seen.update(kw, method=method)
    call(max_shift=0.3, guide_below=0.6, strength=2.0, width=1.5)
    assert seen['method'] == 'diverse_restrained_chain' and seen['info'] == (ConditionalDDPM.ENERGY_INFO, ConditionalDDPM.OVERLAP_INFO)
    s = seen['steer']
    assert (s['max_shift'], s['guide_below'], s['diverse_max_shift'], s['diverse_guide_below'], s['strength'], s['width']) == (0.3, 0.6, 0.3, 0.6, 2.0, 1.5)
    assert seen['behind'][0].tolist() == list(case.sets) and len(seen['behind'][1]) == len(r['rec'])
    call(diverse_max_shift=0.9, diverse_guide_below=0.25)
    assert (seen['steer']['diverse_max_shift'], seen['steer']['diverse_guide_below']) == (0.9, 0.25)


def test_generate_phars_diverse_restrained_checks_its_restraints_before_the_chain():
    from cmdgen_amd.lightning_modules import PharPocketDDPM
    model = PharPocketDDPM(**_hparams('CA', 64, 2))
    model.ddpm.sample_diverse_restrained = _never
    pdb, ids = os.path.join(GOLDEN, 'g7_pocket.pdb'), [f'A:{i}' for i in range(1, 30)]
    query = [{'kind': 'position', 'point': 0, 'center': (9.0, 2.0, -15.0), 'radius': 1.5, 'k': 1.0},
             {'kind': 'distance', 'points': (0, 1), 'lo': 5.0, 'hi': 7.0, 'k': 1.0}]
    with pytest.raises(ValueError, match=r"restraints\[0\].*without 'sample'"):
        model.generate_phars_diverse_restrained(pdb, 2, [dict(query[0], sample=0)], pocket_ids=ids, timesteps=50)
    with pytest.raises(ValueError, match=r'restraints\[1\].*point 1'):
        model.generate_phars_diverse_restrained(pdb, 2, query, pocket_ids=ids, num_nodes_phar=torch.tensor([4, 1]), timesteps=50)
    seen = {}

    def chain(pocket, num_nodes_phar, set_sizes, restraints, **kw):
        seen.update(kw, sets=list(set_sizes), restraints=restraints, nph=num_nodes_phar.tolist())
        raise StopIteration

    model.ddpm.sample_diverse_restrained = chain
    with pytest.raises(StopIteration):
        model.generate_phars_diverse_restrained(pdb, 3, query, pocket_ids=ids, num_nodes_phar=torch.tensor([4, 7, 3]), strength=2.0, seed=5)
    assert seen['sets'] == [3] and seen['nph'] == [4, 7, 3] and seen['strength'] == 2.0 and seen['diverse_max_shift'] is None
    assert [q['sample'] for q in seen['restraints']] == [0, 0, 1, 1, 2, 2]                 # every copy gets the list; all copies form one set


def test_the_other_models_refuse_with_a_reason():
    from cmdgen_amd.equivariant_diffusion.conditional_model import ConditionalDDPM, SimpleConditionalDDPM
    from cmdgen_amd.equivariant_diffusion.en_diffusion import EnVariationalDiffusion
    with pytest.raises(NotImplementedError, match='SimpleConditionalDDPM'):
        SimpleConditionalDDPM.sample_diverse_restrained(None)
    with pytest.raises(NotImplementedError, match='joint model'):
        EnVariationalDiffusion.sample_diverse_restrained(None)
    assert ConditionalDDPM.sample_diverse_restrained is not SimpleConditionalDDPM.sample_diverse_restrained
