"""GPU tests of ConditionalDDPM.sample_diverse_restrained / cmdgen_diverse_restrained_chain: parity with diverse_restrained_ref on injected noise (a
batch that takes every branch of the mean, the clash term, both clips, a sample above 128 nodes), every reduction to a parent chain bit for bit,
graphs against eager launches and run to run with the parents' chains interleaved, the two guide_belows, the effect itself, refusals, and the
Python entry points up to PharPocketDDPM.generate_phars_diverse_restrained.

Bounds against the model are the chain tests' (chain_kit.PARITY): per-op z and pocket <= 1e-4 max(1, max|.|), final x and pocket RMS under the same
bound, types exact; energy, max_violation, op_energy, overlap and op_overlap within 1e-4 max(1, |want|), the parents' bound.  A set with a member
within 1e-4 A of the cutoff at any reference evaluation is left out whole (diverse_restrained_cases.py: none for the committed inputs)."""
import os
from collections import namedtuple

import numpy as np
import pytest
import torch

import diverse_restrained_cases as drc
import chain_kit as kit
from chain_kit import PARITY, PLAIN, SMALL, check_against_ref, dev, handle, lightning_model, model, pocket_dev, record, status_key
from helpers import GOLDEN
from cmdgen_amd import hip_backend
from cmdgen_amd.synthetic import ModelConfig, make_state_dict, make_pockets

pytestmark = pytest.mark.gpu
FIELDS = PLAIN + ('energy', 'op_energy', 'overlap', 'op_overlap', 'chain_z')
ENERGY, OVERLAP = ('energy', 'op_energy'), ('overlap', 'op_overlap')
CHAIN = PLAIN + ('chain_z',)
Run = namedtuple('Run', FIELDS)


def run(h, pb, K, kind='both', sets=None, rec=None, clash=drc.NO_CLASH, scale=drc.SCALE, max_shift=drc.MAX_SHIFT, guide_below=1.0,
        strength=drc.STRENGTH, width=drc.WIDTH, diverse_max_shift=drc.DIVERSE_MAX_SHIFT, diverse_guide_below=1.0, noise=None, seed=7, ids=None,
        use_graph=True):
    """One chain on the layout of pb through the binding of `kind`: 'both' (cmdgen_diverse_restrained_chain), 'restrained', 'diverse' or 'plain'
    - each with its own arguments of those above -> Run (the fields a kind lacks None), chain status."""
    h.set_layout(pb.num_nodes_phar, pb.size)
    kit.host_tables(h, K)
    px, poh = dev(pb.x), dev(pb.one_hot)
    tail = dict(noise=noise, seed=seed, pocket_ids=ids, want_steps=True, use_graph=use_graph)
    g = dict(clash_radius=clash[0], clash_k=clash[1], scale=scale, max_shift=max_shift, guide_below=guide_below)
    en = oe = ov = oo = None
    if kind == 'both':
        x, q, zs, en, oe, ov, oo = h.diverse_restrained_chain(px, poh, K, sets, rec, strength=strength, width=width,
                                                              diverse_max_shift=diverse_max_shift, diverse_guide_below=diverse_guide_below, **g, **tail)
    elif kind == 'restrained':
        x, q, zs, en, oe = h.restrained_chain(px, poh, K, rec, **g, **tail)
    elif kind == 'diverse':
        x, q, zs, ov, oo = h.diverse_chain(px, poh, K, sets, strength=strength, width=width, max_shift=diverse_max_shift,
                                           guide_below=diverse_guide_below, **tail)
    else:
        x, q, zs = h.sample_chain(px, poh, K, **tail)
    st = h.chain_status()
    return Run(*[t.cpu().numpy() if t is not None else None for t in (x, q, zs, h.last_pocket_steps, en, oe, ov, oo)], kit.chain_z(h)), st


def same(a, b, names):
    """Bit for bit: the fields `names` of two Runs."""
    for n in names:
        u, v = getattr(a, n), getattr(b, n)
        assert u is not None and v is not None and u.shape == v.shape and np.array_equal(u, v), n


def plain_handle():
    """The launches of SMALL with the evaluations' own k_readout: what the reductions are stated for."""
    return handle(options=dict(SMALL, readout_in_coord=0))


def case_args(r, case, variant=None):
    """run()'s arguments of a case (and variant) of diverse_restrained_cases."""
    v = dict(drc.VARIANTS[variant]) if variant else {}
    return dict(sets=case.sets, rec=r['rec'], clash=v.get('clash', case.clash), max_shift=v.get('max_shift', drc.MAX_SHIFT),
                diverse_max_shift=v.get('diverse_max_shift', drc.DIVERSE_MAX_SHIFT))


# ------------------------------------------------------------------------------------------------ 1. against the model
@pytest.mark.parametrize('case,variant,use_graph', [(drc.MIXED, None, True), (drc.MIXED, None, False), (drc.MIXED, 'clash', False),
                                                    (drc.MIXED, 'clipped', False), (drc.LARGE, None, False)],
                         ids=['mixed-graph', 'mixed-eager', 'mixed-clash-eager', 'mixed-clipped-eager', 'large-eager'])
def test_chain_matches_the_model(case, variant, use_graph):
    r = drc.reference(case, variant)
    pb, want, keep, ks = r['pb'], r['both'], r['keep'], r['keep_samples']
    h = handle()
    h.set_option('graph_steps', 2)                                   # K = 5: two replays of two steps, one eager step
    got, st = run(h, pb, case.K, noise=r['noise'].cuda(), use_graph=use_graph, **case_args(r, case, variant))
    rows, rows_q = ks[np.repeat(np.arange(len(case.nph)), case.nph)], ks[pb.mask]
    label = f'{case.name}{" " + variant if variant else ""} {"graph" if use_graph else "eager"}'
    check_against_ref(label, got, st, {k: want[k] for k in PLAIN}, rows, rows_q, keep, 'sets', final='rms')
    rel = lambda g, w: float((np.abs(g - w.numpy()) / (PARITY * np.maximum(1.0, np.abs(w.numpy())))).max())
    ratios = {'energy': rel(got.energy[ks, 0], want['energy'][ks]), 'max_violation': rel(got.energy[ks, 1], want['max_violation'][ks]),
              'op_energy': rel(got.op_energy[:, ks], want['op_energy'][:, ks]), 'overlap': rel(got.overlap[ks], want['overlap'][ks]),
              'op_overlap': rel(got.op_overlap[:, ks], want['op_overlap'][:, ks])}
    print(f'[{label}] worst ratio to the bound: ' + '  '.join(f'{k} {v:.3f}' for k, v in ratios.items()))
    assert all(v <= 1.0 for v in ratios.values()), ratios
    if case.big_set is not None:
        assert int((pb.size + pb.num_nodes_phar).max()) > 128           # the 1024-thread step ran


# ------------------------------------------------------------------------------------------------ 2. the reductions
@pytest.mark.parametrize('use_graph', [True, False], ids=['graph', 'eager'])
@pytest.mark.parametrize('inject', [False, True], ids=['device-draws', 'injected'])
def test_with_a_term_off_it_is_the_parent_chain_bit_for_bit(inject, use_graph):
    """Every row of the reductions table, on a handle whose evaluations run their own k_readout: the overlap term off three ways against
    cmdgen_restrained_chain (energy and op_energy too), the restraint term off two ways against cmdgen_diverse_chain (overlap and op_overlap
    too), both off against cmdgen_sample_chain - every output, chain_z and the chain status."""
    case = drc.MIXED
    r = drc.reference(case)
    pb, rec, K = r['pb'], r['rec'], 10
    ones = (1,) * len(case.nph)
    h = plain_handle()
    h.set_option('graph_steps', 8)
    h.set_layout(pb.num_nodes_phar, pb.size)
    assert h.query('readout_in_coord') == 0
    noise = dev(np.random.default_rng(6).normal(size=(K + 2, int(pb.num_nodes_phar.sum()), 11)).astype(np.float32)) if inject else None
    kw = dict(noise=noise, seed=11, ids=pb.pocket_index, use_graph=use_graph)
    both, sb = run(h, pb, K, sets=case.sets, rec=rec, **kw)
    restrained, sr = run(h, pb, K, 'restrained', rec=rec, **kw)
    diverse, sd = run(h, pb, K, 'diverse', sets=case.sets, **kw)
    plain, sp = run(h, pb, K, 'plain', **kw)
    for how, a in (('strength = 0', dict(sets=case.sets, strength=0.0)), ('diverse_guide_below = 0', dict(sets=case.sets, diverse_guide_below=0.0)),
                   ('sets of one', dict(sets=ones))):
        got, st = run(h, pb, K, rec=rec, **a, **kw)
        same(got, restrained, CHAIN + ENERGY)
        assert status_key(st) == status_key(sr), how
    for how, a in (('scale = 0', dict(rec=rec, scale=0.0)), ('nothing touched', dict(rec=None))):
        got, st = run(h, pb, K, sets=case.sets, **a, **kw)
        same(got, diverse, CHAIN + OVERLAP)
        assert status_key(st) == status_key(sd), how
    for a in (dict(sets=case.sets, rec=rec, scale=0.0, strength=0.0), dict(sets=ones, rec=None),
              dict(sets=case.sets, rec=rec, guide_below=0.0, diverse_guide_below=0.0)):
        got, st = run(h, pb, K, **a, **kw)
        same(got, plain, CHAIN)
        assert status_key(st) == status_key(sp)
    assert sb['nan_resets'] == sp['nan_resets'] == 0
    for parent in (restrained, diverse, plain):                         # ... and neither term is a no-op here
        assert not np.array_equal(both.z_steps[0], parent.z_steps[0]) and not np.array_equal(both.xh_phar, parent.xh_phar)


# ------------------------------------------------------------------------------------------------ 3. graphs and slots
def test_captured_equals_eager_and_either_parts_change_prepares_the_slot_again():
    case = drc.MIXED
    r = drc.reference(case)
    pb, rec = r['pb'], r['rec']
    h = handle()
    h.set_option('graph_steps', 2)
    kw = dict(seed=31)
    own = dict(sets=case.sets, rec=rec)
    a, sa = run(h, pb, case.K, **own, **kw)
    assert h.query('chain_graphs') >= 1
    pr, _ = run(h, pb, case.K, 'restrained', rec=rec, **kw)             # the parents' chains in between, on their own slots
    pd, _ = run(h, pb, case.K, 'diverse', sets=case.sets, **kw)
    a2, sa2 = run(h, pb, case.K, **own, **kw)
    e, se = run(h, pb, case.K, use_graph=False, **own, **kw)
    same(a, a2, FIELDS)
    same(a, e, FIELDS)
    assert status_key(sa) == status_key(sa2) == status_key(se) and sa['nan_resets'] == 0
    moved = rec.copy()
    moved['c'][moved['kind'] == 0] += 2.0                               # every position restraint's centre
    changes = {'a record': dict(own, rec=moved), 'the partition': dict(own, sets=(5, 3, 3)), 'clash_k': dict(own, clash=(3.0, 2.0)),
               'scale': dict(own, scale=0.5), 'width': dict(own, width=3.0), 'diverse_max_shift': dict(own, diverse_max_shift=0.01),
               'guide_below': dict(own, guide_below=0.5), 'diverse_guide_below': dict(own, diverse_guide_below=0.5)}
    for what, args in changes.items():
        b, _ = run(h, pb, case.K, **args, **kw)
        assert not np.array_equal(a.xh_phar, b.xh_phar), what
    b_eager, _ = run(h, pb, case.K, use_graph=False, **changes['diverse_guide_below'], **kw)
    same(b, b_eager, FIELDS)
    back, sb = run(h, pb, case.K, **own, **kw)
    same(a, back, FIELDS)
    assert status_key(sa) == status_key(sb)
    pr2, _ = run(h, pb, case.K, 'restrained', rec=rec, **kw)
    pd2, _ = run(h, pb, case.K, 'diverse', sets=case.sets, **kw)
    same(pr, pr2, CHAIN + ENERGY)
    same(pd, pd2, CHAIN + OVERLAP)


# ------------------------------------------------------------------------------------------------ 4. the two guide_belows
def test_the_two_guide_belows_are_independent():
    """K = 5, the restraint side guided throughout, the overlap side from t / T = 0.5 down: t / T = 1, .8, .6 have no overlap term - the first
    three saved steps are the restraints-only run's, the fourth differs."""
    case = drc.MIXED
    r = drc.reference(case)
    pb, rec = r['pb'], r['rec']
    h = handle()
    only, _ = run(h, pb, case.K, sets=case.sets, rec=rec, strength=0.0, seed=51)
    part, _ = run(h, pb, case.K, sets=case.sets, rec=rec, guide_below=1.0, diverse_guide_below=0.5, seed=51)
    full, _ = run(h, pb, case.K, sets=case.sets, rec=rec, seed=51)
    assert np.array_equal(part.z_steps[:3], only.z_steps[:3]) and not np.array_equal(part.z_steps[3], only.z_steps[3])
    assert not np.array_equal(part.z_steps[0], full.z_steps[0])
    assert np.array_equal(part.op_energy[:4], only.op_energy[:4]) and np.array_equal(part.op_overlap[:4], only.op_overlap[:4])
    # ... and the other way round: the restraint side from 0.5 down under a full overlap term
    pushed, _ = run(h, pb, case.K, sets=case.sets, rec=rec, scale=0.0, seed=51)
    late, _ = run(h, pb, case.K, sets=case.sets, rec=rec, guide_below=0.5, diverse_guide_below=1.0, seed=51)
    assert np.array_equal(late.z_steps[:3], pushed.z_steps[:3]) and not np.array_equal(late.z_steps[3], pushed.z_steps[3])


# ------------------------------------------------------------------------------------------------ 5. the effect
def test_both_terms_take_effect_together():
    """What test_diverse_restrained_cpu.py established on the model, on the device with the same noise: under both terms the coupled sets overlap
    less than under the restraints alone, and the touched samples violate their restraints less than under the overlap term alone."""
    case = drc.MIXED
    r = drc.reference(case)
    h = handle()
    kw = dict(sets=case.sets, rec=r['rec'], noise=r['noise'].cuda())
    both, _ = run(h, r['pb'], case.K, **kw)
    restrained, _ = run(h, r['pb'], case.K, strength=0.0, **kw)
    diverse, _ = run(h, r['pb'], case.K, scale=0.0, **kw)
    c, t = r['coupled'], r['touched']
    ov = [float(x.overlap[c].sum()) for x in (both, restrained)]
    en = [float(x.energy[t, 0].sum()) for x in (both, diverse)]
    print(f'\n[effect] summed overlap of the coupled sets: both {ov[0]:.4f}, restraints only {ov[1]:.4f}; summed energy of the touched samples: '
          f'both {en[0]:.4f}, overlap only {en[1]:.4f}')
    assert c.sum() >= 9 and t.sum() >= 7
    assert ov[0] < ov[1] and en[0] < en[1]


# ------------------------------------------------------------------------------------------------ 6. refusals
def _small_handle(**cfg_kw):
    cfg = ModelConfig(hidden_nf=64, n_layers=1, **cfg_kw)
    h = hip_backend.Handle(cfg.as_dict(), 0)
    h.load_state_dict(make_state_dict(cfg, seed=0))
    return h, cfg


def _refusal_inputs():
    pb = make_pockets(3, 'CA', ragged=True, first_index=9700)
    pb.num_nodes_phar[:] = (3, 1, 5)
    return pb, dev(pb.x), dev(pb.one_hot)


@pytest.fixture(scope='module')
def refusing():
    pb, px, poh = _refusal_inputs()
    h, cfg = _small_handle(timesteps=500)
    h.set_layout(pb.num_nodes_phar, pb.size)
    yield h, px, poh, (lambda match, sets=(3,), rec=None, **kw: kit.refused(h, lambda: h.diverse_restrained_chain(px, poh, 5, sets, rec, **kw), match))
    h.close()


def test_a_null_pointer_is_refused(refusing):
    h, px, poh, _ = refusing
    lib, out = h.lib, torch.empty((9, 11), device='cuda')
    sizes = np.asarray([3], dtype=np.int64)
    sp = sizes.ctypes.data_as(hip_backend._i64p)
    ptr = hip_backend._ptr
    q = torch.empty((int(h.n_pocket), 3 + h.cfg['residue_nf']), device='cuda')
    en, ov = torch.empty((3, 2), device='cuda'), torch.empty(3, device='cuda')
    full = [h.h, ptr(px), ptr(poh), 5, None, 0, 0.0, 0.0, 1.0, 1.0, 1.0, 1, sp, 1.0, 2.0, 1.0, 1.0, None, 3, None, ptr(out), ptr(q), None, None,
            ptr(en), None, ptr(ov), None, 0, None]
    assert lib.cmdgen_diverse_restrained_chain(*full) == 0                # the list itself is a valid call
    for at in (1, 2, 12, 20, 21, 24, 26):               # pocket_x, pocket_onehot, set_size_host, xh_phar_out, xh_pocket_out, energy_out, overlap_out
        args = list(full)
        args[at] = None
        assert lib.cmdgen_diverse_restrained_chain(*args) == kit.EINVAL and 'null pointer' in lib.cmdgen_last_error(h.h).decode(), at
    args = list(full)
    args[5] = 2                                                           # records announced, none given
    assert lib.cmdgen_diverse_restrained_chain(*args) == kit.EINVAL and 'without a restraint list' in lib.cmdgen_last_error(h.h).decode()


def test_a_bad_argument_of_either_side_is_refused_in_the_parents_words(refusing):
    _, _, _, refused = refusing
    # the partition and the overlap term's scalars: cmdgen_diverse_chain's
    refused('n_sets=4', sets=(1, 1, 1, 1))
    refused('n_sets=0', sets=())
    refused(r'set_size\[1\]=0', sets=(3, 0))
    refused('set_size sums to 2', sets=(1, 1))
    refused('set_size sums to 4', sets=(2, 2))
    for bad in (-1.0, float('nan')):
        refused('strength=', strength=bad)
    for bad in (0.0, float('inf')):
        refused('width=', width=bad)
    refused('max_shift=-1', diverse_max_shift=-1.0)
    refused('guide_below=1.5', diverse_guide_below=1.5)
    # the records and the restraint term's scalars: cmdgen_restrained_chain's
    refused('unknown kind', rec=record(kind=3))
    refused('outside the layout', rec=record(sample=3))
    refused('point 1, sample 1 has 1 points', rec=record(sample=1, i=1))
    refused('i == j', rec=record(kind=1, sample=2, i=2, j=2, a=1.0, b=2.0))
    refused('scale=', rec=record(), scale=-1.0)
    refused('clash_radius=', clash_radius=-1.0)
    refused('max_shift=0', rec=record(), max_shift=0.0)
    refused('guide_below=-0.1', rec=record(), guide_below=-0.1)


def test_the_handle_stays_usable_after_refusals(refusing):
    h, px, poh, refused = refusing
    refused('strength', strength=-1.0)
    refused('scale', scale=-1.0)
    good = h.diverse_restrained_chain(px, poh, 5, (2, 1), record(), clash_radius=3.0, clash_k=1.0, seed=3, want_steps=True)
    plain = h.sample_chain(px, poh, 5, seed=3)                          # ... and an ordinary chain follows
    st = h.chain_status()
    assert good[0].shape == plain[0].shape == (9, 11) and good[3].shape == (3, 2) and good[4].shape == (5, 3) and good[5].shape == (3,)
    assert good[6].shape == (5, 3) and st['max_rel_com_error'] < 1e-2
    assert all(bool(torch.isfinite(t).all()) for t in (*good[:1], *good[3:], plain[0]))
    assert float(good[5][2]) == 0.0 and float(good[5][:2].min()) >= 0.0


def test_a_sample_the_diverse_chain_takes_is_beyond_this_steps_lds():
    """800 nodes: 64 B per node for the diverse step (1024 fit), 92 B per node here (712 fit) - refused before anything is launched."""
    h, cfg = _small_handle(timesteps=500)
    h.set_layout([3, 2], [797, 5])
    px, poh = torch.zeros((802, 3), device='cuda'), torch.zeros((802, cfg.residue_nf), device='cuda')
    px[:, 0] = torch.arange(802, device='cuda') * 3.8                   # a chain of atoms: no clump of neighbours
    assert h.diverse_chain(px, poh, 2, (2,), seed=3)[0].shape == (5, 11)
    before = h.counters()
    kit.refused(h, lambda: h.diverse_restrained_chain(px, poh, 2, (2,), record()), '800 nodes: the restrained step keeps')
    assert h.counters() == before                                       # nothing ran
    h.set_layout([3, 2], [709, 5])                                      # 712 nodes: the largest sample that fits
    assert h.diverse_restrained_chain(px[:714], poh[:714], 2, (2,), record(), seed=3)[0].shape == (5, 11)
    h.close()


def test_the_joint_and_the_no_com_handles_refuse_and_run_their_own_chains():
    pb, px, poh = _refusal_inputs()
    joint, _ = _small_handle(update_pocket_coords=True)
    joint.set_layout(pb.num_nodes_phar, pb.size)
    kit.refused(joint, lambda: joint.diverse_restrained_chain(px, poh, 5, (3,), record()), 'the restrained diverse chain is not supported for the joint',
                code=kit.ESTATE)
    assert joint.joint_chain(5, seed=3)[0].shape == (9, 11)
    joint.close()
    simple, _ = _small_handle(timesteps=500, no_com_projection=True)
    simple.set_layout(pb.num_nodes_phar, pb.size)
    kit.refused(simple, lambda: simple.diverse_restrained_chain(px, poh, 5, (3,), record()),
                'the restrained diverse chain is not supported for no_com_projection')
    assert simple.sample_chain(px, poh, 5, seed=3)[0].shape == (9, 11)
    simple.close()


def test_groups_or_given_rows_are_not_combined_with_it(refusing):
    h, px, poh, _ = refusing
    g, s = (None, 0.0, 0.0, 1.0, 1.0, 1.0), ((3,), 1.0, 2.0, 1.0, 1.0)
    kw = dict(guide=g, sets=s, noise=None, seed=3, ids=None, want_steps=False, use_graph=False)
    with pytest.raises(hip_backend.CmdgenError, match='no chain entry'):
        h._sampling_chain(px, poh, 5, groups=((3,), np.ones(3, np.float32)), **kw)
    with pytest.raises(hip_backend.CmdgenError, match='no chain entry'):
        h._sampling_chain(px, poh, 5, given=(None,) * 4, plan=(None, 1, 1), **kw)


# ------------------------------------------------------------------------------------------------ 7. the Python entry points
def test_sample_diverse_restrained_returns_the_chains_result():
    """ConditionalDDPM.sample_diverse_restrained on the mixed case: the chain's outputs (bit for bit the binding's, same tables and draws), frames
    and info keys, strength = 0 as sample_restrained and scale = 0 as sample_diverse."""
    case = drc.MIXED
    r = drc.reference(case)
    pb = r['pb']
    ddpm = model()
    ddpm.use_hip_graph = True
    pocket = pocket_dev(pb)
    noise = r['noise'].cuda()
    both = dict(clash=drc.CLASH, scale=drc.SCALE, strength=drc.STRENGTH, width=drc.WIDTH, max_shift=drc.MAX_SHIFT, timesteps=case.K, noise=noise)
    x, q, pm, qm, info = ddpm.sample_diverse_restrained(pocket, case.nph, case.sets, r['restraints'], **both)
    want, _ = run(ddpm.dynamics.hip_handle(), pb, case.K, sets=case.sets, rec=r['rec'], clash=drc.CLASH, noise=noise)
    assert np.array_equal(x.cpu().numpy(), want.xh_phar) and np.array_equal(q.cpu().numpy(), want.xh_pocket)
    assert np.array_equal(info['energy'].cpu().numpy(), want.energy[:, 0]) and np.array_equal(info['max_violation'].cpu().numpy(), want.energy[:, 1])
    assert np.array_equal(info['overlap'].cpu().numpy(), want.overlap)
    assert set(info) == {'energy', 'max_violation', 'overlap'} and pm.shape == (sum(case.nph),)
    frames = ddpm.sample_diverse_restrained(pocket, case.nph, case.sets, r['restraints'], return_frames=case.K, **both)
    assert frames[0].shape == (case.K, sum(case.nph), 11) and set(frames[4]) == {'energy', 'max_violation', 'overlap', 'op_energy', 'op_overlap'}
    assert torch.equal(frames[0][0], x)
    assert np.array_equal(frames[4]['op_energy'].cpu().numpy(), want.op_energy) and np.array_equal(frames[4]['op_overlap'].cpu().numpy(), want.op_overlap)
    restrained = ddpm.sample_restrained(pocket, case.nph, r['restraints'], clash=drc.CLASH, timesteps=case.K, noise=noise)
    off = ddpm.sample_diverse_restrained(pocket, case.nph, case.sets, r['restraints'], **dict(both, strength=0.0))
    assert torch.equal(off[0], restrained[0]) and torch.equal(off[1], restrained[1]) and torch.equal(off[4]['energy'], restrained[4]['energy'])
    diverse = ddpm.sample_diverse(pocket, case.nph, case.sets, timesteps=case.K, noise=noise)
    off = ddpm.sample_diverse_restrained(pocket, case.nph, case.sets, r['restraints'], **dict(both, scale=0.0))
    assert torch.equal(off[0], diverse[0]) and torch.equal(off[1], diverse[1]) and torch.equal(off[4]['overlap'], diverse[4]['overlap'])
    assert not torch.equal(x, restrained[0]) and not torch.equal(x, diverse[0])


def test_generate_phars_diverse_restrained_end_to_end():
    """PharPocketDDPM.generate_phars_diverse_restrained on the g7 pocket (30 C-alpha residues): per-sample point lists in the PDB's frame, the
    three diagnostics, the same seed the same result, strength = 0 generate_phars_restrained's lists exactly.  Width 100 A and strength 100 for
    the reason test_hip_diverse.py's end-to-end test gives (an untrained model's 50-op chain leaves the points hundreds of A out).  The
    measured overlap and energy against both parents are printed, not asserted."""
    m = lightning_model()
    pdb = os.path.join(GOLDEN, 'g7_pocket.pdb')
    ids = [f'A:{i}' for i in range(1, 30)]
    query = [{'kind': 'position', 'point': 0, 'center': (9.0, 2.0, -15.0), 'radius': 1.5, 'k': 1.0},
             {'kind': 'distance', 'points': (0, 1), 'lo': 5.0, 'hi': 7.0, 'k': 1.0}]
    nph = torch.tensor([4, 7, 3])
    kw = dict(pocket_ids=ids, num_nodes_phar=nph, timesteps=50, seed=5)
    out, info = m.generate_phars_diverse_restrained(pdb, 3, query, clash=3.0, strength=100.0, width=100.0, **kw)
    assert [len(s) for s in out] == [4, 7, 3] and all(tuple(info[k].shape) == (3,) for k in ('energy', 'max_violation', 'overlap'))
    names = set(m.dataset_info['phar_decoder'])
    assert all(name in names and len(xyz) == 3 for s in out for name, xyz in s)
    out2, info2 = m.generate_phars_diverse_restrained(pdb, 3, query, clash=3.0, strength=100.0, width=100.0, **kw)
    assert out == out2 and all(torch.equal(info[k], info2[k]) for k in info)
    off, info0 = m.generate_phars_diverse_restrained(pdb, 3, query, clash=3.0, strength=0.0, width=100.0, **kw)
    restrained, info_r = m.generate_phars_restrained(pdb, 3, query, clash=3.0, **kw)
    assert off == restrained and torch.equal(info0['energy'], info_r['energy']) and torch.equal(info0['max_violation'], info_r['max_violation'])
    _, info_d = m.generate_phars_diverse(pdb, 3, strength=100.0, width=100.0, **kw)
    print(f'\n[generate_phars_diverse_restrained] overlap: both {info["overlap"].tolist()}, restraints only {info0["overlap"].tolist()}, overlap only '
          f'{info_d["overlap"].tolist()}; energy: both {info["energy"].tolist()}, restraints only {info_r["energy"].tolist()}')
