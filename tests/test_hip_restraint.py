"""GPU tests of ConditionalDDPM.sample_restrained / cmdgen_restrained_chain: parity with restraint_ref on injected noise for a batch with every
restraint kind and for a sample above 128 nodes, the two reductions to cmdgen_sample_chain bit for bit, graphs against eager launches and run to
run, a shard against the full batch, guide_below = 0 against scale = 0, the effect itself, refusals, and PharPocketDDPM.generate_phars_restrained.

Bounds against the reference are the chain tests' (test_hip_edit.py): per-op z and pocket <= 1e-4 max(1, max|.|), final x and pocket RMS
<= 1e-4 max(1, max|.|), types exact; energy, max_violation and op_energy within 1e-4 max(1, |want|).  A sample with a pair within 1e-4 A of the
cutoff at any reference evaluation is left out (restraint_cases.py: at most 20 % of a case's samples; none for the committed inputs)."""
import os

import numpy as np
import pytest
import torch

import restraint_cases as rc
import chain_kit as kit
from chain_kit import (GUIDED, PLAIN, SMALL, check_against_ref, dev, guide, handle, lightning_model, model, pocket_dev, record, run_chain, same,
                       status_key, sub_batch)
from helpers import GOLDEN
from cmdgen_amd import hip_backend
from cmdgen_amd import restraints as rs
from cmdgen_amd.synthetic import ModelConfig, PocketBatch, make_state_dict, make_pockets

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ 1. against the reference
def own_velocity_handle():
    """The launches under which the step kernel forms the velocity and the NaN flag itself (readout_in_coord), forced on a small layout."""
    return handle(options=dict(SMALL, readout_in_coord=1))


@pytest.mark.parametrize('use_graph', [True, False], ids=['graph', 'eager'])
@pytest.mark.parametrize('case,own_vel', [(rc.MIXED, False), (rc.MIXED, True), (rc.LARGE, False)], ids=['mixed', 'mixed-own-velocity', 'large'])
def test_chain_matches_the_reference(case, own_vel, use_graph):
    r = rc.reference(case)
    pb, want, keep = r['pb'], r['guided'], r['keep']
    h = own_velocity_handle() if own_vel else handle()
    h.set_option('graph_steps', 2)                                   # K = 5: two replays of two steps, one eager step
    h.set_layout(pb.num_nodes_phar, pb.size)
    assert h.query('readout_in_coord') == int(own_vel)
    got, st = run_chain(h, pb, rc.K, guide=guide(r['rec']), noise=r['noise'].cuda(), use_graph=use_graph)
    rows, rows_q = keep[np.repeat(np.arange(len(case.nph)), case.nph)], keep[pb.mask]
    # the final x and pocket by their RMS, the pocket over its whole row (test_hip_edit.py's bounds); at most CHAIN_CAP of the samples left out
    check_against_ref(f'{case.name} {"graph" if use_graph else "eager"}', got, st, want, rows, rows_q, keep, 'samples', final='rms')
    if case.big_sample is not None:
        assert int((pb.size + pb.num_nodes_phar).max()) > 128           # the 1024-thread step ran


# ------------------------------------------------------------------------------------------------ 2. the reductions
@pytest.mark.parametrize('use_graph', [True, False], ids=['graph', 'eager'])
@pytest.mark.parametrize('inject', [False, True], ids=['device-draws', 'injected'])
@pytest.mark.parametrize('readout', [0, 1], ids=['k_readout', 'own-velocity'])
def test_without_guidance_it_is_sample_chain_bit_for_bit(readout, inject, use_graph):
    """No restraint and r_c = 0, and scale = 0 with restraints and the clash term present: xh_phar, xh_pocket, z_steps, pocket_steps and the
    chain status of cmdgen_sample_chain, with the evaluations' own k_readout and with the step kernel forming the velocity itself."""
    K = 10
    h = handle(options=dict(SMALL, readout_in_coord=readout))
    h.set_option('graph_steps', 8)
    pb = make_pockets(6, 'CA', ragged=True, first_index=9500)
    nph = 1 + (np.arange(6, dtype=np.int64) * 3) % 8
    pb = PocketBatch(x=pb.x, one_hot=pb.one_hot, size=pb.size, mask=pb.mask, num_nodes_phar=nph, pocket_index=pb.pocket_index)
    h.set_layout(pb.num_nodes_phar, pb.size)
    assert h.query('readout_in_coord') == readout and h.query('coord_mt') == 32
    noise = dev(np.random.default_rng(6).normal(size=(K + 2, int(nph.sum()), 11)).astype(np.float32)) if inject else None
    restraints = [{'kind': 'position', 'sample': 0, 'point': 0, 'center': (1.0, 0.0, -1.0), 'radius': 1.0, 'k': 1.0},
                  {'kind': 'distance', 'sample': 2, 'points': (0, 3), 'lo': 5.0, 'hi': 7.0, 'k': 1.0},
                  {'kind': 'exclusion', 'sample': 5, 'center': (0.0, 0.0, 0.0), 'radius': 4.0, 'k': 1.0}]
    rec = rs.records(restraints, nph)
    kw = dict(noise=noise, seed=11, ids=pb.pocket_index, use_graph=use_graph)
    want, sw = run_chain(h, pb, K, **kw)
    none, s0 = run_chain(h, pb, K, guide=guide(None, clash=(0.0, 0.0)), **kw)
    zero, s1 = run_chain(h, pb, K, guide=guide(rec, scale=0.0), **kw)
    same(want, none, PLAIN)
    same(want, zero, PLAIN)
    assert status_key(sw) == status_key(s0) == status_key(s1) and sw['nan_resets'] == 0
    assert not none[4].any() and not none[5].any()                      # nothing restrains: zero energies
    assert zero[4][:, 0].max() > 0 and zero[5].max() > 0                # scale = 0 still reports them
    guided, _ = run_chain(h, pb, K, guide=guide(rec), **kw)
    assert not np.array_equal(guided[0], want[0])                       # ... and the guidance is not a no-op here


# ------------------------------------------------------------------------------------------------ 3. graphs, run to run
def test_captured_equals_eager_and_a_changed_table_prepares_the_slot_again():
    """Device draws on the mixed case, the step kernel forming its own velocity: A captured twice and eager, bit for bit; then B (other
    restraints) and A again - A's first result."""
    case = rc.MIXED
    r = rc.reference(case)
    pb = r['pb']
    h = own_velocity_handle()
    h.set_option('graph_steps', 2)
    a, sa = run_chain(h, pb, rc.K, guide=guide(r['rec']), seed=31, use_graph=True)
    assert h.query('chain_graphs') >= 1
    a2, sa2 = run_chain(h, pb, rc.K, guide=guide(r['rec']), seed=31, use_graph=True)
    e, se = run_chain(h, pb, rc.K, guide=guide(r['rec']), seed=31, use_graph=False)
    same(a, a2, GUIDED)
    same(a, e, GUIDED)
    assert status_key(sa) == status_key(sa2) == status_key(se) and sa['nan_resets'] == 0
    other = [dict(q) for q in r['restraints']]
    for q in other:
        if q['kind'] == 'position':
            q['center'] = tuple(v + 2.0 for v in q['center'])
    rec_b = rs.records(other, case.nph)
    b, _ = run_chain(h, pb, rc.K, guide=guide(rec_b), seed=31, use_graph=True)
    b_eager, _ = run_chain(h, pb, rc.K, guide=guide(rec_b), seed=31, use_graph=False)
    assert not np.array_equal(a[0], b[0])
    same(b, b_eager, GUIDED)
    c, _ = run_chain(h, pb, rc.K, guide=guide(r['rec'], clash=(rc.CLASH[0], 2.0)), seed=31, use_graph=True)      # a scalar of the key alone
    assert not np.array_equal(a[0], c[0])
    back, sb = run_chain(h, pb, rc.K, guide=guide(r['rec']), seed=31, use_graph=True)
    same(a, back, GUIDED)
    assert status_key(sa) == status_key(sb)


# ------------------------------------------------------------------------------------------------ 4. a shard
def test_a_shard_gives_the_full_batchs_rows():
    """Samples 2..4 of the mixed case alone, with their pocket ids and their restraints renumbered, device draws: the rows of the full batch
    within test_hip_edit.py's shard bound (not bit for bit: the tile rule differs with the batch size)."""
    case = rc.MIXED
    r = rc.reference(case)
    pb = r['pb']
    members = [2, 3, 4]
    h = handle()
    full, _ = run_chain(h, pb, rc.K, guide=guide(r['rec']), seed=41, ids=pb.pocket_index)
    xf, ef = full.xh_phar, full.energy
    sub = sub_batch(pb, members)
    sub_restraints = [dict(q, sample=members.index(q['sample'])) for q in r['restraints'] if q['sample'] in members]
    alone, _ = run_chain(h, sub, rc.K, guide=guide(rs.records(sub_restraints, sub.num_nodes_phar)), seed=41, ids=sub.pocket_index)
    xsub, esub = alone.xh_phar, alone.energy
    rows = np.isin(np.repeat(np.arange(len(case.nph)), case.nph), members)
    diff = float(np.abs(xsub[:, :3] - xf[rows, :3]).max())
    print(f'\n[shard] max |dx| {diff:.3e} A, bound {1e-4 * max(1.0, float(np.abs(xf[rows, :3]).max())):.3e}; energies {esub[:, 0]} / {ef[members, 0]}')
    assert diff <= 1e-4 * max(1.0, float(np.abs(xf[rows, :3]).max()))
    assert np.array_equal(xsub[:, 3:], xf[rows, 3:])
    assert np.all(np.abs(esub - ef[members]) <= 1e-4 * np.maximum(1.0, np.abs(ef[members])))


# ------------------------------------------------------------------------------------------------ 5. guide_below
def test_guide_below_zero_equals_scale_zero():
    case = rc.MIXED
    r = rc.reference(case)
    h = own_velocity_handle()
    a, sa = run_chain(h, r['pb'], rc.K, guide=guide(r['rec'], guide_below=0.0), seed=51)
    b, sb = run_chain(h, r['pb'], rc.K, guide=guide(r['rec'], scale=0.0), seed=51)
    same(a, b, GUIDED)
    assert status_key(sa) == status_key(sb)
    # ... and a threshold between two ops guides only the ops at or below it: t / T = 1, .8, .6 unguided, .4 and .2 guided
    part, _ = run_chain(h, r['pb'], rc.K, guide=guide(r['rec'], guide_below=0.5), seed=51)
    full, _ = run_chain(h, r['pb'], rc.K, guide=guide(r['rec']), seed=51)
    assert np.array_equal(part[2][:3], b[2][:3]) and not np.array_equal(part[2][3], b[2][3]) and not np.array_equal(part[2][0], full[2][0])


# ------------------------------------------------------------------------------------------------ 6. the effect
def test_guidance_lowers_the_energy_of_every_restrained_sample():
    case = rc.MIXED
    r = rc.reference(case)
    h = handle()
    noise = r['noise'].cuda()
    g, _ = run_chain(h, r['pb'], rc.K, guide=guide(r['rec']), noise=noise)
    u, _ = run_chain(h, r['pb'], rc.K, guide=guide(r['rec'], scale=0.0), noise=noise)
    restrained = np.isin(np.arange(len(case.nph)), [q['sample'] for q in r['restraints']]) & r['keep']
    print(f'\n[effect] final energy unguided {u[4][:, 0]}\n         guided   {g[4][:, 0]}\n         largest violation (A) unguided {u[4][:, 1]}\n'
          f'         guided   {g[4][:, 1]}')
    assert restrained.sum() >= 6
    assert np.all(g[4][restrained, 0] < u[4][restrained, 0])


# ------------------------------------------------------------------------------------------------ 7. refusals
def test_refusals_leave_the_handle_usable():
    cfg = ModelConfig(hidden_nf=64, n_layers=1, timesteps=500)
    pb = make_pockets(3, 'CA', ragged=True, first_index=9700)
    pb.num_nodes_phar[:] = (3, 1, 5)
    px, poh = dev(pb.x), dev(pb.one_hot)
    h = hip_backend.Handle(cfg.as_dict(), 0)
    h.load_state_dict(make_state_dict(cfg, seed=0))
    h.set_layout(pb.num_nodes_phar, pb.size)

    refused = lambda match, rec=None, **kw: kit.refused(h, lambda: h.restrained_chain(px, poh, 5, rec, **kw), match, code=None)   # the message

    refused('unknown kind', record(kind=3))
    refused('unknown kind', record(kind=-1))
    refused('outside the layout', record(sample=3))
    refused('outside the layout', record(sample=-1))
    refused('point 3, sample 0 has 3 points', record(i=3))
    refused('point 1, sample 1 has 1 points', record(sample=1, i=1))
    refused('point 5, sample 2 has 5 points', record(kind=1, sample=2, i=0, j=5, a=1.0, b=2.0))
    refused('i == j', record(kind=1, sample=2, i=2, j=2, a=1.0, b=2.0))
    refused('lo=3 > hi=2', record(kind=1, sample=2, i=0, j=1, a=3.0, b=2.0))
    refused('lo=', record(kind=1, sample=2, i=0, j=1, a=-1.0, b=2.0))
    refused('hi=', record(kind=1, sample=2, i=0, j=1, a=1.0, b=np.inf))
    refused('radius', record(a=-1.0))
    refused('radius', record(kind=2, a=np.nan))
    refused('k=', record(k=-0.5))
    refused('k=', record(kind=2, k=np.inf))
    refused('non-finite centre', record(c=(0.0, np.nan, 0.0)))
    refused('scale', record(), scale=-1.0)
    refused('scale', record(), scale=float('nan'))
    refused('clash_radius', record(), clash_radius=-1.0)
    refused('clash_k', record(), clash_radius=3.0, clash_k=float('inf'))
    refused('max_shift', record(), max_shift=0.0)
    refused('max_shift', record(), max_shift=-1.0)
    refused('guide_below', record(), guide_below=1.5)
    refused('guide_below', record(), guide_below=-0.1)
    refused('guide_below', record(), guide_below=float('nan'))
    refused('more than 256 restraints', np.concatenate([record(kind=2, sample=1)] * 257))
    cap = h.restrained_chain(px, poh, 5, np.concatenate([record(kind=2, sample=1)] * 256), seed=3)      # the cap itself runs
    good = h.restrained_chain(px, poh, 5, record(), clash_radius=3.0, clash_k=1.0, seed=3)
    plain = h.sample_chain(px, poh, 5, seed=3)                            # ... and an ordinary chain follows
    st = h.chain_status()
    assert good[0].shape == plain[0].shape == (9, 11) and good[3].shape == (3, 2) and st['max_rel_com_error'] < 1e-2
    assert all(bool(torch.isfinite(t).all()) for t in (cap[0], cap[3], good[0], good[3], plain[0]))
    # a sample beyond the step's 64 KiB of LDS (104 B per node at phar_nf 8): refused before anything is launched
    h.set_layout([3], [700])
    with pytest.raises(hip_backend.CmdgenError, match='703 nodes'):
        h.restrained_chain(torch.zeros((700, 3), device='cuda'), torch.zeros((700, cfg.residue_nf), device='cuda'), 5, record())
    h.close()
    jcfg = ModelConfig(hidden_nf=64, n_layers=1, update_pocket_coords=True)
    joint = hip_backend.Handle(jcfg.as_dict(), 0)
    joint.load_state_dict(make_state_dict(jcfg, seed=0))
    joint.set_layout(pb.num_nodes_phar, pb.size)
    with pytest.raises(hip_backend.CmdgenError, match='joint model'):
        joint.restrained_chain(px, poh, 5, record())
    assert joint.joint_chain(5, seed=3)[0].shape == (9, 11)
    joint.close()
    scfg = ModelConfig(hidden_nf=64, n_layers=1, timesteps=500, no_com_projection=True)
    simple = hip_backend.Handle(scfg.as_dict(), 0)
    simple.load_state_dict(make_state_dict(scfg, seed=0))
    simple.set_layout(pb.num_nodes_phar, pb.size)
    with pytest.raises(hip_backend.CmdgenError, match='no_com_projection'):
        simple.restrained_chain(px, poh, 5, record())
    assert simple.sample_chain(px, poh, 5, seed=3)[0].shape == (9, 11)
    simple.close()


def test_the_other_models_refuse_with_a_reason():
    from cmdgen_amd.equivariant_diffusion.conditional_model import SimpleConditionalDDPM
    from cmdgen_amd.equivariant_diffusion.en_diffusion import EnVariationalDiffusion
    with pytest.raises(NotImplementedError, match='SimpleConditionalDDPM'):
        SimpleConditionalDDPM.sample_restrained(None)
    with pytest.raises(NotImplementedError, match='joint model'):
        EnVariationalDiffusion.sample_restrained(None)


# ------------------------------------------------------------------------------------------------ 8. the Python entry points
def test_sample_restrained_returns_the_chains_result():
    """ConditionalDDPM.sample_restrained on the mixed case: the chain's outputs (bit for bit the binding's, same tables and draws), frames, and
    scale = 0 as sample_given_pocket."""
    case = rc.MIXED
    r = rc.reference(case)
    pb = r['pb']
    ddpm = model()
    ddpm.use_hip_graph = True
    pocket = pocket_dev(pb)
    noise = r['noise'].cuda()
    x, q, pm, qm, info = ddpm.sample_restrained(pocket, case.nph, r['restraints'], clash=rc.CLASH, scale=rc.SCALE, max_shift=rc.MAX_SHIFT,
                                               timesteps=rc.K, noise=noise)
    want, _ = run_chain(ddpm.dynamics.hip_handle(), pb, rc.K, guide=guide(r['rec']), noise=noise)
    assert np.array_equal(x.cpu().numpy(), want[0]) and np.array_equal(q.cpu().numpy(), want[1])
    assert np.array_equal(info['energy'].cpu().numpy(), want[4][:, 0]) and np.array_equal(info['max_violation'].cpu().numpy(), want[4][:, 1])
    assert 'op_energy' not in info and pm.shape == (sum(case.nph),)
    frames = ddpm.sample_restrained(pocket, case.nph, r['restraints'], clash=rc.CLASH, return_frames=rc.K, timesteps=rc.K, noise=noise)
    assert frames[0].shape == (rc.K, sum(case.nph), 11) and frames[4]['op_energy'].shape == (rc.K, len(case.nph))
    assert torch.equal(frames[0][0], x)
    plain = ddpm.sample_given_pocket(pocket, case.nph, timesteps=rc.K, noise=noise)
    off = ddpm.sample_restrained(pocket, case.nph, r['restraints'], clash=rc.CLASH, scale=0.0, timesteps=rc.K, noise=noise)
    assert torch.equal(off[0], plain[0]) and torch.equal(off[1], plain[1])
    with pytest.raises(ValueError, match=r'restraints\[0\]'):
        ddpm.sample_restrained(pocket, case.nph, [{'kind': 'position', 'sample': 1, 'point': 1, 'center': (0, 0, 0), 'radius': 1, 'k': 1}],
                               timesteps=rc.K)


def test_generate_phars_restrained_end_to_end():
    """PharPocketDDPM.generate_phars_restrained on the g7 pocket (30 C-alpha residues): per-sample point lists in the PDB's frame, the two
    diagnostics, the same seed the same result, and the guided samples closer to the query than the unguided ones on the same draws."""
    m = lightning_model()
    pdb = os.path.join(GOLDEN, 'g7_pocket.pdb')
    ids = [f'A:{i}' for i in range(1, 30)]
    spot = (9.0, 2.0, -15.0)
    query = [{'kind': 'position', 'point': 0, 'center': spot, 'radius': 1.5, 'k': 1.0},
             {'kind': 'distance', 'points': (0, 1), 'lo': 5.0, 'hi': 7.0, 'k': 1.0}]
    nph = torch.tensor([4, 7, 3])
    out, info = m.generate_phars_restrained(pdb, 3, query, pocket_ids=ids, num_nodes_phar=nph, clash=3.0, timesteps=50, seed=5)
    assert [len(s) for s in out] == [4, 7, 3] and tuple(info['energy'].shape) == tuple(info['max_violation'].shape) == (3,)
    names = set(m.dataset_info['phar_decoder'])
    assert all(name in names and len(xyz) == 3 for s in out for name, xyz in s)
    out2, info2 = m.generate_phars_restrained(pdb, 3, query, pocket_ids=ids, num_nodes_phar=nph, clash=3.0, timesteps=50, seed=5)
    assert out == out2 and torch.equal(info['energy'], info2['energy'])
    off, info0 = m.generate_phars_restrained(pdb, 3, query, pocket_ids=ids, num_nodes_phar=nph, clash=3.0, scale=0.0, timesteps=50, seed=5)
    dist = lambda samples: np.array([np.linalg.norm(np.asarray(s[0][1]) - np.asarray(spot)) for s in samples])
    print(f'\n[generate_phars_restrained] |point 0 - spot| (A): guided {dist(out)}, unguided {dist(off)}; energy {info["energy"].tolist()} '
          f'against {info0["energy"].tolist()}')
    assert float(info['energy'].sum()) < float(info0['energy'].sum())
    # the position term's violation is what the points' distances say, in the PDB's frame (the move back undoes the chain's shift)
    viol = np.maximum(dist(out) - 1.5, 0.0)
    maxv = info['max_violation'].cpu().numpy()                      # (an untrained model's points lie hundreds of A out: fp32 steps of ~1e-4 A)
    assert np.all(viol <= maxv * (1 + 1e-4) + 1e-2)
    scores = m.score_phars(pdb, out, pocket_ids=ids, timesteps=10, seed=3)
    assert tuple(scores['nll'].shape) == (3,)
    with pytest.raises(ValueError, match=r"restraints\[0\].*without 'sample'"):
        m.generate_phars_restrained(pdb, 3, [dict(query[0], sample=0)], pocket_ids=ids, num_nodes_phar=nph, timesteps=50)
    with pytest.raises(ValueError, match=r'restraints\[1\].*point 1'):
        m.generate_phars_restrained(pdb, 2, query, pocket_ids=ids, num_nodes_phar=torch.tensor([4, 1]), timesteps=50)
