"""GPU tests of ConditionalDDPM.sample_restrained_given_pockets / cmdgen_multi_restrained_chain: parity with multi_restraint_ref on injected
noise for a batch that mixes groups of 1, 2 and 3 members with every restraint kind and for a member above 128 nodes, the reductions to
cmdgen_multi_pocket_chain and to cmdgen_restrained_chain bit for bit, the members' copies of the latent, graphs against eager launches and
run to run, a group no record touches, the effect itself, the other engines, and refusals.

Bounds against the reference are test_hip_restraint.py's: per-op z and pocket <= 1e-4 max(1, max|.|), final x and pocket RMS
<= 1e-4 max(1, max|.|), types exact; energy, max_violation and op_energy within 1e-4 max(1, |want|).  A group with a pair within 1e-4 A of the
cutoff at any reference evaluation is left out (multi_restraint_cases.py: at most 20 % of a case's groups; none for the committed inputs)."""
import numpy as np
import pytest
import torch

import multi_restraint_cases as mrc
import chain_kit as kit
from chain_kit import (EINVAL, ESTATE, GUIDED, PLAIN, SMALL, check_against_ref, dev, guide, handle, model, pocket_dev, record, run_chain, same,
                       status_key)
from cmdgen_amd import hip_backend
from cmdgen_amd import restraints as rs
from cmdgen_amd.synthetic import ModelConfig, PocketBatch, make_state_dict, make_pockets

pytestmark = pytest.mark.gpu


def run_guided(h, pb, sizes, w, rec, K, noise=None, seed=7, ids=None, use_graph=True, **g):
    """cmdgen_multi_restrained_chain; g: guide()'s clash, scale, max_shift, guide_below"""
    return run_chain(h, pb, K, groups=(sizes, w), guide=guide(rec, **g), noise=noise, seed=seed, ids=ids, use_graph=use_graph)


def run_multi(h, pb, sizes, w, K, **kw):
    """cmdgen_multi_pocket_chain on the host's tables, as the guided chain it is compared with bit for bit"""
    return run_chain(h, pb, K, groups=(sizes, w), **kw)


# ------------------------------------------------------------------------------------------------ 1. / 5. against the reference
def check_case(case, engine, use_graph):
    r = mrc.reference(case)
    pb, gr, keep = r['pb'], r['groups'], r['keep']
    h = handle(engine)
    h.set_option('graph_steps', 2)                                   # K = 5: two replays of two steps, one eager step
    got, st = run_guided(h, pb, case.group_sizes, r['weights'], r['rec'], mrc.K, noise=r['noise'].cuda(), use_graph=use_graph)
    # test_hip_restraint.py's metric: the final x and pocket by their RMS, the pocket over its whole row; at most CHAIN_CAP of the groups left out
    check_against_ref(f'{case.name} {engine} {"graph" if use_graph else "eager"}', got, st, r['guided'], keep[gr.unique_mask.numpy()],
                      keep[gr.group_of][pb.mask], keep, 'groups', final='rms')
    return r


@pytest.mark.parametrize('use_graph', [True, False], ids=['graph', 'eager'])
@pytest.mark.parametrize('case', [mrc.MIXED, mrc.LARGE], ids=lambda c: c.name)
def test_chain_matches_the_reference(case, use_graph):
    r = check_case(case, 'half', use_graph)
    if case.big_member is not None:
        assert int((r['pb'].size + r['pb'].num_nodes_phar).max()) > 128           # the 1024-thread path ran


@pytest.mark.parametrize('engine', ['bf3', 'fp32'])
def test_other_engines_match_the_reference(engine):
    check_case(mrc.PAIRS, engine, True)


# ------------------------------------------------------------------------------------------------ 2. the reductions
@pytest.mark.parametrize('use_graph', [True, False], ids=['graph', 'eager'])
@pytest.mark.parametrize('inject', [False, True], ids=['device-draws', 'injected'])
def test_without_guidance_it_is_the_multi_pocket_chain_bit_for_bit(inject, use_graph):
    """No record and r_c = 0, scale = 0 with records and the clash term present, and guide_below = 0: xh_phar, xh_pocket, z_steps,
    pocket_steps and the chain status of cmdgen_multi_pocket_chain."""
    case, K = mrc.MIXED, 10
    r = mrc.reference(case)
    pb, w, gr = r['pb'], r['weights'], r['groups']
    h = handle()
    h.set_option('graph_steps', 8)
    ids = 300 + np.arange(gr.G)
    noise = dev(np.random.default_rng(6).normal(size=(K + 2, gr.Nu, 11)).astype(np.float32)) if inject else None
    kw = dict(noise=noise, seed=11, ids=ids, use_graph=use_graph)
    want, sw = run_multi(h, pb, case.group_sizes, w, K, **kw)
    none, s0 = run_guided(h, pb, case.group_sizes, w, None, K, clash=(0.0, 0.0), **kw)
    zero, s1 = run_guided(h, pb, case.group_sizes, w, r['rec'], K, scale=0.0, **kw)
    below, s2 = run_guided(h, pb, case.group_sizes, w, r['rec'], K, guide_below=0.0, **kw)
    for got in (none, zero, below):
        same(want, got, PLAIN)
    assert status_key(sw) == status_key(s0) == status_key(s1) == status_key(s2) and sw['nan_resets'] == 0
    assert not none[4].any() and not none[5].any()                      # nothing restrains: zero energies
    assert zero[4][:, 0].max() > 0 and zero[5].max() > 0                # scale = 0 still reports them
    assert np.array_equal(zero[4], below[4]) and np.array_equal(zero[5], below[5])
    guided, _ = run_guided(h, pb, case.group_sizes, w, r['rec'], K, **kw)
    assert not np.array_equal(guided[0], want[0])                       # ... and the guidance is not a no-op here


@pytest.mark.parametrize('use_graph', [True, False], ids=['graph', 'eager'])
@pytest.mark.parametrize('inject', [False, True], ids=['device-draws', 'injected'])
def test_groups_of_one_are_the_restrained_chain_bit_for_bit(inject, use_graph):
    """Every M_g = 1: cmdgen_restrained_chain's outputs on a handle whose evaluations use their own k_readout, energy_out and op_energy_out
    included, and the chain status."""
    K = 10
    h = handle(options=dict(SMALL, readout_in_coord=0))
    h.set_option('graph_steps', 8)
    pb = make_pockets(6, 'CA', ragged=True, first_index=9500)
    nph = 1 + (np.arange(6, dtype=np.int64) * 3) % 8
    pb = PocketBatch(x=pb.x, one_hot=pb.one_hot, size=pb.size, mask=pb.mask, num_nodes_phar=nph, pocket_index=pb.pocket_index)
    h.set_layout(pb.num_nodes_phar, pb.size)
    assert h.query('readout_in_coord') == 0
    noise = dev(np.random.default_rng(6).normal(size=(K + 2, int(nph.sum()), 11)).astype(np.float32)) if inject else None
    restraints = [{'kind': 'position', 'sample': 0, 'point': 0, 'center': (1.0, 0.0, -1.0), 'radius': 1.0, 'k': 1.0},
                  {'kind': 'distance', 'sample': 2, 'points': (0, 3), 'lo': 5.0, 'hi': 7.0, 'k': 1.0},
                  {'kind': 'exclusion', 'sample': 5, 'center': (0.0, 0.0, 0.0), 'radius': 4.0, 'k': 1.0}]
    rec = rs.records(restraints, nph)
    for clash in (mrc.CLASH, (0.0, 0.0)):                               # with the clash term every group is guided; without it three are
        want, sw = run_chain(h, pb, K, guide=guide(rec, clash=clash), noise=noise, seed=11, ids=pb.pocket_index, use_graph=use_graph)
        got, sg = run_guided(h, pb, [1] * 6, np.ones(6, np.float32), rec, K, clash=clash, noise=noise, seed=11, ids=pb.pocket_index,
                             use_graph=use_graph)
        same(want, got, GUIDED)
        assert status_key(sw) == status_key(sg) and sw['nan_resets'] == 0
        assert want[4][:, 0].max() > 0 and want[5].max() > 0


# ------------------------------------------------------------------------------------------------ 3. copies, graphs, run to run
def test_copies_stay_identical_and_runs_repeat_bit_for_bit():
    """Device draws on the mixed case.  After a guided run every member's copy of z equals its group's first; the captured chain twice and
    the eager one agree on every output; and with the clash term off, the group no record touches follows cmdgen_multi_pocket_chain through
    the first op."""
    case = mrc.MIXED
    r = mrc.reference(case)
    pb, w, gr = r['pb'], r['weights'], r['groups']
    h = handle()
    h.set_option('graph_steps', 2)
    a, sa = run_guided(h, pb, case.group_sizes, w, r['rec'], mrc.K, seed=31, use_graph=True)
    assert h.query('chain_graphs') >= 1
    z = h.debug_read('chain_z', gr.Nl * 11).reshape(gr.Nl, 11)
    first_rows = gr.first_rows().numpy()[gr.urow.numpy()]              # per member row: the same row of the group's first member
    assert gr.max_m == 3 and np.array_equal(z, z[first_rows])
    b, sb = run_guided(h, pb, case.group_sizes, w, r['rec'], mrc.K, seed=31, use_graph=True)
    e, se = run_guided(h, pb, case.group_sizes, w, r['rec'], mrc.K, seed=31, use_graph=False)
    same(a, b, GUIDED)
    same(a, e, GUIDED)
    assert status_key(sa) == status_key(sb) == status_key(se) and sa['nan_resets'] == 0
    # a changed scalar prepares the slot again; the first arguments give the first result back
    c, _ = run_guided(h, pb, case.group_sizes, w, r['rec'], mrc.K, clash=(mrc.CLASH[0], 2.0), seed=31, use_graph=True)
    assert not np.array_equal(a[0], c[0])
    back, _ = run_guided(h, pb, case.group_sizes, w, r['rec'], mrc.K, seed=31, use_graph=True)
    same(a, back, GUIDED)
    # the bare group: no record, r_c = 0
    g = case.bare_group
    rows, rows_q = gr.unique_mask.numpy() == g, gr.group_of[pb.mask] == g
    off, _ = run_guided(h, pb, case.group_sizes, w, r['rec'], mrc.K, clash=(0.0, 0.0), seed=31, use_graph=True)
    plain, _ = run_multi(h, pb, case.group_sizes, w, mrc.K, seed=31, use_graph=True)
    assert np.array_equal(off[2][0][rows], plain[2][0][rows]) and np.array_equal(off[3][0][rows_q], plain[3][0][rows_q])
    assert not np.array_equal(off[2][0][~rows], plain[2][0][~rows])     # ... while the others are steered
    assert off[4][g, 0] == 0 and not off[5][:, g].any()


# ------------------------------------------------------------------------------------------------ 4. the effect
def test_guidance_lowers_the_final_energy():
    case = mrc.PAIRS
    pb, w = mrc.member_pockets(case), mrc.weights_of(case)
    rec = rs.records(mrc.restraints_of(case, pb), case.nph)
    h = handle()
    g, _ = run_guided(h, pb, case.group_sizes, w, rec, mrc.K, seed=61)
    u, _ = run_guided(h, pb, case.group_sizes, w, rec, mrc.K, scale=0.0, seed=61)
    print(f'\n[effect] final energy per group unguided {u[4][:, 0]}\n         guided   {g[4][:, 0]}\n         largest violation (A) unguided '
          f'{u[4][:, 1]}\n         guided   {g[4][:, 1]}')
    assert float(g[4][:, 0].sum()) < float(u[4][:, 0].sum())


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_refusals_leave_the_handle_usable():
    cfg = ModelConfig(hidden_nf=64, n_layers=1, timesteps=500)
    pb = make_pockets(4, 'CA', ragged=True, first_index=9700)
    pb.num_nodes_phar[:] = (3, 3, 5, 5)
    px, poh = dev(pb.x), dev(pb.one_hot)
    h = hip_backend.Handle(cfg.as_dict(), 0)
    h.load_state_dict(make_state_dict(cfg, seed=0))
    h.set_layout(pb.num_nodes_phar, pb.size)
    half = np.full(4, 0.5, np.float32)

    refused = lambda h, match, rec=None, sizes=(2, 2), w=half, code=EINVAL, **kw: kit.refused(          # the message, and the code
        h, lambda: h.multi_restrained_chain(px, poh, list(sizes), w, 5, rec, **kw), match, code)

    # of a restraint list and the scalars: cmdgen_restrained_chain's refusals, saying "group"
    refused(h, "group 2 outside the call's 2 groups", record(sample=2))
    refused(h, "group -1 outside the call's 2 groups", record(sample=-1))
    refused(h, 'point 3, group 0 has 3 points', record(i=3))
    refused(h, 'point 5, group 1 has 5 points', record(kind=1, sample=1, i=0, j=5, a=1.0, b=2.0))
    refused(h, 'point 3, group 1 has 3 points', record(sample=1, i=3), sizes=(1, 1, 2), w=np.array([1, 1, 0.5, 0.5], np.float32))
    refused(h, 'i == j', record(kind=1, sample=1, i=2, j=2, a=1.0, b=2.0))
    refused(h, 'lo=3 > hi=2', record(kind=1, sample=1, i=0, j=1, a=3.0, b=2.0))
    refused(h, 'max_shift', record(), max_shift=0.0)
    refused(h, 'max_shift', record(), max_shift=-1.0)
    refused(h, 'unknown kind', record(kind=3))
    refused(h, 'scale', record(), scale=-1.0)
    refused(h, 'guide_below', record(), guide_below=1.5)
    refused(h, 'clash_radius', record(), clash_radius=-1.0)
    refused(h, 'group 1 has more than 256 restraints', np.concatenate([record(kind=2, sample=1)] * 257))
    # of a grouping: cmdgen_multi_pocket_chain's refusals
    refused(h, 'share one latent', record(), sizes=(1, 2, 1), w=np.array([1, 0.5, 0.5, 1], np.float32))          # members of 3 and 5 points
    refused(h, 'not 1', record(), w=np.array([0.5, 0.6, 0.5, 0.5], np.float32))
    refused(h, 'sum to 3', record(), sizes=(2, 1), w=np.array([0.5, 0.5, 1, 1], np.float32))
    refused(h, 'sizes must be in', record(), sizes=(2, 0, 2))
    good = h.multi_restrained_chain(px, poh, [2, 2], half, 5, record(), clash_radius=3.0, clash_k=1.0, seed=3)
    plain = h.multi_pocket_chain(px, poh, [2, 2], half, 5, seed=3)        # ... and an ordinary chain follows
    st = h.chain_status()
    assert good[0].shape == plain[0].shape == (8, 11) and good[3].shape == (2, 2) and st['max_rel_com_error'] < 1e-2
    assert all(bool(torch.isfinite(t).all()) for t in (good[0], good[3], plain[0]))
    h.close()
    jcfg = ModelConfig(hidden_nf=64, n_layers=1, update_pocket_coords=True)
    joint = hip_backend.Handle(jcfg.as_dict(), 0)
    joint.load_state_dict(make_state_dict(jcfg, seed=0))
    joint.set_layout(pb.num_nodes_phar, pb.size)
    refused(joint, 'restrained multi-pocket chain is not supported for the joint model', record(), code=ESTATE)
    assert joint.joint_chain(5, seed=3)[0].shape == (16, 11)
    joint.close()
    scfg = ModelConfig(hidden_nf=64, n_layers=1, timesteps=500, no_com_projection=True)
    simple = hip_backend.Handle(scfg.as_dict(), 0)
    simple.load_state_dict(make_state_dict(scfg, seed=0))
    simple.set_layout(pb.num_nodes_phar, pb.size)
    refused(simple, 'restrained multi-pocket chain is not supported for no_com_projection', record(), code=ESTATE)
    assert simple.sample_chain(px, poh, 5, seed=3)[0].shape == (16, 11)
    simple.close()


# ------------------------------------------------------------------------------------------------ the Python entry point
def test_sample_restrained_given_pockets_returns_the_chains_result():
    """ConditionalDDPM.sample_restrained_given_pockets on the pairs case: the chain's outputs (bit for bit the binding's, same tables and
    draws) split per pocket, the info dict, frames, and scale = 0 as sample_given_pockets."""
    case = mrc.PAIRS
    r = mrc.reference(case)
    pb, gr = r['pb'], r['groups']
    ddpm = model()
    ddpm.use_hip_graph = True
    pockets = [pocket_dev(pb, [2 * g + m for g in range(gr.G)]) for m in range(2)]
    w = r['weights'].reshape(gr.G, 2)
    noise = r['noise'].cuda()
    x, qs, pm, qms, info = ddpm.sample_restrained_given_pockets(pockets, case.nph, r['restraints'], weights=w, clash=mrc.CLASH, scale=mrc.SCALE,
                                                                max_shift=mrc.MAX_SHIFT, timesteps=mrc.K, noise=noise)
    want, _ = run_guided(ddpm.dynamics.hip_handle(), pb, case.group_sizes, r['weights'], r['rec'], mrc.K, noise=noise)
    assert np.array_equal(x.cpu().numpy(), want[0]) and len(qs) == 2 and pm.shape == (gr.Nu,)
    for m in range(2):
        assert np.array_equal(qs[m].cpu().numpy(), want[1][np.isin(pb.mask, [2 * g + m for g in range(gr.G)])])
    assert np.array_equal(info['energy'].cpu().numpy(), want[4][:, 0]) and np.array_equal(info['max_violation'].cpu().numpy(), want[4][:, 1])
    assert 'op_energy' not in info
    frames = ddpm.sample_restrained_given_pockets(pockets, case.nph, r['restraints'], weights=w, clash=mrc.CLASH, return_frames=mrc.K,
                                                  timesteps=mrc.K, noise=noise)
    assert frames[0].shape == (mrc.K, gr.Nu, 11) and frames[4]['op_energy'].shape == (mrc.K, gr.G) and torch.equal(frames[0][0], x)
    plain = ddpm.sample_given_pockets(pockets, case.nph, weights=w, timesteps=mrc.K, noise=noise)
    off = ddpm.sample_restrained_given_pockets(pockets, case.nph, r['restraints'], weights=w, clash=mrc.CLASH, scale=0.0, timesteps=mrc.K,
                                               noise=noise)
    assert torch.equal(off[0], plain[0]) and all(torch.equal(a, b) for a, b in zip(off[1], plain[1]))
