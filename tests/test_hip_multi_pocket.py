"""GPU tests of ConditionalDDPM.sample_given_pockets / cmdgen_multi_pocket_chain: the reduction to the single chain (groups of one
member; weights (1, 0, ...)), parity with multi_pocket_ref on injected noise for a batch that mixes groups of 1, 2 and 3 members and for
a member above 128 nodes, graphs against eager launches, run-to-run reproducibility, a group alone against the same group inside a
larger batch, the other engines, refusals, and PharPocketDDPM.generate_phars_multi.

Bounds against the reference are the chain tests' (test_hip_rule_sweep.py, test_hip_edit.py): per-step z <= 1e-4 max(1, |z|), pocket steps
<= 1e-4 max(1, |P|), final x RMS <= 1e-4 max(1, |x|), types exact; a group with a pair within 1e-4 A of the cutoff at any reference
evaluation is left out (multi_pocket_cases.py: at most 20 % of a case's groups; none for the committed inputs)."""
import os

import numpy as np
import pytest
import torch

import multi_pocket_cases as mc
import chain_kit as kit
from chain_kit import (PLAIN, check_against_ref, dev, handle, lightning_model, model, parity_ratios, philox_noise, pocket_dev, run_chain, same,
                       sub_batch, types_equal)
from helpers import GOLDEN
from cmdgen_amd import hip_backend
from cmdgen_amd.synthetic import ModelConfig, make_state_dict, make_pockets

pytestmark = pytest.mark.gpu


def run_multi(h, pb, sizes, weights, K, **kw):
    """cmdgen_multi_pocket_chain on the library's own step table (run_chain's docstring)"""
    return run_chain(h, pb, K, groups=(sizes, weights), tables=False, **kw)


def check_case(case, engine, use_graph):
    r = mc.reference(case)
    pb, gr, keep = r['pb'], r['groups'], r['keep']
    h = handle(engine)
    h.set_option('graph_steps', 2)                                   # K = 5: two replays of two steps, one eager step
    got, st = run_multi(h, pb, case.group_sizes, r['weights'], mc.K, noise=r['noise'].cuda(), use_graph=use_graph)
    want = dict(xh_phar=r['want'], xh_pocket=r['want_pocket'], z_steps=r['z_steps'], pocket_steps=r['pocket_steps'])
    # the final x and pocket by their RMS, the pocket over its whole row; at most 20 % (CHAIN_CAP) of the groups left out
    check_against_ref(f'{case.name} {engine} {"graph" if use_graph else "eager"}', got, st, want, keep[r['unique_mask']], keep[gr.group_of][pb.mask],
                      keep, 'groups', final='rms')


# ------------------------------------------------------------------------------------------------ 1. M = 1
@pytest.mark.parametrize('use_graph', [True, False], ids=['graph', 'eager'])
@pytest.mark.parametrize('inject', [False, True], ids=['device-draws', 'injected'])
@pytest.mark.parametrize('B', [1, 3, 20])
def test_groups_of_one_are_the_single_chain_bit_for_bit(B, inject, use_graph):
    """sample_given_pockets([pocket]) against sample_given_pocket(pocket): the final xh, every frame (z and the pocket after every
    step), and below it cmdgen_multi_pocket_chain against cmdgen_sample_chain in z_steps and pocket_steps."""
    K = 10
    ddpm = model()
    ddpm.use_hip_graph = use_graph
    pb = make_pockets(B, 'CA', ragged=True, first_index=9500)
    nph = 1 + (np.arange(B, dtype=np.int64) * 3) % 8
    ids = pb.pocket_index
    noise = dev(np.random.default_rng(B).normal(size=(K + 2, int(nph.sum()), 11)).astype(np.float32)) if inject else None
    pocket = pocket_dev(pb)
    a = ddpm.sample_given_pocket(pocket, nph, return_frames=K, timesteps=K, noise=noise, seed=11, pocket_ids=ids)
    b = ddpm.sample_given_pockets([pocket], nph, return_frames=K, timesteps=K, noise=noise, seed=11, group_ids=ids)
    assert a[0].shape == b[0].shape == (K, int(nph.sum()), 11) and len(b[1]) == 1 and len(b[3]) == 1
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1][0])
    assert torch.equal(a[2], b[2]) and torch.equal(a[3], b[3][0])
    h = ddpm.dynamics.hip_handle()
    h.set_layout(nph, pb.size)
    xa, qa, za = h.sample_chain(pocket['x'], pocket['one_hot'], K, noise=noise, seed=11, pocket_ids=ids, want_steps=True, use_graph=use_graph)
    pa = h.last_pocket_steps
    sa = h.chain_status()
    xb, qb, zb = h.multi_pocket_chain(pocket['x'], pocket['one_hot'], [1] * B, np.ones(B, np.float32), K, noise=noise, seed=11,
                                      group_ids=ids, want_steps=True, use_graph=use_graph)
    pb_steps = h.last_pocket_steps
    sb = h.chain_status()
    assert torch.equal(za, zb) and torch.equal(pa, pb_steps) and torch.equal(xa, xb) and torch.equal(qa, qb)
    assert sa['max_rel_com_error'] == sb['max_rel_com_error'] and sa['max_cog'] == sb['max_cog'] and sb['nan_resets'] == 0


# ------------------------------------------------------------------------------------------------ 2. weights (1, 0, ...)
@pytest.mark.parametrize('M', [2, 3])
def test_weights_one_zero_follow_the_first_pocket(M):
    """Weights (1, 0, ...) over M different pockets per group: the phar output is the single chain's on the first pockets, bit for
    bit, and the riding pockets come out translated by the same total shift as the first (within 1e-5 normalised units)."""
    K, G = 10, 2
    ddpm = model()
    ddpm.use_hip_graph = True
    pb = make_pockets(G * M, 'CA', ragged=True, first_index=9600 + 10 * M)
    nph = np.array([5, 8], dtype=np.int64)
    pockets = [pocket_dev(pb, [g * M + m for g in range(G)]) for m in range(M)]
    w = [1.0] + [0.0] * (M - 1)
    want = ddpm.sample_given_pocket(pockets[0], nph, timesteps=K, seed=21, pocket_ids=[40, 41])
    got = ddpm.sample_given_pockets(pockets, nph, weights=w, timesteps=K, seed=21, group_ids=[40, 41])
    nv = mc.config().norm_values[0]
    moves = []
    for m in range(M):
        d = (got[1][m][:, :3].double() - pockets[m]['x'].double()) / nv
        mask = pockets[m]['mask']
        moves.append(torch.stack([d[mask == g].mean(0) for g in range(G)]))
    spread = max(float((mv - moves[0]).abs().max()) for mv in moves)
    diff = float((got[0] - want[0]).abs().max())
    print(f'\n[M = {M}] phar output against the single chain: max abs difference {diff:.3e}; shift spread between the pockets {spread:.2e}')
    assert spread <= 1e-5
    assert torch.equal(got[0], want[0])
    assert torch.equal(got[1][0], want[1])


# ------------------------------------------------------------------------------------------------ 3. against the reference
@pytest.mark.parametrize('use_graph', [True, False], ids=['graph', 'eager'])
@pytest.mark.parametrize('case', [mc.MIXED, mc.LARGE], ids=lambda c: c.name)
def test_mixed_batch_matches_the_reference(case, use_graph):
    check_case(case, 'half', use_graph)
    if case.big_member is not None:
        assert max(mc.reference(case)['pb'].size + mc.reference(case)['pb'].num_nodes_phar) > 128      # the 1024-thread step ran


# ------------------------------------------------------------------------------------------------ 4. / 5. graphs, run to run
def test_captured_equals_eager_and_repeats_bit_for_bit():
    """An M = 2 batch with device draws: the captured chain twice (run to run) and the eager one, every output bit for bit."""
    case = mc.PAIRS
    pb, w = mc.member_pockets(case), mc.weights_of(case)
    h = handle('half')
    h.set_option('graph_steps', 2)
    a, sa = run_multi(h, pb, case.group_sizes, w, mc.K, seed=31, use_graph=True)
    assert h.query('chain_graphs') >= 1
    b, sb = run_multi(h, pb, case.group_sizes, w, mc.K, seed=31, use_graph=True)
    c, sc = run_multi(h, pb, case.group_sizes, w, mc.K, seed=31, use_graph=False)
    same(a, b, PLAIN)
    same(a, c, PLAIN)
    assert sa['max_rel_com_error'] == sb['max_rel_com_error'] == sc['max_rel_com_error'] and sa['nan_resets'] == 0
    # another seed replays the graph with other numbers; a changed weight prepares the chain again
    d, _ = run_multi(h, pb, case.group_sizes, w, mc.K, seed=32, use_graph=True)
    assert not np.array_equal(a[0], d[0])
    w2 = w.copy(); w2[:2] = (0.5, 0.5)
    e2, _ = run_multi(h, pb, case.group_sizes, w2, mc.K, seed=31, use_graph=True)
    f2, _ = run_multi(h, pb, case.group_sizes, w2, mc.K, seed=31, use_graph=False)
    assert np.array_equal(e2[0], f2[0]) and not np.array_equal(e2[0][:case.nph[0]], a[0][:case.nph[0]])


# ------------------------------------------------------------------------------------------------ 6. a group alone / in a batch
def test_a_group_alone_and_inside_a_larger_batch():
    """Group 2 of the mixed case (three members, eight points) alone and as part of the batch of ten groups, same group id, device
    draws.  In both layouts the device draws are cmdgen_debug_noise's numbers for (seed, group id, draw, node) - the chain run on
    them as injected noise is the device-draw chain bit for bit - so the two runs draw alike; their results agree within the bounds
    of the reference comparison (not bit for bit: the tile rule differs with the batch size)."""
    case = mc.MIXED
    pb, w = mc.member_pockets(case), mc.weights_of(case)
    K, seed, g = mc.K, 41, 2
    gids = 700 + np.arange(len(case.group_sizes))
    first = int(np.sum(case.group_sizes[:g])); members = list(range(first, first + case.group_sizes[g]))
    h = handle('half')
    full, st = run_multi(h, pb, case.group_sizes, w, K, seed=seed, ids=gids)
    draws = range(K + 2)                                               # the plain chain's counters: z_T, one per op, the decode
    full_inj, _ = run_multi(h, pb, case.group_sizes, w, K, noise=philox_noise(h, seed, gids, case.nph, draws), ids=gids)
    same(full, full_inj, PLAIN)
    sub = sub_batch(pb, members)
    alone, st2 = run_multi(h, sub, [len(members)], w[members], K, seed=seed, ids=gids[g:g + 1])
    alone_inj, _ = run_multi(h, sub, [len(members)], w[members], K, noise=philox_noise(h, seed, gids[g:g + 1], case.nph[g:g + 1], draws),
                             ids=gids[g:g + 1])
    same(alone, alone_inj, PLAIN)
    u0 = int(np.sum(case.nph[:g])); rows = slice(u0, u0 + case.nph[g])
    rows_q = np.isin(pb.mask, members)
    part = dict(xh_phar=full[0][rows], xh_pocket=full[1][rows_q], z_steps=full[2][:, rows], pocket_steps=full[3][:, rows_q])
    all_rows, all_q = np.ones(case.nph[g], bool), np.ones(int(sub.size.sum()), bool)
    ratios = parity_ratios(alone, part, all_rows, all_q, final='rms')      # the reference comparison's bounds
    print('\n[group alone against the batch] worst ratio to each bound: ' + '  '.join(f'{k} {v:.3f}' for k, v in ratios.items()))
    assert all(v <= 1.0 for v in ratios.values()), ratios
    assert types_equal(alone, part, all_rows) and st['nan_resets'] == 0 and st2['nan_resets'] == 0


# ------------------------------------------------------------------------------------------------ 7. the other engines
@pytest.mark.parametrize('engine', ['bf3', 'fp32'])
def test_other_engines_match_the_reference(engine):
    check_case(mc.PAIRS, engine, True)


# ------------------------------------------------------------------------------------------------ 8. refusals
def test_refusals_leave_the_handle_usable():
    cfg = ModelConfig(hidden_nf=64, n_layers=1, timesteps=500)
    pb = make_pockets(4, 'CA', ragged=True, first_index=9700)
    pb.num_nodes_phar[:] = (3, 3, 5, 5)
    px, poh = dev(pb.x), dev(pb.one_hot)
    h = hip_backend.Handle(cfg.as_dict(), 0)
    h.load_state_dict(make_state_dict(cfg, seed=0))
    h.set_layout(pb.num_nodes_phar, pb.size)
    half = np.full(4, 0.5, np.float32)

    refused = lambda match, sizes, w: kit.refused(h, lambda: h.multi_pocket_chain(px, poh, sizes, w, 5), match, code=None)     # the message

    refused('share one latent', [1, 2, 1], np.array([1, 0.5, 0.5, 1], np.float32))          # members 1 and 2 have 3 and 5 points
    refused('sum to 3', [2, 1], np.array([0.5, 0.5, 1, 1], np.float32))
    refused('sum to 5', [2, 3], np.array([0.5, 0.5, 1, 0, 0], np.float32)[:4])
    refused('sizes must be in', [2, 0, 2], half)
    refused('sizes must be in', [9], half)
    refused('not 1', [2, 2], np.array([0.5, 0.6, 0.5, 0.5], np.float32))
    refused('finite and >= 0', [2, 2], np.array([1.5, -0.5, 0.5, 0.5], np.float32))
    refused('finite and >= 0', [2, 2], np.array([np.nan, 0.5, 0.5, 0.5], np.float32))
    good = h.multi_pocket_chain(px, poh, [2, 2], half, 5, seed=3)
    plain = h.sample_chain(px, poh, 5, seed=3)                        # ... and an ordinary chain follows
    st = h.chain_status()
    assert good[0].shape == (8, 11) and plain[0].shape == (16, 11) and st['max_rel_com_error'] < 1e-2
    assert bool(torch.isfinite(good[0]).all()) and bool(torch.isfinite(plain[0]).all())
    h.close()
    jcfg = ModelConfig(hidden_nf=64, n_layers=1, update_pocket_coords=True)
    joint = hip_backend.Handle(jcfg.as_dict(), 0)
    joint.load_state_dict(make_state_dict(jcfg, seed=0))
    joint.set_layout(pb.num_nodes_phar, pb.size)
    with pytest.raises(hip_backend.CmdgenError, match='joint model'):
        joint.multi_pocket_chain(px, poh, [2, 2], half, 5)
    assert joint.joint_chain(5, seed=3)[0].shape == (16, 11)
    joint.close()
    scfg = ModelConfig(hidden_nf=64, n_layers=1, timesteps=500, no_com_projection=True)
    simple = hip_backend.Handle(scfg.as_dict(), 0)
    simple.load_state_dict(make_state_dict(scfg, seed=0))
    simple.set_layout(pb.num_nodes_phar, pb.size)
    with pytest.raises(hip_backend.CmdgenError, match='no_com_projection'):
        simple.multi_pocket_chain(px, poh, [2, 2], half, 5)
    assert simple.sample_chain(px, poh, 5, seed=3)[0].shape == (16, 11)
    simple.close()


# ------------------------------------------------------------------------------------------------ 9. generate_phars_multi
def test_generate_phars_multi_with_weights_one_zero_is_generate_phars():
    """The synthetic PDB given twice, weights (1, 0), the same seed and sizes: the dict of generate_phars."""
    m = lightning_model()
    pdb = os.path.join(GOLDEN, 'g7_pocket.pdb')
    ids = [f'A:{i}' for i in range(1, 30)]
    nph = torch.tensor([4, 7, 3])
    want = m.generate_phars(pdb, 3, pocket_ids=ids, num_nodes_phar=nph, timesteps=20, seed=5)
    got = m.generate_phars_multi([pdb, pdb], 3, pocket_ids=[ids, ids], num_nodes_phar=nph, weights=[1.0, 0.0], timesteps=20, seed=5)
    assert sorted(got) == sorted(want)
    worst = 0.0
    for mol in want:
        assert sorted(got[mol]) == sorted(want[mol])
        for name in want[mol]:
            assert len(got[mol][name]) == len(want[mol][name])
            worst = max([worst] + [float((a - b).abs().max()) for a, b in zip(got[mol][name], want[mol][name])])
    print(f'\n[generate_phars_multi] largest coordinate difference to generate_phars {worst:.3e} A')
    assert all(torch.equal(a, b) for mol in want for name in want[mol] for a, b in zip(got[mol][name], want[mol][name]))
    uniform = m.generate_phars_multi([pdb, pdb], 3, pocket_ids=[ids, ids], num_nodes_phar=nph, timesteps=20, seed=5)
    assert sorted(uniform) == sorted(want)
