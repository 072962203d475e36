"""GPU tests of ConditionalDDPM.edit_given_pockets / cmdgen_multi_edit_chain: the two reductions bit for bit (groups of one member are
cmdgen_edit_chain; nothing held from the prior at (1, 1) is cmdgen_multi_pocket_chain), parity with multi_edit_ref on injected noise for
a batch that mixes groups of 1, 2 and 3 members and every kind of mark and for a member above 128 nodes, the members' copies of the
latent, graphs against eager launches while start, seed, grouping and weights change, held types and coordinates, refusals, and
PharPocketDDPM.edit_phars_multi.

Bounds against the reference are the chain tests' (test_hip_multi_pocket.py, test_hip_edit.py): per-op z <= 1e-4 max(1, |z|), pocket steps
<= 1e-4 max(1, |P|), final x RMS <= 1e-4 max(1, |x|), types exact; a group with a pair within 1e-4 A of the cutoff at any reference
evaluation is left out (multi_edit_cases.py: at most 20 % of a case's groups; none for the committed inputs).  Held coordinates:
test_hip_edit.py's 0.1 A.

Measured on an MI355X (worst ratio to each bound: per-op z / pocket steps / final x RMS / final pocket RMS; no group left out):
  mixed from the prior at (2, 2), half, graph and eager   0.003 / 0.002 / 0.001 / 0.000
  mixed part-way from start 3, graph and eager            0.002 / 0.001 / 0.001 / 0.000
  large member, graph and eager                           0.004 / 0.001 / 0.001 / 0.000
  mixed on the bf3 and fp32 engines                       0.003 / 0.002 / 0.001 / 0.000
  a group alone against the batch                         0.001 / 0.000 / 0.000 / 0.000 (not bit for bit)
  held rows, K = 100: coordinates within 0.0062 A of the given points (bound 0.1 A); edit_phars_multi 0.0093 A"""
import os

import numpy as np
import pytest
import torch

import multi_edit_cases as mec
import multi_pocket_cases as mc
from helpers import GOLDEN
from oracle import ref_cpu
from cmdgen_amd import hip_backend
from cmdgen_amd.synthetic import ModelConfig, make_state_dict, make_pockets
import chain_kit as kit
from chain_kit import (PLAIN, check_against_ref, dev, given_for, handle, handle_for, lightning_model, model, parity_ratios, philox_noise, pocket_dev,
                       run_chain, same, status_key, sub_batch, types_equal)

pytestmark = pytest.mark.gpu


# every chain here runs on the library's own step table (run_chain's docstring)
def run_medit(h, pb, sizes, weights, given, K, start=None, r=1, j=1, **kw):
    """given = (phar_x, phar_one_hot, fix_x, fix_h) over the unique rows"""
    return run_chain(h, pb, K, groups=(sizes, weights), given=given, plan=(start, r, j), tables=False, **kw)


# ------------------------------------------------------------------------------------------------ 1. M = 1
@pytest.mark.parametrize('use_graph', [True, False], ids=['graph', 'eager'])
@pytest.mark.parametrize('inject', [False, True], ids=['device-draws', 'injected'])
@pytest.mark.parametrize('B', [1, 3])
def test_groups_of_one_are_the_edit_chain_bit_for_bit(B, inject, use_graph):
    """cmdgen_multi_edit_chain with every M_g = 1 against cmdgen_edit_chain: the final xh, z and the pocket after every op and the
    chain status, from the prior without and with jumps and part-way."""
    h = handle('half')
    h.set_option('graph_steps', 2)
    pb = make_pockets(B, 'CA', ragged=True, first_index=9500)
    pb.num_nodes_phar[:] = 1 + (np.arange(B, dtype=np.int64) * 3) % 8
    nu = int(pb.num_nodes_phar.sum())
    given = given_for(pb.num_nodes_phar, B)
    ids = pb.pocket_index
    for K, start, r, j in ((6, 6, 1, 1), (6, 6, 2, 2), (6, 3, 1, 1)):
        h.set_layout(pb.num_nodes_phar, pb.size)
        n_draws = h.edit_plan(K, start, r, j)[1]
        noise = dev(np.random.default_rng(10 * B + start).normal(size=(n_draws, nu, 11)).astype(np.float32)) if inject else None
        a, sa = run_chain(h, pb, K, given=given, plan=(start, r, j), noise=noise, seed=11, ids=ids, use_graph=use_graph, tables=False)
        b, sb = run_medit(h, pb, [1] * B, np.ones(B, np.float32), given, K, start, r, j, noise=noise, seed=11, ids=ids, use_graph=use_graph)
        same(a, b, PLAIN)
        assert status_key(sa) == status_key(sb) and sb['nan_resets'] == 0 and sb['max_rel_com_error'] < 1e-2


# ------------------------------------------------------------------------------------------------ 2. nothing held
@pytest.mark.parametrize('use_graph', [True, False], ids=['graph', 'eager'])
@pytest.mark.parametrize('inject', [False, True], ids=['device-draws', 'injected'])
def test_no_marks_from_the_prior_are_the_multi_pocket_chain_bit_for_bit(inject, use_graph):
    """No mark, start = timesteps, (1, 1) on multi_pocket_cases.PAIRS' inputs against cmdgen_multi_pocket_chain.  Injected: the edit plan
    draws A and B per op, so the multi-pocket chain's K + 2 rows sit in rows 0, 1, 3, 5, .. and the last of the edit chain's noise."""
    case = mc.PAIRS
    pb, w = mc.member_pockets(case), mc.weights_of(case)
    h = handle('half')
    h.set_option('graph_steps', 2)
    K, nu = mc.K, int(sum(case.nph))
    x, oh, _, _ = given_for(np.asarray(case.nph), 3)
    zero = np.zeros(nu, np.float32)
    noise = spread = None
    if inject:
        noise = mc.noise_of(case).numpy()
        n_draws = 2 + 2 * K
        spread = np.random.default_rng(6).normal(size=(n_draws, nu, 11)).astype(np.float32)
        spread[[0] + [1 + 2 * i for i in range(K)] + [n_draws - 1]] = noise
        noise, spread = dev(noise), dev(spread)
    a, sa = run_chain(h, pb, K, groups=(case.group_sizes, w), noise=noise, seed=31, use_graph=use_graph, tables=False)
    b, sb = run_medit(h, pb, case.group_sizes, w, (x, oh, zero, zero), K, noise=spread, seed=31, use_graph=use_graph)
    same(a, b, PLAIN)
    assert status_key(sa) == status_key(sb) and sb['nan_resets'] == 0


# ------------------------------------------------------------------------------------------------ 3. against the reference
def check_run(run, engine, use_graph):
    r = mec.reference(run)
    case = mec.CASES[run.case]
    pb, gr, keep = r['pb'], r['groups'], r['keep']
    h = handle(engine)
    h.set_option('graph_steps', 2)
    got, st = run_medit(h, pb, case.group_sizes, r['weights'], mec.given_rows(case), mec.K, run.start, run.r, run.j, noise=r['noise'].cuda(),
                        use_graph=use_graph)
    want = dict(xh_phar=r['want'], xh_pocket=r['want_pocket'], z_steps=r['z_steps'], pocket_steps=r['pocket_steps'])
    # test_hip_multi_pocket.py's metric: the final x and pocket by their RMS, the pocket over its whole row; at most 20 % of the groups left out
    check_against_ref(f'{mec.run_id(run)} {engine} {"graph" if use_graph else "eager"}', got, st, want, keep[r['unique_mask']],
                      keep[gr.group_of][pb.mask], keep, 'groups', final='rms')


@pytest.mark.parametrize('use_graph', [True, False], ids=['graph', 'eager'])
@pytest.mark.parametrize('run', mec.RUNS, ids=mec.run_id)
def test_matches_the_reference(run, use_graph):
    check_run(run, 'half', use_graph)
    if run.case == 'large':
        pb = mec.reference(run)['pb']
        assert max(pb.size + pb.num_nodes_phar) > 128                      # the 1024-thread step ran


@pytest.mark.parametrize('engine', ['bf3', 'fp32'])
def test_other_engines_match_the_reference(engine):
    check_run(mec.RUNS[0], engine, True)


# ------------------------------------------------------------------------------------------------ 4. the copies of z
@pytest.mark.parametrize('run', mec.RUNS[:2], ids=mec.run_id)
def test_every_members_copy_of_the_latent_is_the_first_members(run):
    """After a chain with marks (every kind, with jumps; from the prior and part-way) every member's copy of z in the chain buffer
    equals the copy of its group's first member bit for bit (debug read "chain_z": the buffer as the decode left it)."""
    case = mec.CASES[run.case]
    pb, w = mc.member_pockets(case), mc.weights_of(case)
    h = handle('half')
    run_medit(h, pb, case.group_sizes, w, mec.given_rows(case), mec.K, run.start, run.r, run.j, seed=41)
    nl = int(pb.num_nodes_phar.sum())
    z = h.debug_read('chain_z', nl * 11).reshape(nl, 11)
    assert np.isfinite(z).all() and np.abs(z).max() > 0
    base = np.concatenate([[0], np.cumsum(pb.num_nodes_phar)])
    b = 0
    for g, m in enumerate(case.group_sizes):
        first = z[base[b]:base[b + 1]]
        for k in range(1, m):
            assert np.array_equal(z[base[b + k]:base[b + k + 1]], first), (g, k)
        b += m


def _edit_draws(start, r, j):
    """The draw counters of an edit chain in its call order (philox_noise then gives [n_draws, Nu, 11]): draw 0: 0, A of op i: 1 + i,
    decode: 1 + n_steps, B of op i: 2 + n_steps + i, C of op i: 2 + 2 n_steps + i."""
    sched = ref_cpu.get_repaint_schedule(r, j, start)
    n_steps = sum(sched)
    counters, op = [0], 0
    for i, n in enumerate(sched):
        for k in range(n):
            counters += [1 + op, 2 + n_steps + op]
            if k == n - 1 and i < len(sched) - 1:
                counters.append(2 + 2 * n_steps + op)
            op += 1
    counters.append(1 + n_steps)
    return counters


def test_a_group_alone_and_inside_a_larger_batch():
    """Group 2 of the mixed case (three members, eight points, every kind of mark) alone and as part of the batch of six groups, same
    group id, device draws, with jumps.  In both layouts the device draws are cmdgen_debug_noise's numbers for (seed, group id,
    counter, node of the group) - the chain run on them as injected noise is the device-draw chain bit for bit - so the two runs draw
    alike.  Their results agree within the bounds of the reference comparison; bit for bit only where the evaluation's tile rule is
    the same for both batch sizes, which the parents do not promise (test_hip_multi_pocket.py; test_hip_edit.py's docstring names the
    fp32 engine's 16-row tiles as the exception even for one layout) - the outcome is printed."""
    case = mec.MIXED
    pb, w = mc.member_pockets(case), mc.weights_of(case)
    given = mec.given_rows(case)
    K, start, r, j, seed, g = mec.K, 6, 2, 2, 43, 2
    gids = 700 + np.arange(len(case.group_sizes))
    first = int(np.sum(case.group_sizes[:g])); members = list(range(first, first + case.group_sizes[g]))
    h = handle('half')
    full, st = run_medit(h, pb, case.group_sizes, w, given, K, start, r, j, seed=seed, ids=gids)
    draws = _edit_draws(start, r, j)
    full_inj, _ = run_medit(h, pb, case.group_sizes, w, given, K, start, r, j, noise=philox_noise(h, seed, gids, case.nph, draws), ids=gids)
    same(full, full_inj, PLAIN)
    sub = sub_batch(pb, members)
    u0 = int(np.sum(case.nph[:g])); rows = slice(u0, u0 + case.nph[g])
    sub_given = [a[rows] for a in given]
    alone, st2 = run_medit(h, sub, [len(members)], w[members], sub_given, K, start, r, j, seed=seed, ids=gids[g:g + 1])
    alone_inj, _ = run_medit(h, sub, [len(members)], w[members], sub_given, K, start, r, j,
                             noise=philox_noise(h, seed, gids[g:g + 1], case.nph[g:g + 1], draws), ids=gids[g:g + 1])
    same(alone, alone_inj, PLAIN)
    rows_q = np.isin(pb.mask, members)
    part = dict(xh_phar=full[0][rows], xh_pocket=full[1][rows_q], z_steps=full[2][:, rows], pocket_steps=full[3][:, rows_q])
    all_rows, all_q = np.ones(case.nph[g], bool), np.ones(int(sub.size.sum()), bool)
    ratios = parity_ratios(alone, part, all_rows, all_q, final='rms')      # the reference comparison's bounds
    print('\n[group alone against the batch] worst ratio to each bound: ' + '  '.join(f'{k} {v:.3f}' for k, v in ratios.items()) +
          f'  bit for bit: {all(np.array_equal(u, part[k]) for u, k in zip(alone, PLAIN))}')
    assert all(v <= 1.0 for v in ratios.values()), ratios
    assert types_equal(alone, part, all_rows) and st['nan_resets'] == 0 and st2['nan_resets'] == 0


# ------------------------------------------------------------------------------------------------ 5. graphs, run to run
def test_captured_equals_eager_and_no_stale_graph_is_replayed():
    """Device draws: the captured chain twice (run to run) and the eager one, every output bit for bit; then start, seed, grouping and
    a weight change one at a time after a captured run, and every captured result is its own eager run's."""
    case = mc.PAIRS
    pb, w = mc.member_pockets(case), mc.weights_of(case)
    given = given_for(np.asarray(case.nph), 5)
    h = handle('half')
    h.set_option('graph_steps', 2)
    K = mec.K

    def both(sizes, weights, given, pb=pb, **kw):
        a, sa = run_medit(h, pb, sizes, weights, given, K, use_graph=True, **kw)
        b, sb = run_medit(h, pb, sizes, weights, given, K, use_graph=False, **kw)
        same(a, b, PLAIN)
        assert status_key(sa) == status_key(sb) and sa['nan_resets'] == 0
        return a

    base = both(case.group_sizes, w, given, start=6, r=2, j=2, seed=31)
    assert h.query('chain_graphs') >= 1
    again, _ = run_medit(h, pb, case.group_sizes, w, given, K, 6, 2, 2, seed=31, use_graph=True)
    same(base, again, PLAIN)
    other_start = both(case.group_sizes, w, given, start=3, r=2, j=2, seed=31)
    assert other_start[2].shape != base[2].shape
    other_seed = both(case.group_sizes, w, given, start=6, r=2, j=2, seed=32)
    assert not np.array_equal(other_seed[0], base[0])
    w2 = w.copy(); w2[:2] = (0.5, 0.5)
    other_w = both(case.group_sizes, w2, given, start=6, r=2, j=2, seed=31)
    assert not np.array_equal(other_w[0][:case.nph[0]], base[0][:case.nph[0]])
    # another grouping of the same six members: groups of one (every member its own latent; six copies of the rows)
    nph1 = pb.num_nodes_phar
    given1 = given_for(nph1, 6)
    singles = both([1] * len(nph1), np.ones(len(nph1), np.float32), given1, start=6, r=2, j=2, seed=31)
    assert singles[0].shape[0] == int(nph1.sum())
    back = both(case.group_sizes, w, given, start=6, r=2, j=2, seed=31)
    same(base, back, PLAIN)


# ------------------------------------------------------------------------------------------------ 6. held rows
def test_held_types_and_coordinates():
    """test_multi_edit_cpu.py's held-rows case on the device: the same inputs, K = 100, the same bound."""
    hc = mec.hold_case()
    cfg = mec.hold_config()
    h = handle_for(cfg, 'seed0', make_state_dict(cfg, seed=0))
    given = (hc['phar_x'], hc['phar_oh'], hc['coords_only'], hc['types_only'])
    (xh_phar, xh_pocket, *_), st = run_medit(h, hc['pb'], hc['sizes'], hc['weights'], given, mec.HOLD_K, seed=hc['seed'])
    assert st['max_rel_com_error'] < 1e-2 and st['nan_resets'] == 0
    err = mec.held_errors(hc, xh_phar, xh_pocket)
    print(f'\n[held rows, device] coords-only max err {err[hc["coords_only"]].max():.4f} A (bound {mec.HOLD_BOUND}); '
          f'types-only max err {err[hc["types_only"]].max():.3f} A')
    assert np.array_equal(xh_phar[hc['types_only'], 3:], hc['phar_oh'][hc['types_only']])
    assert err[hc['coords_only']].max() < mec.HOLD_BOUND


# ------------------------------------------------------------------------------------------------ 7. refusals
def test_refusals_leave_the_handle_usable():
    cfg = ModelConfig(hidden_nf=64, n_layers=1, timesteps=500)
    pb = make_pockets(4, 'CA', ragged=True, first_index=9700)
    pb.num_nodes_phar[:] = (3, 3, 5, 5)
    px, poh = dev(pb.x), dev(pb.one_hot)
    h = hip_backend.Handle(cfg.as_dict(), 0)
    h.load_state_dict(make_state_dict(cfg, seed=0))
    h.set_layout(pb.num_nodes_phar, pb.size)
    half = np.full(4, 0.5, np.float32)

    def args(nu):
        x, oh, fx, fh = given_for(np.array([nu]), 1)
        return [dev(a) for a in (x, oh, fx, fh)]

    refused = lambda match, sizes, w, nu=8, K=5, **kw: kit.refused(                    # the message
        h, lambda: h.multi_edit_chain(px, poh, sizes, w, *args(nu), K, **kw), match, code=None)

    refused('share one latent', [1, 2, 1], np.array([1, 0.5, 0.5, 1], np.float32), nu=11)     # members 1 and 2 have 3 and 5 points
    refused('sum to 3', [2, 1], np.array([0.5, 0.5, 1, 1], np.float32), nu=8)
    refused('sizes must be in', [2, 0, 2], half, nu=13)
    refused('sizes must be in', [9], half, nu=3)
    refused('not 1', [2, 2], np.array([0.5, 0.6, 0.5, 0.5], np.float32))
    refused('finite and >= 0', [2, 2], np.array([1.5, -0.5, 0.5, 0.5], np.float32))
    refused('finite and >= 0', [2, 2], np.array([np.nan, 0.5, 0.5, 0.5], np.float32))
    refused('finite and >= 0', [2, 2], np.array([np.inf, 0.5, 0.5, 0.5], np.float32))
    for bad in (0, 6, -3):
        with pytest.raises(hip_backend.CmdgenError, match='start'):
            _raw_call(h, px, poh, [2, 2], half, args(8), 5, start=bad)
    n_steps, n_draws = h.edit_plan(10, 6, 2, 1)
    short = torch.zeros((n_draws - 1, 8, 11), device='cuda')
    refused('draws', [2, 2], half, K=10, start=6, resamplings=2, noise=short)
    good = h.multi_edit_chain(px, poh, [2, 2], half, *args(8), 5, start=3, seed=3)
    plain = h.sample_chain(px, poh, 5, seed=3)                        # ... and an ordinary chain follows
    st = h.chain_status()
    assert good[0].shape == (8, 11) and plain[0].shape == (16, 11) and st['max_rel_com_error'] < 1e-2
    assert bool(torch.isfinite(good[0]).all()) and bool(torch.isfinite(plain[0]).all())
    # a sample above the step's 64 KiB of LDS (64 bytes per node: positions, degrees, z)
    big = np.array([1100, 30], dtype=np.int64)
    h.set_layout(np.array([3, 3], dtype=np.int64), big)
    with pytest.raises(hip_backend.CmdgenError, match='64 KiB'):
        h.multi_edit_chain(torch.zeros((1130, 3), device='cuda'), torch.zeros((1130, 20), device='cuda'), [2], half[:2], *args(3), 5)
    h.close()
    jcfg = ModelConfig(hidden_nf=64, n_layers=1, update_pocket_coords=True)
    joint = hip_backend.Handle(jcfg.as_dict(), 0)
    joint.load_state_dict(make_state_dict(jcfg, seed=0))
    joint.set_layout(pb.num_nodes_phar, pb.size)
    with pytest.raises(hip_backend.CmdgenError, match='joint model'):
        _raw_call(joint, px, poh, [2, 2], half, args(8), 5)
    assert joint.joint_chain(5, seed=3)[0].shape == (16, 11)
    joint.close()
    scfg = ModelConfig(hidden_nf=64, n_layers=1, timesteps=500, no_com_projection=True)
    simple = hip_backend.Handle(scfg.as_dict(), 0)
    simple.load_state_dict(make_state_dict(scfg, seed=0))
    simple.set_layout(pb.num_nodes_phar, pb.size)
    with pytest.raises(hip_backend.CmdgenError, match='no_com_projection'):
        _raw_call(simple, px, poh, [2, 2], half, args(8), 5)
    assert simple.sample_chain(px, poh, 5, seed=3)[0].shape == (16, 11)
    simple.close()


def _raw_call(h, px, poh, sizes, w, given, K, start=None):
    """The C entry itself (Handle.multi_edit_chain asks cmdgen_edit_plan first, which refuses the same things with its own message)."""
    import ctypes as C
    sizes = np.ascontiguousarray(np.asarray(sizes, dtype=np.int64))
    w = np.ascontiguousarray(np.asarray(w, dtype=np.float32))
    out_p = torch.empty((8, 11), device='cuda'); out_q = torch.empty((px.shape[0], 23), device='cuda')
    ptr = lambda t: C.c_void_p(t.data_ptr())
    h._check(h.lib.cmdgen_multi_edit_chain(h.h, ptr(px), ptr(poh), len(sizes), sizes.ctypes.data_as(C.POINTER(C.c_int64)),
                                           w.ctypes.data_as(C.c_void_p), *[ptr(a) for a in given], K, K if start is None else start, 1, 1, C.c_void_p(0), 0,
                                           C.c_uint64(0), None, ptr(out_p), ptr(out_q), C.c_void_p(0), C.c_void_p(0), 1, h._stream()),
             'cmdgen_multi_edit_chain')


# ------------------------------------------------------------------------------------------------ 8. end to end
def test_edit_given_pockets_returns_the_chains_result():
    """ConditionalDDPM.edit_given_pockets (bool masks of shape [Nu, 1], weights per pocket) against the raw chain on the same seed."""
    K, G, M = 6, 2, 2
    ddpm = model()
    ddpm.use_hip_graph = True
    pb = make_pockets(G * M, 'CA', ragged=True, first_index=9620)
    nph = np.array([5, 8], dtype=np.int64)
    pb.num_nodes_phar[:] = np.repeat(nph, M)
    x, oh, fx, fh = given_for(nph, 9)
    pockets = [pocket_dev(pb, [g * M + m for g in range(G)]) for m in range(M)]
    phar = {'x': dev(x), 'one_hot': dev(oh), 'size': dev(nph), 'mask': dev(np.repeat(np.arange(G), nph))}
    got = ddpm.edit_given_pockets(phar, pockets, fix_coords=dev(fx != 0)[:, None], fix_types=dev(fh != 0)[:, None], start=4, resamplings=2,
                                  weights=[1.0, 3.0], timesteps=K, seed=21, group_ids=[40, 41])
    h = ddpm.dynamics.hip_handle()
    want, _ = run_medit(h, pb, [M] * G, np.tile(np.array([0.25, 0.75], np.float32), G), (x, oh, fx, fh), K, 4, 2, 1, seed=21, ids=[40, 41])
    assert torch.equal(got[0].cpu(), torch.from_numpy(want[0]))
    assert len(got[1]) == M and len(got[3]) == M and torch.equal(got[2].cpu(), phar['mask'].cpu())
    base = np.concatenate([[0], np.cumsum(pb.size)])
    for m in range(M):
        rows = np.concatenate([np.arange(base[g * M + m], base[g * M + m + 1]) for g in range(G)])
        assert torch.equal(got[1][m].cpu(), torch.from_numpy(want[1][rows]))


def test_edit_phars_multi_end_to_end():
    """PharPocketDDPM.edit_phars_multi on the synthetic PDB given twice as two pockets with weights (0.5, 0.5): held points come back
    within 0.1 A in the PDB's frame, keep='both' from the prior returns them typed as given, the same seed gives the same result."""
    m = lightning_model()
    pdb = os.path.join(GOLDEN, 'g7_pocket.pdb')
    ids = [f'A:{i}' for i in range(1, 30)]
    names = list(m.dataset_info['phar_decoder'])
    phars = [(names[1], (9.0, 2.0, -15.0)), (names[3], (11.5, 4.0, -13.0)), (names[1], (7.0, 5.0, -12.0))]
    kw = dict(pocket_ids=[ids, ids], weights=[0.5, 0.5], timesteps=50)
    both = m.edit_phars_multi([pdb, pdb], 3, phars, keep='both', num_nodes_phar=torch.tensor([3, 5, 4]), seed=6, **kw)
    assert [len(s) for s in both] == [3, 5, 4]
    worst = 0.0
    for sample in both:
        assert [n for n, _ in sample[:3]] == [n for n, _ in phars]
        for (_, xyz), (_, got) in zip(phars, sample):
            worst = max(worst, float(np.linalg.norm(np.asarray(got) - np.asarray(xyz))))
    print(f'\n[edit_phars_multi] keep=both from the prior: worst distance of a held point {worst:.4f} A')
    assert worst < 0.1
    again = m.edit_phars_multi([pdb, pdb], 3, phars, keep='both', num_nodes_phar=torch.tensor([3, 5, 4]), seed=6, **kw)
    assert both == again
    part = m.edit_phars_multi([pdb, pdb], 2, phars, keep=['coords', 'types', 'none'], strength=0.4, seed=7, **kw)
    for sample in part:
        assert len(sample) == 3 and sample[1][0] == phars[1][0]
        assert float(np.linalg.norm(np.asarray(sample[0][1]) - np.asarray(phars[0][1]))) < 0.1
