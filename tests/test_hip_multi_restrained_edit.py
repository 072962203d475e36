"""GPU tests of ConditionalDDPM.edit_restrained_given_pockets / cmdgen_multi_restrained_edit_chain: parity with
multi_restrained_edit_ref on injected noise for a batch that mixes groups of 1, 2 and 3 members with every kind of mark and restraint (from
the prior with jumps, and part-way) and for a member above 128 nodes, the other engines, the three reductions bit for bit (to
cmdgen_multi_edit_chain, to cmdgen_restrained_edit_chain, to cmdgen_multi_restrained_chain), the members' copies of the latent, graphs
against eager launches and run to run, the effect itself with held rows, refusals, and the Python entry point.

Bounds against the reference are test_hip_restraint.py's: per-op z and pocket <= 1e-4 max(1, max|.|), final x and pocket RMS
<= 1e-4 max(1, max|.|), types exact; energy, max_violation and op_energy within 1e-4 max(1, |want|).  A group with a pair within 1e-4 A of the
cutoff at any reference evaluation is left out (multi_restrained_edit_cases.py: at most 20 % of a case's groups; none for the committed
inputs).  Held coordinates: test_hip_edit.py's 0.1 A.

Measured on an MI355X (worst ratio to each bound: per-op z / pocket steps / final x RMS / energy / max_violation / op_energy; no group left
out; the final pocket RMS is 0.000 everywhere):
  mixed from the prior at (2, 2), half, graph and eager   0.002 / 0.002 / 0.001 / 0.006 / 0.004 / 0.005
  mixed part-way from start 3, graph and eager            0.002 / 0.001 / 0.000 / 0.004 / 0.002 / 0.004
  large member at (1, 1), graph and eager                 0.001 / 0.001 / 0.000 / 0.010 / 0.004 / 0.005
  pairs on the bf3 and fp32 engines                       0.002 / 0.001 / 0.001 / 0.010 / 0.002 / 0.013
  held rows, K = 100, restraints on: coordinates within 0.0061 A of the given points (bound 0.1 A); the four groups' energies
  65704 / 2963 / 41338 / 38658 guided against 370228 / 50132 / 204165 / 134534 with scale = 0 (untrained weights)"""
import ctypes as C

import numpy as np
import pytest
import torch

import multi_edit_cases as mec
import multi_restrained_edit_cases as xc
import multi_restraint_cases as mrc
import chain_kit as kit
from chain_kit import (EINVAL, ESTATE, PLAIN, check_against_ref, dev, given_for, guide, handle, handle_for, model, pocket_dev, record, run_chain, same,
                       status_key)
from cmdgen_amd import hip_backend
from cmdgen_amd import restraints as rs
from cmdgen_amd.synthetic import ModelConfig, PocketBatch, make_state_dict, make_pockets

pytestmark = pytest.mark.gpu

EDIT = PLAIN + ('chain_z',)                            # what the unguided chains share with the guided ones


def given_dev(given):
    return [dev(np.asarray(a, np.float32)) for a in given]


def run_xedit(h, pb, sizes, w, given, rec, K, start=None, r=1, j=1, noise=None, seed=7, ids=None, use_graph=True, tables=True, **g):
    """cmdgen_multi_restrained_edit_chain; given = (phar_x, phar_one_hot, fix_x, fix_h) over the unique rows; g: guide()'s clash, scale,
    max_shift, guide_below"""
    return run_chain(h, pb, K, groups=(sizes, w), given=given, plan=(start, r, j), guide=guide(rec, **g), noise=noise, seed=seed, ids=ids,
                     use_graph=use_graph, tables=tables)


def run_medit(h, pb, sizes, w, given, K, start=None, r=1, j=1, **kw):
    """cmdgen_multi_edit_chain, on the host's tables as the guided chain it is compared with bit for bit"""
    return run_chain(h, pb, K, groups=(sizes, w), given=given, plan=(start, r, j), **kw)


# ------------------------------------------------------------------------------------------------ 1. / 2. against the reference
def check_run(run, engine, use_graph):
    r = xc.reference(run)
    case = xc.CASES[run.case]
    pb, gr, want, keep = r['pb'], r['groups'], r['guided'], r['keep']
    n_steps = xc.plan(run)[0]
    h = handle(engine)
    h.set_option('graph_steps', 2)
    got, st = run_xedit(h, pb, case.group_sizes, r['weights'], xc.given_rows(case), r['rec'], xc.K, run.start, run.r, run.j,
                        noise=r['noise'].cuda(), use_graph=use_graph)
    assert got.z_steps.shape == want['z_steps'].shape and got.pocket_steps.shape == want['pocket_steps'].shape
    assert got.op_energy.shape == (n_steps, gr.G)
    # test_hip_restraint.py's metric, not test_hip_restrained_edit.py's: the final x and pocket by their RMS, the pocket over its whole row
    check_against_ref(f'{xc.run_id(run)} {engine} {"graph" if use_graph else "eager"}', got, st, want, keep[gr.unique_mask.numpy()],
                      keep[gr.group_of][pb.mask], keep, 'groups', final='rms')
    return r


@pytest.mark.parametrize('use_graph', [True, False], ids=['graph', 'eager'])
@pytest.mark.parametrize('run', xc.RUNS, ids=xc.run_id)
def test_chain_matches_the_reference(run, use_graph):
    r = check_run(run, 'half', use_graph)
    if run.case == 'large':
        assert int((r['pb'].size + r['pb'].num_nodes_phar).max()) > 128           # the 1024-thread path ran


@pytest.mark.parametrize('engine', ['bf3', 'fp32'])
def test_other_engines_match_the_reference(engine):
    check_run(xc.ENGINE_RUN, engine, True)


# ------------------------------------------------------------------------------------------------ 3. the reductions
@pytest.mark.parametrize('inject', [False, True], ids=['device-draws', 'injected'])
@pytest.mark.parametrize('run', xc.RUNS, ids=xc.run_id)
def test_without_guidance_it_is_the_multi_edit_chain_bit_for_bit(run, inject):
    """No record and r_c = 0, scale = 0 with records and the clash term present, and guide_below = 0: xh_phar, xh_pocket, z_steps,
    pocket_steps, the chain status and the chain_z debug read of cmdgen_multi_edit_chain."""
    case = xc.CASES[run.case]
    r = xc.reference(run)
    pb, w, gr = r['pb'], r['weights'], r['groups']
    given = xc.given_rows(case)
    h = handle()
    h.set_option('graph_steps', 2)
    ids = 300 + np.arange(gr.G)
    kw = dict(start=run.start, r=run.r, j=run.j, noise=r['noise'].cuda() if inject else None, seed=11, ids=ids)
    want, sw = run_medit(h, pb, case.group_sizes, w, given, xc.K, **kw)
    none, s0 = run_xedit(h, pb, case.group_sizes, w, given, None, xc.K, clash=(0.0, 0.0), **kw)
    zero, s1 = run_xedit(h, pb, case.group_sizes, w, given, r['rec'], xc.K, scale=0.0, **kw)
    below, s2 = run_xedit(h, pb, case.group_sizes, w, given, r['rec'], xc.K, guide_below=0.0, **kw)
    for got in (none, zero, below):
        same(want, got, EDIT)
    assert status_key(sw) == status_key(s0) == status_key(s1) == status_key(s2) and sw['nan_resets'] == 0
    assert not none[4].any() and not none[5].any()                      # nothing restrains: zero energies
    assert zero[4][:, 0].max() > 0 and zero[5].max() > 0                # scale = 0 still reports them
    assert np.array_equal(zero[4], below[4]) and np.array_equal(zero[5], below[5])
    guided, _ = run_xedit(h, pb, case.group_sizes, w, given, r['rec'], xc.K, **kw)
    assert not np.array_equal(guided[0], want[0])                       # ... and the guidance is not a no-op here


@pytest.mark.parametrize('use_graph', [True, False], ids=['graph', 'eager'])
@pytest.mark.parametrize('inject', [False, True], ids=['device-draws', 'injected'])
def test_groups_of_one_are_the_restrained_edit_chain_bit_for_bit(inject, use_graph):
    """Every M_g = 1: cmdgen_restrained_edit_chain's outputs, energy_out and op_energy_out included, the chain status and chain_z, with no
    option set - from the prior without and with jumps, and part-way."""
    h = handle()
    h.set_option('graph_steps', 2)
    pb = make_pockets(6, 'CA', ragged=True, first_index=9500)
    nph = 1 + (np.arange(6, dtype=np.int64) * 3) % 8
    pb = PocketBatch(x=pb.x, one_hot=pb.one_hot, size=pb.size, mask=pb.mask, num_nodes_phar=nph, pocket_index=pb.pocket_index)
    nu = int(nph.sum())
    given = given_for(nph, 6)
    restraints = [{'kind': 'position', 'sample': 0, 'point': 0, 'center': (1.0, 0.0, -1.0), 'radius': 1.0, 'k': 1.0},
                  {'kind': 'distance', 'sample': 2, 'points': (0, 3), 'lo': 5.0, 'hi': 7.0, 'k': 1.0},       # a held-x and a free point
                  {'kind': 'distance', 'sample': 3, 'points': (0, 1), 'lo': 5.0, 'hi': 7.0, 'k': 1.0},
                  {'kind': 'exclusion', 'sample': 5, 'center': (0.0, 0.0, 0.0), 'radius': 4.0, 'k': 1.0}]
    rec = rs.records(restraints, nph)
    base2 = int(nph[:2].sum())
    assert given[2][base2] != given[2][base2 + 3]
    for K, start, r, j, clash in ((6, 6, 1, 1, xc.CLASH), (6, 6, 2, 2, (0.0, 0.0)), (6, 3, 1, 1, xc.CLASH)):
        h.set_layout(pb.num_nodes_phar, pb.size)
        n_draws = h.edit_plan(K, start, r, j)[1]
        noise = dev(np.random.default_rng(10 + start).normal(size=(n_draws, nu, 11)).astype(np.float32)) if inject else None
        kw = dict(noise=noise, seed=11, ids=pb.pocket_index, use_graph=use_graph)
        want, sw = run_chain(h, pb, K, given=given, plan=(start, r, j), guide=guide(rec, clash=clash), **kw)
        got, sg = run_xedit(h, pb, [1] * 6, np.ones(6, np.float32), given, rec, K, start, r, j, clash=clash, **kw)
        same(want, got)
        assert status_key(sw) == status_key(sg) and sw['nan_resets'] == 0
        assert want[4][:, 0].max() > 0 and want[5].max() > 0


@pytest.mark.parametrize('use_graph', [True, False], ids=['graph', 'eager'])
@pytest.mark.parametrize('inject', [False, True], ids=['device-draws', 'injected'])
def test_no_marks_from_the_prior_are_the_multi_restrained_chain_bit_for_bit(inject, use_graph):
    """No mark in either mask, start = timesteps, r = j = 1 on multi_restraint_cases.MIXED's inputs against cmdgen_multi_restrained_chain.
    Injected: the edit plan draws A and B per op, so the restrained multi-pocket chain's K + 2 rows sit in rows 0, 1, 3, 5, .. and the last
    of this chain's noise."""
    case = mrc.MIXED
    pb, w = mrc.member_pockets(case), mrc.weights_of(case)
    rec = rs.records(mrc.restraints_of(case, pb), case.nph)
    h = handle()
    h.set_option('graph_steps', 2)
    K, nu = mrc.K, int(sum(case.nph))
    x, oh, _, _ = given_for(np.asarray(case.nph), 3)
    zero = np.zeros(nu, np.float32)
    noise = spread = None
    if inject:
        noise = mrc.noise_of(case).numpy()
        n_draws = 2 + 2 * K
        spread = np.random.default_rng(6).normal(size=(n_draws, nu, 11)).astype(np.float32)
        spread[[0] + [1 + 2 * i for i in range(K)] + [n_draws - 1]] = noise
        noise, spread = dev(noise), dev(spread)
    ids = 500 + np.arange(len(case.nph))
    want, sw = run_chain(h, pb, K, groups=(case.group_sizes, w), guide=guide(rec), noise=noise, seed=31, ids=ids, use_graph=use_graph)
    got, sg = run_xedit(h, pb, case.group_sizes, w, (x, oh, zero, zero), rec, K, noise=spread, seed=31, ids=ids, use_graph=use_graph)
    same(want, got)
    assert status_key(sw) == status_key(sg) and sw['nan_resets'] == 0
    assert want[4][:, 0].max() > 0 and want[5].max() > 0


# ------------------------------------------------------------------------------------------------ 4. copies, graphs, run to run
def test_copies_stay_identical_and_runs_repeat_bit_for_bit():
    """Device draws with group ids on the mixed case, from the prior with jumps.  After a guided run every member's copy of z equals its
    group's first; the captured chain twice and the eager one agree on every output; other group ids give other draws; a changed scalar
    prepares the slot again and the first arguments give the first result back; and with the clash term off, the group no record touches
    follows cmdgen_multi_edit_chain through the first op."""
    run = xc.RUNS[0]
    case = xc.CASES[run.case]
    r = xc.reference(run)
    pb, w, gr = r['pb'], r['weights'], r['groups']
    given = xc.given_rows(case)
    h = handle()
    h.set_option('graph_steps', 2)
    ids = 700 + 3 * np.arange(gr.G)
    kw = dict(start=run.start, r=run.r, j=run.j, seed=31, ids=ids)
    a, sa = run_xedit(h, pb, case.group_sizes, w, given, r['rec'], xc.K, use_graph=True, **kw)
    assert h.query('chain_graphs') >= 1
    z = a.chain_z.reshape(gr.Nl, 11)
    first_rows = gr.first_rows().numpy()[gr.urow.numpy()]              # per member row: the same row of the group's first member
    assert gr.max_m == 3 and np.array_equal(z, z[first_rows])
    b, sb = run_xedit(h, pb, case.group_sizes, w, given, r['rec'], xc.K, use_graph=True, **kw)
    e, se = run_xedit(h, pb, case.group_sizes, w, given, r['rec'], xc.K, use_graph=False, **kw)
    same(a, b)
    same(a, e)
    assert status_key(sa) == status_key(sb) == status_key(se) and sa['nan_resets'] == 0
    other, _ = run_xedit(h, pb, case.group_sizes, w, given, r['rec'], xc.K, **dict(kw, ids=ids + 1))
    assert not np.array_equal(a[0], other[0])
    c, _ = run_xedit(h, pb, case.group_sizes, w, given, r['rec'], xc.K, clash=(xc.CLASH[0], 2.0), **kw)
    assert not np.array_equal(a[0], c[0])
    back, _ = run_xedit(h, pb, case.group_sizes, w, given, r['rec'], xc.K, **kw)
    same(a, back)
    # the bare group: no record, r_c = 0
    g = case.bare_group
    rows, rows_q = gr.unique_mask.numpy() == g, gr.group_of[pb.mask] == g
    off, _ = run_xedit(h, pb, case.group_sizes, w, given, r['rec'], xc.K, clash=(0.0, 0.0), **kw)
    plain, _ = run_medit(h, pb, case.group_sizes, w, given, xc.K, **kw)
    assert np.array_equal(off[2][0][rows], plain[2][0][rows]) and np.array_equal(off[3][0][rows_q], plain[3][0][rows_q])
    assert not np.array_equal(off[2][0][~rows], plain[2][0][~rows])     # ... while the others are steered
    assert off[4][g, 0] == 0 and not off[5][:, g].any()


# ------------------------------------------------------------------------------------------------ 5. the effect
def test_held_rows_stay_and_guidance_lowers_the_energy():
    """multi_edit_cases' held-rows case (groups of two, K = 100 on hold_config, device draws) with multi_restraint_cases' recipe of restraints:
    the rows whose coordinates are held come back within HOLD_BOUND of their given points, held types come back, and the touched groups end
    with less energy than with scale = 0 on the same seed."""
    hc = mec.hold_case()
    cfg = mec.hold_config()
    h = handle_for(cfg, 'seed0', make_state_dict(cfg, seed=0))
    case = xc.Case(*hc['case'], None)
    rec = rs.records(mrc.restraints_of(case, hc['pb']), case.nph)
    given = (hc['phar_x'], hc['phar_oh'], hc['coords_only'], hc['types_only'])
    kw = dict(seed=hc['seed'], tables=False)             # hold_config is another model: host_tables' are the bounded model's
    g, st = run_xedit(h, hc['pb'], hc['sizes'], hc['weights'], given, rec, mec.HOLD_K, **kw)
    u, _ = run_xedit(h, hc['pb'], hc['sizes'], hc['weights'], given, rec, mec.HOLD_K, scale=0.0, **kw)
    assert st['max_rel_com_error'] < 1e-2 and st['nan_resets'] == 0
    err = mec.held_errors(hc, g[0], g[1])
    print(f'\n[effect] coords-held max err {err[hc["coords_only"]].max():.4f} A (bound {mec.HOLD_BOUND}); final energy per group unguided '
          f'{u[4][:, 0]}\n         guided   {g[4][:, 0]}\n         largest violation (A) unguided {u[4][:, 1]}\n         guided   {g[4][:, 1]}')
    assert set(hc['sizes']) == {2} and hc['coords_only'].any() and hc['types_only'].any()
    assert np.array_equal(g[0][hc['types_only'], 3:], hc['phar_oh'][hc['types_only']])
    assert err[hc['coords_only']].max() < mec.HOLD_BOUND
    assert float(g[4][:, 0].sum()) < float(u[4][:, 0].sum())            # (the clash term touches every group)


# ------------------------------------------------------------------------------------------------ 6. refusals
def _raw_call(h, px, poh, sizes, w, given, K, start=None, rec=None):
    """The C entry itself (Handle.multi_restrained_edit_chain asks cmdgen_edit_plan first, which refuses a start or a joint handle with its own
    message)."""
    sizes = np.ascontiguousarray(np.asarray(sizes, dtype=np.int64))
    w = np.ascontiguousarray(np.asarray(w, dtype=np.float32))
    out_p, out_q = torch.empty((8, 11), device='cuda'), torch.empty((px.shape[0], 23), device='cuda')
    energy = torch.empty((len(sizes), 2), device='cuda')
    ptr = lambda t: C.c_void_p(t.data_ptr())
    rec_p, n_rec = h._restraint_arg(rec)
    return h.lib.cmdgen_multi_restrained_edit_chain(
        h.h, ptr(px), ptr(poh), len(sizes), sizes.ctypes.data_as(C.POINTER(C.c_int64)), w.ctypes.data_as(C.c_void_p), *[ptr(a) for a in given],
        K, K if start is None else start, 1, 1, C.c_void_p(0), 0, C.c_uint64(0), None, ptr(out_p), ptr(out_q), C.c_void_p(0), C.c_void_p(0),
        rec_p, n_rec, 0.0, 0.0, 1.0, 1.0, 1.0, ptr(energy), C.c_void_p(0), 1, h._stream())


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
        return given_dev(given_for(np.array([nu]), 1))

    refused = lambda h, match, rec=None, sizes=(2, 2), w=half, nu=8, K=5, code=EINVAL, **kw: kit.refused(      # the message, and the code
        h, lambda: h.multi_restrained_edit_chain(px, poh, list(sizes), w, *args(nu), K, restraints=rec, **kw), match, code)

    def refused_raw(h, match, code, **kw):
        rc = _raw_call(h, px, poh, [2, 2], half, args(8), 5, **kw)
        assert rc == code
        with pytest.raises(hip_backend.CmdgenError, match=match):
            h._check(rc, 'cmdgen_multi_restrained_edit_chain')

    # of a restraint list and the scalars: cmdgen_multi_restrained_chain's refusals, saying "group"
    refused(h, "group 2 outside the call's 2 groups", record(sample=2))
    refused(h, "group -1 outside the call's 2 groups", record(sample=-1))
    refused(h, 'point 3, group 0 has 3 points', record(i=3))
    refused(h, 'point 5, group 1 has 5 points', record(kind=1, sample=1, i=0, j=5, a=1.0, b=2.0))
    refused(h, 'point 3, group 1 has 3 points', record(sample=1, i=3), sizes=(1, 1, 2), w=np.array([1, 1, 0.5, 0.5], np.float32), nu=11)
    refused(h, 'i == j', record(kind=1, sample=1, i=2, j=2, a=1.0, b=2.0))
    refused(h, 'lo=3 > hi=2', record(kind=1, sample=1, i=0, j=1, a=3.0, b=2.0))
    refused(h, 'max_shift', record(), max_shift=0.0)
    refused(h, 'unknown kind', record(kind=3))
    refused(h, 'scale', record(), scale=-1.0)
    refused(h, 'guide_below', record(), guide_below=1.5)
    refused(h, 'clash_radius', record(), clash_radius=-1.0)
    refused(h, 'group 1 has more than 256 restraints', np.concatenate([record(kind=2, sample=1)] * 257))
    # of a grouping and a plan: cmdgen_multi_edit_chain's refusals
    refused(h, 'share one latent', record(), sizes=(1, 2, 1), w=np.array([1, 0.5, 0.5, 1], np.float32), nu=11)   # members of 3 and 5 points
    refused(h, 'not 1', record(), w=np.array([0.5, 0.6, 0.5, 0.5], np.float32))
    refused(h, 'sum to 3', record(), sizes=(2, 1), w=np.array([0.5, 0.5, 1, 1], np.float32))
    refused(h, 'sizes must be in', record(), sizes=(2, 0, 2), nu=13)
    for bad in (0, 6, -3):
        refused_raw(h, r'start=-?\d+ must be in \[1, timesteps=5\]', EINVAL, start=bad)
    n_steps, n_draws = h.edit_plan(10, 6, 2, 1)
    short = torch.zeros((n_draws - 1, 8, 11), device='cuda')
    refused(h, f'noise holds {n_draws - 1} draws, the schedule needs {n_draws}', record(), K=10, start=6, resamplings=2, noise=short)
    good = h.multi_restrained_edit_chain(px, poh, [2, 2], half, *args(8), 5, start=3, restraints=record(), clash_radius=3.0, clash_k=1.0, seed=3)
    plain = h.multi_edit_chain(px, poh, [2, 2], half, *args(8), 5, start=3, seed=3)       # ... and an ordinary chain follows
    st = h.chain_status()
    assert good[0].shape == plain[0].shape == (8, 11) and good[3].shape == (2, 2) and st['max_rel_com_error'] < 1e-2
    assert all(bool(torch.isfinite(t).all()) for t in (good[0], good[3], plain[0]))
    h.close()
    jcfg = ModelConfig(hidden_nf=64, n_layers=1, update_pocket_coords=True)
    joint = hip_backend.Handle(jcfg.as_dict(), 0)
    joint.load_state_dict(make_state_dict(jcfg, seed=0))
    joint.set_layout(pb.num_nodes_phar, pb.size)
    refused_raw(joint, 'restrained multi-pocket edit chain is not supported for the joint model', ESTATE, rec=record())
    assert joint.joint_chain(5, seed=3)[0].shape == (16, 11)
    joint.close()
    scfg = ModelConfig(hidden_nf=64, n_layers=1, timesteps=500, no_com_projection=True)
    simple = hip_backend.Handle(scfg.as_dict(), 0)
    simple.load_state_dict(make_state_dict(scfg, seed=0))
    simple.set_layout(pb.num_nodes_phar, pb.size)
    refused_raw(simple, 'restrained multi-pocket edit chain is not supported for no_com_projection', ESTATE, rec=record())
    assert simple.sample_chain(px, poh, 5, seed=3)[0].shape == (16, 11)
    simple.close()


# ------------------------------------------------------------------------------------------------ the Python entry point
def test_edit_restrained_given_pockets_returns_the_chains_result():
    """ConditionalDDPM.edit_restrained_given_pockets on the pairs run: the chain's outputs (bit for bit the binding's, same tables and draws)
    split per pocket, the info dict, and scale = 0 as edit_given_pockets."""
    run = xc.ENGINE_RUN
    case = xc.CASES[run.case]
    r = xc.reference(run)
    pb, gr = r['pb'], r['groups']
    ddpm = model()
    ddpm.use_hip_graph = True
    pockets = [pocket_dev(pb, [2 * g + m for g in range(gr.G)]) for m in range(2)]
    px, poh, fx, fh = xc.given_rows(case)
    nph = np.asarray(case.nph, dtype=np.int64)
    phar = {'x': dev(px), 'one_hot': dev(poh), 'size': dev(nph), 'mask': dev(np.repeat(np.arange(gr.G), nph))}
    w = r['weights'].reshape(gr.G, 2)
    noise = r['noise'].cuda()
    kw = dict(fix_coords=dev(fx != 0)[:, None], fix_types=dev(fh != 0)[:, None], start=run.start, resamplings=run.r, jump_length=run.j,
              weights=w, timesteps=xc.K, noise=noise)
    x, qs, pm, qms, info = ddpm.edit_restrained_given_pockets(phar, pockets, r['restraints'], clash=xc.CLASH, scale=xc.SCALE,
                                                              max_shift=xc.MAX_SHIFT, **kw)
    want, _ = run_xedit(ddpm.dynamics.hip_handle(), pb, case.group_sizes, r['weights'], (px, poh, fx, fh), r['rec'], xc.K, run.start, run.r,
                        run.j, noise=noise)
    assert np.array_equal(x.cpu().numpy(), want[0]) and len(qs) == 2 and pm.shape == (gr.Nu,)
    for m in range(2):
        assert np.array_equal(qs[m].cpu().numpy(), want[1][np.isin(pb.mask, [2 * g + m for g in range(gr.G)])])
    assert np.array_equal(info['energy'].cpu().numpy(), want[4][:, 0]) and np.array_equal(info['max_violation'].cpu().numpy(), want[4][:, 1])
    assert set(info) == {'energy', 'max_violation'}
    plain = ddpm.edit_given_pockets(phar, pockets, **kw)
    off = ddpm.edit_restrained_given_pockets(phar, pockets, r['restraints'], clash=xc.CLASH, scale=0.0, **kw)
    assert torch.equal(off[0], plain[0]) and all(torch.equal(a, b) for a, b in zip(off[1], plain[1]))
    assert not torch.equal(x, plain[0])
