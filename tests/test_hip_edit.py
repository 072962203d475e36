"""GPU tests of ConditionalDDPM.edit / cmdgen_edit_chain: parity with the G22 vectors (composed from the reference's own
methods, tests/golden/make_golden_edit.py), the plan, the reduction to the inpainting chain bit for bit, graphs against eager
runs while the start level, the seed and want_steps change, the two kinds of hold, shard independence, refusals and
PharPocketDDPM.edit_phars.

Tolerances are those of test_hip_inpaint.py for G20: coordinate RMS <= 1e-4 * max(1, max|x|), types exact, per-op z and pocket
max-abs <= 1e-4 * max(1, max|.|) (every G22 fixture keeps its pairs >= 2e-3 A away from the cutoff); reductions bit for bit."""
import os
from functools import partial

import numpy as np
import pytest
import torch

from helpers import load_golden, cases_of, cfg_from_meta, rms, GOLDEN
from edit_ref import edit_plan
from chain_kit import dev, fixed_inputs, handle_for, lightning_model, model_for, pocket_dev, run_chain, same, PLAIN
from cmdgen_amd import hip_backend
from cmdgen_amd.synthetic import ModelConfig, make_state_dict, make_pockets
from bench import bounded_config

pytestmark = pytest.mark.gpu

G22 = load_golden('g22_edit.npz')
run = partial(run_chain, tables=False, want_steps=False)          # as test_hip_inpaint.py


def g22_case(name):
    H, L, B, R, seed, K, r, j, first, start = [int(v) for v in G22[name + '/meta']]
    cfg = cfg_from_meta(H, L, R)
    sd = make_state_dict(cfg, seed=seed, coord_gain=1.0)
    pb = make_pockets(B, 'CA', ragged=True, n_phar=7, first_index=first)
    return cfg, sd, pb, (K, start, r, j)


def run_edit(h, pb, phar_x, phar_oh, fix_x, fix_h, K, start=None, r=1, j=1, **kw):
    return run(h, pb, K, given=(phar_x, phar_oh, fix_x, fix_h), plan=(start, r, j), **kw)


@pytest.mark.parametrize('use_graph', [True, False])
@pytest.mark.parametrize('name', cases_of(G22))
def test_edit_chain_matches_g22(name, use_graph):
    cfg, sd, pb, (K, start, r, j) = g22_case(name)
    h = handle_for(cfg, name, sd)
    noise = dev(G22[name + '/noise'])
    h.set_layout(pb.num_nodes_phar, pb.size)
    assert h.edit_plan(K, start, r, j) == edit_plan(r, j, K, start)[:2]
    (xh_phar, xh_pocket, z_steps, p_steps, *_), st = run_edit(h, pb, G22[name + '/phar_x'], G22[name + '/phar_one_hot'], G22[name + '/fix_x'],
                                                              G22[name + '/fix_h'], K, start, r, j, noise=noise, use_graph=use_graph,
                                                              want_steps=True)
    want = G22[name + '/xh_phar']
    e = rms(xh_phar[:, :3], want[:, :3])
    print(name, 'graph' if use_graph else 'eager', 'x rms', e, 'scale', float(np.abs(want[:, :3]).max()))
    assert e <= 1e-4 * max(1.0, float(np.abs(want[:, :3]).max()))
    assert np.array_equal(xh_phar[:, 3:], want[:, 3:])
    wq = G22[name + '/xh_pocket']
    assert rms(xh_pocket, wq) <= 1e-4 * max(1.0, float(np.abs(wq).max()))
    zs, ps = G22[name + '/z_steps'], G22[name + '/pocket_steps']
    assert z_steps.shape == zs.shape and p_steps.shape == ps.shape
    for k in range(len(zs)):
        ez, ep = float(np.abs(z_steps[k] - zs[k]).max()), float(np.abs(p_steps[k] - ps[k]).max())
        print('  op', k, 'z', ez, 'pocket', ep)
        assert ez <= 1e-4 * max(1.0, float(np.abs(zs[k]).max())), k
        assert ep <= 1e-4 * max(1.0, float(np.abs(ps[k]).max())), k
    assert st['max_rel_com_error'] < 1e-2 and st['nan_resets'] == 0


@pytest.mark.parametrize('K,start,r,j', [(20, 20, 1, 1), (20, 7, 1, 1), (17, 9, 2, 1), (30, 30, 3, 2), (30, 11, 3, 2), (50, 1, 4, 3)])
def test_plan_equals_the_cpu_plan(K, start, r, j):
    cfg = ModelConfig(hidden_nf=64, n_layers=1, timesteps=500)
    h = handle_for(cfg, 'seed0', make_state_dict(cfg, seed=0))
    assert h.edit_plan(K, start, r, j) == edit_plan(r, j, K, start)[:2]
    if start == K:
        assert h.edit_plan(K, None, r, j) == h.inpaint_plan(K, r, j)


def _max_degree(h, pb, z_steps, p_steps):
    """The largest number of edges one receiver has in the radius graphs of the saved states (the inputs of the evaluations 1 ..)."""
    nl, nq = pb.num_nodes_phar, pb.size
    a, b = np.concatenate([[0], np.cumsum(nl)]), np.concatenate([[0], np.cumsum(nq)])
    worst = 0
    for z, p in zip(z_steps, p_steps):
        x = np.concatenate([np.concatenate([z[a[i]:a[i + 1], :3], p[b[i]:b[i + 1]]]) for i in range(len(nl))]).astype(np.float32)
        row, _ = h.radius_graph(dev(x), nl + nq)
        worst = max(worst, int(torch.bincount(row.long()).max()))
    return worst


@pytest.mark.parametrize('split', [True, False])
@pytest.mark.parametrize('use_graph', [True, False])
def test_equal_masks_from_the_prior_equal_inpaint_chain_bit_for_bit(use_graph, split):
    """edit_chain(m, m, start = K) is inpaint_chain(m): outputs, saved steps and chain status, with device draws and with
    injected noise, for (r, j) = (1, 1) and (2, 2), on the default and the fp32 instruction engine.

    Tile rows on the fp32 instruction engine.  Comparing two runs bit for bit presupposes that one run is reproducible, and the library
    states when it is (make_plan, cmdgen_plan.h): k_edge_msg / k_edge_coord add a receiver's per-tile partial sums with float atomics, so
    a receiver whose edges span three or more tiles is summed in an order the hardware picks.  At this size that engine would choose
    16-row tiles, and a phar point in the pocket's centre has more than the 17 edges two such tiles are sure to hold (measured: two
    inpaint_chain runs of the SAME inputs then differ in the last bit of ~1000 saved h values, max 1.4e-6, outputs equal).  With 64-row
    tiles - the library's own rule for dense samples - a receiver of up to 65 edges is at most two partials, whose sum does not depend on
    the order; the test checks that premise on the saved states (_max_degree).  The default engine keeps the library's choices."""
    cfg = bounded_config(20, 1000)
    h = hip_backend.Handle(cfg.as_dict(), 0)
    h.load_state_dict(make_state_dict(cfg, seed=0))
    h.set_gemm_mode(split)
    pb = make_pockets(6, 'CA', ragged=True, first_index=300)
    if not split:
        h.set_option('edge_mt', 64)
        h.set_option('coord_mt', 64)
        h.set_layout(pb.num_nodes_phar, pb.size)
        assert h.query('edge_mt') == 64 and h.query('coord_mt') == 64
    px, poh, fixed, _ = fixed_inputs(pb, 0.25, np.random.default_rng(8))
    fixed[np.repeat(np.arange(6), pb.num_nodes_phar) == 3] = 0.0          # one sample without a mark
    nl = int(pb.num_nodes_phar.sum())
    K = 20
    for r, j in ((1, 1), (2, 2)):
        h.set_layout(pb.num_nodes_phar, pb.size)
        n_draws = h.inpaint_plan(K, r, j)[1]
        noise = dev(np.random.default_rng(9).normal(size=(n_draws, nl, 3 + cfg.phar_nf)).astype(np.float32))
        for inject in (None, noise):
            a, sa = run(h, pb, K, given=(px, poh, fixed), plan=(None, r, j), noise=inject, seed=11, use_graph=use_graph, want_steps=True)
            b, sb = run_edit(h, pb, px, poh, fixed, fixed, K, K, r, j, noise=inject, seed=11, use_graph=use_graph, want_steps=True)
            same(a, b, PLAIN)
            assert sa == sb
            assert sb['max_rel_com_error'] < 1e-2
            if not split:
                deg = _max_degree(h, pb, a.z_steps, a.pocket_steps)
                print('fp32 engine, r, j =', r, j, 'max edges per receiver over the saved states:', deg)
                assert deg <= 65
    h.close()


def test_graph_runs_equal_eager_runs_as_start_seed_and_steps_change():
    """On one handle, graph-mode plain, inpainting and edit chains each equal their eager run bit for bit (outputs, saved steps,
    chain status) while the start level, the seed and want_steps change one at a time; the three kinds alternate on the handle and
    the inpainting and the edit chain share one slot."""
    cfg = bounded_config(20, 1000)
    h = hip_backend.Handle(cfg.as_dict(), 0)
    h.load_state_dict(make_state_dict(cfg, seed=0))
    pb = make_pockets(5, 'CA', ragged=True, first_index=500)
    px, poh, fixed, pm = fixed_inputs(pb, 0.5, np.random.default_rng(5))
    fix_x = fixed * (np.arange(len(fixed)) % 2 == 0)
    fix_h = fixed * (np.arange(len(fixed)) % 3 != 0)
    K = 17
    h.set_layout(pb.num_nodes_phar, pb.size)
    args = {'plain': (dev(pb.x), dev(pb.one_hot)),
            'inpaint': (dev(pb.x), dev(pb.one_hot), dev(px), dev(poh), dev(np.asarray(fixed, np.float32))),
            'edit': (dev(pb.x), dev(pb.one_hot), dev(px), dev(poh), dev(np.asarray(fix_x, np.float32)), dev(np.asarray(fix_h, np.float32)))}

    def run(kind, use_graph, seed, start=None, want_steps=False):
        chain = {'plain': h.sample_chain, 'inpaint': h.inpaint_chain, 'edit': h.edit_chain}[kind]
        kw = {'start': start} if kind == 'edit' else {}
        out = chain(*args[kind], K, noise=None, seed=seed, want_steps=want_steps, use_graph=use_graph, **kw)
        st = h.chain_status()
        arrays = [t.cpu().numpy() for t in out + (h.last_pocket_steps,) if t is not None]
        return arrays, (st['max_rel_com_error'], st['max_cog'], st['nan_resets'])

    variants = [dict(seed=1), dict(seed=1, start=9), dict(seed=2, start=9), dict(seed=2, start=9, want_steps=True),
                dict(seed=2, start=17, want_steps=True), dict(seed=2, start=4), dict(seed=2, start=9)]
    for v in variants:
        plain_kw = {k: v[k] for k in v if k != 'start'}
        graph = {kind: run(kind, True, **(v if kind == 'edit' else plain_kw)) for kind in ('plain', 'inpaint', 'edit')}
        for kind in ('plain', 'inpaint', 'edit'):
            eager = run(kind, False, **(v if kind == 'edit' else plain_kw))
            assert len(graph[kind][0]) == len(eager[0]) == (4 if v.get('want_steps') else 2), (kind, v)
            for a, b in zip(graph[kind][0], eager[0]):
                assert np.array_equal(a, b), (kind, v)
            assert graph[kind][1] == eager[1], (kind, v)
    h.close()


def test_types_hold_and_coordinates_hold():
    """64 C-alpha pockets, K = 100, the first quarter of each sample's rows marked: in even samples the types are held, in odd
    samples the coordinates.  Held types come back exactly; held coordinates sit within 0.1 A of the given point in the pocket's
    frame (test_fixed_points_hold's bound: sigma_0 ~ 3.2e-3 at noise precision 1e-5, times the B draw, the decode draw and eps_x -
    the x columns of a held row see the arithmetic of a fixed row).  The free part of a marked row actually moves: some types-only
    row ends more than that bound away from its input point, some coordinates-only row ends with another type."""
    cfg = ModelConfig(timesteps=500)
    h = handle_for(cfg, 'seed0', make_state_dict(cfg, seed=0))
    pb = make_pockets(64, 'CA', ragged=True, first_index=1000)
    px, poh, marked, pm = fixed_inputs(pb, 0.25, np.random.default_rng(1))
    types_only = (marked != 0) & (pm % 2 == 0)
    coords_only = (marked != 0) & (pm % 2 == 1)
    (xh_phar, xh_pocket, *_), st = run_edit(h, pb, px, poh, coords_only, types_only, 100, seed=21)
    assert st['max_rel_com_error'] < 1e-2 and st['nan_resets'] == 0
    assert np.array_equal(xh_phar[types_only, 3:], poh[types_only])
    B = len(pb.size)
    shift = np.stack([pb.x[pb.mask == b].mean(0) - xh_pocket[pb.mask == b, :3].mean(0) for b in range(B)])
    err = np.linalg.norm(xh_phar[:, :3] + shift[pm] - px, axis=1)
    retyped = (xh_phar[:, 3:].argmax(1) != poh.argmax(1))
    print('coords-only max err', err[coords_only].max(), 'types-only: moved rows', int((err[types_only] > 0.1).sum()), 'of',
          int(types_only.sum()), 'max', err[types_only].max(), '; coords-only: retyped rows', int(retyped[coords_only].sum()), 'of',
          int(coords_only.sum()))
    assert err[coords_only].max() < 0.1, err[coords_only].max()
    assert (err[types_only] > 0.1).any()
    assert retyped[coords_only].any()


def test_shards_reproduce_the_full_batch():
    cfg = bounded_config(20, 1000)
    h = handle_for(cfg, 'seed0', make_state_dict(cfg, seed=0))
    K, start = 8, 5
    full = make_pockets(8, 'CA', ragged=True)
    px, poh, marked, pm = fixed_inputs(full, 0.25, np.random.default_rng(3))
    fx, fh = marked * (pm % 2 == 1), marked * (pm % 2 == 0)
    (xf, *_), _ = run_edit(h, full, px, poh, fx, fh, K, start, 2, 1, ids=full.pocket_index)
    parts = []
    for first in (0, 4):
        sub = make_pockets(4, 'CA', ragged=True, first_index=first)
        rows = np.isin(pm, np.arange(first, first + 4))
        (xs, *_), _ = run_edit(h, sub, px[rows], poh[rows], fx[rows], fh[rows], K, start, 2, 1, ids=sub.pocket_index)
        parts.append(xs)
    xs = np.concatenate(parts)
    assert np.abs(xs[:, :3] - xf[:, :3]).max() <= 1e-4 * max(1.0, np.abs(xf[:, :3]).max())
    assert np.array_equal(xs[:, 3:], xf[:, 3:])


def test_refusals():
    cfg = ModelConfig(hidden_nf=64, n_layers=1, timesteps=500)
    pb = make_pockets(2, 'CA', ragged=True)
    px, poh, fixed, _ = fixed_inputs(pb, 0.25, np.random.default_rng(4))
    jcfg = ModelConfig(hidden_nf=64, n_layers=1, update_pocket_coords=True)
    joint = hip_backend.Handle(jcfg.as_dict(), 0)
    joint.load_state_dict(make_state_dict(jcfg, seed=0))
    with pytest.raises(hip_backend.CmdgenError, match='cmdgen_joint_chain'):
        joint.edit_plan(10, 5)
    joint.set_layout(pb.num_nodes_phar, pb.size)
    with pytest.raises(hip_backend.CmdgenError, match='cmdgen_joint_chain'):
        run_edit(joint, pb, px, poh, fixed, fixed, 10, 5)
    joint.close()
    simple_cfg = ModelConfig(hidden_nf=64, n_layers=1, timesteps=500, no_com_projection=True)
    simple = hip_backend.Handle(simple_cfg.as_dict(), 0)
    simple.load_state_dict(make_state_dict(simple_cfg, seed=0))
    with pytest.raises(hip_backend.CmdgenError, match='SimpleConditionalDDPM'):
        simple.edit_plan(10, 5)
    simple.set_layout(pb.num_nodes_phar, pb.size)
    with pytest.raises(hip_backend.CmdgenError, match='SimpleConditionalDDPM'):
        run_edit(simple, pb, px, poh, fixed, fixed, 10, 5)
    simple.close()
    h = handle_for(cfg, 'seed0', make_state_dict(cfg, seed=0))
    h.set_layout(pb.num_nodes_phar, pb.size)
    for bad in (0, 11, -3):
        with pytest.raises(hip_backend.CmdgenError, match='start'):
            h.edit_plan(10, bad)
        with pytest.raises(hip_backend.CmdgenError, match='start'):
            run_edit(h, pb, px, poh, fixed, fixed, 10, bad)
    n_steps, n_draws = h.edit_plan(10, 6, 2, 1)
    short = torch.zeros((n_draws - 1, int(pb.num_nodes_phar.sum()), 11), device='cuda')
    with pytest.raises(hip_backend.CmdgenError, match='draws'):
        run_edit(h, pb, px, poh, fixed, fixed, 10, 6, 2, 1, noise=short)
    ddpm = model_for(cfg, make_state_dict(cfg, seed=0))
    phar = {'x': dev(px), 'one_hot': dev(poh), 'size': dev(pb.num_nodes_phar), 'mask': dev(np.repeat(np.arange(2), pb.num_nodes_phar))}
    with pytest.raises(ValueError, match='draws'):
        ddpm.edit(phar, pocket_dev(pb), fix_types=dev(fixed), start=6, resamplings=2, timesteps=10, noise=short)
    with pytest.raises(ValueError, match='start'):
        ddpm.edit(phar, pocket_dev(pb), fix_types=dev(fixed), start=11, timesteps=10)


def test_python_edit_matches_g22():
    """ConditionalDDPM.edit (bool masks of shape [Nl, 1]) returns the chain's result."""
    name = 'h64_K10_s6_mixed_r2j1'
    cfg, sd, pb, (K, start, r, j) = g22_case(name)
    ddpm = model_for(cfg, sd)
    nph = torch.from_numpy(pb.num_nodes_phar)
    phar = {'x': dev(G22[name + '/phar_x']), 'one_hot': dev(G22[name + '/phar_one_hot']), 'size': nph.cuda(),
            'mask': dev(np.repeat(np.arange(len(nph)), pb.num_nodes_phar))}
    out_phar, out_pocket, phar_mask, _ = ddpm.edit(phar, pocket_dev(pb), fix_coords=dev(G22[name + '/fix_x'] != 0)[:, None],
                                                   fix_types=dev(G22[name + '/fix_h'] != 0)[:, None], start=start, resamplings=r,
                                                   jump_length=j, timesteps=K, noise=dev(G22[name + '/noise']))
    want = G22[name + '/xh_phar']
    out_phar = out_phar.cpu().numpy()
    assert rms(out_phar[:, :3], want[:, :3]) <= 1e-4 * max(1.0, float(np.abs(want[:, :3]).max()))
    assert np.array_equal(out_phar[:, 3:], want[:, 3:])
    assert torch.equal(phar_mask.cpu(), phar['mask'].cpu())


def test_edit_phars_end_to_end():
    """PharPocketDDPM.edit_phars on the g7 pocket (30 C-alpha residues): held types come back in every sample, held points within
    0.1 A, the same seed gives the same result, strength with extra free rows is refused, and the result feeds score_phars."""
    model = lightning_model()
    pdb = os.path.join(GOLDEN, 'g7_pocket.pdb')
    ids = [f'A:{i}' for i in range(1, 30)]
    names = list(model.dataset_info['phar_decoder'])
    phars = [(names[1], (9.0, 2.0, -15.0)), (names[3], (11.5, 4.0, -13.0)), (names[1], (7.0, 5.0, -12.0))]
    out = model.edit_phars(pdb, 3, phars, keep='types', pocket_ids=ids, timesteps=50, seed=5)
    assert len(out) == 3
    for sample in out:            # the given points are the first rows; the size prior may add free rows behind them
        assert len(sample) >= len(phars) and [n for n, _ in sample[:len(phars)]] == [n for n, _ in phars]
    # the same seed gives the same result (sizes given: the size prior draws them from torch's global generator, not from `seed`)
    nph = torch.tensor([len(s) for s in out])
    out2 = model.edit_phars(pdb, 3, phars, keep='types', pocket_ids=ids, num_nodes_phar=nph, timesteps=50, seed=5)
    assert out == out2
    kept = model.edit_phars(pdb, 3, phars, keep='coords', pocket_ids=ids, num_nodes_phar=torch.tensor([3, 5, 4]), timesteps=50, seed=6)
    assert [len(s) for s in kept] == [3, 5, 4]
    for sample in kept:
        for (_, xyz), (_, got) in zip(phars, sample):
            assert float(np.linalg.norm(np.asarray(got) - np.asarray(xyz))) < 0.1
    per_point = model.edit_phars(pdb, 2, phars, keep=['both', 'types', 'none'], strength=0.4, pocket_ids=ids, timesteps=50, seed=7)
    for sample in per_point:
        assert sample[0][0] == phars[0][0] and sample[1][0] == phars[1][0]
        assert float(np.linalg.norm(np.asarray(sample[0][1]) - np.asarray(phars[0][1]))) < 0.1
    with pytest.raises(ValueError, match='strength'):
        model.edit_phars(pdb, 2, phars, keep='types', strength=0.5, num_nodes_phar=5, pocket_ids=ids, timesteps=50, seed=5)
    with pytest.raises(ValueError, match='keep'):
        model.edit_phars(pdb, 2, phars, keep='type', pocket_ids=ids, timesteps=50, seed=5)
    scores = model.score_phars(pdb, out, pocket_ids=ids, timesteps=10, seed=3)
    assert tuple(scores['nll'].shape) == (3,) and bool(torch.isfinite(scores['nll']).all())
