"""GPU tests of ConditionalDDPM.inpaint / cmdgen_inpaint_chain: parity with the G20 vectors (composed from the reference's
own methods, tests/golden/make_golden_cond_inpaint.py), the reduction to the plain chain, graphs alternating with the plain
chain's on one handle, the fixed points holding, shard independence, refusals and PharPocketDDPM.inpaint_phars.

Tolerances: chains with injected noise as the G4 parity tests (coordinate RMS <= 1e-4 * max(1, max|x|), types exact;
every G20 fixture keeps its pairs >= 2e-3 A away from the cutoff); device-draw reductions bit for bit."""
import os

import numpy as np
import pytest
import torch

from functools import partial

from helpers import load_golden, cases_of, cfg_from_meta, rms, GOLDEN
from cond_inpaint_ref import inpaint_plan
from chain_kit import dev, fixed_inputs, handle_for, lightning_model, model_for, pocket_dev, run_chain, same
from cmdgen_amd import hip_backend
from cmdgen_amd.synthetic import ModelConfig, make_state_dict, make_pockets
from bench import bounded_config

pytestmark = pytest.mark.gpu

G20 = load_golden('g20_cond_inpaint.npz')
# the library's own step table (run_chain's docstring); steps are saved only where a test reads them (want_steps is part of a graph's key)
run = partial(run_chain, tables=False, want_steps=False)


def g20_case(name):
    H, L, B, R, seed, K, r, j, first = [int(v) for v in G20[name + '/meta']]
    cfg = cfg_from_meta(H, L, R)
    sd = make_state_dict(cfg, seed=seed, coord_gain=1.0)
    pb = make_pockets(B, 'CA', ragged=True, n_phar=7, first_index=first)
    return cfg, sd, pb, (K, r, j)


def run_inpaint(h, pb, phar_x, phar_oh, fixed, K, r=1, j=1, **kw):
    return run(h, pb, K, given=(phar_x, phar_oh, fixed), plan=(None, r, j), **kw)


@pytest.mark.parametrize('use_graph', [True, False])
@pytest.mark.parametrize('name', cases_of(G20))
def test_inpaint_chain_matches_g20(name, use_graph):
    cfg, sd, pb, (K, r, j) = g20_case(name)
    h = handle_for(cfg, name, sd)
    noise = dev(G20[name + '/noise'])
    assert h.inpaint_plan(K, r, j) == inpaint_plan(r, j, K)[:2]
    (xh_phar, xh_pocket, z_steps, p_steps, *_), st = run_inpaint(h, pb, G20[name + '/phar_x'], G20[name + '/phar_one_hot'],
                                                                 G20[name + '/phar_fixed'], K, r, j, noise=noise, use_graph=use_graph,
                                                                 want_steps=True)
    want = G20[name + '/xh_phar']
    assert rms(xh_phar[:, :3], want[:, :3]) <= 1e-4 * max(1.0, float(np.abs(want[:, :3]).max()))
    assert np.array_equal(xh_phar[:, 3:], want[:, 3:])
    wq = G20[name + '/xh_pocket']
    assert rms(xh_pocket, wq) <= 1e-4 * max(1.0, float(np.abs(wq).max()))
    zs, ps = G20[name + '/z_steps'], G20[name + '/pocket_steps']
    for k in range(len(zs)):
        assert float(np.abs(z_steps[k] - zs[k]).max()) <= 1e-4 * max(1.0, float(np.abs(zs[k]).max())), k
        assert float(np.abs(p_steps[k] - ps[k]).max()) <= 1e-4 * max(1.0, float(np.abs(ps[k]).max())), k
    assert st['max_rel_com_error'] < 1e-2 and st['nan_resets'] == 0


def test_python_inpaint_frames_match_g20():
    """ConditionalDDPM.inpaint with return_frames > 1: frame 0 is the final sample, the others the states at the end of the
    resample cycles, un-normalised."""
    name = 'h64_K8_r2j1'
    cfg, sd, pb, (K, r, j) = g20_case(name)
    ddpm = model_for(cfg, sd)
    nph = torch.from_numpy(pb.num_nodes_phar)
    phar = {'x': dev(G20[name + '/phar_x']), 'one_hot': dev(G20[name + '/phar_one_hot']), 'size': nph.cuda(),
            'mask': dev(np.repeat(np.arange(len(nph)), pb.num_nodes_phar))}
    F = 4
    out_phar, out_pocket, _, _ = ddpm.inpaint(phar, pocket_dev(pb), dev(G20[name + '/phar_fixed'] != 0), resamplings=r,
                                              jump_length=j, return_frames=F, timesteps=K, noise=dev(G20[name + '/noise']))
    out_phar, out_pocket = out_phar.cpu().numpy(), out_pocket.cpu().numpy()
    want = G20[name + '/xh_phar']
    assert rms(out_phar[0][:, :3], want[:, :3]) <= 1e-4 * max(1.0, float(np.abs(want[:, :3]).max()))
    assert np.array_equal(out_phar[0][:, 3:], want[:, 3:])
    last = {}
    for step, idx in ddpm.inpaint_frames(r, j, K, F):      # a later resample cycle overwrites a frame (as the joint model's inpaint)
        last[idx] = step
    assert sorted(last) == list(range(F))
    zs, ps = G20[name + '/z_steps'], G20[name + '/pocket_steps']
    for idx, step in last.items():
        if idx == 0:
            continue
        wz = np.concatenate([zs[step][:, :3], zs[step][:, 3:] * 4.0], 1)          # unnormalize_z: x * 1, h * 4
        assert float(np.abs(out_phar[idx] - wz).max()) <= 1e-4 * max(1.0, float(np.abs(wz).max())), idx
        assert float(np.abs(out_pocket[idx][:, :3] - ps[step]).max()) <= 1e-4 * max(1.0, float(np.abs(ps[step]).max())), idx


@pytest.mark.parametrize('split', [True, False])
@pytest.mark.parametrize('use_graph', [True, False])
def test_without_fixed_rows_equals_sample_chain_bit_for_bit(use_graph, split):
    """resamplings = jump_length = 1, device draws, no fixed row: the inpainting chain is the plain chain (same Philox keys for
    z_T, every posterior draw and the decode draw; k_step_count's arithmetic), on the default and the fp32 instruction engine."""
    cfg = bounded_config(20, 1000)          # the bench's weights: coordinates stay bounded, chains are bit-reproducible
    sd = make_state_dict(cfg, seed=0)
    h = hip_backend.Handle(cfg.as_dict(), 0)
    h.load_state_dict(sd)
    h.set_gemm_mode(split)
    pb = make_pockets(6, 'CA', ragged=True, first_index=300)
    nl = int(pb.num_nodes_phar.sum())
    K = 20
    (xa, qa, *_), _ = run(h, pb, K, seed=11, use_graph=use_graph)
    (xb, qb, *_), st = run_inpaint(h, pb, np.ones((nl, 3), np.float32), np.eye(8, dtype=np.float32)[np.zeros(nl, int)],
                                  np.zeros(nl), K, seed=11, use_graph=use_graph)
    assert np.array_equal(xa, xb) and np.array_equal(qa, qb)
    assert st['max_rel_com_error'] < 1e-2
    h.close()


def test_plain_and_inpaint_chains_alternate_on_one_handle():
    """sample, inpaint, sample, inpaint with graphs on one handle: each result equals its own eager run bit for bit."""
    cfg = bounded_config(20, 1000)
    sd = make_state_dict(cfg, seed=0)
    h = hip_backend.Handle(cfg.as_dict(), 0)
    h.load_state_dict(sd)
    pb = make_pockets(5, 'CA', ragged=True, first_index=500)
    px, poh, fixed, _ = fixed_inputs(pb, 0.25, np.random.default_rng(5))
    K = 17
    ref_plain = [run(h, pb, K, seed=s, use_graph=False)[0] for s in (1, 2)]
    ref_inp = [run_inpaint(h, pb, px, poh, fixed, K, seed=s, use_graph=False)[0] for s in (3, 4)]
    got = [run(h, pb, K, seed=1)[0], run_inpaint(h, pb, px, poh, fixed, K, seed=3)[0],
           run(h, pb, K, seed=2)[0], run_inpaint(h, pb, px, poh, fixed, K, seed=4)[0]]
    for g, w in zip(got, [ref_plain[0], ref_inp[0], ref_plain[1], ref_inp[1]]):
        same(g, w, ('xh_phar', 'xh_pocket'))
    h.close()


def test_graph_runs_equal_eager_runs_as_the_key_changes():
    """On one conditional handle, graph-mode plain and inpainting chains each equal their eager run bit for bit (outputs,
    saved steps, chain status) while one input of the captured graph's key changes at a time: the seed, injected noise
    against Philox draws, want_steps, graph_steps = 5 at K = 17 (three replays, two eager steps) and a caller's own stream."""
    cfg = bounded_config(20, 1000)
    h = hip_backend.Handle(cfg.as_dict(), 0)
    h.load_state_dict(make_state_dict(cfg, seed=0))
    pb = make_pockets(5, 'CA', ragged=True, first_index=500)
    px, poh, fixed, _ = fixed_inputs(pb, 0.25, np.random.default_rng(5))
    K = 17
    h.set_layout(pb.num_nodes_phar, pb.size)
    nl, n_draws = int(pb.num_nodes_phar.sum()), h.inpaint_plan(K)[1]
    rng = np.random.default_rng(6)
    noise = {'plain': dev(rng.normal(size=(K + 2, nl, 3 + cfg.phar_nf)).astype(np.float32)),
             'inpaint': dev(rng.normal(size=(n_draws, nl, 3 + cfg.phar_nf)).astype(np.float32))}
    args = {'plain': (dev(pb.x), dev(pb.one_hot)),
            'inpaint': (dev(pb.x), dev(pb.one_hot), dev(px), dev(poh), dev(np.asarray(fixed, np.float32)))}
    side = torch.cuda.Stream()

    def run(kind, use_graph, seed, inject=False, want_steps=False, on_side=False):
        chain = h.sample_chain if kind == 'plain' else h.inpaint_chain
        with torch.cuda.stream(side if on_side else torch.cuda.current_stream()):
            out = chain(*args[kind], K, noise=noise[kind] if inject else None, seed=seed, want_steps=want_steps, use_graph=use_graph)
            st = h.chain_status()
            arrays = [t.cpu().numpy() for t in out + (h.last_pocket_steps,) if t is not None]
        return arrays, (st['max_rel_com_error'], st['max_cog'], st['nan_resets'])

    variants = [dict(seed=1), dict(seed=2), dict(seed=2, inject=True), dict(seed=2, want_steps=True),
                dict(seed=2, graph_steps=5), dict(seed=2, graph_steps=5, on_side=True)]
    for v in variants:
        v = dict(v)
        if 'graph_steps' in v:
            h.set_option('graph_steps', v.pop('graph_steps'))
        graph = {kind: run(kind, True, **v) for kind in ('plain', 'inpaint')}       # the two kinds alternate on the handle
        for kind in ('plain', 'inpaint'):
            eager = run(kind, False, **v)
            assert len(graph[kind][0]) == len(eager[0]) == (4 if v.get('want_steps') else 2), (kind, v)
            for a, b in zip(graph[kind][0], eager[0]):
                assert np.array_equal(a, b), (kind, v)
            assert graph[kind][1] == eager[1], (kind, v)
    h.close()


def _check_fixed_points_hold(h, pb, K, r, j, rng):
    px, poh, fixed, pm = fixed_inputs(pb, 0.25, rng)
    (xh_phar, xh_pocket, *_), st = run_inpaint(h, pb, px, poh, fixed, K, r, j, seed=21)
    f = fixed != 0
    assert np.array_equal(xh_phar[f, 3:], poh[f])
    B = len(pb.size)
    shift = np.stack([pb.x[pb.mask == b].mean(0) - xh_pocket[pb.mask == b, :3].mean(0) for b in range(B)])
    err = np.linalg.norm(xh_phar[:, :3] + shift[pm] - px, axis=1)[f]
    assert err.max() < 0.1, err.max()
    assert st['max_rel_com_error'] < 1e-2 and st['nan_resets'] == 0


def test_fixed_points_hold():
    """64 C-alpha pockets, K = 100, a quarter of each sample's points fixed: types exact and positions relative to the pocket
    within 0.1 A (sigma_0 ~ 3.2e-3 at noise precision 1e-5, times the B draw, the decode draw and eps_x); then r = 3, j = 2."""
    cfg = ModelConfig(timesteps=500)
    h = handle_for(cfg, 'seed0', make_state_dict(cfg, seed=0))
    _check_fixed_points_hold(h, make_pockets(64, 'CA', ragged=True, first_index=1000), 100, 1, 1, np.random.default_rng(1))
    _check_fixed_points_hold(h, make_pockets(8, 'CA', ragged=True, first_index=2000), 30, 3, 2, np.random.default_rng(2))


def test_shards_reproduce_the_full_batch():
    cfg = bounded_config(20, 1000)
    h = handle_for(cfg, 'seed0', make_state_dict(cfg, seed=0))
    K = 8
    full = make_pockets(8, 'CA', ragged=True)
    px, poh, fixed, pm = fixed_inputs(full, 0.25, np.random.default_rng(3))
    (xf, *_), _ = run_inpaint(h, full, px, poh, fixed, K, 2, 1, ids=full.pocket_index)
    parts = []
    for first in (0, 4):
        sub = make_pockets(4, 'CA', ragged=True, first_index=first)
        rows = np.isin(pm, np.arange(first, first + 4))
        (xs, *_), _ = run_inpaint(h, sub, px[rows], poh[rows], fixed[rows], K, 2, 1, ids=sub.pocket_index)
        parts.append(xs)
    xs = np.concatenate(parts)
    assert np.abs(xs[:, :3] - xf[:, :3]).max() <= 1e-4 * max(1.0, np.abs(xf[:, :3]).max())
    assert np.array_equal(xs[:, 3:], xf[:, 3:])


def test_refusals():
    cfg = ModelConfig(hidden_nf=64, n_layers=1, timesteps=500)
    pb = make_pockets(2, 'CA', ragged=True)
    px, poh, fixed, _ = fixed_inputs(pb, 0.25, np.random.default_rng(4))
    joint = hip_backend.Handle(ModelConfig(hidden_nf=64, n_layers=1, update_pocket_coords=True).as_dict(), 0)
    joint.load_state_dict(make_state_dict(ModelConfig(hidden_nf=64, n_layers=1, update_pocket_coords=True), seed=0))
    with pytest.raises(hip_backend.CmdgenError, match='cmdgen_joint_chain'):
        joint.inpaint_plan(10)
    joint.set_layout(pb.num_nodes_phar, pb.size)
    with pytest.raises(hip_backend.CmdgenError, match='cmdgen_joint_chain'):
        run_inpaint(joint, pb, px, poh, fixed, 10)
    joint.close()
    simple_cfg = ModelConfig(hidden_nf=64, n_layers=1, timesteps=500, no_com_projection=True)
    simple = hip_backend.Handle(simple_cfg.as_dict(), 0)
    simple.load_state_dict(make_state_dict(simple_cfg, seed=0))
    with pytest.raises(hip_backend.CmdgenError, match='SimpleConditionalDDPM'):
        simple.inpaint_plan(10)
    simple.close()
    h = handle_for(cfg, 'seed0', make_state_dict(cfg, seed=0))
    n_steps, n_draws = h.inpaint_plan(10, 2, 1)
    short = torch.zeros((n_draws - 1, int(pb.num_nodes_phar.sum()), 11), device='cuda')
    with pytest.raises(hip_backend.CmdgenError, match='draws'):
        run_inpaint(h, pb, px, poh, fixed, 10, 2, 1, noise=short)
    with pytest.raises(hip_backend.CmdgenError):
        h.inpaint_plan(10, 0, 1)
    ddpm = model_for(cfg, make_state_dict(cfg, seed=0))
    nl = int(pb.num_nodes_phar.sum())
    phar = {'x': dev(px), 'one_hot': dev(poh), 'size': dev(pb.num_nodes_phar),
            'mask': dev(np.repeat(np.arange(2), pb.num_nodes_phar))}
    with pytest.raises(ValueError, match='draws'):
        ddpm.inpaint(phar, pocket_dev(pb), dev(fixed), resamplings=2, timesteps=10, noise=short)
    with pytest.raises(ValueError, match='phar_fixed'):
        ddpm.inpaint(phar, pocket_dev(pb), torch.ones(nl + 1, device='cuda'), timesteps=10)
    with pytest.raises(ValueError, match='jump_length'):
        ddpm.inpaint(phar, pocket_dev(pb), dev(fixed), jump_length=2, return_frames=2, timesteps=10)


def test_inpaint_phars_end_to_end():
    """PharPocketDDPM.inpaint_phars on the g7 pocket (30 C-alpha residues): the given types appear at the given points (back in
    the PDB frame), and the same seed gives the same result."""
    model = lightning_model()
    pdb = os.path.join(GOLDEN, 'g7_pocket.pdb')
    ids = [f'A:{i}' for i in range(1, 30)]
    names = list(model.dataset_info['phar_decoder'])
    fixed = [(names[1], (9.0, 2.0, -15.0)), (names[3], (11.5, 4.0, -13.0))]
    out = model.inpaint_phars(pdb, 3, fixed, pocket_ids=ids, num_nodes_phar=torch.tensor([6, 7, 5]), timesteps=50, seed=5)
    for name, xyz in fixed:          # every sample holds each given point with its type (the dict groups points by index and type)
        near = [c for m in out.values() for c in m.get(name, []) if float(np.linalg.norm(c.numpy() - np.asarray(xyz))) < 0.1]
        assert len(near) == 3
    out2 = model.inpaint_phars(pdb, 3, fixed, pocket_ids=ids, num_nodes_phar=torch.tensor([6, 7, 5]), timesteps=50, seed=5)
    a = torch.stack([c for k in sorted(out) for t in sorted(out[k]) for c in out[k][t]])
    b = torch.stack([c for k in sorted(out2) for t in sorted(out2[k]) for c in out2[k][t]])
    assert torch.equal(a, b)
    with pytest.raises(ValueError, match='num_nodes_phar'):
        model.inpaint_phars(pdb, 1, fixed, pocket_ids=ids, num_nodes_phar=torch.tensor([1]), timesteps=5, seed=5)
    torch.manual_seed(0)
    out3 = model.inpaint_phars(pdb, 2, fixed, pocket_ids=ids, timesteps=10, seed=6)      # size prior, clamped to >= 2
    assert f'Molecule_{len(fixed)}' in out3
