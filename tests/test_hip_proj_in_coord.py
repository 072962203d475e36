"""Option "proj_in_coord" (include/cmdgen_hip.h; kernels_coord_proj.hip): the next block's P | Q projections as tiles of the coordinate launch
instead of inside k_node16w.  Every P / Q element sees the same MFMAs in the same order from the same fp32 h, so at the headline layout - where
the chain itself is reproducible bit for bit (test_chains_are_reproducible_bit_for_bit) - option 1 and option 0 must give identical bits."""
import dataclasses

import numpy as np
import pytest
import torch

from helpers import load_golden, cases_of, dynamics_case
from cmdgen_amd import hip_backend
from cmdgen_amd.synthetic import make_state_dict, make_pockets
from bench import bounded_config
from chain_kit import dev
from helpers import EVAL_TOL, eval_inputs, forward, handle_with_layout as handle_for, new_handle

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda')
G2 = load_golden('g2_dynamics.npz')


def headline(B=64):
    cfg = bounded_config(20, 1000)
    return cfg, make_state_dict(cfg, seed=0), make_pockets(B, 'CA')


@pytest.mark.parametrize('half', [1, 0], ids=['half_engine', 'three_piece_engine'])
def test_option_1_against_option_0_bit_for_bit_at_the_headline_layout(half):
    cfg, sd, pb = headline()
    xh, xq, t = eval_inputs(pb, cfg)
    px, poh = torch.from_numpy(pb.x).to(DEV), torch.from_numpy(pb.one_hot).to(DEV)
    got = {}
    for on in (0, 1):
        h = handle_for(cfg, sd, pb)
        if not half:
            h.set_option('half_engine', 0)
        h.set_option('proj_in_coord', on)
        assert h.query('proj_in_coord') == on and h.query('node_mfmas_per_product') == (3 if half else 6)
        res = [forward(h, xh, xq, t)]
        for graph in (True, False):
            x, xp, zs = h.sample_chain(px, poh, 16, seed=9, pocket_ids=pb.pocket_index, want_steps=True, use_graph=graph)
            res += [x.cpu().numpy(), xp.cpu().numpy(), zs.cpu().numpy()]
        assert h.chain_status()['nan_resets'] == 0
        h.close()
        got[on] = res
    for a, b in zip(got[0], got[1]):
        assert np.isfinite(a).all() and np.array_equal(a, b)


def test_g2_fixtures_with_the_projection_tiles_forced():
    """Every H = 256 fixture on the launches the rule asks for (16-row eight-wave node tiles, 32-row full-K coordinate tiles) with option 1: inside
    the evaluation tolerance of the reference, and as close to option 0 as two runs of option 0 are to each other (the segment sums upstream
    add tile partials with float atomics: test_eight_wave_node_tile_against_the_four_wave_one)."""
    took = 0
    for name in [n for n in cases_of(G2) if '_h256_' in n]:
        cfg, sd, inp = dynamics_case(G2, name)
        want = G2[name + '/eps_phar']
        got = []
        for on in (1, 0, 0):
            h = new_handle(cfg, sd)
            h.set_option('node_mt', 16); h.set_option('node64', 0); h.set_option('coord_mt', 32); h.set_option('proj_in_coord', on)
            h.set_layout(G2[name + '/num_nodes_phar'], G2[name + '/pocket_size'])
            assert h.query('node_mt') == 16 and h.query('coord_mt') == 32
            if on:
                took += h.query('proj_in_coord')
            else:
                assert h.query('proj_in_coord') == 0
            eps, _ = h.dynamics_forward(dev(inp['xh_phar']), dev(inp['xh_pocket']), dev(inp['t']))
            got.append(eps.cpu().numpy())
            h.close()
        scale = max(1.0, float(np.abs(want).max()))
        run_to_run = float(np.abs(got[1] - got[2]).max())
        assert float(np.abs(got[0] - got[1]).max()) <= max(4.0 * run_to_run, 2e-6 * scale), name
        for g in got:
            assert float(np.abs(g - want).max()) <= EVAL_TOL * scale, name
    assert took > 0           # (the fixtures with more than one block take the merged launch)


def test_where_the_rule_resolves_to_the_projection_tiles():
    cfg, sd, pb = headline()
    h = handle_for(cfg, sd, pb)
    assert h.get_option('proj_in_coord') is None and h.query('proj_in_coord') == 1
    h.set_option('node16w', 0)
    assert h.query('proj_in_coord') == 0
    h.set_option('node16w', None)
    assert h.query('proj_in_coord') == 1
    h.set_option('proj_in_coord', 0)
    assert h.query('proj_in_coord') == 0
    h.close()
    big = make_pockets(256, 'CA')
    h = handle_for(cfg, sd, big)
    assert h.query('proj_in_coord') == 0
    h.set_option('proj_in_coord', 1)                  # 1 = wherever the launches allow it: never on 64-row node tiles / 128-row coordinate tiles
    assert h.query('proj_in_coord') == 0
    h.close()
    for change in (dict(update_pocket_coords=True), dict(inv_sublayers=2)):
        c2 = dataclasses.replace(cfg, **change)
        h = handle_for(c2, make_state_dict(c2, seed=0), pb)
        assert h.query('proj_in_coord') == 0
        h.set_option('proj_in_coord', 1)
        assert h.query('proj_in_coord') == 0
        h.close()


def test_setting_the_option_drops_the_captured_graph():
    cfg, sd, pb = headline()
    px, poh = torch.from_numpy(pb.x).to(DEV), torch.from_numpy(pb.one_hot).to(DEV)
    h = handle_for(cfg, sd, pb)

    def chain():
        x, _, _ = h.sample_chain(px, poh, 12, seed=3, pocket_ids=pb.pocket_index)
        return x.cpu().numpy()
    h.set_option('proj_in_coord', 0)
    base = chain()
    assert h.query('chain_graphs') == 1
    h.set_option('proj_in_coord', 1)                  # the graph captured above holds k_edge_coord and the full node tile: it must not be replayed
    assert h.query('chain_graphs') == 0
    on = chain()
    assert h.query('chain_graphs') == 1               # the launches were issued (and captured) again
    h.set_option('proj_in_coord', 0)
    assert h.query('chain_graphs') == 0
    off = chain()
    h.set_option('proj_in_coord', None)
    auto = chain()
    h.close()
    assert np.isfinite(base).all()
    for other in (on, off, auto):
        assert np.array_equal(base, other)
