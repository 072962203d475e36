"""Option "readout_in_coord" (include/cmdgen_hip.h; kernels_coord_proj.hip, kernels_ddpm.hip): the plain sampling chain without k_readout - its
feature part as tiles of the last block's coordinate launch (the same device function), the velocity and the batch-global NaN flag formed by their
consumer (the same expression), X0 / ACC of the phar rows stored by pass 2 of the radius graph instead of the step kernel (the same values).  Every
number is produced by the operations that produced it before, so option 1 and option 0 give identical bits wherever the chain itself is
reproducible bit for bit."""
import dataclasses

import numpy as np
import pytest
import torch

from cmdgen_amd import hip_backend
from cmdgen_amd.synthetic import make_state_dict, make_pockets
from bench import bounded_config
from chain_kit import dev
from helpers import handle_with_layout as handle_for, host_step_table, small_case

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda')
SMALL = dict(node_mt=16, node64=0, coord_mt=32)        # the launches the rule asks for at the headline, forced on the small layouts
_shared = {}


def model():
    if 'model' not in _shared:
        cfg = bounded_config(20, 1000)
        _shared['model'] = (cfg, make_state_dict(cfg, seed=0))
    return _shared['model']


def layout(name):
    """1x8: one full readout tile, Nl smaller than a workgroup; ragged3: a one-node sample, a partial last readout tile (17 rows), a ragged scan;
    20x3: the driver shape; 64x15: the headline."""
    if name == '1x8':
        return make_pockets(1, 'CA', n_phar=8, first_index=40)
    if name == 'ragged3':
        pb = make_pockets(3, 'CA', ragged=True, first_index=50)
        return dataclasses.replace(pb, num_nodes_phar=np.array([1, 9, 7], dtype=np.int64))
    if name == '20x3':
        return make_pockets(20, 'CA', n_phar=3)
    return make_pockets(64, 'CA')


def new_handle(cfg, sd, pb, engine, small, on, other=None):
    h = handle_for(cfg, sd, pb)
    if engine == 'bf3':
        h.set_option('half_engine', 0)
    if small:
        for k, v in SMALL.items():
            h.set_option(k, v)
    if other:
        for k, v in other.items():
            h.set_option(k, v)
    h.set_option('readout_in_coord', on)
    return h


def status_of(h):
    st = h.chain_status()
    return [st['max_rel_com_error'], st['max_cog'], st['nan_resets']]


def plain_chains(h, pb, K, noise):
    """graph and eager runs on device draws and on injected noise -> flat list of arrays (final xh_phar, xh_pocket, z_steps, status, nan_resets)"""
    px, poh = dev(pb.x), dev(pb.one_hot)
    out = []
    for graph in (True, False):
        for nz in (None, noise):
            x, xp, zs = h.sample_chain(px, poh, K, noise=nz, seed=9, pocket_ids=pb.pocket_index, want_steps=True, use_graph=graph)
            out += [x.cpu().numpy(), xp.cpu().numpy(), zs.cpu().numpy(), np.asarray(status_of(h), np.float64),
                    np.asarray([h.counters()['nan_resets']])]
    return out


CASES = [('1x8', 'half'), ('ragged3', 'half'), ('ragged3', 'bf3'), ('20x3', 'half'), ('64x15', 'half'), ('64x15', 'bf3')]
LOOSE = ('ragged3', 'bf3')          # the one case that may be held to the run-to-run form (three-piece engine on 16-row fp32 edge tiles)


@pytest.mark.parametrize('name, engine', CASES, ids=['%s-%s' % c for c in CASES])
def test_option_1_against_option_0_bit_for_bit(name, engine):
    cfg, sd = model()
    pb = layout(name)
    small = name != '64x15'
    K = 12 if small else 16           # (graph_steps 8: one replayed graph and an eager remainder)
    Nl = int(pb.num_nodes_phar.sum())
    noise = dev(np.random.Generator(np.random.PCG64(5)).normal(size=(K + 2, Nl, 3 + cfg.phar_nf)).astype(np.float32))
    got = []
    for on in (0, 0, 1):
        h = new_handle(cfg, sd, pb, engine, small, on)
        assert h.query('readout_in_coord') == on and h.query('coord_mt') == 32
        assert h.query('coord_mfmas_per_product') == (3 if engine == 'half' else 6)
        got.append(plain_chains(h, pb, K, noise))
        h.close()
    reproducible = all(np.array_equal(a, b) for a, b in zip(got[0], got[1]))
    print(f'\n[{name} {engine}] option 0 reproduces itself: {reproducible}')
    assert reproducible or (name, engine) == LOOSE
    for a, a2, b in zip(got[0], got[1], got[2]):
        assert np.isfinite(a).all()
        if reproducible:
            assert np.array_equal(a, b)
        else:
            run_to_run = float(np.abs(a - a2).max())
            diff = float(np.abs(a - b).max())
            print(f'   run to run {run_to_run:.3e}  option 1 against option 0 {diff:.3e}')
            assert diff <= max(4.0 * run_to_run, 2e-6 * max(1.0, float(np.abs(a).max())))


@pytest.mark.parametrize('use_graph', [True, False], ids=['graph', 'eager'])
def test_the_batch_global_reset(use_graph):
    """The chain of test_mean_zero_assertion_fires_like_reference (small_case, one inf in one sample's injected draw of step 2) at hidden_nf 256 on
    the forced launches, where the option resolves to 1.  The NaN reaches one sample's positions; the reference zeroes the velocity of EVERY sample
    in that evaluation (dynamics.py:129-131), so the other samples' states show whether each workgroup found the flag on its own.
    The messages run on the headline's 128-row kernel: on the 16-row fp32 tiles this size would get, a receiver's sum is three or more float-atomic
    partials in the order the hardware picks, and option 0 does not reproduce ITSELF bit for bit (measured: 6e-5 on |z| ~ 600 between two runs)."""
    cfg, _, pb, K, noise = small_case(seed=92)
    cfg = dataclasses.replace(cfg, hidden_nf=256)
    sd = make_state_dict(cfg, seed=92, coord_gain=1e-3)
    noise[2, 5, 1] = np.inf
    got = {}
    for on in (0, 1, 2):                                # (2: option 0 once more - the premise of a comparison bit for bit)
        h = new_handle(cfg, sd, pb, 'half', True, on & 1, {'edge_mt': 128})
        assert h.query('readout_in_coord') == on & 1 and h.query('edge_mt') == 128
        h.set_step_table(K, host_step_table(cfg, K))
        x, xp, zs = h.sample_chain(dev(pb.x), dev(pb.one_hot), K, noise=dev(noise), want_steps=True, use_graph=use_graph)
        st = h.chain_status()
        got[on] = [x.cpu().numpy(), xp.cpu().numpy(), zs.cpu().numpy(), np.asarray([st['max_rel_com_error'], st['max_cog']]), st['nan_resets']]
        h.close()
    assert got[0][4] >= 1 and got[0][4] == got[1][4]
    assert np.isnan(got[0][3][0])
    sample_of = np.repeat(np.arange(len(pb.size)), pb.num_nodes_phar)
    hit = sample_of == sample_of[5]
    assert np.isfinite(got[0][2][:, ~hit]).all() and not np.isfinite(got[0][2][:, hit]).all()      # (the other samples stay finite)
    for a, b, a2 in zip(got[0][:4], got[1][:4], got[2][:4]):
        assert np.array_equal(a, a2, equal_nan=True)
        assert np.array_equal(a, b, equal_nan=True)


def test_where_the_option_resolves():
    cfg, sd = model()
    pb = layout('64x15')
    h = handle_for(cfg, sd, pb)
    assert h.get_option('readout_in_coord') is None and h.query('readout_in_coord') == 1
    h.set_option('readout_in_coord', 0)
    assert h.query('readout_in_coord') == 0
    h.set_option('readout_in_coord', 1)
    assert h.query('readout_in_coord') == 1
    h.set_option('readout_in_coord', None)
    h.set_gemm_mode(False)                              # the fp32 engine has no full-K coordinate tile
    assert h.query('readout_in_coord') == 0
    h.set_option('readout_in_coord', 1)
    assert h.query('readout_in_coord') == 0
    h.close()
    h = handle_for(cfg, sd, make_pockets(32, 'CA'))
    assert h.query('readout_in_coord') == 1
    h.close()
    h = handle_for(cfg, sd, make_pockets(256, 'CA'))
    assert h.query('readout_in_coord') == 0
    h.set_option('readout_in_coord', 1)                # 1 = wherever the launches allow it: never beside 128-row coordinate tiles
    assert h.query('readout_in_coord') == 0
    h.close()
    for change in (dict(update_pocket_coords=True), dict(inv_sublayers=2), dict(hidden_nf=128)):
        c2 = dataclasses.replace(cfg, **change)
        h = handle_for(c2, make_state_dict(c2, seed=0), pb)
        assert h.query('readout_in_coord') == 0
        h.set_option('readout_in_coord', 1)
        assert h.query('readout_in_coord') == 0
        h.close()


def test_setting_the_option_drops_the_captured_graph():
    cfg, sd = model()
    pb = layout('64x15')
    px, poh = dev(pb.x), dev(pb.one_hot)
    h = handle_for(cfg, sd, pb)

    def chain():
        x, _, _ = h.sample_chain(px, poh, 12, seed=3, pocket_ids=pb.pocket_index)
        return x.cpu().numpy()
    h.set_option('readout_in_coord', 0)
    base = chain()
    assert h.query('chain_graphs') == 1
    h.set_option('readout_in_coord', 1)               # the graph captured above holds k_readout and the storing step kernel: it must not be replayed
    assert h.query('chain_graphs') == 0
    on = chain()
    assert h.query('chain_graphs') == 1
    h.set_option('readout_in_coord', 0)
    assert h.query('chain_graphs') == 0
    off = chain()
    h.set_option('readout_in_coord', None)
    auto = chain()
    h.close()
    assert np.isfinite(base).all()
    for other in (on, off, auto):
        assert np.array_equal(base, other)


def test_the_other_chains_are_unaffected():
    """The inpainting chain and the multi-pocket chain keep k_readout and their own step kernels: with the option at 1 (and resolving to 1 for the
    plain chain on this layout) they give the bits they give with it at 0 - also right after a plain chain that ran without k_readout."""
    cfg, sd = model()
    pb = make_pockets(3, 'CA', n_phar=5, first_index=60)
    Nl = int(pb.num_nodes_phar.sum())
    rng = np.random.Generator(np.random.PCG64(8))
    phar_x = (rng.normal(size=(Nl, 3)) * 2.0).astype(np.float32)
    phar_oh = np.eye(cfg.phar_nf, dtype=np.float32)[rng.integers(0, cfg.phar_nf, size=Nl)]
    fixed = (np.arange(Nl) % 3 == 0).astype(np.float32)
    px, poh = dev(pb.x), dev(pb.one_hot)
    got = {}
    for on in (0, 1):
        h = new_handle(cfg, sd, pb, 'half', True, on)
        assert h.query('readout_in_coord') == on
        res = []
        for graph in (True, False):
            x, _, _ = h.sample_chain(px, poh, 6, seed=4, pocket_ids=pb.pocket_index, use_graph=graph)
            out = h.inpaint_chain(px, poh, dev(phar_x), dev(phar_oh), dev(fixed), 6, seed=4, pocket_ids=pb.pocket_index, want_steps=True,
                                  use_graph=graph)
            res += [x.cpu().numpy()] + [o.cpu().numpy() for o in out]
            out = h.multi_pocket_chain(px, poh, [2, 1], [0.5, 0.5, 1.0], 6, seed=4, want_steps=True, use_graph=graph)
            res += [o.cpu().numpy() for o in out] + [h.last_pocket_steps.cpu().numpy()]
        assert h.chain_status()['nan_resets'] == 0
        h.close()
        got[on] = res
    for a, b in zip(got[0], got[1]):
        assert np.isfinite(a).all() and np.array_equal(a, b)
