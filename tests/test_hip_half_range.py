"""The half matrix engine's range (round 6; cmdgen_split.h: two fp16 pieces per operand) - both ends of it.

An activation beyond fp16's 65504 becomes Inf, its second piece -Inf, the product NaN - and the evaluation's NaN guard turns that into a
batch-global reset step which the fp32 reference (whose activations stay finite) never takes.  These tests DRIVE such activations through each of
the half-engine tile kernels - k_edge128<msg>, k_edge128<coord>, the 32-row full-K edge tiles, k_node64, k_node16w - with weight sets whose
oracle output is finite, and check the library's contract:

  * the raw C-ABI call on a half-engine handle does reset (the overflow is real: the test reaches the path it is about) and reports it
    (cmdgen_counters.nan_resets / cmdgen_chain_status);
  * the Python mirror (hip_backend.Handle.run_range_guarded, used by EGNNDynamics.forward and by every chain entry point) never returns that
    result: it repeats the call on the three-piece bf16 split engine (fp32's exponent range), warns, and the output equals the ORACLE's within
    the evaluation tolerance.

The LOW end fails without a NaN: a row of activations all below 2^-3 has subnormal second pieces and loses fp32 accuracy.  underflow_case scales a
first layer by s and its second layer by 1 / s - the half GEMM's A operand sits at scale s, the output stays O(1) - and the tests check that the
raw call is wrong by more than the tolerance (the test reaches the defect) and counts the rows (cmdgen_counters.half_low_range), and that the guard
repeats it on the bf16 split engine with a warning of its own.
"""
import warnings

import numpy as np
import pytest
import torch

from helpers import dynamics_case
from cmdgen_amd import hip_backend
from chain_kit import dev
from helpers import (EVAL_TOL, RANGE_NAME as NAME, RANGE_TARGETS as TARGETS, g2, host_step_table, new_handle,
                     overflow_case, underflow_case)

pytestmark = pytest.mark.gpu

G2 = g2()

# launch choices that put the three tile kernels on each half-engine family
OPTION_SETS = {
    'rows128_node64': dict(edge_mt=128, coord_mt=128, node64=1, e128_fused=0),
    'rows128_fused': dict(edge_mt=128, coord_mt=128, node64=1, e128_fused=3),
    'fullk32_node16w': dict(edge_mt=32, coord_mt=32, node_mt=16),
    # the plane node tiles the launcher picks on the half engine (k_node32p, k_node64e, k_node64d), beside the full-K 32-row edge tiles
    'fullk32_node32p': dict(edge_mt=32, coord_mt=32, node64=32),
    'fullk32_node64e': dict(edge_mt=32, coord_mt=32, node64=8),
    'fullk32_node64d': dict(edge_mt=32, coord_mt=32, node64=2),
}
LOW_SCALES = [2.0 ** -6, 2.0 ** -10, 2.0 ** -14]
# the smallest scale per target at which the raw half-engine call misses the oracle by more than the tolerance: the message MLP's error is
# diluted by the aggregation (sum / normalization_factor) - at 2^-14 its raw error is 4.8e-7, at the fp32 floor - so it is driven to 2^-22
SMALLEST = {'msg': 2.0 ** -22, 'coord': 2.0 ** -14, 'node': 2.0 ** -14}


def oracle_eps(cfg, sd, inp):
    from oracle import ref_cpu
    p = ref_cpu.to_torch_params(sd)
    with torch.no_grad():
        want, _ = ref_cpu.dynamics_forward(p, cfg.as_dict(), torch.from_numpy(inp['xh_phar']), torch.from_numpy(inp['xh_pocket']), torch.from_numpy(inp['t']),
                                           torch.from_numpy(inp['mask_phar']), torch.from_numpy(inp['mask_pocket']))
    return want.numpy()


def assert_tiles(h, target, optset):
    assert h.query({'msg': 'msg_mfmas_per_product', 'coord': 'coord_mfmas_per_product', 'node': 'node_mfmas_per_product'}[target]) == 3, \
        'the targeted kernel must run on the half engine for this test to mean anything'
    if 'node64' in OPTION_SETS[optset]:
        assert h.query('node64') == OPTION_SETS[optset]['node64']


@pytest.mark.parametrize('optset', list(OPTION_SETS))
@pytest.mark.parametrize('target', list(TARGETS))
def test_overflowing_activation_is_rerun_not_reset(target, optset, monkeypatch):
    for k, v in OPTION_SETS[optset].items():
        monkeypatch.setitem(hip_backend.DEFAULT_OPTIONS, k, v)
    cfg, sd, inp = overflow_case(target)
    want = oracle_eps(cfg, sd, inp)
    assert np.isfinite(want).all() and np.abs(want[:, :3]).max() > 0, 'the oracle must stay finite and take no reset'
    nl, npk = G2[NAME + '/num_nodes_phar'], G2[NAME + '/pocket_size']
    h = new_handle(cfg, sd)
    h.set_layout(nl, npk)
    assert h.half_engine_active()
    assert_tiles(h, target, optset)
    xp, xq, t = dev(inp['xh_phar']), dev(inp['xh_pocket']), dev(inp['t'])
    # 1. the raw C-ABI call: the half engine overflows, the guard resets the batch and counts it
    h.reset_counters()
    eps, _ = h.dynamics_forward(xp, xq, t)
    torch.cuda.synchronize()
    assert h.counters()['nan_resets'] == 1, 'expected the fp16 overflow to surface as a NaN reset on the raw half-engine call'
    assert np.all(eps.cpu().numpy()[:, :3] == 0.0)
    # 2. the mirror's guard: re-run on the bf16 split engine, warning, oracle-equal output
    seen = [h.nan_resets_total()]

    def status():
        now = h.nan_resets_total()
        d, seen[0] = now - seen[0], now
        return {'nan_resets': d}
    with pytest.warns(RuntimeWarning, match='half matrix engine'):
        (eps2, _p), st = h.run_range_guarded(lambda: h.dynamics_forward(xp, xq, t), status)
    torch.cuda.synchronize()
    got = eps2.cpu().numpy()
    assert st.get('half_engine_fallback') and st['nan_resets'] == 0
    assert h.half_engine_active(), 'the handle goes back to its own engine choice after the guarded call'
    tol = EVAL_TOL * max(1.0, float(np.abs(want).max()))
    err = float(np.abs(got - want).max())
    print(f'{target} / {optset}: |eps| max {np.abs(want).max():.3e}, guarded call vs oracle {err:.2e} (tolerance {tol:.1e})')
    assert np.isfinite(got).all() and err <= tol
    h.close()


def test_mirror_forward_equals_the_oracle_on_an_overflowing_model():
    """EGNNDynamics.forward (the reference's module interface) on a model whose message MLP overflows fp16: oracle-equal output, no reset."""
    from cmdgen_amd.equivariant_diffusion.dynamics import EGNNDynamics
    cfg, sd, inp = overflow_case('msg')
    want = oracle_eps(cfg, sd, inp)
    c = cfg.as_dict()
    dyn = EGNNDynamics(phar_nf=c['phar_nf'], residue_nf=c['residue_nf'], n_dims=3, joint_nf=c['joint_nf'], hidden_nf=c['hidden_nf'],
                       n_layers=c['n_layers'], attention=c['attention'], tanh=c['tanh'], norm_constant=c['norm_constant'],
                       inv_sublayers=c.get('inv_sublayers', 1), sin_embedding=False, normalization_factor=c['normalization_factor'],
                       aggregation_method=c.get('aggregation_method', 'sum'), update_pocket_coords=False, edge_cutoff=c['edge_cutoff'])
    state = {k[len('ddpm.dynamics.'):]: torch.from_numpy(np.asarray(v)) for k, v in sd.items() if k.startswith('ddpm.dynamics.')}
    dyn.load_state_dict(state)
    dyn = dyn.cuda()
    with pytest.warns(RuntimeWarning, match='half matrix engine'), torch.no_grad():
        eps, _ = dyn(dev(inp['xh_phar']), dev(inp['xh_pocket']), dev(inp['t']), dev(inp['mask_phar']), dev(inp['mask_pocket']))
    got = eps.cpu().numpy()
    assert np.isfinite(got).all() and np.abs(got - want).max() <= EVAL_TOL * max(1.0, float(np.abs(want).max()))


def test_chain_on_an_overflowing_model_equals_the_bf16_engine_chain():
    """A short chain: the guarded call returns exactly what a handle with half_engine = 0 returns (same draws), reports no reset and warns;
    a model inside the range takes the half engine's result and does not warn."""
    from cmdgen_amd.synthetic import make_pockets
    cfg, sd, _ = overflow_case('msg')
    pb = make_pockets(8, 'CA', n_phar=8)
    K = 6
    px, poh = dev(pb.x), dev(pb.one_hot)

    def run_on(h):
        return lambda: h.sample_chain(px, poh, K, noise=None, seed=5, pocket_ids=pb.pocket_index, use_graph=True)
    ref = new_handle(cfg, sd)
    ref.set_option('half_engine', 0)
    ref.set_layout(pb.num_nodes_phar, pb.size)
    ref.set_step_table(K, host_step_table(cfg, K))
    want = ref.sample_chain(px, poh, K, noise=None, seed=5, pocket_ids=pb.pocket_index, use_graph=True)[0].cpu().numpy()
    ref_resets = ref.chain_status()['nan_resets']
    ref.close()
    h = new_handle(cfg, sd)
    h.set_layout(pb.num_nodes_phar, pb.size)
    h.set_step_table(K, host_step_table(cfg, K))
    assert h.half_engine_active()
    raw = run_on(h)()
    assert h.chain_status()['nan_resets'] >= 1, 'the raw half-engine chain is expected to reset on this model'
    del raw
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter('always')
        (xh, _q, _z), st = h.run_range_guarded(run_on(h), h.chain_status)
    got = xh.cpu().numpy()
    assert st['nan_resets'] == ref_resets and st.get('half_engine_fallback')
    if ref_resets == 0:
        assert any('half matrix engine' in str(x.message) for x in w)
    # (the two handles may pick other tiles - the choice depends on the engine - so sums differ in their last bits: the evaluation tolerance, types exact)
    assert np.abs(got[:, :3] - want[:, :3]).max() <= EVAL_TOL * max(1.0, float(np.abs(want[:, :3]).max())) and np.array_equal(got[:, 3:], want[:, 3:])
    h.close()
    # inside the range: no second run, no warning
    cfg2, sd2, _ = dynamics_case(G2, NAME)
    h2 = new_handle(cfg2, sd2)
    h2.set_layout(pb.num_nodes_phar, pb.size)
    h2.set_step_table(K, host_step_table(cfg2, K))
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        _out, st2 = h2.run_range_guarded(run_on(h2), h2.chain_status)
    assert st2['nan_resets'] == 0 and 'half_engine_fallback' not in st2
    h2.close()


def low_range_model_handle(cfg, sd, nl, npk, half=True):
    h = new_handle(cfg, sd)
    if not half:
        h.set_option('half_engine', 0)
    h.set_layout(nl, npk)
    return h


@pytest.mark.parametrize('optset', list(OPTION_SETS))
@pytest.mark.parametrize('target', list(TARGETS))
def test_low_range_activation_is_rerun_on_the_bf16_engine(target, optset, monkeypatch):
    """Activations at scale s = 2^-6, 2^-10, 2^-14 (and SMALLEST) in the targeted kernel's A operand: the raw half-engine call is wrong beyond
    the evaluation tolerance at the smallest s and counts the rows, without a NaN reset; the guarded call equals the oracle at every s, falls
    back exactly when rows were counted and warns exactly when it fell back."""
    for k, v in OPTION_SETS[optset].items():
        monkeypatch.setitem(hip_backend.DEFAULT_OPTIONS, k, v)
    nl, npk = G2[NAME + '/num_nodes_phar'], G2[NAME + '/pocket_size']
    report = []
    scales = sorted(set(LOW_SCALES + [SMALLEST[target]]), reverse=True)
    for s in scales:
        cfg, sd, inp = underflow_case(target, s)
        want = oracle_eps(cfg, sd, inp)
        assert np.isfinite(want).all(), 'the oracle must stay finite'
        tol = EVAL_TOL * max(1.0, float(np.abs(want).max()))
        xp, xq, t = dev(inp['xh_phar']), dev(inp['xh_pocket']), dev(inp['t'])
        # the case is well posed: the three-piece bf16 engine gets the oracle's output
        ref = low_range_model_handle(cfg, sd, nl, npk, half=False)
        assert not ref.half_engine_active()
        ref_eps, _ = ref.dynamics_forward(xp, xq, t)
        ref_err = float(np.abs(ref_eps.cpu().numpy() - want).max())
        ref.close()
        assert ref_err <= tol, f's = {s}: the bf16 split engine misses the oracle ({ref_err:.2e} > {tol:.1e})'
        h = low_range_model_handle(cfg, sd, nl, npk)
        assert h.half_engine_active()
        assert_tiles(h, target, optset)
        # the raw C-ABI call
        h.reset_counters()
        raw, _ = h.dynamics_forward(xp, xq, t)
        torch.cuda.synchronize()
        raw_err = float(np.abs(raw.cpu().numpy() - want).max())
        c = h.counters()
        assert c['nan_resets'] == 0, 'the low end of the range takes no NaN reset'
        if s == SMALLEST[target]:
            assert raw_err > tol, f'the raw half-engine call should miss the oracle at s = {s} (error {raw_err:.2e}, tolerance {tol:.1e})'
            assert c['half_low_range'] >= 1, 'the rows below the half engine\'s range must be counted'
        # the guard
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter('always')
            (eps, _p), st = h.run_range_guarded(lambda: h.dynamics_forward(xp, xq, t), dict)
        torch.cuda.synchronize()
        got = eps.cpu().numpy()
        err = float(np.abs(got - want).max())
        fell_back = bool(st.get('half_engine_fallback'))
        warned = [x for x in w if issubclass(x.category, RuntimeWarning) and 'precision range' in str(x.message)]
        assert bool(warned) == fell_back, 'a warning exactly when the call was repeated'
        assert fell_back == (c['half_low_range'] > 0), 'the guard repeats exactly the calls that counted rows below the range'
        assert st['nan_resets'] == 0
        assert h.half_engine_active(), 'the handle goes back to its own engine choice after the guarded call'
        h.close()
        report.append(f's=2^{int(np.log2(s))}: raw {raw_err:.2e} (rows {c["half_low_range"]}), guarded {err:.2e}{" (fallback)" if fell_back else ""}')
        assert np.isfinite(got).all() and err <= tol, f's = {s}: guarded call vs oracle {err:.2e} > {tol:.1e}'
    print(f'{target} / {optset}: ' + '; '.join(report))


def test_mirror_forward_equals_the_oracle_on_a_low_range_model():
    """EGNNDynamics.forward on a model whose message MLP works at 2^-14: the mirror's guard repeats the call, warns, and gets the oracle's output."""
    from cmdgen_amd.equivariant_diffusion.dynamics import EGNNDynamics
    cfg, sd, inp = underflow_case('msg', LOW_SCALES[-1])
    want = oracle_eps(cfg, sd, inp)
    c = cfg.as_dict()
    dyn = EGNNDynamics(phar_nf=c['phar_nf'], residue_nf=c['residue_nf'], n_dims=3, joint_nf=c['joint_nf'], hidden_nf=c['hidden_nf'],
                       n_layers=c['n_layers'], attention=c['attention'], tanh=c['tanh'], norm_constant=c['norm_constant'],
                       inv_sublayers=c.get('inv_sublayers', 1), sin_embedding=False, normalization_factor=c['normalization_factor'],
                       aggregation_method=c.get('aggregation_method', 'sum'), update_pocket_coords=False, edge_cutoff=c['edge_cutoff'])
    state = {k[len('ddpm.dynamics.'):]: torch.from_numpy(np.asarray(v)) for k, v in sd.items() if k.startswith('ddpm.dynamics.')}
    dyn.load_state_dict(state)
    dyn = dyn.cuda()
    with pytest.warns(RuntimeWarning, match='precision range'), torch.no_grad():
        eps, _ = dyn(dev(inp['xh_phar']), dev(inp['xh_pocket']), dev(inp['t']), dev(inp['mask_phar']), dev(inp['mask_pocket']))
    got = eps.cpu().numpy()
    assert np.isfinite(got).all() and np.abs(got - want).max() <= EVAL_TOL * max(1.0, float(np.abs(want).max()))


def test_chain_on_a_low_range_model_equals_the_bf16_engine_chain():
    """K = 6 chain (graph replay) of a model whose message MLP works at 2^-14: the replayed graphs count the low-range rows, and the guarded
    chain equals a half_engine = 0 chain (same draws) within the evaluation tolerance, types exact, with a warning."""
    from cmdgen_amd.synthetic import make_pockets
    cfg, sd, _ = underflow_case('msg', LOW_SCALES[-1])
    pb = make_pockets(8, 'CA', n_phar=8)
    K = 6
    px, poh = dev(pb.x), dev(pb.one_hot)

    def run_on(h):
        return lambda: h.sample_chain(px, poh, K, noise=None, seed=5, pocket_ids=pb.pocket_index, use_graph=True)
    ref = new_handle(cfg, sd)
    ref.set_option('half_engine', 0)
    ref.set_layout(pb.num_nodes_phar, pb.size)
    ref.set_step_table(K, host_step_table(cfg, K))
    want = run_on(ref)()[0].cpu().numpy()
    ref_resets = ref.chain_status()['nan_resets']
    ref.close()
    h = new_handle(cfg, sd)
    h.set_layout(pb.num_nodes_phar, pb.size)
    h.set_step_table(K, host_step_table(cfg, K))
    assert h.half_engine_active()
    run_on(h)()
    st0 = h.chain_status()
    assert st0['half_low_range'] >= 1, 'the raw half-engine chain is expected to count rows below the range'
    run_on(h)()                                # a replay of the captured step graphs counts again
    assert h.chain_status()['half_low_range'] >= 1
    with pytest.warns(RuntimeWarning, match='precision range'):
        (xh, _q, _z), st = h.run_range_guarded(run_on(h), h.chain_status)
    got = xh.cpu().numpy()
    assert st.get('half_engine_fallback') and st['nan_resets'] == ref_resets and st['half_low_range'] == 0
    assert np.abs(got[:, :3] - want[:, :3]).max() <= EVAL_TOL * max(1.0, float(np.abs(want[:, :3]).max())) and np.array_equal(got[:, 3:], want[:, 3:])
    h.close()


def test_guard_charges_no_earlier_reset_to_a_clean_chain():
    """A reset counted by an earlier call on the same handle (a raw overflowing evaluation) belongs to that call: the next guarded chain of a
    model inside the range is neither repeated nor warned about."""
    from cmdgen_amd.synthetic import make_pockets
    cfg, sd, inp = overflow_case('msg')
    nl, npk = G2[NAME + '/num_nodes_phar'], G2[NAME + '/pocket_size']
    h = new_handle(cfg, sd)
    h.set_layout(nl, npk)
    assert h.half_engine_active()
    h.dynamics_forward(dev(inp['xh_phar']), dev(inp['xh_pocket']), dev(inp['t']))
    torch.cuda.synchronize()
    assert h.counters()['nan_resets'] == 1, 'the raw overflowing evaluation resets'
    # the same handle, a clean model (weights reloaded) and a chain
    cfg2, sd2, _ = dynamics_case(G2, NAME)
    h.load_state_dict(sd2)
    pb = make_pockets(8, 'CA', n_phar=8)
    K = 6
    h.set_layout(pb.num_nodes_phar, pb.size)
    h.set_step_table(K, host_step_table(cfg2, K))
    px, poh = dev(pb.x), dev(pb.one_hot)
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        _out, st = h.run_range_guarded(lambda: h.sample_chain(px, poh, K, noise=None, seed=5, pocket_ids=pb.pocket_index, use_graph=True),
                                       h.chain_status)
    assert st['nan_resets'] == 0 and st['half_low_range'] == 0 and 'half_engine_fallback' not in st
    h.close()


@pytest.mark.parametrize('rep,n_pockets', [('CA', 64), ('CA', 256), ('full-atom', 8)])
def test_random_init_bench_model_stays_inside_the_range(rep, n_pockets):
    """No false positives: K = 20 chains of bench.py's random-init model (bounded schedule) count no low-range row and do not warn."""
    from cmdgen_amd.synthetic import ModelConfig, make_state_dict, make_pockets
    K = 20
    cfg = ModelConfig(residue_nf=20 if rep == 'CA' else 11, timesteps=K, noise_precision=0.1, norm_values=(1.0, 0.25))
    h = new_handle(cfg, make_state_dict(cfg, seed=0))
    pb = make_pockets(n_pockets, rep)
    if rep == 'full-atom':
        assert int(pb.size.max()) == 366
    h.set_layout(pb.num_nodes_phar, pb.size)
    assert h.half_engine_active()
    px, poh = dev(pb.x), dev(pb.one_hot)
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        _out, st = h.run_range_guarded(lambda: h.sample_chain(px, poh, K, noise=None, seed=3, pocket_ids=pb.pocket_index, use_graph=True),
                                       h.chain_status)
    assert st['half_low_range'] == 0 and st['nan_resets'] == 0 and 'half_engine_fallback' not in st
    h.close()


def test_only_the_low_rows_of_a_mixed_tile_are_counted(monkeypatch):
    """Low rows BETWEEN normal ones: the first layer of one message MLP takes its node features and bias at 2^-10 and its radial / d0
    features at 64x, so that exactly the self-loop edges of that GCL (radial = d0 = 0) have activations far below tau while every other edge of
    the same tiles is far above it.  Every edge-tile family must count exactly the rows the oracle's activations put below tau - a wrong
    row-to-flag mapping (swizzle, slot, row mask) would miss or add rows here, where a uniformly scaled model cannot tell."""
    import torch.nn.functional as F
    from oracle import ref_cpu
    from helpers import tau_from_header
    tau = tau_from_header()
    cfg, sd, inp = dynamics_case(G2, NAME)
    sd = dict(sd)
    first = TARGETS['msg']
    H = cfg.hidden_nf
    w = sd[first + '.weight'].copy()
    w[:, :2 * H] *= np.float32(2.0 ** -10)
    w[:, 2 * H:] *= np.float32(64.0)
    sd[first + '.weight'] = w.astype(np.float32)
    sd[first + '.bias'] = (sd[first + '.bias'] * np.float32(2.0 ** -10)).astype(np.float32)
    # the oracle's activations of every covered producer: rows below tau over all of K, and no row near tau on any quarter
    rows = []
    lin = ref_cpu._lin

    def spy(p, name, x):
        y = lin(p, name, x)
        if name.endswith(('edge_mlp.0', 'coord_mlp.0', 'node_mlp.0')):
            rows.append(F.silu(y).abs().reshape(y.shape[0], 4, -1).amax(dim=2).numpy())
        return y
    monkeypatch.setattr(ref_cpu, '_lin', spy)
    want = oracle_eps(cfg, sd, inp)
    monkeypatch.setattr(ref_cpu, '_lin', lin)
    q = np.concatenate(rows)                                    # [rows, quarter] max |a|
    low = (q < tau).all(axis=1)
    assert np.all(low | (q >= 1.5 * tau).all(axis=1)), 'the case must keep every row clear of tau on each quarter of K'
    expected = int(low.sum())
    n_nodes = len(inp['xh_phar']) + len(inp['xh_pocket'])
    assert expected == n_nodes, 'the low rows are the self loops of one GCL'
    nl, npk = G2[NAME + '/num_nodes_phar'], G2[NAME + '/pocket_size']
    xp, xq, t = dev(inp['xh_phar']), dev(inp['xh_pocket']), dev(inp['t'])
    tol = EVAL_TOL * max(1.0, float(np.abs(want).max()))
    for optset in ('rows128_node64', 'rows128_fused', 'fullk32_node16w'):
        for k, v in OPTION_SETS[optset].items():
            monkeypatch.setitem(hip_backend.DEFAULT_OPTIONS, k, v)
        monkeypatch.setitem(hip_backend.DEFAULT_OPTIONS, 'dead_skip', 0)        # every tile runs: the count is the whole layout's
        h = new_handle(cfg, sd)
        h.set_layout(nl, npk)
        assert_tiles(h, 'msg', optset)
        h.reset_counters()
        h.dynamics_forward(xp, xq, t)
        torch.cuda.synchronize()
        got = h.counters()['half_low_range']
        with pytest.warns(RuntimeWarning, match='precision range'):
            (eps, _p), st = h.run_range_guarded(lambda: h.dynamics_forward(xp, xq, t), dict)
        err = float(np.abs(eps.cpu().numpy() - want).max())
        h.close()
        print(f'mixed / {optset}: {got} rows counted, {expected} below tau in the oracle; guarded call vs oracle {err:.2e}')
        assert got == expected, f'{optset}: {got} rows counted, the oracle has {expected} below tau'
        assert st.get('half_engine_fallback') and err <= tol
