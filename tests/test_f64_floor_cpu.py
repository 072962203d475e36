"""The float64 yardstick (f64_ref.py) checked on the CPU alone: the dtype switch leaves ref_cpu as it found it and is the existing oracle bit for
bit in fp32; every case's radius graph is the same in both dtypes, with every sample clear of the cutoff, and every compared quantity has a floor;
the forced launches of test_hip_f64_floor.py resolve as named in the launch planner; the CPU models of the correct engines stay under the bounds
the GPU test asserts, and a product dropped in ONE layer - one per layer kind, in the first, a middle and the last block, on both engine models -
exceeds the bound of some stage quantity at least twofold.  The last test prints, per planted defect, what EVAL_TOL sees of it (pytest -s)."""
import numpy as np
import pytest
import torch

import f64_ref as fr
import rule_sweep_ref as rs
from oracle import ref_cpu

EVAL_TOL = 2e-5                 # test_hip_parity_r2.EVAL_TOL (that module needs a GPU to import): max|d eps| <= EVAL_TOL * max(1, |eps|)


def test_dtype_switch_restores_float_and_fp32_is_the_existing_oracle():
    assert ref_cpu.FLOAT is torch.float32
    lin = ref_cpu._lin
    with pytest.raises(RuntimeError):
        with fr.oracle_dtype(torch.float64, lambda p, name, x: x):
            assert ref_cpu.FLOAT is torch.float64 and ref_cpu._lin is not lin
            raise RuntimeError('inside')
    assert ref_cpu.FLOAT is torch.float32 and ref_cpu._lin is lin
    for case, kind in ((fr.BASE, 'cond'), (fr.JOINT, 'joint')):
        o = rs.oracle_evaluation(rs._c(case.B, (), kind=kind))
        r = fr.run_of(case, torch.float32)
        assert r['eps_phar'].dtype == torch.float32
        assert np.array_equal(r['eps_phar'].numpy(), o['want_phar']) and np.array_equal(r['eps_pocket'].numpy(), o['want_pocket'])
        assert r['edges'].shape[1] == o['edges']
        r64 = fr.run_of(case, torch.float64)
        assert r64['eps_phar'].dtype == torch.float64
        assert ref_cpu.FLOAT is torch.float32
    # the gradients' helper as well
    d = fr.training_cotangent(fr.HX[0])
    w, ins = fr.gradients(fr.HX[0], torch.float64, d)
    assert ref_cpu.FLOAT is torch.float32 and np.isfinite(d).all() and d.dtype == np.float32
    assert all(v.dtype == np.float64 for v in w.values()) and ins['xh_phar'].shape == d.shape


def test_ratio_is_relative_to_the_fp32_floor_and_clamped():
    f64 = np.linspace(-1.0, 1.0, 101)
    f32 = f64 + 1e-7
    assert fr.ratio(f32, f32, f64) == pytest.approx((1.0, 1.0))
    assert fr.ratio(f64 + 3e-7, f32, f64) == pytest.approx((3.0, 3.0))
    # an oracle that happens to be exact: the floor is one fp32 rounding of the result itself
    r, m = fr.ratio(f64 + 2.0 ** -24, f64, f64)
    assert r == pytest.approx(1.0 / fr._rms(f64)) and m == pytest.approx(1.0)
    assert [fr.bound_of(v) for v in (0.617, 1.0, 6.04, 0.0555)] == pytest.approx([1.3, 2.0, 13.0, 0.12], rel=1e-12)


@pytest.mark.parametrize('case', fr.CASES, ids=lambda c: c.name)
def test_every_case_has_one_graph_a_margin_and_a_floor(case):
    a, b = fr.run_of(case, torch.float32), fr.run_of(case, torch.float64)
    assert np.array_equal(a['edges'], b['edges'])
    margin = fr.margin_of(case)
    print(f'{case.name}: {a["edges"].shape[1]} edges, margin {margin:.2e} A')
    assert margin >= fr.MARGIN                     # no sample is ever left out
    assert set(a['stages']) == set(b['stages'])
    for k in a['stages']:
        assert fr._rms(a['stages'][k] - b['stages'][k]) > 0.0, k
        assert np.isfinite(b['stages'][k]).all()
    if case is fr.BASE:
        pb = fr.pockets_of(case)
        nl, N = int(pb.num_nodes_phar.sum()), int(pb.num_nodes_phar.sum() + pb.size.sum())
        assert (nl, N, a['edges'].shape[1]) == (57, 179, 1907)
        assert N % 16 and N % 32 and N % 64 and N > 128                 # full and partial node tiles of every size
        assert 1907 // 128 == 14 and 1907 % 128                         # 14 full and one partial 128-row message tile
        assert int((a['edges'][0] < nl).sum()) >= 2 * 128               # the phar-receiver list: more than two 128-row coordinate tiles


def test_the_forced_launches_resolve_as_named_in_the_planner():
    """Every launch of the GPU test through the launch planner on the host (256 CUs): the options given resolve to the keys the GPU test asserts
    through Handle.query (the keys the planner check prints; 'embed_mfma' is asserted on the GPU only)."""
    import plan_table_ref as pt
    ids = [fr.launch_id(l) for l in fr.LAUNCHES]
    assert len(set(ids)) == len(ids)
    layouts, plans = [], []
    for l in fr.LAUNCHES:
        cfg, pb = fr.config_of(l.case), fr.pockets_of(l.case)
        layouts.append((pb.num_nodes_phar, pb.size))
        opts = dict(l.options)
        if l.engine == 'bf3' and cfg.edge_cutoff is not None:
            opts['half_engine'] = 0
        plans.append(dict(H=cfg.hidden_nf, L=cfg.n_layers, S=cfg.inv_sublayers, joint=int(cfg.update_pocket_coords), sin=0, no_cutoff=int(cfg.edge_cutoff is None),
                          n_cus=256, gemm_split=int(l.engine != 'fp32'), layout=len(layouts) - 1, opts=opts))
    got = pt.run_planner(layouts, plans)
    for l, g in zip(fr.LAUNCHES, got):
        res = dict(zip(pt.QUERY_KEYS, (int(v) for v in g)))
        for k, v in l.expect:
            if k in res:
                assert res[k] == v, (fr.launch_id(l), k, res[k], v)
    # the rule table's regimes are all there, on the engine they belong to
    assert {l.name for l in fr.H256_LAUNCHES if l.engine == 'half'} >= set(fr.RULE_TUPLES)
    assert len([l for l in fr.H256_LAUNCHES if l.engine == 'bf3']) == 6 and len([l for l in fr.H256_LAUNCHES if l.engine == 'fp32']) == 5


# ----------------------------------------------------------------------------- the engine models and the planted defects
BLOCK_LAYERS = ('gcl_0.edge_mlp.0', 'gcl_0.edge_mlp.2', 'gcl_0.att_mlp.0', 'gcl_0.node_mlp.0', 'gcl_0.node_mlp.2',
                'gcl_equiv.coord_mlp.0', 'gcl_equiv.coord_mlp.2', 'gcl_equiv.coord_mlp.4')
BLOCKS = (0, 2, 4)                                # the first, a middle and the last block of L = 5
OTHER_LAYERS = ('dynamics.egnn.embedding', 'dynamics.egnn.embedding_out', 'dynamics.phar_decoder.0')
DEFECTS = [f'dynamics.egnn.e_block_{b}.{layer}' for layer in BLOCK_LAYERS for b in BLOCKS] + list(OTHER_LAYERS)
# piece 0 is the high one: the half engine's a_lo * w_hi (11 bits lost in that GEMM) and the three-piece engine's a_mid * w_hi (16 bits lost).
# (The three-piece engine's smallest products, 2^-16 of the leading one, are at the resolution of the measure: dropped in one layer, a_lo * w_hi
# gives agg / acc 5.7 - 9.6, twice their bounds or a little more, h 2.0 - 2.6 from a node layer, under its bound, and nothing from att_mlp.)
DROPPED = {'half': (1, 0), 'bf3': (1, 0)}


def bounds_of(engine):
    b = fr.BOUNDS.get(engine)
    assert b is not None and all(b.get(k) is not None for k in fr.KINDS), f'the bounds of the {engine} engine are not measured yet (f64_ref.BOUNDS)'
    return b


@pytest.mark.parametrize('engine', ['half', 'bf3'])
@pytest.mark.parametrize('case', [fr.BASE, fr.HX[0]], ids=lambda c: c.name)
def test_correct_engine_models_stay_under_the_bounds(case, engine):
    st, eps = fr.engine_stages(case, engine)
    worst = fr.worst_per_kind(fr.ratios(st, case))
    print(f'{case.name} {engine} model: ' + '  '.join(f'{k} {worst[k][0]:.2f} (max-norm {worst[k][1]:.2f})' for k in fr.KINDS))
    b = bounds_of(engine)
    for k in fr.KINDS:
        assert worst[k][0] <= b[k], (k, worst[k][0], b[k])


@pytest.mark.parametrize('engine', ['half', 'bf3'])
def test_a_dropped_product_in_one_layer_exceeds_a_bound_twofold(engine):
    case = fr.BASE
    f32 = fr.run_of(case, torch.float32)
    want = f32['eps_phar'].numpy()
    tol = EVAL_TOL * max(1.0, float(np.abs(want).max()))
    clean_st, clean_eps = fr.engine_stages(case, engine)
    rows = [('none (correct model)', clean_st, clean_eps)] + [(name, *fr.engine_stages(case, engine, (name, DROPPED[engine]))) for name in DEFECTS]
    bounds = fr.BOUNDS.get(engine) or {}
    missed = []
    print(f'\n{engine} model, product {DROPPED[engine]} dropped in one layer; ratios are rms(result - float64) / rms(fp32 oracle - float64)')
    print(f'{"planted defect":46s} {"max|d eps| vs fp32 oracle":>26s} {"passes EVAL_TOL":>16s}  ' + ' '.join(f'{k:>8s}' for k in fr.KINDS) + '   caught by')
    for name, st, eps in rows:
        rt = fr.ratios(st, case)
        worst = fr.worst_per_kind(rt)
        err = float(np.abs(eps - want).max())
        over = {k: worst[k][0] / bounds[k] for k in fr.KINDS if bounds.get(k)}
        seen = max(over, key=over.get) if over else None
        where = max((key for key in rt if key[0] == seen), key=lambda key: rt[key][0]) if seen else None
        caught = f'{seen} of {where[1]}: {over[seen]:.1f} x its bound' if seen else 'bounds not measured'
        print(f'{name[len("dynamics."):] if name.startswith("dynamics.") else name:46s} {err:26.2e} {"yes" if err <= tol else "no":>16s}  '
              + ' '.join(f'{worst[k][0]:8.2f}' for k in fr.KINDS) + '   ' + caught)
        if name in DEFECTS and not (seen and over[seen] >= 2.0):
            missed.append((name, over))
    bounds_of(engine)
    assert not missed, missed
