"""The conditions the tile-rule sweep (test_hip_rule_sweep.py) puts on its own inputs, checked with the input builder and the CPU oracle alone,
so that inputs which break a cap are found without a GPU: per case at most EVAL_CAP of the samples of an evaluation, and CHAIN_CAP of the
samples of a K = 5 chain, come within MARGIN of the radius graph's cutoff and are left out of the comparison."""
import numpy as np
import pytest

import rule_sweep_ref as rs
from cmdgen_amd.synthetic import min_cutoff_margin


def test_case_table_is_consistent():
    ids = [rs.case_id(c) for c in rs.ONE_EVALUATION]
    assert len(set(ids)) == len(ids)
    assert len({rs.case_id(c) for c in rs.CHAIN_CASES}) == len(rs.CHAIN_CASES)
    for c in rs.ONE_EVALUATION + rs.CHAIN_CASES:
        assert len(c.launch) == len(rs.LAUNCH_KEYS)
    # every regime of the default engine's rule table is the expected launch of some case with the phar points inside the pocket
    reached = {c.launch for c in rs.EVAL_CASES}
    assert reached == {rs.R1, rs.R4, rs.R9, rs.R47, rs.R70, rs.R78, rs.R106, rs.R139, rs.R176, rs.R278}
    # each engine of part (c) at four launches or more
    for eng in ('bf3', 'fp32'):
        assert len({c.launch for c in rs.ENGINE_CASES if c.engine == eng}) >= 4


def test_planner_resolves_the_case_tables_launch_at_256_cus():
    """Every case's expected launch is what the launch planner (csrc/cmdgen_plan.h, on the host through tests/plan_check.cpp) resolves for its
    layout, engine and model on 256 CUs with no option set - the table test_hip_rule_sweep.py asserts on such a device."""
    import plan_table_ref as pt
    cases = rs.ONE_EVALUATION + rs.CHAIN_CASES
    layouts, plans = [], []
    for c in cases:
        cfg, pb = rs.config_of(c), rs.pockets_of(c)
        layouts.append((pb.num_nodes_phar, pb.size))
        plans.append(dict(H=cfg.hidden_nf, L=cfg.n_layers, S=cfg.inv_sublayers, joint=int(c.kind == 'joint'), sin=0, no_cutoff=0, n_cus=256,
                          gemm_split=int(c.engine != 'fp32'), layout=len(layouts) - 1, opts={'half_engine': 0} if c.engine == 'bf3' else {}))
    got = pt.run_planner(layouts, plans)
    cols = [pt.QUERY_KEYS.index(k) for k in rs.LAUNCH_KEYS]
    for c, g in zip(cases, got):
        assert tuple(int(v) for v in g[cols]) == c.launch, (rs.case_id(c), tuple(g[cols]), c.launch)


def test_inside_geometry_is_the_property_tests_input_builder():
    from helpers import eval_inputs
    case = rs.EVAL_CASES[1]
    pb, cfg = rs.pockets_of(case), rs.config_of(case)
    for a, b in zip(rs.eval_inputs(pb, cfg), eval_inputs(pb, cfg)):
        assert np.array_equal(a, b)
    # 'drifted': the phar points sit 10-14 A from the centre of mass of their pocket
    xh, _, _ = rs.eval_inputs(pb, cfg, geometry='drifted')
    pm, qm = rs.masks_of(pb)
    com = np.stack([pb.x[qm == b].astype(np.float64).mean(0) for b in range(case.B)])
    r = np.linalg.norm(xh[:, :3] - com[pm], axis=1)
    assert r.min() > 10.0 - 1e-4 and r.max() < 14.0 + 1e-4


def test_sample_margins_is_min_cutoff_margin_per_sample():
    case = rs.EVAL_CASES[2]
    pb, cfg = rs.pockets_of(case), rs.config_of(case)
    xh, xq, _ = rs.eval_inputs(pb, cfg)
    pm, qm = rs.masks_of(pb)
    m = rs.sample_margins(xh[:, :3], xq[:, :3], (pm, qm))
    assert m.shape == (case.B,)
    for b in range(case.B):
        x = np.concatenate([xh[pm == b, :3], xq[qm == b, :3]])
        assert m[b] == min_cutoff_margin(x, np.zeros(len(x), np.int64), rs.CUTOFF)
    assert m.min() == min_cutoff_margin(np.concatenate([xh[:, :3], xq[:, :3]]), np.concatenate([pm, qm]), rs.CUTOFF)
    # a pair moved onto the cutoff is found, in its sample only
    x2 = xq[:, :3].copy()
    i, j = np.flatnonzero(qm == 1)[:2]
    d = x2[j] - x2[i]
    x2[j] = x2[i] + d / np.linalg.norm(d) * (rs.CUTOFF + 2e-5)
    m2 = rs.sample_margins(xh[:, :3], x2, (pm, qm))
    assert m2[1] < rs.MARGIN and rs.pairs_under_margin(xh[:, :3], x2, (pm, qm))[1] >= 1
    assert np.array_equal(rs.kept_samples(m2), [m[0] >= rs.MARGIN, False] + list(m[2:] >= rs.MARGIN))


@pytest.mark.parametrize('case', rs.ONE_EVALUATION, ids=rs.case_id)
def test_an_evaluation_leaves_out_at_most_5_percent(case):
    _, margins, near = rs.eval_margins(case)
    out = ~rs.kept_samples(margins)
    print(f'{rs.case_id(case)}: {int(out.sum())} of {case.B} samples within {rs.MARGIN} A of the cutoff ({int(near[out].sum())} pairs)')
    assert out.sum() <= rs.EVAL_CAP * case.B
    assert (near[out] >= 1).all() and not near[~out].any()


def test_the_recorded_oracle_sees_every_evaluation_of_a_chain(monkeypatch):
    from oracle import ref_cpu
    case = rs.CHAIN_CASES[0]
    orig = ref_cpu.dynamics_forward
    r = rs.oracle_chain(case, monkeypatch)
    assert ref_cpu.dynamics_forward is orig
    assert r['margins'].shape == (rs.CHAIN_K + 1, case.B) and len(r['chain']) == rs.CHAIN_K + 1
    # the first evaluation's phar coordinates are the chain's initial z
    rec = rs.RecordedForward(orig)
    monkeypatch.setattr(ref_cpu, 'dynamics_forward', rec)
    import torch
    pb, cfg = r['pb'], rs.config_of(case)
    tape = iter(r['noise'])
    with torch.no_grad():
        ref_cpu.sample_given_pocket(rs.params_of(case), cfg.as_dict(), rs.pocket_dict(pb), pb.num_nodes_phar, timesteps=rs.CHAIN_K,
                                    noise=lambda shape: next(tape))
    assert len(rec.calls) == rs.CHAIN_K + 1
    assert np.array_equal(rec.calls[0]['x_phar'], r['chain'][0][:, :3])
    assert np.array_equal(rec.margins(), r['margins'])


@pytest.mark.parametrize('case', rs.CHAIN_CASES, ids=rs.case_id)
def test_a_chain_leaves_out_at_most_20_percent(case, monkeypatch):
    """K = 5 exactly as the GPU test runs it.  The cases of 70 and 106 pockets take 6 and 10 s of oracle on 16 threads; with them the file takes
    under half a minute, so they run everywhere, unmarked (where the GPU suite runs too, it finds their chains in rule_sweep_ref's cache)."""
    r = rs.oracle_chain(case, monkeypatch)
    out = ~rs.kept_samples(r['margins'])
    print(f'{rs.case_id(case)}: {int(out.sum())} of {case.B} samples within {rs.MARGIN} A of the cutoff at one of {rs.CHAIN_K + 1} evaluations')
    assert out.sum() <= rs.CHAIN_CAP * case.B
