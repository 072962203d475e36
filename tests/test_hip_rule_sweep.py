"""The library's OWN launches against the oracle on both sides of every boundary of its tile rules, 1 - 278 C-alpha pockets.

The launch planner (make_plan, csrc/cmdgen_plan.h) chooses the kernels of an evaluation from the layout alone, about ten times between 1 and 300
pockets; the other suites compare the library's own choice with the reference in three of those regimes and are self-consistency checks
(option against option, permutation, reflection) everywhere else, which a mistake shared by both sides passes.  Here no tile option is set:

(a) one evaluation per boundary size, ragged pockets, against ref_cpu.dynamics_forward run live (fp32 on the CPU, pinned to the real reference
    by G1-G19) at the project's bound for one evaluation, EVAL_TOL; (b) the same with the phar points drifted out, where the dead-work skip
    drops tiles; (c) the three-piece and fp32 engines and the joint model; (d) K = 5 chains through the chain driver (k_step_count, the
    pocket-row cache, skip_count, graph capture and replay: two replays of two steps and one eager step) at the project's chain bounds.

Every checked evaluation follows one of the same layout on OTHER inputs, so h, P|Q, Pc|Qc, agg and ACC hold plausible but wrong values: a tile
no workgroup owns shows up as an error instead of hiding behind zeros or the right answer of an earlier call.  The radius graph is a hard
threshold the reference has too: a sample with a pair within 1e-4 A of the cutoff is left out (rule_sweep_ref.py), and at most 5 % (an
evaluation) / 20 % (a chain) of a case's samples may be - asserted, never skipped.  On a 256-CU device the resolved launch must be the case
table's, so a moved threshold moves these sizes with it; the parity assertions run on any device.

Every case prints one line (pytest -s): sizes, coord_grid, the resolved launch, errors, samples left out - the table DESIGN.md section 7 refers to.
"""
import numpy as np
import pytest
import torch

import rule_sweep_ref as rs
from helpers import EVAL_TOL, rms
from chain_kit import dev
from cmdgen_amd import hip_backend

pytestmark = pytest.mark.gpu


def new_handle(case):
    """A fresh handle with no launch option set; the engine is the case's."""
    h = hip_backend.Handle(rs.config_of(case).as_dict(), 0)
    h.load_state_dict(rs.state_dict_of(case))
    if case.engine == 'bf3':
        h.set_option('half_engine', 0)
    elif case.engine == 'fp32':
        h.set_gemm_mode(False)
    return h


def resolved(h):
    return tuple(int(h.query(k)) for k in rs.LAUNCH_KEYS)


def table_applies():
    """The case table's launches are those of 256 CUs with every choice left to the library (conftest's CMDGEN_TEST_OPTIONS sets some)."""
    return torch.cuda.get_device_properties(0).multi_processor_count == 256 and not hip_backend.DEFAULT_OPTIONS


def test_query_replays_the_recorded_launch_table():
    """tests/golden/plan_table.npz - every launch key of cmdgen_query over a sweep of configs, engines, options and layouts, recorded from the
    library before the launch planner (csrc/cmdgen_plan.h) replaced its rules - through Handle.query of this build; no kernel is launched.  And
    the three *_mfmas_per_product keys answer on a handle that has a layout but no finalized weights."""
    import plan_table_ref as pt
    c = rs.EVAL_CASES[3]
    h = hip_backend.Handle(rs.config_of(c).as_dict(), 0)
    pb = rs.pockets_of(c)
    h.set_layout(pb.num_nodes_phar, pb.size)
    assert [h.query(r + '_mfmas_per_product') for r in ('msg', 'node', 'coord')] == [6, 1, 6] or not table_applies()
    assert all(h.query(r + '_mfmas_per_product') in (1, 6) for r in ('msg', 'node', 'coord'))      # (the half forms need their packs)
    h.load_state_dict(rs.state_dict_of(c))
    assert resolved(h) == c.launch or not table_applies()                  # ... and the plan follows the weights
    h.close()
    t = pt.table()
    if table_applies() and torch.cuda.get_device_properties(0).multi_processor_count == t['n_cus']:
        got, want = pt.replay_on_gpu(), t['rows'][:, pt.N_IN:]
        bad = np.flatnonzero((got != want).any(axis=1))
        assert len(bad) == 0, [(pt.describe(t['rows'][i]), {k: (int(w), int(g)) for k, w, g in zip(pt.QUERY_KEYS, want[i], got[i]) if w != g}) for i in bad[:5]]


def evaluate(h, inputs):
    """The evaluation as the model's own chain asks for it: the conditional model without the pocket output (launch_eval skips dead tiles only
    then: a pocket node's new h is somebody's output otherwise), the joint model with it."""
    xh, xq, t = inputs
    ep, eq = h.dynamics_forward(dev(xh), dev(xq), dev(t), want_pocket=bool(h.cfg['update_pocket_coords']))
    return ep.cpu().numpy(), (eq.cpu().numpy() if eq is not None else None)


def check_evaluation(case):
    """Steps 1-7 of a one-evaluation case; -> the counters of the checked call."""
    torch.set_num_threads(min(16, torch.get_num_threads()))
    o = rs.oracle_evaluation(case)
    pb, (pm, qm) = o['pb'], o['masks']
    h = new_handle(case)
    h.set_layout(pb.num_nodes_phar, pb.size)
    launch, coord_grid = resolved(h), int(h.query('coord_grid'))
    N = int(pb.num_nodes_phar.sum() + pb.size.sum())
    evaluate(h, o['poison'])                                          # 1. every buffer holds another input's values
    c0 = h.counters()
    got = evaluate(h, o['inputs'])                                    # 2. the checked call
    c1 = h.counters()
    again, third = evaluate(h, o['inputs']), evaluate(h, o['inputs'])  # 5. the repeat, and one more for the run-to-run noise
    c3 = h.counters()
    h.close()
    used = {k: c1[k] - c0[k] for k in c1}
    keep = rs.kept_samples(o['margins'])                              # 3. samples within MARGIN of the cutoff are left out ...
    n_out = int((~keep).sum())
    outputs = [(got[0], o['want_phar'], keep[pm])]
    if case.kind == 'joint':
        outputs.append((got[1], o['want_pocket'], keep[qm]))
    errs = [(float(np.abs(g[rows] - w[rows]).max()), max(1.0, float(np.abs(w[rows]).max()))) for g, w, rows in outputs]
    n_out_all = case.kind == 'joint' and 2 or 1
    scale = max(float(np.abs(g).max()) for g in got[:n_out_all])
    noise = max(float(np.abs(a - b).max()) for a, b in zip(again[:n_out_all], third[:n_out_all]))
    first = max(float(np.abs(a - b).max()) for a, b in zip(got[:n_out_all], again[:n_out_all]))
    # 7.
    print(f'\n[{rs.case_id(case)}] B {case.B}  N {N}  N%32 {N % 32}  coord_grid {coord_grid}  coord_grid%8 {coord_grid % 8}  launch {launch}  '
          f'half_low_range {used["half_low_range"]}  max error {max(e / s for e, s in errs):.2e} of max(1, |eps|)  left out {n_out} of {case.B}  '
          f'edges {used["edges"]} (oracle {o["edges"]}; skipped {used["edges_skipped"]}, node rows skipped {used["node_rows_skipped"]})  '
          f'first vs repeat {first / scale:.1e}, run to run {noise / scale:.1e}')
    assert n_out <= rs.EVAL_CAP * case.B                              # ... at most 5 % of them
    for err, s in errs:
        assert err <= EVAL_TOL * s, (err, s)
    assert used['evaluations'] == 1
    if n_out == 0:                                                    # 4. the graph
        assert used['edges'] == o['edges']
    else:
        assert abs(used['edges'] - o['edges']) <= 2 * int(o['near'][~keep].sum())
    assert first <= max(4.0 * noise, 2e-6 * scale), (first, noise, scale)
    assert c3['nan_resets'] == 0                                      # 6.
    if table_applies():
        assert launch == case.launch, (launch, case.launch)
    return used


@pytest.mark.parametrize('case', rs.EVAL_CASES, ids=rs.case_id)
def test_own_launch_matches_oracle_at_every_rule_boundary(case):
    check_evaluation(case)


@pytest.mark.parametrize('case', rs.DRIFT_CASES, ids=rs.case_id)
def test_own_launch_matches_oracle_with_drifted_phar_points(case):
    """The pharmacophore as a compact body 12-14 A from the centre of its pocket: 5 % of the pocket nodes are within a hop of a moving node,
    and the default dead_skip leaves the others' tiles out.  A replay of the hop levels over these inputs gives, in the last block alone, 37
    of 152 32-row message tiles without a live receiver at 9 pockets, 29 / 42 / 72 128-row tiles at 47 / 70 / 139, and two 64-row node
    tiles at 139 - so the counters must move."""
    used = check_evaluation(case)
    assert used['edges_skipped'] > 0
    if case.B == 139:
        assert used['node_rows_skipped'] > 0


@pytest.mark.parametrize('case', rs.ENGINE_CASES + rs.JOINT_CASES, ids=rs.case_id)
def test_own_launch_matches_oracle_on_the_other_engines_and_the_joint_model(case):
    check_evaluation(case)


@pytest.mark.parametrize('use_graph', [True, False], ids=['graph', 'eager'])
@pytest.mark.parametrize('case', rs.CHAIN_CASES, ids=rs.case_id)
def test_short_chain_matches_oracle(case, use_graph, monkeypatch):
    torch.set_num_threads(min(16, torch.get_num_threads()))
    K = rs.CHAIN_K
    r = rs.oracle_chain(case, monkeypatch)
    pb, (pm, qm) = r['pb'], r['masks']
    h = new_handle(case)
    h.set_option('graph_steps', 2)                                   # K = 5: two replays of two steps, one eager step
    h.set_layout(pb.num_nodes_phar, pb.size)
    launch = resolved(h)
    got, got_p, z_steps = h.sample_chain(dev(pb.x), dev(pb.one_hot), K, noise=r['noise'].cuda(), want_steps=True, use_graph=use_graph)
    st = h.chain_status()
    got, got_p, z_steps = got.cpu().numpy(), got_p.cpu().numpy(), z_steps.cpu().numpy()
    h.close()
    keep = rs.kept_samples(r['margins'])                               # margin >= 1e-4 A at every one of the six evaluations
    n_out = int((~keep).sum())
    rows, rows_q = keep[pm], keep[qm]
    step_err = [float(np.abs(z_steps[k][rows] - r['chain'][k + 1][rows]).max()) / max(1.0, float(np.abs(r['chain'][k + 1][rows]).max())) for k in range(K)]
    want, want_p = r['want'], r['want_pocket']
    x_err = rms(got[rows, :3], want[rows, :3]) / max(1.0, float(np.abs(want[rows, :3]).max()))
    print(f'\n[{rs.case_id(case)} chain, {"graph" if use_graph else "eager"}] launch {launch}  per-step z {max(step_err):.2e}  final x RMS {x_err:.2e}  '
          f'(relative to max(1, |.|))  left out {n_out} of {case.B}')
    assert n_out <= rs.CHAIN_CAP * case.B
    for k in range(K):
        assert step_err[k] <= 1e-4, (k, step_err)
    assert x_err <= 1e-4
    assert np.array_equal(got[rows, 3:], want[rows, 3:])
    assert rms(got_p[rows_q], want_p[rows_q]) <= 1e-4 * max(1.0, float(np.abs(want_p[rows_q]).max()))
    assert st['nan_resets'] == 0 and st['max_rel_com_error'] < 1e-2
    if table_applies():
        assert launch == case.launch, (launch, case.launch)
