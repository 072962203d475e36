"""Every matrix engine against the float64 oracle, stage by stage (f64_ref.py): is a launch still at the fp32 floor, not merely under 2e-5?

One evaluation on the 3-pocket ragged layout (179 rows, 1907 edges, every pair 2.5e-3 A or more from the cutoff: no sample is ever left out), each
launch FORCED with set_option and asserted through query: at H = 256, L = 5 the ten regimes of the rule table on the half engine, the launches of
rule_sweep_ref.ENGINE_CASES on the three-piece and fp32 engines, the 64-row tiles and the variants an option selects; H = 64 / 128 / 512 at L = 2 on
16-, 32- and 64-row tiles; the joint model, inv_sublayers 2 with 'mean', attention and tanh off, no cutoff.  Per launch, for every block, the
prefix runs read agg, h and acc; then one whole evaluation with the pocket output and dead_skip 0 gives eps, acc and xl of every block and the
final h (launches with proj_in_coord exist only there).  Everything is a ratio to the fp32 oracle's own error against float64 and is asserted
against one bound per (engine, quantity kind), f64_ref.BOUNDS.  The training step's forward and gradients (weights, inputs) the same way, per
engine, against autograd through the oracle in both dtypes.

pytest -s prints one line per launch: the table of profiles/f64_floor.txt and DESIGN.md section 7."""
import numpy as np
import pytest
import torch

import f64_ref as fr
from chain_kit import dev
from cmdgen_amd import hip_backend

pytestmark = pytest.mark.gpu


def new_handle(l):
    """A handle on the launch's model, engine and options, laid out; every expected key asserted through query."""
    cfg, pb = fr.config_of(l.case), fr.pockets_of(l.case)
    h = hip_backend.Handle(cfg.as_dict(), 0)
    h.load_state_dict(fr.state_dict_of(l.case))
    if l.engine == 'fp32':
        h.set_gemm_mode(False)
    elif l.engine == 'bf3' and cfg.edge_cutoff is not None:           # (no cutoff: the three-piece engine by the library's own rule)
        h.set_option('half_engine', 0)
    h.set_option('dead_skip', 0)
    for k, v in l.options:
        h.set_option(k, v)
    h.set_layout(pb.num_nodes_phar, pb.size)
    for k, v in l.expect:
        assert h.query(k) == v, (fr.launch_id(l), k, h.query(k), v)
    assert h.query('dead_skip') == 0
    return h


def merge(into, rt):
    for k, v in fr.worst_per_kind(rt).items():
        a = into.get(k, (0.0, 0.0))
        into[k] = (max(a[0], v[0]), max(a[1], v[1]))


def check_bounds(engine, worst, bounds, kinds, what):
    b = bounds.get(engine) or {}
    missing = [k for k in kinds if b.get(k) is None]
    assert not missing, f'{what}: no measured bound for {missing} of the {engine} engine (f64_ref)'
    for k in kinds:
        assert worst[k][0] <= b[k], (what, k, worst[k][0], b[k])


@pytest.mark.parametrize('l', fr.LAUNCHES, ids=fr.launch_id)
def test_one_evaluation_stays_at_the_fp32_floor(l):
    case = l.case
    cfg, pb = fr.config_of(case), fr.pockets_of(case)
    fr.stages(case, torch.float32), fr.stages(case, torch.float64)          # (the cached CPU oracles)
    xh, xq, t = fr.inputs_of(case)
    xp, xqd, td = dev(xh), dev(xq), dev(t)
    nl, N, H, L = int(pb.num_nodes_phar.sum()), int(pb.num_nodes_phar.sum() + pb.size.sum()), cfg.hidden_nf, cfg.n_layers
    Nm = N if cfg.update_pocket_coords else nl
    div = fr.divisors(case)
    h = new_handle(l)
    launch = tuple(int(h.query(k)) for k in fr.rs.LAUNCH_KEYS)
    mfmas = tuple(int(h.query(r + '_mfmas_per_product')) for r in ('msg', 'node', 'coord'))

    def read(what, shape):
        return h.debug_read(what, int(np.prod(shape))).reshape(shape).astype(np.float64)
    worst = {}
    pre = {}
    for b in range(L):                                                       # the prefix runs: the projections stay in the node launch
        h.debug_eval_prefix(xp, xqd, td, b, 1)
        pre['agg', b] = read('agg', (N, H)) / div[:, None]
        h.debug_eval_prefix(xp, xqd, td, b, 2)
        pre['h', b] = read('h', (N, H))
        h.debug_eval_prefix(xp, xqd, td, b, 3)
        pre['acc', b] = read('acc', (L, Nm, 4))[b, :, :3] / div[:Nm, None]
    merge(worst, fr.ratios(pre, case))
    ep, eq = h.dynamics_forward(xp, xqd, td, want_pocket=True)              # the whole evaluation, as launched
    ep, eq = ep.cpu().numpy().astype(np.float64), eq.cpu().numpy().astype(np.float64)
    edges = h.get_edges()
    acc, xl = read('acc', (L, Nm, 4)), read('xl', (L, Nm, 4))
    full = {('h', L - 1): read('h', (N, H)), ('vel', 'phar'): ep[:, :3], ('feat', 'phar'): ep[:, 3:], ('feat', 'pocket'): eq[:, 3:]}
    if cfg.update_pocket_coords:
        full['vel', 'pocket'] = eq[:, :3]
    for b in range(L):
        full['acc', b] = acc[b, :, :3] / div[:Nm, None]
        if b + 1 < L:
            full['x', b] = xl[b + 1, :, :3]                                  # the positions block b leaves are those block b + 1 starts from
    c = h.counters()
    h.close()
    merge(worst, fr.ratios(full, case))
    print(f'\n[f64 floor] {fr.launch_id(l):34s} launch {launch} mfmas {mfmas}  ' + '  '.join(f'{k} {worst[k][0]:.2f} ({worst[k][1]:.2f})' for k in fr.KINDS))
    assert np.array_equal(edges, fr.run_of(case, torch.float64)['edges'])   # one graph: no sample is left out
    assert c['nan_resets'] == 0
    assert all(np.isfinite(v).all() for v in list(pre.values()) + list(full.values()))
    check_bounds(l.engine, worst, fr.BOUNDS, fr.KINDS, fr.launch_id(l))


# ----------------------------------------------------------------------------- the training step
def flat_theta(h, sd):
    theta = torch.zeros(h.param_count(), dtype=torch.float32)
    for k, v in sd.items():
        if k.startswith('ddpm.dynamics.'):
            off, cnt = h.param_offset(k[len('ddpm.dynamics.'):])
            assert cnt == v.size
            theta[off:off + cnt] = torch.from_numpy(v.reshape(-1))
    return theta.cuda()


@pytest.mark.parametrize('case, engine', fr.TRAIN_CASES, ids=lambda v: v if isinstance(v, str) else v.name)
def test_training_step_against_float64_autograd(case, engine):
    """cmdgen_train_forward / train_backward / train_backward_inputs with fp32 operands (the bf16-operand step is bf16 by design and has its own
    test): the saving forward's eps, every weight tensor's gradient and the input gradients, each as a ratio to the fp32 autograd floor."""
    cfg, pb = fr.config_of(case), fr.pockets_of(case)
    sd = fr.state_dict_of(case)
    d_eps, _, (w64, _) = fr.gradient_oracles(case)
    xh, xq, t = fr.inputs_of(case)
    h = hip_backend.Handle(cfg.as_dict(), 0)
    if engine == 'fp32':
        h.set_gemm_mode(False)
    elif engine == 'bf3':
        h.set_option('train_half', 0)
    theta = flat_theta(h, sd)
    h.set_layout(pb.num_nodes_phar, pb.size)
    assert h.query('gemm_split') == int(engine != 'fp32')
    xp, xqd = dev(xh), dev(xq)
    eps = h.train_forward(theta, xp, xqd, dev(t)).cpu().numpy().astype(np.float64)
    ran_half = int(h.query('train_half_ran'))
    assert ran_half == 0 or engine == 'half'
    if engine == 'half' and cfg.hidden_nf == 256 and cfg.inv_sublayers == 1:
        assert ran_half == 1
    g1, g2 = torch.zeros_like(theta), torch.zeros_like(theta)
    h.train_backward(dev(d_eps), g1)
    d_xp, d_xq, d_t = torch.empty_like(xp), torch.empty_like(xqd), torch.empty(case.B, dtype=torch.float32, device='cuda')
    h.train_backward_inputs(dev(d_eps), g2, d_xh_phar=d_xp, d_xh_pocket=d_xq, d_t=d_t)
    g1, g2 = g1.cpu().numpy(), g2.cpu().numpy()
    offs = {k: h.param_offset(k) for k in w64}
    h.close()
    got_in = dict(xh_phar=d_xp.cpu().numpy(), xh_pocket=d_xq.cpu().numpy(), t=d_t.cpu().numpy())
    worst = {k: v for k, v in fr.worst_per_kind(fr.ratios({('vel', 'phar'): eps[:, :3], ('feat', 'phar'): eps[:, 3:]}, case)).items()}
    lines = []
    for tag, g in (('train_backward', g1), ('train_backward_inputs', g2)):
        got_w = {k: g[o:o + n] for k, (o, n) in offs.items()}
        rw, ri, dead = fr.gradient_ratios(got_w, got_in, case)
        for k in dead:
            assert not got_w[k].any(), (tag, k)
        top = sorted(rw, key=lambda k: -rw[k][0])[:3]
        lines.append(f'   {tag}: worst tensors ' + '  '.join(f'{k} {rw[k][0]:.1f}' for k in top))
        a = worst.get('wgrad', (0.0, 0.0))
        worst['wgrad'] = (max([a[0]] + [v[0] for v in rw.values()]), max([a[1]] + [v[1] for v in rw.values()]))
    worst['igrad_x'] = ri['xh_phar.x']
    rest = [v for k, v in ri.items() if k != 'xh_phar.x']
    worst['igrad'] = (max(v[0] for v in rest), max(v[1] for v in rest))
    print(f'\n[f64 floor, training] {case.name}-{engine:5s} half forward {ran_half}  ' + '  '.join(f'{k} {worst[k][0]:.2f} ({worst[k][1]:.2f})' for k in fr.TRAIN_KINDS)
          + '  inputs ' + '  '.join(f'{k} {v[0]:.2f}' for k, v in ri.items()))
    print('\n'.join(lines))
    assert np.isfinite(g1).all() and np.isfinite(g2).all() and all(np.isfinite(v).all() for v in got_in.values())
    check_bounds(engine, worst, fr.TRAIN_BOUNDS, fr.TRAIN_KINDS, f'{case.name}-{engine}')
