"""GPU tests of training and of the derived chains (score, conditional inpaint, edit, the joint chains) on full-atom sample sizes: the
layout of tests/large_layout_ref.py - samples of 128, 129, ~300, 370 and 258 nodes, residue_nf = 11, up to ~85 neighbours per node -
where the per-sample step kernels launch 1024 threads (max_n > 128), the 256- and 64-row per-sample loops take a second trip, the
planner switches the edge and coordinate tiles, and the backward pass sums receiver runs of eleven waves.  Everything is compared with
the oracle or the CPU models run live; the bounds are those of the tests that own them (imported where they are names, quoted with
their owner where they are literals).  Every test prints one line: the worst ratio to its bound and the tile rule the planner resolved.

Margins (large_layout_ref's docstring): no sample is left out of a single evaluation; a score entry inside the 1e-4 band and a chain's
sample from the first evaluation that brings a pair within 2e-5 A of the cutoff are left out, within the caps, and the committed seeds
leave none out on the oracle (test_large_layout_cpu.py)."""
from argparse import Namespace

import numpy as np
import pytest
import torch

import large_layout_ref as L
import score_ref
import helpers
from helpers import GRAD_TOL, LOSS_NAMES, dev, flat_theta, make_handle, rms
from oracle import ref_cpu
from cmdgen_amd import hip_backend
from cmdgen_amd.synthetic import make_state_dict
from bench import bounded_config
from rule_sweep_ref import MARGIN
from chain_kit import model_for, philox_noise, run_chain, run_joint_inpaint, score_entry_ratios as entry_ratios, to_dev

pytestmark = pytest.mark.gpu

MEAN2 = {'inv_sublayers': 2, 'aggregation_method': 'mean'}


def rule(h):
    """the tile rule the planner resolved for the handle's layout, for the log"""
    return 'edge_mt/coord_mt/node_mt = %d/%d/%d' % tuple(h.query(k) for k in ('edge_mt', 'coord_mt', 'node_mt'))


def assert_large_rule(h, H):
    """the layout is on the far side of max_n > 128 (cmdgen_plan.h): 128-row edge and coordinate kernels at width 256 on the split engine,
    64-row tiles elsewhere - the same lay.max_n > 128 gives k_score_step / k_inpaint_step_count their 1024 threads"""
    want = 128 if (H == 256 and h.query('gemm_split') == 1) else 64
    assert h.query('edge_mt') == want and h.query('coord_mt') == want, rule(h)


# ================================================================================ training kernels
_TRAIN_ORACLE = {}


def train_oracle(H, kw):
    """eps and every parameter gradient of ref_cpu.dynamics_forward under a fixed cotangent, once per model (all engines share it)"""
    key = (H, tuple(sorted(kw.items())))
    if key not in _TRAIN_ORACLE:
        L._threads()
        cfg, lay = L.config(H, 2, **kw), L.build()
        sd = L.state_dict_of(cfg, seed=300 + H)
        xh_phar, xh_pocket, t = L.eval_inputs(lay, cfg)
        p = L.params_of(cfg, seed=300 + H)
        leaves = {k: v.clone().requires_grad_(True) for k, v in p.items() if k.startswith('dynamics.')}
        p2 = dict(p); p2.update(leaves)
        want, _ = ref_cpu.dynamics_forward(p2, cfg.as_dict(), torch.from_numpy(xh_phar), torch.from_numpy(xh_pocket), torch.from_numpy(t),
                                           torch.from_numpy(lay['pm']), torch.from_numpy(lay['pb'].mask))
        d_eps = np.random.Generator(np.random.PCG64(H)).normal(size=tuple(want.shape)).astype(np.float32)
        (want * torch.from_numpy(d_eps)).sum().backward()
        grads = {k[len('dynamics.'):]: (None if v.grad is None else v.grad.numpy().reshape(-1)) for k, v in leaves.items()}
        _TRAIN_ORACLE[key] = dict(cfg=cfg, lay=lay, sd=sd, inputs=(xh_phar, xh_pocket, t), want=want.detach().numpy(), d_eps=d_eps, grads=grads)
    return _TRAIN_ORACLE[key]


def grad_ratios(h, grad, want_grads):
    """{name: max |dg| / (GRAD_TOL * max |g|)} of a flat gradient against the oracle's tensors (test_hip_train's bound)"""
    out, checked = {}, 0
    for nm, g_want in want_grads.items():
        off, cnt = h.param_offset(nm)
        g_want = np.zeros(cnt, np.float32) if g_want is None else g_want
        scale = max(float(np.abs(g_want).max()), 1e-6)
        out[nm] = float(np.abs(grad[off:off + cnt] - g_want).max()) / (GRAD_TOL * scale)
        checked += cnt
    assert checked <= grad.size < checked + 4 * len(want_grads) + 4
    return out


@pytest.mark.parametrize('H,kw,engine', [(64, {}, 'default'), (256, {}, 'default'), (256, {}, 'split'), (256, {}, 'fp32'),
                                         (64, MEAN2, 'default'), (256, MEAN2, 'default')],
                         ids=['h64', 'h256-half', 'h256-split', 'h256-fp32', 'h64-mean2', 'h256-mean2-half'])
def test_training_forward_and_backward_vs_oracle_autograd(H, kw, engine):
    """train_forward / train_backward on the layout (L = 2) against autograd through the oracle, in the form of test_hip_train's test of
    that name: eps to 2e-5 max(1, |eps|), every parameter tensor to GRAD_TOL of its own scale; at width 256 on each of the three engines
    as test_hip_autograd selects them, and which engine the forward ran on is asserted (the raw entries repeat nothing)."""
    o = train_oracle(H, kw)
    cfg, lay = o['cfg'], o['lay']
    assert (L.layout_margins(lay) >= MARGIN).all()
    h = make_handle(cfg)
    if engine == 'split':
        h.set_option('half_engine', 0)
    elif engine == 'fp32':
        h.set_gemm_mode(False)
    theta = flat_theta(h, o['sd'])
    h.set_layout(lay['pb'].num_nodes_phar, lay['pb'].size)
    xh_phar, xh_pocket, t = (dev(a) for a in o['inputs'])
    got = h.train_forward(theta, xh_phar, xh_pocket, t).cpu().numpy()
    want = o['want']
    r_eps = float(np.abs(got - want).max()) / (2e-5 * max(1.0, float(np.abs(want).max())))
    grad = torch.zeros_like(theta)
    h.train_backward(dev(o['d_eps']), grad)
    ratios = grad_ratios(h, grad.cpu().numpy(), o['grads'])
    worst = max(ratios, key=ratios.get)
    half_ran = h.query('train_half_ran')
    print(f'training H={H} {kw or ""} {engine}: eps {r_eps:.3f} of its bound, gradients worst {ratios[worst]:.3f} of GRAD_TOL ({worst}); '
          f'{h.query("train_edges")} edges, {rule(h)}, half engine ran {half_ran}')
    assert half_ran == (1 if (H == 256 and engine == 'default') else 0)
    assert r_eps <= 1.0
    assert ratios[worst] <= 1.0, {k: v for k, v in ratios.items() if v > 1.0}
    h.close()


@pytest.mark.parametrize('with_pocket', [False, True])
def test_input_gradients_match_oracle_autograd(with_pocket, monkeypatch):
    """The differentiable EGNNDynamics on the layout: weights and xh_phar / xh_pocket (about 1 000 position rows) / t against autograd
    through the oracle, with and without the pocket output in the loss - helpers.check_against_oracle itself."""
    cfg, lay = L.config(64, 2), L.build()
    sd = L.state_dict_of(cfg, seed=41)
    xh_phar, xh_pocket, t = L.eval_inputs(lay, cfg, seed=2)
    rng = np.random.Generator(np.random.PCG64(3))
    g, gq = rng.normal(size=xh_phar.shape).astype(np.float32), rng.normal(size=xh_pocket.shape).astype(np.float32)
    inp = dict(xh_phar=xh_phar, xh_pocket=xh_pocket, t=t, mask_phar=lay['pm'], mask_pocket=lay['pb'].mask)
    seen, orig = {}, helpers.assert_close

    def recording(got, want, tol, what):
        w = np.zeros_like(got) if want is None else np.asarray(want, dtype=np.float64)
        seen[what] = float(np.abs(np.asarray(got, dtype=np.float64) - w).max()) / (tol * max(float(np.abs(w).max()), 1e-6))
        orig(got, want, tol, what)
    monkeypatch.setattr(helpers, 'assert_close', recording)
    L._threads()
    try:
        dyn, gi, gp = helpers.check_against_oracle(cfg, sd, inp, g, gq, with_pocket)
    finally:
        worst = max(seen, key=seen.get) if seen else None
        print(f'input gradients, pocket output {with_pocket}: worst {seen.get(worst, float("nan")):.3f} of GRAD_TOL ({worst}); inputs: '
              + ', '.join(f'{k} {seen[k]:.3f}' for k in ('xh_phar', 'xh_pocket', 't') if k in seen))
    assert {'xh_phar', 'xh_pocket', 't'} <= set(seen)
    assert gi['xh_pocket'].shape == (int(lay['pb'].size.sum()), 14)


def lightning_model(mode, H=64, n_layers=2):
    """PharPocketDDPM on full-atom pockets (residue_nf = 11), T = 100, the layout's histogram, L.config's weights"""
    from cmdgen_amd.lightning_modules import PharPocketDDPM
    cfg = L.config(H, n_layers, joint=(mode == 'joint'))
    hp = dict(outdir='out', dataset='crossdock_full', datadir='data', batch_size=5, lr=1e-3,
              egnn_params=Namespace(device='cuda', edge_cutoff=6.0, joint_nf=32, hidden_nf=H, n_layers=n_layers, attention=True, tanh=True,
                                    norm_constant=1, inv_sublayers=1, sin_embedding=False, aggregation_method='sum', normalization_factor=100),
              diffusion_params=Namespace(diffusion_steps=L.T, diffusion_noise_schedule='polynomial_2', diffusion_noise_precision=1e-5,
                                         diffusion_loss_type='l2', normalize_factors=[1, 4]),
              num_workers=0, augment_noise=0, augment_rotation=False, clip_grad=True, eval_epochs=50,
              eval_params=Namespace(n_eval_samples=10, eval_batch_size=10), mode=mode, node_histogram=L.HIST, pocket_representation='full-atom')
    model = PharPocketDDPM(**hp)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in L.state_dict_of(cfg).items()}, strict=True)
    return cfg, model.cuda()


def batch_of(lay):
    phar, pocket = L.dicts(lay)
    return {'phar_coords': phar['x'], 'phar_one_hot': phar['one_hot'], 'num_phar_atoms': phar['size'], 'phar_mask': phar['mask'],
            'pocket_c_alpha': pocket['x'], 'pocket_one_hot': pocket['one_hot'], 'num_pocket_nodes': pocket['size'], 'pocket_mask': pocket['mask']}


def joint_eps(lay, noise):
    Nl, Np = len(lay['pm']), len(lay['pb'].mask)
    return [(dev(row[:Nl * 11].reshape(Nl, 11).copy()), dev(row[Nl * 11:].reshape(Np, 14).copy())) for row in noise]


@pytest.mark.parametrize('mode', ['train', 'eval'])
def test_loss_terms_match_oracle(mode):
    """ConditionalDDPM.forward's twelve terms and PharPocketDDPM.forward's nll on the layout against ref_cpu.ddpm_forward, t = 0 and t = T
    in the batch; tolerances of test_hip_parity.test_loss_terms_match_reference (terms rtol 1e-4, atol 1e-4 max(1, |want|); nll rtol
    1e-4, atol 1e-3)."""
    o = L.oracle_loss(mode)
    assert (o['margins'] >= MARGIN).all()
    cfg, model = lightning_model('pocket_conditioning')
    model.train() if mode == 'train' else model.eval()
    phar, pocket = L.dicts(o['lay'])
    terms = model.ddpm(to_dev(phar), to_dev(pocket), return_info=True, t_int=o['t_int'], eps=o['eps'])
    worst = (0.0, None)
    for n, v, want in zip(LOSS_NAMES, terms[:-1], o['terms'][:-1]):
        want = np.asarray(want.numpy() if torch.is_tensor(want) else want, dtype=np.float32)
        got = np.asarray(v.detach().cpu().numpy() if torch.is_tensor(v) else v, dtype=np.float32)
        tol = 1e-4 * max(1.0, float(np.abs(want).max())) + 1e-4 * np.abs(want)
        r = float((np.abs(got - want) / tol).max())
        worst = (r, n) if r >= worst[0] else worst
        assert np.allclose(got, want, rtol=1e-4, atol=1e-4 * max(1.0, float(np.abs(want).max()))), (n, got, want)
    nll, info = model(batch_of(o['lay']), t_int=o['t_int'], eps=o['eps'])
    d = np.abs(nll.cpu().numpy() - o['nll'].numpy()) / (1e-3 + 1e-4 * np.abs(o['nll'].numpy()))
    print(f'loss terms ({mode}): worst {worst[0]:.3f} of its tolerance ({worst[1]}), nll {float(d.max()):.3f}; {rule(model.ddpm.dynamics.hip_handle())}')
    assert np.allclose(nll.cpu().numpy(), o['nll'].numpy(), rtol=1e-4, atol=1e-3)


@pytest.mark.parametrize('mode', ['train', 'eval'])
def test_joint_loss_terms_match_oracle(mode):
    """EnVariationalDiffusion.forward on the layout with residue_nf = 11 against ref_cpu.joint_ddpm_forward; every term to 2e-5 max(1, |want|)
    (test_hip_joint.test_joint_loss_terms_match_reference)."""
    o = L.oracle_joint_loss(mode)
    assert (o['margins'] >= MARGIN).all()
    cfg, model = lightning_model('joint')
    ddpm = model.ddpm
    ddpm.train() if mode == 'train' else ddpm.eval()
    phar, pocket = L.dicts(o['lay'])
    terms = ddpm(to_dev(phar), to_dev(pocket), return_info=True, t_int=o['t_int'].cuda(), eps=joint_eps(o['lay'], o['noise']))
    worst = (0.0, None)
    for n, v, want in zip(LOSS_NAMES, terms[:-1], o['terms'][:-1]):
        want = np.asarray(want.numpy() if torch.is_tensor(want) else want, dtype=np.float32)
        got = np.asarray(v.detach().cpu().numpy() if torch.is_tensor(v) else v, dtype=np.float32)
        assert got.shape == want.shape, n
        r = float(np.abs(got - want).max()) / (2e-5 * max(1.0, float(np.abs(want).max())))
        worst = (r, n) if r >= worst[0] else worst
    print(f'joint loss terms ({mode}): worst {worst[0]:.3f} of its tolerance ({worst[1]}); {rule(ddpm.dynamics.hip_handle())}')
    assert worst[0] <= 1.0, worst
    for kk, v in terms[-1].items():
        assert abs(float(v) - float(o['terms'][-1][kk])) < 2e-5, kk


_STEP_ORACLE = {}


def step_oracle(mode):
    """nll and parameter gradients of the l2 training loss by autograd through the oracle, on the loss case's draws"""
    if mode not in _STEP_ORACLE:
        L._threads()
        joint = mode == 'joint'
        o = L.oracle_joint_loss('train') if joint else L.oracle_loss('train')
        cfg, lay = o['cfg'], o['lay']
        phar, pocket = L.dicts(lay)
        p = L.params_of(cfg)
        leaves = {k: v.clone().requires_grad_(True) for k, v in p.items() if k.startswith('dynamics.')}
        p2 = dict(p); p2.update(leaves)
        if joint:
            from helpers import JointNoiseTape
            tape = JointNoiseTape(o['noise'], len(lay['pm']), len(lay['pb'].mask), R=11)
            terms = ref_cpu.joint_ddpm_forward(p2, cfg.as_dict(), phar, pocket, o['t_int'], tape, True, L.HIST)
        else:
            terms = ref_cpu.ddpm_forward(p2, cfg.as_dict(), phar, pocket, o['t_int'], o['eps'], True, L.HIST)
        nll = ref_cpu.nll_from_terms(terms, cfg.as_dict(), phar['size'], pocket['size'], True)
        nll.mean(0).backward()
        _STEP_ORACLE[mode] = dict(o=o, nll=nll.detach().numpy(), grads={k[len('dynamics.'):]: (None if v.grad is None else v.grad.numpy().reshape(-1))
                                                                         for k, v in leaves.items()})
    return _STEP_ORACLE[mode]


@pytest.mark.parametrize('mode', ['pocket_conditioning', 'joint'])
def test_training_step_matches_oracle_gradients_and_optimizer(mode):
    """One full HipTrainer step on the layout - cmdgen_train_noise / cmdgen_train_loss (mode 'joint': their _joint forms, pocket rows of width
    14) with more than 256 pocket and more than 64 phar rows in a sample, the activation-saving forward, the backward pass, clipping and
    AdamW(amsgrad) - with the oracle's autograd in G11's place.
    'pocket_conditioning' compares as test_hip_train.test_training_step_matches_reference_gradients_and_optimizer does: loss 2e-6, nll 1e-5
    (of max(1, max |nll|): G11's nll are O(1), this layout's are not), every gradient tensor GRAD_TOL, the gradient norm 1e-4, and after the
    update every element whose gradient is significant within 5e-5 of torch's AdamW(amsgrad) on the oracle's gradient.
    'joint' has no G11; its nll bound is the one test_hip_train.test_joint_training_gradients_vs_oracle_autograd asserts against the
    oracle, 2e-5 max(1, max |nll|), the rest as above (the loss, a mean of five such nll, is printed)."""
    from cmdgen_amd.training import HipTrainer
    so = step_oracle(mode)
    o = so['o']
    assert (o['margins'] >= MARGIN).all()
    cfg, model = lightning_model(mode)
    tr = HipTrainer(model)
    assert tr._fused_ok() and tr._variant() == ('joint' if mode == 'joint' else 'conditional')
    eps = joint_eps(o['lay'], o['noise'][:1]) if mode == 'joint' else [o['eps'][0].cuda()]
    loss, nll, info = tr.loss_and_grad(batch_of(o['lay']), t_int=o['t_int'].cuda(), eps=eps)
    scale = max(1.0, float(np.abs(so['nll']).max()))
    r_nll = float(np.abs(nll.cpu().numpy() - so['nll']).max()) / ((2e-5 if mode == 'joint' else 1e-5) * scale)
    r_loss = abs(float(loss) - float(so['nll'].mean())) / (2e-6 * scale)
    grad = tr.grad.cpu().numpy()
    ratios = grad_ratios(tr.h, grad, so['grads'])
    worst = max(ratios, key=ratios.get)
    # the update: free (the queue holds 3000, the bound is 4500)
    theta0 = tr.theta.clone()
    grad_norm, mx = tr.optimizer_step()
    flat = np.zeros_like(grad)
    for nm, gw in so['grads'].items():
        off, cnt = tr.h.param_offset(nm)
        if gw is not None:
            flat[off:off + cnt] = gw
    want_norm = float(np.linalg.norm(flat.astype(np.float64)))
    ref = theta0.cpu().clone().requires_grad_(True)
    opt = torch.optim.AdamW([ref], lr=tr.lr, betas=tr.betas, eps=tr.eps, weight_decay=tr.weight_decay, amsgrad=True)
    ref.grad = torch.from_numpy(flat)
    opt.step()
    moved = np.abs(tr.theta.cpu().numpy() - ref.detach().numpy())
    sig = np.abs(flat) > 1e-3 * np.abs(flat).max()
    print(f'training step ({mode}): loss {r_loss:.3f} of 2e-6 max(1, |nll|), nll {r_nll:.3f} of its bound (max |nll| {scale:.1f}), gradients worst '
          f'{ratios[worst]:.3f} of GRAD_TOL ({worst}), norm {abs(grad_norm - want_norm) / (1e-4 * want_norm):.3f}, significant parameters '
          f'{float(moved[sig].max()) / 5e-5:.3f} of their bounds; {tr.h.query("train_edges")} edges, {rule(tr.h)}')
    assert r_nll <= 1.0
    if mode != 'joint':
        assert r_loss <= 1.0
    assert ratios[worst] <= 1.0, {k: v for k, v in ratios.items() if v > 1.0}
    if mode == 'joint':
        assert all(g is not None and np.abs(g).max() > 0 for g in so['grads'].values())          # the residue decoder is trained in joint mode
    assert grad_norm < mx and abs(grad_norm - want_norm) <= 1e-4 * want_norm
    assert sig.any() and float(moved[sig].max()) < 5e-5
    assert float(moved.max()) <= 3 * 1e-3 * 2 + 1e-6


# ================================================================================ chains against the CPU models, injected draws
def kept_rows(lay, kept):
    """(phar rows, pocket rows) bool of the kept samples"""
    return kept[lay['pm']], kept[lay['pb'].mask]


def check_kept(margins, what):
    kept = L.kept_from(margins)
    assert (~kept).sum() <= L.MAX_LEFT_OUT, f'{what}: {(~kept).sum()} samples inside the band: more than CHAIN_CAP'
    return kept


@pytest.mark.parametrize('use_graph', [True, False])
def test_score_matches_the_cpu_model(use_graph):
    """Five levels and the t = 0 level against score_ref.score_levels: every kept (level, sample) entry to score_ref.error_bound, kl_prior and
    the categorical term to their bounds of test_hip_score.test_score_matches_g21."""
    o = L.oracle_score()
    cfg, lay, raw, K = o['cfg'], o['lay'], o['raw'], L.SCORE_K
    phar, pocket = L.dicts(lay)
    ddpm = model_for(cfg, L.state_dict_of(cfg), hist=L.HIST).eval()
    ddpm.use_hip_graph = use_graph
    out = ddpm.score(to_dev(phar), to_dev(pocket), timesteps=K, noise=dev(o['noise']), return_levels=True)
    out = {k: v.cpu().numpy() for k, v in out.items()}
    st = ddpm.last_chain_status
    h = ddpm.dynamics.hip_handle()
    assert_large_rule(h, 64)
    assert st['max_rel_com_error'] < 1e-2 and st['nan_resets'] == 0
    assert list(out['t_levels']) == o['levels']
    sums = out['level_sums'][0]
    keep = o['margins'] >= L.SCORE_BAND
    left_out = int((~keep).sum())
    assert left_out <= L.SCORE_CAP * keep.size, f'{left_out} of {keep.size} entries inside the band: more than 2 %'
    n_rows = lay['pb'].num_nodes_phar
    want_err, want_l0x = raw['err'][:K].numpy().astype(np.float64), 0.5 * raw['err_x'][K].numpy().astype(np.float64)
    ratios = entry_ratios(sums, want_err, want_l0x, raw['netmax'].numpy(), n_rows, keep)
    print(f'score graph={use_graph}: {left_out} entries left out, worst |d error| / bound {ratios.max():.3e} over {ratios.size} entries; {rule(h)}')
    assert ratios.max() <= 1.0
    assert (sums[..., 3] == 0).all() and (sums[:K, :, 2] == 0).all()
    if keep[K].all():
        assert np.allclose(out['loss_0_h'], -raw['log_ph'][K].numpy(), rtol=1e-4, atol=1e-3)
        assert np.allclose(out['loss_0_x'], 0.5 * sums[K, :, 1], rtol=0, atol=0)
    want_kl = raw['kl_prior'].numpy()
    assert np.allclose(out['kl_prior'], want_kl, rtol=2e-5, atol=2e-5 * max(1.0, float(np.abs(want_kl).max())))
    assert np.isfinite(out['nll']).all()


def compare_conditional_chain(what, use_graph, h, o, xh_phar, xh_pocket, z_steps, p_steps, st):
    """bounds of test_inpaint_chain_matches_g20 / test_edit_chain_matches_g22: coordinate RMS <= 1e-4 max(1, max |x|), types exact, z and the
    pocket after every op max-abs <= 1e-4 max(1, max |.|) - over the rows of the kept samples"""
    lay = o['lay']
    kept = check_kept(o['margins'], what)
    rp, rq = kept_rows(lay, kept)
    want, wq = o['want'][0][rp], o['want'][1][rq]
    r_x = rms(xh_phar[rp][:, :3], want[:, :3]) / (1e-4 * max(1.0, float(np.abs(want[:, :3]).max())))
    r_q = rms(xh_pocket[rq], wq) / (1e-4 * max(1.0, float(np.abs(wq).max())))
    zs, ps = o['z_steps'][:, rp], o['p_steps'][:, rq]
    assert z_steps.shape == o['z_steps'].shape and p_steps.shape == o['p_steps'].shape
    r_z = max(float(np.abs(z_steps[k][rp] - zs[k]).max()) / (1e-4 * max(1.0, float(np.abs(zs[k]).max()))) for k in range(len(zs)))
    r_p = max(float(np.abs(p_steps[k][rq] - ps[k]).max()) / (1e-4 * max(1.0, float(np.abs(ps[k]).max()))) for k in range(len(ps)))
    print(f'{what} graph={use_graph}: {int((~kept).sum())} samples left out; of their bounds: final x {r_x:.3f}, pocket {r_q:.3f}, z per op {r_z:.3f}, '
          f'pocket per op {r_p:.3f}; max |x| {float(np.abs(want[:, :3]).max()):.1f}; {rule(h)}')
    assert_large_rule(h, 64)
    assert max(r_x, r_q, r_z, r_p) <= 1.0
    assert np.array_equal(xh_phar[rp][:, 3:], want[:, 3:])
    assert st['max_rel_com_error'] < 1e-2 and st['nan_resets'] == 0


@pytest.mark.parametrize('use_graph', [True, False])
def test_inpaint_chain_matches_the_cpu_model(use_graph):
    """K = 4, r = 2, j = 1 against cond_inpaint_ref.cond_inpaint: z after every op, then the final rows and types; fixed rows
    large_layout_ref.fixed_rows (the fixed / free split of the 70-point sample falls across a wavefront)."""
    o = L.oracle_inpaint()
    cfg, lay = o['cfg'], o['lay']
    h = make_handle(cfg)
    h.load_state_dict(L.state_dict_of(cfg))
    got, st = run_chain(h, lay['pb'], L.INPAINT['K'], given=(lay['phar_x'], lay['phar_one_hot'], o['fixed']), plan=(None, L.INPAINT['r'], L.INPAINT['j']),
                        noise=dev(o['noise']), use_graph=use_graph, tables=False)
    compare_conditional_chain('inpaint', use_graph, h, o, got.xh_phar, got.xh_pocket, got.z_steps, got.pocket_steps, st)
    h.close()


@pytest.mark.parametrize('use_graph', [True, False])
def test_edit_chain_matches_the_cpu_model(use_graph):
    """K = 6, start = 3, r = 2, j = 1 with mixed fix_x / fix_h masks (large_layout_ref.edit_masks) against edit_ref.cond_edit: the only route
    into k_edit_start with large samples."""
    o = L.oracle_edit()
    cfg, lay = o['cfg'], o['lay']
    h = make_handle(cfg)
    h.load_state_dict(L.state_dict_of(cfg))
    e = L.EDIT
    got, st = run_chain(h, lay['pb'], e['K'], given=(lay['phar_x'], lay['phar_one_hot'], o['fix_x'], o['fix_h']), plan=(e['start'], e['r'], e['j']),
                        noise=dev(o['noise']), use_graph=use_graph, tables=False)
    compare_conditional_chain('edit', use_graph, h, o, got.xh_phar, got.xh_pocket, got.z_steps, got.pocket_steps, st)
    h.close()


@pytest.mark.parametrize('use_graph', [True, False])
@pytest.mark.parametrize('kind', ['sample', 'inpaint'])
def test_joint_chains_match_the_oracle(kind, use_graph):
    """ref_cpu.joint_sample (K = 4) and ref_cpu.joint_inpaint (K = 4, r = 2, j = 1) on the update_pocket_coords model with residue_nf = 11 (pocket
    rows of width 14 noised, projected and decoded); bounds of test_hip_joint.test_joint_inpaint_schedules_vs_oracle: z after every step
    max-abs < 2e-4 max(1, max |z|), final types exact, coordinate RMS <= 1e-4 max(1, max |x|)."""
    o = L.oracle_joint(kind)
    cfg, lay = o['cfg'], o['lay']
    pb = lay['pb']
    h = make_handle(cfg)
    h.load_state_dict(L.state_dict_of(cfg))
    if kind == 'sample':
        h.set_layout(pb.num_nodes_phar, pb.size)
        xh_phar, xh_pocket, z_steps = h.joint_chain(o['K'], noise=dev(o['noise']), want_steps=True, use_graph=use_graph)
    else:
        phar = {'x': lay['phar_x'], 'one_hot': lay['phar_one_hot'], 'size': pb.num_nodes_phar, 'mask': lay['pm']}
        pocket = {'x': pb.x, 'one_hot': pb.one_hot, 'size': pb.size, 'mask': pb.mask}
        xh_phar, xh_pocket, z_steps = run_joint_inpaint(h, phar, pocket, o['fixed'][0], o['fixed'][1], o['K'], o['r'], o['j'], o['noise'],
                                                        use_graph, want_steps=True)
    st = h.chain_status()
    assert h.joint_plan(o['K'], o['r'], o['j'], kind == 'inpaint') == (o['n_steps'], o['n_draws'])
    kept = check_kept(o['margins'], 'joint ' + kind)
    rp, rq = kept_rows(lay, kept)
    cols = np.concatenate([np.repeat(rp, 11), np.repeat(rq, 14)])
    z = z_steps.cpu().numpy()
    assert z.shape == o['chain'].shape
    r_z = max(float(np.abs(z[s][cols] - o['chain'][s][cols]).max()) / (2e-4 * max(1.0, float(np.abs(o['chain'][s][cols]).max()))) for s in range(len(z)))
    r_x = 0.0
    for got, ref, rows in ((xh_phar.cpu().numpy(), o['want'][0], rp), (xh_pocket.cpu().numpy(), o['want'][1], rq)):
        assert np.array_equal(got[rows][:, 3:], ref[rows][:, 3:])
        r_x = max(r_x, rms(got[rows][:, :3], ref[rows][:, :3]) / (1e-4 * max(1.0, float(np.abs(ref[rows][:, :3]).max()))))
    print(f'joint {kind} graph={use_graph}: {int((~kept).sum())} samples left out; of their bounds: z per step {r_z:.3f}, final x {r_x:.3f}; {rule(h)}')
    assert_large_rule(h, 64)
    assert r_z < 1.0 and r_x <= 1.0
    assert st['max_rel_com_error'] < 1e-2 and st['nan_resets'] == 0
    h.close()


# ================================================================================ device draws: graph against eager, batch independence
def shipped_width_model(joint=False):
    """width 256 (the 128-row edge kernels keep a receiver of up to ~128 edges at two float-atomic partials, so a chain is reproducible
    bit for bit: test_hip_properties.test_chains_are_reproducible_bit_for_bit), two blocks, bench.bounded_config's schedule and weights:
    coordinates stay bounded, the graph stays dense"""
    from dataclasses import replace
    cfg = replace(bounded_config(11, 1000), n_layers=2, update_pocket_coords=joint)
    return cfg, make_state_dict(cfg, seed=0)


def device_draw_chain(h, lay, kind, use_graph, seed=13):
    """one chain of `kind` with device draws keyed by the samples' pocket ids -> list of arrays"""
    pb, ids = lay['pb'], lay['ids']
    h.set_layout(pb.num_nodes_phar, pb.size)
    if kind == 'score':
        terms, kl = h.score_chain(dev(lay['phar_x']), dev(lay['phar_one_hot']), dev(pb.x), dev(pb.one_hot), [800, 600, 400, 200, 0], seed=seed,
                                  pocket_ids=ids, use_graph=use_graph)
        out = [terms, kl]
    elif kind == 'inpaint':
        out = h.inpaint_chain(dev(pb.x), dev(pb.one_hot), dev(lay['phar_x']), dev(lay['phar_one_hot']), dev(L.fixed_rows(lay)), 4, resamplings=2,
                              jump_length=1, seed=seed, pocket_ids=ids, use_graph=use_graph, want_steps=True)
    elif kind == 'edit':
        fx, fh = L.edit_masks(lay)
        out = h.edit_chain(dev(pb.x), dev(pb.one_hot), dev(lay['phar_x']), dev(lay['phar_one_hot']), dev(fx), dev(fh), 6, start=3, resamplings=2,
                           jump_length=1, seed=seed, pocket_ids=ids, use_graph=use_graph, want_steps=True)
    else:
        fp, fq = L.joint_fixed(lay)
        out = h.joint_chain(4, phar=(dev(lay['phar_x']), dev(lay['phar_one_hot'])), pocket=(dev(pb.x), dev(pb.one_hot)), phar_fixed=dev(fp),
                            pocket_fixed=dev(fq), resamplings=2, jump_length=1, seed=seed, pocket_ids=ids, use_graph=use_graph, want_steps=True)
    st = h.chain_status()
    assert st['nan_resets'] == 0
    return [t.cpu().numpy() for t in out if t is not None]


@pytest.mark.parametrize('kind', ['score', 'inpaint', 'edit', 'joint'])
def test_graph_runs_equal_eager_runs(kind):
    """Each chain with device draws keyed by pocket id, captured and eager.  The conditional chains (score, inpaint, edit): identical bits,
    a repeated captured run too.  The joint chain: what test_hip_joint.test_joint_graph_runs_equal_eager_runs_as_the_key_changes asserts,
    types exact and coordinates and saved steps within 1e-3 max(1, max |x|) - its chain starts with every node of a sample inside the cutoff
    of every other (369 edges per receiver here), a receiver's sum is then more than the two float-atomic partials whose order does not
    matter (make_plan, cmdgen_plan.h), and two runs of the SAME kind differ as much as a captured and an eager one: both differences are
    printed, and the captured-against-eager one may not exceed the bound either way."""
    cfg, sd = shipped_width_model(joint=(kind == 'joint'))
    h = make_handle(cfg)
    h.load_state_dict(sd)
    lay = L.build()
    graph = device_draw_chain(h, lay, kind, True)
    eager = device_draw_chain(h, lay, kind, False)
    again = device_draw_chain(h, lay, kind, True)
    assert_large_rule(h, 256)
    diff = max(float(np.abs(a - b).max()) for a, b in zip(graph, eager))
    rerun = max(float(np.abs(a - c).max()) for a, c in zip(graph, again))
    print(f'{kind} with device draws: captured against eager max |d| {diff:.1e}, captured against captured {rerun:.1e}, over {len(graph)} outputs; {rule(h)}')
    assert len(graph) == len(eager) == len(again) >= 2
    assert all(np.isfinite(a).all() for a in graph)
    if kind != 'joint':
        for a, b, c in zip(graph, eager, again):
            assert np.array_equal(a, b) and np.array_equal(a, c)
    else:
        (gp, gq, gz), (ep, eq, ez), (cp, cq, cz) = graph, eager, again
        scale = max(1.0, float(np.abs(ep[:, :3]).max()), float(np.abs(eq[:, :3]).max()))
        for a, b in ((gp, ep), (gq, eq), (gp, cp), (gq, cq)):
            assert np.array_equal(a[:, 3:], b[:, 3:])
            assert float(np.abs(a[:, :3] - b[:, :3]).max()) < 1e-3 * scale
        assert float(np.abs(gz - ez).max()) < 1e-3 * scale and float(np.abs(gz - cz).max()) < 1e-3 * scale
    h.close()


def test_an_inpainted_sample_does_not_depend_on_its_batch():
    """The whole layout against each sample alone (same pocket ids, same device draws): types identical, coordinates within the bounds of
    test_hip_properties.test_a_pockets_chain_does_not_depend_on_its_batch_at_256_pockets (1e-4 A max, 1e-5 A RMS).  The 128-node sample alone
    runs the 256-thread k_inpaint_step_count and the small-layout tiles, inside the batch the 1024-thread one."""
    cfg, sd = shipped_width_model()
    h = make_handle(cfg)
    h.load_state_dict(sd)
    whole_lay = L.build()
    whole = device_draw_chain(h, whole_lay, 'inpaint', True)[0]
    assert_large_rule(h, 256)
    rules = [rule(h)]
    parts = []
    for k in range(L.B):
        parts.append(device_draw_chain(h, L.build(samples=[k]), 'inpaint', True)[0])
        rules.append(rule(h))
        if k == 0:
            assert h.query('edge_mt') < 128          # 128 nodes: the small side of max_n > 128
    parts = np.concatenate(parts)
    d = np.abs(whole[:, :3] - parts[:, :3])
    print(f'inpaint, the layout against each sample alone: coordinates max {float(d.max()):.1e} A ({float(d.max()) / 1e-4:.3f} of its bound), RMS '
          f'{float(np.sqrt(np.mean(d ** 2))):.1e} A ({float(np.sqrt(np.mean(d ** 2))) / 1e-5:.3f}); whole: {rules[0]}; alone: ' + '; '.join(rules[1:]))
    assert np.array_equal(whole[:, 3:], parts[:, 3:])
    assert float(d.max()) <= 1e-4 and float(np.sqrt(np.mean(d ** 2))) <= 1e-5
    h.close()


def test_a_scored_sample_does_not_depend_on_its_batch():
    """Score entries of the whole layout against each sample alone, same pocket ids and device draws: within score_ref.error_bound of each
    other (err and max |net| from the CPU model at the same Philox draws; an entry inside the band is left out, at most 2 %)."""
    cfg, lay = L.config(), L.build()
    sd = L.state_dict_of(cfg)
    ddpm = model_for(cfg, sd, hist=L.HIST).eval()
    phar, pocket = L.dicts(lay)
    K, seed, ids = L.SCORE_K, L.SEEDS['score_device'], [int(i) for i in lay['ids']]
    whole = ddpm.score(to_dev(phar), to_dev(pocket), timesteps=K, seed=seed, pocket_ids=ids, return_levels=True)
    h = ddpm.dynamics.hip_handle()
    assert_large_rule(h, 64)
    rules = [rule(h)]
    nl = lay['pb'].num_nodes_phar
    noise = philox_noise(h, seed, ids, nl, range(K + 1)).cpu().numpy()
    L._threads()
    with torch.no_grad(), L.RecordedEdges() as rec:
        raw = score_ref.score_levels(L.params_of(cfg), cfg.as_dict(), phar, pocket, whole['t_levels'].tolist(), noise)
    keep = rec.array() >= L.SCORE_BAND
    assert (~keep).sum() <= L.SCORE_CAP * keep.size
    sums = whole['level_sums'][0].cpu().numpy()
    want_err, want_l0x = raw['err'][:K].numpy().astype(np.float64), 0.5 * raw['err_x'][K].numpy().astype(np.float64)
    r_oracle = entry_ratios(sums, want_err, want_l0x, raw['netmax'].numpy(), nl, keep)
    alone = []
    for k in range(L.B):
        one = L.build(samples=[k])
        ph1, pk1 = L.dicts(one)
        alone.append(ddpm.score(to_dev(ph1), to_dev(pk1), timesteps=K, seed=seed, pocket_ids=[ids[k]], return_levels=True)['level_sums'][0].cpu().numpy())
        rules.append(rule(h))
    alone = np.concatenate(alone, axis=1)
    b_t = score_ref.error_bound(want_err, raw['netmax'].numpy()[:K], nl, 11)
    b_0 = score_ref.error_bound(2.0 * want_l0x, raw['netmax'].numpy()[K], nl, 3)
    d_t = (np.abs(alone[:K, :, 0].astype(np.float64) - sums[:K, :, 0]) / b_t)[keep[:K]]
    d_0 = (np.abs(alone[K, :, 1].astype(np.float64) - sums[K, :, 1]) / b_0)[keep[K]]
    print(f'score, the layout against each sample alone: worst |d error| / bound {max(d_t.max(), d_0.max()):.3e}, against the CPU model {r_oracle.max():.3e}, '
          f'{int((~keep).sum())} entries left out; whole: {rules[0]}; alone: ' + '; '.join(rules[1:]))
    assert r_oracle.max() <= 1.0
    assert d_t.max() <= 1.0 and d_0.max() <= 1.0
