"""GPU tests of the opt-in differentiable EGNNDynamics (cmdgen_amd.autograd, cmdgen_train_backward_inputs): gradients to the weights and to
xh_phar / xh_pocket / t against autograd through the oracle, against the library's own parameter pass, by finite differences, through two
forwards before one backward, through the reference's training idiom, with the switch off, and on the half engine's overflow case.

Tolerances as tests/test_hip_train.py: a tensor's gradient max|dg| <= GRAD_TOL * max|g| of that tensor.  The library's passes add with float
atomics, so two runs of the same pass agree up to the order of those sums; "the same pass" is checked to SAME_TOL of a tensor's scale.
"""
import numpy as np
import pytest
import torch

from helpers import (GRAD_TOL, assert_close, autograd_case as case, build_trainer, check_against_oracle, dev, hip_grads, make_module, npy,
                     oracle_grads)

pytestmark = pytest.mark.gpu
SAME_TOL = 2e-5


# ------------------------------------------------------------------ 1 + 2: weights and inputs against the oracle
@pytest.mark.parametrize('H,L,B,kw,engine', [
    (64, 2, 3, {}, 'default'),
    (128, 2, 2, {'attention': False, 'tanh': False}, 'default'),
    (64, 2, 2, {'inv_sublayers': 2, 'aggregation_method': 'mean'}, 'default'),
    (256, 3, 3, {}, 'default'),                 # the half engine (default at 256 with an edge cutoff)
    (256, 3, 3, {}, 'split'),                   # the three-piece bf16 engine
    (256, 2, 2, {}, 'fp32'),                    # the fp32 instruction
    (256, 2, 2, {'inv_sublayers': 2, 'aggregation_method': 'mean'}, 'default'),
])
def test_weight_and_input_gradients_match_oracle_autograd(H, L, B, kw, engine):
    cfg, sd, inp, g, gq = case(H, L, B, 40 + H + L + B, **kw)
    dyn = make_module(cfg, sd)
    h = dyn.hip_handle()
    if engine == 'split':
        h.set_option('half_engine', 0)
    elif engine == 'fp32':
        h.set_gemm_mode(False)
    check_against_oracle(cfg, sd, inp, g, gq, False, dyn=dyn)
    # the engine the forward actually ran on: the half engine wherever it is the default (width 256 with an edge cutoff)
    assert h.query('train_half_ran') == (1 if (H == 256 and engine == 'default') else 0)


@pytest.mark.parametrize('variant', ['simple', 'conditional_pocket_output'])
def test_simple_handle_and_conditional_pocket_output_match_oracle_autograd(variant):
    """A SimpleConditionalDDPM handle (no_com_projection; the network is the conditional one), and a conditional handle whose loss reads
    the pocket output as well (d_eps_pocket: the residue decoder, and the pocket velocity - identically zero - passes nothing)."""
    cfg, sd, inp, g, gq = case(64, 2, 3, 123)
    dyn = make_module(cfg, sd)
    if variant == 'simple':
        dyn._cfg['no_com_projection'] = True
    check_against_oracle(cfg, sd, inp, g, gq, variant == 'conditional_pocket_output', dyn=dyn)
    assert dyn.hip_handle().cfg.get('no_com_projection', False) == (variant == 'simple')


def test_bf16_operands_agree_with_oracle_autograd_to_bf16_accuracy():
    """GEMM operands in bf16 (cmdgen_train_set_precision): weight and input gradients point the oracle's way and have its size, to bf16
    accuracy (as test_hip_train.py's bf16 training test)."""
    cfg, sd, inp, g, gq = case(256, 2, 3, 131)
    dyn = make_module(cfg, sd)
    with torch.no_grad():
        dyn(*[dev(inp[k]) for k in ('xh_phar', 'xh_pocket', 't', 'mask_phar', 'mask_pocket')])      # (a layout for the handle)
    dyn.hip_handle().train_set_precision(True)
    _, gi, gp = hip_grads(dyn, inp, g, gq, False)
    _, wi, wp = oracle_grads(cfg, sd, inp, g, gq, False)
    flat = lambda d: np.concatenate([np.zeros(p.numel(), np.float32) if d[k] is None else npy(d[k]).reshape(-1)
                                     for k, p in dyn.named_parameters()])          # (None: a tensor the loss does not reach)
    got, want = flat(gp), flat(wp)
    for name, a, b in [('weights', got, want)] + [(k, npy(gi[k]).reshape(-1), npy(wi[k]).reshape(-1)) for k in ('xh_phar', 'xh_pocket', 't')]:
        cos = float(np.dot(a, b) / (np.linalg.norm(a) * np.linalg.norm(b)))
        assert cos > 0.999 and abs(np.linalg.norm(a) / np.linalg.norm(b) - 1.0) < 2e-2, (name, cos)
    assert np.abs(got - want).max() > 1e-6 * np.abs(want).max()                # not the fp32 path


def test_backward_after_another_evaluation_reruns_its_forward():
    """A differentiable forward, then evaluations on the same handle that rewrite its graph - a no_grad call at other inputs of the same
    layout, one at another layout - then backward: the gradient is the single call's.  The C entry itself refuses a forward whose graph
    was replaced."""
    from cmdgen_amd import hip_backend
    cfg, sd, inp, g, gq = case(64, 2, 3, 141)
    _, _, inp_b, _, _ = case(64, 2, 2, 142)                     # another batch: 2 samples, another layout
    dyn = make_module(cfg, sd)
    _, want_i, want_p = hip_grads(dyn, inp, g, gq, False)
    for other in ('same_layout', 'other_layout'):
        xp, xq, t = (dev(inp[k]).requires_grad_(True) for k in ('xh_phar', 'xh_pocket', 't'))
        eps, _ = dyn(xp, xq, t, dev(inp['mask_phar']), dev(inp['mask_pocket']))
        with torch.no_grad():
            if other == 'same_layout':
                moved = inp['xh_phar'].copy(); moved[:, :3] += 0.7
                dyn(dev(moved), dev(inp['xh_pocket']), dev(inp['t']) * 0.5, dev(inp['mask_phar']), dev(inp['mask_pocket']))
            else:
                dyn(*[dev(inp_b[k]) for k in ('xh_phar', 'xh_pocket', 't', 'mask_phar', 'mask_pocket')])
        names = [n for n, _ in dyn.named_parameters()]
        gr = torch.autograd.grad((eps * dev(g)).sum(), [xp, xq, t] + list(dyn.parameters()))
        for k, v in zip(('xh_phar', 'xh_pocket', 't'), gr[:3]):
            assert_close(npy(v), npy(want_i[k]), SAME_TOL, (other, k))
        for n, v in zip(names, gr[3:]):
            assert_close(npy(v), npy(want_p[n]), SAME_TOL, (other, n))
    # the raw entry: an evaluation between the training forward and the input pass is refused, not differentiated on the wrong graph
    h = dyn.hip_handle()
    from cmdgen_amd.autograd import flat_theta
    theta = flat_theta(h, dyn, list(dyn.parameters())).clone()
    h.set_layout(*dyn._layout_from_masks(dev(inp['mask_phar']), dev(inp['mask_pocket']), 3))
    xp, xq, t = dev(inp['xh_phar']), dev(inp['xh_pocket']), dev(inp['t'])
    h.train_forward(theta, xp, xq, t, want_pocket=True)
    h.dynamics_forward(xp, xq, t)
    with pytest.raises(hip_backend.CmdgenError, match='replaced the graph'):
        h.train_backward_inputs(dev(g), None, None, torch.empty_like(xp), None, None)


@pytest.mark.parametrize('H,with_pocket', [(64, False), (64, True), (256, True)])
def test_joint_handle_input_gradients_match_oracle_autograd(H, with_pocket):
    """update_pocket_coords True: every row moves, the velocity's centre of mass is removed; with_pocket: the loss reads the pocket output
    too (d_eps_pocket)."""
    cfg, sd, inp, g, gq = case(H, 2, 3, 90 + H, update_pocket_coords=True)
    check_against_oracle(cfg, sd, inp, g, gq, with_pocket)


def test_weight_gradient_equals_the_parameter_pass():
    """The Function's parameter gradient is the one cmdgen_train_backward forms on the same forward (up to the order of float atomics), and
    calling the new entry changes nothing cmdgen_train_backward computes afterwards."""
    cfg, sd, inp, g, gq = case(256, 3, 3, 77)
    dyn = make_module(cfg, sd)
    eps, gi, gp = hip_grads(dyn, inp, g, gq, False)
    h = dyn.hip_handle()
    from cmdgen_amd.autograd import flat_theta
    theta = flat_theta(h, dyn, list(dyn.parameters())).clone()
    xp, xq, t = dev(inp['xh_phar']), dev(inp['xh_pocket']), dev(inp['t'])
    h.train_forward(theta, xp, xq, t, want_pocket=True)
    grads = []
    for _ in range(2):
        gr = torch.zeros_like(theta)
        h.train_backward(dev(g), gr)
        grads.append(gr)
    h.train_backward_inputs(dev(g), None, None, torch.empty_like(xp), None, None)
    gr = torch.zeros_like(theta)
    h.train_backward(dev(g), gr)
    grads.append(gr)
    ref = grads[0].cpu().numpy()
    for name, v in gp.items():
        off, cnt = h.param_offset(name)
        for other in [npy(v).reshape(-1)] + [x.cpu().numpy()[off:off + cnt] for x in grads[1:]]:
            assert_close(other, ref[off:off + cnt], SAME_TOL, name)


def test_finite_differences_on_the_fp32_instruction():
    """Central differences of a float64-accumulated loss along random input directions (positions, features, t) agree with the analytic
    input gradient; the edge set is the same at both ends of every step."""
    cfg, sd, inp, g, gq = case(64, 2, 2, 55)
    dyn = make_module(cfg, sd)
    h = dyn.hip_handle()
    h.set_gemm_mode(False)
    _, gi, _ = hip_grads(dyn, inp, g, gq, False)
    dyn.set_differentiable(False)
    rng = np.random.Generator(np.random.PCG64(5))
    mp, mq = dev(inp['mask_phar']), dev(inp['mask_pocket'])
    gd = torch.from_numpy(g).double()

    def loss_and_edges(xp, xq, t):
        with torch.no_grad():
            e, _ = dyn(dev(xp), dev(xq), dev(t), mp, mq)
        return float((e.cpu().double() * gd).sum()), dyn.get_edges()

    step = 2e-3
    for k in range(4):
        v = {key: rng.normal(size=inp[key].shape).astype(np.float32) for key in ('xh_phar', 'xh_pocket', 't')}
        for key in ('xh_phar', 'xh_pocket'):
            v[key][:, :3] *= 0.05             # positions move by ~1e-4: inside the inputs' 2e-3 margin to the cutoff
        if k < 2:
            v['t'][:] = 0
        lp, ep = loss_and_edges(*(inp[key] + step * v[key] for key in ('xh_phar', 'xh_pocket', 't')))
        lm, em = loss_and_edges(*(inp[key] - step * v[key] for key in ('xh_phar', 'xh_pocket', 't')))
        assert torch.equal(ep, em), 'the step crossed the cutoff'
        fd = (lp - lm) / (2 * step)
        an = sum(float((gi[key].cpu().double() * torch.from_numpy(v[key]).double()).sum()) for key in ('xh_phar', 'xh_pocket', 't'))
        assert abs(fd - an) <= 2e-2 * max(abs(an), 5e-2), (k, fd, an)      # (floor: the fp32 loss's rounding / 2 step)


# ------------------------------------------------------------------ 3: two forwards, one backward
def test_two_forwards_one_backward_is_the_sum():
    cfg, sd, inp, g, gq = case(64, 2, 3, 61)
    dyn = make_module(cfg, sd).set_differentiable(True)
    mp, mq = dev(inp['mask_phar']), dev(inp['mask_pocket'])
    xp = dev(inp['xh_phar']).requires_grad_(True)
    xq = dev(inp['xh_pocket'])
    t1, t0 = dev(inp['t']), torch.zeros_like(dev(inp['t']))
    # the second call sees other inputs (another pocket layout would do as well): its forward overwrites the handle's activations
    xp2 = lambda: xp * 1.01
    singles = []
    for which in range(2):
        dyn.zero_grad()
        e = dyn(xp, xq, t1, mp, mq)[0] if which == 0 else dyn(xp2(), xq, t0, mp, mq)[0]
        (e * dev(g)).sum().backward(inputs=[xp] + list(dyn.parameters()))
        singles.append(({n: p.grad.clone() for n, p in dyn.named_parameters()}, xp.grad.clone()))
        xp.grad = None
    dyn.zero_grad()
    e1, _ = dyn(xp, xq, t1, mp, mq)
    e2, _ = dyn(xp2(), xq, t0, mp, mq)
    ((e1 * dev(g)).sum() + (e2 * dev(g)).sum()).backward(inputs=[xp] + list(dyn.parameters()))
    for n, p in dyn.named_parameters():
        assert_close(npy(p.grad), npy(singles[0][0][n] + singles[1][0][n]), 1e-5, n)
    assert_close(npy(xp.grad), npy(singles[0][1] + singles[1][1]), 1e-5, 'xh_phar')


# ------------------------------------------------------------------ 4: the reference's training idiom
@pytest.mark.parametrize('loss_type', ['l2', 'vlb'])
def test_reference_training_idiom_equals_the_trainer(loss_type):
    """nll, _ = model(data, t_int, eps); nll.mean().backward() with the switch on leaves the HipTrainer's flat gradient in the .grads."""
    model, tr, data, g6 = build_trainer()
    model.loss_type = loss_type
    t_int, eps = dev(g6['t_int']), [dev(g6['eps0'])]
    loss, nll, info = tr.loss_and_grad(data, t_int=t_int, eps=eps)
    want = tr.grad.clone()
    model.set_differentiable(True)
    model.train()
    model.zero_grad()
    d = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in data.items()}
    nll2, _ = model(d, t_int=t_int, eps=eps)
    assert nll2.grad_fn is not None
    assert float((nll2.detach() - nll).abs().max()) <= 2e-5 * max(1.0, float(nll.abs().max()))
    nll2.mean().backward()
    for name, p in model.ddpm.dynamics.named_parameters():
        off, cnt = tr.h.param_offset(name)
        w = want[off:off + cnt].view(p.shape)
        got = torch.zeros_like(w) if p.grad is None else p.grad
        assert_close(npy(got), npy(w), GRAD_TOL, name)
    # the eval-mode loss evaluates the network at t and at 0 before one backward (the first call's activations are overwritten by the
    # second): its gradient equals the sum of the two calls' gradients taken on separate handles - the first call through a copy of the
    # module (`_net`), whose handle nothing else touches
    import copy
    model.eval()
    dyn = model.ddpm.dynamics
    model.zero_grad()
    nll3, _ = model(d, t_int=t_int, eps=[dev(g6['eps0']), dev(g6['eps0'])])
    nll3.mean().backward()
    both = {n: p.grad.clone() for n, p in dyn.named_parameters()}
    keep, dyn._handle = dyn._handle, None
    dup = copy.deepcopy(dyn)
    dyn._handle = keep
    model.zero_grad(); dup.zero_grad()
    nll4, _ = model(d, t_int=t_int, eps=[dev(g6['eps0']), dev(g6['eps0'])], _net=dup)
    assert float((nll4 - nll3).detach().abs().max()) <= 2e-5 * max(1.0, float(nll3.detach().abs().max()))
    nll4.mean().backward()
    dup_grads = dict(dup.named_parameters())
    for n, p in dyn.named_parameters():
        assert dup_grads[n].grad is not None and p.grad is not None
        assert_close(npy(both[n]), npy(p.grad + dup_grads[n].grad), SAME_TOL, n)


# ------------------------------------------------------------------ 5: defaults unchanged
def test_switch_off_leaves_the_plain_evaluation():
    cfg, sd, inp, g, gq = case(64, 2, 2, 33)
    dyn = make_module(cfg, sd)
    args = [dev(inp[k]) for k in ('xh_phar', 'xh_pocket', 't', 'mask_phar', 'mask_pocket')]
    args[0].requires_grad_(True)
    a, aq = dyn(*args)
    assert a.grad_fn is None and aq.grad_fn is None and not a.requires_grad
    with torch.no_grad():
        b, bq = dyn(*args)
    # (the plain evaluation sums some receivers with float atomics: two runs of it agree up to the order of those sums)
    assert_close(npy(a), npy(b), SAME_TOL, 'eps'); assert_close(npy(aq), npy(bq), SAME_TOL, 'eps_pocket')
    dyn.set_differentiable(True)
    with torch.no_grad():
        c, _ = dyn(*args)
    assert c.grad_fn is None
    assert_close(npy(c), npy(b), SAME_TOL, 'eps')
    dyn.set_differentiable(False)
    d, _ = dyn(*args)
    assert d.grad_fn is None
    assert_close(npy(d), npy(b), SAME_TOL, 'eps')


# ------------------------------------------------------------------ 6: the half engine's range guard
def test_half_overflow_case_warns_and_equals_the_split_engine():
    from helpers import overflow_case
    cfg, sd, inp = overflow_case('msg')
    rng = np.random.Generator(np.random.PCG64(9))
    g = rng.normal(size=inp['xh_phar'].shape).astype(np.float32)
    res = []
    for split in (False, True):
        dyn = make_module(cfg, sd)
        if split:
            dyn.hip_handle().set_option('half_engine', 0)
            res.append(hip_grads(dyn, inp, g, None, False))
        else:
            with pytest.warns(RuntimeWarning, match='half matrix engine'):
                res.append(hip_grads(dyn, inp, g, None, False))
    (ea, ia, pa), (eb, ib, pb) = res
    assert torch.isfinite(ea).all()
    assert_close(npy(ea), npy(eb), SAME_TOL, 'eps')
    # (a model whose activations reach ~1e6 cancels in its sums: the atomic order shows at up to ~2e-5 of a tensor's scale here)
    for k in ('xh_phar', 'xh_pocket', 't'):
        assert_close(npy(ia[k]), npy(ib[k]), GRAD_TOL, k)
    for k in pa:
        assert_close(npy(pa[k]), npy(pb[k]), GRAD_TOL, k)
