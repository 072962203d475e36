"""The TRAINING step at both ends of the half matrix engine's range.  The training forward runs the sampler's half-engine tiles in their
save-hook forms (the full-K 32-row edge and coordinate tiles, k_node16w: cmdgen_train.hip, fwd_half / node_half) - the default at
hidden_nf = 256.  The weight edits are test_hip_half_range.py's: overflow_case (first layer x 3e6: an activation beyond fp16's 65504) and
underflow_case (first layer x s, second layer x 1 / s: the half GEMM's A operand at scale s, below HALF_LOW_TAU = 2^-5).

  * the raw step (train_forward + train_backward with train_half on) reaches the low-range defect: rows are counted, and the loss or a
    gradient misses oracle autograd by more than GRAD_TOL at the scale recorded in TRAIN_SMALLEST;
  * the guarded waiting step warns about the low range, repeats the batch on the bf16 split engine and equals oracle autograd;
  * pipelined steps on an overflowing / low-range model drop exactly the batches whose forwards ran on the half engine and keep the
    queue, the step count and the optimizer state of a trainer that saw only the applied batches;
  * autograd through EGNNDynamics on a low-range model warns and equals oracle autograd;
  * the benchmark's random-init model at 64 complexes trains without a single low-range row.
The oracle is autograd through oracle/ref_cpu.py in fp32 (its training loss is written for fp32 tensors)."""
import warnings

import numpy as np
import pytest
import torch

from oracle import ref_cpu
from helpers import GRAD_TOL, RANGE_TARGETS as TARGETS, _bench_trainer, underflow_case

pytestmark = pytest.mark.gpu

B = 8
LOW_SCALES = [2.0 ** -6, 2.0 ** -10]
# the largest scale per target (of 2^-14, -18, -22, -26) at which the RAW half-engine training step misses oracle autograd by more than
# GRAD_TOL (loss or a gradient tensor at its own scale).  The weight gradients read the saved fp32 activations, so only the forward's output
# error reaches them, through dL/d eps.  Measured on an MI355X (8 complexes, batch 9100): worst gradient error at s = 2^-14 / -18 / -22 / -26
#   msg   5.9e-5 / 4.5e-3 / 9.0e-2 / 3.3e-1  (att_mlp.0 of the targeted GCL)     loss error <= 1.5e-6 throughout
#   coord 4.9e-5 / 9.8e-4 / 4.5e-2 / 9.8e-1  (coord_mlp.4)
#   node  6.1e-4 / 1.1e-2 / 1.2e-1 / 1.2e-1  (node_mlp.2 of the following blocks)
TRAIN_SMALLEST = {'msg': 2.0 ** -18, 'coord': 2.0 ** -18, 'node': 2.0 ** -14}


def scaled(target, s):
    """sd_edit for _bench_trainer: underflow_case's edit of the benchmark model (s < 1) or overflow_case's (s = None)."""
    first = TARGETS[target]
    second = first[:-len('.0')] + '.2.weight'

    def edit(sd):
        if s is None:
            for suf in ('.weight', '.bias'):
                sd[first + suf] = (sd[first + suf] * np.float32(3.0e6)).astype(np.float32)
            return sd
        for key in (first + '.weight', first + '.bias'):
            sd[key] = (sd[key] * np.float32(s)).astype(np.float32)
        sd[second] = (sd[second] * np.float32(1.0 / s)).astype(np.float32)
        return sd
    return edit


def draws(bt, first, seed=3):
    batch = bt.synthetic_batch(B, first, torch.device('cuda', 0))
    gen = torch.Generator().manual_seed(seed)
    t_int = torch.randint(1, 501, (B, 1), generator=gen).float()
    eps0 = torch.randn((int(batch['num_phar_atoms'].sum()), 11), generator=gen)
    return batch, t_int, eps0


def oracle_step(cfg, sd, batch, t_int, eps0):
    """-> (loss, {param name: gradient}) of oracle autograd on the batch, draws and time steps."""
    cpu = lambda k: batch[k].detach().cpu()
    phar = {'x': cpu('phar_coords'), 'one_hot': cpu('phar_one_hot'), 'size': cpu('num_phar_atoms'), 'mask': cpu('phar_mask')}
    pocket = {'x': cpu('pocket_c_alpha'), 'one_hot': cpu('pocket_one_hot'), 'size': cpu('num_pocket_nodes'), 'mask': cpu('pocket_mask')}
    p = ref_cpu.to_torch_params(sd)
    leaves = {k: v.clone().requires_grad_(True) for k, v in p.items() if k.startswith('dynamics.')}
    p2 = dict(p); p2.update(leaves)
    terms = ref_cpu.ddpm_forward(p2, cfg.as_dict(), phar, pocket, t_int, [eps0], training=True, histogram=np.ones((30, 500)))
    nll = ref_cpu.nll_from_terms(terms, cfg.as_dict(), phar['size'], pocket['size'], training=True)
    loss = nll.mean(0)
    loss.backward()
    return float(loss), {k[len('dynamics.'):]: (torch.zeros_like(v) if v.grad is None else v.grad).numpy().reshape(-1) for k, v in leaves.items()}


def low_rows_so_far(tr, batch):
    """The handle's low-range counter once the batch's layout is set (a layout that outgrows the workspace starts the counters afresh)."""
    tr.h.set_layout(batch['num_phar_atoms'].cpu().numpy().astype(np.int64), batch['num_pocket_nodes'].cpu().numpy().astype(np.int64),
                    on_stream=tr.pipelined)
    return tr.h.counters()['half_low_range']


def misses(tr, loss, want_loss, want):
    """-> (relative loss error, worst gradient tensor's error at its own scale, its name)"""
    grad = tr.grad.cpu().numpy()
    worst = (0.0, None)
    for name, g_want in want.items():
        off, cnt = tr.h.param_offset(name)
        rel = float(np.abs(grad[off:off + cnt] - g_want).max()) / max(float(np.abs(g_want).max()), 1e-6)
        worst = max(worst, (rel, name))
    return abs(float(loss) - want_loss) / max(1.0, abs(want_loss)), worst[0], worst[1]


@pytest.mark.parametrize('target', list(TARGETS))
def test_raw_half_engine_step_reaches_the_low_range_defect(target):
    """train_forward + train_backward with train_half on (no guard involved): at TRAIN_SMALLEST[target] the targeted kernel ran on the half
    engine, counted low-range rows, and the loss or a gradient misses oracle autograd by more than GRAD_TOL."""
    report = []
    for s in sorted({2.0 ** -14, 2.0 ** -18, TRAIN_SMALLEST[target]}, reverse=True):
        cfg, sd, model, tr, bt = _bench_trainer(B, sd_edit=scaled(target, s))
        batch, t_int, eps0 = draws(bt, 9100)
        c0 = low_rows_so_far(tr, batch)
        loss, _nll, _info = tr.loss_and_grad(batch, t_int=t_int.cuda(), eps=[eps0.cuda()])
        torch.cuda.synchronize()
        moved = tr.h.counters()['half_low_range'] - c0
        assert tr.h.query('train_half_ran') == 1
        assert tr.h.query({'msg': 'msg_mfmas_per_product', 'coord': 'coord_mfmas_per_product', 'node': 'node_mfmas_per_product'}[target]) == 3
        want_loss, want = oracle_step(cfg, sd, batch, t_int, eps0)
        err_loss, err_grad, name = misses(tr, loss, want_loss, want)
        report.append(f's=2^{int(np.log2(s))}: rows {moved}, loss {err_loss:.1e}, worst gradient {err_grad:.1e} ({name})')
        assert moved >= 1, 'the rows below the half engine\'s range must be counted'
        if s == TRAIN_SMALLEST[target]:
            assert max(err_loss, err_grad) > GRAD_TOL, f'the raw step should miss the oracle at s = {s}: ' + '; '.join(report)
    print(f'{target}: ' + '; '.join(report))


@pytest.mark.parametrize('target', list(TARGETS))
def test_guarded_waiting_step_repeats_on_the_bf16_engine_and_equals_the_oracle(target):
    for s in LOW_SCALES + [TRAIN_SMALLEST[target]]:
        res = {}
        for th in (None, 0):
            cfg, sd, model, tr, bt = _bench_trainer(B, sd_edit=scaled(target, s))
            if th is not None:
                tr.h.set_option('train_half', th)
            batch, t_int, eps0 = draws(bt, 9100)
            if th is None:
                with warnings.catch_warnings(record=True) as w:
                    warnings.simplefilter('always')
                    info = tr.training_step(batch, t_int=t_int.cuda(), eps=[eps0.cuda()])
                msgs = [str(x.message) for x in w if issubclass(x.category, RuntimeWarning)]
                assert len(msgs) == 1 and 'below the half matrix engine' in msgs[0] and '65504' not in msgs[0], (s, msgs)
                assert tr.h.get_option('train_half') == 0 and tr.half_range_fallbacks == 1
                want_loss, want = oracle_step(cfg, sd, batch, t_int, eps0)
                err_loss, err_grad, name = misses(tr, info['loss'], want_loss, want)
                assert err_loss <= GRAD_TOL and err_grad <= GRAD_TOL, (s, err_loss, err_grad, name)
            else:
                info = tr.training_step(batch, t_int=t_int.cuda(), eps=[eps0.cuda()])
            assert tr.step_count == 1 and np.isfinite(tr.last_grad_norm) and bool(torch.isfinite(tr.theta).all())
            res[th] = (float(info['loss']), tr.theta.cpu().numpy().copy(), float(tr.last_grad_norm))
        assert abs(res[None][0] - res[0][0]) <= 1e-6 * max(1.0, abs(res[0][0]))
        assert abs(res[None][2] - res[0][2]) <= 1e-4 * res[0][2]
        d = np.abs(res[None][1] - res[0][1])
        assert d.max() <= 2.1e-3 and np.mean(d > 1e-6) < 1e-3, (s, float(d.max()), float(np.mean(d > 1e-6)))


@pytest.mark.parametrize('kind', ['overflow', 'low'])
def test_pipelined_steps_drop_the_half_engine_batches_and_keep_the_optimizer_state(kind):
    """Four pipelined steps on b1..b4 of a model that hits the event on the half engine: b1 and b2 (both forwards ran there) are dropped,
    every norm handed out and queued is finite, step_count counts the two applied updates, and after the last collect the parameters,
    moments and queue equal those of a waiting train_half = 0 trainer fed b3 and b4 only."""
    edit = scaled('msg', None if kind == 'overflow' else 2.0 ** -10)
    _cfg, _sd, _m, tr, bt = _bench_trainer(B, pipelined=True, sd_edit=edit)
    steps = [draws(bt, 9100 + 10 * i, seed=i) for i in range(4)]
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter('always')
        for batch, t_int, eps0 in steps:
            info = tr.training_step(batch, t_int=t_int.cuda(), eps=[eps0.cuda()])
            assert info['grad_norm'] is None
            assert np.isfinite(1.5 * tr.gradnorm_queue.mean() + 2 * tr.gradnorm_queue.std()), 'the clipping bound of the next step'
        tr._collect_norm()
    torch.cuda.synchronize()
    msgs = [str(x.message) for x in w if issubclass(x.category, RuntimeWarning)]
    # (the overflowing model counts low rows too - SiLU of a pre-activation near -1e5 is 0 - so only the low model's text is pinned)
    assert len(msgs) == 2 and all('half matrix engine' in m and (kind != 'low' or 'below the half matrix engine' in m) for m in msgs), msgs
    assert tr.dropped_steps == [0, 1] and tr.step_count == 2 and tr.h.get_option('train_half') == 0
    assert all(np.isfinite(x) for x in tr.gradnorm_queue.items) and len(tr.gradnorm_queue) == 3, tr.gradnorm_queue.items
    _c, _s, _m2, ref, _bt = _bench_trainer(B, pipelined=False, sd_edit=edit)
    ref.h.set_option('train_half', 0)
    for batch, t_int, eps0 in steps[2:]:
        ref.training_step(batch, t_int=t_int.cuda(), eps=[eps0.cuda()])
    assert ref.step_count == 2
    assert np.allclose(tr.gradnorm_queue.items, ref.gradnorm_queue.items, rtol=1e-4), (tr.gradnorm_queue.items, ref.gradnorm_queue.items)
    # (as test_pipelined_steps_equal_waiting_steps: Adam moves an element whose gradient is round-off noise by up to lr per step either way)
    d = (tr.theta - ref.theta).abs()
    assert float(d.max()) <= 2 * 2.1e-3 and float(d.mean()) <= 2e-6, (float(d.max()), float(d.mean()))
    for name in ('exp_avg', 'exp_avg_sq', 'max_exp_avg_sq'):
        a, b = getattr(tr, name), getattr(ref, name)
        assert float((a - b).abs().max()) <= 1e-3 * float(b.abs().max()), name


@pytest.mark.parametrize('target', list(TARGETS))
def test_differentiable_dynamics_on_a_low_range_model_warns_and_equals_oracle_autograd(target):
    from helpers import make_module, check_against_oracle
    cfg, sd, inp = underflow_case(target, 2.0 ** -10)
    g = np.random.Generator(np.random.PCG64(9)).normal(size=inp['xh_phar'].shape).astype(np.float32)
    dyn = make_module(cfg, sd)
    with pytest.warns(RuntimeWarning, match='precision range'):
        check_against_oracle(cfg, sd, inp, g, None, False, dyn=dyn)


@pytest.mark.parametrize('pipelined', [False, True])
def test_random_init_bench_trainer_stays_inside_the_range(pipelined):
    """No false positives at the benchmark's size: 64 complexes, the random-init model, a few steps - no low-range row, no fallback."""
    _cfg, _sd, _m, tr, bt = _bench_trainer(64, pipelined=pipelined)
    batch = bt.synthetic_batch(64, 7000, torch.device('cuda', 0))          # (one layout: the counters stay comparable; new draws every step)
    low0 = low_rows_so_far(tr, batch)
    resets0 = tr.h.counters()['nan_resets']
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        for i in range(4):
            tr.training_step(batch)
            assert tr.h.query('train_half_ran') == 1
        tr._collect_norm()
    c1 = tr.h.counters()
    print(f'pipelined={pipelined}: low-range rows {c1["half_low_range"] - low0}, resets {c1["nan_resets"] - resets0}, last norm {tr.last_grad_norm:.3f}')
    assert c1['half_low_range'] - low0 == 0 and c1['nan_resets'] - resets0 == 0 and tr.h.query('train_range_event') == 0
    assert tr.half_range_fallbacks == 0 and tr.dropped_steps == [] and tr.h.get_option('train_half') is None and tr.step_count == 4
