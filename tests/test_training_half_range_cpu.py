"""HipTrainer's bookkeeping around the half matrix engine's range events (CPU, no GPU): a fake library handle stands in for the device side
of a training step - what include/cmdgen_hip.h promises for cmdgen_train_forward, cmdgen_train_range_event and cmdgen_adamw_step_clipped:
after a forward on the half engine, a range event (this process's own, or the value the caller's all-reduce left in the event slot) makes the
norm non-finite and the update is skipped.  The product code under test is HipTrainer's: the queue of recent norms, the step count AdamW's
bias correction uses, the switch to the bf16 engine, the repeated batch (waiting mode), the dropped batches (pipelined mode) and, over gloo,
one decision for all ranks."""
import math
import os
import sys
import warnings
from datetime import timedelta
from types import SimpleNamespace

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cmdgen_amd.training import HipTrainer  # noqa: E402

N = 64
LOW, RESET = 4096.0, 1.0                     # cmdgen_train_range_event's values
# stages of the fake backward pass -> the gradient range each one finishes (the chunks of grad_chunks() for n_layers = 2: [32, 64), [16, 32), [0, 16))
STAGES = {0: (32, 64), 1: (32, 32), 2: (16, 32), 3: (0, 16)}


def batch_grad(batch, rank=0):
    return torch.randn(N, generator=torch.Generator().manual_seed(100 * batch + rank)) * (1.0 + batch)


class FakeDevice:
    """The library's side of the step.  events(batch) -> the range event a forward of that batch has on the half engine."""

    def __init__(self, events, rank=0):
        self.events, self.rank, self.opts = events, rank, {}
        self.fwd_half, self.local_event, self.shared, self.pending, self.seen_event, self.batch = 0, 0.0, None, None, 0, None
        self.adamw_steps, self.applied = [], []

    def param_count(self):
        return N

    def param_offset(self, name):
        if name == 'w':
            return 0, N
        return 16 * (int(name.split('_')[2].split('.')[0]) + 1), 16            # 'egnn.e_block_<l>....': the chunk boundaries

    def get_option(self, key):
        return self.opts.get(key)

    def set_option(self, key, value):
        self.opts[key] = value

    def half_engine_active(self):
        return True

    def query(self, key):
        return {'train_half_ran': self.fwd_half, 'train_range_event': self.seen_event}[key]

    def forward(self, batch):                                          # cmdgen_train_forward
        self.fwd_half = int(self.opts.get('train_half', 1) != 0)
        self.local_event = float(self.events(batch)) if self.fwd_half else 0.0
        self.shared, self.batch = None, batch

    def train_range_event(self, out):
        out.fill_(self.local_event)
        self.shared = out

    def train_backward(self, d_eps, grad, d_eps_q=None):
        grad.copy_(batch_grad(self.batch, self.rank))

    def train_backward_stages(self, d_eps, grad, first, last, d_eps_q=None):
        g = batch_grad(self.batch, self.rank)
        for stage in range(first, last + 1):
            lo, hi = STAGES[stage]
            grad[lo:hi] = g[lo:hi]

    def adamw_step_clipped(self, theta, grad, m, v, vmax, step, lr, betas, eps, weight_decay, max_grad_norm, defer=False):
        norm = math.sqrt(float((grad.double() ** 2).sum()))
        ev = 0.0
        if self.fwd_half:                                              # k_norm_guard
            ev = float(self.shared[0]) if self.shared is not None else self.local_event
            if ev > 0:
                norm = float('nan')
        self.adamw_steps.append(int(step))
        if not (self.fwd_half and not math.isfinite(norm)):           # k_adamw
            clip = min(1.0, max_grad_norm / (norm + 1e-6)) if max_grad_norm > 0 else 1.0
            g = grad * clip
            theta.mul_(1.0 - lr * weight_decay)
            m.lerp_(g, 1.0 - betas[0])
            v.mul_(betas[1]).add_((1.0 - betas[1]) * g * g)
            torch.maximum(vmax, v, out=vmax)
            denom = vmax.sqrt() / math.sqrt(1.0 - betas[1] ** step) + eps
            theta.sub_((lr / (1.0 - betas[0] ** step)) * m / denom)
            self.applied.append((self.batch, int(step)))
        self.pending = (norm, ev)
        return None if defer else self.last_grad_norm()

    def last_grad_norm(self):
        norm, self.seen_event = self.pending
        self.pending = None
        return norm


class Dyn(torch.nn.Module):
    def __init__(self, handle):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(N))
        self._cfg = {'n_layers': 2}
        self._handle = handle

    def hip_handle(self):
        return self._handle


class StubTrainer(HipTrainer):
    """HipTrainer itself (constructor, _backward / _allreduce, optimizer_step, training_step) on the fake device; loss_and_grad runs the
    fake forward and the real _backward."""

    def __init__(self, events, rank=0, pipelined=False):
        dev = FakeDevice(events, rank)
        ddpm = SimpleNamespace(dynamics=Dyn(dev), learned_schedule=False)
        super().__init__(SimpleNamespace(mode='pocket_conditioning', loss_type='l2', ddpm=ddpm, lr=1e-3, clip_grad=True))
        self.pipelined = pipelined
        self.batches_run = []

    def loss_and_grad(self, data, t_int=None, eps=None):
        self.h.forward(data)
        self.grad.zero_()
        self._backward(None, None)
        self.batches_run.append(data)
        return torch.zeros(()), None, {}


def run_steps(tr, batches):
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter('always')
        for b in batches:
            tr.training_step(b)
        tr._collect_norm()
    return [str(x.message) for x in w if issubclass(x.category, RuntimeWarning)]


@pytest.mark.parametrize('kind', ['low', 'overflow'])
def test_waiting_step_skips_switches_and_repeats_the_batch(kind):
    tr = StubTrainer(lambda b: (LOW if kind == 'low' else RESET) if b == 0 else 0.0)
    msgs = run_steps(tr, [0, 1, 2])
    assert all(math.isfinite(x) for x in tr.gradnorm_queue.items), tr.gradnorm_queue.items
    assert tr.h.adamw_steps == [1, 1, 2, 3], tr.h.adamw_steps            # the skipped update, then the repeat with the same step
    assert tr.h.applied == [(0, 1), (1, 2), (2, 3)] and tr.step_count == 3
    assert tr.batches_run == [0, 0, 1, 2] and tr.h.get_option('train_half') == 0 and tr.half_range_fallbacks == 1
    assert len(msgs) == 1 and 'half matrix engine' in msgs[0] and 'repeated' in msgs[0]
    assert ('below the half matrix engine' in msgs[0]) == (kind == 'low') and ('65504' in msgs[0]) == (kind == 'overflow'), msgs
    assert len(tr.gradnorm_queue) == 1 + 3 and tr.dropped_steps == []


@pytest.mark.parametrize('kind', ['low', 'overflow'])
def test_pipelined_steps_drop_both_half_engine_batches_and_count_only_applied_updates(kind):
    """Every forward on the half engine has the event: b1 and b2 both ran there (b2 was queued before b1's norm came back), so both
    updates are skipped on the device and both batches are dropped; b3 and b4 run on the bf16 engine."""
    tr = StubTrainer(lambda b: LOW if kind == 'low' else RESET, pipelined=True)
    msgs = run_steps(tr, [0, 1, 2, 3])
    assert all(math.isfinite(x) for x in tr.gradnorm_queue.items), tr.gradnorm_queue.items
    assert tr.h.adamw_steps == [1, 1, 1, 2], tr.h.adamw_steps            # 1 + the updates applied before each
    assert tr.h.applied == [(2, 1), (3, 2)] and tr.step_count == 2
    assert tr.dropped_steps == [0, 1] and tr.half_range_fallbacks == 1 and tr.h.get_option('train_half') == 0
    assert len(tr.gradnorm_queue) == 1 + 2
    assert len(msgs) == 2 and all(('below the half matrix engine' in m) == (kind == 'low') for m in msgs), msgs
    # the state equals that of a waiting trainer on the bf16 engine fed only the applied batches
    ref = StubTrainer(lambda b: 0.0)
    ref.h.set_option('train_half', 0)
    assert run_steps(ref, [2, 3]) == []
    for name in ('theta', 'exp_avg', 'exp_avg_sq', 'max_exp_avg_sq'):
        assert torch.equal(getattr(tr, name), getattr(ref, name)), name
    assert tr.gradnorm_queue.items == ref.gradnorm_queue.items


def test_pipelined_step_after_a_clean_half_engine_forward_is_applied():
    """Only b1 has the event: b2's forward ran on the half engine too but cleanly - its update stands, and only b1 is dropped."""
    tr = StubTrainer(lambda b: LOW if b == 0 else 0.0, pipelined=True)
    run_steps(tr, [0, 1, 2])
    assert all(math.isfinite(x) for x in tr.gradnorm_queue.items)
    assert tr.h.adamw_steps == [1, 1, 2] and tr.h.applied == [(1, 1), (2, 2)] and tr.step_count == 2 and tr.dropped_steps == [0]


# ------------------------------------------------------------------ world size 2 over gloo: only rank 0 has the event
def _worker(rank, world, port, pipelined, q):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    dist.init_process_group('gloo', rank=rank, world_size=world, timeout=timedelta(seconds=30))
    torch.set_num_threads(1)
    sizes = []
    real = dist.all_reduce

    def recording(t, *a, **k):
        sizes.append(t.numel())
        return real(t, *a, **k)
    dist.all_reduce = recording
    try:
        tr = StubTrainer(lambda b: LOW if (rank == 0 and b == 0) else 0.0, rank=rank, pipelined=pipelined)
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            for b in (0, 1, 2):
                tr.training_step(b)
            tr._collect_norm()
        q.put((rank, tr.theta.clone(), tr.batches_run, sizes, tr.h.adamw_steps, tr.h.applied, tr.step_count, tr.dropped_steps,
               tr.h.get_option('train_half'), list(tr.gradnorm_queue.items)))
    finally:
        dist.all_reduce = real
    dist.destroy_process_group()


@pytest.mark.parametrize('pipelined', [False, True])
def test_two_ranks_skip_switch_and_repeat_together(pipelined):
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = 29850 + os.getpid() % 100 + (50 if pipelined else 0)
    procs = [ctx.Process(target=_worker, args=(r, 2, port, pipelined, q)) for r in range(2)]
    for p in procs:
        p.start()
    try:
        res = dict((r[0], r[1:]) for r in (q.get(timeout=120), q.get(timeout=120)))
        for p in procs:
            p.join(timeout=60)
            assert p.exitcode == 0
    finally:
        for p in procs:
            if p.is_alive():
                p.terminate()
    (th0, run0, sz0, st0, ap0, sc0, dr0, half0, q0), (th1, run1, sz1, st1, ap1, sc1, dr1, half1, q1) = res[0], res[1]
    assert run0 == run1 and sz0 == sz1, (run0, run1, sz0, sz1)          # the same batches, the same collectives
    assert st0 == st1 and ap0 == ap1 and sc0 == sc1 and dr0 == dr1 and half0 == half1 == 0
    if pipelined:           # b0 is dropped on both ranks (rank 1 had no event of its own); b1's forward was clean on the half engine
        assert run0 == [0, 1, 2] and st0 == [1, 1, 2] and [b for b, _ in ap0] == [1, 2] and dr0 == [0]
    else:                   # b0 is repeated on both ranks
        assert run0 == [0, 0, 1, 2] and st0 == [1, 1, 2, 3] and [b for b, _ in ap0] == [0, 1, 2] and dr0 == []
    assert sc0 == len(ap0)
    assert torch.equal(th0, th1) and q0 == q1 and all(math.isfinite(x) for x in q0)
