"""Autograd through the HIP denoiser: EGNNDynamics.forward as a torch.autograd.Function (opt-in).

``EGNNDynamics.set_differentiable(True)`` routes the module's forward, in grad mode, through ``DynamicsFunction``:

* forward: the activation-saving training forward of the library (``cmdgen_train_forward``) on a flat parameter buffer ``theta`` in
  ``cmdgen_param_offset`` order - zero-copy when the parameters already are views of one such buffer (``training.HipTrainer``), else
  gathered;
* backward: ``cmdgen_train_backward_inputs`` - gradients to xh_phar, xh_pocket, t and every parameter (as views of one flat gradient),
  so autograd accumulates them into ``.grad`` and DDP's hooks fire as for any module.

The radius graph is a constant of the pass (the reference's ``get_edges`` carries no gradient either).  The handle keeps the saved
activations and the graph of ONE evaluation: a backward after anything else evaluated on the handle or changed its layout since this
call's forward (the eval-mode loss evaluates the network at t and at 0 before one backward; a plain no_grad call; a sampling chain) re-runs
its own forward first - the library's evaluation counter (cmdgen_query "eval_gen") tells.  Once differentiable: no double backward.
"""
from __future__ import annotations

import numpy as np
import torch
from torch.autograd.function import once_differentiable


def _param_offsets(h, module):
    """[(offset, count)] of module.parameters() inside the flat buffer (cached on the handle: the table depends on its dims only)."""
    cache = getattr(h, '_ad_offsets', None)
    names = tuple(n for n, _ in module.named_parameters())
    if cache is None or cache[0] != names:
        cache = (names, [h.param_offset(n) for n in names])
        h._ad_offsets = cache
    return cache[1]


def flat_theta(h, module, params):
    """The flat parameter buffer of this call: a zero-copy view when every parameter sits at its offset of one storage of
    param_count() floats (HipTrainer's layout), else a gathered copy."""
    n = h.param_count()
    offs = _param_offsets(h, module)
    p0 = params[0]
    st = p0.untyped_storage()
    if (p0.is_cuda and p0.dtype == torch.float32 and st.nbytes() == 4 * n and
            all(p.untyped_storage().data_ptr() == st.data_ptr() and p.storage_offset() == off and p.is_contiguous()
                for p, (off, _) in zip(params, offs))):
        return torch.as_strided(p0.detach(), (n,), (1,), 0)
    theta = torch.zeros(n, dtype=torch.float32, device=p0.device)
    for p, (off, cnt) in zip(params, offs):
        theta[off:off + cnt] = p.detach().reshape(-1).to(torch.float32)
    return theta


class DynamicsFunction(torch.autograd.Function):
    """(module, xh_phar, xh_pocket, t, *module.parameters()) -> (eps_phar, eps_pocket).  The caller has set the handle's layout."""

    @staticmethod
    def forward(ctx, module, xh_phar, xh_pocket, t, *params):
        h = module.hip_handle(upload=False)
        theta = flat_theta(h, module, params)
        xp = xh_phar.detach().to(torch.float32).contiguous()
        xq = xh_pocket.detach().to(torch.float32).contiguous()
        tt = t.detach().reshape(-1).to(torch.float32)
        if tt.numel() == 1 and h.batch > 1:
            tt = tt.expand(h.batch)
        tt = tt.contiguous()
        ctx.h, ctx.module = h, module
        ctx.layout = (np.frombuffer(h._layout_key[0], dtype=np.int64).copy(), np.frombuffer(h._layout_key[1], dtype=np.int64).copy())
        ctx.keep = (theta, xp, xq, tt)          # the library reads these device pointers again in the backward pass
        ctx.t_shape = tuple(t.shape)
        ctx.fallback = False
        (eps, eps_q), st = DynamicsFunction._run(ctx, guarded=True)
        ctx.fallback = bool(st.get('half_engine_fallback', False))
        return eps, eps_q

    @staticmethod
    def _run(ctx, guarded):
        """The training forward of this call; guarded: a half-engine run that reset or saw a low-range row repeats on the bf16 split
        engine (Handle.run_range_guarded, with its warning); a re-run repeats on the engine the first run ended on."""
        h = ctx.h
        theta, xp, xq, tt = ctx.keep
        run = lambda: h.train_forward(theta, xp, xq, tt, want_pocket=True)
        if guarded:
            out, st = h.run_range_guarded(run, dict) if h.half_engine_active() else (run(), {})
        else:
            prev = h.get_option('half_engine') if ctx.fallback else None
            if ctx.fallback:
                h.set_option('half_engine', 0)
            try:
                out, st = run(), {}
            finally:
                if ctx.fallback:
                    h.set_option('half_engine', prev)
        ctx.gen = h.query('eval_gen')            # the handle's evaluation counter right after this call's forward
        return out, st

    @staticmethod
    @once_differentiable
    def backward(ctx, g_eps, g_eps_q):
        h = ctx.h
        h.set_layout(*ctx.layout)
        if h.query('eval_gen') != ctx.gen:       # another evaluation or layout since this forward: re-make this call's graph and activations
            DynamicsFunction._run(ctx, guarded=False)
        theta, xp, xq, tt = ctx.keep
        want_x, want_q, want_t = ctx.needs_input_grad[1], ctx.needs_input_grad[2], ctx.needs_input_grad[3]
        want_t = want_t and bool(h.cfg.get('condition_time', True))
        d_xp = torch.empty_like(xp) if want_x else None
        d_xq = torch.empty_like(xq) if want_q else None
        d_t = torch.empty_like(tt) if want_t else None
        params = list(ctx.module.parameters())
        want_w = any(ctx.needs_input_grad[4:])
        grad = torch.zeros_like(theta) if want_w else None
        g = torch.zeros_like(xp) if g_eps is None else g_eps.detach().to(torch.float32).contiguous()
        gq = None if g_eps_q is None else g_eps_q.detach().to(torch.float32).contiguous()
        h.train_backward_inputs(g, grad, gq, d_xp, d_xq, d_t)
        if d_t is not None:
            d_t = d_t.sum().reshape(ctx.t_shape) if int(np.prod(ctx.t_shape)) == 1 else d_t.reshape(ctx.t_shape)
        pg = [None] * len(params)
        if grad is not None:
            pg = [grad[off:off + cnt].view(p.shape) for p, (off, cnt) in zip(params, _param_offsets(h, ctx.module))]
        return (None, d_xp, d_xq, d_t, *pg)


def dynamics_apply(module, xh_phar, xh_pocket, t):
    """EGNNDynamics.forward in differentiable mode (layout already set on the module's handle)."""
    return DynamicsFunction.apply(module, xh_phar, xh_pocket, t, *module.parameters())
