"""ConditionalDDPM.inpaint on the CPU: the oracle-built model of the conditional RePaint loop (cond_inpaint_ref) against the
G20 vectors composed from the reference's own methods (tests/golden/make_golden_cond_inpaint.py), its reduction to the
plain sampler, the draw plan, and the argument checks that need no device."""
import numpy as np
import pytest
import torch

from helpers import (NoiseTape, bare_inputs as _inputs, bare_model as _model, cases_of, g20, g20_oracle_case as g20_case,
                     pocket_dict as pocket_of)
from cond_inpaint_ref import cond_inpaint, inpaint_plan
from oracle import ref_cpu
from cmdgen_amd.synthetic import make_pockets

G20 = g20()


def test_g20_covers_the_specified_cases():
    names = cases_of(G20)
    plans = {tuple(int(v) for v in G20[n + '/meta'][6:8]) for n in names}
    assert {(1, 1), (2, 1), (3, 2)} <= plans
    assert {int(G20[n + '/meta'][0]) for n in names} >= {64, 256}
    for n in names:
        fixed, B = G20[n + '/phar_fixed'], int(G20[n + '/meta'][2])
        pm = np.repeat(np.arange(B), make_pockets(B, 'CA', ragged=True, n_phar=7, first_index=int(G20[n + '/meta'][8])).num_nodes_phar)
        per = [fixed[pm == b] for b in range(B)]
        assert 0 < per[0].sum() < len(per[0]) and per[1].sum() == 0 and per[2].all()       # some, none, all fixed
        assert float(G20[n + '/margins'].min()) > 2e-3


@pytest.mark.parametrize('name', cases_of(G20))
def test_oracle_model_reproduces_g20(name):
    cfg, p, pb, phar, fixed, (K, r, j) = g20_case(name)
    tape = NoiseTape(G20[name + '/noise'])
    with torch.no_grad():
        xh_phar, xh_pocket, pm, _, z_steps, p_steps = cond_inpaint(p, cfg.as_dict(), phar, pocket_of(pb), fixed, r, j, K,
                                                                   noise=tape, return_steps=True)
    assert tape.i == len(G20[name + '/noise']) == inpaint_plan(r, j, K)[1]
    want = G20[name + '/xh_phar']
    scale = max(1.0, float(np.abs(want[:, :3]).max()))
    assert float(np.abs(xh_phar[:, :3].numpy() - want[:, :3]).max()) <= 1e-5 * scale
    assert np.array_equal(xh_phar[:, 3:].numpy(), want[:, 3:])
    wq = G20[name + '/xh_pocket']
    assert float(np.abs(xh_pocket.numpy() - wq).max()) <= 1e-5 * max(1.0, float(np.abs(wq).max()))
    zs, ps = G20[name + '/z_steps'], G20[name + '/pocket_steps']
    assert z_steps.shape == zs.shape and p_steps.shape == ps.shape
    assert float(np.abs(z_steps.numpy() - zs).max()) <= 1e-5 * max(1.0, float(np.abs(zs).max()))
    assert float(np.abs(p_steps.numpy() - ps).max()) <= 1e-5 * max(1.0, float(np.abs(ps).max()))


def test_fixed_rows_of_g20_stay_near_the_given_points():
    """The property inpainting exists for: relative to the pocket, a fixed row ends where it was given (and keeps its type)."""
    for name in cases_of(G20):
        _, _, pb, phar, fixed, _ = g20_case(name)
        f = fixed != 0
        pm = phar['mask'].numpy()
        out, outq = G20[name + '/xh_phar'], G20[name + '/xh_pocket']
        B = len(pb.size)
        shift = np.stack([pb.x[pb.mask == b].mean(0) - outq[pb.mask == b, :3].mean(0) for b in range(B)])
        back = out[:, :3] + shift[pm]
        assert np.abs(back[f] - phar['x'].numpy()[f]).max() < 0.1
        assert np.array_equal(out[f, 3:], phar['one_hot'].numpy()[f])


def test_without_fixed_rows_equals_the_plain_sampler_bit_for_bit():
    name = 'h64_K12_r1j1'
    cfg, p, pb, phar, fixed, (K, _, _) = g20_case(name)
    noise = G20[name + '/noise']
    with torch.no_grad():
        a = cond_inpaint(p, cfg.as_dict(), phar, pocket_of(pb), np.zeros_like(fixed), 1, 1, K, noise=NoiseTape(noise))
        plain = np.concatenate([noise[:1], noise[1:1 + 2 * K:2], noise[-1:]])       # draw 0, the A draws, the decode draw
        b = ref_cpu.sample_given_pocket(p, cfg.as_dict(), pocket_of(pb), pb.num_nodes_phar, timesteps=K, noise=NoiseTape(plain))
    for u, v in zip(a, b):
        assert torch.equal(u, v)


@pytest.mark.parametrize('K', [1, 2, 7, 50, 500])
@pytest.mark.parametrize('r,j', [(1, 1), (2, 1), (3, 2), (10, 10), (4, 3), (2, 20)])
def test_plan_counts(K, r, j):
    n_steps, n_draws, n_jumps = inpaint_plan(r, j, K)
    sched = ref_cpu.get_repaint_schedule(r, j, K)
    assert n_steps == sum(sched) and n_jumps == len(sched) - 1
    assert n_draws == 2 + 2 * n_steps + n_jumps
    if r == 1:
        assert n_steps == K                              # no resampling: every step once
    # ops = K steps down plus jump_length steps again for every jump back
    assert n_steps == K + n_jumps * j


def test_argument_checks_without_a_device():
    from cmdgen_amd.equivariant_diffusion.conditional_model import ConditionalDDPM, SimpleConditionalDDPM
    phar, pocket = _inputs()
    m = _model(ConditionalDDPM)
    with pytest.raises(ValueError, match='jump_length'):
        m.inpaint(phar, pocket, torch.ones(5), jump_length=2, return_frames=2, timesteps=10)
    with pytest.raises(ValueError, match='phar_fixed'):
        m.inpaint(phar, pocket, torch.ones(4), timesteps=10)
    with pytest.raises(ValueError, match='phar_fixed'):
        m.inpaint(phar, pocket, torch.ones(5, 2), timesteps=10)
    with pytest.raises(NotImplementedError, match='SimpleConditionalDDPM'):
        _model(SimpleConditionalDDPM).inpaint(phar, pocket, torch.ones(5), timesteps=10)


def test_inpaint_entries_are_bound():
    from cmdgen_amd import hip_backend
    lib = hip_backend.load_library()
    assert lib.cmdgen_inpaint_chain.argtypes is not None and lib.cmdgen_inpaint_plan.argtypes is not None
    assert hasattr(hip_backend.Handle, 'inpaint_chain') and hasattr(hip_backend.Handle, 'inpaint_plan')
