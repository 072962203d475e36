"""The multi-pocket chain on the CPU: the oracle-built model (multi_pocket_ref) against ref_cpu.sample_given_pocket where the two must
coincide, the frame (every pocket of a group carries the same translation), the leave-out cap of the GPU cases, and the argument
checks of ConditionalDDPM.sample_given_pockets that need no device."""
import numpy as np
import pytest
import torch

import multi_pocket_cases as mc
import multi_pocket_ref as mp
from helpers import NoiseTape, small, sub_pockets
from oracle import ref_cpu
from cmdgen_amd.synthetic import make_pockets

K = 6


def single_chain(cfg, p, pocket, nph, noise):
    with torch.no_grad():
        out = ref_cpu.sample_given_pocket(p, cfg.as_dict(), pocket, nph, timesteps=K, noise=NoiseTape(noise), return_chain=True)
    return out[0], out[1], torch.stack(out[4][1:])


def multi_chain(cfg, p, pocket, sizes, nph, w, noise):
    with torch.no_grad():
        out = mp.multi_pocket_chain(p, cfg.as_dict(), pocket, sizes, nph, w, timesteps=K, noise=NoiseTape(noise), return_steps=True)
    return out[0], out[1], out[4], out[5]


def test_groups_of_one_are_the_single_chain_exactly():
    cfg, p = small()
    pb = make_pockets(4, 'CA', ragged=True, first_index=9400)
    nph = np.minimum(pb.num_nodes_phar, 8)
    noise = np.random.default_rng(1).normal(size=(K + 2, int(nph.sum()), 11)).astype(np.float32)
    pocket = sub_pockets(pb, range(4))
    want, want_p, chain = single_chain(cfg, p, pocket, nph, noise)
    got, got_p, z_steps, _ = multi_chain(cfg, p, pocket, [1, 1, 1, 1], nph, np.ones(4, np.float32), noise)
    assert torch.equal(z_steps, chain)                       # every step
    assert torch.equal(got, want) and torch.equal(got_p, want_p)


def test_weights_one_zero_are_the_single_chain_on_the_first_pocket_exactly():
    cfg, p = small()
    pb = make_pockets(2, 'CA', ragged=True, first_index=9410)
    noise = np.random.default_rng(2).normal(size=(K + 2, 7, 11)).astype(np.float32)
    want, want_p, chain = single_chain(cfg, p, sub_pockets(pb, [0]), np.array([7]), noise)
    got, got_p, z_steps, _ = multi_chain(cfg, p, sub_pockets(pb, [0, 1]), [2], [7], np.array([1.0, 0.0], np.float32), noise)
    assert torch.equal(z_steps, chain)
    assert torch.equal(got, want) and torch.equal(got_p[:pb.size[0]], want_p)


def test_two_copies_of_one_pocket_with_equal_weights_stay_within_the_chain_bound():
    """0.5 eps + 0.5 eps of two equal contexts: the bounds of the chain tests (per-step z <= 1e-4 max(1, |z|), final x RMS <= 1e-4
    max(1, |x|), types exact) against the single chain."""
    cfg, p = small()
    pb = make_pockets(1, 'CA', ragged=True, first_index=9420)
    noise = np.random.default_rng(3).normal(size=(K + 2, 5, 11)).astype(np.float32)
    want, want_p, chain = single_chain(cfg, p, sub_pockets(pb, [0]), np.array([5]), noise)
    got, got_p, z_steps, _ = multi_chain(cfg, p, sub_pockets(pb, [0, 0]), [2], [5], np.array([0.5, 0.5], np.float32), noise)
    for k in range(K):
        assert float((z_steps[k] - chain[k]).abs().max()) <= 1e-4 * max(1.0, float(chain[k].abs().max())), k
    x, wx = got[:, :3].double(), want[:, :3].double()
    assert float(((x - wx) ** 2).mean().sqrt()) <= 1e-4 * max(1.0, float(wx.abs().max()))
    assert torch.equal(got[:, 3:], want[:, 3:])
    n = int(pb.size[0])
    assert torch.equal(got_p[:n], got_p[n:])                 # the two copies of the pocket moved alike


@pytest.mark.parametrize('case', list(mc.CASES.values()), ids=lambda c: c.name)
def test_every_pocket_of_a_group_carries_the_same_translation_and_the_cap_holds(case):
    """A reference chain translates every member pocket of a group by the same total vector (within 1e-5 normalised units: each
    pocket's rows round on their own), and the GPU cases' leave-out rule keeps at least 80 % of the groups."""
    r = mc.reference(case)
    pb, gr = r['pb'], r['groups']
    nv = mc.config().norm_values
    move = (r['want_pocket'][:, :3].astype(np.float64) - pb.x.astype(np.float64)) / nv[0]
    per_member = np.stack([move[pb.mask == b].mean(axis=0) for b in range(gr.B)])
    spread = max(float(np.abs(per_member[f:f + m] - per_member[f]).max()) for f, m in zip(gr.first, gr.sizes))
    step_move = (r['pocket_steps'][-1].astype(np.float64) - pb.x.astype(np.float64) / nv[0])
    per_member_k = np.stack([step_move[pb.mask == b].mean(axis=0) for b in range(gr.B)])
    spread_k = max(float(np.abs(per_member_k[f:f + m] - per_member_k[f]).max()) for f, m in zip(gr.first, gr.sizes))
    n_out = int((~r['keep']).sum())
    print(f'\n[{case.name}] translation spread inside a group {spread:.2e} (after the last step {spread_k:.2e}); left out {n_out} of {gr.G} groups, '
          f'smallest margin {r["margins"].min():.2e} A')
    assert spread <= 1e-5 and spread_k <= 1e-5
    assert r['margins'].shape == (mc.K + 1, gr.B)
    assert n_out <= mp.CHAIN_CAP * gr.G
    assert r['z_steps'].shape == (mc.K, gr.Nu, 11) and r['pocket_steps'].shape == (mc.K, len(pb.x), 3)
    assert max(pb.num_nodes_phar + pb.size) > 128 or case.big_member is None


def test_argument_checks_without_a_device():
    from helpers import bare_model as _model
    from cmdgen_amd.equivariant_diffusion.conditional_model import ConditionalDDPM, SimpleConditionalDDPM
    from cmdgen_amd.equivariant_diffusion.en_diffusion import EnVariationalDiffusion

    def pocket(sizes):
        n = int(sum(sizes))
        return {'x': torch.randn(n, 3), 'one_hot': torch.zeros(n, 20), 'size': torch.tensor(sizes),
                'mask': torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))}
    m = _model(ConditionalDDPM)
    m.dynamics.hip_handle = None                             # every check below raises before a handle is asked for
    a, b = pocket([3, 4]), pocket([5, 2])
    with pytest.raises(ValueError, match='same groups'):
        m.sample_given_pockets([a, pocket([3, 4, 2])], [2, 3], timesteps=10)
    with pytest.raises(ValueError, match='weights has shape'):
        m.sample_given_pockets([a, b], [2, 3], weights=[1.0, 2.0, 3.0], timesteps=10)
    with pytest.raises(ValueError, match='weights has shape'):
        m.sample_given_pockets([a, b], [2, 3], weights=torch.ones(3, 2), timesteps=10)
    with pytest.raises(ValueError, match='>= 0'):
        m.sample_given_pockets([a, b], [2, 3], weights=[1.5, -0.5], timesteps=10)
    with pytest.raises(ValueError, match='sum to zero'):
        m.sample_given_pockets([a, b], [2, 3], weights=[[1.0, 1.0], [0.0, 0.0]], timesteps=10)
    with pytest.raises(ValueError, match='num_nodes_phar'):
        m.sample_given_pockets([a, b], [2, 3, 4], timesteps=10)
    w = ConditionalDDPM.group_weights([1.0, 3.0], 2, 2)
    assert w.dtype == np.float32 and w.shape == (2, 2) and np.array_equal(w, np.array([[0.25, 0.75]] * 2, np.float32))
    assert np.array_equal(ConditionalDDPM.group_weights(None, 3, 2), np.full((3, 2), 0.5, np.float32))
    with pytest.raises(NotImplementedError, match='SimpleConditionalDDPM'):
        _model(SimpleConditionalDDPM).sample_given_pockets([a, b], [2, 3], timesteps=10)
    with pytest.raises(NotImplementedError, match='joint'):
        EnVariationalDiffusion.sample_given_pockets(m, [a, b], [2, 3])
