"""GPU parity tests, round 3: the in-loop guards driven INTO their triggered branches, and the sampling
chain at BASELINE configs[1]'s literal size against the reference (golden G14).

* CoG-drift re-projection (conditional_model.py:451-457): a final draw scaled so that |x| ~ 1e6 A leaves several ulp of
  centre-of-mass residual (> 5e-2 A) after the COM projection; the reference then projects once more.  HIP result vs oracle.
* ``assert_mean_zero_with_mask`` (en_diffusion.py:919-924) can only fail through a non-finite state (a finite state after
  the projection has a relative COM error of ~1e-7): an infinite draw makes the sample's mean infinite and its
  coordinates NaN; ``x.abs().max()`` is then NaN and ``rel_error < 1e-2`` is False.  The device-side maxima must carry
  the NaN (fmaxf drops it) so that the deferred check raises the reference's AssertionError.
"""
import numpy as np
import pytest
import torch

from helpers import (CHAIN_BAND as BAND, EVAL_TOL, NoiseTape, load_golden, pocket_dict, rms, cases_of, dynamics_case, g14, g14_case,
                     host_step_table, new_handle, per_sample_rms, small_case)
from chain_kit import dev
from cmdgen_amd import hip_backend
from cmdgen_amd.synthetic import ModelConfig, make_state_dict, make_pockets

pytestmark = pytest.mark.gpu


def oracle_chain(cfg, sd, pb, K, noise):
    """-> oracle outputs and how often it projected onto the COM-free subspace (K+2 draws, +1 when the drift fix fires)"""
    from oracle import ref_cpu
    calls = [0]
    orig = ref_cpu.remove_mean_batch

    def counting(*a, **k):
        calls[0] += 1
        return orig(*a, **k)
    ref_cpu.remove_mean_batch = counting
    try:
        with torch.no_grad():
            out = ref_cpu.sample_given_pocket(ref_cpu.to_torch_params(sd), cfg.as_dict(), pocket_dict(pb), pb.num_nodes_phar,
                                              timesteps=K, noise=NoiseTape(noise))
    finally:
        ref_cpu.remove_mean_batch = orig
    return out, calls[0]


# ----------------------------------------------------------------------------- a16: the drift fix, taken
@pytest.mark.parametrize('use_graph', [False, True])
@pytest.mark.parametrize('amp, fires', [(1.0, False), (1e8, True), (1e9, True)])
def test_cog_drift_reprojection_matches_oracle(amp, fires, use_graph):
    cfg, sd, pb, K, noise = small_case()
    noise[K + 1, :, :3] *= amp          # x = mu_x + exp(gamma_0 / 2) * draw: |x| ~ 3e-3 * amp
    (want, want_p, _, _), n_proj = oracle_chain(cfg, sd, pb, K, noise)
    assert n_proj == K + 2 + (1 if fires else 0)                       # the oracle took / did not take the branch
    h = new_handle(cfg, sd)
    h.set_layout(pb.num_nodes_phar, pb.size)
    h.set_step_table(K, host_step_table(cfg, K))
    got, got_p, _ = h.sample_chain(dev(pb.x), dev(pb.one_hot), K, noise=dev(noise), use_graph=use_graph)
    st = h.chain_status()
    assert (st['max_cog'] > 5e-2) == fires, st                         # the drift the device recorded BEFORE the fix
    assert st['max_rel_com_error'] < 1e-2                               # relative error stays ~1e-7: no assertion
    got, got_p, want, want_p = got.cpu().numpy(), got_p.cpu().numpy(), want.numpy(), want_p.numpy()
    # same operations in the same order on (nearly) the same numbers: agreement to a few units in the last place of |x|
    tol = 4.0 * float(np.spacing(np.float32(np.abs(want[:, :3]).max()))) if fires else 1e-4 * max(1.0, float(np.abs(want[:, :3]).max()))
    assert float(np.abs(got[:, :3] - want[:, :3]).max()) <= tol
    assert float(np.abs(got_p[:, :3] - want_p[:, :3]).max()) <= tol
    assert np.array_equal(got[:, 3:], want[:, 3:]) and np.array_equal(got_p[:, 3:], want_p[:, 3:])
    if fires:
        # the re-projection moved the result: without it the pocket would sit where the last in-loop projection left it.
        # The second projection subtracts each sample's residual mean (|residual| / n_b); recompute it from the oracle's output.
        pm = np.repeat(np.arange(len(pb.size)), pb.num_nodes_phar)
        resid = np.stack([want[pm == b, :3].sum(0) for b in range(len(pb.size))])
        assert np.abs(resid).max() <= st['max_cog'] * 4 + 1.0              # still ulp-sized, not grown
    h.close()


# ----------------------------------------------------------------------------- a16: the assertion, failing
def test_mean_zero_assertion_fires_like_reference():
    from oracle import ref_cpu
    cfg, sd, pb, K, noise = small_case(seed=92)
    noise[2, 5, 1] = np.inf             # one infinite draw in the second posterior step
    with pytest.raises(AssertionError, match='Mean is not zero, relative_error nan'):
        with torch.no_grad():
            ref_cpu.sample_given_pocket(ref_cpu.to_torch_params(sd), cfg.as_dict(), pocket_dict(pb), pb.num_nodes_phar,
                                        timesteps=K, noise=NoiseTape(noise))
    # C ABI: the deferred check reports NaN (not 0: fmaxf / `rel > worst` would both have dropped it)
    h = new_handle(cfg, sd)
    h.set_layout(pb.num_nodes_phar, pb.size)
    h.set_step_table(K, host_step_table(cfg, K))
    for use_graph in (False, True):
        h.sample_chain(dev(pb.x), dev(pb.one_hot), K, noise=dev(noise), use_graph=use_graph)
        st = h.chain_status()
        assert np.isnan(st['max_rel_com_error']), st
        assert st['nan_resets'] >= 1                                    # the evaluations after it saw NaN positions (dynamics.py:129-131)
    h.close()
    # Python mirror: the same exception, the same text
    from cmdgen_amd.equivariant_diffusion.dynamics import EGNNDynamics
    from cmdgen_amd.equivariant_diffusion.conditional_model import ConditionalDDPM
    dyn = EGNNDynamics(phar_nf=8, residue_nf=20, n_dims=3, joint_nf=32, hidden_nf=64, n_layers=2, attention=True,
                       tanh=True, norm_constant=1, inv_sublayers=1, normalization_factor=100, aggregation_method='sum',
                       edge_cutoff=6.0, update_pocket_coords=False)
    ddpm = ConditionalDDPM(dynamics=dyn, phar_nf=8, residue_nf=20, n_dims=3, timesteps=500,
                           noise_schedule='polynomial_2', noise_precision=1e-5, loss_type='l2', norm_values=[1, 4],
                           size_histogram=np.ones((30, 70)))
    ddpm.load_state_dict({k[len('ddpm.'):]: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    ddpm = ddpm.cuda()
    pocket = {k: v.cuda() for k, v in pocket_dict(pb).items()}
    with pytest.raises(AssertionError, match='Mean is not zero, relative_error nan'):
        ddpm.sample_given_pocket(pocket, torch.from_numpy(pb.num_nodes_phar), timesteps=K, noise=torch.from_numpy(noise))
    # and a clean chain right after on the same model still passes its checks
    noise[2, 5, 1] = 0.5
    ddpm.sample_given_pocket(pocket, torch.from_numpy(pb.num_nodes_phar), timesteps=K, noise=torch.from_numpy(noise))
    assert ddpm.last_chain_status['max_rel_com_error'] < 1e-2


# ----------------------------------------------------------------------------- G14: configs[1] / configs[4] at their literal size
G14 = g14()


def batch_rms(a, b):
    return float(np.sqrt(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2)))


@pytest.mark.parametrize('engine', ['split', 'fp32'])
@pytest.mark.parametrize('name', ['ca_b64_K1000', 'fa_b8_K100', 'ca_b256_K50', 'fa_b32_K10'])
def test_fullsize_chain_matches_reference_g14(name, engine):
    """BASELINE configs[1] at its literal size (64 C-alpha pockets, H=256, L=5, K = T = 1000), configs[4]'s pocket shape
    (8 x 366 full-atom atoms, K = 100) and the north-star batch (256 C-alpha pockets, K = 50: on a 256-CU device the split engine
    runs its node blocks on k_node64 here; and 32 full-atom pockets, K = 10: the same kernel on full-atom geometry) against the REAL
    reference's chain, eager and graph, both matrix engines:
      * north_star's sentence, literally: coordinate RMS over the WHOLE batch (no sample excluded) <= 1e-4 A absolute, at
        every checkpoint (every 100 / 10 steps) and at the end; pocket translation likewise;
      * per sample: every sample none of whose pairs came within BAND of the cutoff (margins recorded by the fixture: the
        radius graph is a hard threshold, and at this size thousands of pair tests per chain land within 1e-5 A of it; the
        reference's own torch.cdist decided 2 of its 4e8 pair tests against the exact rule) <= 1e-4 A, types exact;
      * pocket types untouched for every sample."""
    cfg, sd, pb, K, window, noise = g14_case(name)
    B = len(pb.size)
    want, want_p = G14[name + '/xh_phar'], G14[name + '/xh_pocket']
    margins = G14[name + '/margins']                                   # [windows, B]
    clean_upto = np.minimum.accumulate(margins, axis=0) > BAND         # [w, b]: every evaluation of windows 0..w kept its margin
    steps, ck_z, ck_com = G14[name + '/ckpt_steps'], G14[name + '/ckpt_z'], G14[name + '/ckpt_pocket_com']
    h = new_handle(cfg, sd)
    h.set_gemm_mode(engine == 'split')
    h.set_layout(pb.num_nodes_phar, pb.size)
    h.set_step_table(K, host_step_table(cfg, K))
    nd = dev(noise.numpy())
    report = []
    for use_graph in (False, True):
        got, got_p, z_steps = h.sample_chain(dev(pb.x), dev(pb.one_hot), K, noise=nd, want_steps=True, use_graph=use_graph)
        st = h.chain_status()
        assert st['max_rel_com_error'] < 1e-2 and st['nan_resets'] == 0
        got, got_p = got.cpu().numpy(), got_p.cpu().numpy()
        ps = h.last_pocket_steps
        for i, s in enumerate(steps):
            # evaluations 0..s-1 produced the state after posterior step s: windows 0..(s-1)//window lie behind it
            ok = clean_upto[(int(s) - 1) // window]
            z = z_steps[int(s) - 1].cpu().numpy()
            assert batch_rms(z[:, :3], ck_z[i][:, :3]) <= 1e-4, (name, engine, use_graph, int(s))
            e = per_sample_rms(z[:, :3], ck_z[i][:, :3], B)
            eh = per_sample_rms(z[:, 3:], ck_z[i][:, 3:], B)            # the feature part of z (what the types are decoded from)
            assert e[ok].max() <= 1e-4 and eh[ok].max() <= 1e-4, (name, engine, use_graph, int(s), float(e[ok].max()), float(eh[ok].max()))
            com = np.stack([ps[int(s) - 1].cpu().numpy().astype(np.float64)[pb.mask == b].mean(0) for b in range(B)])
            assert float(np.sqrt(np.mean((com - ck_com[i]) ** 2))) <= 1e-4 and np.abs(com - ck_com[i])[ok].max() <= 1e-4
        ok = clean_upto[-1]
        assert ok.sum() >= max(2, B // 8), int(ok.sum())
        all_rms, all_rms_p = batch_rms(got[:, :3], want[:, :3]), batch_rms(got_p[:, :3], want_p[:, :3])
        assert all_rms <= 1e-4 and all_rms_p <= 1e-4, (name, engine, use_graph, all_rms, all_rms_p)
        e = per_sample_rms(got[:, :3], want[:, :3], B)
        ep = per_sample_rms(got_p[:, :3], want_p[:, :3], B)
        types_ok = (got[:, 3:] == want[:, 3:]).reshape(B, -1).all(1)
        report.append((use_graph, all_rms, int(ok.sum()), float(e[ok].max()), int((e <= 1e-4).sum()), float(np.median(e)), float(e.max()), int(types_ok.sum())))
        assert e[ok].max() <= 1e-4 and ep[ok].max() <= 1e-4, (name, engine, use_graph, float(e[ok].max()))
        assert types_ok[ok].all()
        assert np.array_equal(got_p[:, 3:], want_p[:, 3:])              # pocket types untouched, every sample
    for use_graph, all_rms, n_ok, worst, n_within, med, mx, n_types in report:
        print(f'{name} {engine} graph={use_graph}: coordinate RMS over the whole batch {all_rms:.2e} A; {n_ok}/{B} samples kept a margin > '
              f'{BAND:g} A over all {K + 1} evaluations, worst of them {worst:.2e} A; per sample: {n_within}/{B} within 1e-4 A, median {med:.2e}, '
              f'max {mx:.2e}; types identical in {n_types}/{B}; max|x| {float(G14[name + "/max_abs_x"]):.1f} A, '
              f'{float(G14[name + "/edges_per_pocket_eval"]):.0f} edges per pocket-evaluation')
    h.close()


# ----------------------------------------------------------------------------- dead work of the last block (round 3)
G2 = load_golden('g2_dynamics.npz')
def test_last_block_dead_work_skip_changes_nothing(monkeypatch):
    """The last EquivariantBlock of a conditional evaluation whose pocket output nobody asks for: the new h of a pocket node is read only if
    the node sends along a coordinate edge, so message tiles without such a receiver and node tiles without such a row are skipped
    (cmdgen_counters.edges_skipped / node_rows_skipped).  (i) every H = 256 evaluation fixture, pocket output not requested, against the
    reference; (ii) a 300-step chain of 24 pockets with the skip on and off: the same result (to the run-to-run noise of the float atomics), work skipped only when on."""
    for name in [n for n in cases_of(G2) if '_h256_' in n]:
        cfg, sd, inp = dynamics_case(G2, name)
        h = new_handle(cfg, sd)
        h.set_layout(G2[name + '/num_nodes_phar'], G2[name + '/pocket_size'])
        assert h.query('dead_skip') == 2
        eps, none = h.dynamics_forward(dev(inp['xh_phar']), dev(inp['xh_pocket']), dev(inp['t']), want_pocket=False)
        eps2, _ = h.dynamics_forward(dev(inp['xh_phar']), dev(inp['xh_pocket']), dev(inp['t']), want_pocket=False)     # agg left zero
        want = G2[name + '/eps_phar']
        assert none is None
        for e in (eps, eps2):
            assert float(np.abs(e.cpu().numpy() - want).max()) <= EVAL_TOL * max(1.0, float(np.abs(want).max())), name
        h.close()
    cfg = ModelConfig(residue_nf=20, timesteps=1000)
    sd = make_state_dict(cfg, seed=0)
    pb = make_pockets(24, 'CA')
    out = {}
    for flag in ('2', '1', '0'):
        monkeypatch.setitem(hip_backend.DEFAULT_OPTIONS, 'dead_skip', int(flag))
        h = new_handle(cfg, sd)
        h.set_layout(pb.num_nodes_phar, pb.size)
        assert h.query('dead_skip') == int(flag)
        h.reset_counters()
        xh, xp, _ = h.sample_chain(dev(pb.x), dev(pb.one_hot), 300, seed=11)
        c = h.counters()
        out[flag] = (xh.cpu().numpy(), xp.cpu().numpy(), c)
        assert h.chain_status()['nan_resets'] == 0
        h.close()
    on, off, last = out['2'][2], out['0'][2], out['1'][2]
    print(f'24 pockets, 300 steps: {on["edges_skipped"] / on["evaluations"]:.0f} of {5 * on["edges"] / on["evaluations"]:.0f} edge visits and '
          f'{on["node_rows_skipped"] / on["evaluations"]:.0f} of {5 * on["nodes"] / on["evaluations"]:.0f} node-row visits skipped per evaluation (all blocks; the last block alone: {last["edges_skipped"] / last["evaluations"]:.0f} edges)')
    assert off['edges_skipped'] == 0 and off['node_rows_skipped'] == 0 and on['edges_skipped'] > last['edges_skipped'] > 0
    # (node tiles are skipped by the plane tiles of large batches only: k_node64; see test_node64_skips_dead_tiles_at_256_pockets)
    # (float atomics at tile boundaries make two runs of the SAME code differ in the last bits; the skip adds nothing to that)
    sc = max(1.0, float(np.abs(out['0'][0][:, :3]).max()))
    for f in ('2', '1'):
        assert np.abs(out[f][0][:, :3] - out['0'][0][:, :3]).max() <= 2e-5 * sc and np.array_equal(out[f][0][:, 3:], out['0'][0][:, 3:])
        assert np.abs(out[f][1][:, :3] - out['0'][1][:, :3]).max() <= 2e-5 * sc


def test_node64_skips_dead_tiles_at_256_pockets(monkeypatch):
    """256 pockets (k_node64 on a 256-CU device): a drifted 60-step chain with every block skipping its dead tiles (default) against the same chain with
    the skip off - same result to the run-to-run noise of the float atomics, node rows skipped only when on."""
    cfg = ModelConfig(residue_nf=20, timesteps=1000)
    sd = make_state_dict(cfg, seed=0)
    pb = make_pockets(256, 'CA')
    out = {}
    for flag in ('2', '0'):
        monkeypatch.setitem(hip_backend.DEFAULT_OPTIONS, 'dead_skip', int(flag))
        h = new_handle(cfg, sd)
        h.set_layout(pb.num_nodes_phar, pb.size)
        h.reset_counters()
        xh, _, _ = h.sample_chain(dev(pb.x), dev(pb.one_hot), 60, seed=3)
        out[flag] = (xh.cpu().numpy(), h.counters(), h.query('node64'))
        assert h.chain_status()['nan_resets'] == 0
        h.close()
    on, off = out['2'][1], out['0'][1]
    print(f'256 pockets, 60 steps: {on["edges_skipped"] / on["evaluations"]:.0f} of {5 * on["edges"] / on["evaluations"]:.0f} edge visits, '
          f'{on["node_rows_skipped"] / on["evaluations"]:.0f} of {5 * on["nodes"] / on["evaluations"]:.0f} node-row visits skipped per evaluation; node64 {out["2"][2]}')
    assert off['edges_skipped'] == 0 and off['node_rows_skipped'] == 0 and on['edges_skipped'] > 0
    if out['2'][2]: assert on['node_rows_skipped'] > 0
    sc = max(1.0, float(np.abs(out['0'][0][:, :3]).max()))
    assert np.abs(out['2'][0][:, :3] - out['0'][0][:, :3]).max() <= 2e-5 * sc and np.array_equal(out['2'][0][:, 3:], out['0'][0][:, 3:])


# ----------------------------------------------------------------------------- G15 (round 4): the SHIPPED schedule, step by step
G15 = load_golden('g15_shipped_schedule_chain.npz')


@pytest.mark.parametrize('engine', ['split', 'fp32'])
def test_shipped_schedule_chain_per_step_g15(engine):
    """The REAL reference's K = T = 500 chain under the shipped schedule (noise_precision 1e-5, norm_values [1, 4]; 8 C-alpha pockets, H = 256,
    L = 5; make_golden_r4.py): with untrained weights the coordinates inflate by 1/alpha_T = 316, so the bound is stated in units of the fp32
    spacing at the coordinates' magnitude - at EVERY 50-step checkpoint the per-step z (x columns AND the h columns carrying the [1, 4] scaling)
    agrees with the reference to <= 4 ulp(max|z|) RMS and <= 32 ulp(max|z|) for the worst element, eager and graph; final x likewise, types exact.
    Every sample kept a cutoff margin > 3e-4 A over the whole chain (fixture), so no edge decision is in question."""
    name = 'ca_b8_KT500_shipped'
    H, L, B, R, seed, K, T, first, nseed, window = [int(v) for v in G15[name + '/meta']]
    cfg = ModelConfig(hidden_nf=H, n_layers=L, residue_nf=R, timesteps=T, noise_precision=float(G15[name + '/noise_precision']),
                      norm_values=tuple(float(v) for v in G15[name + '/norm_values']))
    assert cfg.noise_precision == 1e-5 and tuple(cfg.norm_values) == (1.0, 4.0)
    sd = make_state_dict(cfg, seed=seed, coord_gain=float(G15[name + '/coord_gain']))
    pb = make_pockets(B, 'CA', n_phar=15, first_index=first)
    Nl = int(pb.num_nodes_phar.sum())
    gen = torch.Generator().manual_seed(nseed)
    noise = torch.stack([torch.randn((Nl, 11), generator=gen) for _ in range(K + 2)])
    probe = G15[name + '/noise_probe']
    assert np.array_equal(noise[0, :4].numpy(), probe[0]) and np.array_equal(noise[K + 1, :4].numpy(), probe[1])
    assert float(G15[name + '/margins'].min()) > 1e-4
    steps, ck_z = G15[name + '/ckpt_steps'], G15[name + '/ckpt_z']
    want = G15[name + '/xh_phar']
    ulp = lambda v: float(2.0 ** (np.floor(np.log2(max(float(v), 1e-30))) - 23))
    h = new_handle(cfg, sd)
    h.set_gemm_mode(engine == 'split')
    h.set_layout(pb.num_nodes_phar, pb.size)
    h.set_step_table(K, host_step_table(cfg, K))
    worst = []
    for use_graph in (False, True):
        got, got_p, z_steps = h.sample_chain(dev(pb.x), dev(pb.one_hot), K, noise=dev(noise.numpy()), want_steps=True, use_graph=use_graph)
        st = h.chain_status()
        assert st['max_rel_com_error'] < 1e-2 and st['nan_resets'] == 0
        for i, s in enumerate(steps):
            z = z_steps[int(s) - 1].cpu().numpy().astype(np.float64)
            for lo, hi, what in ((0, 3, 'x'), (3, 11, 'h')):
                ref = ck_z[i][:, lo:hi].astype(np.float64)
                u = ulp(np.abs(ref).max())
                d = z[:, lo:hi] - ref
                r, m = float(np.sqrt((d ** 2).mean())) / u, float(np.abs(d).max()) / u
                worst.append((r, m, int(s), what, use_graph, float(np.abs(ref).max())))
                assert r <= 4.0 and m <= 32.0, (engine, use_graph, int(s), what, r, m)
        g = got.cpu().numpy()
        u = ulp(np.abs(want[:, :3]).max())
        assert float(np.sqrt(((g[:, :3].astype(np.float64) - want[:, :3]) ** 2).mean())) <= 4.0 * u
        assert np.array_equal(g[:, 3:], want[:, 3:])
    r, m, s, what, ug, mag = max(worst)
    print(f'G15 {engine}: worst checkpoint RMS {r:.2f} ulp (max element {max(w[1] for w in worst):.1f} ulp) at step {s} ({what} columns, max|z| {mag:.1f}); '
          f'final max|x| {float(np.abs(want[:, :3]).max()):.1f} A')
    h.close()
