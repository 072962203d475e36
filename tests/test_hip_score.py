"""GPU tests of ConditionalDDPM.score / cmdgen_score_chain: parity with the G21 vectors (the reference's own forward, one call per
level; tests/golden/make_golden_score.py), the existing forward as a second route through the same kernels, independence of the
levels, graphs against eager runs while scoring, sampling and inpainting alternate on one handle, device draws and sharding, the half
engine's range guard, the driver entries and the refusals.

The bound of an entry.  The project's evaluation bound is max |d eps| <= 2e-5 max(1, |eps|); through the square,
    |d error| <= 2 d sqrt(D error) + D d^2,   d = 2e-5 max(1, max |net|),  D = rows x columns of the sample
(score_ref.error_bound), with net the oracle's for that sample and level.  The categorical term gets rtol 1e-4, atol 1e-3 (the bound
tests/test_hip_parity.py asserts for G6's eval-mode nll, of which loss_0_h is a part).  A (level, sample) entry whose input positions
hold a pair within 1e-4 A of the cutoff is left out - at most 2 % of a case, and none in the committed cases."""
import os
import warnings

import numpy as np
import pytest
import torch

from helpers import GOLDEN, HIST, RANGE_NAME, RANGE_TARGETS, SCORE_BAND as BAND, SCORE_CASES as CASES, g2, g21, overflow_case, score_case
import score_ref
from chain_kit import dev, lightning_model, model_for, philox_noise, score_entry_ratios as entry_ratios, to_dev
from oracle import ref_cpu
from cmdgen_amd import hip_backend
from cmdgen_amd.synthetic import ModelConfig, make_pockets, make_state_dict
from bench import bounded_config

pytestmark = pytest.mark.gpu

G21 = g21()


def score_model(cfg, sd, hist=HIST):
    """The model as ddpm.forward's comparisons need it: in eval mode, with the goldens' size histogram."""
    return model_for(cfg, sd, hist).eval()


def case_arrays(case):
    return {k[len(case) + 1:]: v for k, v in G21.items() if k.startswith(case + '/')}


@pytest.mark.parametrize('use_graph', [True, False])
@pytest.mark.parametrize('case', CASES)
def test_score_matches_g21(case, use_graph):
    """1. Every (level, sample) entry against the reference's forward at that level, and the assembled nll against its own entries."""
    cfg, sd, phar, pocket = score_case()
    g = case_arrays(case)
    K = int(case[1:])
    ddpm = score_model(cfg, sd)
    ddpm.use_hip_graph = use_graph
    out = ddpm.score(to_dev(phar), to_dev(pocket), timesteps=K, noise=dev(g['noise']), return_levels=True)
    out = {k: v.cpu().numpy() for k, v in out.items()}
    st = ddpm.last_chain_status
    assert st['max_rel_com_error'] < 1e-2 and st['nan_resets'] == 0
    assert np.array_equal(out['t_levels'], g['t_levels'])
    sums = out['level_sums'][0]
    keep = g['margins'] >= BAND
    left_out = int((~keep).sum())
    assert left_out <= 0.02 * keep.size, f'{left_out} of {keep.size} entries inside the band: more than 2 %'
    n_rows = phar['size'].numpy()
    ratios = entry_ratios(sums, g['error_t'].astype(np.float64), g['loss_0_x'][0].astype(np.float64), g['netmax'], n_rows, keep)
    print(f'{case} graph={use_graph}: {left_out} entries left out, worst |d error| / bound {ratios.max():.3e} over {ratios.size} entries')
    assert ratios.max() <= 1.0
    assert (sums[..., 3] == 0).all() and (sums[:K, :, 2] == 0).all()
    if keep[K].all():
        assert np.allclose(out['loss_0_h'], g['loss_0_h'][0], rtol=1e-4, atol=1e-3)
        assert np.allclose(out['loss_0_x'], 0.5 * sums[K, :, 1], rtol=0, atol=0)
    assert np.allclose(out['kl_prior'], g['kl_prior'][0], rtol=2e-5, atol=2e-5 * max(1.0, float(np.abs(g['kl_prior']).max())))
    assert np.array_equal(out['neg_log_const_0'], g['neg_log_const_0'][0]) and np.array_equal(out['log_pN'], g['log_pN'][0])
    # the assembly: the device entries summed by the mirror against the same entries summed in float64 here
    f64 = out['level_terms'][0].astype(np.float64).sum(0) + (out['neg_log_const_0'].astype(np.float64) + out['kl_prior']
                                                             - out['delta_log_px'] - out['log_pN'])
    assert np.allclose(out['nll'], f64, rtol=1e-6, atol=0)
    assert np.isfinite(out['nll']).all()


def test_score_and_forward_are_two_routes_through_the_same_kernels():
    """2. error_k, loss_0_x and loss_0_h of score against ddpm.forward(t_int=t, eps=[eps_t, eps_0]) on the same handle: the evaluation
    kernels are the same, z is formed by different code (last-bit differences), so the bound is item 1's with net from forward."""
    case = 'K20'
    cfg, sd, phar, pocket = score_case()
    g = case_arrays(case)
    K = 20
    ddpm = score_model(cfg, sd)
    ph, pk = to_dev(phar), to_dev(pocket)
    out = ddpm.score(ph, pk, timesteps=K, noise=dev(g['noise']), return_levels=True)
    sums = out['level_sums'][0].cpu().numpy()
    assert (g['margins'] >= BAND).all()
    n_rows, pm, B = phar['size'].numpy(), phar['mask'].numpy(), len(phar['size'])
    worst = 0.0
    for k in (0, 7, 12, 19):
        t = float(g['t_levels'][k])
        terms = ddpm.forward(ph, pk, t_int=torch.full((B, 1), t), eps=[dev(g['noise'][k]), dev(g['noise'][K])])
        net = ddpm._last_train_ctx['net_out'].cpu().numpy()
        netmax = np.asarray([np.abs(net[pm == b]).max() for b in range(B)])
        err = terms[1].cpu().numpy().astype(np.float64)
        r = np.abs(sums[k, :, 0] - err) / score_ref.error_bound(err, netmax, n_rows, 11)
        ddpm.forward(ph, pk, t_int=torch.zeros((B, 1)), eps=[dev(g['noise'][K]), dev(g['noise'][K])])      # its net_out is the t = 0 level's
        net0 = ddpm._last_train_ctx['net_out'].cpu().numpy()
        netmax0 = np.asarray([np.abs(net0[pm == b]).max() for b in range(B)])
        l0x = terms[4].cpu().numpy().astype(np.float64)
        r0 = np.abs(0.5 * sums[K, :, 1] - l0x) / (0.5 * score_ref.error_bound(2.0 * l0x, netmax0, n_rows, 3))
        worst = max(worst, float(r.max()), float(r0.max()))
        assert np.allclose(-sums[K, :, 2], terms[6].cpu().numpy(), rtol=1e-4, atol=1e-3)
    print(f'two routes: worst |d error| / bound {worst:.3e} (far inside 1: rounding; near 1: the routes disagree about the formula)')
    assert worst <= 1.0


def test_levels_are_independent():
    """3. With injected draws the K = 20 entries are bit-identical to the matching entries of the K = 100 run."""
    cfg, sd, phar, pocket = score_case()
    g = case_arrays('K100')
    ddpm = score_model(cfg, sd)
    ph, pk = to_dev(phar), to_dev(pocket)
    full = ddpm.score(ph, pk, timesteps=100, noise=dev(g['noise']), return_levels=True)
    pick = [5 * (j + 1) - 1 for j in range(20)] + [100]
    part = ddpm.score(ph, pk, timesteps=20, noise=dev(g['noise'][pick]), return_levels=True)
    assert torch.equal(part['t_levels'], full['t_levels'][pick])
    assert torch.equal(part['level_sums'][0], full['level_sums'][0][pick])
    assert torch.equal(part['kl_prior'], full['kl_prior'])


def _bench_inputs(B=5, first=500, seed=5):
    pb = make_pockets(B, 'CA', ragged=True, first_index=first)
    rng = np.random.default_rng(seed)
    nl = pb.num_nodes_phar
    pm = np.repeat(np.arange(len(nl)), nl)
    com = np.stack([pb.x[pb.mask == b].mean(0) for b in range(len(nl))])
    px = (com[pm] + rng.normal(size=(len(pm), 3)) * 2.5).astype(np.float32)
    poh = np.eye(8, dtype=np.float32)[rng.integers(0, 8, size=len(pm))]
    first_row = np.concatenate([[0], np.cumsum(nl)[:-1]])
    fixed = ((np.arange(len(pm)) - first_row[pm]) < np.maximum(1, nl[pm] // 4)).astype(np.float32)
    return pb, px, poh, fixed


def test_graph_runs_equal_eager_runs_while_chains_alternate():
    """4. score -> sample -> inpaint -> score with graphs on one handle: each equals its own eager run bit for bit (a repeated call
    too), with device draws, injected draws and graph_steps = 5 at 21 levels (four replays and one eager step)."""
    cfg = bounded_config(20, 1000)
    h = hip_backend.Handle(cfg.as_dict(), 0)
    h.load_state_dict(make_state_dict(cfg, seed=0))
    pb, px, poh, fixed = _bench_inputs()
    h.set_layout(pb.num_nodes_phar, pb.size)
    K = 20
    levels = np.concatenate([(np.arange(K) + 1) * (1000 // K), [0]])
    nl = int(pb.num_nodes_phar.sum())
    noise = dev(np.random.default_rng(6).normal(size=(K + 1, nl, 11)).astype(np.float32))
    a_sc = (dev(px), dev(poh), dev(pb.x), dev(pb.one_hot))
    a_in = (dev(pb.x), dev(pb.one_hot), dev(px), dev(poh), dev(fixed))

    def score(use_graph, seed, inject=False):
        terms, kl = h.score_chain(*a_sc, levels, noise=noise if inject else None, seed=seed, use_graph=use_graph)
        st = h.chain_status()
        return [terms.cpu().numpy(), kl.cpu().numpy()], (st['max_rel_com_error'], st['nan_resets'])

    def plain(use_graph, seed):
        out = h.sample_chain(a_in[0], a_in[1], K, seed=seed, use_graph=use_graph)
        h.chain_status()
        return [o.cpu().numpy() for o in out[:2]]

    def inpaint(use_graph, seed):
        out = h.inpaint_chain(*a_in, K, seed=seed, use_graph=use_graph)
        h.chain_status()
        return [o.cpu().numpy() for o in out[:2]]

    for gs in (None, 5):
        if gs:
            h.set_option('graph_steps', gs)
        eager = [score(False, 1), plain(False, 2), inpaint(False, 3), score(False, 4), score(False, 4, inject=True)]
        graph = [score(True, 1), plain(True, 2), inpaint(True, 3), score(True, 4), score(True, 4, inject=True)]
        again = [score(True, 1), plain(True, 2), inpaint(True, 3), score(True, 4), score(True, 4, inject=True)]
        for run in (graph, again):
            for i, (a, b) in enumerate(zip(run, eager)):
                if i in (0, 3, 4):
                    assert a[1] == b[1], (gs, i)
                    a, b = a[0], b[0]
                for x, y in zip(a, b):
                    assert np.array_equal(x, y), (gs, i)
        assert np.isfinite(graph[0][0][0]).all() and (graph[0][0][0][..., 0] > 0).all()
        assert not np.array_equal(graph[0][0][0], graph[3][0][0])            # seeds 1 and 4
    h.close()


def test_device_draws():
    """5. noise=None equals the run that injects the same Philox draws (cmdgen_debug_noise) bit for bit; two seeds differ; a batch
    scored in two shards with global pocket ids gives the whole batch's entries within item 1's bound."""
    cfg, sd, phar, pocket = score_case()
    ddpm = score_model(cfg, sd)
    ph, pk = to_dev(phar), to_dev(pocket)
    K, B = 20, len(phar['size'])
    nl = phar['size'].numpy()
    a = ddpm.score(ph, pk, timesteps=K, seed=11, return_levels=True)
    h = ddpm.dynamics.hip_handle()
    noise = philox_noise(h, 11, range(B), nl, range(K + 1))
    b = ddpm.score(ph, pk, timesteps=K, noise=noise, return_levels=True)
    assert torch.equal(a['level_sums'], b['level_sums']) and torch.equal(a['nll'], b['nll'])
    c = ddpm.score(ph, pk, timesteps=K, seed=12, return_levels=True)
    assert not torch.equal(a['level_sums'], c['level_sums'])
    # the oracle at these draws: margins (the comparison needs a case without band entries) and max |net|
    p = ref_cpu.to_torch_params(sd)
    with torch.no_grad():
        raw = score_ref.score_levels(p, cfg.as_dict(), phar, pocket, a['t_levels'].tolist(), noise.cpu().numpy())
    from cmdgen_amd.synthetic import min_cutoff_margin
    pm, qm = phar['mask'].numpy(), pocket['mask'].numpy()
    margins = np.asarray([[min_cutoff_margin(np.concatenate([raw['z'][k][pm == s, :3].numpy(), raw['pocket_x'][k][qm == s].numpy()]),
                                             np.zeros(int((pm == s).sum() + (qm == s).sum()), dtype=np.int64), 6.0)
                           for s in range(B)] for k in range(K + 1)])
    keep = margins >= BAND
    assert (~keep).sum() <= 0.02 * keep.size
    whole = a['level_sums'][0].cpu().numpy()
    want_err, want_l0x = raw['err'][:K].numpy().astype(np.float64), 0.5 * raw['err_x'][K].numpy().astype(np.float64)
    r = entry_ratios(whole, want_err, want_l0x, raw['netmax'].numpy(), nl, keep)
    print(f'device draws against the oracle at the same draws: worst ratio {r.max():.3e}, {int((~keep).sum())} entries left out')
    assert r.max() <= 1.0
    shards = []
    for lo, hi in ((0, 2), (2, 4)):
        rows_l = (pm >= lo) & (pm < hi)
        rows_q = (qm >= lo) & (qm < hi)
        sp = {'x': ph['x'][dev(rows_l)], 'one_hot': ph['one_hot'][dev(rows_l)], 'size': ph['size'][lo:hi], 'mask': ph['mask'][dev(rows_l)] - lo}
        sq = {'x': pk['x'][dev(rows_q)], 'one_hot': pk['one_hot'][dev(rows_q)], 'size': pk['size'][lo:hi], 'mask': pk['mask'][dev(rows_q)] - lo}
        shards.append(ddpm.score(sp, sq, timesteps=K, seed=11, pocket_ids=list(range(lo, hi)), return_levels=True)['level_sums'][0].cpu().numpy())
    sharded = np.concatenate(shards, axis=1)
    # both runs lie within the bound of the oracle, so they lie within twice the bound of each other
    bound_t = score_ref.error_bound(want_err, raw['netmax'].numpy()[:K], nl, 11)
    d = (np.abs(sharded[:K, :, 0].astype(np.float64) - whole[:K, :, 0]) / bound_t)[keep[:K]]
    r2 = entry_ratios(sharded, want_err, want_l0x, raw['netmax'].numpy(), nl, keep)
    print(f'two shards: worst ratio to the oracle {r2.max():.3e}, to the whole batch {d.max():.3e}')
    assert r2.max() <= 1.0 and d.max() <= 1.0


# ---------------------------------------------------------------- 6. the half engine's range (recipe of tests/test_hip_half_range.py)
@pytest.mark.parametrize('target', list(RANGE_TARGETS))
def test_range_guard(target):
    """The raw score_chain on the half engine reports reset levels; ddpm.score warns, re-runs on the bf16 engine and meets item 1's
    bound against the oracle.  (The guard's normal path, as in the existing range tests.)"""
    cfg, sd, inp = overflow_case(target)
    nl, npk = g2()[RANGE_NAME + '/num_nodes_phar'], g2()[RANGE_NAME + '/pocket_size']
    B = len(nl)
    pm, qm = inp['mask_phar'], inp['mask_pocket']
    phar = {'x': torch.from_numpy(inp['xh_phar'][:, :3].copy()),
            'one_hot': torch.from_numpy(np.eye(8, dtype=np.float32)[inp['xh_phar'][:, 3:].argmax(1)]),
            'size': torch.from_numpy(nl.astype(np.int64)), 'mask': torch.from_numpy(pm.copy())}
    pocket = {'x': torch.from_numpy(inp['xh_pocket'][:, :3].copy()),
              'one_hot': torch.from_numpy(np.round(inp['xh_pocket'][:, 3:] * cfg.norm_values[1]).astype(np.float32)),
              'size': torch.from_numpy(npk.astype(np.int64)), 'mask': torch.from_numpy(qm.copy())}
    K, T = 4, cfg.timesteps
    levels = score_ref.level_list(T, K)
    noise = np.random.default_rng(3).normal(size=(K + 1, len(pm), 11)).astype(np.float32)
    p = ref_cpu.to_torch_params(sd)
    with torch.no_grad():
        raw = score_ref.score_levels(p, cfg.as_dict(), phar, pocket, levels, noise)
    assert torch.isfinite(raw['err']).all() and float(raw['netmax'].min()) > 0, 'the oracle must stay finite and take no reset'
    # 1. the raw chain on the half engine
    h = hip_backend.Handle(cfg.as_dict(), 0)
    h.load_state_dict(sd)
    h.set_layout(nl, npk)
    assert h.half_engine_active()
    h.reset_counters()
    terms, _ = h.score_chain(dev(phar['x'].numpy()), dev(phar['one_hot'].numpy()), dev(pocket['x'].numpy()), dev(pocket['one_hot'].numpy()),
                             np.asarray(levels), noise=dev(noise))
    st = h.chain_status()
    terms = terms.cpu().numpy()
    print(f'{target}: raw half-engine chain: {st["nan_resets"]} reset levels, flags {terms[:, 0, 3]}')
    assert st['nan_resets'] >= 1 and st['nan_resets'] == int(terms[:, 0, 3].sum())
    h.close()
    # 2. the mirror: warning, bf16 re-run, oracle-equal entries
    ddpm = score_model(cfg, sd, hist=np.ones((30, 70)))
    with pytest.warns(RuntimeWarning, match='half matrix engine'):
        out = ddpm.score(to_dev(phar), to_dev(pocket), timesteps=K, noise=dev(noise), return_levels=True)
    st = ddpm.last_chain_status
    assert st.get('half_engine_fallback') and st['nan_resets'] == 0
    assert ddpm.dynamics.hip_handle().half_engine_active()
    sums = out['level_sums'][0].cpu().numpy()
    keep = np.ones((K + 1, B), dtype=bool)
    r = entry_ratios(sums, raw['err'][:K].numpy().astype(np.float64), 0.5 * raw['err_x'][K].numpy().astype(np.float64),
                     raw['netmax'].numpy(), nl, keep)
    print(f'{target}: guarded score against the oracle: worst ratio {r.max():.3e}')
    assert r.max() <= 1.0 and torch.isfinite(out['nll']).all()


# ---------------------------------------------------------------- 7. the driver
def test_driver_entries():
    model = lightning_model().eval()
    cfg, sd, phar, pocket = score_case()
    data = {'phar_coords': phar['x'], 'phar_one_hot': phar['one_hot'], 'num_phar_atoms': phar['size'], 'phar_mask': phar['mask'],
            'pocket_c_alpha': pocket['x'], 'pocket_one_hot': pocket['one_hot'], 'num_pocket_nodes': pocket['size'],
            'pocket_mask': pocket['mask']}
    a = model.score(data, timesteps=10, seed=3, return_levels=True)
    ph, pk = model.get_phar_and_pocket(data)
    b = model.ddpm.score(ph, pk, timesteps=10, seed=3, return_levels=True)
    assert sorted(a) == sorted(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert a['nll'].shape == (4,) and a['level_terms'].shape == (1, 11, 4)
    # repeats = 2 is the mean of two single runs with the matching draws
    nl = int(phar['size'].sum())
    noise = torch.from_numpy(np.random.default_rng(8).normal(size=(2, 11, nl, 11)).astype(np.float32)).cuda()
    both = model.score(data, timesteps=10, repeats=2, noise=noise)
    one = [model.score(data, timesteps=10, noise=noise[r]) for r in range(2)]
    for k in ('nll', 'loss_t', 'loss_0_x', 'loss_0_h'):
        assert torch.equal(both[k + '_repeats'], torch.stack([o[k] for o in one])), k
        assert torch.equal(both[k], torch.stack([o[k] for o in one]).double().mean(0).float()), k
    # score_phars: three candidates in the g7 pocket
    pdb = os.path.join(GOLDEN, 'g7_pocket.pdb')
    ids = [f'A:{i}' for i in range(1, 30)]
    names = list(model.dataset_info['phar_decoder'])
    c0 = [(names[1], (9.0, 2.0, -15.0)), (names[3], (11.5, 4.0, -13.0)), (names[0], (8.0, 5.0, -12.0))]
    c1 = [(names[2], (10.0, 3.0, -14.0)), (names[2], (12.0, 1.0, -16.0))]
    c2 = [(names[4], (7.0, 2.5, -13.5)), (names[1], (9.5, 6.0, -15.5)), (names[5], (11.0, 3.0, -12.0)), (names[0], (13.0, 4.0, -14.0))]
    out = model.score_phars(pdb, [c0, c1, c2], pocket_ids=ids, timesteps=10, seed=5)
    assert out['nll'].shape == (3,) and bool(torch.isfinite(out['nll']).all())
    again = model.score_phars(pdb, [c0, c1, c2], pocket_ids=ids, timesteps=10, seed=5)
    assert torch.equal(out['nll'], again['nll'])
    # a candidate's entries do not depend on its position in the batch (same seed, same global id): c0 alone against c0 in the batch
    pocket1 = model._pdb_pocket(pdb, 1, ids, None)
    x = torch.tensor([list(xyz) for _, xyz in c0], device='cuda', dtype=torch.float32)
    oh = torch.nn.functional.one_hot(torch.tensor([names.index(n) for n, _ in c0], device='cuda'), 8).float()
    phar1 = {'x': x, 'one_hot': oh, 'size': torch.tensor([3], device='cuda'), 'mask': torch.zeros(3, dtype=torch.int64, device='cuda')}
    pocket3 = model._pdb_pocket(pdb, 3, ids, None)
    sizes = torch.tensor([len(c0), len(c1), len(c2)], device='cuda')
    allx = torch.tensor([list(xyz) for c in (c0, c1, c2) for _, xyz in c], device='cuda', dtype=torch.float32)
    alloh = torch.nn.functional.one_hot(torch.tensor([names.index(n) for c in (c0, c1, c2) for n, _ in c], device='cuda'), 8).float()
    phar3 = {'x': allx, 'one_hot': alloh, 'size': sizes, 'mask': torch.repeat_interleave(torch.arange(3, device='cuda'), sizes)}
    in_batch = model.ddpm.score(phar3, pocket3, timesteps=10, seed=5, return_levels=True)
    assert torch.equal(in_batch['nll'], out['nll'])
    alone = model.ddpm.score(phar1, pocket1, timesteps=10, seed=5, pocket_ids=[0], return_levels=True)
    # the oracle's max |net| at these draws for the bound
    h = model.ddpm.dynamics.hip_handle()
    h.set_layout([3], [int(pocket1['size'][0])])
    noise1 = philox_noise(h, 5, [0], [3], range(11)).cpu().numpy()
    cfg500 = ModelConfig(hidden_nf=64, n_layers=2, timesteps=500)
    p = ref_cpu.to_torch_params(make_state_dict(cfg500, seed=0))
    cpu = lambda d: {k: v.cpu() for k, v in d.items()}
    with torch.no_grad():
        raw = score_ref.score_levels(p, cfg500.as_dict(), cpu(phar1), cpu(pocket1), alone['t_levels'].tolist(), noise1)
    bound = score_ref.error_bound(raw['err'][:10, 0].numpy(), raw['netmax'][:10, 0].numpy(), 3, 11)
    d = np.abs(alone['level_sums'][0, :10, 0, 0].cpu().numpy().astype(np.float64) - in_batch['level_sums'][0, :10, 0, 0].cpu().numpy())
    print(f'candidate alone against in a batch of three: worst |d error| / bound {float((d / bound).max()):.3e}')
    assert (d <= bound).all()


# ---------------------------------------------------------------- 8. refusals
def test_refusals():
    cfg, sd, phar, pocket = score_case()
    nl, npk = phar['size'].numpy(), pocket['size'].numpy()
    args = (dev(phar['x'].numpy()), dev(phar['one_hot'].numpy()), dev(pocket['x'].numpy()), dev(pocket['one_hot'].numpy()))
    h = hip_backend.Handle(cfg.as_dict(), 0)
    h.load_state_dict(sd)
    h.set_layout(nl, npk)
    with pytest.raises(hip_backend.CmdgenError, match=r'levels must be in \[0, 100\]'):
        h.score_chain(*args, [10, 101, 0])
    with pytest.raises(hip_backend.CmdgenError, match='levels must be in'):
        h.score_chain(*args, [-1])
    terms, kl = h.score_chain(*args, [100, 100, 0])            # any order, repeats allowed
    assert torch.isfinite(terms).all() and not torch.equal(terms[0], terms[1])       # two draws of their own
    h.close()
    import dataclasses
    for extra, msg in ((dict(update_pocket_coords=True), 'joint model'), (dict(no_com_projection=True), 'no_com_projection')):
        c2 = dataclasses.replace(cfg, **extra)
        h = hip_backend.Handle(c2.as_dict(), 0)
        h.load_state_dict(make_state_dict(c2, seed=1))
        h.set_layout(nl, npk)
        with pytest.raises(hip_backend.CmdgenError, match=msg):
            h.score_chain(*args, [50, 0])
        h.close()
