"""Shared helpers of the tests (test infrastructure): golden cases, tolerances, model and trainer builders.  Test modules do not import each
other: a name that two of them need lives here, or in chain_kit.py when it belongs to the GPU chain tests.  Importing this module touches no GPU."""
import json
import os
import re

import numpy as np
import torch

import cmdgen_amd  # noqa: F401  (alias shim)
from cmdgen_amd import hip_backend
from cmdgen_amd.synthetic import ModelConfig, make_state_dict, make_pockets, min_cutoff_margin
from oracle import ref_cpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def load_golden(name):
    with np.load(os.path.join(GOLDEN, name)) as f:
        return {k: f[k] for k in f.files}


def cases_of(g):
    return sorted({k.split('/')[0] for k in g if '/' in k})


def cfg_from_meta(H, L, R, timesteps=500, simple=False):
    return ModelConfig(hidden_nf=int(H), n_layers=int(L), residue_nf=int(R), timesteps=timesteps, no_com_projection=simple)


def masks_from_sizes(pocket_size, num_nodes_phar):
    B = len(pocket_size)
    return (np.repeat(np.arange(B, dtype=np.int64), num_nodes_phar),
            np.repeat(np.arange(B, dtype=np.int64), pocket_size))


def dynamics_case(g, name):
    """-> cfg, numpy state dict, inputs dict for one G2 case."""
    H, L, B, R, seed, gain1, first = [int(v) for v in g[name + '/meta']]
    cfg = cfg_from_meta(H, L, R)
    sd = make_state_dict(cfg, seed=seed, coord_gain=1.0 if gain1 else 1e-3)
    pm, qm = masks_from_sizes(g[name + '/pocket_size'], g[name + '/num_nodes_phar'])
    inp = dict(xh_phar=g[name + '/xh_phar'], xh_pocket=g[name + '/xh_pocket'], t=g[name + '/t'],
               mask_phar=pm, mask_pocket=qm)
    return cfg, sd, inp


def chain_case(g, name):
    H, L, B, R, seed, K, gain1, first = [int(v) for v in g[name + '/meta']]
    cfg = cfg_from_meta(H, L, R, simple=name.startswith('simple'))
    sd = make_state_dict(cfg, seed=seed, coord_gain=1.0 if gain1 else 1e-3)
    rep = 'CA' if R == 20 else 'full-atom'
    ragged = bool(int(g[name + '/ragged']))
    if rep == 'full-atom':
        pb = make_pockets(B, rep, n_pocket_nodes=90, n_phar=9, first_index=first)
    else:
        pb = make_pockets(B, rep, ragged=ragged, n_phar=8, first_index=first)
    return cfg, sd, pb, K


class NoiseTape:
    """Replays recorded Gaussian draws in order (noise-injection interface)."""
    def __init__(self, arr):
        self.arr, self.i = arr, 0

    def __call__(self, shape):
        out = torch.from_numpy(self.arr[self.i].copy())
        assert tuple(out.shape) == tuple(shape)
        self.i += 1
        return out


def rms(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.sqrt(np.mean((a - b) ** 2)))


HIST = np.zeros((30, 70), dtype=np.float64)
for _i in range(3, 26):
    for _j in range(20, 66):
        HIST[_i, _j] = 1 + ((_i * 7 + _j * 3) % 11)       # the histogram make_golden.py uses


def loss_case(g):
    H, L, B, R, seed, first = [int(v) for v in g['meta']]
    cfg = cfg_from_meta(H, L, R)
    sd = make_state_dict(cfg, seed=seed, coord_gain=1.0)
    pb = make_pockets(B, 'CA', ragged=True, first_index=first)
    nl = g['num_nodes_phar']
    phar = {'x': torch.from_numpy(g['phar_x'].copy()), 'one_hot': torch.from_numpy(g['phar_one_hot'].copy()),
            'size': torch.from_numpy(nl.copy()), 'mask': torch.from_numpy(np.repeat(np.arange(B), nl))}
    pocket = {'x': torch.from_numpy(pb.x.copy()), 'one_hot': torch.from_numpy(pb.one_hot.copy()),
              'size': torch.from_numpy(pb.size.copy()), 'mask': torch.from_numpy(pb.mask.copy())}
    return cfg, sd, phar, pocket, HIST


# ---------------------------------------------------------------- joint model (G9)
class JointNoiseTape:
    """Replays packed combined draws ([D, Nl*(3+P) + Np*(3+R)], make_golden_joint.pack_draws) as the
    three randn calls the reference makes per combined draw: x [Nl+Np,3], h_phar [Nl,P], h_pocket [Np,R]."""
    def __init__(self, arr, Nl, Np, P=8, R=20):
        self.arr, self.Nl, self.Np, self.P, self.R = arr, Nl, Np, P, R
        self.i = 0          # combined draws consumed
        self.sub = 0

    def __call__(self, shape):
        row = self.arr[self.i]
        a = row[:self.Nl * (3 + self.P)].reshape(self.Nl, 3 + self.P)
        b = row[self.Nl * (3 + self.P):].reshape(self.Np, 3 + self.R)
        out = [np.concatenate([a[:, :3], b[:, :3]]), a[:, 3:], b[:, 3:]][self.sub]
        assert tuple(out.shape) == tuple(shape), (out.shape, shape)
        self.sub += 1
        if self.sub == 3:
            self.sub, self.i = 0, self.i + 1
        return torch.from_numpy(np.ascontiguousarray(out))


def joint_cfg(H, L, R=20, timesteps=500):
    return ModelConfig(hidden_nf=int(H), n_layers=int(L), residue_nf=int(R), timesteps=timesteps,
                       update_pocket_coords=True)


def joint_cases(g, kind):
    return sorted({k.split('/')[1] for k in g if k.startswith(kind + '/')})


def joint_inpaint_case(g, name):
    H, L, B, R, seed, K, resamplings, jump, first = [int(v) for v in g[f'inpaint/{name}/meta']]
    cfg = joint_cfg(H, L, R)
    sd = make_state_dict(cfg, seed=seed, coord_gain=1.0)
    pb = make_pockets(B, 'CA', ragged=True, first_index=first)
    nl = pb.num_nodes_phar
    phar = {'x': g[f'inpaint/{name}/phar_x'], 'one_hot': g[f'inpaint/{name}/phar_one_hot'],
            'size': nl, 'mask': np.repeat(np.arange(B, dtype=np.int64), nl)}
    pocket = {'x': pb.x, 'one_hot': pb.one_hot, 'size': pb.size, 'mask': pb.mask}
    return cfg, sd, phar, pocket, K, resamplings, jump


def joint_loss_case(g):
    H, L, B, R, seed, first = [int(v) for v in g['loss/meta']]
    cfg = joint_cfg(H, L, R)
    sd = make_state_dict(cfg, seed=seed, coord_gain=1.0)
    pb = make_pockets(B, 'CA', ragged=True, first_index=first)
    nl = g['loss/num_nodes_phar']
    phar = {'x': torch.from_numpy(g['loss/phar_x'].copy()), 'one_hot': torch.from_numpy(g['loss/phar_one_hot'].copy()),
            'size': torch.from_numpy(nl.copy()), 'mask': torch.from_numpy(np.repeat(np.arange(B), nl))}
    pocket = {'x': torch.from_numpy(g['loss/pocket_x'].copy()), 'one_hot': torch.from_numpy(pb.one_hot.copy()),
              'size': torch.from_numpy(pb.size.copy()), 'mask': torch.from_numpy(pb.mask.copy())}
    return cfg, sd, phar, pocket, HIST


LOSS_NAMES = ['delta_log_px', 'error_t_phar', 'error_t_pocket', 'SNR_weight', 'loss_0_x_phar', 'loss_0_x_pocket',
              'loss_0_h', 'neg_log_constants', 'kl_prior', 'log_pN', 't_int', 'xh_phar_hat']


# ---------------------------------------------------------------- round-2 goldens (make_golden_r2.py)
def bounded_case(g, name):
    """G13: chains of a model with noise_precision 0.05 / norm_values [1, 0.5] (|x| stays O(10 A))."""
    H, L, B, R, seed, K, gain1, first, T = [int(v) for v in g[name + '/meta']]
    cfg = ModelConfig(hidden_nf=H, n_layers=L, residue_nf=R, timesteps=T, noise_precision=float(g[name + '/noise_precision']),
                      norm_values=tuple(float(v) for v in g[name + '/norm_values']))
    sd = make_state_dict(cfg, seed=seed, coord_gain=1.0 if gain1 else 1e-3)
    pb = make_pockets(B, 'CA', ragged=bool(int(g[name + '/ragged'])), n_phar=8, first_index=first)
    return cfg, sd, pb, K


def fullsize_chain_case(g, name='chain_fa366_K5'):
    """G12: BASELINE configs[4]'s real shape - 366 full-atom pocket atoms + 15 phar points per sample."""
    H, L, B, R, seed, K, gain1, first = [int(v) for v in g[name + '/meta']]
    cfg = cfg_from_meta(H, L, R)
    sd = make_state_dict(cfg, seed=seed, coord_gain=1.0 if gain1 else 1e-3)
    pb = make_pockets(B, 'full-atom', n_phar=15, first_index=first)
    return cfg, sd, pb, K


def g5_case(g):
    H, L, B, R, seed, gain1, first = [int(v) for v in g['meta']]
    cfg = cfg_from_meta(H, L, R)
    sd = make_state_dict(cfg, seed=seed, coord_gain=1.0 if gain1 else 1e-3)
    pm, qm = masks_from_sizes(g['pocket_size'], g['num_nodes_phar'])
    inp = dict(xh_phar=g['xh_phar'], xh_pocket=g['xh_pocket'], t=g['t'], mask_phar=pm, mask_pocket=qm)
    return cfg, sd, inp


def pocket_dict(pb):
    return {'x': torch.from_numpy(pb.x), 'one_hot': torch.from_numpy(pb.one_hot),
            'size': torch.from_numpy(pb.size), 'mask': torch.from_numpy(pb.mask)}


def _hparams(rep, H, L):
    from argparse import Namespace
    return dict(outdir='out', dataset='crossdock' if rep == 'CA' else 'crossdock_full', datadir='data', batch_size=4, lr=1e-4,
                egnn_params=Namespace(device='cpu', edge_cutoff=6.0, joint_nf=32, hidden_nf=H, n_layers=L, attention=True,
                                      tanh=True, norm_constant=1, inv_sublayers=1, sin_embedding=False,
                                      aggregation_method='sum', normalization_factor=100),
                diffusion_params=Namespace(diffusion_steps=500, diffusion_noise_schedule='polynomial_2',
                                           diffusion_noise_precision=1e-5, diffusion_loss_type='l2', normalize_factors=[1, 4]),
                num_workers=0, augment_noise=0, augment_rotation=False, clip_grad=True, eval_epochs=50,
                eval_params=Namespace(n_eval_samples=100, eval_batch_size=100), mode='pocket_conditioning',
                node_histogram=HIST, pocket_representation=rep)


# ---------------------------------------------------------------- scoring (G21, make_golden_score.py)
SCORE_CASES = ['K100', 'K20']
SCORE_BAND = 1e-4          # A: a (level, sample) entry with a pair closer than this to the cutoff is left out of a comparison
_G21 = []


def g21():
    if not _G21:
        _G21.append(load_golden('g21_score.npz'))
    return _G21[0]


def score_case(g=None):
    """-> cfg, numpy state dict, phar, pocket (torch dicts) of the G21 complexes (those of G6, timesteps = 100)."""
    H, L, B, R, seed, first, T = [int(v) for v in (g21() if g is None else g)['meta']]
    g6 = load_golden('g6_loss.npz')
    cfg = ModelConfig(hidden_nf=H, n_layers=L, residue_nf=R, timesteps=T)
    sd = make_state_dict(cfg, seed=seed, coord_gain=1.0)
    pb = make_pockets(B, 'CA', ragged=True, first_index=first)
    nl = g6['num_nodes_phar']
    phar = {'x': torch.from_numpy(g6['phar_x'].copy()), 'one_hot': torch.from_numpy(g6['phar_one_hot'].copy()),
            'size': torch.from_numpy(nl.copy()), 'mask': torch.from_numpy(np.repeat(np.arange(B), nl))}
    pocket = {'x': torch.from_numpy(pb.x.copy()), 'one_hot': torch.from_numpy(pb.one_hot.copy()),
              'size': torch.from_numpy(pb.size.copy()), 'mask': torch.from_numpy(pb.mask.copy())}
    return cfg, sd, phar, pocket


def close(got, want):
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    return np.allclose(got, want, rtol=2e-5, atol=2e-5 * max(1.0, float(np.abs(want).max())))


# ---------------------------------------------------------------- the GPU evaluation tests (nothing here touches the GPU at import)
EVAL_TOL = 2e-5


def new_handle(cfg, sd):
    h = hip_backend.Handle(cfg.as_dict(), 0)
    h.load_state_dict(sd)
    return h


def host_step_table(cfg, K):
    """Per-step scalars evaluated exactly as the reference does (bit-identical table, oracle-side helper)."""
    from oracle import ref_cpu
    table = ref_cpu.gamma_table(cfg.noise_schedule, cfg.timesteps, cfg.noise_precision)
    coef = ref_cpu.step_coefficients(table, cfg.timesteps, K).numpy()
    g0 = table[0]
    final = np.array([[float(torch.sqrt(torch.sigmoid(g0))), float(torch.sqrt(torch.sigmoid(-g0))),
                       float(torch.exp(0.5 * g0)), 0.0]], np.float32)
    return np.concatenate([coef, final])


def small_case(seed=91, B=3, K=4):
    cfg = ModelConfig(hidden_nf=64, n_layers=2, timesteps=500)
    sd = make_state_dict(cfg, seed=seed, coord_gain=1e-3)
    pb = make_pockets(B, 'CA', ragged=True, n_phar=8, first_index=100 * seed)
    Nl = int(pb.num_nodes_phar.sum())
    noise = np.random.Generator(np.random.PCG64(seed)).normal(size=(K + 2, Nl, 11)).astype(np.float32)
    return cfg, sd, pb, K, noise


CHAIN_BAND = 2e-5   # a pair this close to the cutoff may be decided differently by torch.cdist's matmul form (quirk Q2): its
                    # rounding at |x| ~ 17 A is ~5e-6 A in d, ours (direct fma chain) ~1e-6 A


def eval_inputs(pb, cfg, seed=12345):
    """Phar points inside the pocket (the geometry a trained model holds: every pocket node within a few hops of a moving node)."""
    B = len(pb.size)
    rng = np.random.Generator(np.random.PCG64(seed))
    nl = int(pb.num_nodes_phar.sum())
    pm = np.repeat(np.arange(B), pb.num_nodes_phar)
    starts = np.concatenate([[0], np.cumsum(pb.size)[:-1]])
    com = np.add.reduceat(pb.x.astype(np.float64), starts, axis=0) / pb.size[:, None]
    v = rng.normal(size=(nl, 3)); v /= np.linalg.norm(v, axis=1, keepdims=True)
    xin = (com[pm] + v * 5.0 * np.cbrt(rng.uniform(size=(nl, 1)))).astype(np.float32)
    xh = np.concatenate([xin, rng.normal(size=(nl, cfg.phar_nf)).astype(np.float32)], 1)
    xq = np.concatenate([pb.x, pb.one_hot / cfg.norm_values[1]], 1).astype(np.float32)
    t = rng.uniform(0.05, 0.95, size=B).astype(np.float32)
    return xh, xq, t


def handle_with_layout(cfg, sd, pb):
    h = hip_backend.Handle(cfg.as_dict(), 0)
    h.load_state_dict(sd)
    h.set_layout(pb.num_nodes_phar, pb.size)
    return h


def forward(h, xh, xq, t):
    eps, _ = h.dynamics_forward(torch.from_numpy(xh).cuda(), torch.from_numpy(xq).cuda(), torch.from_numpy(t).cuda())
    return eps.cpu().numpy()

G7_RUNS = [('ca_ids', 'CA', dict(pocket_ids=True)), ('ca_lig', 'CA', dict(ref_ligand='B:501')),
           ('ca_pep', 'CA', dict(ref_ligand='B:601')), ('fa_ids', 'full-atom', dict(pocket_ids=True))]


def g7_select(g, tag, sel):
    return {'pocket_ids': [str(s) for s in g[tag + '/pocket_ids']]} if sel.get('pocket_ids') else dict(sel)


def assert_same_result(out, want_json, atol):
    want = json.loads(want_json)
    assert list(out) == list(want)                                     # Molecule_k keys in creation order (Q9)
    for m in want:
        assert list(out[m]) == list(want[m]), m                        # type names in first-seen order
        for t in want[m]:
            a = np.asarray([[float(v) for v in c] for c in out[m][t]])
            b = np.asarray(want[m][t])
            assert a.shape == b.shape and np.abs(a - b).max() <= atol, (m, t)


_G14 = []


def g14():
    """G14: configs[1] / configs[4] at their literal size."""
    if not _G14:
        _G14.append(load_golden('g14_fullsize_chains.npz'))
    return _G14[0]


def g14_case(name):
    G14 = g14()
    H, L, B, R, seed, K, T, first, nseed, window = [int(v) for v in G14[name + '/meta']]
    cfg = ModelConfig(hidden_nf=H, n_layers=L, residue_nf=R, timesteps=T, noise_precision=float(G14[name + '/noise_precision']),
                      norm_values=tuple(float(v) for v in G14[name + '/norm_values']))
    sd = make_state_dict(cfg, seed=seed, coord_gain=1.0)
    pb = make_pockets(B, 'CA' if R == 20 else 'full-atom', n_phar=15, first_index=first)
    Nl = int(pb.num_nodes_phar.sum())
    gen = torch.Generator().manual_seed(nseed)                       # the reference's draws, regenerated (42 MB for K = 1000: not stored)
    noise = torch.stack([torch.randn((Nl, 11), generator=gen) for _ in range(K + 2)])
    probe = G14[name + '/noise_probe']
    assert np.array_equal(noise[0, :4].numpy(), probe[0]) and np.array_equal(noise[K + 1, :4].numpy(), probe[1]), \
        'torch.Generator stream differs from the one the golden was made with'
    return cfg, sd, pb, K, window, noise


def per_sample_rms(a, b, B):
    d = (np.asarray(a, np.float64) - np.asarray(b, np.float64)).reshape(B, -1, a.shape[-1])
    return np.sqrt((d ** 2).mean((1, 2)))


# ---------------------------------------------------------------- the training and autograd tests
GRAD_TOL = 2e-4


def make_handle(cfg):
    return hip_backend.Handle(cfg.as_dict(), 0)


def flat_theta(h, sd):
    theta = torch.zeros(h.param_count(), dtype=torch.float32)
    for k, v in sd.items():
        name = k[len('ddpm.dynamics.'):] if k.startswith('ddpm.dynamics.') else None
        if name is None:
            continue
        off, cnt = h.param_offset(name)
        assert cnt == v.size
        theta[off:off + cnt] = torch.from_numpy(v.reshape(-1))
    return theta.cuda()


def case_inputs(cfg, B, first, rng, spread=3.0):
    while True:
        pb = make_pockets(B, 'CA', ragged=True, first_index=first)
        nl = pb.num_nodes_phar
        pm = np.repeat(np.arange(B), nl)
        com = np.stack([pb.x[pb.mask == b].mean(0) for b in range(B)])
        xp = (com[pm] + rng.normal(size=(len(pm), 3)) * spread).astype(np.float32)
        if min_cutoff_margin(np.concatenate([xp, pb.x]), np.concatenate([pm, pb.mask]), 6.0) > 2e-3:
            break
        first += 13
    xh_phar = np.concatenate([xp, rng.normal(size=(len(pm), cfg.phar_nf)).astype(np.float32)], 1)
    xh_pocket = np.concatenate([pb.x, pb.one_hot / cfg.norm_values[1]], 1).astype(np.float32)
    t = rng.uniform(size=(B, 1)).astype(np.float32)
    return pb, pm, xh_phar, xh_pocket, t


def build_trainer(lr=1e-3, inv_sublayers=1, aggregation_method='sum'):
    from argparse import Namespace
    from cmdgen_amd.lightning_modules import PharPocketDDPM
    from cmdgen_amd.training import HipTrainer
    g6 = load_golden('g6_loss.npz')
    cfg, sd, phar, pocket, hist = loss_case(g6)
    if inv_sublayers != 1 or aggregation_method != 'sum':
        import dataclasses
        cfg = dataclasses.replace(cfg, inv_sublayers=inv_sublayers, aggregation_method=aggregation_method)
        sd = make_state_dict(cfg, seed=int(g6['meta'][4]), coord_gain=1.0)
    hp = dict(outdir='out', dataset='crossdock', datadir='data', batch_size=4, lr=lr,
              egnn_params=Namespace(device='cuda', edge_cutoff=6.0, joint_nf=32, hidden_nf=cfg.hidden_nf,
                                    n_layers=cfg.n_layers, attention=True, tanh=True, norm_constant=1, inv_sublayers=inv_sublayers,
                                    sin_embedding=False, aggregation_method=aggregation_method, normalization_factor=100),
              diffusion_params=Namespace(diffusion_steps=500, diffusion_noise_schedule='polynomial_2',
                                         diffusion_noise_precision=1e-5, diffusion_loss_type='l2',
                                         normalize_factors=[1, 4]),
              num_workers=0, augment_noise=0, augment_rotation=False, clip_grad=True, eval_epochs=50,
              eval_params=Namespace(n_eval_samples=100, eval_batch_size=100), mode='pocket_conditioning',
              node_histogram=hist, pocket_representation='CA')
    model = PharPocketDDPM(**hp)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    model = model.cuda()
    data = {'phar_coords': phar['x'], 'phar_one_hot': phar['one_hot'], 'num_phar_atoms': phar['size'],
            'phar_mask': phar['mask'], 'pocket_c_alpha': pocket['x'], 'pocket_one_hot': pocket['one_hot'],
            'num_pocket_nodes': pocket['size'], 'pocket_mask': pocket['mask']}
    return model, HipTrainer(model), data, g6


def _bench_trainer(B, pipelined=False, sd_edit=None, lr=1e-3):
    """PharPocketDDPM (shipped hyper-parameters, seeded weights) + HipTrainer + one synthetic batch of B ragged C-alpha complexes (tools/bench_train.py)."""
    import importlib.util, os
    spec = importlib.util.spec_from_file_location('bench_train', os.path.join(os.path.dirname(__file__), '..', 'tools', 'bench_train.py'))
    bt = importlib.util.module_from_spec(spec); spec.loader.exec_module(bt)
    cfg, model, tr = bt.build_trainer(B, 'CA', 'fp32', torch.device('cuda', 0), pipelined=pipelined)
    sd = make_state_dict(cfg, seed=0)
    if sd_edit is not None:
        sd = sd_edit(dict(sd))
        model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
        tr = bt.HipTrainer(model, gemm_dtype='fp32')
        tr.pipelined = pipelined
    tr.lr = lr
    return cfg, sd, model, tr, bt


def make_module(cfg, sd):
    from cmdgen_amd.equivariant_diffusion.dynamics import EGNNDynamics
    c = cfg.as_dict()
    dyn = EGNNDynamics(phar_nf=c['phar_nf'], residue_nf=c['residue_nf'], n_dims=3, joint_nf=c['joint_nf'], hidden_nf=c['hidden_nf'],
                       n_layers=c['n_layers'], attention=c['attention'], tanh=c['tanh'], norm_constant=c['norm_constant'],
                       inv_sublayers=c.get('inv_sublayers', 1), sin_embedding=False, normalization_factor=c['normalization_factor'],
                       aggregation_method=c.get('aggregation_method', 'sum'), update_pocket_coords=c['update_pocket_coords'],
                       edge_cutoff=c['edge_cutoff'], condition_time=c['condition_time'])
    state = {k[len('ddpm.dynamics.'):]: torch.from_numpy(np.asarray(v)) for k, v in sd.items() if k.startswith('ddpm.dynamics.')}
    dyn.load_state_dict(state)
    return dyn.cuda()


def autograd_case(H, L, B, seed, **kw):
    cfg = ModelConfig(hidden_nf=H, n_layers=L, **kw)
    sd = make_state_dict(cfg, seed=seed, coord_gain=1.0)
    rng = np.random.Generator(np.random.PCG64(seed))
    pb, pm, xh_phar, xh_pocket, t = case_inputs(cfg, B, 700000 + seed, rng)
    g = rng.normal(size=xh_phar.shape).astype(np.float32)
    gq = rng.normal(size=xh_pocket.shape).astype(np.float32)
    return cfg, sd, dict(xh_phar=xh_phar, xh_pocket=xh_pocket, t=t, mask_phar=pm.astype(np.int64), mask_pocket=pb.mask.astype(np.int64)), g, gq


def hip_grads(dyn, inp, g, gq, with_pocket):
    """autograd through the module in differentiable mode -> (eps, {input: grad}, {param name: grad})"""
    dyn.set_differentiable(True)
    xp, xq, t = (dev(inp[k]).requires_grad_(True) for k in ('xh_phar', 'xh_pocket', 't'))
    eps, eps_q = dyn(xp, xq, t, dev(inp['mask_phar']), dev(inp['mask_pocket']))
    assert eps.grad_fn is not None
    loss = (eps * dev(g)).sum() + ((eps_q * dev(gq)).sum() if with_pocket else 0.0)
    names = [n for n, _ in dyn.named_parameters()]
    gr = torch.autograd.grad(loss, [xp, xq, t] + list(dyn.parameters()), allow_unused=True)
    return eps.detach(), dict(zip(('xh_phar', 'xh_pocket', 't'), gr[:3])), dict(zip(names, gr[3:]))


def oracle_grads(cfg, sd, inp, g, gq, with_pocket):
    p = ref_cpu.to_torch_params(sd)
    leaves = {k: v.clone().requires_grad_(True) for k, v in p.items() if k.startswith('dynamics.')}
    p2 = dict(p); p2.update(leaves)
    xs = {k: torch.from_numpy(inp[k].copy()).requires_grad_(True) for k in ('xh_phar', 'xh_pocket', 't')}
    eps, eps_q = ref_cpu.dynamics_forward(p2, cfg.as_dict(), xs['xh_phar'], xs['xh_pocket'], xs['t'],
                                          torch.from_numpy(inp['mask_phar']), torch.from_numpy(inp['mask_pocket']))
    loss = (eps * torch.from_numpy(g)).sum() + ((eps_q * torch.from_numpy(gq)).sum() if with_pocket else 0.0)
    loss.backward()
    return eps.detach(), {k: v.grad for k, v in xs.items()}, {k[len('dynamics.'):]: v.grad for k, v in leaves.items()}


def assert_close(got, want, tol, what):
    want = np.zeros_like(got) if want is None else np.asarray(want, dtype=np.float64)
    scale = max(float(np.abs(want).max()), 1e-6)
    err = float(np.abs(np.asarray(got, dtype=np.float64) - want).max())
    assert err <= tol * scale, (what, err, scale)


def npy(x):
    return None if x is None else x.detach().cpu().numpy()


def check_against_oracle(cfg, sd, inp, g, gq, with_pocket, dyn=None, inputs=True):
    dyn = make_module(cfg, sd) if dyn is None else dyn
    eps, gi, gp = hip_grads(dyn, inp, g, gq, with_pocket)
    want_eps, wi, wp = oracle_grads(cfg, sd, inp, g, gq, with_pocket)
    assert np.abs(npy(eps) - want_eps.numpy()).max() <= 2e-5 * max(1.0, float(want_eps.abs().max()))
    for k, v in gp.items():
        assert_close(npy(v), npy(wp[k]), GRAD_TOL, k)
    if inputs:
        for k in ('xh_phar', 'xh_pocket', 't'):
            assert_close(npy(gi[k]), npy(wi[k]), GRAD_TOL, k)
        assert float(gi['xh_pocket'][:, :3].abs().max()) > 0          # static pocket rows carry a position gradient too
    return dyn, gi, gp


# ---------------------------------------------------------------- the half engine's range: G2's ca_h256_b8 with the first layer of one MLP scaled
RANGE_NAME = 'ca_h256_b8'
OVERFLOW_FACTOR = 3.0e6           # first-layer gain: the hidden activation of the targeted MLP reaches ~1e5 ... 1e6 (> 65504, far below fp32's 3e38)
# which first layer is scaled -> which kernel's A operand (the SiLU output feeding the second layer) overflows first
RANGE_TARGETS = {
    'msg': 'ddpm.dynamics.egnn.e_block_1.gcl_0.edge_mlp.0',            # GCL.edge_model           (egnn_new.py:31-42)
    'coord': 'ddpm.dynamics.egnn.e_block_1.gcl_equiv.coord_mlp.0',     # EquivariantUpdate        (egnn_new.py:87-96)
    'node': 'ddpm.dynamics.egnn.e_block_1.gcl_0.node_mlp.0',           # GCL.node_model           (egnn_new.py:48-58)
}
_G2 = []


def g2():
    if not _G2:
        _G2.append(load_golden('g2_dynamics.npz'))
    return _G2[0]


def overflow_case(target):
    cfg, sd, inp = dynamics_case(g2(), RANGE_NAME)
    sd = dict(sd)
    for suffix in ('.weight', '.bias'):
        sd[RANGE_TARGETS[target] + suffix] = (sd[RANGE_TARGETS[target] + suffix] * OVERFLOW_FACTOR).astype(np.float32)
    return cfg, sd, inp


def underflow_case(target, s):
    """The targeted first layer's weight and bias times s, the matching second layer's weight times 1 / s: the half GEMM's A operand
    (SiLU of the first layer) sits at scale s, the evaluation's output stays O(1)."""
    cfg, sd, inp = dynamics_case(g2(), RANGE_NAME)
    sd = dict(sd)
    first = RANGE_TARGETS[target]
    second = first[:-len('.0')] + '.2.weight'
    for key in (first + '.weight', first + '.bias'):
        sd[key] = (sd[key] * np.float32(s)).astype(np.float32)
    sd[second] = (sd[second] * np.float32(1.0 / s)).astype(np.float32)
    return cfg, sd, inp


# ---------------------------------------------------------------- the CPU tests of the derived chains
_G20 = []


def g20():
    if not _G20:
        _G20.append(load_golden('g20_cond_inpaint.npz'))
    return _G20[0]


def g20_oracle_case(name):
    """-> cfg, oracle params, pocket batch, phar dict, fixed mask, (K, resamplings, jump_length)."""
    G20 = g20()
    H, L, B, R, seed, K, r, j, first = [int(v) for v in G20[name + '/meta']]
    cfg = cfg_from_meta(H, L, R)
    p = ref_cpu.to_torch_params(make_state_dict(cfg, seed=seed, coord_gain=1.0))
    pb = make_pockets(B, 'CA', ragged=True, n_phar=7, first_index=first)
    phar = {'x': torch.from_numpy(G20[name + '/phar_x']), 'one_hot': torch.from_numpy(G20[name + '/phar_one_hot']),
            'size': torch.from_numpy(pb.num_nodes_phar), 'mask': torch.from_numpy(np.repeat(np.arange(B), pb.num_nodes_phar))}
    return cfg, p, pb, phar, G20[name + '/phar_fixed'], (K, r, j)


def bare_model(cls):
    """An untrained ConditionalDDPM-like model of class cls for host-side argument checks."""
    from cmdgen_amd.equivariant_diffusion.dynamics import EGNNDynamics
    dyn = EGNNDynamics(phar_nf=8, residue_nf=20, n_dims=3, joint_nf=16, hidden_nf=64, n_layers=1, update_pocket_coords=False)
    return cls(dynamics=dyn, phar_nf=8, residue_nf=20, n_dims=3, timesteps=50, noise_schedule='polynomial_2',
               noise_precision=1e-5, loss_type='l2', norm_values=[1, 4], size_histogram=np.ones((30, 70)))


def bare_inputs():
    phar = {'x': torch.zeros(5, 3), 'one_hot': torch.zeros(5, 8), 'size': torch.tensor([2, 3]), 'mask': torch.tensor([0, 0, 1, 1, 1])}
    pocket = {'x': torch.randn(7, 3), 'one_hot': torch.zeros(7, 20), 'size': torch.tensor([3, 4]),
              'mask': torch.tensor([0, 0, 0, 1, 1, 1, 1])}
    return phar, pocket


_SMALL = {}


def small():
    """A small model of the bounded config (the CPU tests need the chain's arithmetic, not the width)."""
    if not _SMALL:
        from dataclasses import replace
        import multi_pocket_cases as mc
        cfg = replace(mc.config(), hidden_nf=64, n_layers=2)
        _SMALL.update(cfg=cfg, p=ref_cpu.to_torch_params(make_state_dict(cfg, seed=3)))
    return _SMALL['cfg'], _SMALL['p']


def sub_pockets(pb, members):
    """The pocket dict of the listed samples of pb, in that order."""
    xs, hs = np.split(pb.x, np.cumsum(pb.size)[:-1]), np.split(pb.one_hot, np.cumsum(pb.size)[:-1])
    size = pb.size[list(members)]
    return {'x': torch.from_numpy(np.concatenate([xs[b] for b in members])), 'one_hot': torch.from_numpy(np.concatenate([hs[b] for b in members])),
            'size': torch.from_numpy(size), 'mask': torch.from_numpy(np.repeat(np.arange(len(size)), size))}


# ---------------------------------------------------------------- host-side pieces that more than one test file uses
PDB_TEXT = """\
ATOM      1  CA  ALA A   1      11.639   6.071  -5.147  1.00  0.00           C
ATOM      2  CA  GLY A   2      14.000   7.500  -3.000  1.00  0.00           C
ATOM      3  CA  TRP A   3      16.500   9.000  -1.000  1.00  0.00           C
ATOM      4  CA  LEU A   4      12.500   9.500  -2.000  1.00  0.00           C
ATOM      5  CA  SER A   5      10.000   8.000   0.500  1.00  0.00           C
ATOM      6  CA  ASP A   6      13.500   4.000  -1.500  1.00  0.00           C
END
"""


def tau_from_header():
    text = open(os.path.join(os.path.dirname(GOLDEN), '..', 'cmdgen_amd', 'csrc', 'cmdgen_split.h')).read()
    m = re.search(r'#define\s+HALF_LOW_TAU\s+([0-9.eE+-]+)f', text)
    assert m, 'HALF_LOW_TAU not found in cmdgen_split.h'
    return float(m.group(1))


def small_ddpm(H=64, L=2, T=500):
    from cmdgen_amd.equivariant_diffusion.dynamics import EGNNDynamics
    from cmdgen_amd.equivariant_diffusion.conditional_model import ConditionalDDPM
    dyn = EGNNDynamics(phar_nf=8, residue_nf=20, n_dims=3, joint_nf=32, hidden_nf=H, n_layers=L, attention=True,
                       tanh=True, norm_constant=1, inv_sublayers=1, sin_embedding=False, normalization_factor=100,
                       aggregation_method='sum', edge_cutoff=6.0, update_pocket_coords=False)
    return ConditionalDDPM(dynamics=dyn, phar_nf=8, residue_nf=20, n_dims=3, timesteps=T,
                           noise_schedule='polynomial_2', noise_precision=1e-5, loss_type='l2',
                           norm_values=[1, 4], size_histogram=np.ones((30, 70)))


def host_hparams(H=64, L=1):
    from argparse import Namespace
    return dict(outdir='out', dataset='crossdock', datadir='data', batch_size=4, lr=1e-4,
                egnn_params=Namespace(device='cuda', edge_cutoff=6.0, joint_nf=32, hidden_nf=H, n_layers=L,
                                      attention=True, tanh=True, norm_constant=1, inv_sublayers=1,
                                      sin_embedding=False, aggregation_method='sum', normalization_factor=100),
                diffusion_params=Namespace(diffusion_steps=500, diffusion_noise_schedule='polynomial_2',
                                           diffusion_noise_precision=1e-5, diffusion_loss_type='l2',
                                           normalize_factors=[1, 4]),
                num_workers=0, augment_noise=0, augment_rotation=False, clip_grad=True, eval_epochs=50,
                eval_params=Namespace(n_eval_samples=100, eval_batch_size=100), mode='pocket_conditioning',
                node_histogram=np.ones((30, 70)), pocket_representation='CA')
