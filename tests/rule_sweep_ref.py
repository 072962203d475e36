"""Cases, inputs and oracle results of the tile-rule sweep (test_hip_rule_sweep.py on the GPU, test_rule_sweep_cpu.py without one).

Between 1 and ~300 C-alpha pockets the launch planner (make_plan, csrc/cmdgen_plan.h) changes the kernels of an evaluation about ten times, from
the layout alone.  Every case below is one layout with NO launch option set, and carries the launch the library resolves for it on a 256-CU
device: LAUNCH_KEYS read through Handle.query (the rule table of uniform 44 + 15 samples: regimes from 1, 4, 9, 47, 70, 78, 106, 139, 176 and
278 pockets).  test_rule_sweep_cpu.py asserts the tuples against the planner itself on the CPU, the GPU test where multi_processor_count == 256,
so whoever moves a threshold moves these sizes with it.

Inputs: ragged pockets (make_pockets(B, 'CA', ragged=True, first_index=7000): tile and chunk boundaries fall inside samples, N is rarely a
multiple of a tile) with the phar points inside the pocket (test_hip_properties.eval_inputs' law) or, geometry 'drifted', as one compact body
on the shell 10-14 A from the pocket's centre of mass, where the hop-level dead-work skip removes a real share of the tiles (with the points
scattered over that shell in every direction, half of the pocket nodes are still within a hop of one and no 64-row node tile is dead).

The radius graph is a hard threshold, so a sample with a pair within MARGIN of the cutoff may legitimately differ from the oracle; such samples
are left out of a comparison, PER SAMPLE (edges never cross samples), and the share left out is itself bounded: EVAL_CAP / CHAIN_CAP.
"""
from collections import namedtuple
from dataclasses import replace

import numpy as np
import torch

from bench import bounded_config
from cmdgen_amd.synthetic import make_state_dict, make_pockets
from helpers import pocket_dict

LAUNCH_KEYS = ('edge_mt', 'coord_mt', 'node_mt', 'node64', 'node16w', 'proj_in_coord', 'e128_fused')
CUTOFF = 6.0
MARGIN = 1e-4          # A: a sample with a pair closer than this to the cutoff may be left out
EVAL_CAP = 0.05        # ... but at most this share of a case's samples in one evaluation
CHAIN_CAP = 0.20       # ... and this share over the K + 1 evaluations of a chain
CHAIN_K = 5
FIRST_INDEX = 7000

Case = namedtuple('Case', 'engine kind B ragged n_phar geometry launch')
# engine: 'half' (the default), 'bf3' (option half_engine = 0: three bf16 pieces), 'fp32' (set_gemm_mode(False): the fp32 instruction)
# kind: 'cond' (pocket fixed) | 'joint' (update_pocket_coords)


def case_id(c):
    shape = f'B{c.B}' if c.ragged else f'{c.B}x{c.n_phar}'
    return '-'.join([c.engine, c.kind, shape] + ([c.geometry] if c.geometry != 'inside' else []))


def _c(B, launch, engine='half', kind='cond', ragged=True, n_phar=15, geometry='inside'):
    return Case(engine, kind, B, ragged, n_phar, geometry, launch)


# the regimes of the default engine on 256 CUs: (edge_mt, coord_mt, node_mt, node64, node16w, proj_in_coord, e128_fused)
R1 = (16, 16, 16, 0, 1, 0, 0)            # 16-row tiles everywhere, k_node16w
R4 = (32, 16, 16, 0, 1, 0, 0)            # 32-row full-K messages
R9 = (32, 32, 16, 0, 1, 1, 0)            # ... and coordinate list: k_coord_proj
R47 = (128, 32, 16, 0, 1, 1, 0)          # k_edge128 messages
R70 = (128, 32, 32, 32, 1, 0, 0)         # k_node32p
R78 = (128, 32, 32, 32, 1, 0, 1)         # fused message loop
R106 = (128, 128, 32, 32, 1, 0, 1)       # coordinate list on 128 rows
R139 = (128, 128, 32, 8, 1, 0, 1)        # k_node64e
R176 = (128, 128, 32, 8, 1, 0, 3)        # fused coordinate loop
R278 = (128, 128, 32, 2, 1, 0, 3)        # k_node64d

# (a) both sides of every boundary of the rule table for uniform 44 + 15 samples (4, 9, 47, 70, 78, 106, 139, 176, 278) ...
EVAL_CASES = [_c(1, R1), _c(3, R1), _c(4, R1), _c(8, R9), _c(9, R9), _c(46, R9), _c(47, R47), _c(69, R47), _c(70, R70), _c(77, R70), _c(78, R78),
              _c(105, R106), _c(106, R106), _c(138, R139), _c(139, R139), _c(175, R176), _c(176, R176), _c(277, R278), _c(278, R278)]
# ... and of those these ragged layouts themselves cross (their samples average 45 + 15 nodes, so the estimates cross a little earlier:
# 5, 6, 47, 70, 78, 100, 138, 160, 274)
EVAL_CASES += [_c(5, R4), _c(6, R9), _c(99, R78), _c(100, R106), _c(137, R106), _c(159, R139), _c(160, R176), _c(273, R176), _c(274, R278)]
# the driver's own shape (generate_phars: 20 samples x 3 phar points) and one pocket of it
EVAL_CASES += [_c(20, R4, ragged=False, n_phar=3), _c(1, R1, ragged=False, n_phar=3)]

# (b) phar points 10-14 A from the centre: the dead-work skip drops tiles
DRIFT_CASES = [_c(9, R9, geometry='drifted'), _c(47, R47, geometry='drifted'), _c(70, R70, geometry='drifted'), _c(139, R139, geometry='drifted')]

# (c) the other engines, at the sizes of {3, 8, 24, 53, 64, 93, 139, 209} where their launch changes, and the joint model
ENGINE_CASES = [
    _c(3, (16, 16, 16, 0, 1, 0, 0), 'bf3'), _c(24, (32, 16, 16, 0, 1, 0, 0), 'bf3'), _c(64, (32, 32, 16, 0, 1, 1, 0), 'bf3'),
    _c(93, (64, 32, 32, 0, 1, 0, 1), 'bf3'), _c(139, (128, 128, 32, 1, 1, 0, 1), 'bf3'), _c(209, (128, 128, 32, 1, 1, 0, 3), 'bf3'),
    _c(3, (16, 16, 16, 0, 1, 0, 0), 'fp32'), _c(24, (32, 16, 16, 0, 1, 0, 0), 'fp32'), _c(64, (32, 32, 16, 0, 1, 0, 0), 'fp32'),
    _c(93, (64, 32, 16, 0, 1, 0, 1), 'fp32'), _c(209, (64, 64, 32, 0, 1, 0, 3), 'fp32'),
]
# (64 pockets: "joint and 128-row messages -> 32-row full-K messages, coordinate list on 128 rows")
JOINT_CASES = [_c(46, (32, 32, 16, 0, 1, 0, 0), kind='joint'), _c(64, (32, 128, 16, 0, 1, 0, 0), kind='joint'),
               _c(80, (32, 128, 32, 32, 1, 0, 3), kind='joint')]

# (d) K = 5 chains through the chain driver, one per regime up to the size the CPU oracle affords (10 s at 106 pockets)
CHAIN_CASES = [_c(3, R1), _c(8, R9), _c(46, R9), _c(70, R70), _c(106, R106), _c(20, R4, ragged=False, n_phar=3)]

ONE_EVALUATION = EVAL_CASES + DRIFT_CASES + ENGINE_CASES + JOINT_CASES


# ----------------------------------------------------------------------------- inputs
def config_of(case):
    cfg = bounded_config(20, 1000)
    return replace(cfg, update_pocket_coords=True) if case.kind == 'joint' else cfg


_SD = {}


def state_dict_of(case):
    if case.kind not in _SD:
        _SD[case.kind] = make_state_dict(config_of(case), seed=0)
    return _SD[case.kind]


def pockets_of(case):
    if case.ragged:
        return make_pockets(case.B, 'CA', ragged=True, first_index=FIRST_INDEX)
    return make_pockets(case.B, 'CA', n_phar=case.n_phar)


def masks_of(pb):
    return np.repeat(np.arange(len(pb.size), dtype=np.int64), pb.num_nodes_phar), pb.mask


def eval_inputs(pb, cfg, seed=12345, geometry='inside'):
    """(xh_phar, xh_pocket, t) of one evaluation.  'inside': test_hip_properties.eval_inputs, draw for draw (uniform in a 5 A ball round the
    pocket's centre of mass); 'drifted': the same points as one compact body on the shell 10-14 A from it."""
    B = len(pb.size)
    rng = np.random.Generator(np.random.PCG64(seed))
    nl = int(pb.num_nodes_phar.sum())
    pm = np.repeat(np.arange(B), pb.num_nodes_phar)
    starts = np.concatenate([[0], np.cumsum(pb.size)[:-1]])
    com = np.add.reduceat(pb.x.astype(np.float64), starts, axis=0) / pb.size[:, None]
    v = rng.normal(size=(nl, 3)); v /= np.linalg.norm(v, axis=1, keepdims=True)
    u = rng.uniform(size=(nl, 1))
    off = v * 5.0 * np.cbrt(u)
    if geometry == 'drifted':
        # the pharmacophore as a compact body (the 'inside' offsets scaled into a 1 A ball) round a centre 13 A from the centre of mass, in a
        # direction of the sample's own: every point lies 12-14 A out, and the far side of the pocket is several hops from all of them
        c = rng.normal(size=(B, 3)); c /= np.linalg.norm(c, axis=1, keepdims=True)
        off = 13.0 * c[pm] + off * (1.0 / 5.0)
    xin = (com[pm] + off).astype(np.float32)
    xh = np.concatenate([xin, rng.normal(size=(nl, cfg.phar_nf)).astype(np.float32)], 1)
    xq = np.concatenate([pb.x, pb.one_hot / cfg.norm_values[1]], 1).astype(np.float32)
    t = rng.uniform(0.05, 0.95, size=B).astype(np.float32)
    return xh, xq, t


# ----------------------------------------------------------------------------- margins
def _sample_pair_gaps(x_phar, x_pocket, masks, cutoff):
    """Per sample: | ||x_i - x_j|| - cutoff | of every pair i < j, float64."""
    pm, qm = (np.asarray(m) for m in masks)
    xp, xq = np.asarray(x_phar, dtype=np.float64), np.asarray(x_pocket, dtype=np.float64)
    # (both masks ascend: a sample's rows are one slice of each)
    B = int(max(pm.max(initial=-1), qm.max(initial=-1))) + 1
    ps, qs = np.searchsorted(pm, np.arange(B + 1)), np.searchsorted(qm, np.arange(B + 1))
    for b in range(B):
        p = np.concatenate([xp[ps[b]:ps[b + 1]], xq[qs[b]:qs[b + 1]]])
        d = np.sqrt(((p[:, None, :] - p[None, :, :]) ** 2).sum(-1))
        yield np.abs(d[np.triu_indices(len(p), k=1)] - cutoff)


def sample_margins(x_phar, x_pocket, masks, cutoff=CUTOFF):
    """[B] float64: per sample the smallest | ||x_i - x_j|| - cutoff | (synthetic.min_cutoff_margin, per sample).  masks = (phar, pocket)."""
    return np.array([g.min() if len(g) else np.inf for g in _sample_pair_gaps(x_phar, x_pocket, masks, cutoff)])


def pairs_under_margin(x_phar, x_pocket, masks, cutoff=CUTOFF, margin=MARGIN):
    """[B] int: per sample the pairs within `margin` of the cutoff - each may add or remove two directed edges."""
    return np.array([int((g < margin).sum()) for g in _sample_pair_gaps(x_phar, x_pocket, masks, cutoff)])


# ----------------------------------------------------------------------------- the oracle, computed once per case
class RecordedForward:
    """ref_cpu.dynamics_forward that keeps the inputs of every evaluation (install it with monkeypatch.setattr(ref_cpu, 'dynamics_forward', ...):
    sample_given_pocket then records the K + 1 evaluations of its chain)."""
    def __init__(self, fn):
        self.fn, self.calls = fn, []

    def __call__(self, p, cfg, xh_phars, xh_residues, t, mask_phars, mask_residues, trace=None):
        self.calls.append(dict(x_phar=xh_phars[:, :3].detach().clone().numpy(), x_pocket=xh_residues[:, :3].detach().clone().numpy(),
                               t=t.detach().clone().numpy(), masks=(mask_phars.numpy().copy(), mask_residues.numpy().copy())))
        return self.fn(p, cfg, xh_phars, xh_residues, t, mask_phars, mask_residues, trace)

    def margins(self, cutoff=CUTOFF):
        """[evaluations, B]"""
        return np.stack([sample_margins(c['x_phar'], c['x_pocket'], c['masks'], cutoff) for c in self.calls])


def _threads():
    torch.set_num_threads(min(16, max(1, torch.get_num_threads())))


_PARAMS, _EVAL, _CHAIN = {}, {}, {}


def params_of(case):
    from oracle import ref_cpu
    if case.kind not in _PARAMS:
        _PARAMS[case.kind] = ref_cpu.to_torch_params(state_dict_of(case))
    return _PARAMS[case.kind]


def eval_margins(case):
    """(inputs, margins [B], pairs under the margin [B]) of a case's checked evaluation - no oracle needed."""
    cfg, pb = config_of(case), pockets_of(case)
    xh, xq, t = eval_inputs(pb, cfg, geometry=case.geometry)
    masks = masks_of(pb)
    return (xh, xq, t), sample_margins(xh[:, :3], xq[:, :3], masks), pairs_under_margin(xh[:, :3], xq[:, :3], masks)


def oracle_evaluation(case):
    """dict(pb, inputs, poison, want_phar, want_pocket, edges, margins, near) - ref_cpu.dynamics_forward, live, fp32 on the CPU.  The engine is
    no part of the key: every engine is compared with the same oracle result."""
    from oracle import ref_cpu
    key = case._replace(engine='', launch=())
    if key not in _EVAL:
        _threads()
        cfg, pb = config_of(case), pockets_of(case)
        (xh, xq, t), margins, near = eval_margins(case)
        pm, qm = masks_of(pb)
        trace = {}
        with torch.no_grad():
            wp, wq = ref_cpu.dynamics_forward(params_of(case), cfg.as_dict(), torch.from_numpy(xh), torch.from_numpy(xq), torch.from_numpy(t[:, None]),
                                              torch.from_numpy(pm), torch.from_numpy(qm), trace=trace)
        _EVAL[key] = dict(pb=pb, inputs=(xh, xq, t), poison=eval_inputs(pb, cfg, seed=54321, geometry=case.geometry), want_phar=wp.numpy(),
                          want_pocket=wq.numpy(), edges=int(len(trace['row'])), margins=margins, near=near, masks=(pm, qm))
    return _EVAL[key]


def chain_noise(case, pb):
    nl = int(pb.num_nodes_phar.sum())
    return torch.randn((CHAIN_K + 2, nl, 11), generator=torch.Generator().manual_seed(FIRST_INDEX + case.B))


def oracle_chain(case, monkeypatch):
    """dict(pb, noise, want [Nl, 11], want_pocket, chain [K + 1 x [Nl, 11]], margins [K + 1, B]) - ref_cpu.sample_given_pocket with K = CHAIN_K on
    injected noise, every evaluation's inputs recorded."""
    from oracle import ref_cpu
    key = case._replace(engine='', launch=())
    if key not in _CHAIN:
        _threads()
        cfg, pb = config_of(case), pockets_of(case)
        noise = chain_noise(case, pb)
        rec = RecordedForward(ref_cpu.dynamics_forward)
        monkeypatch.setattr(ref_cpu, 'dynamics_forward', rec)
        tape = iter(noise)
        with torch.no_grad():
            want, want_p, _, _, chain = ref_cpu.sample_given_pocket(params_of(case), cfg.as_dict(), pocket_dict(pb), pb.num_nodes_phar, timesteps=CHAIN_K,
                                                                   noise=lambda shape: next(tape), return_chain=True)
        monkeypatch.setattr(ref_cpu, 'dynamics_forward', rec.fn)
        assert len(rec.calls) == CHAIN_K + 1
        _CHAIN[key] = dict(pb=pb, noise=noise, want=want.numpy(), want_pocket=want_p.numpy(), chain=[z.numpy() for z in chain], margins=rec.margins(),
                           masks=masks_of(pb))
    return _CHAIN[key]


def kept_samples(margins):
    """[B] bool: the samples every bound applies to - margin >= MARGIN at the evaluation ([B]) or at every evaluation of a chain ([K + 1, B])."""
    m = np.asarray(margins)
    return (m if m.ndim == 1 else m.min(axis=0)) >= MARGIN
