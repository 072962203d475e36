"""What the Python wrapper layers hand down, entry by entry, on the CPU: every sampling and scoring entry of ConditionalDDPM against a
recording stand-in for the Handle (which Handle method, the layout, every scalar, every tensor and record array), and every PDB-level
entry of PharPocketDDPM against recording stand-ins for the ConditionalDDPM entries (the pocket dicts, num_nodes_phar, the masks and
start, the per-sample restraint list, the returned structure after the move back).  The expected values are literals: the wrappers may
be reorganised freely, what they pass on may not change.  No library and no GPU are needed."""
import inspect

import numpy as np
import pytest
import torch

from helpers import PDB_TEXT, bare_model, host_hparams
from cmdgen_amd.equivariant_diffusion.conditional_model import ConditionalDDPM
from cmdgen_amd.hip_backend import Handle
from cmdgen_amd.lightning_modules import PharPocketDDPM

P, R, K = 8, 20, 10


# ---------------------------------------------------------------- what is compared: plain Python values
def norm(v):
    """A tensor or array as (dtype, shape, contents): every element, or where that is shorter the non-zero elements [(flat index,
    value)] (the large ones here are sparse by construction).  Record arrays as their tuples; containers element by element."""
    if isinstance(v, torch.Tensor):
        v = v.detach().cpu().numpy()
    if isinstance(v, np.ndarray):
        if v.dtype.names:
            return [norm(list(r)) for r in v.tolist()]
        flat = np.round(v, 4).reshape(-1) if v.dtype.kind == 'f' else v.reshape(-1)
        nz = np.nonzero(flat)[0]
        if flat.size <= 8 or 2 * len(nz) >= flat.size:
            assert flat.size <= 48, 'a large tensor of this test is sparse'
            return (str(v.dtype), list(v.shape), norm(flat.reshape(v.shape).tolist()))
        return (str(v.dtype), list(v.shape), 'nonzero', [(int(i), norm(flat[i].item())) for i in nz])
    if isinstance(v, dict):
        return {k: norm(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [norm(x) for x in v]
    if isinstance(v, (bool, int, str)) or v is None:
        return v
    if isinstance(v, (float, np.floating)):
        return round(float(v), 4)
    if isinstance(v, np.integer):
        return int(v)
    raise TypeError(type(v))


def bound(fn, args, kw, skip=1):
    """The call's arguments by parameter name with the defaults filled in, so that passing by position or by keyword reads the same."""
    names = list(inspect.signature(fn).parameters)[:skip]
    b = inspect.signature(fn).bind(*([None] * skip), *args, **kw)
    b.apply_defaults()
    return {k: v for k, v in b.arguments.items() if k not in names}


# ---------------------------------------------------------------- ConditionalDDPM against a recording Handle
def rows_x(ids):
    """Coordinates that name their row: row id -> (id, id / 2, -id), float64 so that the cast to float32 shows."""
    i = torch.tensor(ids, dtype=torch.float64)
    return torch.stack([i, i / 2, -i], dim=1)


def rows_onehot(ids, nf):
    return torch.nn.functional.one_hot(torch.tensor(ids) % nf, nf).to(torch.float64)


def batch(ids, sizes, nf):
    sizes = torch.tensor(sizes)
    return {'x': rows_x(ids), 'one_hot': rows_onehot(ids, nf), 'size': sizes, 'mask': torch.repeat_interleave(torch.arange(len(sizes)), sizes)}


def inputs():
    phar = batch([1, 2, 3, 4, 5], [2, 3], P)
    pocket = batch([10, 11, 12, 13, 14, 15, 16], [3, 4], R)
    other = batch([100, 101, 102, 103, 104, 105, 106], [2, 5], R)
    return phar, pocket, other


def marked(*shape):
    """An injected noise tensor: float64 zeros with two marked entries."""
    t = torch.zeros(shape, dtype=torch.float64)
    t.view(-1)[3], t.view(-1)[-2] = 1.5, -2.25
    return t


class RecordingHandle:
    """Stands in for hip_backend.Handle: records what it is given and returns CPU tensors of the shapes the library would fill."""

    def __init__(self):
        self.calls, self.last_pocket_steps = [], None

    def set_layout(self, num_phar, num_pocket, on_stream=False):
        self.calls.append(('set_layout', norm(np.asarray(num_phar)), norm(np.asarray(num_pocket)), on_stream))
        self.batch, self.n_phar, self.n_pocket = len(num_phar), int(np.sum(num_phar)), int(np.sum(num_pocket))

    def set_step_table(self, K, coef):
        self.calls.append(('set_step_table', K, list(np.shape(coef))))

    def set_guide_table(self, K, sigma_alpha):
        self.calls.append(('set_guide_table', K, list(np.shape(sigma_alpha))))

    def edit_plan(self, timesteps, start=None, resamplings=1, jump_length=1):
        self.calls.append(('edit_plan', timesteps, start, resamplings, jump_length))
        start = timesteps if start is None else start
        return start * resamplings, start * resamplings + 2

    def chain_status(self):
        self.calls.append(('chain_status',))
        return {'max_rel_com_error': 0.0, 'max_cog': 0.0, 'nan_resets': 0, 'nan_resets_total': 0, 'half_low_range': 0, 'half_low_range_total': 0}

    def run_range_guarded(self, run, status):
        self.calls.append(('run_range_guarded',))
        out = run()
        return out, status()

    def __getattr__(self, name):
        if not name.endswith('_chain'):
            raise AttributeError(name)
        return lambda *a, **kw: self._chain(name, a, kw)

    def _chain(self, name, args, kw):
        a = bound(getattr(Handle, name), args, kw)
        self.calls.append((name, norm(a)))
        groups = len(a['group_sizes']) if 'group_sizes' in a else None
        rows = self.n_phar if groups is None else self.n_phar * groups // self.batch
        owners = self.batch if groups is None else groups
        if 'score' in name:
            n = len(np.asarray(a['t_levels']).reshape(-1))
            terms = (torch.arange(n * owners * 4, dtype=torch.float32).reshape(n, owners, 4) + 1) / 64
            terms[..., 3] = 0                                            # (no reset)
            kl = (torch.arange(owners * 2, dtype=torch.float32).reshape(owners, 2) + 1) / 8
            if groups is None:
                return terms, kl
            members = None
            if a['want_members']:
                members = (torch.arange(n * self.batch * 4, dtype=torch.float32).reshape(n, self.batch, 4) + 1) / 128
                members[..., 3] = 0
            return terms, members, kl
        if 'edit' in name or 'inpaint' in name:
            steps = (a['timesteps'] if a.get('start') is None else a['start']) * a['resamplings']
        else:
            steps = a['timesteps']
        xh_phar = torch.arange(rows * (3 + P), dtype=torch.float32).reshape(rows, 3 + P)
        xh_pocket = torch.cat([a['pocket_x'], a['pocket_onehot']], dim=1)         # (the pocket rows come back as they went in)
        z_steps = None
        if a['want_steps']:
            z_steps = torch.arange(steps, dtype=torch.float32)[:, None, None] + xh_phar[None] / 1000
            self.last_pocket_steps = torch.arange(steps, dtype=torch.float32)[:, None, None] + a['pocket_x'][None]
        out = (xh_phar, xh_pocket, z_steps)
        if 'restrained' in name:
            out += (torch.arange(owners * 2, dtype=torch.float32).reshape(owners, 2) / 4,
                    torch.arange(steps * owners, dtype=torch.float32).reshape(steps, owners) if a['want_steps'] else None)
        if 'diverse' in name:
            out += (torch.arange(owners, dtype=torch.float32) / 4,
                    torch.arange(steps * owners, dtype=torch.float32).reshape(steps, owners) if a['want_steps'] else None)
        return out


RESTRAINTS = [{'kind': 'position', 'sample': 0, 'point': 1, 'center': (1.0, 2.0, 3.0), 'radius': 1.5, 'k': 2.0},
              {'kind': 'distance', 'sample': 1, 'points': (0, 2), 'lo': 5.0, 'hi': 7.0, 'k': 1.0},
              {'kind': 'exclusion', 'sample': 1, 'center': (0.5, -0.5, 0.25), 'radius': 3.0, 'k': 0.5}]


def ddpm_calls():
    phar, pocket, other = inputs()
    fixed = torch.tensor([[True], [False], [False], [True], [False]])
    fx, ft = torch.tensor([1.0, 0, 0, 2.0, 0]), torch.tensor([[0], [1], [0], [0], [1]])
    return {
        'sample_given_pocket': lambda m: m.sample_given_pocket(pocket, [2, 3], timesteps=K, seed=7, pocket_ids=[4, 9]),
        'sample_given_pocket-frames': lambda m: m.sample_given_pocket(pocket, torch.tensor([2, 3]), 2, K, marked(K + 2, 5, 3 + P), 7),
        'sample_restrained': lambda m: m.sample_restrained(pocket, [2, 3], RESTRAINTS, clash=2.5, scale=0.5, guide_below=0.75, timesteps=K, seed=7),
        'sample_diverse': lambda m: m.sample_diverse(pocket, [2, 3], [2], strength=0.75, width=1.5, max_shift=0.25, return_frames=2, timesteps=K,
                                                     seed=7),
        'sample_given_pockets': lambda m: m.sample_given_pockets([pocket, other], [2, 3], weights=[1.0, 3.0], timesteps=K, seed=7,
                                                                 group_ids=[5, 6]),
        'sample_restrained_given_pockets': lambda m: m.sample_restrained_given_pockets(
            [pocket, other], [2, 3], RESTRAINTS, clash=(2.0, 0.5), max_shift=0.5, return_frames=5, timesteps=K, seed=7),
        'inpaint': lambda m: m.inpaint(phar, pocket, fixed, resamplings=2, timesteps=K, seed=7, pocket_ids=[4, 9]),
        'edit': lambda m: m.edit(phar, pocket, fix_coords=fx, start=4, timesteps=K, noise=marked(6, 5, 3 + P), seed=7),
        'edit_restrained': lambda m: m.edit_restrained(phar, pocket, RESTRAINTS, fix_types=ft, resamplings=2, clash=2.5, scale=2.0, timesteps=K,
                                                       seed=7, pocket_ids=[4, 9]),
        'edit_given_pockets': lambda m: m.edit_given_pockets(phar, [pocket, other], fix_coords=fx, fix_types=ft, start=4,
                                                             weights=[[1.0, 1.0], [1.0, 3.0]], timesteps=K, seed=7, group_ids=[5, 6]),
        'edit_restrained_given_pockets': lambda m: m.edit_restrained_given_pockets(
            phar, [pocket, other], RESTRAINTS, fix_coords=fx, start=4, clash=2.5, guide_below=0.5, timesteps=K, noise=marked(6, 5, 3 + P), seed=7),
        'score': lambda m: m.score(phar, pocket, timesteps=K, repeats=2, noise=marked(2, K + 1, 5, 3 + P), seed=7, pocket_ids=[4, 9]),
        'score_given_pockets': lambda m: m.score_given_pockets(phar, [pocket, other], weights=[1.0, 3.0], timesteps=K, seed=7, group_ids=[5, 6],
                                                               return_levels=True, return_members=True),
    }


def ddpm_trace(name):
    model, h = bare_model(ConditionalDDPM), RecordingHandle()
    model.dynamics.hip_handle = lambda upload=True: h
    out = ddpm_calls()[name](model)
    if isinstance(out, dict):                                            # the scoring entries: what came back, and nll itself
        out = {'keys': {k: list(v.shape) for k, v in out.items()}, 'nll': [round(float(v), 2) for v in out['nll']]}
    else:                                                                # x of the phar rows, the pocket rows by their ids, the masks, the info
        pockets = out[1] if isinstance(out[1], list) else [out[1]]
        out = {'xh_phar': list(out[0].shape), 'phar_corner': norm(out[0][..., 0, 0]), 'pocket_ids': [norm(q[..., 0]) for q in pockets],
               'phar_mask': norm(out[2]), 'pocket_mask': norm(out[3]), 'info': norm(out[4]) if len(out) > 4 else None}
    return {'calls': h.calls, 'out': out}


# the expected traces, as literals.  Calls every entry makes:
ONE = ('set_layout', ('int64', [2], [2, 3]), ('int64', [2], [3, 4]), False)                  # one pocket per sample
MEMBERS = ('set_layout', ('int64', [4], [2, 2, 3, 3]), ('int64', [4], [3, 2, 4, 5]), False)  # sample g * M + m is pocket m of group g
STEP, GUIDE, RUN, STATUS = ('set_step_table', 10, [11, 4]), ('set_guide_table', 10, [10, 2]), ('run_range_guarded',), ('chain_status',)
# ... and the tensors they hand down
POCKET = {'pocket_x': ('float32', [7, 3], [[10.0, 5.0, -10.0], [11.0, 5.5, -11.0], [12.0, 6.0, -12.0], [13.0, 6.5, -13.0], [14.0, 7.0, -14.0],
                                           [15.0, 7.5, -15.0], [16.0, 8.0, -16.0]]),
          'pocket_onehot': ('float32', [7, 20], 'nonzero', [(10, 1.0), (31, 1.0), (52, 1.0), (73, 1.0), (94, 1.0), (115, 1.0), (136, 1.0)])}
POCKETS = {'pocket_x': ('float32', [14, 3], [[10.0, 5.0, -10.0], [11.0, 5.5, -11.0], [12.0, 6.0, -12.0], [100.0, 50.0, -100.0],
                                             [101.0, 50.5, -101.0], [13.0, 6.5, -13.0], [14.0, 7.0, -14.0], [15.0, 7.5, -15.0], [16.0, 8.0, -16.0],
                                             [102.0, 51.0, -102.0], [103.0, 51.5, -103.0], [104.0, 52.0, -104.0], [105.0, 52.5, -105.0],
                                             [106.0, 53.0, -106.0]]),
           'pocket_onehot': ('float32', [14, 20], 'nonzero', [(10, 1.0), (31, 1.0), (52, 1.0), (60, 1.0), (81, 1.0), (113, 1.0), (134, 1.0),
                                                              (155, 1.0), (176, 1.0), (182, 1.0), (203, 1.0), (224, 1.0), (245, 1.0), (266, 1.0)]),
           'group_sizes': [2, 2]}
GIVEN = {'phar_x': ('float32', [5, 3], [[1.0, 0.5, -1.0], [2.0, 1.0, -2.0], [3.0, 1.5, -3.0], [4.0, 2.0, -4.0], [5.0, 2.5, -5.0]]),
         'phar_onehot': ('float32', [5, 8], 'nonzero', [(1, 1.0), (10, 1.0), (19, 1.0), (28, 1.0), (37, 1.0)])}
RECORDS = [[0, 0, 1, 0, ('float32', [3], [1.0, 2.0, 3.0]), 1.5, 0.0, 2.0], [1, 1, 0, 2, ('float32', [3], [0.0, 0.0, 0.0]), 5.0, 7.0, 1.0],
           [2, 1, 0, 0, ('float32', [3], [0.5, -0.5, 0.25]), 3.0, 0.0, 0.5]]
FIX_A, FIX_B, FIX_0 = ('float32', [5], [1.0, 0.0, 0.0, 1.0, 0.0]), ('float32', [5], [0.0, 1.0, 0.0, 0.0, 1.0]), ('float32', [5], [0.0] * 5)
NOISE_6 = ('float32', [6, 5, 11], 'nonzero', [(3, 1.5), (328, -2.25)])
LEVELS = [5, 10, 15, 20, 25, 30, 35, 40, 45, 50, 0]
COEF = [[0.99, 0.1411], [0.96, 0.28], [0.91, 0.4146], [0.84, 0.5426], [0.75, 0.6614], [0.64, 0.7684], [0.51, 0.8602], [0.36, 0.9329],
        [0.19, 0.9818], [0.0034, 1.0], [1.0, 0.0032]]
# ... and what comes back
PHAR_MASK, POCKET_MASK = ('int64', [5], [0, 0, 1, 1, 1]), ('int64', [7], [0, 0, 0, 1, 1, 1, 1])
POCKET_MASKS = [POCKET_MASK, ('int64', [7], [0, 0, 1, 1, 1, 1, 1])]
IDS, OTHER_IDS = [10.0, 11.0, 12.0, 13.0, 14.0, 15.0, 16.0], [100.0, 101.0, 102.0, 103.0, 104.0, 105.0, 106.0]
ENERGY = {'energy': ('float32', [2], [0.0, 0.5]), 'max_violation': ('float32', [2], [0.25, 0.75])}
PER_OP = ('float32', [10, 2], [[0.0, 1.0], [2.0, 3.0], [4.0, 5.0], [6.0, 7.0], [8.0, 9.0], [10.0, 11.0], [12.0, 13.0], [14.0, 15.0], [16.0, 17.0],
                               [18.0, 19.0]])
SCORE_KEYS = {'nll': [2], 'loss_t': [2], 'loss_0_x': [2], 'loss_0_h': [2], 'neg_log_const_0': [2], 'kl_prior': [2], 'delta_log_px': [2],
              'log_pN': [2]}


def came_back(info=None, groups=False):
    """The last frame alone: the phar rows as returned, every pocket's rows back in its own order."""
    return {'xh_phar': [5, 11], 'phar_corner': ('float32', [], 0.0), 'phar_mask': PHAR_MASK, 'info': info,
            'pocket_ids': [('float32', [7], IDS), ('float32', [7], OTHER_IDS)] if groups else [('float32', [7], IDS)],
            'pocket_mask': POCKET_MASKS if groups else POCKET_MASK}


def two_frames(info):
    """Frame 0 the result, frame 1 the state after op 4 (s = 5 on the frame grid of 10 steps)."""
    return {'xh_phar': [2, 5, 11], 'phar_corner': ('float32', [2], [0.0, 4.0]), 'phar_mask': PHAR_MASK, 'pocket_mask': POCKET_MASK, 'info': info,
            'pocket_ids': [('float32', [2, 7], [IDS, [14.0, 15.0, 16.0, 17.0, 18.0, 19.0, 20.0]])]}


def five_frames(ids):
    return [[i + op for i in ids] for op in (0, 7, 5, 3, 1)]


EXPECTED_DDPM = {
    'sample_given_pocket': {
        'calls': [ONE, STEP, RUN, ('sample_chain', {**POCKET, 'timesteps': 10, 'noise': None, 'seed': 7, 'pocket_ids': [4, 9], 'want_steps': False,
                                                    'use_graph': True}), STATUS],
        'out': came_back()},
    'sample_given_pocket-frames': {
        'calls': [ONE, STEP, RUN, ('sample_chain', {**POCKET, 'timesteps': 10, 'noise': ('float32', [12, 5, 11], 'nonzero', [(3, 1.5), (658, -2.25)]),
                                                    'seed': 7, 'pocket_ids': None, 'want_steps': True, 'use_graph': True}), STATUS],
        'out': two_frames(None)},
    'sample_restrained': {
        'calls': [ONE, STEP, GUIDE, RUN,
                  ('restrained_chain', {**POCKET, 'timesteps': 10, 'restraints': RECORDS, 'clash_radius': 2.5, 'clash_k': 1.0, 'scale': 0.5,
                                        'max_shift': 1.0, 'guide_below': 0.75, 'noise': None, 'seed': 7, 'pocket_ids': None, 'want_steps': False,
                                        'use_graph': True}), STATUS],
        'out': came_back(ENERGY)},
    'sample_diverse': {
        'calls': [ONE, STEP, GUIDE, RUN,
                  ('diverse_chain', {**POCKET, 'timesteps': 10, 'set_sizes': ('int64', [1], [2]), 'strength': 0.75, 'width': 1.5, 'max_shift': 0.25,
                                     'guide_below': 1.0, 'noise': None, 'seed': 7, 'pocket_ids': None, 'want_steps': True, 'use_graph': True}),
                  STATUS],
        'out': two_frames({'overlap': ('float32', [2], [0.0, 0.25]), 'op_overlap': PER_OP})},
    'sample_given_pockets': {
        'calls': [MEMBERS, STEP, RUN,
                  ('multi_pocket_chain', {**POCKETS, 'weights': ('float32', [4], [0.25, 0.75, 0.25, 0.75]), 'timesteps': 10, 'noise': None, 'seed': 7,
                                          'group_ids': [5, 6], 'want_steps': False, 'use_graph': True}), STATUS],
        'out': came_back(groups=True)},
    'sample_restrained_given_pockets': {
        'calls': [MEMBERS, STEP, GUIDE, RUN,
                  ('multi_restrained_chain', {**POCKETS, 'weights': ('float32', [4], [0.5, 0.5, 0.5, 0.5]), 'timesteps': 10, 'restraints': RECORDS,
                                              'clash_radius': 2.0, 'clash_k': 0.5, 'scale': 1.0, 'max_shift': 0.5, 'guide_below': 1.0, 'noise': None,
                                              'seed': 7, 'group_ids': None, 'want_steps': True, 'use_graph': True}), STATUS],
        'out': {'xh_phar': [5, 5, 11], 'phar_corner': ('float32', [5], [0.0, 7.0, 5.0, 3.0, 1.0]), 'phar_mask': PHAR_MASK,
                'pocket_ids': [('float32', [5, 7], five_frames(IDS)), ('float32', [5, 7], five_frames(OTHER_IDS))], 'pocket_mask': POCKET_MASKS,
                'info': {**ENERGY, 'op_energy': PER_OP}}},
    'inpaint': {
        'calls': [ONE, STEP, ('edit_plan', 10, 10, 2, 1), RUN,
                  ('inpaint_chain', {**POCKET, **GIVEN, 'phar_fixed': FIX_A, 'timesteps': 10, 'resamplings': 2, 'jump_length': 1, 'noise': None,
                                     'seed': 7, 'pocket_ids': [4, 9], 'want_steps': False, 'use_graph': True}), STATUS],
        'out': came_back()},
    'edit': {
        'calls': [ONE, STEP, ('edit_plan', 10, 4, 1, 1), RUN,
                  ('edit_chain', {**POCKET, **GIVEN, 'fix_x': FIX_A, 'fix_h': FIX_0, 'timesteps': 10, 'start': 4, 'resamplings': 1, 'jump_length': 1,
                                  'noise': NOISE_6, 'seed': 7, 'pocket_ids': None, 'want_steps': False, 'use_graph': True}), STATUS],
        'out': came_back()},
    'edit_restrained': {
        'calls': [ONE, STEP, GUIDE, ('edit_plan', 10, 10, 2, 1), RUN,
                  ('restrained_edit_chain', {**POCKET, **GIVEN, 'fix_x': FIX_0, 'fix_h': FIX_B, 'timesteps': 10, 'start': 10, 'resamplings': 2,
                                             'jump_length': 1, 'restraints': RECORDS, 'clash_radius': 2.5, 'clash_k': 1.0, 'scale': 2.0,
                                             'max_shift': 1.0, 'guide_below': 1.0, 'noise': None, 'seed': 7, 'pocket_ids': [4, 9],
                                             'want_steps': False, 'use_graph': True}), STATUS],
        'out': came_back(ENERGY)},
    'edit_given_pockets': {
        'calls': [MEMBERS, STEP, ('edit_plan', 10, 4, 1, 1), RUN,
                  ('multi_edit_chain', {**POCKETS, **GIVEN, 'weights': ('float32', [4], [0.5, 0.5, 0.25, 0.75]), 'fix_x': FIX_A, 'fix_h': FIX_B,
                                        'timesteps': 10, 'start': 4, 'resamplings': 1, 'jump_length': 1, 'noise': None, 'seed': 7,
                                        'group_ids': [5, 6], 'want_steps': False, 'use_graph': True}), STATUS],
        'out': came_back(groups=True)},
    'edit_restrained_given_pockets': {
        'calls': [MEMBERS, STEP, GUIDE, ('edit_plan', 10, 4, 1, 1), RUN,
                  ('multi_restrained_edit_chain', {**POCKETS, **GIVEN, 'weights': ('float32', [4], [0.5, 0.5, 0.5, 0.5]), 'fix_x': FIX_A,
                                                   'fix_h': FIX_0, 'timesteps': 10, 'start': 4, 'resamplings': 1, 'jump_length': 1,
                                                   'restraints': RECORDS, 'clash_radius': 2.5, 'clash_k': 1.0, 'scale': 1.0, 'max_shift': 1.0,
                                                   'guide_below': 0.5, 'noise': NOISE_6, 'seed': 7, 'group_ids': None, 'want_steps': False,
                                                   'use_graph': True}), STATUS],
        'out': came_back(ENERGY, groups=True)},
    'score': {
        'calls': [ONE, RUN,
                  ('score_chain', {**GIVEN, **POCKET, 't_levels': ('int32', [22], LEVELS * 2),
                                   'level_coef': ('float32', [23, 2], COEF * 2 + COEF[9:10]),
                                   'noise': ('float32', [22, 5, 11], 'nonzero', [(3, 1.5), (1208, -2.25)]), 'seed': 7, 'pocket_ids': [4, 9],
                                   'use_graph': True}), STATUS],
        'out': {'keys': {**SCORE_KEYS, 'nll_repeats': [2, 2], 'loss_t_repeats': [2, 2], 'loss_0_x_repeats': [2, 2], 'loss_0_h_repeats': [2, 2]},
                'nll': [614.37, 621.61]}},
    'score_given_pockets': {
        'calls': [MEMBERS, RUN,
                  ('multi_score_chain', {**GIVEN, **POCKETS, 'weights': ('float32', [4], [0.25, 0.75, 0.25, 0.75]),
                                         't_levels': ('int32', [11], LEVELS),
                                         'level_coef': ('float32', [12, 2], COEF + COEF[9:10]), 'noise': None, 'seed': 7, 'group_ids': [5, 6],
                                         'want_members': True, 'use_graph': True}), STATUS],
        'out': {'keys': {**SCORE_KEYS, 'nll_repeats': [1, 2], 'loss_t_repeats': [1, 2], 'loss_0_x_repeats': [1, 2], 'loss_0_h_repeats': [1, 2],
                         'member_nll': [2, 2], 'member_loss_t': [2, 2], 'member_loss_0_x': [2, 2], 'member_log_pN': [2, 2], 't_levels': [11],
                         'level_terms': [1, 11, 2], 'level_sums': [1, 11, 2, 4], 'member_level_sums': [1, 11, 2, 2, 4]},
                'nll': [377.81, 385.05]}},
}


@pytest.mark.parametrize('name', sorted(ddpm_calls()))
def test_conditional_ddpm_hands_down(name):
    assert ddpm_trace(name) == EXPECTED_DDPM[name]


# ---------------------------------------------------------------- PharPocketDDPM against recording ConditionalDDPM entries
SAMPLERS = ('sample_given_pocket', 'sample_restrained', 'sample_diverse', 'sample_given_pockets', 'sample_restrained_given_pockets', 'inpaint',
            'edit', 'edit_restrained', 'edit_given_pockets', 'edit_restrained_given_pockets')
BARE_RESTRAINTS = [{'kind': 'position', 'point': 3, 'center': (12.0, 7.0, -3.0), 'radius': 1.5, 'k': 2.0},
                   {'kind': 'distance', 'points': (0, 1), 'lo': 5.0, 'hi': 7.0, 'k': 1.0}]
POINTS = [('Aromatic', (12.0, 7.0, -3.0)), ('Donor', (13.0, 6.5, -2.0))]


def record_samplers(model, seen, returned):
    """Every ConditionalDDPM entry replaced by a recorder that answers as the sampler would: row r of the phar at (r, 2 r, 3 r) with type
    r mod P, everything translated by a shift of its sample's own, which the caller has to undo.  returned: the pocket tensors handed
    back, which some callers move back in place."""
    def fake(name):
        real = getattr(ConditionalDDPM, name)

        def call(*args, **kw):
            a = bound(real, args, kw)
            seen.append((name, norm(a)))
            pockets = a['pockets'] if 'pockets' in a else [a['pocket']]
            sizes = a['phar']['size'] if 'phar' in a else torch.as_tensor(a['num_nodes_phar']).reshape(-1)
            n = len(sizes)
            phar_mask = torch.repeat_interleave(torch.arange(n), sizes.cpu())
            r = torch.arange(len(phar_mask), dtype=torch.float32)
            shift = torch.stack([torch.arange(n) + 1.0, torch.full((n,), -2.0), torch.full((n,), 3.0)], dim=1)
            xh_phar = torch.cat([torch.stack([r, 2 * r, 3 * r], dim=1) + shift[phar_mask],
                                 torch.nn.functional.one_hot(torch.arange(len(r)) % P, P).float()], dim=1)
            xh_pockets = [torch.cat([q['x'] + shift[q['mask']], q['one_hot'].float()], dim=1) for q in pockets]
            masks = [q['mask'] for q in pockets]
            returned.extend(xh_pockets)
            out = (xh_phar, xh_pockets, phar_mask, masks) if 'pockets' in a else (xh_phar, xh_pockets[0], phar_mask, masks[0])
            if 'restrained' in name:
                out += ({'energy': torch.arange(n) / 4, 'max_violation': torch.arange(n) / 8},)
            if 'diverse' in name:
                out += ({'overlap': torch.arange(n) / 4},)
            return out
        return call
    for name in SAMPLERS:
        setattr(model.ddpm, name, fake(name))


def pdb_calls(f):
    one, two = dict(pocket_ids=['A:1', 'A:2', 'A:3']), dict(pocket_ids=[['A:4', 'A:5'], ['A:1', 'A:2', 'A:3']])
    return {
        'generate_phars': lambda m: m.generate_phars(f, 2, num_nodes_phar=torch.tensor([3, 2]), timesteps=K, seed=7, resamplings=3, **one),
        'generate_phars-prior': lambda m: m.generate_phars(f, 2, timesteps=K, **one),
        'generate_phars_multi': lambda m: m.generate_phars_multi([f, f], 2, weights=[1.0, 3.0], timesteps=K, seed=7, group_ids=[5, 6], **two),
        'generate_phars_restrained': lambda m: m.generate_phars_restrained(f, 2, BARE_RESTRAINTS, clash=2.5, scale=0.5, timesteps=K, seed=7, **one),
        'generate_phars_restrained-given': lambda m: m.generate_phars_restrained(f, 2, BARE_RESTRAINTS, num_nodes_phar=5, max_shift=0.5,
                                                                                 guide_below=0.75, **one),
        'generate_phars_diverse': lambda m: m.generate_phars_diverse(f, 2, strength=0.75, width=1.5, timesteps=K, seed=7, **one),
        'generate_phars_diverse-given': lambda m: m.generate_phars_diverse(f, 2, num_nodes_phar=3, max_shift=0.5, guide_below=0.75, **one),
        'generate_phars_multi_restrained': lambda m: m.generate_phars_multi_restrained([f, f], 2, BARE_RESTRAINTS, weights=[1.0, 3.0], clash=2.5,
                                                                                       timesteps=K, seed=7, group_ids=[5, 6], **two),
        'inpaint_phars': lambda m: m.inpaint_phars(f, 2, POINTS, timesteps=K, resamplings=2, seed=7, **one),
        'inpaint_phars-given': lambda m: m.inpaint_phars(f, 2, POINTS, num_nodes_phar=torch.tensor([2, 4]), jump_length=2, **one),
        'edit_phars': lambda m: m.edit_phars(f, 2, POINTS, keep=['types', 'both'], strength=0.5, timesteps=K, seed=7, **one),
        'edit_phars-prior': lambda m: m.edit_phars(f, 2, POINTS, keep='coords', timesteps=K, resamplings=2, **one),
        'edit_phars_restrained': lambda m: m.edit_phars_restrained(f, 2, POINTS, BARE_RESTRAINTS, clash=2.5, scale=0.5, timesteps=K, seed=7, **one),
        'edit_phars_multi': lambda m: m.edit_phars_multi([f, f], 2, POINTS, strength=0.5, weights=[1.0, 3.0], timesteps=K, seed=7, **two),
        'edit_phars_multi_restrained': lambda m: m.edit_phars_multi_restrained([f, f], 2, POINTS, BARE_RESTRAINTS, num_nodes_phar=4, clash=2.5,
                                                                               max_shift=0.5, timesteps=K, resamplings=2, seed=7, **two),
    }


def pdb_trace(name, tmp_path):
    f = tmp_path / 'p.pdb'
    f.write_text(PDB_TEXT)
    model, seen, returned = PharPocketDDPM(**host_hparams()), [], []
    record_samplers(model, seen, returned)
    model.ddpm.size_distribution.sample_conditional = lambda n1, n2: torch.tensor([1, 3])       # (the size prior's draw)
    out = pdb_calls(str(f))[name](model)
    return {'calls': seen, 'out': norm(out), 'first_pocket_rows_after': [norm(q[0, :3]) for q in returned]}


# the expected traces, as literals.  The pocket dicts: residues 1-3 of the file, and residues 4-5 as the FIRST pocket of the multi entries
CA_123 = {'x': ('float32', [6, 3], [[11.639, 6.071, -5.147], [14.0, 7.5, -3.0], [16.5, 9.0, -1.0]] * 2),
          'one_hot': ('int64', [6, 20], 'nonzero', [(0, 1), (25, 1), (58, 1), (60, 1), (85, 1), (118, 1)]),
          'size': ('int64', [2], [3, 3]), 'mask': ('int64', [6], [0, 0, 0, 1, 1, 1])}
CA_45 = {'x': ('float32', [4, 3], [[12.5, 9.5, -2.0], [10.0, 8.0, 0.5]] * 2),
         'one_hot': ('int64', [4, 20], 'nonzero', [(9, 1), (35, 1), (49, 1), (75, 1)]),
         'size': ('int64', [2], [2, 2]), 'mask': ('int64', [4], [0, 0, 1, 1])}
TWO_POCKETS = [CA_45, CA_123]
GIVEN_ROWS, NO_ROW = [[12.0, 7.0, -3.0], [13.0, 6.5, -2.0]], [[0.0, 0.0, 0.0]]
PER_SAMPLE = [{'kind': 'position', 'point': 3, 'center': [12.0, 7.0, -3.0], 'radius': 1.5, 'k': 2.0, 'sample': 0},
              {'kind': 'distance', 'points': [0, 1], 'lo': 5.0, 'hi': 7.0, 'k': 1.0, 'sample': 0},
              {'kind': 'position', 'point': 3, 'center': [12.0, 7.0, -3.0], 'radius': 1.5, 'k': 2.0, 'sample': 1},
              {'kind': 'distance', 'points': [0, 1], 'lo': 5.0, 'hi': 7.0, 'k': 1.0, 'sample': 1}]
# a pocket row the sampler handed back: left translated (by sample 0's shift), or moved back in place
MOVED_123, BACK_123 = ('float32', [3], [12.639, 4.071, -2.147]), ('float32', [3], [11.639, 6.071, -5.147])
MOVED_45 = ('float32', [3], [13.5, 7.5, 1.0])
NAMES = ['Aromatic', 'Hydrophobe', 'PosIonizable', 'NegIonizable', 'Acceptor', 'Donor', 'LumpedHydrophobe', 'others']
INFO = {'energy': ('float32', [2], [0.0, 0.25]), 'max_violation': ('float32', [2], [0.0, 0.125])}
OVERLAP = {'overlap': ('float32', [2], [0.0, 0.25])}


def phar_given(sizes):
    """The phar dict of the edit kinds: POINTS as the first rows of every sample, the other rows zero."""
    n, first = sum(sizes), [sum(sizes[:b]) for b in range(len(sizes))]
    onehot = ('float32', [n, 8], 'nonzero', sorted((r * 8 + t, 1.0) for f in first for r, t in ((f, 0), (f + 1, 5))))
    return {'x': ('float32', [n, 3], [row for s in sizes for row in GIVEN_ROWS + NO_ROW * (s - 2)]), 'one_hot': onehot,
            'size': ('int64', [len(sizes)], sizes), 'mask': ('int64', [n], [b for b, s in enumerate(sizes) for _ in range(s)])}


def point_lists(sizes):
    """Row r came back at (r, 2 r, 3 r) with type r mod 8 once the sample's shift is undone."""
    first = [sum(sizes[:b]) for b in range(len(sizes))]
    return [[[NAMES[r % 8], [float(r), 2.0 * r, 3.0 * r]] for r in range(f, f + s)] for f, s in zip(first, sizes)]


def molecules(sizes):
    """generate_phars' dict (quirk Q9): 'Molecule_k' collects the k-th point of ALL samples by type."""
    out = {}
    for sample in point_lists(sizes):
        for k, (name, xyz) in enumerate(sample, start=1):
            out.setdefault(f'Molecule_{k}', {}).setdefault(name, []).append(('float32', [3], xyz))
    return out


EXPECTED_PDB = {
    'generate_phars': {
        'calls': [('sample_given_pocket', {'pocket': CA_123, 'num_nodes_phar': ('int64', [2], [3, 2]), 'return_frames': 1, 'timesteps': 10,
                                           'noise': None, 'seed': 7, 'pocket_ids': None})],
        'out': molecules([3, 2]), 'first_pocket_rows_after': [BACK_123]},
    'generate_phars-prior': {
        'calls': [('sample_given_pocket', {'pocket': CA_123, 'num_nodes_phar': ('int64', [2], [1, 3]), 'return_frames': 1, 'timesteps': 10,
                                           'noise': None, 'seed': None, 'pocket_ids': None})],
        'out': molecules([1, 3]), 'first_pocket_rows_after': [BACK_123]},
    'generate_phars_multi': {
        'calls': [('sample_given_pockets', {'pockets': TWO_POCKETS, 'num_nodes_phar': ('int64', [2], [1, 3]), 'weights': [1.0, 3.0],
                                            'return_frames': 1, 'timesteps': 10, 'noise': None, 'seed': 7, 'group_ids': [5, 6]})],
        'out': molecules([1, 3]), 'first_pocket_rows_after': [MOVED_45, MOVED_123]},
    'generate_phars_restrained': {
        'calls': [('sample_restrained', {'pocket': CA_123, 'num_nodes_phar': ('int64', [2], [4, 4]), 'restraints': PER_SAMPLE, 'clash': 2.5,
                                         'scale': 0.5, 'max_shift': None, 'guide_below': 1.0, 'return_frames': 1, 'timesteps': 10, 'noise': None,
                                         'seed': 7, 'pocket_ids': None})],
        'out': [point_lists([4, 4]), INFO], 'first_pocket_rows_after': [MOVED_123]},
    'generate_phars_restrained-given': {
        'calls': [('sample_restrained', {'pocket': CA_123, 'num_nodes_phar': ('int64', [2], [5, 5]), 'restraints': PER_SAMPLE, 'clash': None,
                                         'scale': 1.0, 'max_shift': 0.5, 'guide_below': 0.75, 'return_frames': 1, 'timesteps': None, 'noise': None,
                                         'seed': None, 'pocket_ids': None})],
        'out': [point_lists([5, 5]), INFO], 'first_pocket_rows_after': [MOVED_123]},
    'generate_phars_diverse': {
        'calls': [('sample_diverse', {'pocket': CA_123, 'num_nodes_phar': ('int64', [2], [1, 3]), 'set_sizes': [2], 'strength': 0.75, 'width': 1.5,
                                      'max_shift': None, 'guide_below': 1.0, 'return_frames': 1, 'timesteps': 10, 'noise': None, 'seed': 7,
                                      'pocket_ids': None})],
        'out': [point_lists([1, 3]), OVERLAP], 'first_pocket_rows_after': [MOVED_123]},
    'generate_phars_diverse-given': {
        'calls': [('sample_diverse', {'pocket': CA_123, 'num_nodes_phar': ('int64', [2], [3, 3]), 'set_sizes': [2], 'strength': 1.0, 'width': 2.0,
                                      'max_shift': 0.5, 'guide_below': 0.75, 'return_frames': 1, 'timesteps': None, 'noise': None, 'seed': None,
                                      'pocket_ids': None})],
        'out': [point_lists([3, 3]), OVERLAP], 'first_pocket_rows_after': [MOVED_123]},
    'generate_phars_multi_restrained': {
        'calls': [('sample_restrained_given_pockets', {'pockets': TWO_POCKETS, 'num_nodes_phar': ('int64', [2], [4, 4]), 'restraints': PER_SAMPLE,
                                                       'weights': [1.0, 3.0], 'clash': 2.5, 'scale': 1.0, 'max_shift': None, 'guide_below': 1.0,
                                                       'return_frames': 1, 'timesteps': 10, 'noise': None, 'seed': 7, 'group_ids': [5, 6]})],
        'out': [point_lists([4, 4]), INFO], 'first_pocket_rows_after': [MOVED_45, MOVED_123]},
    'inpaint_phars': {
        'calls': [('inpaint', {'phar': phar_given([2, 3]), 'pocket': CA_123, 'phar_fixed': ('float32', [5], [1.0, 1.0, 1.0, 1.0, 0.0]),
                               'resamplings': 2, 'jump_length': 1, 'return_frames': 1, 'timesteps': 10, 'noise': None, 'seed': 7,
                               'pocket_ids': None})],
        'out': molecules([2, 3]), 'first_pocket_rows_after': [BACK_123]},
    'inpaint_phars-given': {
        'calls': [('inpaint', {'phar': phar_given([2, 4]), 'pocket': CA_123, 'phar_fixed': ('float32', [6], [1.0, 1.0, 1.0, 1.0, 0.0, 0.0]),
                               'resamplings': 1, 'jump_length': 2, 'return_frames': 1, 'timesteps': None, 'noise': None, 'seed': None,
                               'pocket_ids': None})],
        'out': molecules([2, 4]), 'first_pocket_rows_after': [BACK_123]},
    'edit_phars': {
        'calls': [('edit', {'phar': phar_given([2, 2]), 'pocket': CA_123, 'fix_coords': ('float32', [4], [0.0, 1.0, 0.0, 1.0]),
                            'fix_types': ('float32', [4], [1.0, 1.0, 1.0, 1.0]), 'start': 5, 'resamplings': 1, 'jump_length': 1, 'timesteps': 10,
                            'noise': None, 'seed': 7, 'pocket_ids': None})],
        'out': point_lists([2, 2]), 'first_pocket_rows_after': [MOVED_123]},
    'edit_phars-prior': {
        'calls': [('edit', {'phar': phar_given([2, 3]), 'pocket': CA_123, 'fix_coords': ('float32', [5], [1.0, 1.0, 1.0, 1.0, 0.0]),
                            'fix_types': ('float32', [5], [0.0, 0.0, 0.0, 0.0, 0.0]), 'start': None, 'resamplings': 2, 'jump_length': 1,
                            'timesteps': 10, 'noise': None, 'seed': None, 'pocket_ids': None})],
        'out': point_lists([2, 3]), 'first_pocket_rows_after': [MOVED_123]},
    'edit_phars_restrained': {
        'calls': [('edit_restrained', {'phar': phar_given([4, 4]), 'pocket': CA_123, 'restraints': PER_SAMPLE,
                                       'fix_coords': ('float32', [8], [1.0, 1.0, 0.0, 0.0, 1.0, 1.0, 0.0, 0.0]),
                                       'fix_types': ('float32', [8], [1.0, 1.0, 0.0, 0.0, 1.0, 1.0, 0.0, 0.0]), 'start': None, 'resamplings': 1,
                                       'jump_length': 1, 'clash': 2.5, 'scale': 0.5, 'max_shift': None, 'guide_below': 1.0, 'timesteps': 10,
                                       'noise': None, 'seed': 7, 'pocket_ids': None})],
        'out': [point_lists([4, 4]), INFO], 'first_pocket_rows_after': [MOVED_123]},
    'edit_phars_multi': {
        'calls': [('edit_given_pockets', {'phar': phar_given([2, 2]), 'pockets': TWO_POCKETS, 'fix_coords': ('float32', [4], [0.0, 0.0, 0.0, 0.0]),
                                          'fix_types': ('float32', [4], [1.0, 1.0, 1.0, 1.0]), 'start': 5, 'resamplings': 1, 'jump_length': 1,
                                          'weights': [1.0, 3.0], 'timesteps': 10, 'noise': None, 'seed': 7, 'group_ids': None})],
        'out': point_lists([2, 2]), 'first_pocket_rows_after': [MOVED_45, MOVED_123]},
    'edit_phars_multi_restrained': {
        'calls': [('edit_restrained_given_pockets', {'phar': phar_given([4, 4]), 'pockets': TWO_POCKETS, 'restraints': PER_SAMPLE,
                                                     'fix_coords': ('float32', [8], [1.0, 1.0, 0.0, 0.0, 1.0, 1.0, 0.0, 0.0]),
                                                     'fix_types': ('float32', [8], [1.0, 1.0, 0.0, 0.0, 1.0, 1.0, 0.0, 0.0]), 'start': None,
                                                     'resamplings': 2, 'jump_length': 1, 'weights': None, 'clash': 2.5, 'scale': 1.0,
                                                     'max_shift': 0.5, 'guide_below': 1.0, 'timesteps': 10, 'noise': None, 'seed': 7,
                                                     'group_ids': None})],
        'out': [point_lists([4, 4]), INFO], 'first_pocket_rows_after': [MOVED_45, MOVED_123]},
}


@pytest.mark.parametrize('name', sorted(pdb_calls('')))
def test_phar_pocket_ddpm_hands_down(name, tmp_path):
    assert pdb_trace(name, tmp_path) == EXPECTED_PDB[name]
