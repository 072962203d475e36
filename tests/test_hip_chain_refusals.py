"""The refusals of the C library's chain entries, traced: one literal table of (entry, one bad input) -> (return code, the exact text of
cmdgen_last_error), for the nine sampling entries, cmdgen_inpaint_chain and the two scoring entries.  The entries are called directly through
Handle.lib with raw ctypes arguments - the Python wrappers check most of these inputs themselves and would hide the library's answer.

Every refusal returns before anything is launched, so a refused call's device pointers are never read.  After an entry's refusals one valid call
of that entry on the ordinary handle returns CMDGEN_OK with finite outputs.  No chain runs longer than 5 steps.

Layouts: S - the first three samples of restraint_cases.MIXED (4, 1 and 8 points), the entries without groups; G - multi_pocket_cases.PAIRS
(three groups of two members; 6, 3 and 8 points), the entries with groups; BIG - two samples of three points, one with a pocket of 1100 atoms
(beyond the 64 KiB of LDS of every step kernel that keeps a sample there), one group of two; ROWS - 513 samples whose single set has one phar
row more than CMDGEN_MAX_SET_ROWS.  Handles: chain_kit's ordinary one (T = 1000), a joint one and a no_com_projection one (T = 500)."""
import ctypes as C

import numpy as np
import pytest
import torch

import chain_kit as kit
import multi_pocket_cases as mc
import restraint_cases as rc
from chain_kit import EINVAL, ESTATE, record
from cmdgen_amd import hip_backend
from cmdgen_amd.synthetic import ModelConfig, make_state_dict

pytestmark = pytest.mark.gpu
OK = 0

# ---------------------------------------------------------------------------------------------------------------------------------------
# the entries: their arguments behind the handle, in the order of include/cmdgen_hip.h
# ---------------------------------------------------------------------------------------------------------------------------------------
_POCKET, _GROUPS, _GIVEN = 'pocket_x pocket_onehot ', 'n_groups group_size weight ', 'phar_x phar_onehot fix_x fix_h '
_PLAN, _DRAWS = 'timesteps start resamplings jump_length noise n_draws seed ids ', 'noise seed ids '
_OUT, _END = 'xh_phar_out xh_pocket_out z_steps_out pocket_steps_out ', 'use_graph stream'
_GUIDE, _ENERGY = 'restraints n_restraints clash_radius clash_k scale max_shift guide_below ', 'energy_out op_energy_out '
_SETS, _LEVELS = 'n_sets set_size strength width max_shift guide_below ', 'n_levels t_levels level_coef '
ENTRY_ARGS = {k: v.split() for k, v in {
    'sample_chain': _POCKET + 'timesteps ' + _DRAWS + _OUT + _END,
    'restrained_chain': _POCKET + 'timesteps ' + _GUIDE + _DRAWS + _OUT + _ENERGY + _END,
    'diverse_chain': _POCKET + 'timesteps ' + _SETS + _DRAWS + _OUT + 'overlap_out op_overlap_out ' + _END,
    'multi_pocket_chain': _POCKET + _GROUPS + 'timesteps ' + _DRAWS + _OUT + _END,
    'multi_restrained_chain': _POCKET + _GROUPS + 'timesteps ' + _GUIDE + _DRAWS + _OUT + _ENERGY + _END,
    'edit_chain': _POCKET + _GIVEN + _PLAN + _OUT + _END,
    'inpaint_chain': _POCKET + 'phar_x phar_onehot fix_x timesteps resamplings jump_length noise n_draws seed ids ' + _OUT + _END,
    'restrained_edit_chain': _POCKET + _GIVEN + _PLAN + _OUT + _GUIDE + _ENERGY + _END,
    'multi_edit_chain': _POCKET + _GROUPS + _GIVEN + _PLAN + _OUT + _END,
    'multi_restrained_edit_chain': _POCKET + _GROUPS + _GIVEN + _PLAN + _OUT + _GUIDE + _ENERGY + _END,
    'score_chain': 'phar_x phar_onehot ' + _POCKET + _LEVELS + _DRAWS + 'terms_out kl_sums_out ' + _END,
    'multi_score_chain': 'phar_x phar_onehot ' + _POCKET + _GROUPS + _LEVELS + _DRAWS + 'terms_out member_terms_out kl_sums_out ' + _END,
}.items()}
ENTRIES = tuple(ENTRY_ARGS)
SAMPLING = ENTRIES[:10]
GROUPED = tuple(e for e in ENTRIES if 'n_groups' in ENTRY_ARGS[e])
GUIDED = tuple(e for e in ENTRIES if 'restraints' in ENTRY_ARGS[e])
PLANNED = tuple(e for e in ENTRIES if 'start' in ENTRY_ARGS[e])
SCORING = ENTRIES[10:]
PER_SAMPLE_GUIDED = ('restrained_chain', 'restrained_edit_chain')
GROUP_GUIDED = ('multi_restrained_chain', 'multi_restrained_edit_chain')

# ---------------------------------------------------------------------------------------------------------------------------------------
# the table.  A row: (entries, handle, layout, the one bad input, return code, text).  layout None: S or G, as the entry has groups
# ---------------------------------------------------------------------------------------------------------------------------------------
_JOINT = ' is not supported for the joint model (update_pocket_coords=1): its pocket nodes diffuse with the latent'
_NO_COM = ' is not supported for no_com_projection handles (SimpleConditionalDDPM)'
_FRAME, _EDIT_FRAME = ': the guidance frame follows the centre-of-mass projections', ': the edit chain and the guidance frame follow the centre-of-mass projections'
_USE_JOINT = 'this handle is the joint model (update_pocket_coords=1): use cmdgen_joint_chain'
_DIVERSE_NULL = 'null pointer (pocket_x, pocket_onehot, set_size_host, xh_phar_out, xh_pocket_out and overlap_out are required)'
_LDS = 'a sample has 1103 nodes: the %s in LDS (64 KiB)'
INF = float('inf')


def _rec(n=1, **kw):
    """The restraint arguments with n copies of one record."""
    return {'restraints': np.repeat(record(**kw), n), 'n_restraints': n}


def _weights(at, value):
    w = mc.weights_of(mc.PAIRS).copy()
    w[at] = value
    return w


NULLS = [   # every required pointer of an entry, one at a time -> EINVAL and the entry's wording
    ('sample_chain', 'pocket_x pocket_onehot xh_phar_out xh_pocket_out', 'null device pointer'),
    ('restrained_chain', 'pocket_x pocket_onehot xh_phar_out xh_pocket_out energy_out', 'null device pointer'),
    ('diverse_chain', 'pocket_x pocket_onehot set_size xh_phar_out xh_pocket_out overlap_out', _DIVERSE_NULL),
    ('multi_pocket_chain', 'pocket_x pocket_onehot group_size weight xh_phar_out xh_pocket_out', 'null pointer'),
    ('multi_restrained_chain', 'pocket_x pocket_onehot group_size weight xh_phar_out xh_pocket_out energy_out', 'null pointer'),
    ('edit_chain', 'pocket_x pocket_onehot phar_x phar_onehot fix_x fix_h xh_phar_out xh_pocket_out', 'null device pointer'),
    ('inpaint_chain', 'pocket_x pocket_onehot phar_x phar_onehot fix_x xh_phar_out xh_pocket_out', 'null device pointer'),
    ('restrained_edit_chain', 'pocket_x pocket_onehot phar_x phar_onehot fix_x fix_h xh_phar_out xh_pocket_out energy_out', 'null device pointer'),
    ('multi_edit_chain', 'pocket_x pocket_onehot group_size weight phar_x phar_onehot fix_x fix_h xh_phar_out xh_pocket_out', 'null pointer'),
    ('multi_restrained_edit_chain', 'pocket_x pocket_onehot group_size weight phar_x phar_onehot fix_x fix_h xh_phar_out xh_pocket_out energy_out',
     'null pointer'),
    ('score_chain', 'phar_x phar_onehot pocket_x pocket_onehot t_levels terms_out kl_sums_out', 'null pointer'),
    ('multi_score_chain', 'phar_x phar_onehot pocket_x pocket_onehot group_size weight t_levels terms_out kl_sums_out', 'null pointer'),
]

TABLE = [((e,), 'ordinary', None, {name: None}, EINVAL, text) for e, names, text in NULLS for name in names.split()] + [
    # ---- timesteps
    (SAMPLING, 'ordinary', None, {'timesteps': 0}, EINVAL, 'timesteps=0 must be in [1, 1000]'),
    (SAMPLING, 'ordinary', None, {'timesteps': 1001}, EINVAL, 'timesteps=1001 must be in [1, 1000]'),
    # ---- a joint handle
    (('sample_chain', 'edit_chain', 'inpaint_chain'), 'joint', None, {}, ESTATE, _USE_JOINT),
    (('restrained_chain',), 'joint', None, {}, ESTATE, 'the restrained chain' + _JOINT),
    (('diverse_chain',), 'joint', None, {}, ESTATE, 'the diverse chain' + _JOINT),
    (('multi_pocket_chain',), 'joint', None, {}, ESTATE, 'the multi-pocket chain' + _JOINT),
    (('multi_restrained_chain',), 'joint', None, {}, ESTATE, 'the restrained multi-pocket chain' + _JOINT),
    (('restrained_edit_chain',), 'joint', None, {}, ESTATE, 'the restrained edit chain' + _JOINT),
    (('multi_edit_chain',), 'joint', None, {}, ESTATE, 'the multi-pocket edit chain' + _JOINT),
    (('multi_restrained_edit_chain',), 'joint', None, {}, ESTATE, 'the restrained multi-pocket edit chain' + _JOINT),
    (SCORING, 'joint', None, {}, ESTATE, "scoring is not supported for the joint model (update_pocket_coords=1): its loss has the pocket's own terms"),
    # ---- a no_com handle (cmdgen_sample_chain runs on one: test_sample_chain_runs_on_a_no_com_handle)
    (('edit_chain', 'inpaint_chain'), 'no_com', None, {}, ESTATE, 'inpainting' + _NO_COM),
    (('restrained_chain',), 'no_com', None, {}, EINVAL, 'the restrained chain' + _NO_COM + _FRAME),
    (('diverse_chain',), 'no_com', None, {}, EINVAL, 'the diverse chain' + _NO_COM + _FRAME),
    (('multi_pocket_chain',), 'no_com', None, {}, ESTATE, 'the multi-pocket chain' + _NO_COM),
    (('multi_restrained_chain',), 'no_com', None, {}, ESTATE, 'the restrained multi-pocket chain' + _NO_COM + _FRAME),
    (('restrained_edit_chain',), 'no_com', None, {}, ESTATE, 'the restrained edit chain' + _NO_COM + _EDIT_FRAME),
    (('multi_edit_chain',), 'no_com', None, {}, ESTATE, 'the multi-pocket edit chain' + _NO_COM),
    (('multi_restrained_edit_chain',), 'no_com', None, {}, ESTATE, 'the restrained multi-pocket edit chain' + _NO_COM + _EDIT_FRAME),
    (SCORING, 'no_com', None, {}, ESTATE, 'scoring' + _NO_COM),
    # ---- check_inpaint_args (the alias has no start of its own)
    (PLANNED, 'ordinary', None, {'start': 0}, EINVAL, 'start=0 must be in [1, timesteps=5]'),
    (PLANNED, 'ordinary', None, {'start': 6}, EINVAL, 'start=6 must be in [1, timesteps=5]'),
    (PLANNED + ('inpaint_chain',), 'ordinary', None, {'resamplings': 0}, EINVAL, 'resamplings and jump_length must be >= 1'),
    (PLANNED + ('inpaint_chain',), 'ordinary', None, {'jump_length': 0}, EINVAL, 'resamplings and jump_length must be >= 1'),
    # ---- injected noise with too few draws (start = 3 of 5: 1 + 2 x 3 + 1 draws; the alias starts at 5: 1 + 2 x 5 + 1)
    (PLANNED, 'ordinary', None, {'noise': 'one draw', 'n_draws': 1}, EINVAL, 'noise holds 1 draws, the schedule needs 8'),
    (('inpaint_chain',), 'ordinary', None, {'noise': 'one draw', 'n_draws': 1}, EINVAL, 'noise holds 1 draws, the schedule needs 12'),
    # ---- build_group_plan
    (GROUPED, 'ordinary', None, {'n_groups': 0}, EINVAL, 'n_groups=0 must be in [1, batch=6]'),
    (GROUPED, 'ordinary', None, {'n_groups': 7}, EINVAL, 'n_groups=7 must be in [1, batch=6]'),
    (GROUPED, 'ordinary', None, {'group_size': (0, 2, 2)}, EINVAL, 'group 0 has 0 members: sizes must be in [1, 8]'),
    (GROUPED, 'ordinary', None, {'group_size': (2, 9, 2)}, EINVAL, 'group 1 has 9 members: sizes must be in [1, 8]'),
    (GROUPED, 'ordinary', None, {'group_size': (2, 2, 3)}, EINVAL, 'the group sizes sum to 7, the layout has 6 samples'),
    (GROUPED, 'ordinary', None, {'group_size': (3, 1, 2)}, EINVAL,
     'group 0: member 2 has 3 phar nodes, member 0 has 6 (the members of a group share one latent)'),
    (GROUPED, 'ordinary', None, {'weight': _weights(3, -0.5)}, EINVAL, 'group 1: weight 1 is -0.5 (weights must be finite and >= 0)'),
    (GROUPED, 'ordinary', None, {'weight': _weights(4, INF)}, EINVAL, 'group 2: weight 0 is inf (weights must be finite and >= 0)'),
    (GROUPED, 'ordinary', None, {'weight': np.full(6, 0.25, dtype=np.float32)}, EINVAL,
     'group 0: its weights sum to 0.5, not 1 (the caller normalises them)'),
    (GROUPED[:4], 'ordinary', 'BIG', {}, EINVAL, _LDS % "multi-pocket step keeps a sample's positions, degrees and z"),
    # ---- the restraint check: the list and the scalars, whoever owns the records
    (GUIDED, 'ordinary', None, {'n_restraints': -1}, EINVAL, 'n_restraints=-1 without a restraint list'),
    (GUIDED, 'ordinary', None, {'restraints': None}, EINVAL, 'n_restraints=1 without a restraint list'),
    (GUIDED, 'ordinary', None, {'clash_radius': -1.0}, EINVAL, 'clash_radius=-1, clash_k=1 must be finite and >= 0'),
    (GUIDED, 'ordinary', None, {'clash_k': INF}, EINVAL, 'clash_radius=3, clash_k=inf must be finite and >= 0'),
    (GUIDED, 'ordinary', None, {'scale': -1.0}, EINVAL, 'scale=-1 must be finite and >= 0'),
    (GUIDED, 'ordinary', None, {'max_shift': 0.0}, EINVAL, 'max_shift=0 must be finite and > 0'),
    (GUIDED, 'ordinary', None, {'guide_below': 1.5}, EINVAL, 'guide_below=1.5 must be in [0, 1]'),
    (GUIDED, 'ordinary', None, _rec(kind=7), EINVAL, 'restraint 0: unknown kind 7'),
    (GUIDED, 'ordinary', None, _rec(kind=1, i=2, j=2, a=1.0, b=2.0), EINVAL, 'restraint 0: a distance between point 2 and itself (i == j)'),
    (GUIDED, 'ordinary', None, _rec(kind=1, i=0, j=1, a=-1.0, b=2.0), EINVAL, 'restraint 0: lo=-1, hi=2 must be finite and >= 0'),
    (GUIDED, 'ordinary', None, _rec(kind=1, i=0, j=1, a=3.0, b=2.0), EINVAL, 'restraint 0: lo=3 > hi=2'),
    (GUIDED, 'ordinary', None, _rec(kind=0, a=-1.0), EINVAL, 'restraint 0: radius=-1 must be finite and >= 0'),
    (GUIDED, 'ordinary', None, _rec(kind=2, c=(0.0, INF, 0.0)), EINVAL, 'restraint 0: a non-finite centre'),
    (GUIDED, 'ordinary', None, _rec(kind=0, k=-1.0), EINVAL, 'restraint 0: k=-1 must be finite and >= 0'),
    # ---- ... with sample owners (4, 1 and 8 points)
    (PER_SAMPLE_GUIDED, 'ordinary', None, _rec(sample=3), EINVAL, "restraint 0: sample 3 outside the layout's 3 samples"),
    (PER_SAMPLE_GUIDED, 'ordinary', None, _rec(sample=-1), EINVAL, "restraint 0: sample -1 outside the layout's 3 samples"),
    (PER_SAMPLE_GUIDED, 'ordinary', None, _rec(kind=0, sample=1, i=1), EINVAL, 'restraint 0: point 1, sample 1 has 1 points'),
    (PER_SAMPLE_GUIDED, 'ordinary', None, _rec(kind=1, sample=0, i=0, j=4, a=1.0, b=2.0), EINVAL, 'restraint 0: point 4, sample 0 has 4 points'),
    (PER_SAMPLE_GUIDED, 'ordinary', None, _rec(257, sample=2), EINVAL, 'sample 2 has more than 256 restraints'),
    (('restrained_chain',), 'ordinary', 'BIG', {}, EINVAL, _LDS % "restrained step keeps a sample's positions, z and guidance terms"),
    (('restrained_edit_chain',), 'ordinary', 'BIG', {}, EINVAL, _LDS % "restrained step keeps a sample's positions, z and guidance terms"),
    # ---- ... with group owners (6, 3 and 8 points)
    (GROUP_GUIDED, 'ordinary', None, _rec(sample=3), EINVAL, "restraint 0: group 3 outside the call's 3 groups"),
    (GROUP_GUIDED, 'ordinary', None, _rec(sample=-1), EINVAL, "restraint 0: group -1 outside the call's 3 groups"),
    (GROUP_GUIDED, 'ordinary', None, _rec(kind=0, sample=1, i=3), EINVAL, 'restraint 0: point 3, group 1 has 3 points'),
    (GROUP_GUIDED, 'ordinary', None, _rec(kind=1, sample=0, i=0, j=6, a=1.0, b=2.0), EINVAL, 'restraint 0: point 6, group 0 has 6 points'),
    (GROUP_GUIDED, 'ordinary', None, _rec(257, sample=2), EINVAL, 'group 2 has more than 256 restraints'),
    # ---- the diverse chain's scalars, then build_set_plan
    (('diverse_chain',), 'ordinary', None, {'strength': -1.0}, EINVAL, 'strength=-1 must be finite and >= 0'),
    (('diverse_chain',), 'ordinary', None, {'width': 0.0}, EINVAL, 'width=0 must be finite and > 0'),
    (('diverse_chain',), 'ordinary', None, {'max_shift': 0.0}, EINVAL, 'max_shift=0 must be finite and > 0'),
    (('diverse_chain',), 'ordinary', None, {'guide_below': 1.5}, EINVAL, 'guide_below=1.5 must be in [0, 1]'),
    (('diverse_chain',), 'ordinary', None, {'n_sets': 0}, EINVAL, 'n_sets=0 must be in [1, batch=3]'),
    (('diverse_chain',), 'ordinary', None, {'n_sets': 4}, EINVAL, 'n_sets=4 must be in [1, batch=3]'),
    (('diverse_chain',), 'ordinary', None, {'n_sets': 2, 'set_size': (2, 0)}, EINVAL, 'set_size[1]=0: every set has at least one sample'),
    (('diverse_chain',), 'ordinary', None, {'n_sets': 2, 'set_size': (1, 1)}, EINVAL, 'set_size sums to 2, the layout has 3 samples'),
    (('diverse_chain',), 'ordinary', 'ROWS', {}, EINVAL, 'set_size[0]: the set has 8193 phar rows, at most 8192 (the pair launch costs rows^2)'),
    (('diverse_chain',), 'ordinary', 'BIG', {}, EINVAL, _LDS % "diverse step keeps a sample's positions, degrees and z"),
    # ---- build_level_rows
    (SCORING, 'ordinary', None, {'n_levels': 0}, EINVAL, 'n_levels=0 must be >= 1'),
    (SCORING, 'ordinary', None, {'t_levels': (3, -1, 700, 1000)}, EINVAL, 'level 1 is t=-1: levels must be in [0, 1000]'),
    (SCORING, 'ordinary', None, {'t_levels': (3, 0, 700, 1001)}, EINVAL, 'level 3 is t=1001: levels must be in [0, 1000]'),
    (SCORING, 'ordinary', 'BIG', {}, EINVAL, _LDS % "scoring step keeps a sample's positions, z and row sums"),
]


# ---------------------------------------------------------------------------------------------------------------------------------------
# layouts, handles and the call
# ---------------------------------------------------------------------------------------------------------------------------------------
_layouts, _other = {}, {}


def _layout(name):
    """dict(nph [B], npk [B], and the valid value of every argument name on this layout, with and without groups) - built once."""
    if name in _layouts:
        return _layouts[name]
    if name == 'S':
        pb = kit.sub_batch(rc.pockets(rc.MIXED), [0, 1, 2])
        nph, npk, px, poh, sizes, w = pb.num_nodes_phar, pb.size, pb.x, pb.one_hot, (3,), np.full(3, 1 / 3, dtype=np.float32)
    elif name == 'G':
        pb = mc.member_pockets(mc.PAIRS)
        nph, npk, px, poh, sizes, w = pb.num_nodes_phar, pb.size, pb.x, pb.one_hot, mc.PAIRS.group_sizes, mc.weights_of(mc.PAIRS)
    else:
        nph, npk = {'BIG': ([3, 3], [1100, 5]), 'ROWS': ([16] * 512 + [1], [1] * 513)}[name]
        px, poh = np.zeros((sum(npk), 3), dtype=np.float32), np.zeros((sum(npk), 20), dtype=np.float32)
        sizes, w = (len(nph),), np.full(len(nph), 1.0 / len(nph), dtype=np.float32)
    nph, npk = np.asarray(nph, dtype=np.int64), np.asarray(npk, dtype=np.int64)
    lay = {'nph': nph, 'npk': npk}
    firsts = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    for multi, counts in ((False, nph), (True, nph[firsts])):
        rows, owners, n_pocket = int(counts.sum()), len(counts), int(npk.sum())
        x, oh, fx, fh = kit.given_for(counts, 5)
        new = lambda *shape: torch.full(shape, float('nan'), dtype=torch.float32, device='cuda')
        lay[multi] = {
            'pocket_x': kit.dev(px), 'pocket_onehot': kit.dev(poh), 'n_groups': len(sizes), 'group_size': sizes, 'weight': w,
            'phar_x': kit.dev(x), 'phar_onehot': kit.dev(oh), 'fix_x': kit.dev(fx), 'fix_h': kit.dev(fh),
            'timesteps': 5, 'start': 3, 'resamplings': 1, 'jump_length': 1, 'noise': None, 'n_draws': 0, 'seed': 7, 'ids': None,
            'xh_phar_out': new(rows, 11), 'xh_pocket_out': new(n_pocket, 23), 'z_steps_out': None, 'pocket_steps_out': None,
            **_rec(kind=0, sample=0, i=0, a=1.0, k=1.0), 'clash_radius': 3.0, 'clash_k': 1.0, 'scale': 1.0, 'max_shift': 1.0, 'guide_below': 1.0,
            'energy_out': new(owners, 2), 'op_energy_out': None,
            'n_sets': 1, 'set_size': (len(nph),), 'strength': 1.0, 'width': 2.0, 'overlap_out': new(owners), 'op_overlap_out': None,
            'n_levels': 4, 't_levels': (3, 0, 700, 1000), 'level_coef': None,
            'terms_out': new(4, owners, 4), 'member_terms_out': None, 'kl_sums_out': new(owners, 2),
            'use_graph': 0, 'stream': None, 'one draw': new(1, rows, 11),
        }
    _layouts[name] = lay
    return lay


def _handle(which):
    if which == 'ordinary':
        return kit.handle()
    if which not in _other:
        cfg = ModelConfig(hidden_nf=64, n_layers=1, **{'joint': dict(update_pocket_coords=True), 'no_com': dict(timesteps=500, no_com_projection=True)}[which])
        _other[which] = kit.handle_for(cfg, 'refusals', make_state_dict(cfg, seed=0))
    return _other[which]


_INT = {'group_size': np.int64, 'set_size': np.int64, 't_levels': np.int32}


def _c(name, v, keep):
    """The ctypes value of argument `name` (keep: what must outlive the call)."""
    if isinstance(v, str):
        raise AssertionError(v)
    if isinstance(v, tuple):
        v = np.asarray(v, dtype=_INT[name])
    if isinstance(v, np.ndarray):
        v = np.ascontiguousarray(v)
        keep.append(v)
        return v.ctypes.data_as(hip_backend._i64p if v.dtype == np.int64 and name != 'restraints' else C.c_void_p)
    if torch.is_tensor(v):
        return hip_backend._ptr(v)
    return v


def call(entry, which='ordinary', layout=None, bad=None):
    """One call of cmdgen_<entry> on the handle `which` under `layout`, the valid arguments with `bad` in place -> (code, last error, values)."""
    multi = entry in GROUPED
    lay = _layout(layout or ('G' if multi else 'S'))
    h = _handle(which)
    h.set_layout(lay['nph'], lay['npk'])
    values = dict(lay[multi], stream=h._stream())
    for name in [n for n, v in values.items() if n.endswith('_out') and v is not None]:      # fresh outputs: NaN, the scoring sums zero
        values[name] = torch.zeros_like(values[name]) if entry in SCORING else torch.full_like(values[name], float('nan'))
    values.update(bad or {})
    if isinstance(values['noise'], str):
        values['noise'] = values[values['noise']]
    keep = []
    args = [_c(name, values[name], keep) for name in ENTRY_ARGS[entry]]
    code = getattr(h.lib, 'cmdgen_' + entry)(h.h, *args)
    return code, h.lib.cmdgen_last_error(h.h).decode(), values


# ---------------------------------------------------------------------------------------------------------------------------------------
# the tests
# ---------------------------------------------------------------------------------------------------------------------------------------
OUTPUTS = {'energy_out': GUIDED, 'overlap_out': ('diverse_chain',), 'terms_out': SCORING, 'kl_sums_out': SCORING,
           'xh_phar_out': SAMPLING, 'xh_pocket_out': SAMPLING}


@pytest.mark.parametrize('entry', ENTRIES)
def test_every_refusal_of_the_entry_then_a_valid_call(entry):
    rows = [r for r in TABLE if entry in r[0]]
    assert len(rows) >= 7, entry
    wrong = []
    for _, which, layout, bad, code, text in rows:
        got = call(entry, which, layout, bad)[:2]
        if got != (code, text):
            wrong.append((which, layout, sorted(bad), got, (code, text)))
    assert not wrong, wrong
    code, _, values = call(entry)
    torch.cuda.synchronize()
    assert code == OK, (entry, _)
    st = _handle('ordinary').chain_status()
    assert st['nan_resets'] == 0
    outs = [values[name] for name, entries in OUTPUTS.items() if entry in entries]
    assert len(outs) >= 2 and all(bool(torch.isfinite(t).all()) for t in outs), entry


def test_the_table_names_every_entry_and_no_other():
    named = {e for r in TABLE for e in r[0]}
    assert named == set(ENTRIES) and all(set(r[3]) <= set(ENTRY_ARGS[e]) for r in TABLE for e in r[0])
    assert all(hasattr(hip_backend.load_library(), 'cmdgen_' + e) for e in ENTRIES)


def test_sample_chain_runs_on_a_no_com_handle():
    """The one sampling entry a no_com_projection handle does not refuse."""
    code, err, values = call('sample_chain', 'no_com')
    torch.cuda.synchronize()
    assert code == OK, err
    assert bool(torch.isfinite(values['xh_phar_out']).all()) and bool(torch.isfinite(values['xh_pocket_out']).all())
