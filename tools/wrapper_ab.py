"""One side of an A/B of the Python wrapper layers (hip_backend.Handle, ConditionalDDPM, PharPocketDDPM): every public chain entry of
the three once, fixed seed, on the smallest cases of tests/*_cases.py - graph on and off, steps / frames on and off - and one line per call
with the SHA-256 of every returned tensor and the chain status.  Run it in a fresh process per side, both on ONE library, and compare:

    export CMDGEN_LIB=$PWD/cmdgen_amd/libcmdgen_hip.so
    python tools/wrapper_ab.py <other root> > other.txt && python tools/wrapper_ab.py . > tree.txt && cmp other.txt tree.txt

<root> is the directory that holds the cmdgen_amd package under test: this tree's root, or a directory with another commit's package
(git archive <commit> cmdgen_amd | tar -x -C <other root>); tests/ and bench.py are this tree's on both sides.
profiles/wrapper_refactor_ab.txt is such a comparison."""
import hashlib
import itertools
import os
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROOT = os.path.abspath(sys.argv[1])
sys.path[:0] = [ROOT, REPO, os.path.join(REPO, 'tests')]

import numpy as np
import torch

import cmdgen_amd
assert os.path.dirname(os.path.dirname(os.path.abspath(cmdgen_amd.__file__))) == ROOT, cmdgen_amd.__file__
print('package:', cmdgen_amd.__file__, 'library:', os.environ.get('CMDGEN_LIB'), file=sys.stderr)

import chain_kit as kit
import diverse_cases as dc
import multi_pocket_cases as mc
import multi_restraint_cases as mrc
import restraint_cases as rc
from helpers import PDB_TEXT, dev
from cmdgen_amd import restraints as rs


def digest(v):
    if isinstance(v, torch.Tensor):
        v = v.detach().cpu().numpy()
    if isinstance(v, np.ndarray):
        return f'{v.dtype}{list(v.shape)}:' + hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest()[:24]
    if isinstance(v, dict):
        return '{' + ', '.join(f'{k}: {digest(x)}' for k, x in sorted(v.items())) + '}'
    if isinstance(v, (list, tuple)):
        return '[' + ', '.join(digest(x) for x in v) + ']'
    return repr(v)


def show(label, out, status):
    st = None if status is None else {k: status[k] for k in ('max_rel_com_error', 'max_cog', 'nan_resets')}
    print(f'{label}: {digest(out)} status {st}', flush=True)


SEED = 7
# ---- Handle: every *_chain method through chain_kit.run_chain, graph on and off, steps on and off
h = kit.handle()
NPH1 = rc.MIXED.nph[:3]                                    # the first three samples of the mixed case: 4, 1 and 8 points
pb1, pbm = kit.sub_batch(rc.pockets(rc.MIXED), [0, 1, 2]), mc.member_pockets(mc.PAIRS)
q1 = [r for r in rc.restraints_of(rc.MIXED) if r['sample'] < 3]
rec1 = rs.records(q1, NPH1)
recm = rs.records(mrc.restraints_of(mrc.PAIRS, pbm), mrc.PAIRS.nph)
groups = (list(mc.PAIRS.group_sizes), mc.weights_of(mc.PAIRS))
given1, givenm = kit.given_for(NPH1, 11), kit.given_for(mc.PAIRS.nph, 12)
for use_graph, want_steps in itertools.product((True, False), (True, False)):
    kw = dict(seed=SEED, use_graph=use_graph, want_steps=want_steps)
    tag = f'graph={int(use_graph)} steps={int(want_steps)}'
    show(f'Handle.sample_chain {tag}', *kit.run_chain(h, pb1, rc.K, ids=[3, 1, 2], **kw))
    show(f'Handle.restrained_chain {tag}', *kit.run_chain(h, pb1, rc.K, guide=kit.guide(rec1), **kw))
    show(f'Handle.inpaint_chain {tag}', *kit.run_chain(h, pb1, rc.K, given=(given1[0], given1[1], given1[2]), plan=(None, 2, 1), **kw))
    show(f'Handle.edit_chain {tag}', *kit.run_chain(h, pb1, rc.K, given=given1, plan=(3, 2, 1), **kw))
    show(f'Handle.restrained_edit_chain {tag}', *kit.run_chain(h, pb1, rc.K, given=given1, plan=(None, 1, 1), guide=kit.guide(rec1), **kw))
    show(f'Handle.multi_pocket_chain {tag}', *kit.run_chain(h, pbm, mc.K, groups=groups, ids=[5, 6, 4], **kw))
    show(f'Handle.multi_restrained_chain {tag}', *kit.run_chain(h, pbm, mc.K, groups=groups, guide=kit.guide(recm), **kw))
    show(f'Handle.multi_edit_chain {tag}', *kit.run_chain(h, pbm, mc.K, groups=groups, given=givenm, plan=(3, 2, 1), **kw))
    show(f'Handle.multi_restrained_edit_chain {tag}', *kit.run_chain(h, pbm, mc.K, groups=groups, given=givenm, plan=(None, 1, 1),
                                                                     guide=kit.guide(recm), **kw))
    pbd = dc.pockets(dc.LARGE)
    h.set_layout(pbd.num_nodes_phar, pbd.size)
    kit.host_tables(h, dc.LARGE.K)
    out = h.diverse_chain(dev(pbd.x), dev(pbd.one_hot), dc.LARGE.K, list(dc.LARGE.sets), seed=SEED, use_graph=use_graph, want_steps=want_steps)
    show(f'Handle.diverse_chain {tag}', [out, h.last_pocket_steps], h.chain_status())
    levels = [200, 600, 1000, 0]
    h.set_layout(pb1.num_nodes_phar, pb1.size)
    out = h.score_chain(dev(given1[0]), dev(given1[1]), dev(pb1.x), dev(pb1.one_hot), levels, seed=SEED, pocket_ids=[3, 1, 2], use_graph=use_graph)
    show(f'Handle.score_chain {tag}', out, h.chain_status())
    h.set_layout(pbm.num_nodes_phar, pbm.size)
    out = h.multi_score_chain(dev(givenm[0]), dev(givenm[1]), dev(pbm.x), dev(pbm.one_hot), *groups, levels, seed=SEED, group_ids=[5, 6, 4],
                              want_members=want_steps, use_graph=use_graph)
    show(f'Handle.multi_score_chain {tag}', out, h.chain_status())

# ---- ConditionalDDPM: the ten sampling and the two scoring entries
m = kit.model()
pocket = kit.pocket_dev(pb1)
G, M = len(mc.PAIRS.nph), 2
pockets = [kit.pocket_dev(pbm, [g * M + k for g in range(G)]) for k in range(M)]
nph1, nphm = torch.tensor(NPH1), torch.tensor(mc.PAIRS.nph)


def phar_of(given, nph):
    return {'x': dev(given[0]), 'one_hot': dev(given[1]), 'size': dev(np.asarray(nph, dtype=np.int64)),
            'mask': dev(np.repeat(np.arange(len(nph)), nph))}


phar1, pharm = phar_of(given1, NPH1), phar_of(givenm, mc.PAIRS.nph)
qm = mrc.restraints_of(mrc.PAIRS, pbm)
for use_graph, frames in ((True, 1), (False, 5)):
    m.use_hip_graph = use_graph
    tag = f'graph={int(use_graph)} frames={frames}'
    calls = {
        'sample_given_pocket': lambda: m.sample_given_pocket(pocket, nph1, frames, 5, seed=SEED, pocket_ids=[3, 1, 2]),
        'sample_restrained': lambda: m.sample_restrained(pocket, nph1, q1, clash=rc.CLASH, return_frames=frames, timesteps=5, seed=SEED),
        'sample_diverse': lambda: m.sample_diverse(pocket, nph1, [2, 1], strength=2.0, return_frames=frames, timesteps=5, seed=SEED),
        'sample_given_pockets': lambda: m.sample_given_pockets(pockets, nphm, weights=[1.0, 3.0], return_frames=frames, timesteps=5, seed=SEED,
                                                               group_ids=[5, 6, 4]),
        'sample_restrained_given_pockets': lambda: m.sample_restrained_given_pockets(pockets, nphm, qm, clash=mrc.CLASH, return_frames=frames,
                                                                                     timesteps=5, seed=SEED),
        'inpaint': lambda: m.inpaint(phar1, pocket, given1[2], resamplings=2, return_frames=frames, timesteps=5, seed=SEED),
        'edit': lambda: m.edit(phar1, pocket, fix_coords=given1[2], fix_types=given1[3], start=3, resamplings=2, timesteps=5, seed=SEED),
        'edit_restrained': lambda: m.edit_restrained(phar1, pocket, q1, fix_coords=given1[2], clash=rc.CLASH, timesteps=5, seed=SEED),
        'edit_given_pockets': lambda: m.edit_given_pockets(pharm, pockets, fix_coords=givenm[2], fix_types=givenm[3], start=3, weights=[1.0, 3.0],
                                                           timesteps=5, seed=SEED, group_ids=[5, 6, 4]),
        'edit_restrained_given_pockets': lambda: m.edit_restrained_given_pockets(pharm, pockets, qm, fix_coords=givenm[2], clash=mrc.CLASH,
                                                                                 timesteps=5, seed=SEED),
        'score': lambda: m.score(phar1, pocket, timesteps=4, repeats=2, seed=SEED, pocket_ids=[3, 1, 2], return_levels=frames > 1),
        'score_given_pockets': lambda: m.score_given_pockets(pharm, pockets, weights=[1.0, 3.0], timesteps=4, seed=SEED, group_ids=[5, 6, 4],
                                                             return_levels=frames > 1, return_members=frames > 1),
    }
    for name, call in calls.items():
        show(f'ConditionalDDPM.{name} {tag}', call(), m.last_chain_status)

# ---- PharPocketDDPM: the ten PDB-level entries and the two that score
lm = kit.lightning_model()
f = os.path.join(tempfile.mkdtemp(), 'p.pdb')
with open(f, 'w') as fh:
    fh.write(PDB_TEXT)
one, two = dict(pocket_ids=['A:1', 'A:2', 'A:3', 'A:4']), dict(pocket_ids=[['A:4', 'A:5', 'A:6'], ['A:1', 'A:2', 'A:3']])
bare = [{'kind': 'position', 'point': 2, 'center': (12.0, 7.0, -3.0), 'radius': 1.5, 'k': 2.0},
        {'kind': 'distance', 'points': (0, 1), 'lo': 5.0, 'hi': 7.0, 'k': 1.0}]
points = [('Aromatic', (12.0, 7.0, -3.0)), ('Donor', (13.0, 6.5, -2.0))]
nn = torch.tensor([3, 4, 3])
calls = {
    'generate_phars': lambda: lm.generate_phars(f, 3, num_nodes_phar=nn, timesteps=10, seed=SEED, **one),
    'generate_phars_multi': lambda: lm.generate_phars_multi([f, f], 3, num_nodes_phar=nn, weights=[1.0, 3.0], timesteps=10, seed=SEED, **two),
    'generate_phars_restrained': lambda: lm.generate_phars_restrained(f, 3, bare, num_nodes_phar=4, clash=2.5, timesteps=10, seed=SEED, **one),
    'generate_phars_diverse': lambda: lm.generate_phars_diverse(f, 3, num_nodes_phar=nn, strength=2.0, timesteps=10, seed=SEED, **one),
    'generate_phars_multi_restrained': lambda: lm.generate_phars_multi_restrained([f, f], 3, bare, num_nodes_phar=4, clash=2.5, timesteps=10,
                                                                                  seed=SEED, group_ids=[5, 6, 4], **two),
    'inpaint_phars': lambda: lm.inpaint_phars(f, 3, points, num_nodes_phar=nn, timesteps=10, resamplings=2, seed=SEED, **one),
    'edit_phars': lambda: lm.edit_phars(f, 3, points, keep=['types', 'both'], strength=0.5, timesteps=10, seed=SEED, **one),
    'edit_phars_restrained': lambda: lm.edit_phars_restrained(f, 3, points, bare, num_nodes_phar=4, clash=2.5, timesteps=10, seed=SEED, **one),
    'edit_phars_multi': lambda: lm.edit_phars_multi([f, f], 3, points, strength=0.5, weights=[1.0, 3.0], timesteps=10, seed=SEED, **two),
    'edit_phars_multi_restrained': lambda: lm.edit_phars_multi_restrained([f, f], 3, points, bare, num_nodes_phar=4, clash=2.5, timesteps=10,
                                                                          resamplings=2, seed=SEED, **two),
    'score_phars': lambda: lm.score_phars(f, [points, points[:1]], timesteps=10, seed=SEED, **one),
    'score_phars_multi': lambda: lm.score_phars_multi([f, f], [points, points[:1]], weights=[1.0, 3.0], timesteps=10, seed=SEED,
                                                      return_members=True, **two),
}
for name, call in calls.items():
    show(f'PharPocketDDPM.{name}', call(), lm.ddpm.last_chain_status)
print('done', flush=True)
