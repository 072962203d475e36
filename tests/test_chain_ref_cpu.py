"""chain_ref.run_chain on the CPU: what the loop itself owes beyond its adapters (their tests are test_cond_inpaint_cpu, test_edit_cpu,
test_multi_pocket_cpu, test_multi_edit_cpu, test_restraint_cpu, test_restrained_edit_cpu, test_multi_restraint_cpu,
test_multi_restrained_edit_cpu) - the `groups` and the `guide` parts together, on every key the loop returns (known_steps among them, which
the grouped adapters drop): a restraint's owner is a sample or a group, and the one guidance block serves both.  multi_pocket_cases.PAIRS'
member pockets, two ops.

What these tests do not reach: in the two reductions (groups of one; scale 0) the owner view's gathers - first, qg, spread - are identities or
their result is not added.  The guidance over real groups of several members is pinned by the adapters' own tests (test_multi_restraint_cpu,
test_multi_restrained_edit_cpu: the bite of a later member's atoms, the clipped and unclipped counts, the three reductions) and by the recorded
byte comparison with the loops these adapters had before (profiles/grouped_guide_ref_refactor.txt); the probe test below checks the owner
view's shapes and that op_terms on it gives the op's energy."""
import numpy as np
import pytest
import torch

import multi_pocket_cases as mc
from chain_ref import Groups, op_terms, run_chain
from cmdgen_amd import restraints as rs

K = 2
CLASH = (3.0, 1.0)
GUIDE_KEYS = ('op_energy', 'kind_violation', 'energy', 'max_violation', 'clipped', 'unclipped')


def _restraints(nph):
    """Per owner a position restraint on point 0, a distance window between points 0 and 1 and an exclusion sphere."""
    out = []
    for b in range(len(nph)):
        out.append({'kind': 'position', 'sample': b, 'point': 0, 'center': (1.0, -0.5, 0.5 * b), 'radius': 1.5, 'k': 1.0})
        out.append({'kind': 'distance', 'sample': b, 'points': (0, 1), 'lo': 5.0, 'hi': 7.0, 'k': 1.0})
        out.append({'kind': 'exclusion', 'sample': b, 'center': (0.0, 0.0, 0.0), 'radius': 3.0, 'k': 0.5})
    return rs.records(out, nph)


def _given(nph, with_edit):
    """(phar rows of an edit, its marks) for the owners' point counts: every owner holds the x of its point 1 and the type of its point 0."""
    if not with_edit:
        return None, None
    gen = torch.Generator().manual_seed(11)
    n = int(sum(nph))
    phar = {'x': torch.randn((n, 3), generator=gen) * 2.5, 'one_hot': torch.eye(8)[torch.randint(0, 8, (n,), generator=gen)],
            'size': torch.tensor(nph), 'mask': torch.repeat_interleave(torch.arange(len(nph)), torch.tensor(nph))}
    base = np.cumsum(nph) - np.asarray(nph)
    fx, fh = np.zeros(n, np.float32), np.zeros(n, np.float32)
    fx[base + 1], fh[base] = 1.0, 1.0
    return phar, dict(fix_x=fx, fix_h=fh, start=None, resamplings=1, jump_length=1)


def _run(pb, nph, groups=None, with_edit=False, guide=None, probe=None):
    phar, edit = _given(nph, with_edit)
    gen = torch.Generator().manual_seed(3)
    with torch.no_grad():
        return run_chain(mc.params(), mc.config().as_dict(), mc.pocket_dict(pb), phar=phar, num_nodes_phar=None if with_edit else nph,
                         groups=groups, edit=edit, guide=guide, timesteps=K, noise=lambda shape: torch.randn(shape, generator=gen), probe=probe)


def _guide(rec, scale=1.0):
    return dict(rec=rec, clash_r=CLASH[0], clash_k=CLASH[1], scale=scale, max_shift=rs.DEFAULT_MAX_SHIFT, guide_below=1.0)


def _equal(a, b):
    if a is None or b is None:
        return a is None and b is None
    if isinstance(a, torch.Tensor):
        return torch.equal(a, b)
    return np.array_equal(a, b)


@pytest.mark.parametrize('with_edit', [False, True], ids=['prior', 'edit'])
def test_groups_of_one_with_a_guide_are_the_ungrouped_guided_chain_bit_for_bit(with_edit):
    """Every owner view is then an identity gather: all keys run_chain returns, known_steps and the counts among them."""
    pb = mc.member_pockets(mc.PAIRS)
    nph = [int(n) for n in pb.num_nodes_phar]
    B = len(nph)
    guide = _guide(_restraints(nph))
    want = _run(pb, nph, with_edit=with_edit, guide=guide)
    got = _run(pb, nph, groups=dict(group_sizes=[1] * B, weights=np.ones(B, np.float32)), with_edit=with_edit, guide=guide)
    assert set(got) == set(want) and set(GUIDE_KEYS) < set(want) and 'known_steps' in want
    for k in want:
        assert _equal(got[k], want[k]), k
    assert (want['known_steps'] is not None) == with_edit
    assert float(want['op_energy'].abs().max()) > 0 and want['clipped'] + want['unclipped'] > 0        # the guidance acted


@pytest.mark.parametrize('with_edit', [False, True], ids=['prior', 'edit'])
def test_a_grouped_guided_chain_at_scale_0_is_the_grouped_unguided_chain_bit_for_bit(with_edit):
    """The energy is still evaluated (op_energy is not zero) and nothing is added to the mean: every key the unguided call returns."""
    case = mc.PAIRS
    pb = mc.member_pockets(case)
    groups = dict(group_sizes=case.group_sizes, weights=mc.weights_of(case))
    rec = _restraints(case.nph)
    want = _run(pb, list(case.nph), groups=groups, with_edit=with_edit)
    got = _run(pb, list(case.nph), groups=groups, with_edit=with_edit, guide=_guide(rec, scale=0.0))
    assert set(got) == set(want) | set(GUIDE_KEYS)
    for k in want:
        assert _equal(got[k], want[k]), k
    assert (got['clipped'], got['unclipped']) == (0, 0) and float(got['op_energy'].abs().max()) > 0
    guided = _run(pb, list(case.nph), groups=groups, with_edit=with_edit, guide=_guide(rec))
    assert not torch.equal(guided['xh_phar'], want['xh_phar'])                           # ... and at scale 1 the guidance is not a no-op
    assert guided['op_energy'].shape == (K, len(case.nph)) and guided['energy'].shape == (len(case.nph),)


def test_a_probe_under_groups_is_called_once_per_op_with_owner_shaped_inputs():
    """One copy of the rows per group, the group of a row and of a pocket atom, every group's first member - and op_terms on exactly these
    inputs gives the op's energy."""
    case = mc.PAIRS
    pb = mc.member_pockets(case)
    gr = Groups(case.group_sizes, case.nph)
    rec = _restraints(case.nph)
    n_x = mc.config().as_dict()['norm_values'][0]
    seen = []

    def probe(op, a):
        assert set(a) == {'z', 'P', 'eps_t', 'known', 'fx', 'sigma_t', 'alpha_t', 'com_in', 'pm', 'qm', 'first', 'qg', 't'}
        assert a['z'].shape == a['eps_t'].shape == a['known'].shape == (gr.Nu, 11) and a['fx'].shape == (gr.Nu,)
        assert torch.equal(a['pm'], gr.unique_mask) and torch.equal(a['first'], torch.from_numpy(gr.first))
        assert torch.equal(a['qm'], torch.from_numpy(pb.mask)) and torch.equal(a['qg'], torch.from_numpy(gr.group_of)[a['qm']])
        assert a['P'].shape[0] == len(pb.x) and a['com_in'].shape == (gr.B, 3)
        assert a['t'].shape == a['sigma_t'].shape == a['alpha_t'].shape == (gr.B, 1) and float(a['t'][0]) == (K - op) / K
        terms_in = {k: v for k, v in a.items() if k != 't'}
        seen.append((op, op_terms(rec=rec, clash_r=CLASH[0], clash_k=CLASH[1], n_x=n_x, nd=3, **terms_in)[2]))

    out = _run(pb, list(case.nph), groups=dict(group_sizes=case.group_sizes, weights=mc.weights_of(case)), with_edit=True, guide=_guide(rec),
               probe=probe)
    assert [op for op, _ in seen] == list(range(K))
    assert torch.equal(torch.stack([E for _, E in seen]), out['op_energy']) and out['op_energy'].shape == (K, gr.G)
