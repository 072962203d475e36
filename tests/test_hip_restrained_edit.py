"""GPU tests of ConditionalDDPM.edit_restrained / cmdgen_restrained_edit_chain: parity with restrained_edit_ref on injected noise (from the
prior, part-way with jumps, a sample above 128 nodes), the reductions to cmdgen_edit_chain and to cmdgen_restrained_chain bit for bit, graphs
against eager launches and run to run, a shard against the full batch, the held rows, the effect of the guidance, refusals, and the Python
entry points.

Bounds against the reference: z and the pocket after every op, the final x and pocket, energy, max_violation and op_energy within PARITY = 1e-4
relative to max(1, max|.|) (test_restraint_cpu.py's bound), types exact.  A sample with a pair within 1e-4 A of the cutoff at any reference
evaluation is left out (restrained_edit_cases.py: at most 20 % of a case's samples)."""
import os

import numpy as np
import pytest
import torch

import restrained_edit_cases as ec
import chain_kit as kit
from chain_kit import (PARITY, PLAIN, SMALL, check_against_ref, dev, guide, handle, lightning_model, model, pocket_dev, record, run_chain,
                       same, status_key)
from helpers import GOLDEN
from cmdgen_amd import hip_backend
from cmdgen_amd import restraints as rs
from cmdgen_amd.synthetic import ModelConfig, make_state_dict, make_pockets

pytestmark = pytest.mark.gpu

ALL = [ec.MIXED, ec.JUMPS, ec.LARGE]
EDIT = PLAIN + ('chain_z',)                            # what cmdgen_edit_chain shares with the restrained edit chain


def run_redit(h, case, r, rec, noise=None, seed=7, ids=None, use_graph=True, marked=True, start=None, resamplings=None, jump_length=None, **g):
    """The case's restrained edit chain (marked=False: with no mark in either mask; start, resamplings, jump_length: another plan; g: guide()'s)."""
    ph, zero = r['phar'], np.zeros(len(r['fx']), np.float32)
    plan = (case.start if start is None else start, case.r if resamplings is None else resamplings, case.j if jump_length is None else jump_length)
    return run_chain(h, r['pb'], case.K, given=(ph['x'], ph['one_hot'], r['fx'] if marked else zero, r['fh'] if marked else zero), plan=plan,
                     guide=guide(rec, **g), noise=noise, seed=seed, ids=ids, use_graph=use_graph)


def run_edit(h, case, r, **kw):
    """cmdgen_edit_chain on the same arguments"""
    ph = r['phar']
    return run_chain(h, r['pb'], case.K, given=(ph['x'], ph['one_hot'], r['fx'], r['fh']), plan=(case.start, case.r, case.j), **kw)


def sub_batch(case, r, members):
    """The samples `members` of a case as a batch of their own: (case, inputs dict, restraint records)."""
    rows = np.isin(np.repeat(np.arange(len(case.nph)), case.nph), members)
    sub_pb = kit.sub_batch(r['pb'], members)
    sub_case = case._replace(nph=tuple(case.nph[b] for b in members))
    sub_r = dict(pb=sub_pb, phar={'x': r['phar']['x'][rows], 'one_hot': r['phar']['one_hot'][rows]}, fx=r['fx'][rows], fh=r['fh'][rows])
    sub_restraints = [dict(q, sample=members.index(q['sample'])) for q in r['restraints'] if q['sample'] in members]
    return sub_case, sub_r, rs.records(sub_restraints, sub_pb.num_nodes_phar), rows


# ------------------------------------------------------------------------------------------------ 1. against the reference
@pytest.mark.parametrize('use_graph', [True, False], ids=['graph', 'eager'])
@pytest.mark.parametrize('case', ALL, ids=lambda c: c.name)
def test_chain_matches_the_reference(case, use_graph):
    r = ec.reference(case)
    pb, want, keep = r['pb'], r['guided'], r['keep']
    n_steps = ec.plan(case)[0]
    h = handle()
    h.set_option('graph_steps', 2)                                   # replays of two ops and, where n_steps is odd, an eager op
    got, st = run_redit(h, case, r, r['rec'], noise=r['noise'].cuda(), use_graph=use_graph)
    rows, rows_q = keep[np.repeat(np.arange(len(case.nph)), case.nph)], keep[pb.mask]
    assert got.z_steps.shape == want['z_steps'].shape and got.pocket_steps.shape == want['pocket_steps'].shape
    assert got.op_energy.shape == (n_steps, len(case.nph))
    # this kind bounds the final x and pocket by their LARGEST difference, not the RMS of test_hip_restraint.py, and compares the pocket's
    # coordinates alone: the docstring's "within PARITY relative to max(1, max|.|)" for every output
    check_against_ref(f'{case.name} {"graph" if use_graph else "eager"}', got, st, want, rows, rows_q, keep, 'samples', final='max',
                      pocket_cols=slice(0, 3))
    if case.big_sample is not None:
        assert int((pb.size + pb.num_nodes_phar).max()) > 128           # the 1024-thread step ran


# ------------------------------------------------------------------------------------------------ 2. the reductions
@pytest.mark.parametrize('inject', [False, True], ids=['device-draws', 'injected'])
@pytest.mark.parametrize('case', [ec.MIXED, ec.JUMPS], ids=lambda c: c.name)
def test_without_guidance_it_is_edit_chain_bit_for_bit(case, inject):
    """No restraint and r_c = 0, and scale = 0 with the restraints and the clash term present: every output, the chain status and chain_z of
    cmdgen_edit_chain for the same arguments - from the prior, and part-way with resampling and jumps."""
    r = ec.reference(case)
    h = handle()
    h.set_option('graph_steps', 2)
    noise = r['noise'].cuda() if inject else None
    ids = r['pb'].pocket_index
    want, sw = run_edit(h, case, r, noise=noise, seed=11, ids=ids)
    none, s0 = run_redit(h, case, r, None, clash=(0.0, 0.0), noise=noise, seed=11, ids=ids)
    zero, s1 = run_redit(h, case, r, r['rec'], scale=0.0, noise=noise, seed=11, ids=ids)
    same(want, none, EDIT)
    same(want, zero, EDIT)
    assert status_key(sw) == status_key(s0) == status_key(s1) and sw['nan_resets'] == 0
    assert not none[4].any() and not none[5].any()                      # nothing restrains: zero energies
    assert zero[4][:, 0].max() > 0 and zero[5].max() > 0                # scale = 0 still reports them
    guided, _ = run_redit(h, case, r, r['rec'], noise=noise, seed=11, ids=ids)
    assert not np.array_equal(guided[0], want[0])                       # ... and the guidance is not a no-op here


@pytest.mark.parametrize('inject', [False, True], ids=['device-draws', 'injected'])
@pytest.mark.parametrize('case', [ec.MIXED, ec.LARGE], ids=lambda c: c.name)
def test_without_marks_it_is_restrained_chain_bit_for_bit(case, inject):
    """No mark in either mask, from the prior, no jumps, on a handle whose evaluations use their own k_readout: every output of
    cmdgen_restrained_chain, energy_out, op_energy_out, z_steps and pocket_steps included, the chain status and chain_z.  Injected draws: the
    restrained chain reads z_T, the A rows and the decode row of the edit chain's noise."""
    r = ec.reference(case)
    pb = r['pb']
    n_steps = ec.plan(case)[0]
    assert n_steps == case.K and case.start == case.K
    h = handle(options=dict(SMALL, readout_in_coord=0))
    h.set_option('graph_steps', 2)
    h.set_layout(pb.num_nodes_phar, pb.size)
    assert h.query('readout_in_coord') == 0
    noise = r['noise'].cuda() if inject else None
    rows = [0] + [1 + 2 * i for i in range(n_steps)] + [len(r['noise']) - 1]
    want, sw = run_chain(h, pb, case.K, guide=guide(r['rec']), noise=noise[rows].contiguous() if inject else None, seed=13, ids=pb.pocket_index)
    got, sg = run_redit(h, case, r, r['rec'], noise=noise, seed=13, ids=pb.pocket_index, marked=False)
    same(want, got)
    assert status_key(sw) == status_key(sg) and sw['nan_resets'] == 0
    assert want[4][:, 0].max() > 0 and want[5].max() > 0


def test_guide_below_zero_equals_scale_zero():
    case = ec.MIXED
    r = ec.reference(case)
    h = handle()
    a, sa = run_redit(h, case, r, r['rec'], guide_below=0.0, seed=51)
    b, sb = run_redit(h, case, r, r['rec'], scale=0.0, seed=51)
    same(a, b)
    assert status_key(sa) == status_key(sb)
    # ... and a threshold between two ops guides only the ops at or below it: t / T = 1, 5/6, 4/6 unguided, 3/6 .. 1/6 guided
    part, _ = run_redit(h, case, r, r['rec'], guide_below=0.5, seed=51)
    full, _ = run_redit(h, case, r, r['rec'], seed=51)
    assert np.array_equal(part[2][:3], b[2][:3]) and not np.array_equal(part[2][3], b[2][3]) and not np.array_equal(part[2][0], full[2][0])


# ------------------------------------------------------------------------------------------------ 3. graphs, run to run
def test_runs_repeat_and_a_changed_key_prepares_the_slot_again():
    """Device draws on the jumps case: A captured twice and eager, bit for bit; then other restraints, another scalar, another start and
    another plan, each equal to its eager run; then A again - A's first result."""
    case = ec.JUMPS
    r = ec.reference(case)
    h = handle()
    h.set_option('graph_steps', 2)
    a, sa = run_redit(h, case, r, r['rec'], seed=31)
    assert h.query('chain_graphs') >= 1
    a2, sa2 = run_redit(h, case, r, r['rec'], seed=31)
    e, se = run_redit(h, case, r, r['rec'], seed=31, use_graph=False)
    same(a, a2)
    same(a, e)
    assert status_key(sa) == status_key(sa2) == status_key(se) and sa['nan_resets'] == 0
    other = [dict(q) for q in r['restraints']]
    for q in other:
        if q['kind'] == 'position':
            q['center'] = tuple(v + 2.0 for v in q['center'])
    rec_b = rs.records(other, case.nph)
    for name, kw in (('restraint', dict(rec=rec_b)), ('scalar', dict(clash=(ec.CLASH[0], 2.0))), ('start', dict(start=5)),
                     ('plan', dict(resamplings=1, jump_length=1))):
        kw = dict(kw)
        rec = kw.pop('rec', r['rec'])
        b, _ = run_redit(h, case, r, rec, seed=31, **kw)
        b_eager, _ = run_redit(h, case, r, rec, seed=31, use_graph=False, **kw)
        assert b[2].shape != a[2].shape or not np.array_equal(a[2], b[2]), name
        same(b, b_eager)
        back, sb = run_redit(h, case, r, r['rec'], seed=31)
        same(a, back)
        assert status_key(sa) == status_key(sb)


# ------------------------------------------------------------------------------------------------ 4. a shard
def test_a_shard_gives_the_full_batchs_rows():
    """Samples 2..5 of the mixed case alone (one without a mark, one with types held, the bare one, one with a held point), with their pocket
    ids and their restraints renumbered, device draws: the rows of the full batch within the parity bound (not bit for bit: the tile rule
    differs with the batch size)."""
    case = ec.MIXED
    r = ec.reference(case)
    pb = r['pb']
    members = [2, 3, 4, 5]
    h = handle()
    full, _ = run_redit(h, case, r, r['rec'], seed=41, ids=pb.pocket_index)
    xf, ef = full[0], full[4]
    sub_case, sub_r, sub_rec, rows = sub_batch(case, r, members)
    sub, _ = run_redit(h, sub_case, sub_r, sub_rec, seed=41, ids=sub_r['pb'].pocket_index)
    xsub, esub = sub[0], sub[4]
    diff = float(np.abs(xsub[:, :3] - xf[rows, :3]).max())
    bound = PARITY * max(1.0, float(np.abs(xf[rows, :3]).max()))
    print(f'\n[shard] max |dx| {diff:.3e} A, bound {bound:.3e}; energies {esub[:, 0]} / {ef[members, 0]}')
    assert diff <= bound
    assert np.array_equal(xsub[:, 3:], xf[rows, 3:])
    assert np.all(np.abs(esub - ef[members]) <= PARITY * np.maximum(1.0, np.abs(ef[members])))


# ------------------------------------------------------------------------------------------------ 5. the held rows
def test_held_rows_follow_the_given_points():
    """The sample without a restraint receives no displacement (no clash term here): its rows, the x-held ones among them, are
    cmdgen_edit_chain's bit for bit at every saved step - in a batch whose other sample is restrained and guided but has nothing free to move
    (the bare sample beside the single held point, with its exclusion sphere and a position restraint it violates by 3 A: a gradient, and no
    displacement), so that both chains evaluate the network on the same inputs.

    In the full mixed batch the same holds bit for bit at the first saved step only.  From the second op on the restrained samples have moved,
    their radius graphs have other edge counts, and the evaluation's edge tiles - which run over the whole batch's edge list and add a
    receiver's per-tile partial sums (test_hip_edit.py, test_equal_masks_from_the_prior_equal_inpaint_chain, says when that is order-free) -
    split the bare sample's edges elsewhere: its z then differs from cmdgen_edit_chain's in the last bits (measured on an MI355X: 0 at the
    first saved step, at most 6.0e-8 over the other five; up to 4.8e-7 when another sample of the batch is made the bare one).  That is the
    existing evaluation's rounding, not the step kernel's: there the rows are held to the parity bound.

    On the restrained samples the x-held rows of z agree with the reference's noised known rows (moved into the step's frame) within the
    parity bound."""
    case = ec.MIXED
    r = ec.reference(case)
    h = handle()
    noise = r['noise'].cuda()
    pm = np.repeat(np.arange(len(case.nph)), case.nph)
    fx = r['fx'] != 0
    bare = pm == case.bare
    assert (fx & bare).any() and (~fx & bare).any()
    # the bare sample beside a guided one, nothing free to move
    sub_case, sub_r, sub_rec, rows = sub_batch(case, r, [1, case.bare])
    assert len(sub_rec) == 1 and int(sub_rec['sample'][0]) == 0 and bool(sub_r['fx'][0])
    away = tuple(float(v) for v in sub_r['phar']['x'][0].numpy() + np.array([4.0, 0.0, 0.0], dtype=np.float32))
    sub_rec = np.concatenate([sub_rec, rs.records([{'kind': 'position', 'sample': 0, 'point': 0, 'center': away, 'radius': 1.0, 'k': 1.0}],
                                                  sub_case.nph)])
    sub_noise = noise[:, torch.from_numpy(rows).cuda()].contiguous()
    for inject in (sub_noise, None):
        got, sg = run_redit(h, sub_case, sub_r, sub_rec, clash=(0.0, 0.0), noise=inject, seed=61)
        want, sw = run_edit(h, sub_case, sub_r, noise=inject, seed=61)
        same(want, got, EDIT)
        assert status_key(sg) == status_key(sw)
        assert np.all(np.abs(got[5][:, 0] - 4.5) <= PARITY * 4.5) and not got[5][:, 1].any()     # 0.5 k v^2 at the held point's given position, op after op
    # the full batch
    got, _ = run_redit(h, case, r, r['rec'], clash=(0.0, 0.0), noise=noise)
    want, _ = run_edit(h, case, r, noise=noise)
    assert np.array_equal(got[2][0][bare], want[2][0][bare])                       # the first saved step: same evaluation inputs
    assert np.array_equal(got[3][0][r['pb'].mask == case.bare], want[3][0][r['pb'].mask == case.bare])
    drift = [float(np.abs(got[2][k][bare] - want[2][k][bare]).max()) for k in range(got[2].shape[0])]
    print(f'\n[held rows] the bare sample in the full batch against edit_chain, max |dz| per saved step: {drift}')
    assert max(drift) <= PARITY * max(1.0, float(np.abs(want[2][:, bare]).max()))
    assert not np.array_equal(got[2][:, pm == 0], want[2][:, pm == 0])             # (a restrained sample does move)
    full, _ = run_redit(h, case, r, r['rec'], noise=noise)
    known = r['guided']['known_steps'].numpy()
    held = fx & r['keep'][pm] & (pm != case.bare)
    assert held.sum() >= 4 and len(set(pm[held])) >= 3                             # several held rows, on several samples
    worst = max(float(np.abs(full[2][k][held, :3] - known[k][held]).max()) / (PARITY * max(1.0, float(np.abs(known[k][held]).max())))
                for k in range(len(known)))
    print(f'[held rows] worst ratio to the parity bound against the noised known rows: {worst:.3f}')
    assert worst <= 1.0


# ------------------------------------------------------------------------------------------------ 6. the effect
def test_guidance_lowers_the_energy_of_every_restrained_sample_with_a_free_point():
    case = ec.MIXED
    r = ec.reference(case)
    h = handle()
    noise = r['noise'].cuda()
    g, _ = run_redit(h, case, r, r['rec'], noise=noise)
    u, _ = run_redit(h, case, r, r['rec'], scale=0.0, noise=noise)
    print(f'\n[effect] final energy unguided {u[4][:, 0]}\n         guided   {g[4][:, 0]}\n         largest violation (A) unguided {u[4][:, 1]}\n'
          f'         guided   {g[4][:, 1]}')
    sel = list(ec.EFFECT_SAMPLES)
    assert np.all(g[4][sel, 0] <= u[4][sel, 0])


# ------------------------------------------------------------------------------------------------ 7. refusals
def test_refusals_leave_the_handle_usable():
    cfg = ModelConfig(hidden_nf=64, n_layers=1, timesteps=500)
    pb = make_pockets(3, 'CA', ragged=True, first_index=9700)
    pb.num_nodes_phar[:] = (3, 1, 5)
    px, poh = dev(pb.x), dev(pb.one_hot)
    phx, phoh = torch.zeros((9, 3), device='cuda'), torch.zeros((9, cfg.phar_nf), device='cuda')
    fx = torch.tensor([1.0, 0, 0, 1, 1, 0, 0, 0, 0], device='cuda')
    h = hip_backend.Handle(cfg.as_dict(), 0)
    h.load_state_dict(make_state_dict(cfg, seed=0))
    h.set_layout(pb.num_nodes_phar, pb.size)

    refused = lambda match, rec=None, K=5, **kw: kit.refused(                          # the message
        h, lambda: h.restrained_edit_chain(px, poh, phx, phoh, fx, fx, K, restraints=rec, **kw), match, code=None)

    # what cmdgen_restrained_chain refuses: one per argument class
    refused('unknown kind', record(kind=3))
    refused('outside the layout', record(sample=3))
    refused('point 1, sample 1 has 1 points', record(sample=1, i=1))
    refused('i == j', record(kind=1, sample=2, i=2, j=2, a=1.0, b=2.0))
    refused('lo=3 > hi=2', record(kind=1, sample=2, i=0, j=1, a=3.0, b=2.0))
    refused('radius', record(kind=2, a=np.nan))
    refused('k=', record(k=-0.5))
    refused('non-finite centre', record(c=(0.0, np.nan, 0.0)))
    refused('scale', record(), scale=-1.0)
    refused('clash_radius', record(), clash_radius=-1.0)
    refused('max_shift', record(), max_shift=0.0)
    refused('guide_below', record(), guide_below=1.5)
    refused('more than 256 restraints', np.concatenate([record(kind=2, sample=1)] * 257))
    # what cmdgen_edit_chain refuses
    refused('timesteps', record(), K=501)
    refused('start', record(), start=6)
    refused('start', record(), start=0)
    refused('resamplings', record(), resamplings=0)
    refused('jump_length', record(), jump_length=0)
    n_steps, n_draws = h.edit_plan(5, 5, 2, 2)
    refused('noise holds', record(), resamplings=2, jump_length=2, noise=torch.zeros((n_draws - 1, 9, 11), device='cuda'))
    good = h.restrained_edit_chain(px, poh, phx, phoh, fx, fx, 5, restraints=record(), clash_radius=3.0, clash_k=1.0, seed=3)
    plain = h.edit_chain(px, poh, phx, phoh, fx, fx, 5, seed=3)             # ... and an ordinary chain follows
    st = h.chain_status()
    assert good[0].shape == plain[0].shape == (9, 11) and good[3].shape == (3, 2) and st['max_rel_com_error'] < 1e-2
    assert all(bool(torch.isfinite(t).all()) for t in (good[0], good[3], plain[0]))
    # a sample beyond the step's 64 KiB of LDS (92 B per node at phar_nf 8): refused before anything is launched
    h.set_layout([3], [800])
    with pytest.raises(hip_backend.CmdgenError, match='803 nodes'):
        h.restrained_edit_chain(torch.zeros((800, 3), device='cuda'), torch.zeros((800, cfg.residue_nf), device='cuda'),
                                torch.zeros((3, 3), device='cuda'), torch.zeros((3, cfg.phar_nf), device='cuda'),
                                torch.zeros(3, device='cuda'), torch.zeros(3, device='cuda'), 5, restraints=record())
    h.close()
    for flag, match in (('update_pocket_coords', 'joint model'), ('no_com_projection', 'no_com_projection')):
        ocfg = ModelConfig(hidden_nf=64, n_layers=1, timesteps=500, **{flag: True})
        other = hip_backend.Handle(ocfg.as_dict(), 0)
        other.load_state_dict(make_state_dict(ocfg, seed=0))
        other.set_layout(pb.num_nodes_phar, pb.size)
        with pytest.raises(hip_backend.CmdgenError, match=match):
            other.restrained_edit_chain(px, poh, phx, phoh, fx, fx, 5, restraints=record())
        other.close()


# ------------------------------------------------------------------------------------------------ 8. the Python entry points
def test_edit_restrained_returns_the_chains_result():
    """ConditionalDDPM.edit_restrained on the jumps case: the chain's outputs (bit for bit the binding's, same tables and draws), and scale = 0
    as ConditionalDDPM.edit."""
    case = ec.JUMPS
    r = ec.reference(case)
    pb = r['pb']
    ddpm = model()
    ddpm.use_hip_graph = True
    pocket = pocket_dev(pb)
    phar = {k: v.cuda() for k, v in r['phar'].items()}
    noise = r['noise'].cuda()
    kw = dict(fix_coords=r['fx'], fix_types=r['fh'], start=case.start, resamplings=case.r, jump_length=case.j, timesteps=case.K, noise=noise)
    x, q, pm, qm, info = ddpm.edit_restrained(phar, pocket, r['restraints'], clash=ec.CLASH, scale=ec.SCALE, max_shift=ec.MAX_SHIFT, **kw)
    want, _ = run_redit(ddpm.dynamics.hip_handle(), case, r, r['rec'], noise=noise)
    assert np.array_equal(x.cpu().numpy(), want[0]) and np.array_equal(q.cpu().numpy(), want[1])
    assert np.array_equal(info['energy'].cpu().numpy(), want[4][:, 0]) and np.array_equal(info['max_violation'].cpu().numpy(), want[4][:, 1])
    assert set(info) == {'energy', 'max_violation'} and pm.shape == (sum(case.nph),)
    plain = ddpm.edit(phar, pocket, **kw)
    off = ddpm.edit_restrained(phar, pocket, r['restraints'], clash=ec.CLASH, scale=0.0, **kw)
    assert torch.equal(off[0], plain[0]) and torch.equal(off[1], plain[1])
    with pytest.raises(ValueError, match=r'restraints\[0\]'):
        ddpm.edit_restrained(phar, pocket, [{'kind': 'position', 'sample': 1, 'point': 1, 'center': (0, 0, 0), 'radius': 1, 'k': 1}], **kw)


def test_edit_phars_restrained_end_to_end():
    """PharPocketDDPM.edit_phars_restrained on the g7 pocket: three given points kept, two grown under a distance window from point 0 and a
    position restraint; per-sample point lists in the PDB's frame with the given points where they were, the two diagnostics, the same seed
    the same result, and less energy than the unguided edit on the same draws."""
    m = lightning_model()
    pdb = os.path.join(GOLDEN, 'g7_pocket.pdb')
    ids = [f'A:{i}' for i in range(1, 30)]
    names = list(m.dataset_info['phar_decoder'])
    phars = [(names[1], (9.0, 2.0, -15.0)), (names[3], (11.5, 4.0, -13.0)), (names[1], (7.0, 5.0, -12.0))]
    query = [{'kind': 'distance', 'points': (0, 3), 'lo': 5.0, 'hi': 7.0, 'k': 1.0},
             {'kind': 'position', 'point': 4, 'center': (10.0, 3.0, -14.0), 'radius': 2.0, 'k': 1.0}]
    kw = dict(pocket_ids=ids, num_nodes_phar=5, clash=3.0, timesteps=50, seed=5)
    out, info = m.edit_phars_restrained(pdb, 3, phars, query, **kw)
    assert [len(s) for s in out] == [5, 5, 5] and tuple(info['energy'].shape) == tuple(info['max_violation'].shape) == (3,)
    assert all(name in names and len(xyz) == 3 for s in out for name, xyz in s)
    for s in out:                                                          # the kept points: their types, and their positions within 0.1 A
        assert [n for n, _ in s[:3]] == [n for n, _ in phars]              # (test_hip_edit.py's bound for held coordinates)
        assert max(np.linalg.norm(np.asarray(got) - np.asarray(xyz)) for (_, xyz), (_, got) in zip(phars, s)) <= 0.1
    out2, info2 = m.edit_phars_restrained(pdb, 3, phars, query, **kw)
    assert out == out2 and torch.equal(info['energy'], info2['energy'])
    off, info0 = m.edit_phars_restrained(pdb, 3, phars, query, scale=0.0, **kw)
    plain = m.edit_phars(pdb, 3, phars, keep='both', pocket_ids=ids, num_nodes_phar=5, timesteps=50, seed=5)
    assert off == plain                                                    # scale = 0 is edit_phars
    print(f'\n[edit_phars_restrained] energy {info["energy"].tolist()} against unguided {info0["energy"].tolist()}')
    assert float(info['energy'].sum()) < float(info0['energy'].sum())
