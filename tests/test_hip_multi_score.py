"""GPU tests of ConditionalDDPM.score_given_pockets / cmdgen_multi_score_chain: the reductions bit for bit (groups of one member are
cmdgen_score_chain; the member columns are cmdgen_score_chain on the member layout; weights (1, 0, ..) give the first member's row),
the members' copies of z, parity with multi_score_ref on injected noise for a batch that mixes groups of 1, 2 and 3 members, for a
member above 128 nodes and for groups of two, independence of the levels, graphs against eager launches and run to run, device draws,
a group alone against the batch, alternation with the other chains on one handle, the driver entries, refusals and the range guard.

The bound of an entry is test_hip_score.py's: |d error| <= 2 d sqrt(D error) + D d^2 with d = 2e-5 max(1, max |net|), D = rows x columns
(score_ref.error_bound), max |net| the oracle's largest over the GROUP's members: |d eps_bar| <= sum_m w_m |d eps_m| carries the
evaluation bound over to a convex combination.  The categorical term (the model's: multi_score_ref's header) gets rtol 1e-4, atol 1e-3, kl_sums test_score_cpu.close()'s 2e-5.
A (level, group) entry with a pair of any member within 1e-4 A of the cutoff is left out - at most 2 % of a case, none in these cases.

Measured on an MI355X (worst |d error| / bound: group rows / member rows; no entry left out):
  mixed, graph and eager            4.0e-3 / 4.5e-3
  large member, graph and eager     3.1e-3 / 2.8e-3
  pairs, graph and eager            2.9e-3 / 4.3e-3
  bf3 and fp32 engines              mixed 4.9e-3 / 4.5e-3; pairs 2.9e-3 / 3.4e-3 (bf3), 4.3e-3 (fp32)
  a group alone against the batch   0.0 (bit for bit on this layout; not promised)
  range-guarded call (bf16 engine)  3.4e-3
  the categorical term, 'large'     6.648e-3 / 2.6e-5 / 1.983e-3 on the device, the model's term to 7 digits (rtol 1e-4, atol 1e-3)"""
import os

import numpy as np
import pytest
import torch

import multi_pocket_ref as mp
import multi_score_cases as msc
import multi_score_ref as ms
import score_ref
import chain_kit as kit
from chain_kit import dev, handle, lightning_model, model, model_for, philox_noise, pocket_dev, score_entry_ratios, sub_batch
from helpers import GOLDEN, RANGE_NAME, close, g2, overflow_case
from cmdgen_amd import hip_backend, scoring
from cmdgen_amd.synthetic import ModelConfig, make_state_dict, make_pockets

pytestmark = pytest.mark.gpu

LEVELS = np.asarray(msc.levels(), dtype=np.int32)


def level_coef():
    gamma = np.asarray(msc.state_dict()['ddpm.gamma.gamma'], dtype=np.float32)
    cfg = msc.config()
    return scoring.level_coef(scoring.level_table(gamma, cfg.timesteps, 3, cfg.norm_values, LEVELS))


def run_mscore(h, pb, sizes, weights, x, oh, levels=LEVELS, coef=None, noise=None, seed=7, ids=None, use_graph=True, members=True):
    """-> [group_terms, member_terms, kl_sums] as numpy, status key"""
    h.set_layout(pb.num_nodes_phar, pb.size)
    out = h.multi_score_chain(dev(x), dev(oh), dev(pb.x), dev(pb.one_hot), sizes, weights, levels, level_coef=coef, noise=noise, seed=seed,
                              group_ids=ids, want_members=members, use_graph=use_graph)
    st = h.chain_status()
    return [o.cpu().numpy() if o is not None else None for o in out], (st['max_rel_com_error'], st['nan_resets'])


def run_score(h, pb, x, oh, levels=LEVELS, coef=None, noise=None, seed=7, ids=None, use_graph=True):
    h.set_layout(pb.num_nodes_phar, pb.size)
    out = h.score_chain(dev(x), dev(oh), dev(pb.x), dev(pb.one_hot), levels, level_coef=coef, noise=noise, seed=seed, pocket_ids=ids,
                        use_graph=use_graph)
    st = h.chain_status()
    return [o.cpu().numpy() for o in out], (st['max_rel_com_error'], st['nan_resets'])


def phar_rows_for(nph, seed):
    rng = np.random.default_rng(seed)
    nu = int(np.sum(nph))
    return (rng.normal(size=(nu, 3)) * 2.0).astype(np.float32), np.eye(8, dtype=np.float32)[rng.integers(0, 8, size=nu)]


# ------------------------------------------------------------------------------------------------ 1. M = 1
@pytest.mark.parametrize('use_graph', [True, False], ids=['graph', 'eager'])
@pytest.mark.parametrize('inject', [False, True], ids=['device-draws', 'injected'])
@pytest.mark.parametrize('B', [1, 3, 20])
def test_groups_of_one_are_the_scoring_chain_bit_for_bit(B, inject, use_graph):
    pb = make_pockets(B, 'CA', ragged=True, first_index=9500)
    nph = 1 + (np.arange(B, dtype=np.int64) * 3) % 8
    pb.num_nodes_phar[:] = nph
    x, oh = phar_rows_for(nph, B)
    noise = dev(np.random.default_rng(B).normal(size=(len(LEVELS), int(nph.sum()), 11)).astype(np.float32)) if inject else None
    h = handle('half')
    h.set_option('graph_steps', 4)                                    # six levels: one replay of four, two eager steps
    ids = pb.pocket_index
    (terms, kl), st = run_score(h, pb, x, oh, noise=noise, seed=11, ids=ids, use_graph=use_graph)
    (gt, mt, gkl), gst = run_mscore(h, pb, [1] * B, np.ones(B, np.float32), x, oh, noise=noise, seed=11, ids=ids, use_graph=use_graph)
    assert np.array_equal(gt, terms) and np.array_equal(mt, terms) and np.array_equal(gkl, kl)
    assert gst == st and st[1] == 0
    assert np.isfinite(terms).all() and (terms[..., 0] > 0).all() and (terms[-1, :, 2] <= 0).all()


# ------------------------------------------------------------------------------------------------ 2. member columns
def test_member_columns_are_the_scoring_chain_on_the_member_layout_bit_for_bit():
    """MIXED: the single chain over the 20 member samples gets the phar rows and the noise gathered by urow."""
    case = msc.MIXED
    pb, w = msc.member_pockets(case), msc.weights_of(case)
    gr = mp.Groups(case.group_sizes, case.nph)
    x, oh = msc.given_rows(case)
    noise = msc.noise_of(case)
    urow = gr.urow.numpy()
    h = handle('half')
    (gt, mt, gkl), gst = run_mscore(h, pb, case.group_sizes, w, x, oh, noise=noise.cuda())
    (terms, kl), st = run_score(h, pb, x[urow], oh[urow], noise=noise[:, gr.urow].contiguous().cuda())
    assert np.array_equal(mt, terms) and np.array_equal(gkl, kl[gr.first]) and gst == st
    ones = gr.sizes == 1
    assert np.array_equal(gt[:, ones], mt[:, gr.first[ones]])
    assert not np.array_equal(gt[:, ~ones, 0], mt[:, gr.first[~ones], 0])


# ------------------------------------------------------------------------------------------------ 3. weights (1, 0)
def test_first_member_weights_give_the_first_members_row_bit_for_bit():
    case = msc.PAIRS
    pb = msc.member_pockets(case)
    gr = mp.Groups(case.group_sizes, case.nph)
    x, oh = msc.given_rows(case)
    w = np.tile(np.array([1, 0], np.float32), gr.G)
    for noise in (msc.noise_of(case).cuda(), None):
        (gt, mt, _), st = run_mscore(handle('half'), pb, case.group_sizes, w, x, oh, noise=noise)
        assert np.array_equal(gt, mt[:, gr.first]) and st[1] == 0


# ------------------------------------------------------------------------------------------------ 4. the copies of z
@pytest.mark.parametrize('name', ['mixed', 'large'])
def test_every_members_copy_of_z_is_the_first_members(name):
    case = msc.CASES[name]
    pb, w = msc.member_pockets(case), msc.weights_of(case)
    gr = mp.Groups(case.group_sizes, case.nph)
    x, oh = msc.given_rows(case)
    h = handle('half')
    run_mscore(h, pb, case.group_sizes, w, x, oh, seed=5)
    z = np.asarray(h.debug_read('chain_z', gr.Nl * 11)).reshape(gr.Nl, 11)       # after the last level (t = 0)
    assert np.isfinite(z).all() and np.abs(z).max() > 0
    assert np.array_equal(z, z[gr.first_rows().numpy()][gr.urow.numpy()])


# ------------------------------------------------------------------------------------------------ 5. the reference
def entry_ratios(sums, want, netmax, n_rows, keep):
    """score_entry_ratios against the reference's dict of err, err_x [K + 1, n]"""
    K = msc.K
    return score_entry_ratios(sums, want['err'][:K].numpy().astype(np.float64), 0.5 * want['err_x'][K].numpy().astype(np.float64), netmax, n_rows, keep)


def check_case(case, engine, use_graph):
    r = msc.reference(case)
    pb, gr, raw = r['pb'], r['groups'], r['raw']
    h = handle(engine)
    h.set_option('graph_steps', 4)
    (gt, mt, kl), st = run_mscore(h, pb, case.group_sizes, r['weights'], r['x'], r['one_hot'], coef=level_coef(), noise=r['noise'].cuda(),
                                  use_graph=use_graph)
    keep = raw['keep']
    left_out = int((~keep).sum())
    assert left_out <= ms.CAP * keep.size
    K = msc.K
    rg = entry_ratios(gt, raw['group'], raw['group']['netmax'].numpy(), gr.nph, keep)
    rm = entry_ratios(mt, raw['member'], raw['member']['netmax'].numpy(), gr.member_nph, keep[:, gr.group_of])
    print(f'\n[{case.name} {engine} {"graph" if use_graph else "eager"}] worst |d error| / bound: group rows {rg.max():.3e} over {rg.size} '
          f'entries, member rows {rm.max():.3e} over {rm.size}; {left_out} of {keep.size} entries left out')
    assert rg.max() <= 1.0 and rm.max() <= 1.0
    assert (gt[..., 3] == 0).all() and (mt[..., 3] == 0).all() and (gt[:K, :, 2] == 0).all() and (mt[:K, :, 2] == 0).all()
    assert close(kl, raw['kl_sums'].numpy())
    assert st[1] == 0 and st[0] < 1e-2
    return gt, mt


@pytest.mark.parametrize('use_graph', [True, False], ids=['graph', 'eager'])
@pytest.mark.parametrize('name', list(msc.CASES))
def test_matches_the_reference(name, use_graph):
    check_case(msc.CASES[name], 'half', use_graph)


@pytest.mark.parametrize('engine', ['bf3', 'fp32'])
@pytest.mark.parametrize('name', ['mixed', 'pairs'])
def test_other_engines_match_the_reference(name, engine):
    check_case(msc.CASES[name], engine, True)


@pytest.mark.parametrize('name', list(msc.CASES))
def test_categorical_term_matches_the_reference(name):
    """log p(h | z_0) of the t = 0 level against multi_score_ref's 'log_ph', rtol 1e-4, atol 1e-3 as in test_hip_score.py, group and member
    rows.  'log_ph' weights log p by the one-hot itself, as the model does (multi_score_ref's header); score_ref.score_levels' expression
    ('log_ph_oracle', which un-normalises the RAW one-hot) is norm_values[1] = 0.25 times that, and the device must NOT meet it where the
    term is large enough to tell: on 'large', -log p of the three groups is 6.648e-3 / 2.6e-5 / 1.983e-3 on the device and in the model,
    1.662e-3 / 6.6e-6 / 4.96e-4 by the oracle's expression (atol 1e-3).  'mixed' and 'pairs' cannot tell: their terms lie below atol."""
    case = msc.CASES[name]
    r = msc.reference(case)
    gr, raw = r['groups'], r['raw']
    gt, mt = check_case(case, 'half', True)
    K = msc.K
    keep = raw['keep']
    g0, m0 = keep[K], keep[K][gr.group_of]
    want_g, want_m = -raw['group']['log_ph'][K].numpy()[g0], -raw['member']['log_ph'][K].numpy()[m0]
    print(f'\n[{name}] -log p(h | z_0), group rows: device {-gt[K, g0, 2]}  reference {want_g}')
    assert np.allclose(-gt[K, g0, 2], want_g, rtol=1e-4, atol=1e-3)
    assert np.allclose(-mt[K, m0, 2], want_m, rtol=1e-4, atol=1e-3)
    if name == 'large':                                               # the case that tells the two expressions apart
        assert not np.allclose(-gt[K, g0, 2], -raw['group']['log_ph_oracle'][K].numpy()[g0], rtol=1e-4, atol=1e-3)


# ------------------------------------------------------------------------------------------------ 6. independence, reproducibility
def test_levels_are_independent():
    """With injected draws, level k of a 3-level call equals that level of the 6-level call bit for bit."""
    case = msc.MIXED
    pb, w = msc.member_pockets(case), msc.weights_of(case)
    x, oh = msc.given_rows(case)
    noise = msc.noise_of(case).cuda()
    h = handle('half')
    full, _ = run_mscore(h, pb, case.group_sizes, w, x, oh, noise=noise)
    pick = [1, 5, 3]
    part, _ = run_mscore(h, pb, case.group_sizes, w, x, oh, levels=LEVELS[pick], noise=noise[pick].contiguous())
    assert np.array_equal(part[0], full[0][pick]) and np.array_equal(part[1], full[1][pick]) and np.array_equal(part[2], full[2])


def test_captured_equals_eager_run_to_run_and_device_draws():
    """Device draws: the captured chain twice and the eager one, bit for bit; the run that injects cmdgen_debug_noise's numbers for
    (seed, group id, level index, node of the group) is the device-draw run; a changed weight, grouping or level list after a captured
    run gives its own eager run's values (no stale graph)."""
    case = msc.PAIRS
    pb, w = msc.member_pockets(case), msc.weights_of(case)
    x, oh = msc.given_rows(case)
    h = handle('half')
    h.set_option('graph_steps', 4)
    gids = 300 + np.arange(len(case.group_sizes))

    def both(sizes, weights, x, oh, **kw):
        a, sa = run_mscore(h, pb, sizes, weights, x, oh, use_graph=True, **kw)
        b, sb = run_mscore(h, pb, sizes, weights, x, oh, use_graph=False, **kw)
        for u, v in zip(a, b):
            assert np.array_equal(u, v), kw
        assert sa == sb and sa[1] == 0
        return a

    base = both(case.group_sizes, w, x, oh, seed=31, ids=gids)
    assert h.query('chain_graphs') >= 1
    again, _ = run_mscore(h, pb, case.group_sizes, w, x, oh, seed=31, ids=gids)
    injected, _ = run_mscore(h, pb, case.group_sizes, w, x, oh, noise=philox_noise(h, 31, gids, case.nph, range(len(LEVELS))), ids=gids)
    for u, v, t in zip(base, again, injected):
        assert np.array_equal(u, v) and np.array_equal(u, t)
    other_seed = both(case.group_sizes, w, x, oh, seed=32, ids=gids)
    assert not np.array_equal(other_seed[0], base[0])
    w2 = w.copy(); w2[:2] = (0.5, 0.5)
    other_w = both(case.group_sizes, w2, x, oh, seed=31, ids=gids)
    assert not np.array_equal(other_w[0][:, 0], base[0][:, 0]) and np.array_equal(other_w[0][:, 1:], base[0][:, 1:])
    assert np.array_equal(other_w[1], base[1])                         # the members' own rows do not see the weights
    x1, oh1 = phar_rows_for(pb.num_nodes_phar, 6)
    singles = both([1] * len(pb.size), np.ones(len(pb.size), np.float32), x1, oh1, seed=31)
    assert singles[0].shape == (len(LEVELS), len(pb.size), 4)
    fewer = both(case.group_sizes, w, x, oh, seed=31, ids=gids, levels=LEVELS[:4])
    assert np.array_equal(fewer[0], base[0][:4])                       # device draws are keyed by the level index
    back = both(case.group_sizes, w, x, oh, seed=31, ids=gids)
    for u, v in zip(base, back):
        assert np.array_equal(u, v)


def test_a_group_alone_and_inside_a_larger_batch():
    """Group 2 of MIXED (three members, eight points) alone and in the batch of ten groups, same group id, device draws: within the
    bound of the reference comparison of each other (both lie within it of the oracle: twice the bound at most; asserted at once the
    bound), not bit for bit in general, because the evaluation's tile rule differs with the batch - the outcome is printed."""
    case = msc.MIXED
    r = msc.reference(case)
    pb, w, gr = r['pb'], r['weights'], r['groups']
    x, oh = r['x'], r['one_hot']
    g, seed = 2, 43
    gids = 700 + np.arange(gr.G)
    members = list(range(gr.first[g], gr.first[g] + gr.sizes[g]))
    h = handle('half')
    full, st = run_mscore(h, pb, case.group_sizes, w, x, oh, seed=seed, ids=gids)
    sub = sub_batch(pb, members)
    u0 = int(np.sum(case.nph[:g])); rows = slice(u0, u0 + case.nph[g])
    alone, st2 = run_mscore(h, sub, [len(members)], w[members], x[rows], oh[rows], seed=seed, ids=gids[g:g + 1])
    # the oracle at these draws, for max |net| and the margins of this group
    noise = philox_noise(h, seed, gids[g:g + 1], case.nph[g:g + 1], range(len(LEVELS))).cpu()
    pocket = {'x': torch.from_numpy(sub.x), 'one_hot': torch.from_numpy(sub.one_hot), 'size': torch.from_numpy(sub.size),
              'mask': torch.from_numpy(sub.mask)}
    with torch.no_grad():
        raw = ms.score_levels(msc.params(), msc.config().as_dict(), mp.Groups([len(members)], [case.nph[g]]), x[rows], oh[rows], pocket,
                              w[members], LEVELS.tolist(), noise)
    keep = raw['keep']
    part = full[0][:, g:g + 1]
    K = msc.K
    err = raw['group']['err'][:K].numpy().astype(np.float64)
    bound = score_ref.error_bound(err, raw['group']['netmax'][:K].numpy(), case.nph[g], 11)
    d = (np.abs(alone[0][:K, :, 0].astype(np.float64) - part[:K, :, 0]) / bound)[keep[:K]]
    ra = entry_ratios(alone[0], raw['group'], raw['group']['netmax'].numpy(), case.nph[g:g + 1], keep)
    print(f'\n[group alone against the batch] worst |d error| / bound: alone to the oracle {ra.max():.3e}, alone to the batch '
          f'{(d.max() if d.size else 0.0):.3e}; bit for bit: {np.array_equal(alone[0], part)}; error_t alone {alone[0][:K, 0, 0]} '
          f'oracle {err[:, 0]} bound {bound[:, 0]}')
    assert ra.max() <= 1.0 and (d.size == 0 or d.max() <= 1.0)
    assert np.array_equal(alone[2], full[2][g:g + 1])                  # the prior KL sums see the group's rows alone
    assert st[1] == 0 and st2[1] == 0


# ------------------------------------------------------------------------------------------------ 7. alternation
def test_the_chain_alternates_with_the_other_chains_on_one_handle():
    """score_given_pockets, score, sample_given_pockets and edit_given_pockets in turn on one model and one layout (score gets the
    member layout: the group's rows once per member): no chain loses its graph (the count of captured graphs stays) or changes its bits
    over a second round, and every captured result is its eager run's."""
    K, G, M = 5, 2, 2
    ddpm = model()
    ddpm.use_hip_graph = True
    h = ddpm.dynamics.hip_handle()
    h.set_option('graph_steps', 2)
    pb = make_pockets(G * M, 'CA', ragged=True, first_index=9620)
    nph = np.array([5, 8], dtype=np.int64)
    gr = mp.Groups([M] * G, nph)
    x, oh = phar_rows_for(nph, 9)
    pockets = [pocket_dev(pb, [g * M + m for g in range(G)]) for m in range(M)]
    phar = {'x': dev(x), 'one_hot': dev(oh), 'size': dev(nph), 'mask': dev(np.repeat(np.arange(G), nph))}
    urow = gr.urow.numpy()
    phar_m = {'x': dev(x[urow]), 'one_hot': dev(oh[urow]), 'size': dev(gr.member_nph), 'mask': dev(gr.phar_mask.numpy())}
    pocket_m = pocket_dev(pb)
    fix = dev((np.arange(int(nph.sum())) % 2 == 0))

    def round_():
        a = ddpm.score_given_pockets(phar, pockets, weights=[1.0, 3.0], timesteps=K, seed=21, return_levels=True, return_members=True)
        b = ddpm.score(phar_m, pocket_m, timesteps=K, seed=22, return_levels=True)
        c = ddpm.sample_given_pockets(pockets, nph, weights=[1.0, 3.0], timesteps=K, seed=23)
        d = ddpm.edit_given_pockets(phar, pockets, fix_types=fix, weights=[1.0, 3.0], timesteps=K, seed=24)
        return [a['level_sums'], a['member_level_sums'], a['nll'], b['level_sums'], b['nll'], c[0], d[0]]

    first = round_()
    graphs = h.query('chain_graphs')
    assert graphs >= 4
    second = round_()
    assert h.query('chain_graphs') == graphs
    for u, v in zip(first, second):
        assert torch.equal(u, v)
    ddpm.use_hip_graph = False
    eager = round_()
    ddpm.use_hip_graph = True
    for u, v in zip(first, eager):
        assert torch.equal(u, v)


def test_all_conditional_chains_alternate_on_one_handle_and_survive_a_layout_change():
    """Every conditional chain of ConditionalDDPM in turn on one model (the single-pocket ones on the member layout): a second round
    keeps every captured graph and every bit, the eager round gives the captured bits, and after a round on another layout (one point
    fewer in group 0) the first layout's round gives its first bits again - every slot was prepared again with nothing stale in it.
    No evaluation is reset throughout."""
    K, G, M = 5, 2, 2
    ddpm = model()
    ddpm.use_hip_graph = True
    h = ddpm.dynamics.hip_handle()
    h.set_option('graph_steps', 2)
    pb = make_pockets(G * M, 'CA', ragged=True, first_index=9660)
    pockets = [pocket_dev(pb, [g * M + m for g in range(G)]) for m in range(M)]
    pocket_m = pocket_dev(pb)
    centre = [float(v) for v in pb.x[:int(pb.size[0])].mean(axis=0)]
    position = [{'kind': 'position', 'sample': 0, 'point': 1, 'center': centre, 'radius': 1.0, 'k': 1.0}]
    distance = [{'kind': 'distance', 'sample': 2, 'points': (0, 3), 'lo': 2.0, 'hi': 4.0, 'k': 1.0}]

    def rounds_for(nph):
        gr = mp.Groups([M] * G, nph)
        x, oh = phar_rows_for(nph, 9)
        urow = gr.urow.numpy()
        phar = {'x': dev(x), 'one_hot': dev(oh), 'size': dev(nph), 'mask': dev(np.repeat(np.arange(G), nph))}
        phar_m = {'x': dev(x[urow]), 'one_hot': dev(oh[urow]), 'size': dev(gr.member_nph), 'mask': dev(gr.phar_mask.numpy())}
        nph_m = gr.member_nph
        fix, fix_m = dev(np.arange(int(nph.sum())) % 2 == 0), dev(np.arange(len(urow)) % 2 == 0)

        def round_():
            resets = []

            def ran(out):
                resets.append(ddpm.last_chain_status['nan_resets'])
                return out

            a = ran(ddpm.sample_given_pocket(pocket_m, nph_m, timesteps=K, seed=31))
            b = ran(ddpm.sample_restrained(pocket_m, nph_m, position, clash=(2.0, 1.0), timesteps=K, seed=32))
            c = ran(ddpm.inpaint(phar_m, pocket_m, fix_m, timesteps=K, seed=33))
            d = ran(ddpm.edit(phar_m, pocket_m, fix_types=fix_m, start=3, timesteps=K, seed=34))
            e = ran(ddpm.edit_restrained(phar_m, pocket_m, distance, fix_coords=fix_m, start=3, timesteps=K, seed=35))
            f = ran(ddpm.sample_given_pockets(pockets, nph, weights=[1.0, 3.0], timesteps=K, seed=36))
            g = ran(ddpm.edit_given_pockets(phar, pockets, fix_types=fix, weights=[1.0, 3.0], timesteps=K, seed=37))
            s = ran(ddpm.score(phar_m, pocket_m, timesteps=K, seed=38, return_levels=True))
            t = ran(ddpm.score_given_pockets(phar, pockets, weights=[1.0, 3.0], timesteps=K, seed=39, return_levels=True, return_members=True))
            assert resets == [0] * 9, resets
            return [a[0], a[1], b[0], b[4]['energy'], b[4]['max_violation'], c[0], d[0], e[0], e[4]['energy'], f[0], f[1][0], f[1][1], g[0],
                    s['level_sums'], s['nll'], t['level_sums'], t['member_level_sums'], t['nll']]

        return round_

    round_ = rounds_for(np.array([5, 8], dtype=np.int64))
    first = round_()
    graphs = h.query('chain_graphs')
    assert graphs >= 8
    second = round_()
    assert h.query('chain_graphs') == graphs
    for i, (u, v) in enumerate(zip(first, second)):
        assert torch.equal(u, v), i
    ddpm.use_hip_graph = False
    eager = round_()
    ddpm.use_hip_graph = True
    for i, (u, v) in enumerate(zip(first, eager)):
        assert torch.equal(u, v), i
    rounds_for(np.array([4, 8], dtype=np.int64))()
    for i, (u, v) in enumerate(zip(first, round_())):
        assert torch.equal(u, v), i


# ------------------------------------------------------------------------------------------------ 8. the driver
def test_score_given_pockets_with_repeats_and_members():
    """repeats = 2 is the mean of two single runs with the matching draws; the member entries are score's own for that pocket on the
    group's draws; one pocket is score, bit for bit; log_pN is the weighted sum."""
    K, G, M = 5, 3, 2
    ddpm = model()
    ddpm.use_hip_graph = True
    pb = make_pockets(G * M, 'CA', ragged=True, first_index=9640)
    nph = np.array([5, 8, 3], dtype=np.int64)
    x, oh = phar_rows_for(nph, 12)
    pockets = [pocket_dev(pb, [g * M + m for g in range(G)]) for m in range(M)]
    phar = {'x': dev(x), 'one_hot': dev(oh), 'size': dev(nph), 'mask': dev(np.repeat(np.arange(G), nph))}
    noise = torch.from_numpy(np.random.default_rng(8).normal(size=(2, K + 1, int(nph.sum()), 11)).astype(np.float32)).cuda()
    both = ddpm.score_given_pockets(phar, pockets, weights=[1.0, 3.0], timesteps=K, repeats=2, noise=noise, return_levels=True,
                                    return_members=True)
    one = [ddpm.score_given_pockets(phar, pockets, weights=[1.0, 3.0], timesteps=K, noise=noise[r], return_members=True) for r in range(2)]
    for k in ('nll', 'loss_t', 'loss_0_x', 'loss_0_h'):
        assert torch.equal(both[k + '_repeats'], torch.stack([o[k] for o in one])), k
        assert torch.equal(both[k], torch.stack([o[k] for o in one]).double().mean(0).float()), k
    assert both['nll'].shape == (G,) and both['member_nll'].shape == (G, M) and both['level_sums'].shape == (2, K + 1, G, 4)
    assert both['member_level_sums'].shape == (2, K + 1, G, M, 4) and bool(torch.isfinite(both['nll']).all())
    w = torch.tensor([0.25, 0.75], dtype=torch.float64, device='cuda')
    assert torch.equal(both['log_pN'], (both['member_log_pN'].double() * w).sum(1).float())
    # the scalars of (n_phar, n_pocket_m) are score's own for that pocket (the member columns themselves: test 2, on the raw chain)
    for m in range(M):
        s = ddpm.score(phar, pockets[m], timesteps=K, noise=noise[0])
        assert torch.equal(s['log_pN'], both['member_log_pN'][:, m])
    solo = ddpm.score_given_pockets(phar, pockets[:1], timesteps=K, noise=noise[0], return_levels=True, return_members=True)
    s = ddpm.score(phar, pockets[0], timesteps=K, noise=noise[0], return_levels=True)
    for k in s:
        assert torch.equal(s[k], solo[k]), k
    assert torch.equal(solo['member_nll'][:, 0], s['nll'])


def test_score_phars_multi_end_to_end():
    """PharPocketDDPM.score_phars_multi on the synthetic PDB given twice, as two different pockets (29 and 20 residues): the same seed
    gives the same result, candidate i draws with group id i, and with weights (1, 0) every entry is the first pocket's own."""
    m = lightning_model().eval()
    pdb = os.path.join(GOLDEN, 'g7_pocket.pdb')
    ids = [f'A:{i}' for i in range(1, 30)]
    names = list(m.dataset_info['phar_decoder'])
    c0 = [(names[1], (9.0, 2.0, -15.0)), (names[3], (11.5, 4.0, -13.0)), (names[0], (8.0, 5.0, -12.0))]
    c1 = [(names[2], (10.0, 3.0, -14.0)), (names[2], (12.0, 1.0, -16.0))]
    kw = dict(pocket_ids=[ids, ids[:20]], weights=[0.5, 0.5], timesteps=10, seed=5)
    out = m.score_phars_multi([pdb, pdb], [c0, c1], return_members=True, **kw)
    assert out['nll'].shape == (2,) and out['member_nll'].shape == (2, 2) and bool(torch.isfinite(out['nll']).all())
    again = m.score_phars_multi([pdb, pdb], [c0, c1], return_members=True, **kw)
    for k in out:
        assert torch.equal(out[k], again[k]), k
    # candidate i is group i and draws with group id i
    ddpm = m.ddpm
    pockets = [m._pdb_pocket(pdb, 2, ids, None), m._pdb_pocket(pdb, 2, ids[:20], None)]
    direct = ddpm.score_given_pockets(m._candidate_batch([c0, c1]), pockets, weights=[0.5, 0.5], timesteps=10, seed=5, group_ids=[0, 1],
                                      return_members=True)
    for k in out:
        assert torch.equal(out[k], direct[k]), k
    other = ddpm.score_given_pockets(m._candidate_batch([c0, c1]), pockets, weights=[0.5, 0.5], timesteps=10, seed=5, group_ids=[1, 0])
    assert not torch.equal(other['nll'], out['nll'])
    # all the weight on the first of two pockets: the group's terms are that member's (the evaluations of two equal samples of a batch
    # are not promised to be equal bit for bit, so equal pockets with weights (0.5, 0.5) prove less)
    first = m.score_phars_multi([pdb, pdb], [c0, c1], pocket_ids=[ids, ids[:20]], weights=[1.0, 0.0], timesteps=10, seed=5, return_members=True)
    assert torch.equal(first['loss_t'], first['member_loss_t'][:, 0]) and torch.equal(first['loss_0_x'], first['member_loss_0_x'][:, 0])
    assert torch.equal(first['nll'], first['member_nll'][:, 0]) and not torch.equal(first['nll'], first['member_nll'][:, 1])


def test_refusals_leave_the_handle_usable():
    cfg = ModelConfig(hidden_nf=64, n_layers=1, timesteps=500)
    pb = make_pockets(4, 'CA', ragged=True, first_index=9700)
    pb.num_nodes_phar[:] = (3, 3, 5, 5)
    px, poh = dev(pb.x), dev(pb.one_hot)
    h = hip_backend.Handle(cfg.as_dict(), 0)
    h.load_state_dict(make_state_dict(cfg, seed=0))
    h.set_layout(pb.num_nodes_phar, pb.size)
    half = np.full(4, 0.5, np.float32)

    def args(nu):
        return [dev(a) for a in phar_rows_for(np.array([nu]), 1)]

    refused = lambda match, sizes, w, nu=8, levels=(250, 0): kit.refused(              # the message
        h, lambda: h.multi_score_chain(*args(nu), px, poh, sizes, w, list(levels)), match, code=None)

    refused('share one latent', [1, 2, 1], np.array([1, 0.5, 0.5, 1], np.float32), nu=11)     # members 1 and 2 have 3 and 5 points
    refused('sum to 3', [2, 1], np.array([0.5, 0.5, 1, 1], np.float32))
    refused('sizes must be in', [2, 0, 2], half, nu=13)
    refused('sizes must be in', [9], half, nu=3)
    refused('not 1', [2, 2], np.array([0.5, 0.6, 0.5, 0.5], np.float32))
    refused('finite and >= 0', [2, 2], np.array([1.5, -0.5, 0.5, 0.5], np.float32))
    refused('finite and >= 0', [2, 2], np.array([np.nan, 0.5, 0.5, 0.5], np.float32))
    refused(r'levels must be in \[0, 500\]', [2, 2], half, levels=(10, 501, 0))
    refused('levels must be in', [2, 2], half, levels=(-1,))
    refused('null pointer|n_levels=0', [2, 2], half, levels=())       # (an empty list reaches the library as a null pointer)
    gt, mt, kl = h.multi_score_chain(*args(8), px, poh, [2, 2], half, [500, 500, 0], want_members=True)     # any order, repeats allowed
    assert gt.shape == (3, 2, 4) and mt.shape == (3, 4, 4) and kl.shape == (2, 2)
    assert bool(torch.isfinite(gt).all()) and not torch.equal(gt[0], gt[1])
    plain = h.sample_chain(px, poh, 5, seed=3)                        # ... and an ordinary chain follows
    st = h.chain_status()
    assert plain[0].shape == (16, 11) and st['max_rel_com_error'] < 1e-2 and bool(torch.isfinite(plain[0]).all())
    # a sample above the step's 64 KiB of LDS
    h.set_layout(np.array([3, 3], dtype=np.int64), np.array([1100, 30], dtype=np.int64))
    with pytest.raises(hip_backend.CmdgenError, match='64 KiB'):
        h.multi_score_chain(*args(3), torch.zeros((1130, 3), device='cuda'), torch.zeros((1130, 20), device='cuda'), [2], half[:2], [250, 0])
    h.close()
    for extra, msg in ((dict(update_pocket_coords=True), 'joint model'), (dict(no_com_projection=True), 'no_com_projection')):
        c2 = ModelConfig(hidden_nf=64, n_layers=1, timesteps=500, **extra)
        h2 = hip_backend.Handle(c2.as_dict(), 0)
        h2.load_state_dict(make_state_dict(c2, seed=0))
        h2.set_layout(pb.num_nodes_phar, pb.size)
        with pytest.raises(hip_backend.CmdgenError, match=msg):
            h2.multi_score_chain(*args(8), px, poh, [2, 2], half, [250, 0])
        h2.close()


def test_range_guard():
    """test_hip_score.py's range-guard recipe on one target, the samples paired into groups of two: the raw chain on the half engine
    reports reset levels in the flag column (nothing is summed in silently); score_given_pockets warns, re-runs on the bf16 engine and
    meets the parity bound against the oracle."""
    cfg, sd, inp = overflow_case('node')
    nl, npk = g2()[RANGE_NAME + '/num_nodes_phar'].astype(np.int64), g2()[RANGE_NAME + '/pocket_size'].astype(np.int64)
    B = len(nl)
    assert B % 2 == 0
    G, M = B // 2, 2
    nph = np.minimum(nl[0::2], nl[1::2])                               # a group's members share the count: the smaller of the pair
    gr = mp.Groups([M] * G, nph)
    x, oh = phar_rows_for(nph, 13)
    qm = inp['mask_pocket']
    pocket = {'x': torch.from_numpy(inp['xh_pocket'][:, :3].copy()),
              'one_hot': torch.from_numpy(np.round(inp['xh_pocket'][:, 3:] * cfg.norm_values[1]).astype(np.float32)),
              'size': torch.from_numpy(npk), 'mask': torch.from_numpy(qm.copy())}
    com = np.stack([pocket['x'].numpy()[qm == b].mean(0) for b in range(B)])
    x = (x + com[gr.first][gr.unique_mask.numpy()]).astype(np.float32)                      # the given rows near the first pocket of their group
    K, T = 4, cfg.timesteps
    levels = score_ref.level_list(T, K)
    noise = np.random.default_rng(3).normal(size=(K + 1, gr.Nu, 11)).astype(np.float32)
    w = np.tile(np.array([0.5, 0.5], np.float32), G)
    from oracle import ref_cpu
    with torch.no_grad():
        raw = ms.score_levels(ref_cpu.to_torch_params(sd), cfg.as_dict(), gr, x, oh, pocket, w, levels, noise)
    assert torch.isfinite(raw['group']['err']).all() and float(raw['member']['netmax'].min()) > 0, 'the oracle stays finite, no reset'
    # 1. the raw chain on the half engine
    h = hip_backend.Handle(cfg.as_dict(), 0)
    h.load_state_dict(sd)
    h.set_layout(gr.member_nph, npk)
    assert h.half_engine_active()
    h.reset_counters()
    gt, mt, _ = h.multi_score_chain(dev(x), dev(oh), dev(pocket['x'].numpy()), dev(pocket['one_hot'].numpy()), [M] * G, w, np.asarray(levels),
                                    noise=dev(noise), want_members=True)
    st = h.chain_status()
    gt, mt = gt.cpu().numpy(), mt.cpu().numpy()
    print(f'\nraw half-engine chain: {st["nan_resets"]} reset levels, flags {gt[:, 0, 3]}')
    assert st['nan_resets'] >= 1 and st['nan_resets'] == int(gt[:, 0, 3].sum())
    assert np.array_equal(gt[:, :, 3], np.repeat(gt[:, :1, 3], G, axis=1)) and np.array_equal(mt[:, :, 3], np.repeat(gt[:, :1, 3], B, axis=1))
    h.close()
    # 2. the mirror: warning, bf16 re-run, oracle-equal entries
    ddpm = model_for(cfg, sd).eval()
    pockets = [{'x': dev(pocket['x'].numpy()[np.isin(qm, np.arange(m, B, M))]), 'one_hot': dev(pocket['one_hot'].numpy()[np.isin(qm, np.arange(m, B, M))]),
                'size': dev(npk[m::M]), 'mask': dev(np.repeat(np.arange(G), npk[m::M]))} for m in range(M)]
    phar = {'x': dev(x), 'one_hot': dev(oh), 'size': dev(nph), 'mask': dev(gr.unique_mask.numpy())}
    with pytest.warns(RuntimeWarning, match='half matrix engine'):
        out = ddpm.score_given_pockets(phar, pockets, timesteps=K, noise=dev(noise), return_levels=True)
    st = ddpm.last_chain_status
    assert st.get('half_engine_fallback') and st['nan_resets'] == 0
    sums = out['level_sums'][0].cpu().numpy()
    keep = raw['keep']                                                 # (the original recipe keeps all; an entry at the cutoff proves nothing either way)
    err, l0x = raw['group']['err'][:K].numpy().astype(np.float64), 0.5 * raw['group']['err_x'][K].numpy().astype(np.float64)
    r = score_entry_ratios(sums, err, l0x, raw['group']['netmax'].numpy(), nph, keep)
    print(f'guarded score_given_pockets against the oracle: worst ratio {r.max():.3e}, {int((~keep).sum())} of {keep.size} entries at the cutoff')
    assert r.max() <= 1.0 and bool(torch.isfinite(out['nll']).all()) and keep.sum() >= 0.8 * keep.size
