"""CPU suite of the full-atom layout (tests/large_layout_ref.py) that test_hip_large_layout.py runs on the GPU: the layout has the
properties it was chosen for, every committed seed meets its margin condition on the oracle's own run, and the CPU models the GPU
tests compare with (score_ref, cond_inpaint_ref, edit_ref) keep, at this size, the identities their docstrings claim."""
import numpy as np
import pytest
import torch

import large_layout_ref as L
import score_ref
from cond_inpaint_ref import cond_inpaint, inpaint_plan
from edit_ref import cond_edit
import helpers
from helpers import NoiseTape
from oracle import ref_cpu
from rule_sweep_ref import MARGIN, CHAIN_CAP


def test_layout_covers_what_it_was_chosen_for():
    lay = L.build()
    pb = lay['pb']
    n = pb.size + pb.num_nodes_phar
    assert len(n) == 5
    assert 128 in n and 129 in n                      # both sides of max_n > 128 (a sample alone); the batch itself is on the far side
    assert n.max() > 128
    assert (pb.size > 256).any()                      # a second trip of the 256-row loops
    assert (pb.num_nodes_phar > 64).any()             # ... and of the 64-row ones over phar rows
    assert (pb.num_nodes_phar == 1).sum() == 1        # a single point: sub_d = 0, its centre of mass is itself
    assert 250 <= pb.size[2] <= 450 and pb.num_nodes_phar[2] == 15
    assert pb.one_hot.shape[1] == 11                  # residue_nf = 11: pocket rows of width 14
    deg = L.max_degree(np.concatenate([lay['phar_x'], pb.x]), np.concatenate([lay['pm'], pb.mask]))
    print('nodes per sample', n.tolist(), 'maximum degree', deg)
    assert deg >= 64
    # the histogram covers every (phar, pocket) size of the layout
    assert all(L.HIST[a, b] > 0 for a, b in zip(pb.num_nodes_phar, pb.size))
    # a sample alone is the sample of the batch
    for k in range(L.B):
        one = L.build(samples=[k])
        a, b = L.rows_of(lay, k)
        assert np.array_equal(one['phar_x'], lay['phar_x'][a]) and np.array_equal(one['pb'].x, lay['pb'].x[b])
        assert np.array_equal(one['phar_one_hot'], lay['phar_one_hot'][a]) and one['ids'][0] == lay['ids'][k]
    # the fixed / free split of the inpainting case falls inside a wavefront's 64 rows of sample 3, and every kind of sample is there
    f = L.fixed_rows(lay)
    s = [L.rows_of(lay, k)[0] for k in range(L.B)]
    assert f[s[0]].sum() == 0 and f[s[1]].all() and 0 < f[s[2]].sum() < 15 and f[s[4]].all()
    assert f[s[3]][:65].all() and f[s[3]][65:].sum() == 0
    fx, fh = L.edit_masks(lay)
    assert (fx != fh).any() and ((fx + fh)[s[2]] == 0).all() and ((fx != 0) & (fh != 0)).any()


def test_the_bands_are_the_owners():
    assert L.SCORE_BAND == helpers.SCORE_BAND == 1e-4 and L.CHAIN_BAND == helpers.CHAIN_BAND == 2e-5
    assert MARGIN == 1e-4 and L.MAX_LEFT_OUT == int(CHAIN_CAP * L.B) == 1


def test_single_evaluation_margins_leave_no_sample_out():
    m = L.layout_margins(L.build())
    print('first_index', L.FIRST_INDEX, 'margins', m)
    assert (m >= MARGIN).all()


@pytest.mark.parametrize('name', sorted(L.SINGLE_CASES))
def test_loss_case_margins_leave_no_sample_out(name):
    """the evaluations of a loss case run on noised positions: their margins come from the oracle's own run"""
    res = L.SINGLE_CASES[name]()
    m = res['margins']
    assert m.shape == (2 if name.endswith('eval') else 1, L.B)
    print(name, 'seed', L.SEEDS[name], 'min margin per evaluation', m.min(axis=1))
    assert L.case_condition(name, m)
    assert 0.0 in res['t_int'] and float(L.T) in res['t_int']


def test_score_margins_leave_no_entry_out():
    res = L.oracle_score()
    m = res['margins']
    assert m.shape == (L.SCORE_K + 1, L.B)
    inside = int((m < L.SCORE_BAND).sum())
    print('score seed', L.SEEDS['score'], 'entries inside the band', inside, 'of', m.size, 'min margin', float(m.min()))
    assert inside <= L.SCORE_CAP * m.size
    assert inside == 0


@pytest.mark.parametrize('name', sorted(L.CHAIN_CASES))
def test_chain_margins_leave_no_sample_out(name):
    res = L.CHAIN_CASES[name]()
    m = res['margins']
    assert m.shape == (res['n_steps'] + 1, L.B)
    kept = L.kept_from(m)
    print(name, 'seed', L.SEEDS[name], 'evaluations', len(m), 'min margin per sample', m.min(axis=0))
    assert (~kept).sum() <= L.MAX_LEFT_OUT
    assert kept.all()


# ----------------------------------------------------------------------------- the CPU models at this size
def test_score_ref_with_one_level_is_ddpm_forward():
    cfg, lay = L.config(), L.build()
    phar, pocket = L.dicts(lay)
    p = L.params_of(cfg)
    noise = L.oracle_score()['noise'][[2, L.SCORE_K]]
    with torch.no_grad():
        got = score_ref.score(p, cfg.as_dict(), phar, pocket, 1, noise, L.HIST)
        terms = ref_cpu.ddpm_forward(p, cfg.as_dict(), phar, pocket, torch.full((L.B, 1), float(L.T)),
                                     [torch.from_numpy(noise[0]), torch.from_numpy(noise[1])], False, L.HIST)
        nll = ref_cpu.nll_from_terms(terms, cfg.as_dict(), phar['size'], pocket['size'], False)
    assert torch.equal(got['raw']['err'][0], terms[1])
    assert torch.equal(got['loss_0_x'], terms[4]) and torch.equal(got['loss_0_h'], terms[6])
    assert torch.equal(got['kl_prior'], terms[8]) and torch.equal(got['neg_log_const_0'], terms[7])
    assert torch.equal(got['nll'], nll) and bool(torch.isfinite(nll).all())
    assert float(got['raw']['z'][0][L.rows_of(lay, 4)[0], :3].abs().max()) == 0.0             # the single point: z.x is 0 after the projection


def test_cond_inpaint_without_fixed_rows_is_the_plain_sampler_bit_for_bit():
    cfg, lay = L.config(), L.build()
    phar, pocket = L.dicts(lay)
    p = L.params_of(cfg)
    K = 3
    noise = torch.randn((inpaint_plan(1, 1, K)[1], len(lay['pm']), 11), generator=torch.Generator().manual_seed(1)).numpy()
    with torch.no_grad():
        a = cond_inpaint(p, cfg.as_dict(), phar, pocket, np.zeros(len(lay['pm']), np.float32), 1, 1, K, noise=NoiseTape(noise))
        plain = np.concatenate([noise[:1], noise[1:1 + 2 * K:2], noise[-1:]])       # draw 0, the A draws, the decode draw
        b = ref_cpu.sample_given_pocket(p, cfg.as_dict(), pocket, lay['pb'].num_nodes_phar, timesteps=K, noise=NoiseTape(plain))
    for u, v in zip(a, b):
        assert torch.equal(u, v)


def test_cond_edit_with_equal_masks_from_the_prior_is_cond_inpaint():
    res = L.oracle_inpaint()
    cfg, lay = res['cfg'], res['lay']
    phar, pocket = L.dicts(lay)
    K, r, j = L.INPAINT['K'], L.INPAINT['r'], L.INPAINT['j']
    with torch.no_grad():
        out = cond_edit(L.params_of(cfg), cfg.as_dict(), phar, pocket, res['fixed'], res['fixed'], K, r, j, K, noise=NoiseTape(res['noise']),
                        return_steps=True)
    assert np.array_equal(out[0].numpy(), res['want'][0]) and np.array_equal(out[1].numpy(), res['want'][1])
    assert np.array_equal(out[4].numpy(), res['z_steps']) and np.array_equal(out[5].numpy(), res['p_steps'])
