"""The multi-pocket scoring chain on the CPU: the oracle-built model (multi_score_ref) against score_ref where they must coincide
(groups of one; the member columns on the member layout; weights (1, 0, ..) on the first member), the leave-out cap of the GPU cases
from the reference alone, the group assembly of cmdgen_amd/scoring.py, the argument checks of ConditionalDDPM.score_given_pockets and
PharPocketDDPM.score_phars_multi that need no device, and the new entry's binding."""
import ctypes
import os

import numpy as np
import pytest
import torch

import multi_pocket_ref as mp
import multi_score_cases as msc
import multi_score_ref as ms
import score_ref
from helpers import GOLDEN, HIST
from cmdgen_amd import scoring
from cmdgen_amd.synthetic import make_pockets
from helpers import small, sub_pockets

LEVELS = [600, 1000, 0, 200]         # any order; one t = 0 level
NAMES = ('err', 'err_x', 'log_ph_oracle', 'netmax')      # multi_score_ref's name -> score_ref's: its l0 term is 'log_ph_oracle' there
REF_NAME = {'log_ph_oracle': 'log_ph'}


def check_categorical_terms(got, nv1):
    """The model's term against score_ref's expression: one-hot rows with norm_biases[1] = 0, so the oracle's weight of the hot column
    is norm_values[1] where the model's is 1 - the two differ by that factor and by nothing else."""
    for part in ('group', 'member'):
        a, b = got[part]['log_ph'].double(), got[part]['log_ph_oracle'].double()
        assert torch.allclose(a * nv1, b, rtol=1e-6, atol=0) and float(a.abs().max()) > 0


def _given(nph, seed):
    rng = np.random.default_rng(seed)
    nu = int(np.sum(nph))
    return (rng.normal(size=(nu, 3)) * 2.0).astype(np.float32), np.eye(8, dtype=np.float32)[rng.integers(0, 8, size=nu)]


def test_groups_of_one_are_the_scoring_model_exactly():
    cfg, p = small()
    pb = make_pockets(4, 'CA', ragged=True, first_index=9600)
    nph = np.minimum(pb.num_nodes_phar, 8)
    x, oh = _given(nph, 1)
    noise = torch.from_numpy(np.random.default_rng(2).normal(size=(len(LEVELS), int(nph.sum()), 11)).astype(np.float32))
    pocket = sub_pockets(pb, range(4))
    gr = mp.Groups([1, 1, 1, 1], nph)
    phar = {'x': torch.from_numpy(x), 'one_hot': torch.from_numpy(oh), 'size': torch.from_numpy(nph), 'mask': gr.phar_mask}
    with torch.no_grad():
        want = score_ref.score_levels(p, cfg.as_dict(), phar, pocket, LEVELS, noise)
        got = ms.score_levels(p, cfg.as_dict(), gr, x, oh, pocket, np.ones(4, np.float32), LEVELS, noise)
    for k in NAMES:
        w_k = want[REF_NAME.get(k, k)]
        assert torch.equal(got['group'][k], w_k) and torch.equal(got['member'][k], w_k), k
    check_categorical_terms(got, cfg.norm_values[1])
    assert cfg.norm_values[1] != 1                           # (otherwise the two terms could not be told apart here)
    assert torch.equal(got['kl_sums'], want['kl_sums'])
    assert torch.equal(got['z'], want['z']) and torch.equal(got['pocket_x'], want['pocket_x'])
    assert float(want['log_ph'][2].abs().min()) > 0 and not want['log_ph'][[0, 1, 3]].any()


def _mixed_small():
    cfg, p = small()
    pb = make_pockets(5, 'CA', ragged=True, first_index=9630)
    sizes, nph = [2, 1, 2], np.array([5, 8, 3])
    x, oh = _given(nph, 3)
    noise = torch.from_numpy(np.random.default_rng(4).normal(size=(len(LEVELS), int(nph.sum()), 11)).astype(np.float32))
    return cfg, p, sub_pockets(pb, range(5)), mp.Groups(sizes, nph), x, oh, noise


def test_first_member_weights_give_the_first_members_columns():
    cfg, p, pocket, gr, x, oh, noise = _mixed_small()
    w = np.array([1, 0, 1, 1, 0], dtype=np.float32)
    with torch.no_grad():
        got = ms.score_levels(p, cfg.as_dict(), gr, x, oh, pocket, w, LEVELS, noise)
    first = torch.from_numpy(gr.first)
    for k in ('err', 'err_x', 'log_ph', 'log_ph_oracle'):
        assert torch.equal(got['group'][k], got['member'][k][:, first]), k


def test_member_columns_are_the_scoring_model_on_the_member_layout():
    """... with every member given its group's rows and draws; and the group's columns differ from every member's."""
    cfg, p, pocket, gr, x, oh, noise = _mixed_small()
    w = np.array([0.3, 0.7, 1.0, 0.6, 0.4], dtype=np.float32)
    phar, member_noise = ms.member_inputs(gr, x, oh, noise)
    with torch.no_grad():
        got = ms.score_levels(p, cfg.as_dict(), gr, x, oh, pocket, w, LEVELS, noise)
        want = score_ref.score_levels(p, cfg.as_dict(), phar, pocket, LEVELS, member_noise)
    for k in NAMES:
        assert torch.equal(got['member'][k], want[REF_NAME.get(k, k)]), k
    check_categorical_terms(got, cfg.norm_values[1])
    assert torch.equal(got['member_kl_sums'], want['kl_sums']) and torch.equal(got['kl_sums'], want['kl_sums'][gr.first])
    assert torch.equal(got['z'], want['z'])
    # every member's copy of z is its group's first member's
    fr = gr.first_rows()
    assert torch.equal(got['z'], got['z'][:, fr][:, gr.urow])
    two = torch.from_numpy(np.flatnonzero(gr.sizes > 1))
    first = torch.from_numpy(gr.first)
    assert not torch.equal(got['group']['err'][:, two], got['member']['err'][:, first[two]])
    assert torch.equal(got['group']['err'][:, 1], got['member']['err'][:, 2])          # the group of one


@pytest.mark.parametrize('name', list(msc.CASES))
def test_the_cases_leave_out_at_most_the_cap(name):
    r = msc.reference(msc.CASES[name])
    keep, margins = r['raw']['keep'], r['raw']['margins']
    left_out = int((~keep).sum())
    print(f'\n[{name}] smallest margin {margins.min():.2e} A, {left_out} of {keep.size} (level, group) entries inside the band')
    assert keep.shape == (msc.K + 1, r['groups'].G)
    assert left_out <= ms.CAP * keep.size
    assert torch.isfinite(r['raw']['group']['err']).all() and float(r['raw']['member']['netmax'].min()) > 0


def _fake_terms(rng, R, nlev, G, M):
    gt = rng.uniform(0.5, 30.0, size=(R, nlev, G, 4)).astype(np.float32)
    mt = rng.uniform(0.5, 30.0, size=(R, nlev, G, M, 4)).astype(np.float32)
    gt[..., 2] = -np.abs(gt[..., 2]); mt[..., 2] = -np.abs(mt[..., 2])
    gt[..., 3] = 0; mt[..., 3] = 0
    return gt, mt


def test_group_assembly():
    """nll against a float64 sum of the assembly's own entries, log_pN as the weighted sum of assemble's per-member values, the member
    entries as assemble's on the member columns, and M = 1 as assemble itself."""
    from helpers import score_case
    from cmdgen_amd.equivariant_diffusion.en_diffusion import DistributionNodes
    cfg, sd = score_case()[:2]
    T, nd, nv = cfg.timesteps, 3, list(cfg.norm_values)
    gamma = np.asarray(sd['ddpm.gamma.gamma'], dtype=np.float32)
    log_pn = DistributionNodes(HIST)._table(1, torch.device('cpu')).numpy()
    K, R, G, M = 4, 2, 3, 2
    levels = scoring.level_list(T, K)
    rng = np.random.default_rng(0)
    gt, mt = _fake_terms(rng, R, K + 1, G, M)
    kl = rng.uniform(1.0, 9.0, size=(G, 2)).astype(np.float32)
    n_phar, n_pocket = np.array([3, 5, 4]), np.array([[20, 31], [25, 22], [30, 30]])
    w = np.array([[0.25, 0.75], [0.5, 0.5], [1.0, 0.0]], dtype=np.float32)
    out = scoring.assemble_groups(gt, mt, kl, w, gamma, log_pn, T, nd, nv, levels, n_phar, n_pocket)
    per_m = [scoring.assemble(mt[:, :, :, m], kl, gamma, log_pn, T, nd, nv, levels, n_phar, n_pocket[:, m]) for m in range(M)]
    want_pn = sum(w[:, m].astype(np.float64) * per_m[m]['log_pN'].astype(np.float64) for m in range(M))
    assert np.array_equal(out['log_pN'], want_pn.astype(np.float32))
    assert np.array_equal(out['member_log_pN'], np.stack([o['log_pN'] for o in per_m], 1))
    assert not np.array_equal(per_m[0]['log_pN'], per_m[1]['log_pN'])
    f64 = out['level_terms'].astype(np.float64).sum(1) + (out['neg_log_const_0'].astype(np.float64) + out['kl_prior']
                                                          - out['delta_log_px'] - out['log_pN'])[None]
    assert np.allclose(out['nll_repeats'], f64, rtol=1e-6, atol=0)
    assert np.allclose(out['nll'], f64.mean(0), rtol=1e-6, atol=0)
    for m in range(M):
        for k in ('nll', 'loss_t', 'loss_0_x'):
            assert np.array_equal(out['member_' + k][:, m], per_m[m][k]), (k, m)
    # every other scalar is the group's own
    g0 = scoring.assemble(gt, kl, gamma, log_pn, T, nd, nv, levels, n_phar, n_pocket[:, 0])
    for k in ('loss_t', 'loss_0_x', 'loss_0_h', 'neg_log_const_0', 'kl_prior', 'delta_log_px', 'level_terms'):
        assert np.array_equal(out[k], g0[k]), k
    # one pocket: assemble itself
    one = scoring.assemble_groups(gt, None, kl, np.ones((G, 1), np.float32), gamma, log_pn, T, nd, nv, levels, n_phar, n_pocket[:, :1])
    for k in g0:
        assert np.array_equal(one[k], g0[k]), k
    assert 'member_nll' not in one


def test_argument_checks_without_a_device():
    from helpers import bare_model as _model
    from cmdgen_amd.equivariant_diffusion.conditional_model import ConditionalDDPM, SimpleConditionalDDPM
    from cmdgen_amd.equivariant_diffusion.en_diffusion import EnVariationalDiffusion

    def pocket(sizes):
        n = int(sum(sizes))
        return {'x': torch.randn(n, 3), 'one_hot': torch.zeros(n, 20), 'size': torch.tensor(sizes),
                'mask': torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))}
    m = _model(ConditionalDDPM)
    m.dynamics.hip_handle = None                             # every check below raises before a handle is asked for
    a, b = pocket([3, 4]), pocket([5, 2])
    phar = {'x': torch.zeros(5, 3), 'one_hot': torch.zeros(5, 8), 'size': torch.tensor([2, 3]), 'mask': torch.tensor([0, 0, 1, 1, 1])}
    T = m.T
    with pytest.raises(ValueError, match='pockets is empty'):
        m.score_given_pockets(phar, [], timesteps=10)
    with pytest.raises(ValueError, match='at most 8'):
        m.score_given_pockets(phar, [a] * 9, timesteps=10)
    with pytest.raises(ValueError, match='same groups'):
        m.score_given_pockets(phar, [a, pocket([3, 4, 2])], timesteps=10)
    with pytest.raises(ValueError, match='ascending'):
        m.score_given_pockets(phar, [a, dict(b, mask=torch.tensor([1, 1, 0, 0, 0, 0, 0]))], timesteps=10)
    with pytest.raises(ValueError, match='ascending'):
        m.score_given_pockets(dict(phar, mask=torch.tensor([1, 1, 1, 0, 0])), [a, b], timesteps=10)
    with pytest.raises(ValueError, match='phar has 3 samples, pocket 2'):
        m.score_given_pockets(dict(phar, size=torch.tensor([2, 2, 1])), [a, b], timesteps=10)
    with pytest.raises(ValueError, match='divisor'):
        m.score_given_pockets(phar, [a, b], timesteps=T + 1)
    with pytest.raises(ValueError, match='repeats'):
        m.score_given_pockets(phar, [a, b], timesteps=10, repeats=0)
    with pytest.raises(ValueError, match='weights has shape'):
        m.score_given_pockets(phar, [a, b], weights=[1.0, 2.0, 3.0], timesteps=10)
    with pytest.raises(ValueError, match='>= 0'):
        m.score_given_pockets(phar, [a, b], weights=[1.5, -0.5], timesteps=10)
    with pytest.raises(ValueError, match='sum to zero'):
        m.score_given_pockets(phar, [a, b], weights=[[1.0, 1.0], [0.0, 0.0]], timesteps=10)
    with pytest.raises(ValueError, match=r'sum\(size\) rows'):
        m.score_given_pockets(dict(phar, x=torch.zeros(4, 3)), [a, b], timesteps=10)
    with pytest.raises(ValueError, match='noise has shape'):
        m.score_given_pockets(phar, [a, b], timesteps=10, noise=torch.zeros(11, 7, 11))      # member rows instead of one copy per group
    with pytest.raises(NotImplementedError, match='SimpleConditionalDDPM'):
        _model(SimpleConditionalDDPM).score_given_pockets(phar, [a, b], timesteps=10)
    with pytest.raises(NotImplementedError, match='joint'):
        EnVariationalDiffusion.score_given_pockets(m, phar, [a, b])


def test_score_phars_multi_builds_the_groups():
    """PharPocketDDPM.score_phars_multi up to the chain (replaced by a recorder): one group per candidate, one pocket dict per file
    batched over the candidates, and the argument checks raise before the chain is called."""
    from cmdgen_amd.lightning_modules import PharPocketDDPM
    from helpers import _hparams
    model = PharPocketDDPM(**_hparams('CA', 64, 2))
    names = list(model.dataset_info['phar_decoder'])
    pdb, ids = os.path.join(GOLDEN, 'g7_pocket.pdb'), [f'A:{i}' for i in range(1, 30)]
    c0 = [(names[1], (9.0, 2.0, -15.0)), (names[3], (11.5, 4.0, -13.0)), (names[0], (8.0, 5.0, -12.0))]
    c1 = [(names[2], (10.0, 3.0, -14.0)), (names[2], (12.0, 1.0, -16.0))]
    seen = {}

    def recorder(phar, pockets, **kw):
        seen.update(kw, phar=phar, pockets=pockets)
        return {'nll': torch.zeros(len(phar['size']))}
    model.ddpm.score_given_pockets = recorder
    out = model.score_phars_multi([pdb, pdb], [c0, c1], pocket_ids=[ids, ids[:20]], weights=[0.25, 0.75], timesteps=10, seed=5,
                                  return_members=True)
    assert out['nll'].shape == (2,)
    assert seen['phar']['size'].tolist() == [3, 2] and seen['phar']['mask'].tolist() == [0, 0, 0, 1, 1]
    assert seen['phar']['one_hot'].argmax(1).tolist() == [1, 3, 0, 2, 2]
    assert np.allclose(seen['phar']['x'][3].tolist(), (10.0, 3.0, -14.0))
    assert len(seen['pockets']) == 2 and [len(q['size']) for q in seen['pockets']] == [2, 2]
    assert int(seen['pockets'][1]['size'][0]) < int(seen['pockets'][0]['size'][0])
    assert seen['weights'] == [0.25, 0.75] and seen['timesteps'] == 10 and seen['seed'] == 5 and seen['return_members'] is True
    model.ddpm.score_given_pockets = None                    # the checks below raise before the chain
    with pytest.raises(ValueError, match='one per file'):
        model.score_phars_multi([pdb, pdb], [c0], pocket_ids=[ids], timesteps=10)
    with pytest.raises(ValueError, match='no candidates'):
        model.score_phars_multi([pdb, pdb], [], pocket_ids=[ids, ids], timesteps=10)
    with pytest.raises(ValueError, match='at least one point'):
        model.score_phars_multi([pdb, pdb], [c0, []], pocket_ids=[ids, ids], timesteps=10)
    with pytest.raises(ValueError, match='unknown pharmacophore type'):
        model.score_phars_multi([pdb, pdb], [[('Nope', (0.0, 0.0, 0.0))]], pocket_ids=[ids, ids], timesteps=10)


def test_the_new_entry_is_bound():
    from cmdgen_amd import hip_backend
    lib = hip_backend.load_library()
    table = dict((s[0], s) for s in hip_backend.SYMBOLS)
    sig, multi, score = table['cmdgen_multi_score_chain'], table['cmdgen_multi_pocket_chain'][2], table['cmdgen_score_chain'][2]
    assert sig[1] is ctypes.c_int and len(sig[2]) == 19
    # the scoring chain's rows and pockets, the multi-pocket chain's grouping, the scoring chain's levels, draws and seed, the group
    # ids, then the two term outputs, the KL sums, use_graph and the stream
    assert sig[2][:5] == score[:5] and sig[2][5:8] == multi[3:6] and sig[2][8:13] == score[5:10] and sig[2][13] == multi[9]
    assert sig[2][14:17] == [score[11]] * 3 and sig[2][17:] == score[13:]
    assert lib.cmdgen_multi_score_chain.argtypes == sig[2] and lib.cmdgen_multi_score_chain.restype is ctypes.c_int
    assert hasattr(hip_backend.Handle, 'multi_score_chain')
    with open(os.path.join(os.path.dirname(GOLDEN), '..', 'include', 'cmdgen_hip.h')) as f:
        assert 'int cmdgen_multi_score_chain(cmdgen_handle* h' in f.read()
