"""CPU suite of ConditionalDDPM.score: the CPU model (tests/score_ref.py) against the G21 vectors recorded from the reference's own
forward (tests/golden/make_golden_score.py), its reduction to ref_cpu.ddpm_forward at one level, the host mirror's level table and
assembly (cmdgen_amd/scoring.py), and the public entries' host-side checks.

Bounds: per-level terms as test_oracle_golden.py uses for G6 (rtol 2e-5, atol 2e-5 max(1, |want|max)); schedule scalars and
constants bit for bit; the one-level reduction bit for bit."""
import numpy as np
import pytest
import torch

from helpers import HIST, SCORE_BAND as BAND, SCORE_CASES as CASES, close, g21, score_case
import score_ref
from oracle import ref_cpu
import cmdgen_amd  # noqa: F401
from cmdgen_amd import hip_backend, scoring

G21 = g21()


@pytest.mark.parametrize('case', CASES)
def test_g21_margins_leave_nothing_out(case):
    """The committed cases keep every (level, sample) entry outside the 1e-4 band of the cutoff; the cap for any case is 2 %."""
    m = G21[f'{case}/margins']
    K = int(case[1:])
    assert m.shape == (K + 1, 4)
    inside = int((m < BAND).sum())
    print(case, 'entries inside the band:', inside, 'of', m.size, 'min margin', float(m.min()))
    assert inside <= 0.02 * m.size
    assert inside == 0


@pytest.mark.parametrize('case', CASES)
def test_score_ref_matches_g21_levels(case):
    """Every level of the CPU model against the reference's forward at that level: error_t, the t = 0 terms, the weights, kl_prior."""
    cfg, sd, phar, pocket = score_case()
    p = ref_cpu.to_torch_params(sd)
    K = int(case[1:])
    g = {k[len(case) + 1:]: v for k, v in G21.items() if k.startswith(case + '/')}
    assert list(g['t_levels']) == score_ref.level_list(cfg.timesteps, K)
    with torch.no_grad():
        raw = score_ref.score_levels(p, cfg.as_dict(), phar, pocket, g['t_levels'].tolist(), g['noise'])
    keep = g['margins'] >= BAND
    assert keep.all()
    assert close(raw['err'][:K].numpy(), g['error_t'])
    assert close(0.5 * raw['err_x'][K].numpy(), g['loss_0_x'][0])
    assert close(-raw['log_ph'][K].numpy(), g['loss_0_h'][0])
    assert close(raw['kl_prior'].numpy(), g['kl_prior'][0])
    assert close(raw['neg_log_const_0'].numpy(), g['neg_log_const_0'][0])
    assert close(raw['w'][:K].numpy(), g['SNR_weight'][:, 0])
    assert np.allclose(raw['netmax'].numpy(), g['netmax'], rtol=1e-3, atol=1e-5)
    assert (raw['err'][:K].numpy() >= 0).all() and (raw['w'][:K].numpy() < 0).all()          # no cancellation in the sum over levels


def test_one_level_is_ddpm_forward_bit_for_bit():
    """K = 1 (the level t = T and the t = 0 level) with the matching draws is ref_cpu.ddpm_forward(training=False) + nll_from_terms."""
    cfg, sd, phar, pocket = score_case()
    p = ref_cpu.to_torch_params(sd)
    T, B = cfg.timesteps, len(phar['size'])
    noise = G21['K20/noise'][[3, 20]]
    with torch.no_grad():
        got = score_ref.score(p, cfg.as_dict(), phar, pocket, 1, noise, HIST)
        terms = ref_cpu.ddpm_forward(p, cfg.as_dict(), phar, pocket, torch.full((B, 1), float(T)),
                                     [torch.from_numpy(noise[0]), torch.from_numpy(noise[1])], False, HIST)
        nll = ref_cpu.nll_from_terms(terms, cfg.as_dict(), phar['size'], pocket['size'], False)
    assert torch.equal(got['raw']['err'][0], terms[1])
    assert torch.equal(got['loss_0_x'], terms[4]) and torch.equal(got['loss_0_h'], terms[6])
    assert torch.equal(got['kl_prior'], terms[8]) and torch.equal(got['neg_log_const_0'], terms[7])
    assert torch.equal(got['raw']['w'][0].expand(B), terms[3])
    assert torch.equal(got['nll'], nll)


@pytest.mark.parametrize('case', CASES)
def test_mirror_level_table_is_the_references_bit_for_bit(case):
    """scoring.level_table / assemble evaluate the schedule on the host as per_sample_table does: alpha, sigma, w_k and the constants
    equal the values the reference's forward returned, bit for bit."""
    cfg, sd, phar, pocket = score_case()
    g = {k[len(case) + 1:]: v for k, v in G21.items() if k.startswith(case + '/')}
    K = int(case[1:])
    gamma = np.asarray(sd['ddpm.gamma.gamma'], dtype=np.float32)
    tab = scoring.level_table(gamma, cfg.timesteps, 3, cfg.norm_values, g['t_levels'])
    assert np.array_equal(tab['alpha'][:K], g['alpha_t']) and np.array_equal(tab['sigma'][:K], g['sigma_t'])
    assert np.array_equal(tab['alpha'][K], g['alpha_0']) and np.array_equal(tab['sigma'][K], g['sigma_0'])
    assert np.array_equal(tab['w'][:K], g['SNR_weight'][:, 0])
    assert np.array_equal(tab['alpha_T'], g['alpha_T']) and np.array_equal(tab['sigma_T'], g['sigma_T'])
    assert np.array_equal(scoring.level_list(cfg.timesteps, K), g['t_levels'])
    coef = scoring.level_coef(tab, 2)
    assert coef.shape == (2 * (K + 1) + 1, 2) and np.array_equal(coef[K + 1:2 * K + 2], coef[:K + 1]) and coef[-1, 0] == g['alpha_T']
    # the assembly on the CPU model's raw sums: constants bit for bit, the rest to fp32 rounding
    p = ref_cpu.to_torch_params(sd)
    with torch.no_grad():
        want = score_ref.score(p, cfg.as_dict(), phar, pocket, K, g['noise'], HIST)
    raw = want['raw']
    sums = torch.stack([raw['err'], raw['err_x'], raw['log_ph'], torch.zeros_like(raw['err'])], dim=2).numpy()
    from cmdgen_amd.equivariant_diffusion.en_diffusion import DistributionNodes
    log_pn = DistributionNodes(HIST)._table(1, torch.device('cpu')).numpy()
    got = scoring.assemble(sums, raw['kl_sums'].numpy(), gamma, log_pn, cfg.timesteps, 3, cfg.norm_values, g['t_levels'],
                           phar['size'].numpy(), pocket['size'].numpy())
    assert np.array_equal(got['neg_log_const_0'], g['neg_log_const_0'][0])
    assert np.array_equal(got['delta_log_px'], g['delta_log_px'][0])
    assert np.array_equal(got['log_pN'], g['log_pN'][0])
    assert np.allclose(got['kl_prior'], g['kl_prior'][0], rtol=1e-6, atol=0)
    assert np.array_equal(got['level_terms'][0], want['level_terms'].numpy())
    for k in ('nll', 'loss_t', 'loss_0_x', 'loss_0_h'):
        assert np.allclose(got[k], want[k].numpy(), rtol=1e-6, atol=0), k
    f64 = got['level_terms'][0].astype(np.float64).sum(0) + (got['neg_log_const_0'].astype(np.float64) + got['kl_prior']
                                                             - got['delta_log_px'] - got['log_pN'])
    assert np.allclose(got['nll'], f64, rtol=1e-6, atol=0)


def test_assemble_repeats_are_means():
    rng = np.random.default_rng(0)
    cfg, sd, phar, pocket = score_case()
    gamma = np.asarray(sd['ddpm.gamma.gamma'], dtype=np.float32)
    lv = scoring.level_list(cfg.timesteps, 4)
    sums = np.abs(rng.normal(size=(2, 5, 4, 4))).astype(np.float32)
    kl = np.abs(rng.normal(size=(4, 2))).astype(np.float32)
    log_pn = np.zeros((30, 70), dtype=np.float32)
    args = (gamma, log_pn, cfg.timesteps, 3, cfg.norm_values, lv, phar['size'].numpy(), pocket['size'].numpy())
    both = scoring.assemble(sums, kl, *args)
    one = [scoring.assemble(sums[r], kl, *args) for r in range(2)]
    for k in ('nll', 'loss_t', 'loss_0_x', 'loss_0_h'):
        assert np.array_equal(both[k + '_repeats'], np.stack([o[k] for o in one]))
        assert np.array_equal(both[k], np.stack([o[k] for o in one]).astype(np.float64).mean(0).astype(np.float32))


# ---------------------------------------------------------------- the public entries (these fail without the feature)
def test_library_exports_and_binds_score_chain():
    lib = hip_backend.load_library()
    assert hasattr(lib, 'cmdgen_score_chain')
    assert 'cmdgen_score_chain' in {n for n, _, _ in hip_backend.SYMBOLS}
    assert lib.cmdgen_score_chain.restype is not None and len(lib.cmdgen_score_chain.argtypes) == 15
    assert callable(getattr(hip_backend.Handle, 'score_chain', None)) and hip_backend.Handle.SC_COLS == 4


def test_score_entries_exist_and_refuse_on_the_host():
    from helpers import small_ddpm, host_hparams as _hparams
    from cmdgen_amd.equivariant_diffusion.conditional_model import ConditionalDDPM, SimpleConditionalDDPM
    from cmdgen_amd.equivariant_diffusion.en_diffusion import EnVariationalDiffusion
    from cmdgen_amd.lightning_modules import PharPocketDDPM
    assert callable(ConditionalDDPM.score) and callable(PharPocketDDPM.score) and callable(PharPocketDDPM.score_phars)
    cfg, sd, phar, pocket = score_case()
    ddpm = small_ddpm(T=100)
    with pytest.raises(ValueError, match='divisor'):          # before any device work: no GPU is needed to get here
        ddpm.score(phar, pocket, timesteps=7)
    with pytest.raises(ValueError, match='divisor'):
        ddpm.score(phar, pocket, timesteps=200)
    with pytest.raises(ValueError, match='repeats'):
        ddpm.score(phar, pocket, timesteps=10, repeats=0)
    with pytest.raises(NotImplementedError, match='joint'):
        EnVariationalDiffusion.score(None)
    with pytest.raises(NotImplementedError, match='SimpleConditionalDDPM'):
        SimpleConditionalDDPM.score(None)
    model = PharPocketDDPM(**_hparams())
    names = list(model.dataset_info['phar_decoder'])
    with pytest.raises(ValueError, match='unknown pharmacophore type'):
        model.score_phars('no_such_file.pdb', [[(names[0], (0., 0., 0.))], [('NotAType', (1., 0., 0.))]], pocket_ids=['A:1'])
    jm = PharPocketDDPM(**{**_hparams(), 'mode': 'joint'})
    with pytest.raises(NotImplementedError, match='conditional model'):
        jm.score_phars('no_such_file.pdb', [[(names[0], (0., 0., 0.))]], pocket_ids=['A:1'])
