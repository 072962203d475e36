"""The chain kit's comparison (chain_kit.parity_ratios, check_against_ref) on small synthetic arrays: a perturbation of known size gives the
ratio computed by hand under both metrics, and each of the things the shared check must refuse - a flipped type, too many owners left out, a
mask that selects nothing, a dirty chain status - fails it.  No GPU: 3 ops, 6 phar rows and 8 pocket rows of 2 owners."""
import numpy as np
import pytest

from chain_kit import CHAIN_CAP, PARITY, Out, check_against_ref, parity_ratios

N_OPS, OWNERS = 3, 2
PM, QM = np.repeat(np.arange(OWNERS), 3), np.repeat(np.arange(OWNERS), 4)         # owner of a phar row / of a pocket row
CLEAN = {'nan_resets': 0, 'max_rel_com_error': 1e-6}


def yardstick():
    """A guided chain's yardstick with max |x| = 10, max |z| = 2 and pocket coordinates below 1 beside one-hot columns."""
    rng = np.random.default_rng(0)
    x = rng.uniform(-1, 1, size=(6, 3)); x[0, 0] = 10.0
    z = rng.uniform(-1, 1, size=(N_OPS, 6, 11)); z[:, 0, 0] = 2.0
    return dict(xh_phar=np.concatenate([x, np.eye(8)[np.arange(6) % 8]], 1), xh_pocket=np.concatenate([rng.uniform(-1, 1, size=(8, 3)), np.eye(20)[:8]], 1),
                z_steps=z, pocket_steps=rng.uniform(-1, 1, size=(N_OPS, 8, 3)), energy=np.array([4.0, 0.5]), max_violation=np.array([2.0, 0.25]),
                op_energy=np.full((N_OPS, OWNERS), 8.0))


def got_from(want, **changed):
    out = {k: np.array(want[k], dtype=np.float64) for k in ('xh_phar', 'xh_pocket', 'z_steps', 'pocket_steps', 'op_energy')}
    out['energy'] = np.stack([want['energy'], want['max_violation']], 1)
    out.update(changed)
    return Out(chain_z=None, **out)


def check(got, want, keep=np.ones(OWNERS, bool), st=CLEAN, **metric):
    check_against_ref('synthetic', got, st, want, keep[PM], keep[QM], keep, 'owners', **metric)


def test_a_known_perturbation_gives_the_ratio_computed_by_hand():
    want = yardstick()
    x, q, z, oe = (want[k].copy() for k in ('xh_phar', 'xh_pocket', 'z_steps', 'op_energy'))
    x[1, 2] += 3e-4                      # one of 18 coordinates: RMS 3e-4 / sqrt(18), largest 3e-4; the scale is max |x| = 10
    q[2, 1] += 5e-5                      # one of 8 x 23 entries of the whole row, one of 8 x 3 coordinates; the scale is 1 (the one-hot's, or the floor)
    z[1, 3, 4] += 1e-4                   # the scale is max |z| = 2
    oe[2, 1] += 4e-4                     # relative to |want| = 8, elementwise
    got = got_from(want, xh_phar=x, xh_pocket=q, z_steps=z, op_energy=oe)
    keep, rows, rows_q = np.ones(OWNERS, bool), np.ones(6, bool), np.ones(8, bool)
    rms = parity_ratios(got, want, rows, rows_q, keep, final='rms')
    top = parity_ratios(got, want, rows, rows_q, keep, final='max', pocket_cols=slice(0, 3))
    assert list(rms) == list(top) == ['z', 'pocket_steps', 'x', 'pocket', 'energy', 'max_violation', 'op_energy']
    assert rms['x'] == pytest.approx(3e-4 / np.sqrt(18) / (PARITY * 10)) and top['x'] == pytest.approx(3e-4 / (PARITY * 10))
    assert rms['pocket'] == pytest.approx(5e-5 / np.sqrt(8 * 23) / PARITY) and top['pocket'] == pytest.approx(5e-5 / PARITY)
    for r in (rms, top):
        assert r['z'] == pytest.approx(1e-4 / (PARITY * 2)) and r['op_energy'] == pytest.approx(4e-4 / (PARITY * 8))
        assert r['pocket_steps'] == r['energy'] == r['max_violation'] == 0
    check(got, want, final='rms')                                        # every ratio is below 1: the check passes under both metrics
    check(got, want, final='max', pocket_cols=slice(0, 3))
    # a row of an owner that is left out is not compared: the same perturbation a hundred times larger, on owner 1's rows only
    x2 = want['xh_phar'].copy(); x2[4, 0] += 3e-2
    only0 = np.array([True, False])
    assert parity_ratios(got_from(want, xh_phar=x2), want, only0[PM], only0[QM], only0)['x'] == 0
    assert parity_ratios(got_from(want, xh_phar=x2), want, rows, rows_q, keep)['x'] > 1
    with pytest.raises(AssertionError, match="'x'"):
        check(got_from(want, xh_phar=x2), want)


def test_an_unguided_chain_has_the_four_ratios():
    want = {k: v for k, v in yardstick().items() if k not in ('energy', 'max_violation', 'op_energy')}
    got = got_from(yardstick())
    assert list(parity_ratios(got, want, np.ones(6, bool), np.ones(8, bool))) == ['z', 'pocket_steps', 'x', 'pocket']


def test_a_flipped_type_fails():
    want = yardstick()
    x = want['xh_phar'].copy()
    x[2, 3:] = np.roll(x[2, 3:], 1)
    with pytest.raises(AssertionError):
        check(got_from(want, xh_phar=x), want)
    check(got_from(want), want)


def test_one_owner_left_out_above_the_cap_fails():
    want = yardstick()
    keep = np.array([True, False])                                       # one of two owners: 50 % > CHAIN_CAP
    assert 1 > CHAIN_CAP * OWNERS
    with pytest.raises(AssertionError):
        check(got_from(want), want, keep=keep)


def test_an_empty_selection_fails():
    want, none = yardstick(), np.zeros(OWNERS, bool)
    for rows, rows_q in ((none[PM], np.ones(8, bool)), (np.ones(6, bool), none[QM])):
        with pytest.raises(AssertionError, match='selects no row'):
            parity_ratios(got_from(want), want, rows, rows_q, np.ones(OWNERS, bool))
    with pytest.raises(AssertionError, match='selects no'):
        check(got_from(want), want, keep=none)


@pytest.mark.parametrize('st', [{'nan_resets': 1, 'max_rel_com_error': 1e-6}, {'nan_resets': 0, 'max_rel_com_error': 2e-2}], ids=['reset', 'com'])
def test_a_dirty_status_fails(st):
    want = yardstick()
    with pytest.raises(AssertionError):
        check(got_from(want), want, st=st)
