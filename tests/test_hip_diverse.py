"""GPU tests of ConditionalDDPM.sample_diverse / cmdgen_diverse_chain: parity with diverse_ref on injected noise (a batch of mixed sets, the clip, a
sample above 128 nodes, a set wider than the pair kernel's tile), the three reductions to cmdgen_sample_chain bit for bit, graphs against eager
launches and run to run, a set alone against the full batch, guide_below, the effect itself, refusals, and PharPocketDDPM.generate_phars_diverse.

Bounds against the reference are the chain tests' (chain_kit.PARITY): per-op z and pocket <= 1e-4 max(1, max|.|), final x and pocket RMS under the
same bound, types exact; overlap and op_overlap within 1e-4 max(1, |want|), the restrained tests' energy bound.  A set with a member within
1e-4 A of the cutoff at any reference evaluation is left out whole (diverse_cases.py: none for the committed inputs)."""
import os

import numpy as np
import pytest
import torch

import diverse_cases as dc
import chain_kit as kit
from chain_kit import PARITY, PLAIN, SMALL, Out, check_against_ref, dev, handle, lightning_model, model, pocket_dev, run_chain, same, status_key, sub_batch
from helpers import GOLDEN
from cmdgen_amd import hip_backend
from cmdgen_amd.synthetic import ModelConfig, make_state_dict, make_pockets

pytestmark = pytest.mark.gpu
DIVERSE = PLAIN + ('energy', 'op_energy')              # the fields of a diverse run's Out: overlap rides in `energy`, op_overlap in `op_energy`


def run_diverse(h, pb, K, sets, strength=dc.STRENGTH, width=dc.WIDTH, max_shift=dc.MAX_SHIFT, guide_below=1.0, noise=None, seed=7, ids=None,
                use_graph=True):
    """One diverse chain on the layout of pb, shaped like chain_kit.run_chain -> Out (overlap [B] in .energy, op_overlap [K, B] in .op_energy),
    chain status."""
    h.set_layout(pb.num_nodes_phar, pb.size)
    kit.host_tables(h, K)
    x, q, zs, ov, oo = h.diverse_chain(dev(pb.x), dev(pb.one_hot), K, sets, strength=strength, width=width, max_shift=max_shift,
                                       guide_below=guide_below, noise=noise, seed=seed, pocket_ids=ids, want_steps=True, use_graph=use_graph)
    st = h.chain_status()
    return Out(*[t.cpu().numpy() for t in (x, q, zs, h.last_pocket_steps, ov, oo)], kit.chain_z(h)), st


def plain_handle():
    """The launches of SMALL with the evaluations' own k_readout: what the diverse chain's reductions are stated for."""
    return handle(options=dict(SMALL, readout_in_coord=0))


# ------------------------------------------------------------------------------------------------ 1. against the model
@pytest.mark.parametrize('case,clipped,use_graph', [(dc.MIXED, False, True), (dc.MIXED, False, False), (dc.MIXED, True, False),
                                                    (dc.LARGE, False, False), (dc.WIDE, False, False)],
                         ids=['mixed-graph', 'mixed-eager', 'mixed-clipped-eager', 'large-eager', 'wide-eager'])
def test_chain_matches_the_model(case, clipped, use_graph):
    r = dc.reference(case, clipped=clipped)
    pb, want, keep, ks = r['pb'], r['guided'], r['keep'], r['keep_samples']
    h = handle()
    h.set_option('graph_steps', 2)                                   # K = 5: two replays of two steps, one eager step
    got, st = run_diverse(h, pb, case.K, case.sets, max_shift=dc.CLIP_SHIFT if clipped else dc.MAX_SHIFT, noise=r['noise'].cuda(),
                          use_graph=use_graph)
    rows, rows_q = ks[np.repeat(np.arange(len(case.nph)), case.nph)], ks[pb.mask]
    label = f'{case.name}{" clipped" if clipped else ""} {"graph" if use_graph else "eager"}'
    check_against_ref(label, got, st, {k: want[k] for k in PLAIN}, rows, rows_q, keep, 'sets', final='rms')
    rel = lambda g, w: float((np.abs(g - w) / (PARITY * np.maximum(1.0, np.abs(w)))).max())
    r_ov, r_op = rel(got.energy[ks], want['overlap'].numpy()[ks]), rel(got.op_energy[:, ks], want['op_overlap'].numpy()[:, ks])
    print(f'[{label}] worst ratio to the bound: overlap {r_ov:.3f}  op_overlap {r_op:.3f}')
    assert r_ov <= 1.0 and r_op <= 1.0
    if case.big_set is not None:
        assert int((pb.size + pb.num_nodes_phar).max()) > 128           # the 1024-thread step ran
    if case is dc.WIDE:
        assert int(np.sum(case.nph[:case.sets[0]])) > 256               # the pair kernel's tile loop took a second trip


# ------------------------------------------------------------------------------------------------ 2. the reductions
@pytest.mark.parametrize('use_graph', [True, False], ids=['graph', 'eager'])
@pytest.mark.parametrize('inject', [False, True], ids=['device-draws', 'injected'])
def test_without_coupling_it_is_sample_chain_bit_for_bit(inject, use_graph):
    """strength = 0, guide_below = 0 and sets of one member: xh_phar, xh_pocket, z_steps, pocket_steps, chain_z and the chain status of
    cmdgen_sample_chain on a handle whose evaluations run their own k_readout."""
    case = dc.MIXED
    pb, K = dc.pockets(case), 10
    h = plain_handle()
    h.set_option('graph_steps', 8)
    h.set_layout(pb.num_nodes_phar, pb.size)
    assert h.query('readout_in_coord') == 0
    noise = dev(np.random.default_rng(6).normal(size=(K + 2, int(pb.num_nodes_phar.sum()), 11)).astype(np.float32)) if inject else None
    kw = dict(noise=noise, seed=11, ids=pb.pocket_index, use_graph=use_graph)
    want, sw = run_chain(h, pb, K, **kw)
    zero, s0 = run_diverse(h, pb, K, case.sets, strength=0.0, **kw)
    above, s1 = run_diverse(h, pb, K, case.sets, guide_below=0.0, **kw)
    ones, s2 = run_diverse(h, pb, K, (1,) * len(case.nph), **kw)
    for got in (zero, above, ones):
        same(want, got, PLAIN + ('chain_z',))
    assert status_key(sw) == status_key(s0) == status_key(s1) == status_key(s2) and sw['nan_resets'] == 0
    assert not ones.energy.any() and not ones.op_energy.any()           # nothing is coupled: zero overlaps
    coupled = np.repeat(np.asarray(case.sets) > 1, case.sets)
    assert np.all(zero.energy[coupled] > 0) and not zero.energy[~coupled].any() and zero.op_energy.max() > 0   # strength = 0 still reports them
    assert np.array_equal(zero.energy, above.energy) and np.array_equal(zero.op_energy, above.op_energy)
    guided, _ = run_diverse(h, pb, K, case.sets, **kw)
    assert not np.array_equal(guided.xh_phar, want.xh_phar)             # ... and the term is not a no-op here


# ------------------------------------------------------------------------------------------------ 3. graphs and keys
def test_captured_equals_eager_and_a_changed_partition_or_scalar_prepares_the_slot_again():
    case = dc.MIXED
    pb = dc.pockets(case)
    h = handle()
    h.set_option('graph_steps', 2)
    a, sa = run_diverse(h, pb, case.K, case.sets, seed=31, use_graph=True)
    assert h.query('chain_graphs') >= 1
    a2, sa2 = run_diverse(h, pb, case.K, case.sets, seed=31, use_graph=True)
    e, se = run_diverse(h, pb, case.K, case.sets, seed=31, use_graph=False)
    same(a, a2, DIVERSE)
    same(a, e, DIVERSE)
    assert status_key(sa) == status_key(sa2) == status_key(se) and sa['nan_resets'] == 0
    b, _ = run_diverse(h, pb, case.K, (5, 3, 2), seed=31, use_graph=True)                  # another partition
    b_eager, _ = run_diverse(h, pb, case.K, (5, 3, 2), seed=31, use_graph=False)
    assert not np.array_equal(a.xh_phar, b.xh_phar)
    same(b, b_eager, DIVERSE)
    c, _ = run_diverse(h, pb, case.K, case.sets, width=3.0, seed=31, use_graph=True)       # a scalar of the key alone
    assert not np.array_equal(a.xh_phar, c.xh_phar)
    back, sb = run_diverse(h, pb, case.K, case.sets, seed=31, use_graph=True)
    same(a, back, DIVERSE)
    assert status_key(sa) == status_key(sb)


# ------------------------------------------------------------------------------------------------ 4. a set alone
def test_a_set_alone_gives_the_full_batchs_rows():
    """Set 2 of the mixed case (samples 5, 6, 7) alone, with its pocket ids, device draws: the rows of the full batch within
    test_hip_restraint.py's shard bound (not bit for bit: the tile rule differs with the batch size)."""
    case = dc.MIXED
    pb = dc.pockets(case)
    members = [5, 6, 7]
    h = handle()
    full, _ = run_diverse(h, pb, case.K, case.sets, seed=41, ids=pb.pocket_index)
    sub = sub_batch(pb, members)
    alone, _ = run_diverse(h, sub, case.K, (3,), seed=41, ids=sub.pocket_index)
    rows = np.isin(np.repeat(np.arange(len(case.nph)), case.nph), members)
    xf, xs = full.xh_phar[rows], alone.xh_phar
    bound = 1e-4 * max(1.0, float(np.abs(xf[:, :3]).max()))
    diff = float(np.abs(xs[:, :3] - xf[:, :3]).max())
    print(f'\n[set alone] max |dx| {diff:.3e} A, bound {bound:.3e}; overlap {alone.energy} / {full.energy[members]}')
    assert diff <= bound
    assert np.array_equal(xs[:, 3:], xf[:, 3:])
    assert np.all(np.abs(alone.energy - full.energy[members]) <= 1e-4 * np.maximum(1.0, np.abs(full.energy[members])))


# ------------------------------------------------------------------------------------------------ 5. guide_below
def test_guide_below_guides_only_the_ops_at_or_below_it():
    """K = 5, guide_below = 0.5: t / T = 1, .8, .6 unguided, .4 and .2 guided - the first three saved steps are the unguided run's, the fourth
    differs."""
    case = dc.MIXED
    pb = dc.pockets(case)
    h = handle()
    off, _ = run_diverse(h, pb, case.K, case.sets, strength=0.0, seed=51)
    part, _ = run_diverse(h, pb, case.K, case.sets, guide_below=0.5, seed=51)
    full, _ = run_diverse(h, pb, case.K, case.sets, seed=51)
    assert np.array_equal(part.z_steps[:3], off.z_steps[:3]) and not np.array_equal(part.z_steps[3], off.z_steps[3])
    assert not np.array_equal(part.z_steps[0], full.z_steps[0])
    assert np.array_equal(part.op_energy[:4], off.op_energy[:4])        # the overlap at an op's input estimate: the same until a guided op has acted


# ------------------------------------------------------------------------------------------------ 6. the effect
def test_guidance_lowers_the_overlap_of_every_member_of_a_coupled_set():
    case = dc.MIXED
    r = dc.reference(case)
    h = handle()
    noise = r['noise'].cuda()
    g, _ = run_diverse(h, r['pb'], case.K, case.sets, noise=noise)
    u, _ = run_diverse(h, r['pb'], case.K, case.sets, strength=0.0, noise=noise)
    coupled = np.repeat(np.asarray(case.sets) > 1, case.sets) & r['keep_samples']
    print(f'\n[effect] final overlap unguided {u.energy}\n         guided   {g.energy}')
    assert coupled.sum() >= 9
    assert np.all(g.energy[coupled] < u.energy[coupled])


# ------------------------------------------------------------------------------------------------ 7. refusals
def _small_handle(**cfg_kw):
    cfg = ModelConfig(hidden_nf=64, n_layers=1, **cfg_kw)
    h = hip_backend.Handle(cfg.as_dict(), 0)
    h.load_state_dict(make_state_dict(cfg, seed=0))
    return h, cfg


def _refusal_inputs():
    pb = make_pockets(3, 'CA', ragged=True, first_index=9700)
    pb.num_nodes_phar[:] = (3, 1, 5)
    return pb, dev(pb.x), dev(pb.one_hot)


@pytest.fixture(scope='module')
def refusing():
    pb, px, poh = _refusal_inputs()
    h, cfg = _small_handle(timesteps=500)
    h.set_layout(pb.num_nodes_phar, pb.size)
    yield h, px, poh, (lambda match, sets=(3,), **kw: kit.refused(h, lambda: h.diverse_chain(px, poh, 5, sets, **kw), match))
    h.close()


def test_a_null_pointer_is_refused(refusing):
    h, px, poh, _ = refusing
    lib, out = h.lib, torch.empty((9, 11), device='cuda')
    sizes = np.asarray([3], dtype=np.int64)
    sp = sizes.ctypes.data_as(hip_backend._i64p)
    ptr = hip_backend._ptr
    q, ov = torch.empty((int(h.n_pocket), 3 + h.cfg['residue_nf']), device='cuda'), torch.empty(3, device='cuda')
    full = [h.h, ptr(px), ptr(poh), 5, 1, sp, 1.0, 2.0, 1.0, 1.0, None, 3, None, ptr(out), ptr(q), None, None, ptr(ov), None, 0, None]
    for at in (1, 2, 5, 13, 14, 17):                                    # pocket_x, pocket_onehot, set_size_host, xh_phar_out, xh_pocket_out, overlap_out
        args = list(full)
        args[at] = None
        assert lib.cmdgen_diverse_chain(*args) == kit.EINVAL and 'null pointer' in lib.cmdgen_last_error(h.h).decode()


def test_a_bad_partition_is_refused(refusing):
    _, _, _, refused = refusing
    refused('n_sets=4', sets=(1, 1, 1, 1))
    refused('n_sets=0', sets=())
    refused(r'set_size\[1\]=0', sets=(3, 0))
    refused(r'set_size\[0\]=-1', sets=(-1, 4))
    refused('set_size sums to 2', sets=(1, 1))
    refused('set_size sums to 4', sets=(2, 2))


def test_a_bad_scalar_is_refused(refusing):
    _, _, _, refused = refusing
    for bad in (-1.0, float('nan'), float('inf')):
        refused('strength', strength=bad)
    for bad in (0.0, -2.0, float('nan'), float('inf')):
        refused('width', width=bad)
    for bad in (0.0, -1.0, float('nan')):
        refused('max_shift', max_shift=bad)
    for bad in (1.5, -0.1, float('nan')):
        refused('guide_below', guide_below=bad)


def test_the_handle_stays_usable_after_refusals(refusing):
    h, px, poh, refused = refusing
    refused('strength', strength=-1.0)
    good = h.diverse_chain(px, poh, 5, (2, 1), seed=3)
    plain = h.sample_chain(px, poh, 5, seed=3)                          # ... and an ordinary chain follows
    st = h.chain_status()
    assert good[0].shape == plain[0].shape == (9, 11) and good[3].shape == (3,) and good[4] is None and st['max_rel_com_error'] < 1e-2
    assert all(bool(torch.isfinite(t).all()) for t in (good[0], good[3], plain[0]))
    assert float(good[3][2]) == 0.0 and float(good[3][:2].min()) >= 0.0


def test_a_set_beyond_the_row_cap_and_a_sample_beyond_the_steps_lds_are_refused():
    h, cfg = _small_handle(timesteps=500)
    nph = np.asarray([16] * 512 + [1], dtype=np.int64)                  # 8192 rows plus one in one set
    assert int(nph.sum()) == hip_backend.Handle.MAX_SET_ROWS + 1
    h.set_layout(nph, np.ones(513, dtype=np.int64))
    px, poh = torch.zeros((513, 3), device='cuda'), torch.zeros((513, cfg.residue_nf), device='cuda')
    kit.refused(h, lambda: h.diverse_chain(px, poh, 5, (513,)), '8193 phar rows, at most 8192')
    # a sample beyond the step's 64 KiB of LDS (64 B per node at phar_nf 8): refused before anything is launched
    h.set_layout([3, 2], [1100, 5])
    px, poh = torch.zeros((1105, 3), device='cuda'), torch.zeros((1105, cfg.residue_nf), device='cuda')
    kit.refused(h, lambda: h.diverse_chain(px, poh, 5, (2,)), '1103 nodes')
    h.close()


def test_the_joint_and_the_no_com_handles_refuse_and_run_their_own_chains():
    pb, px, poh = _refusal_inputs()
    joint, _ = _small_handle(update_pocket_coords=True)
    joint.set_layout(pb.num_nodes_phar, pb.size)
    with pytest.raises(hip_backend.CmdgenError, match='joint model'):
        joint.diverse_chain(px, poh, 5, (3,))
    assert joint.joint_chain(5, seed=3)[0].shape == (9, 11)
    joint.close()
    simple, _ = _small_handle(timesteps=500, no_com_projection=True)
    simple.set_layout(pb.num_nodes_phar, pb.size)
    with pytest.raises(hip_backend.CmdgenError, match='no_com_projection'):
        simple.diverse_chain(px, poh, 5, (3,))
    assert simple.sample_chain(px, poh, 5, seed=3)[0].shape == (9, 11)
    simple.close()


# ------------------------------------------------------------------------------------------------ 8. the Python entry points
def test_sample_diverse_returns_the_chains_result():
    """ConditionalDDPM.sample_diverse on the mixed case: the chain's outputs (bit for bit the binding's, same tables and draws), frames, and
    strength = 0 as sample_given_pocket."""
    case = dc.MIXED
    r = dc.reference(case)
    pb = r['pb']
    ddpm = model()
    ddpm.use_hip_graph = True
    pocket = pocket_dev(pb)
    noise = r['noise'].cuda()
    x, q, pm, qm, info = ddpm.sample_diverse(pocket, case.nph, case.sets, strength=dc.STRENGTH, width=dc.WIDTH, max_shift=dc.MAX_SHIFT,
                                             timesteps=case.K, noise=noise)
    want, _ = run_diverse(ddpm.dynamics.hip_handle(), pb, case.K, case.sets, noise=noise)
    assert np.array_equal(x.cpu().numpy(), want.xh_phar) and np.array_equal(q.cpu().numpy(), want.xh_pocket)
    assert np.array_equal(info['overlap'].cpu().numpy(), want.energy)
    assert 'op_overlap' not in info and pm.shape == (sum(case.nph),) and tuple(info['overlap'].shape) == (len(case.nph),)
    frames = ddpm.sample_diverse(pocket, case.nph, case.sets, return_frames=case.K, timesteps=case.K, noise=noise)
    assert frames[0].shape == (case.K, sum(case.nph), 11) and frames[4]['op_overlap'].shape == (case.K, len(case.nph))
    assert torch.equal(frames[0][0], x) and np.array_equal(frames[4]['op_overlap'].cpu().numpy(), want.op_energy)
    plain = ddpm.sample_given_pocket(pocket, case.nph, timesteps=case.K, noise=noise)
    off = ddpm.sample_diverse(pocket, case.nph, case.sets, strength=0.0, timesteps=case.K, noise=noise)
    assert torch.equal(off[0], plain[0]) and torch.equal(off[1], plain[1])
    with pytest.raises(ValueError, match='set_sizes sums to 9'):
        ddpm.sample_diverse(pocket, case.nph, (4, 5), timesteps=case.K)
    with pytest.raises(ValueError, match='width'):
        ddpm.sample_diverse(pocket, case.nph, case.sets, width=0.0, timesteps=case.K)


def test_generate_phars_diverse_end_to_end():
    """PharPocketDDPM.generate_phars_diverse on the g7 pocket (30 C-alpha residues): per-sample point lists in the PDB's frame, the overlap, the
    same seed the same result, and less overlap than the independent draws of the same seed.

    The model's weights are untrained and its schedule is the shipped one (1 / alpha_T = 316): a 50-op chain leaves the points hundreds of A
    out ("Restrained sampling"; measured here: a spread of 730 A at seed 5), where the default width of 2 A sees overlaps of
    exactly 0 guided or not.  The comparison therefore uses a width on the scale of that spread, 100 A, and strength 100 (the gradient carries
    1 / width^2): measured on an MI355X, the summed overlap goes 1.866 -> 1.506 at seed 5 and 0.962 -> 0.784 at seed 6."""
    m = lightning_model()
    pdb = os.path.join(GOLDEN, 'g7_pocket.pdb')
    ids = [f'A:{i}' for i in range(1, 30)]
    nph = torch.tensor([4, 7, 3])
    kw = dict(pocket_ids=ids, num_nodes_phar=nph, width=100.0, timesteps=50, seed=5)
    out, info = m.generate_phars_diverse(pdb, 3, strength=100.0, **kw)
    assert [len(s) for s in out] == [4, 7, 3] and tuple(info['overlap'].shape) == (3,)
    names = set(m.dataset_info['phar_decoder'])
    assert all(name in names and len(xyz) == 3 for s in out for name, xyz in s)
    out2, info2 = m.generate_phars_diverse(pdb, 3, strength=100.0, **kw)
    assert out == out2 and torch.equal(info['overlap'], info2['overlap'])
    off, info0 = m.generate_phars_diverse(pdb, 3, strength=0.0, **kw)
    print(f'\n[generate_phars_diverse] overlap guided {info["overlap"].tolist()} against independent draws {info0["overlap"].tolist()}')
    assert float(info0['overlap'].sum()) > 0 and float(info['overlap'].sum()) < float(info0['overlap'].sum())
    scores = m.score_phars(pdb, out, pocket_ids=ids, timesteps=10, seed=3)
    assert tuple(scores['nll'].shape) == (3,)
    default = m.generate_phars_diverse(pdb, 3, pocket_ids=ids, num_nodes_phar=nph, timesteps=50, seed=5)      # the defaults run too
    assert [len(s) for s in default[0]] == [4, 7, 3]
