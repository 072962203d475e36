"""The kit of the GPU chain tests (test_hip_inpaint, _edit, _restraint, _restrained_edit, _multi_pocket, _multi_edit, _multi_restraint,
_multi_restrained_edit, _score, _multi_score): what they share, each piece once.  The GPU-side counterpart of chain_ref.py.

  dev, to_dev, pocket_dev, sub_batch, fixed_inputs, given_for,    inputs on the device and the device's own draws
  philox_noise
  handle, handle_for, model, model_for, lightning_model,          one cache of handles of the bounded model (engine x options), one of handles for
  host_tables                                                     the golden-file models, the model constructions
  run_chain (guide, chain_z, status_key, same), run_joint_inpaint  ONE runner shaped like chain_ref.run_chain: the kind follows from the parts passed
  parity_ratios, types_equal, check_against_ref                   the comparison with a yardstick, and its printed line and assertions
  score_entry_ratios                                              the bound of a scoring entry
  record, refused                                                 the refusal tests' restraint record and the refusal check

Importing this module touches no GPU: everything that does happens inside functions.  Test modules do not import each other; what two of them
need lives here or in helpers.py."""
from collections import namedtuple

import numpy as np
import pytest
import torch

import multi_pocket_cases as mc
import restraint_cases as rc
import score_ref
from chain_ref import CHAIN_CAP
from helpers import _hparams, dev, rms
from cmdgen_amd import hip_backend
from cmdgen_amd import restraints as rs
from cmdgen_amd.synthetic import ModelConfig, PocketBatch, make_state_dict

EINVAL, ESTATE = -1, -2                                # include/cmdgen_hip.h: CMDGEN_EINVAL, CMDGEN_ESTATE
SMALL = dict(node_mt=16, node64=0, coord_mt=32)        # the launches readout_in_coord needs, forced on a small layout (test_hip_readout_in_coord.py)
PARITY = 1e-4                                          # the chain tests' bound, relative to max(1, max|.|)
_handles, _golden_handles, _model = {}, {}, []


# ---------------------------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------------------------
def to_dev(d):
    return {k: v.cuda() for k, v in d.items()}


def sub_batch(pb, members):
    """The samples `members` of pb as a batch of their own."""
    members = list(members)
    xs, hs = np.split(pb.x, np.cumsum(pb.size)[:-1]), np.split(pb.one_hot, np.cumsum(pb.size)[:-1])
    size = pb.size[members]
    return PocketBatch(x=np.concatenate([xs[b] for b in members]), one_hot=np.concatenate([hs[b] for b in members]), size=size,
                       mask=np.repeat(np.arange(len(members), dtype=np.int64), size), num_nodes_phar=pb.num_nodes_phar[members],
                       pocket_index=None if pb.pocket_index is None else pb.pocket_index[members])


def pocket_dev(pb, members=None):
    """The pocket dict of pb's samples (or of the listed ones) on the device."""
    if members is not None:
        pb = sub_batch(pb, members)
    return {'x': dev(pb.x), 'one_hot': dev(pb.one_hot), 'size': dev(pb.size), 'mask': dev(pb.mask)}


def fixed_inputs(pb, frac, rng):
    """Known rows near each pocket's centre, the first `frac` of each sample's rows fixed."""
    nl = pb.num_nodes_phar
    pm = np.repeat(np.arange(len(nl)), nl)
    com = np.stack([pb.x[pb.mask == b].mean(0) for b in range(len(nl))])
    phar_x = (com[pm] + rng.normal(size=(len(pm), 3)) * 2.5).astype(np.float32)
    phar_oh = np.eye(8, dtype=np.float32)[rng.integers(0, 8, size=len(pm))]
    first = np.concatenate([[0], np.cumsum(nl)[:-1]])
    local = np.arange(len(pm)) - first[pm]
    fixed = (local < np.maximum(1, (nl[pm] * frac).astype(int))).astype(np.float32)
    return phar_x, phar_oh, fixed, pm


def given_for(nph, seed):
    """Given rows (phar_x, phar_one_hot, fix_x, fix_h) for unique-row counts nph: every kind of mark, and the last group (when there are
    several) without one."""
    rng = np.random.default_rng(seed)
    nu = int(np.sum(nph))
    um = np.repeat(np.arange(len(nph)), nph)
    x = (rng.normal(size=(nu, 3)) * 2.5).astype(np.float32)
    oh = np.eye(8, dtype=np.float32)[rng.integers(0, 8, size=nu)]
    fx = (np.arange(nu) % 2 == 0).astype(np.float32)
    fh = (np.arange(nu) % 3 == 0).astype(np.float32)
    if len(nph) > 1:
        fx[um == len(nph) - 1] = 0.0
        fh[um == len(nph) - 1] = 0.0
    return x, oh, fx, fh


def philox_noise(h, seed, ids, n_rows, draws, width=11):
    """[len(draws), sum n_rows, width]: what cmdgen_debug_noise returns for (seed, id of the sample or group, draw counter, node of it).  A
    sampling chain's counters are its plan's (K + 2 of them for a plain chain), a scoring chain's the level indices."""
    return torch.stack([torch.cat([h.debug_noise(seed, int(i), int(c), int(n), width) for i, n in zip(ids, n_rows)]) for c in draws]).contiguous()


# ---------------------------------------------------------------------------------------------------------------------------------------
# handles and models
# ---------------------------------------------------------------------------------------------------------------------------------------
def handle(engine='half', options=None):
    """A handle of the bounded model of the chain tests (the bench's weights: bounded_config(20, 1000), seed 0), one per engine - as
    rule_sweep_ref: 'half' (the default), 'bf3' (three bf16 pieces), 'fp32' - and set of options.  Shared by every test that asks for the same
    one: a test leaves nothing on it that another test's numbers depend on (graph_steps only splits the replays)."""
    key = (engine, tuple(sorted((options or {}).items())))
    if key not in _handles:
        assert engine in ('half', 'bf3', 'fp32'), engine
        h = hip_backend.Handle(mc.config().as_dict(), 0)
        h.load_state_dict(mc.state_dict())
        if engine == 'bf3':
            h.set_option('half_engine', 0)
        elif engine == 'fp32':
            h.set_gemm_mode(False)
        for k, v in key[1]:
            h.set_option(k, v)
        _handles[key] = h
    return _handles[key]


def handle_for(cfg, key, sd):
    """A handle of another model (a golden file's, the held-rows cases'), one per configuration and key."""
    k = (tuple(sorted((a, str(b)) for a, b in cfg.as_dict().items())), key)
    if k not in _golden_handles:
        h = hip_backend.Handle(cfg.as_dict(), 0)
        h.load_state_dict(sd)
        _golden_handles[k] = h
    return _golden_handles[k]


def model_for(cfg, sd, hist=None):
    """ConditionalDDPM of cfg with the weights sd, on the device (size_histogram: all ones unless given)."""
    from cmdgen_amd.equivariant_diffusion.dynamics import EGNNDynamics
    from cmdgen_amd.equivariant_diffusion.conditional_model import ConditionalDDPM
    dyn = EGNNDynamics(phar_nf=cfg.phar_nf, residue_nf=cfg.residue_nf, n_dims=3, joint_nf=cfg.joint_nf, hidden_nf=cfg.hidden_nf,
                       n_layers=cfg.n_layers, attention=True, tanh=True, norm_constant=1, inv_sublayers=1, sin_embedding=False,
                       normalization_factor=100, aggregation_method='sum', edge_cutoff=6.0, update_pocket_coords=False)
    ddpm = ConditionalDDPM(dynamics=dyn, phar_nf=cfg.phar_nf, residue_nf=cfg.residue_nf, n_dims=3, timesteps=cfg.timesteps,
                           noise_schedule=cfg.noise_schedule, noise_precision=cfg.noise_precision, loss_type='l2',
                           norm_values=list(cfg.norm_values), size_histogram=np.ones((30, 70)) if hist is None else hist)
    ddpm.load_state_dict({k[len('ddpm.'):]: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return ddpm.cuda()


def model():
    """The bounded model as a ConditionalDDPM on the device, built once."""
    if not _model:
        _model.append(model_for(mc.config(), mc.state_dict()))
    return _model[0]


def lightning_model():
    """PharPocketDDPM (C-alpha, width 64, two layers) with seed-0 weights, on the device: the model of the end-to-end tests."""
    from cmdgen_amd.lightning_modules import PharPocketDDPM
    m = PharPocketDDPM(**_hparams('CA', 64, 2))
    sd = make_state_dict(ModelConfig(hidden_nf=64, n_layers=2, timesteps=500), seed=0)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return m.cuda()


def host_tables(h, K):
    """The step table and the guide table in the reference's own fp32 ops, as ConditionalDDPM's sampling entries supply them."""
    ddpm = model()
    h.set_step_table(K, ddpm.step_table(K))
    h.set_guide_table(K, ddpm.guide_table(K))


# ---------------------------------------------------------------------------------------------------------------------------------------
# the runner
# ---------------------------------------------------------------------------------------------------------------------------------------
FIELDS = ('xh_phar', 'xh_pocket', 'z_steps', 'pocket_steps', 'energy', 'op_energy', 'chain_z')
PLAIN, GUIDED = FIELDS[:4], FIELDS[:6]                 # what an unguided / a guided chain returns; chain_z is the debug read
Out = namedtuple('Out', FIELDS)


def chain_z(h):
    """The chain buffer's z as the decode left it (the multi-pocket chains: every member's copy), flat."""
    return h.debug_read('chain_z', int(np.sum(h.num_phar_host)) * 11)


def status_key(st):
    return (st['max_rel_com_error'], st['max_cog'], st['nan_resets'])


def guide(rec, clash=rc.CLASH, scale=rc.SCALE, max_shift=rc.MAX_SHIFT, guide_below=1.0):
    """run_chain's `guide` argument.  The defaults are restraint_cases': the other guided cases modules take theirs from it or repeat them."""
    return rec, clash, scale, max_shift, guide_below


def run_chain(h, pb, K, groups=None, given=None, guide=None, plan=None, noise=None, seed=7, ids=None, use_graph=True, tables=True,
              want_steps=True):
    """One chain on the layout of pb, as chain_ref.run_chain composes its yardstick: the binding follows from the parts passed.

      groups = (sizes, weights)                                  the multi-pocket chains; ids are then group ids
      given  = (x, one_hot, fix_x, fix_h) | (x, one_hot, fixed)  four: the edit chains; three: cmdgen_inpaint_chain (no groups, no guide)
      guide  = (rec, clash, scale, max_shift, guide_below)       the restrained chains (guide() fills in the defaults)
      plan   = (start, r, j)                                     of the chains with `given`

    tables: set the host's step and guide tables for K first (host_tables).  The multi-pocket, multi-edit, inpainting and edit tests pass
    False, as they ran before there was a kit: that keeps the library's own evaluation of the gamma table - what a caller without the Python
    model gets - under test.  (A handle keeps a host table until one for another K replaces it; both tables meet every bound, and every
    bit-for-bit test compares runs under the same one.)
    -> Out (numpy; energy [owners, 2] and op_energy [n_steps, owners] of a guided chain, z_steps and pocket_steps where want_steps, else
    None), chain status"""
    multi, guided = groups is not None, guide is not None
    h.set_layout(pb.num_nodes_phar, pb.size)
    if tables:
        host_tables(h, K)
    args = [dev(pb.x), dev(pb.one_hot)] + (list(groups) if multi else [])
    kw = dict(noise=noise, seed=seed, use_graph=use_graph, want_steps=want_steps, **{'group_ids' if multi else 'pocket_ids': ids})
    if guided:
        rec, clash, scale, max_shift, guide_below = guide
        kw.update(clash_radius=clash[0], clash_k=clash[1], scale=scale, max_shift=max_shift, guide_below=guide_below)
    if given is None:
        name = 'restrained' if guided else 'pocket' if multi else 'sample'
        args += [K] + ([rec] if guided else [])
    else:
        start, r, j = plan or (None, 1, 1)
        kw.update(resamplings=r, jump_length=j)
        if len(given) == 4:
            kw['start'] = start
        else:
            assert not multi and not guided and start is None      # cmdgen_inpaint_chain: from the prior, one mask
        if guided:
            kw['restraints'] = rec
        name = 'restrained_edit' if guided else 'edit' if len(given) == 4 else 'inpaint'
        args += [dev(np.asarray(a, np.float32)) for a in given] + [K]
    out = getattr(h, ('multi_' if multi else '') + name + '_chain')(*args, **kw)
    st = h.chain_status()
    x, q, zs = out[:3]
    en, oe = out[3:] if guided else (None, None)
    steps = h.last_pocket_steps if want_steps else None
    return Out(*[t.cpu().numpy() if t is not None else None for t in (x, q, zs, steps, en, oe)], chain_z(h)), st


def run_joint_inpaint(h, phar, pocket, fp, fq, K, r, j, noise, use_graph, want_steps=False):
    """The joint model's inpainting chain (test_hip_joint.py's runner; the large-layout tests need it too): device tensors as the binding
    returns them."""
    h.set_layout(phar['size'], pocket['size'])
    return h.joint_chain(K, phar=(dev(phar['x']), dev(phar['one_hot'])), pocket=(dev(pocket['x']), dev(pocket['one_hot'])),
                         phar_fixed=dev(fp), pocket_fixed=dev(fq), resamplings=r, jump_length=j,
                         noise=None if noise is None else dev(noise), use_graph=use_graph, want_steps=want_steps)


def same(a, b, names=None):
    """Bit for bit: the fields `names` of two Outs (default: every field a has), or two sequences of arrays."""
    if isinstance(a, Out):
        names = [n for n in FIELDS if getattr(a, n) is not None] if names is None else names
        a, b = [getattr(a, n) for n in names], [getattr(b, n) for n in names]
    names = range(len(a)) if names is None else names
    assert len(a) == len(b)
    for name, u, v in zip(names, a, b):
        assert u is not None and v is not None and u.shape == v.shape and np.array_equal(u, v), name


# ---------------------------------------------------------------------------------------------------------------------------------------
# the comparison with a yardstick
# ---------------------------------------------------------------------------------------------------------------------------------------
def _np(t):
    return t.numpy() if torch.is_tensor(t) else np.asarray(t)


def parity_ratios(got, want, rows, rows_q, keep=None, final='rms', pocket_cols=None):
    """The worst ratio to each bound of an Out against a yardstick.  want: a mapping with xh_phar, xh_pocket, z_steps, pocket_steps and, for a
    guided chain, energy, max_violation [owners] and op_energy [n_steps, owners]; rows / rows_q: bool masks of the phar / pocket rows
    compared (those of the owners `keep`, bool [owners], which selects the energy terms).

      z, pocket_steps                      per op, max-abs <= PARITY max(1, max|want|)
      x, pocket (the final ones)           final='rms': RMS, final='max': max-abs, <= PARITY max(1, max|want|); x over the coordinates,
                                           pocket over the columns pocket_cols (None: the whole row, one-hot included)
      energy, max_violation, op_energy     elementwise <= PARITY max(1, |want|)

    A mask that selects nothing would compare nothing: refused."""
    rows, rows_q = np.asarray(rows), np.asarray(rows_q)
    assert rows.dtype == bool and rows_q.dtype == bool and rows.any() and rows_q.any(), 'the comparison selects no row'
    assert final in ('rms', 'max')
    cols = slice(None) if pocket_cols is None else pocket_cols
    wx, wq, wzs, wps = (_np(want[k]) for k in PLAIN)
    top = lambda g, w: float(np.abs(g - w).max()) / (PARITY * max(1.0, float(np.abs(w).max())))
    end = top if final == 'max' else lambda g, w: rms(g, w) / (PARITY * max(1.0, float(np.abs(w).max())))
    ratios = {
        'z': max(top(got.z_steps[k][rows], wzs[k][rows]) for k in range(len(wzs))),
        'pocket_steps': max(top(got.pocket_steps[k][rows_q], wps[k][rows_q]) for k in range(len(wps))),
        'x': end(got.xh_phar[rows, :3], wx[rows, :3]),
        'pocket': end(got.xh_pocket[rows_q][:, cols], wq[rows_q][:, cols]),
    }
    if 'energy' in want:
        assert keep is not None and keep.any(), 'the comparison selects no owner'
        rel = lambda g, w: float((np.abs(g - w) / (PARITY * np.maximum(1.0, np.abs(w)))).max())
        ratios['energy'] = rel(got.energy[keep, 0], _np(want['energy'])[keep])
        ratios['max_violation'] = rel(got.energy[keep, 1], _np(want['max_violation'])[keep])
        ratios['op_energy'] = rel(got.op_energy[:, keep], _np(want['op_energy'])[:, keep])
    return ratios


def types_equal(got, want, rows):
    return bool(np.array_equal(got.xh_phar[rows, 3:], _np(want['xh_phar'])[rows, 3:]))


def check_against_ref(label, got, st, want, rows, rows_q, keep, owners, **metric):
    """The parity check of a chain: print the worst ratio to each bound, then assert, in this order, that at most CHAIN_CAP of the owners
    (samples or groups: keep [owners]) were left out, every ratio <= 1, the types exact, and the chain status clean.  metric: parity_ratios'
    final and pocket_cols."""
    ratios = parity_ratios(got, want, rows, rows_q, keep, **metric)
    left_out = int((~keep).sum())
    print(f'\n[{label}] worst ratio to each bound: ' + '  '.join(f'{k} {v:.3f}' for k, v in ratios.items()) +
          f'  left out {left_out} of {len(keep)} {owners}')
    assert left_out <= CHAIN_CAP * len(keep)
    assert all(v <= 1.0 for v in ratios.values()), ratios
    assert types_equal(got, want, rows)
    assert st['nan_resets'] == 0 and st['max_rel_com_error'] < 1e-2


def score_entry_ratios(sums, want_err, want_l0x, netmax, n_rows, keep, P=8):
    """|got - want| / bound (score_ref.error_bound) of every kept scoring entry: error_t of the K levels and loss_0_x of the t = 0 level.
    sums [K + 1, n, 4]; want_err [K, n], want_l0x [n], netmax and keep [K + 1, n]."""
    K = len(want_err)
    netmax = np.asarray(netmax)
    r_t = np.abs(sums[:K, :, 0].astype(np.float64) - want_err) / score_ref.error_bound(want_err, netmax[:K], n_rows, 3 + P)
    r_0 = np.abs(0.5 * sums[K, :, 1].astype(np.float64) - want_l0x) / (0.5 * score_ref.error_bound(2.0 * want_l0x, netmax[K], n_rows, 3))
    return np.concatenate([r_t[keep[:K]], r_0[keep[K]]])


# ---------------------------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------------------------
def record(kind=0, sample=0, i=0, j=0, c=(0.0, 0.0, 0.0), a=1.0, b=0.0, k=1.0):
    q = np.zeros(1, dtype=rs.RESTRAINT_DTYPE)
    q['kind'], q['sample'], q['i'], q['j'], q['c'], q['a'], q['b'], q['k'] = kind, sample, i, j, c, a, b, k
    return q


def refused(h, call, match, code=EINVAL):
    """call() - a closure over the entry under test - raises CmdgenError with the message `match`, and the entry returned `code` (read where
    the binding checks it; a check that fails raises, so the refusing one is the last).  code=None: the message alone."""
    codes, check = [], h._check
    h._check = lambda rc, what: (codes.append(rc), check(rc, what))
    try:
        with pytest.raises(hip_backend.CmdgenError, match=match):
            call()
    finally:
        del h._check
    assert code is None or codes[-1] == code, (match, codes)
