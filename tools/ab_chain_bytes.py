#!/usr/bin/env python
"""Byte comparison of the derived chains between two builds of the library (profiles/step_parts_refactor.txt): one process per dump, so that
two builds can alternate on one device through CMDGEN_LIB.
  ab_chain_bytes.py dump OUT.npz          every case below through the library CMDGEN_LIB names (default: the in-tree one): every output array
  ab_chain_bytes.py compare A.npz B.npz   the arrays that differ in any byte (exit status 1 if any does)
Cases: the seven wrappers that reach the seven derived chain kinds - inpaint, edit, multi-pocket, multi-pocket edit, restrained, restrained
edit, restrained multi-pocket and restrained multi-pocket edit - each with device Philox draws and with injected noise, eager and captured
(graph_steps = 2), on two layouts: six member samples in groups of 1, 2 and 3 with 5 / 9 / 7 points and 20 .. 40 pocket atoms, one member of
weight 0 (max_n <= 128: 256-thread step kernels), and the same with one pocket of 150 atoms (max_n > 128: 1024 threads).  The per-sample
chains take the first members' pockets.  timesteps = 6; the edit kinds run resamplings = jump_length = 2 from the prior and from start = 4;
group 0 has no mark, group 1 only held x, group 2 only held types; one position restraint, one distance restraint between a held and a free
point and one exclusion sphere, with the clash term on and off, with and without op_energy, guide_below = 0.5 (ops 3 .. 5 guided, 0 .. 2 not).
Stored per case: xh_phar, xh_pocket, z_steps, pocket_steps, energy and op_energy where the chain has them, the "chain_z" debug read and the
chain status."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K, R, J, START = 6, 2, 2, 4
SIZES, NPH = (1, 2, 3), (5, 9, 7)
WEIGHTS = np.array([1.0, 0.3, 0.7, 0.6, 0.0, 0.4], dtype=np.float32)
ATOMS = {'small': (23, 37, 20, 31, 40, 26), 'large': (23, 37, 150, 31, 40, 26)}
CLASH = (3.0, 1.0)


def pockets(atoms):
    from cmdgen_amd.synthetic import PocketBatch, make_pockets
    # (make_pockets' own density: a receiver's edges then span at most two tiles of the edge kernels, whose float-atomic partial sums are
    # reproducible only up to two - the premise of every bit-for-bit test of the suite, tests/test_hip_edit.py)
    one = [make_pockets(1, 'CA', n_pocket_nodes=n, radius=16.0 if n > 128 else 12.0, first_index=700 + m) for m, n in enumerate(atoms)]
    size = np.asarray(atoms, dtype=np.int64)
    return PocketBatch(x=np.concatenate([p.x for p in one]), one_hot=np.concatenate([p.one_hot for p in one]), size=size,
                       mask=np.repeat(np.arange(len(atoms), dtype=np.int64), size), num_nodes_phar=np.repeat(np.asarray(NPH, dtype=np.int64), SIZES))


def first_members(pb):
    """the per-sample layout: the first member of every group"""
    from cmdgen_amd.synthetic import PocketBatch
    firsts = np.concatenate([[0], np.cumsum(SIZES)[:-1]])
    keep = np.isin(pb.mask, firsts)
    size = pb.size[firsts]
    return PocketBatch(x=pb.x[keep], one_hot=pb.one_hot[keep], size=size, mask=np.repeat(np.arange(len(firsts), dtype=np.int64), size),
                       num_nodes_phar=np.asarray(NPH, dtype=np.int64))


def given_rows():
    """(phar_x, phar_onehot, fix_x, fix_h) over the 21 rows: group 0 without a mark, group 1 with x held on its even rows, group 2 with its types
    held on every third row"""
    rng = np.random.default_rng(11)
    nu, owner = int(sum(NPH)), np.repeat(np.arange(len(NPH)), NPH)
    local = np.concatenate([np.arange(n) for n in NPH])
    x = (rng.normal(size=(nu, 3)) * 2.5).astype(np.float32)
    oh = np.eye(8, dtype=np.float32)[rng.integers(0, 8, size=nu)]
    fx = ((owner == 1) & (local % 2 == 0)).astype(np.float32)
    fh = ((owner == 2) & (local % 3 == 0)).astype(np.float32)
    return x, oh, fx, fh


def restraint_records():
    from cmdgen_amd import restraints as rs
    lst = [{'kind': 'position', 'sample': 0, 'point': 1, 'center': (1.0, -0.5, 0.5), 'radius': 1.0, 'k': 1.0},
           {'kind': 'distance', 'sample': 1, 'points': (0, 1), 'lo': 4.0, 'hi': 6.0, 'k': 1.0},      # point 0 held, point 1 free
           {'kind': 'exclusion', 'sample': 2, 'center': (0.5, 0.5, -1.0), 'radius': 3.0, 'k': 0.5}]
    return rs.records(lst, np.asarray(NPH, dtype=np.int64))


def dump(out):
    sys.path.insert(0, ROOT)
    import torch
    from cmdgen_amd import hip_backend
    from cmdgen_amd.synthetic import make_state_dict
    from bench import bounded_config

    cfg = bounded_config(20, 1000)
    h = hip_backend.Handle(cfg.as_dict(), 0)
    h.load_state_dict(make_state_dict(cfg, seed=0))
    h.set_option('graph_steps', 2)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    given = [dev(a) for a in given_rows()]
    rec = restraint_records()
    rows = int(sum(NPH))
    res = {}

    def keep(tag, outs, names):
        torch.cuda.synchronize()
        for name, t in zip(names, outs):
            if t is not None:
                res[f'{tag}/{name}'] = t.cpu().numpy()
        if h.last_pocket_steps is not None:
            res[f'{tag}/pocket_steps'] = h.last_pocket_steps.cpu().numpy()
        res[f'{tag}/chain_z'] = h.debug_read('chain_z', int(np.sum(h.num_phar_host)) * 11)
        st = h.chain_status()
        res[f'{tag}/status'] = np.array([float(st[k]) for k in sorted(st)], dtype=np.float64)

    plain = ('xh_phar', 'xh_pocket', 'z_steps')
    guided = plain + ('energy', 'op_energy')
    for layout, atoms in ATOMS.items():
        members = pockets(atoms)
        singles = first_members(members)
        for draws in ('philox', 'injected'):
            for graph in (True, False):
                def noise(n_draws):
                    if draws == 'philox':
                        return None
                    return torch.randn((n_draws, rows, 11), generator=torch.Generator().manual_seed(1000 + n_draws)).cuda()
                mode = f'{layout}/{draws}/{"captured" if graph else "eager"}'
                # ---- one sample per pocket
                h.set_layout(singles.num_nodes_phar, singles.size)
                px, poh = dev(singles.x), dev(singles.one_hot)
                n_draws = h.edit_plan(K, K, R, J)[1]
                keep(f'{mode}/inpaint', h.inpaint_chain(px, poh, given[0], given[1], given[2], K, R, J, noise=noise(n_draws), seed=7, want_steps=True,
                                                        use_graph=graph), plain)
                for start in (K, START):
                    n_draws = h.edit_plan(K, start, R, J)[1]
                    keep(f'{mode}/edit_start{start}', h.edit_chain(px, poh, *given, K, start, R, J, noise=noise(n_draws), seed=7, want_steps=True,
                                                                   use_graph=graph), plain)
                    for clash, steps in ((CLASH, True), ((0.0, 0.0), True), (CLASH, False)):
                        keep(f'{mode}/restrained_edit_start{start}_clash{clash[0]:g}_steps{int(steps)}',
                             h.restrained_edit_chain(px, poh, *given, K, start, R, J, restraints=rec, clash_radius=clash[0], clash_k=clash[1],
                                                     guide_below=0.5, noise=noise(n_draws), seed=7, want_steps=steps, use_graph=graph), guided)
                for clash, steps in ((CLASH, True), ((0.0, 0.0), True), (CLASH, False)):
                    keep(f'{mode}/restrained_clash{clash[0]:g}_steps{int(steps)}',
                         h.restrained_chain(px, poh, K, rec, clash_radius=clash[0], clash_k=clash[1], guide_below=0.5, noise=noise(K + 2), seed=7,
                                            want_steps=steps, use_graph=graph), guided)
                # ---- groups of members
                h.set_layout(members.num_nodes_phar, members.size)
                px, poh = dev(members.x), dev(members.one_hot)
                keep(f'{mode}/multi_pocket', h.multi_pocket_chain(px, poh, SIZES, WEIGHTS, K, noise=noise(K + 2), seed=7, want_steps=True, use_graph=graph),
                     plain)
                for clash, steps in ((CLASH, True), ((0.0, 0.0), True), (CLASH, False)):
                    keep(f'{mode}/multi_restrained_clash{clash[0]:g}_steps{int(steps)}',
                         h.multi_restrained_chain(px, poh, SIZES, WEIGHTS, K, rec, clash_radius=clash[0], clash_k=clash[1], guide_below=0.5,
                                                  noise=noise(K + 2), seed=7, want_steps=steps, use_graph=graph), guided)
                for start in (K, START):
                    n_draws = h.edit_plan(K, start, R, J)[1]
                    keep(f'{mode}/multi_edit_start{start}', h.multi_edit_chain(px, poh, SIZES, WEIGHTS, *given, K, start, R, J, noise=noise(n_draws),
                                                                               seed=7, want_steps=True, use_graph=graph), plain)
                    for clash, steps in ((CLASH, True), ((0.0, 0.0), True), (CLASH, False)):
                        keep(f'{mode}/multi_restrained_edit_start{start}_clash{clash[0]:g}_steps{int(steps)}',
                             h.multi_restrained_edit_chain(px, poh, SIZES, WEIGHTS, *given, K, start, R, J, restraints=rec, clash_radius=clash[0],
                                                           clash_k=clash[1], guide_below=0.5, noise=noise(n_draws), seed=7, want_steps=steps,
                                                           use_graph=graph), guided)
    h.close()
    np.savez(out, **res)
    nbytes = sum(v.nbytes for v in res.values())
    nonfinite = sum(int(not np.isfinite(v).all()) for v in res.values())
    print(f'wrote {out}: {len(res)} arrays, {nbytes} bytes, {nonfinite} with a non-finite value, library {os.environ.get("CMDGEN_LIB", hip_backend.library_path())}')


def compare(fa, fb):
    a, b = np.load(fa), np.load(fb)
    only = sorted(set(a.files) ^ set(b.files))
    differ = [k for k in sorted(set(a.files) & set(b.files))
              if a[k].dtype != b[k].dtype or a[k].shape != b[k].shape or a[k].tobytes() != b[k].tobytes()]
    for k in only:
        print('in one file only:', k)
    for k in differ:
        n = int((a[k] != b[k]).sum()) if a[k].shape == b[k].shape else -1
        print(f'differs: {k} ({n} of {a[k].size} values)')
    print(f'{fa} against {fb}: {len(a.files)} arrays, {len(differ)} differ, {len(only)} in one file only')
    return 1 if differ or only else 0


if __name__ == '__main__':
    if len(sys.argv) == 3 and sys.argv[1] == 'dump':
        dump(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == 'compare':
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
