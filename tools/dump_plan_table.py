"""Record which kernels the library resolves for a sweep of configs, engines, options and layouts: every launch key of cmdgen_query, one row
per (config, engine, option, layout), as one integer table (tests/golden/plan_table.npz).  No kernel is launched.

    python tools/dump_plan_table.py OUT.npz

The committed table is a recorded result of the commit BEFORE the launch planner (csrc/cmdgen_plan.h) existed and is never regenerated from
the planner: tests/test_host_cpu.py replays it through the planner on the CPU, tests/test_hip_rule_sweep.py through Handle.query.

Arrays: `rows` [R, len(IN_COLS) + len(QUERY_KEYS)] int32 - the inputs (IN_COLS) then the answers (QUERY_KEYS); `lay_ptr`, `lay_nph`, `lay_npk`
- layout i is samples lay_ptr[i] : lay_ptr[i + 1]; `n_cus` - multi_processor_count of the device the table was recorded on."""
import os
import sys
from dataclasses import replace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

QUERY_KEYS = ('node_mt', 'edge_mt', 'coord_mt', 'edge_grid', 'coord_grid', 'e128_fused', 'gemm_split', 'half_engine', 'node16_split', 'node64',
              'node16w', 'proj_in_coord', 'edge_fullk', 'dead_skip', 'msg_mfmas_per_product', 'node_mfmas_per_product', 'coord_mfmas_per_product')
# the options a row may set (column opt_key indexes this list, -1: none); half_engine has a column of its own (-1: unset)
OPTION_KEYS = ('node_mt', 'edge_mt', 'coord_mt', 'embed_mt', 'edge_wgs_per_cu', 'coord_wgs_per_cu', 'e128_wgs_per_cu', 'e128_fused', 'edge_fullk',
               'node64', 'node16_split', 'node16w', 'proj_in_coord', 'dead_skip')
IN_COLS = ('H', 'L', 'S', 'joint', 'sin', 'no_cutoff', 'gemm_split_mode', 'half_engine_opt', 'opt_key', 'opt_value', 'layout')
ENGINES = (('half', 1, -1), ('bf3', 1, 0), ('half2', 1, 2), ('fp32', 0, -1))       # (name, set_gemm_mode, option half_engine or -1)

SINGLE_OPTIONS = (
    [('node64', v) for v in (0, 1, 2, 8, 32)] + [('node_mt', v) for v in (16, 32, 64, 48)] + [('edge_mt', v) for v in (16, 32, 64, 128, 48)] +
    [('coord_mt', v) for v in (16, 32, 64, 128, 48)] + [('edge_fullk', 0), ('node16w', 0), ('node16_split', 0), ('proj_in_coord', 0), ('proj_in_coord', 1),
                                                        ('dead_skip', 0), ('dead_skip', 1)] +
    [('e128_fused', v) for v in (0, 1, 2, 3)] + [('edge_wgs_per_cu', v) for v in (1, 3)] + [('coord_wgs_per_cu', v) for v in (1, 3)] +
    [('e128_wgs_per_cu', v) for v in (1, 3)] + [('embed_mt', v) for v in (16, 32, 64, 48)])
OPTION_SIZES = (1, 4, 9, 47, 70, 78, 106, 139, 176, 278)          # one per regime of the default engine on 256 CUs (tests/rule_sweep_ref.py)
VARIANT_SIZES = (1, 3, 8, 16, 32, 48, 64, 96, 128, 160, 224, 320)


def main(out):
    import torch
    import rule_sweep_ref as rs
    from bench import bounded_config
    from cmdgen_amd import hip_backend
    from cmdgen_amd.synthetic import make_pockets, make_state_dict
    assert not hip_backend.DEFAULT_OPTIONS
    n_cus = torch.cuda.get_device_properties(0).multi_processor_count

    layouts, lay_index = [], {}

    def layout_id(nph, npk):
        key = (np.asarray(nph, np.int64).tobytes(), np.asarray(npk, np.int64).tobytes())
        if key not in lay_index:
            lay_index[key] = len(layouts)
            layouts.append((np.asarray(nph, np.int64), np.asarray(npk, np.int64)))
        return lay_index[key]

    uniform = [layout_id([15] * B, [44] * B) for B in range(1, 321)]
    ragged = []
    for c in rs.ONE_EVALUATION + rs.CHAIN_CASES:
        pb = rs.pockets_of(c)
        i = layout_id(pb.num_nodes_phar, pb.size)
        if i not in ragged:
            ragged.append(i)
    full_atom = []
    for B in (1, 2, 4, 8, 16, 32, 64, 128):
        for rag in (False, True):
            pb = make_pockets(B, 'full-atom', ragged=rag, first_index=rs.FIRST_INDEX)
            full_atom.append(layout_id(pb.num_nodes_phar, pb.size))
    sized = lambda sizes: [uniform[B - 1] for B in sizes]

    base = bounded_config(20, 1000)
    rows = []

    def sweep(cfg, engines, lays, options=((None, 0),)):
        h = hip_backend.Handle(cfg.as_dict(), 0)
        h.load_state_dict(make_state_dict(cfg, seed=0))
        big = max(lays, key=lambda i: int((layouts[i][0] + layouts[i][1]).sum()))
        h.set_layout(*layouts[big])                             # the workspaces grow once
        head = [cfg.hidden_nf, cfg.n_layers, cfg.inv_sublayers, int(cfg.update_pocket_coords), int(cfg.sin_embedding), int(cfg.edge_cutoff is None)]
        for _, split, he in engines:
            if not cfg.sin_embedding:
                h.set_gemm_mode(bool(split))
            h.set_option('half_engine', None if he < 0 else he)
            for key, val in options:
                if key is not None:
                    h.set_option(key, val)
                for i in lays:
                    h.set_layout(*layouts[i])
                    rows.append(head + [split, he, -1 if key is None else OPTION_KEYS.index(key), val, i] + [int(h.query(k)) for k in QUERY_KEYS])
                if key is not None:
                    h.set_option(key, None)
        h.close()

    for joint in (False, True):
        cfg = replace(base, update_pocket_coords=joint)
        sweep(cfg, ENGINES, uniform + ragged + full_atom)
        sweep(cfg, ENGINES[:2] if not joint else ENGINES[:1], sized(OPTION_SIZES) + full_atom[6:8], SINGLE_OPTIONS)
    for cfg in (replace(base, hidden_nf=64), replace(base, hidden_nf=128), replace(base, hidden_nf=512), replace(base, inv_sublayers=2),
                replace(base, edge_cutoff=None)):
        sweep(cfg, ENGINES, sized(VARIANT_SIZES) + full_atom[4:6])
    sweep(replace(base, sin_embedding=True), (('fp32', 0, -1), ('fp32', 0, 2)), sized(VARIANT_SIZES) + full_atom[4:6])
    sweep(replace(base, sin_embedding=True, hidden_nf=512), (('fp32', 0, -1),), sized(VARIANT_SIZES) + full_atom[4:6])

    rows = np.asarray(rows, dtype=np.int32)
    lay_ptr = np.concatenate([[0], np.cumsum([len(a) for a, _ in layouts])]).astype(np.int32)
    np.savez_compressed(out, rows=rows, lay_ptr=lay_ptr, lay_nph=np.concatenate([a for a, _ in layouts]).astype(np.int32),
                        lay_npk=np.concatenate([b for _, b in layouts]).astype(np.int32), n_cus=np.asarray([n_cus], np.int32))
    print(f'{len(rows)} rows, {len(layouts)} layouts, {n_cus} CUs -> {out} ({os.path.getsize(out)} bytes)')


if __name__ == '__main__':
    main(sys.argv[1])
