"""CPU suite for the host layer: C-ABI symbol check, schedule table, node-count prior, masks,
PDB reader / generate_phars bookkeeping, checkpoint format, failure without a GPU."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

from helpers import host_hparams as _hparams, load_golden, small_ddpm
import cmdgen_amd  # noqa: F401
from cmdgen_amd import hip_backend, utils
from cmdgen_amd.constants import dataset_params
from cmdgen_amd.equivariant_diffusion.en_diffusion import DistributionNodes, PredefinedNoiseSchedule
from cmdgen_amd.equivariant_diffusion.dynamics import EGNNDynamics
from cmdgen_amd.lightning_modules import PharPocketDDPM
from cmdgen_amd.synthetic import ModelConfig, make_state_dict, linear_specs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    """The in-tree .so loads (no GPU needed) and exports every function include/cmdgen_hip.h declares."""
    hdr = open(os.path.join(ROOT, 'include', 'cmdgen_hip.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    declared = set(re.findall(r'\b(cmdgen_[a-z_0-9]+)\s*\(', hdr))
    assert len(declared) >= 17
    lib = hip_backend.load_library()
    for name in declared:
        assert hasattr(lib, name), name
    bound = {n for n, _, _ in hip_backend.SYMBOLS}
    assert declared == bound, declared ^ bound
    assert b'gfx950' in lib.cmdgen_version()
    assert ctypes.sizeof(hip_backend.Config) == 21 * 4 and ctypes.sizeof(hip_backend.Counters) == 64


def test_library_source_reads_no_environment_variable():
    """Launch choices are per-handle options (cmdgen_set_option); the C ABI library has no process-global switches."""
    csrc = os.path.join(ROOT, 'cmdgen_amd', 'csrc')
    for f in os.listdir(csrc):
        if f.endswith(('.hip', '.h')):
            assert 'getenv' not in open(os.path.join(csrc, f)).read(), f


def _file_scope_declarations(code):
    """(text joined to one line, ';' or '{') of every declaration at brace depth 0 of comment-free code"""
    out, depth, cur = [], 0, []
    for ch in code:
        if ch == '{':
            if depth == 0:
                out.append((' '.join(''.join(cur).split()), '{'))
                cur = []
            depth += 1
        elif ch == '}':
            depth -= 1
        elif depth == 0 and ch == ';':
            out.append((' '.join(''.join(cur).split()), ';'))
            cur = []
        elif depth == 0:
            cur.append(ch)
    assert depth == 0
    return out


def test_library_source_declares_each_struct_and_launcher_once():
    """What two translation units must agree on is written once, in a header both include: no struct is defined in two files of
    csrc/ (a table struct copied into the host file and the kernel file can drift apart, and the kernel then indexes the uploaded
    table with the wrong stride), and no .hip file carries a bare prototype of a cmdgen_* / tr_* function or an extern object
    declaration (a copied prototype with default arguments silently passes stale defaults)."""
    csrc = os.path.join(ROOT, 'cmdgen_amd', 'csrc')
    proto = re.compile(r'^(?:extern C_LINKAGE )?(?:template ?<[^>]*> ?)?(?:[\w:]+[ *&]+)+((?:cmdgen_|tr_)\w+) ?\(')
    structs, prototypes = {}, []
    for f in sorted(os.listdir(csrc)):
        if not f.endswith(('.hip', '.h')):
            continue
        code = open(os.path.join(csrc, f)).read()
        code = re.sub(r'/\*.*?\*/', ' ', code, flags=re.S)                      # comments, preprocessor lines, literals
        code = re.sub(r'//[^\n]*', '', code)
        code = re.sub(r'(?m)^[ \t]*#(?:[^\n]*\\\n)*[^\n]*', '', code)
        code = code.replace('"C"', 'C_LINKAGE')
        code = re.sub(r'"(?:\\.|[^"\\\n])*"', '""', code)
        code = re.sub(r"'(?:\\.|[^'\\\n])'", "' '", code)
        for name in set(re.findall(r'\bstruct\s+(\w+)\s*(?::[^;{()]*)?\{', code)):
            structs.setdefault(name, []).append(f)
        if not f.endswith('.hip'):
            continue
        for text, end in _file_scope_declarations(code):                          # multi-line prototypes arrive joined
            if end != ';' or text.startswith(('static ', 'typedef ', 'using ')):
                continue
            if proto.match(text) or (text.startswith('extern ') and not text.startswith('extern C_LINKAGE ')):
                prototypes.append((f, text))
    twice = {name: files for name, files in structs.items() if len(files) > 1}
    assert not twice, twice
    assert not prototypes, prototypes
    assert len(structs) > 30 and 'RepackHalf16' in structs and 'WPack' in structs       # the scan sees the structs it is about


def test_half_scale_rule_equals_both_rules_it_replaced(tmp_path):
    """tests/whalf_exp_check.cpp: whalf_exp (cmdgen_wlayout.h) against the former host and device rules, on the host."""
    import subprocess
    exe = str(tmp_path / 'whalf_exp_check')
    r = subprocess.run(['/opt/rocm/bin/hipcc', '-x', 'hip', '--offload-arch=gfx950', '-O2', '-I' + os.path.join(ROOT, 'cmdgen_amd', 'csrc'),
                        os.path.join(ROOT, 'tests', 'whalf_exp_check.cpp'), '-o', exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and 'bad 0' in r.stdout, (r.stdout + r.stderr)[-2000:]
    assert int(r.stdout.split('checked')[1].split()[0]) > 2500


def test_planner_reproduces_the_recorded_launch_table():
    """tests/plan_check.cpp: the launch planner (csrc/cmdgen_plan.h) on the host against every row of tests/golden/plan_table.npz - the launch keys
    cmdgen_query gave BEFORE the planner existed, for a sweep of configs, engines, options and layouts, with n_cus taken from the table."""
    import plan_table_ref as pt
    t = pt.table()
    assert len(t['rows']) > 4000 and t['rows'].shape[1] == pt.N_IN + len(pt.QUERY_KEYS)
    got = pt.run_planner(t['layouts'], pt.table_plans())
    want = t['rows'][:, pt.N_IN:]
    bad = np.flatnonzero((got != want).any(axis=1))
    assert len(bad) == 0, [(pt.describe(t['rows'][i]), {k: (int(w), int(g)) for k, w, g in zip(pt.QUERY_KEYS, want[i], got[i]) if w != g}) for i in bad[:5]]


def test_planner_names_the_kernels_the_former_launchers_took():
    """The query keys are not what the launchers switch on: the kernel of each role, its engine and the 128-row kernels' grid are.  Before the
    planner, each launcher tested the launch keys itself and fell through to the next; those guards, applied here to the RECORDED keys of every
    row of the table (weights uploaded, sampler), must name the kernel the planner names."""
    import plan_table_ref as pt
    t = pt.table()
    plans = pt.table_plans()
    got = pt.run_planner(t['layouts'], plans, extra=True)[:, len(pt.QUERY_KEYS):]
    for row, p, g in zip(t['rows'], plans, got):
        q = dict(zip(pt.QUERY_KEYS, (int(v) for v in row[pt.N_IN:])))
        H, split, he = p['H'], q['gemm_split'], p['opts'].get('half_engine', 1)
        half = he == 2 or (he == 1 and not p['no_cutoff'])
        sp256 = H == 256 and split
        eng256 = pt.ENG['half'] if half else pt.ENG['bf3']                       # (ws and wh exist for every uploaded matrix)

        def edge_role(mt, e128, fullk, tiles):
            if mt == 128 and sp256:
                return e128, eng256
            if q['edge_fullk'] and sp256 and mt == 32:
                return fullk, eng256
            return tiles, pt.ENG['bf3'] if split and mt >= 32 else pt.ENG['fp32']
        msg = edge_role(q['edge_mt'], pt.MSG['e128'], pt.MSG['fullk32'], pt.MSG['tiles'])
        coord = edge_role(q['coord_mt'], pt.COORD['e128'], pt.COORD['fullk32'], pt.COORD['tiles'])
        if q['proj_in_coord']:
            assert coord[0] == pt.COORD['fullk32']
            coord = pt.COORD['fullk32_proj'], coord[1]
        ws16 = (2 * H) % 128 == 0                                                 # node_mlp.0 takes 2H inputs
        if q['node64'] and sp256:
            n64 = q['node64']
            node = (pt.NODE['node64d'] if n64 == 2 and half else pt.NODE['node64e'] if n64 == 8 and half else pt.NODE['node32p'] if n64 == 32
                    else pt.NODE['node64']), eng256
        elif H == 256 and q['node_mt'] == 16 and q['node16_split'] and q['node16w'] and ws16:
            node = pt.NODE['node16w'], eng256
        elif q['node_mt'] >= 32:
            node = pt.NODE['tiles'], pt.ENG['bf3'] if split else pt.ENG['fp32']
        else:
            node = pt.NODE['tiles'], pt.ENG['bf3'] if q['node16_split'] and ws16 and H >= 128 else pt.ENG['fp32']
        wgs = p['opts'].get('e128_wgs_per_cu', 2)
        nph = t['layouts'][p['layout']][0]
        embed = p['opts'].get('embed_mt', 16 if int(nph.sum()) / 16.0 <= 2.0 * p['n_cus'] and not p['joint'] else q['node_mt'])
        if embed not in (16, 32, 64):
            embed = q['node_mt']
        want = dict(msg=msg[0], node=node[0], coord=coord[0], msg_eng=msg[1], node_eng=node[1], coord_eng=coord[1],
                    e128_grid=(wgs if 1 <= wgs <= 4 else 2) * p['n_cus'], embed_mt=embed, write_embed=1,
                    reads_frag=int(pt.MSG['tiles'] == msg[0] or pt.COORD['tiles'] == coord[0] or pt.NODE['tiles'] == node[0]), fwd_half=0, node_half=0)
        assert dict(zip(pt.EXTRA_KEYS, (int(v) for v in g))) == want, (pt.describe(row), q)
    # (no row of the table sets write_embed; make_launch read it as `opt_of(h, "write_embed", 1) != 0`)
    few = [dict(p, opts=dict(p['opts'], write_embed=v)) for p in plans[:3] for v in (0, 1, 5)]
    assert list(pt.run_planner(t['layouts'], few, extra=True)[:, len(pt.QUERY_KEYS) + pt.EXTRA_KEYS.index('write_embed')]) == [0, 1, 1] * 3


def test_planner_training_mode_is_the_former_training_forwards_patches():
    """cmdgen_train_forward used to patch the sampler's launch after the fact (train_half, train_node16, rows / grids from the real list lengths,
    the half save forms) and to predict from its own copy of the launchers' guards whether a launch would read the fp32 fragment packs.  Those
    rules, applied to the planner's sampler answer (pinned by the recorded table), against the planner's training mode."""
    import plan_table_ref as pt
    t = pt.table()
    n_cus, cases = 256, []
    for layout in (7, 63, 199):                                                                   # 8, 64 and 200 uniform C-alpha pockets
        for H, split, opts in ((256, 1, {}), (256, 1, {'half_engine': 0}), (256, 0, {}), (128, 1, {})):
            for extra in ({}, {'train_half': 0}, {'train_half': 2}, {'train_node16': 0}, {'edge_mt': 64}, {'edge_mt': 128}, {'edge_mt': 16, 'coord_mt': 128},
                          {'edge_fullk': 0}, {'edge_wgs_per_cu': 1, 'edge_mt': 32}):
                for packs in (7, 3, 1, 0):
                    for E, Ec in ((100, 50), (34000, 9000), (300000, 70000)):
                        cases.append(dict(H=H, L=5, S=1, joint=0, sin=0, no_cutoff=0, n_cus=n_cus, gemm_split=split, layout=layout, opts=dict(opts, **extra),
                                          packs=packs, E=E, Ec=Ec))
    sampler = pt.run_planner(t['layouts'], [dict(c, packs=1) for c in cases])
    got = pt.run_planner(t['layouts'], [dict(c, training=1) for c in cases], extra=True)
    keys = pt.QUERY_KEYS + pt.EXTRA_KEYS
    seen = set()
    for c, s, g in zip(cases, sampler, got):
        q, g = dict(zip(pt.QUERY_KEYS, (int(v) for v in s))), dict(zip(keys, (int(v) for v in g)))
        o, H, split = c['opts'], c['H'], c['gemm_split']
        fwd_half = bool(split and H == 256 and q['half_engine'] and q['edge_fullk'] and c['packs'] & 2 and o.get('train_half', 1) != 0)
        node_mt = 16 if fwd_half and o.get('train_node16', 1) != 0 else q['node_mt']
        node_half = bool(fwd_half and node_mt == 16 and c['packs'] & 4 and o.get('train_half', 1) != 2)
        rows = lambda n: 64 if n // 64 >= 4 * n_cus else 32 if n // 32 >= n_cus // 4 else 16
        grid = lambda n, mt: min(max(int((n // mt + 1) * 1.25) + 8, n_cus // 4), (2 if mt >= 64 else 4) * n_cus)
        want = {}
        for role, mt_key, grid_key, n in (('msg', 'edge_mt', 'edge_grid', c['E']), ('coord', 'coord_mt', 'coord_grid', c['Ec'])):
            mt, gr = q[mt_key], q[grid_key]
            if mt_key not in o or mt == 128:
                mt = rows(n); gr = grid(n, mt)
            if fwd_half:
                mt, gr = 32, grid(n, 32)
            sp = split and c['packs'] & 1 and H == 256 and mt >= 32
            want.update({mt_key: mt, grid_key: gr, role: 1 if fwd_half else 0, role + '_eng': pt.ENG['half'] if fwd_half else pt.ENG['bf3'] if sp else pt.ENG['fp32']})
        node16w = H == 256 and node_mt == 16 and node_half
        want.update(node_mt=node_mt, node=pt.NODE['node16w'] if node16w else pt.NODE['tiles'], node_eng=pt.ENG['half'] if node16w else pt.ENG['fp32'],
                    fwd_half=int(fwd_half), node_half=int(node_half), reads_frag=int(not (fwd_half and node16w)), dead_skip=0, node64=0, proj_in_coord=0)
        assert {k: g[k] for k in want} == want, (c, q)
        seen.add((want['fwd_half'], want['node_half'], want['reads_frag'], want['edge_mt']))
    assert {s[:3] for s in seen} == {(1, 1, 0), (1, 0, 1), (0, 0, 1)} and {s[3] for s in seen} == {16, 32, 64}       # the cases reach every outcome


def test_planner_header_is_plain_cpp():
    """cmdgen_plan.h takes no HIP header and no cmdgen_handle (plan_check.cpp compiles it with -x c++), and before cmdgen_finalize_weights - no
    packs - every role resolves to a kernel that needs none."""
    import plan_table_ref as pt
    src = open(os.path.join(ROOT, 'cmdgen_amd', 'csrc', 'cmdgen_plan.h')).read()
    assert all(inc.startswith('<') and 'hip' not in inc for inc in re.findall(r'#include\s+(\S+)', src)) and 'cmdgen_handle' not in src
    t = pt.table()
    plans = [dict(p, packs=0) for p in pt.table_plans()[:320]]                  # uniform C-alpha layouts of 1 .. 320 pockets, the default engine
    got = pt.run_planner(t['layouts'], plans)
    k = {key: i for i, key in enumerate(pt.QUERY_KEYS)}
    assert (got[:, k['proj_in_coord']] == 0).all()
    for role in ('msg', 'node', 'coord'):
        assert np.isin(got[:, k[role + '_mfmas_per_product']], (1, 6)).all()                          # (the half forms need their packs)
    assert (got[:, k['node_mfmas_per_product']] == np.where(got[:, k['node_mt']] >= 32, 6, 1)).all()


def _train_plan_sweep():
    """Every case of the training-step planner sweep: weight-gradient groups, plain GEMMs, data gradients (tests/train_plan_ref.py: run_planner)."""
    import train_plan_ref as tp
    Ks = (1, 63, 64, 127, 128, 129, 3721, 8191, 8192, 16127, 32767, 32768, 36147, 65535, 65536, 156316)
    sq = tp.shape(256, 256)
    groups = [[sq], [sq] * 3, [sq] * 4, [sq] * 7, [sq] * 8,               # 3 / 4: the two node-level groups of a block (coord_mlp.0's halves + node_mlp.2; node_mlp.0's + edge_mlp.0's)
              [tp.shape(256, 512), sq],                                   # a whole 256 x 512 first layer beside one of its halves
              [tp.shape(64, 128)], [tp.shape(40, 24)],                    # 64-tile only; the generic kernel only
              [tp.shape(256, 256, aligned=0)], [sq, tp.shape(256, 256, lddy_mod4=2)], [tp.shape(256, 256, ldx_mod4=1), sq]]
    tunes = [dict(tp.TUNE)] + [dict(tp.TUNE, **o) for o in ({'wgrad_split': 0}, {'wgrad_split': 1}, {'wgrad_tile': 64}, {'wgrad_k128': 1},
                                                           {'wgrad_split_wgs128': 100}, {'wgrad_split_wgs64': 100}, {'wgrad_wgs': 100})]
    cases = []
    for tune in tunes:
        for g in groups:
            for xs in (0, 1):
                shapes = [s[:5] + (xs,) if i == 0 else s for i, s in enumerate(g)]
                for K in Ks:
                    for flags in range(8):
                        cases.append(('wgrad', tune, shapes, K, flags & 1, (flags >> 1) & 1, (flags >> 2) & 1))
    gemm_shapes = [(64, 64, 16), (70, 33, 20), (1, 256, 514), (300, 8, 11), (257, 129, 1000), (5, 5, 3), (24, 64, 5000),      # test_training_gemm_all_layouts
                   (31 * 64, 33 * 64, 72), (2048, 2048, 72), (256, 256, 36147), (2048, 2048, 1000)]                          # 1023 and 1024 workgroups; long K
    for M, N, K in gemm_shapes:
        for split_k in (0, 1, 7):
            for bits in range(32):
                for epi in (0, 1, 2):
                    cases.append(('sgemm', bits & 1, (bits >> 1) & 1, M, N, K, (bits >> 2) & 1, (bits >> 3) & 1, split_k, (bits >> 4) & 1, epi))
    for mt in (0, 32, 64):
        tune = dict(tp.TUNE, dgrad_mt=mt)
        for M in (1, 24575, 24576, 100000):
            for force in (0, 32, 64):
                cases.append(('dgrad', tune, M, force))
    return cases


def test_training_planners_are_the_former_launchers_decisions():
    """tests/train_plan_check.cpp: plan_wgrad, plan_sgemm and plan_dgrad (csrc/cmdgen_train_plan.h) on the host against the rules cmdgen_wgrad_group,
    cmdgen_sgemm and cmdgen_dgrad_split evaluated themselves before the header existed (tests/train_plan_ref.py, transcribed from that source): every
    field of every plan, over a sweep that is checked to reach every outcome and both sides of every threshold."""
    import train_plan_ref as tp
    cases = _train_plan_sweep()
    got = tp.run_planner(cases)
    bad = [(c, g, tp.reference(c)) for c, g in zip(cases, got) if g != tp.reference(c)]
    assert not bad, (len(bad), bad[:3])
    w = [(c, g) for c, g in zip(cases, got) if c[0] == 'wgrad']
    assert {g[:3] for _, g in w} == {(k, p, x) for k in (tp.GROUP, tp.SPLIT64, tp.SPLIT128) for p in (1, 3) for x in (0, 1)}     # kernel x pieces x xs
    # the threshold K x 128-tiles >= wgrad_k128: default options, three pieces by the engine (not forced), shapes the 128-tile kernel takes
    fits128 = lambda shapes: all(s[0] % 128 == 0 and s[1] % 128 == 0 and s[2] == 0 and s[3] == 0 and s[4] for s in shapes)
    by_rule = {(c[3] * sum((s[0] // 128) * (s[1] // 128) for s in c[2]) >= tp.TUNE['wgrad_k128'], g[0]) for c, g in w
               if c[1] == tp.TUNE and (c[4], c[5], c[6]) == (0, 1, 0) and fits128(c[2])}
    assert by_rule == {(False, tp.SPLIT64), (True, tp.SPLIT128)}
    by_k = {(c[3] >= 65536, g[0]) for c, g in w if c[1] == tp.TUNE and (c[4], c[6]) == (1, 0) and fits128(c[2])}                # bf16 operands: K >= 65536
    assert by_k == {(False, tp.SPLIT64), (True, tp.SPLIT128)} and {c[3] for c, _ in w} >= {65535, 65536}
    s = [(c, g) for c, g in zip(cases, got) if c[0] == 'sgemm']
    assert {(g[1] * g[2] * g[3] >= 1024, g[0]) for _, g in s} == {(False, 64), (True, 32)}                                         # 1024 workgroups: the k tile
    assert {g[1] * g[2] * g[3] for _, g in s} >= {1023, 1024} and {g[7] for _, g in s} == set(range(64))                           # ... and every instantiation
    assert {g[5] > 1 for _, g in s} == {False, True} and all(g[6] == (0 if g[5] > 1 else c[10]) for c, g in s)
    d = [(c, g) for c, g in zip(cases, got) if c[0] == 'dgrad']
    assert {(c[2] >= 24576, g[0]) for c, g in d if c[1]['dgrad_mt'] == 0 and c[3] == 0} == {(False, 32), (True, 64)}               # 24576 rows: the tile
    assert {c[2] for c, _ in d} >= {24575, 24576} and {g[0] for c, g in d if c[2] == 1} == {32, 64}                                # (an option or a test overrides it)


def test_training_planner_fixed_points():
    """The thresholds of the weight-gradient and data-gradient rules at their defaults, as literals: a 256 x 256 product has four 128 x 128 tiles, so
    K x tiles >= 131072 is K >= 32768 for one product and K >= 8192 for four; bf16 operands change at 65536 rows; the data gradient at 24576."""
    import train_plan_ref as tp
    one, four = [tp.shape(256, 256)], [tp.shape(256, 256)] * 4
    tune = dict(tp.TUNE)
    assert tune['wgrad_k128'] == 131072 and tune['wgrad_split'] == -1 and tune['dgrad_mt'] == 0
    got = tp.run_planner([('wgrad', tune, one, 32767, 0, 1, 0), ('wgrad', tune, one, 32768, 0, 1, 0),
                          ('wgrad', tune, four, 8191, 0, 1, 0), ('wgrad', tune, four, 8192, 0, 1, 0),
                          ('wgrad', tune, one, 65535, 1, 1, 0), ('wgrad', tune, one, 65536, 1, 1, 0),
                          ('dgrad', tune, 24575, 0), ('dgrad', tune, 24576, 0)])
    assert [g[:2] for g in got[:6]] == [(1, 3), (2, 3), (1, 3), (2, 3), (1, 1), (2, 1)]          # (kernel: 1 = 64-tile split, 2 = 128-tile split; pieces)
    assert got[6:] == [(32,), (64,)]
    # one product at K = 32768 on 128 tiles: 4 tiles, 384 / 4 = 96 workgroups each, 32768 / 96 -> chunks of 352 rows, 94 of them
    assert got[1] == (2, 3, 0, 2, 2, 94, 352, 94)


def test_training_planner_header_is_plain_cpp_and_the_globals_are_gone():
    """cmdgen_train_plan.h takes no HIP header and no cmdgen_handle (train_plan_check.cpp compiles it with -x c++), and no launcher of the training step
    reads a precision or a tuning that some earlier call left in a global."""
    csrc = os.path.join(ROOT, 'cmdgen_amd', 'csrc')
    src = open(os.path.join(csrc, 'cmdgen_train_plan.h')).read()
    assert all(inc.startswith('<') and 'hip' not in inc for inc in re.findall(r'#include\s+(\S+)', src)) and 'cmdgen_handle' not in src
    assert 'struct TrainTune' in src and 'dbg' not in src
    for f in os.listdir(csrc):
        if f.endswith(('.hip', '.h')):
            text = open(os.path.join(csrc, f)).read()
            assert 'g_train_tune' not in text and 'g_bf16' not in text, f


def test_product_fails_loudly_without_gpu():
    if torch.cuda.is_available():
        pytest.skip('GPU present')
    ddpm = small_ddpm()
    with pytest.raises(hip_backend.CmdgenError):
        ddpm.dynamics(torch.zeros(3, 11), torch.zeros(5, 23), torch.zeros(1, 1), torch.zeros(3, dtype=torch.long),
                      torch.zeros(5, dtype=torch.long))
    with pytest.raises(hip_backend.CmdgenError):
        hip_backend.Handle(ModelConfig().as_dict(), 0)
    # and nothing in the product imports the oracle
    for dirpath, _, files in os.walk(os.path.join(ROOT, 'cmdgen_amd')):
        for f in files:
            if f.endswith('.py') and f != 'selftest.py':
                src = open(os.path.join(dirpath, f)).read()
                assert 'oracle' not in src.replace('the oracle', ''), f


def test_state_dict_names_match_reference_checkpoint():
    """97 tensors, same names/shapes as the reference's 'ddpm.' sub-tree."""
    cfg = ModelConfig()
    ddpm = small_ddpm(H=256, L=5)
    sd = make_state_dict(cfg, seed=0, prefix='')
    mine = ddpm.state_dict()
    assert set(mine) == set(sd) and len(mine) == 97
    for k, v in sd.items():
        assert tuple(mine[k].shape) == v.shape, k
    ddpm.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    n_params = sum(p.numel() for p in ddpm.parameters())
    assert n_params == 2987815


def test_step_table_is_bit_identical_to_reference_scalars():
    g = load_golden('g1_schedule.npz')
    ddpm = small_ddpm(T=500)
    assert np.array_equal(ddpm.gamma.gamma.numpy(), g['gamma_T500'])
    for K in (5, 50, 500):
        tab = ddpm.step_table(K)
        assert tab.shape == (K + 1, 4)
        assert np.array_equal(tab[:K], g[f'coef_T500_K{K}'])
        assert np.array_equal(tab[K, :3], g['final_T500'])
    sched = PredefinedNoiseSchedule('polynomial_2', 1000, 1e-5)
    t = torch.tensor([[0.0], [0.5004], [1.0]])
    assert np.array_equal(sched(t).numpy().ravel(), g['gamma_T1000'][[0, 500, 1000]])


def test_distribution_nodes_matches_reference():
    g = load_golden('g8_nodes.npz')
    dn = DistributionNodes(g['hist'])
    lp = dn.log_prob_n1_given_n2(torch.from_numpy(g['n1']), torch.from_numpy(g['n2'])).numpy()
    assert np.allclose(lp, g['logp'], rtol=1e-6, atol=1e-7)
    torch.manual_seed(0)
    s = dn.sample_conditional(n1=None, n2=torch.tensor([44, 44, 30, 60]))
    assert s.shape == (4,) and bool(((s >= 3) & (s <= 25)).all())      # support of the histogram
    with pytest.raises(AssertionError):
        dn.sample_conditional(n1=None, n2=None)


def test_mask_helpers():
    m = utils.num_nodes_to_batch_mask(3, torch.tensor([2, 0, 3]), 'cpu')
    assert m.tolist() == [0, 0, 2, 2, 2]
    parts = utils.batch_to_list(torch.arange(5), m)
    assert [p.tolist() for p in parts] == [[0, 1], [2, 3, 4]]
    assert utils.sizes_from_mask(m, 3).tolist() == [2, 0, 3]
    with pytest.raises(ValueError):
        utils.sizes_from_mask(torch.tensor([1, 0]), 2)
    q = utils.Queue(max_len=3)
    for v in (1, 2, 3, 4):
        q.add(v)
    assert len(q) == 3 and q.mean() == 3.0


PDB = """\
ATOM      1  N   ALA A   1      11.104   6.134  -6.504  1.00  0.00           N
ATOM      2  CA  ALA A   1      11.639   6.071  -5.147  1.00  0.00           C
ATOM      3  C   ALA A   1      10.500   6.000  -4.100  1.00  0.00           C
ATOM      4  CA  GLY A   2      14.000   7.500  -3.000  1.00  0.00           C
ATOM      5  CA  TRP A   3      16.500   9.000  -1.000  1.00  0.00           C
ATOM      6  H   TRP A   3      16.900   9.100  -1.100  1.00  0.00           H
HETATM    7  C1  LIG A 101      13.000   7.000  -4.000  1.00  0.00           C
HETATM    8  O   HOH A 201      30.000  30.000  30.000  1.00  0.00           O
END
"""


def test_pdb_reader_and_pocket_selection(tmp_path):
    f = tmp_path / 'p.pdb'
    f.write_text(PDB)
    m = utils.parse_pdb(str(f))
    assert [r.get_resname() for r in m['A'].get_residues()] == ['ALA', 'GLY', 'TRP', 'LIG', 'HOH']
    res = m['A'][(' ', 2, ' ')]
    assert np.allclose(res['CA'].get_coord(), [14.0, 7.5, -3.0])
    assert utils.three_to_one('TRP') == 'W'
    near = utils.get_pocket_from_ligand(m, 'A:101')
    assert [r.get_resname() for r in near] == ['ALA', 'GLY', 'TRP']     # standard amino acids within 8 A


def test_checkpoint_round_trip_lightning_format(tmp_path):
    model = PharPocketDDPM(**_hparams())
    assert all(k.startswith('ddpm.') for k in model.state_dict())
    ck = tmp_path / 'best.ckpt'
    model.save_checkpoint(str(ck))
    again = PharPocketDDPM.load_from_checkpoint(str(ck), map_location='cpu')
    for k, v in model.state_dict().items():
        assert torch.equal(v, again.state_dict()[k])
    assert again.T == 500 and again.phar_nf == 8 and again.aa_nf == 20
    # mode 'joint' builds the base diffusion class over dynamics that also move the pocket (lightning_modules.py:110-139)
    jm = PharPocketDDPM(**{**_hparams(), 'mode': 'joint'})
    assert type(jm.ddpm).__name__ == 'EnVariationalDiffusion' and jm.ddpm.dynamics.update_pocket_coords
    assert set(jm.state_dict()) == set(model.state_dict())
    assert jm.ddpm.get_repaint_schedule(2, 2, 6) == [4, 4, 2]            # en_diffusion.py:649-670 (G9 schedule/r2_j2_T6)


def test_generate_phars_bookkeeping_with_stub_sampler(tmp_path, monkeypatch):
    """Post-parse behaviour of generate_phars (lightning_modules.py:439-541): pocket tensors repeated
    n_samples x, COM restore, and the 'Molecule_k' grouping quirk (Q9) - the sampler itself is stubbed
    here (it needs the GPU; covered by tests/test_hip_parity.py)."""
    f = tmp_path / 'p.pdb'
    f.write_text(PDB)
    model = PharPocketDDPM(**_hparams())
    seen = {}

    def fake_sample(pocket, num_nodes_phar, timesteps=None, **kw):
        seen['pocket'] = {k: v.clone() for k, v in pocket.items()}
        n = len(pocket['size'])
        pm = utils.num_nodes_to_batch_mask(n, num_nodes_phar, 'cpu')
        x = torch.arange(len(pm) * 3, dtype=torch.float32).view(-1, 3)
        types = torch.tensor([0, 4, 4, 1, 4, 0][:len(pm)])
        xh = torch.cat([x, torch.nn.functional.one_hot(types, 8).float()], 1)
        shift = torch.tensor([1.0, -2.0, 3.0])
        xp = torch.cat([pocket['x'] + shift, pocket['one_hot'].float()], 1)     # sampler translated the pocket
        xh[:, :3] += shift
        return xh, xp, pm, pocket['mask']
    monkeypatch.setattr(model.ddpm, 'sample_given_pocket', fake_sample)
    out = model.generate_phars(str(f), 2, pocket_ids=['A:1', 'A:2', 'A:3'], num_nodes_phar=torch.tensor([3, 3]))
    p = seen['pocket']
    assert p['x'].shape == (6, 3) and p['size'].tolist() == [3, 3] and p['mask'].tolist() == [0, 0, 0, 1, 1, 1]
    assert p['one_hot'].argmax(1).tolist() == [dataset_params['crossdock']['aa_encoder'][a] for a in 'AGW'] * 2
    assert sorted(out) == ['Molecule_1', 'Molecule_2', 'Molecule_3']           # k-th point of ALL samples
    assert sorted(out['Molecule_1']) == ['Aromatic', 'Hydrophobe']
    assert len(out['Molecule_2']['Acceptor']) == 2
    # the sampler's translation is undone: first point of sample 0 is back at (0,1,2)
    assert torch.allclose(out['Molecule_1']['Aromatic'][0], torch.tensor([0.0, 1.0, 2.0]), atol=1e-5)
    json.dumps({m: {t: [c.tolist() for c in cs] for t, cs in d.items()} for m, d in out.items()})


def test_generate_phars_cli_flags():
    from cmdgen_amd.generate_phars import build_parser
    a = build_parser().parse_args(['ckpt', '--pdbfile', 'x.pdb', '--resi_list', 'A:1', 'A:2', '--timesteps', '50'])
    assert a.n_samples == 20 and a.num_nodes_phar == 3 and a.resamplings == 10 and a.jump_length == 1
    assert a.resi_list == ['A:1', 'A:2'] and a.timesteps == 50 and not a.sanitize and not a.relax


def test_linear_specs_cover_all_weights():
    """2 987 314 trainable parameters + the frozen 501-entry gamma table."""
    n = sum(o * i + (o if b else 0) for o, i, b in linear_specs(ModelConfig()).values())
    assert n == 2987314 and n + 501 == 2987815


def test_dataset_npz_schema_centering_and_collate(tmp_path):
    """dataset.py:7-64: split by mask, per-complex joint centring, collate to a flat batch with float masks (Q13)."""
    from cmdgen_amd.dataset import ProcessedLigandPharPocketDataset, write_synthetic_npz
    f = tmp_path / 'val.npz'
    pb = write_synthetic_npz(str(f), n_complexes=5, seed=2)
    ds = ProcessedLigandPharPocketDataset(str(f))
    assert len(ds) == 5 and ds.data['num_pocket_nodes'].tolist() == pb.size.tolist()
    for i in range(5):
        it = ds[i]
        allx = torch.cat([it['phar_coords'], it['pocket_c_alpha']])
        assert float(allx.mean(0).abs().max()) < 1e-4                      # centred on the joint COG
        assert it['phar_one_hot'].shape[1] == 8 and it['pocket_one_hot'].shape[1] == 20
    batch = ds.collate_fn([ds[3], ds[1]])
    assert batch['names'] == ['complex_3', 'complex_1']
    assert batch['phar_mask'].dtype == torch.float32 and batch['phar_mask'].unique().tolist() == [0.0, 1.0]
    assert batch['num_pocket_nodes'].tolist() == [int(pb.size[3]), int(pb.size[1])]
    assert len(batch['pocket_c_alpha']) == int(pb.size[3] + pb.size[1])
    raw = ProcessedLigandPharPocketDataset(str(f), center=False)
    assert float(torch.cat([raw[0]['phar_coords'], raw[0]['pocket_c_alpha']]).mean(0).abs().max()) > 1.0


def test_consensus_posp_matches_reference_script(tmp_path):
    """get_phar/GMM_json.py (run unmodified by tests/golden/make_golden_posp.py) vs cmdgen_amd.get_phar: same
    GMM (scikit-learn, random_state=42), same typing rule, same .posp text; the lines parse the way
    GCPG/utils/file_utils.py:67-102 splits them."""
    import json
    from cmdgen_amd import get_phar
    cases = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'g10_posp.json')))['cases']
    assert len(cases) == 3
    for c in cases:
        clusters = get_phar.gmm_consensus(c['input'])
        text = ''.join(line + '\n' for line in get_phar.posp_lines(clusters))
        assert text == c['posp']
        for line in text.strip().split('\n'):
            types, x, y, z = line.strip().split(' ')
            assert types in get_phar.IDX2PHAR.values() and all(np.isfinite(float(v)) for v in (x, y, z))
    assert any(len(c['posp'].splitlines()) < 7 for c in cases)          # a 'NegIonizable' cluster is dropped (quirk kept)
    src = tmp_path / 'in.json'
    src.write_text(json.dumps(cases[0]['input']))
    lines = get_phar.main([str(src), '--out', str(tmp_path / 'o.posp')])
    assert (tmp_path / 'o.posp').read_text() == cases[0]['posp'] and len(lines) == len(cases[0]['posp'].splitlines())


def test_per_sample_table_matches_the_tensor_op_scalars():
    """training.per_sample_table (numpy on the host: the `tab` argument of cmdgen_train_noise / cmdgen_train_loss) against the
    same per-sample scalars formed with ConditionalDDPM's own tensor operations, t = 0 and t = T included."""
    from cmdgen_amd.training import per_sample_table
    model = PharPocketDDPM(**_hparams())
    ddpm = model.ddpm
    B = 7
    t_int = torch.tensor([0., 1., 2., 17., 250., 499., 500.][:B]).reshape(B, 1)
    n_phar, n_pocket = torch.tensor([3, 5, 8, 12, 15, 20, 9]), torch.tensor([30, 44, 51, 38, 60, 47, 33])
    tab = per_sample_table(ddpm.gamma.gamma.detach().numpy(), ddpm.size_distribution._table(1, torch.device('cpu')).numpy(), ddpm.T,
                           ddpm.n_dims, ddpm.norm_values, t_int, n_phar.numpy(), n_pocket.numpy())
    assert tuple(tab.shape) == (12, B) and tab.dtype == torch.float32
    x = torch.zeros(B, 3)
    s, t = (t_int - 1) / ddpm.T, t_int / ddpm.T
    gamma_s, gamma_t = ddpm.inflate_batch_array(ddpm.gamma(s), x), ddpm.inflate_batch_array(ddpm.gamma(t), x)
    ones = torch.ones((B, 1))
    want = [ddpm.alpha(gamma_t, x).reshape(-1), ddpm.sigma(gamma_t, x).reshape(-1), (t_int == 0).float().reshape(-1),
            (1 - ddpm.SNR(gamma_s - gamma_t)).reshape(-1), ddpm.alpha(ddpm.gamma(ones), x).reshape(-1), ddpm.sigma(ddpm.gamma(ones), x).reshape(-1),
            -ddpm.log_constants_p_x_given_z0(n_nodes=n_phar, device='cpu'), ddpm.delta_log_px(n_phar).float(), ddpm.log_pN(n_phar, n_pocket),
            t_int.reshape(-1), t.reshape(-1), ddpm.sigma(gamma_t, x).reshape(-1) * ddpm.norm_values[1]]
    for i, w in enumerate(want):
        w = torch.as_tensor(w, dtype=torch.float32).reshape(-1)
        assert torch.allclose(tab[i], w, rtol=2e-6, atol=1e-7), (i, tab[i], w)


def test_gamma_network_host_copy_leaves_the_global_rng_alone():
    """GammaNetwork.cpu_copy() constructs a fresh network (PositiveLinear.__init__ draws from the global generator): it must not advance the
    caller's stream - the reference's sampler does not touch it, so host-side randn after a sampling call stays reproducible against it."""
    from cmdgen_amd.equivariant_diffusion.en_diffusion import GammaNetwork
    g = GammaNetwork()
    torch.manual_seed(123)
    want = torch.rand(4)
    torch.manual_seed(123)
    g.cpu_copy(); g.table(50)
    assert torch.equal(torch.rand(4), want)


def test_joint_sampler_refuses_a_learned_schedule_off_the_T_grid():
    """mode 'joint' + noise_schedule='learned': the joint chain's op table reads gamma from the network's tabulation on the T-grid, which
    equals the reference's gamma(step / K) only when K divides T - any other K is refused before the handle is touched (no GPU needed)."""
    from cmdgen_amd.equivariant_diffusion.en_diffusion import EnVariationalDiffusion
    dyn = EGNNDynamics(phar_nf=8, residue_nf=20, n_dims=3, joint_nf=16, hidden_nf=64, n_layers=1, attention=True, tanh=True, norm_constant=1,
                       inv_sublayers=1, normalization_factor=100, aggregation_method='sum', edge_cutoff=6.0, update_pocket_coords=True)
    ddpm = EnVariationalDiffusion(dynamics=dyn, phar_nf=8, residue_nf=20, n_dims=3, timesteps=500, noise_schedule='learned', noise_precision=1e-5,
                                  loss_type='vlb', norm_values=[1, 4], size_histogram=np.ones((30, 70)))
    with pytest.raises(NotImplementedError, match='divide T'):
        ddpm._joint_handle(np.array([8]), np.array([40]), timesteps=7)
