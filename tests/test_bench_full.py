"""bench.py's two lines on the GPU: a plain run reports the headline from the timed steps alone and does no work after them;
--full adds every record that takes runs of its own (roofline and kernel breakdown, steady state, the other shapes, training
step, CPU baseline).  Small chains (8 pockets, T = 40) so that the whole --full line stays short."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ['--gpus', '1', '--batch', '8', '--timesteps', '40', '--steps', '1', '--warmup', '1']
FULL_ONLY_CONFIG = ('kernel_ms_one_evaluation', 'steady_state_evaluation', 'north_star_trained', 'fullatom_trained', 'drifted_shipped_schedule_chain',
                    'fp32_instruction_engine', 'training_step', 'driver_shapes', 'gpu_over_cpu')


def _bench(extra):
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT')}
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py')] + SMALL + extra, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def _headline(d):
    assert d['metric'] == 'denoising steps/sec' and d['unit'] == 'pocket-steps/s' and d['higher_is_better'] is True and d['dtype'] == 'f32'
    assert d['value'] > 0 and d['ms_per_step'] > 0 and d['n_gpus'] == 1
    c = d['config']
    assert c['pockets_per_gpu'] == 8 and c['timesteps'] == 40 and c['chain_status']['nan_resets'] == 0
    assert set(c['launch']) >= {'node_mt', 'edge_mt', 'coord_mt', 'gemm_split', 'half_engine'}


def test_plain_run_reports_the_headline_alone():
    d = _bench([])
    _headline(d)
    assert 'roofline' not in d and d['cpu_baseline'] is None
    assert not set(d['config']) & set(FULL_ONLY_CONFIG)


def test_full_run_adds_every_other_record():
    d = _bench(['--full', '--cpu-seconds', '1'])
    _headline(d)
    c = d['config']
    assert set(c) >= set(FULL_ONLY_CONFIG), sorted(set(FULL_ONLY_CONFIG) - set(c))
    r = d['roofline']
    assert r['achieved'] > 0 and 0 < r['frac'] <= 1 and set(r['per_kernel']) >= {'edge_msg', 'node', 'edge_coord'}
    assert c['steady_state_evaluation']['us_per_evaluation'] > 0
    assert c['north_star_trained']['pockets'] == 256 and c['north_star_trained']['roofline']['achieved'] > 0
    assert c['fullatom_trained']['pockets'] == 256 and c['training_step']['fp32_results']['ms_per_step'] > 0
    assert set(c['driver_shapes']) == {'driver_shape', 'driver_shape_t50', 'single_pocket'}
    assert d['cpu_baseline']['value'] > 0 and c['gpu_over_cpu'] > 0
