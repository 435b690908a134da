"""The driver depends on bench.py's CLI + JSON contract; pin it."""

import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_json_contract():
    r = subprocess.run(
        [sys.executable, 'bench.py', '--steps', '1', '--warmup', '0',
         '--batch', '1'],
        capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = r.stdout.strip().splitlines()[-1]
    d = json.loads(line)
    for key in ('metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup',
                'ms_per_step', 'higher_is_better', 'scaling',
                'vs_baseline', 'dtype', 'data', 'config'):
        assert key in d, key
    assert d['metric'] == 'training images/sec'
    assert d['higher_is_better'] is True
    assert d['scaling'] == 'weak'
    assert d['data'] == 'synthetic'
    assert d['value'] > 0
    assert {'model', 'global_batch', 'seq_len',
            'parallelism'} <= set(d['config'])


def test_bench_dump_outputs_and_full(tmp_path):
    """--dump-outputs writes the last timed step's outputs as float .npy
    files (64 MB at most); --full is accepted and keeps the result line."""
    import numpy as np
    out_dir = tmp_path / 'dump'
    r = subprocess.run(
        [sys.executable, 'bench.py', '--gpus', '1', '--steps', '2',
         '--warmup', '0', '--batch', '1', '--full',
         '--dump-outputs', str(out_dir)],
        capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads(r.stdout.strip().splitlines()[-1])
    assert d['metric'] == 'training images/sec'
    assert d['steps'] == 2
    assert d['ms_per_step'] > 0
    assert abs(d['value'] - 1000.0 / d['ms_per_step']) \
        <= 0.01 * d['value']  # batch 1: images/sec == steps/sec
    files = sorted(os.listdir(out_dir))
    assert {'total_loss.npy', 'accuracy.npy', 'attentions.npy',
            'params_sample.npy'} <= set(files)
    total = 0
    for f in files:
        a = np.load(out_dir / f)
        assert a.dtype in (np.float32, np.float64), f
        assert np.isfinite(a).all(), f
        total += a.nbytes
    assert total <= 64 * 2 ** 20
    assert np.load(out_dir / 'attentions.npy').shape == (1, 196)
    assert float(np.load(out_dir / 'total_loss.npy').reshape(-1)[0]) > 0


def test_graft_entry_has_build_and_smoke():
    import importlib.util
    spec = importlib.util.spec_from_file_location(
        'graft_entry', os.path.join(ROOT, '__graft_entry__.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert callable(mod.build) and callable(mod.smoke)
