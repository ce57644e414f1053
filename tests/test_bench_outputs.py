"""bench.py's plain line and ``--dump-outputs``: the plain run reports the headline alone (what else the benchmark measures runs with
``--full``), and the dump holds what the last timed step returned, the same from run to run with the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO

HEADLINE = ('metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step')
FULL_ONLY = ('host_io', 'roofline', 'f32_arm', 'cpu_baseline')


def test_dump_outputs_dtypes_and_budget(tmp_path, monkeypatch):
    import bench
    small = {'images': torch.arange(2 * 3 * 4, dtype=torch.uint8).view(2, 3, 4), 'cams': torch.ones(2, 7, dtype=torch.float64),
             'loss': 1.5, 'frames': [0, 2, 5], 'label': 'not an array'}
    bench.dump_outputs(str(tmp_path / 'a'), small)
    got = {f[:-4]: np.load(tmp_path / 'a' / f) for f in os.listdir(tmp_path / 'a')}
    assert sorted(got) == ['cams', 'frames', 'images', 'loss']
    assert got['images'].dtype == np.float32 and np.array_equal(got['images'], small['images'].numpy().astype(np.float32))
    assert got['cams'].dtype == np.float64 and got['cams'].shape == (2, 7)
    assert got['loss'].dtype == np.float64 and got['loss'].tolist() == [1.5]
    assert got['frames'].dtype == np.float32 and got['frames'].tolist() == [0, 2, 5]
    # over the budget: every array cut to the same fraction of its rows, the same rows in every call
    monkeypatch.setattr(bench, 'DUMP_BUDGET_BYTES', 4000)
    big = {'x': torch.arange(1000 * 2, dtype=torch.float32).view(1000, 2), 'y': torch.arange(1000, dtype=torch.float32)}
    bench.dump_outputs(str(tmp_path / 'b'), big)
    bench.dump_outputs(str(tmp_path / 'c'), big)
    x, y = np.load(tmp_path / 'b' / 'x.npy'), np.load(tmp_path / 'b' / 'y.npy')
    assert x.nbytes + y.nbytes <= 4000 and len(x) == len(y) == 333
    assert np.array_equal(x[:, 0] / 2, y) and np.all(np.diff(y) > 0)                 # sorted rows, the same ones in both arrays
    assert np.array_equal(x, np.load(tmp_path / 'c' / 'x.npy')) and np.array_equal(y, np.load(tmp_path / 'c' / 'y.npy'))


def _bench(extra, timeout=600):
    r = subprocess.run([sys.executable, os.path.join(REPO, 'bench.py'), '--gpus', '1'] + extra, cwd=REPO, capture_output=True, text=True,
                       timeout=timeout)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
@pytest.mark.timeout(1200, method='thread')
def test_plain_line_full_line_and_dumped_outputs(tmp_path):
    args = ['--steps', '3', '--warmup', '1', '--batch', '4']
    plain = _bench(args + ['--dump-outputs', str(tmp_path / 'plain')])
    assert all(k in plain for k in HEADLINE) and plain['steps'] == 3 and plain['ms_per_step'] > 0
    assert plain['unit'] == 'novel views/s' and plain['higher_is_better'] is True and plain['dtype'] == 'bf16'
    assert not [k for k in FULL_ONLY if k in plain], sorted(plain)
    full = _bench(args + ['--full', '--no-cpu-baseline', '--no-f32-arm', '--dump-outputs', str(tmp_path / 'full')])
    assert 'host_io' in full and full['roofline']['achieved'] > 0
    names = sorted(os.listdir(tmp_path / 'plain'))
    assert names == ['generated_cameras.npy', 'generated_images.npy', 'ground_truth_cameras.npy', 'ground_truth_images.npy']
    assert names == sorted(os.listdir(tmp_path / 'full'))
    for n in names:
        a, b = np.load(tmp_path / 'plain' / n), np.load(tmp_path / 'full' / n)
        assert a.dtype == np.float32 and a.shape[0] == 4 and np.array_equal(a, b), n     # same inputs, same bits, run to run
    img = np.load(tmp_path / 'plain' / 'generated_images.npy')
    assert img.shape == (4, 128, 128, 3) and img.min() >= 0 and img.max() <= 255 and img.std() > 0
