"""GPU, >= 2 devices: the driver's multi-GPU launch line on a real RCCL communicator (VERDICT r2 'next' #8).

``bench.py --gpus 2`` under ``torch.distributed.run`` exactly as the contract launches it — one process per GPU, backend "nccl"
(= RCCL on ROCm), HSA_ENABLE_IPC_MODE_LEGACY=0 — for the inference workload (scene shards, no data-path collective: only the barrier
and the max-over-ranks time touch the communicator) and for the training step (per-layer gradient all-reduce SUM over xGMI,
viewformer/train/utils.py:145-153, models/migt.py:471-476,488).  Skipped on the 1-GPU boxes gpurun provides; the world-2 logic itself
is covered there by tests/test_hip_multirank.py and tests/test_hip_train_full.py (gloo transport on device tensors) and on CPU by
tests/test_sharding.py."""
import json
import os
import socket
import subprocess
import sys

import pytest
import torch

from conftest import REPO

pytestmark = pytest.mark.gpu
two_gpus = pytest.mark.skipif(not torch.cuda.is_available() or torch.cuda.device_count() < 2, reason='needs >= 2 GPUs (RCCL path)')


def _port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _launch(extra, n=2, timeout=420, backend=None):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY='0')
    if backend:
        env['VF_DIST_BACKEND'] = backend
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', f'--nproc-per-node={n}', '--master-addr', '127.0.0.1',
           '--master-port', str(_port()), os.path.join(REPO, 'bench.py'), '--gpus', str(n)] + extra
    r = subprocess.run(cmd, cwd=REPO, env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, r.stdout[-2000:]                 # rank 0 prints ONE JSON line
    return json.loads(lines[0])


@two_gpus
@pytest.mark.timeout(1500, method='thread')          # (launches of up to 420 s each: above conftest's 600 s default for GPU tests)
def test_views_workload_two_gpus_scene_shards():
    one = _launch(['--steps', '2', '--warmup', '1', '--batch', '16', '--no-cpu-baseline', '--no-f32-arm'], n=1)
    two = _launch(['--steps', '2', '--warmup', '1', '--batch', '16', '--no-cpu-baseline', '--no-f32-arm'], n=2)
    assert two['n_gpus'] == 2 and two['scaling'] == 'weak' and two['value'] > 0
    assert two['value'] > 1.5 * one['value'], (one['value'], two['value'])      # independent shards: close to 2x


@two_gpus
@pytest.mark.timeout(1500, method='thread')          # (launches of up to 420 s each: above conftest's 600 s default for GPU tests)
def test_train_workload_two_gpus_rccl_allreduce():
    line = _launch(['--workload', 'train', '--steps', '3', '--warmup', '1', '--full'], n=2)
    assert line['n_gpus'] == 2 and line['value'] > 0
    c = line['config']['collective']
    assert c['backend'] == 'nccl'                                               # RCCL
    assert c['ms_per_step_without_allreduce'] > 0 and c['exposed_allreduce_wait_ms'] >= 0
    half = _launch(['--workload', 'train', '--steps', '3', '--warmup', '1', '--grad-dtype', 'bf16', '--full'], n=2)
    assert half['config']['collective']['gradient_dtype_on_the_links'] == 'bf16' and half['value'] > 0


@pytest.mark.timeout(1500, method='thread')          # (launches of up to 420 s each: above conftest's 600 s default for GPU tests)
def test_two_rank_launch_line_on_one_gpu_over_gloo():
    """the same launch line with two ranks on whatever GPUs the box has (VF_DIST_BACKEND=gloo: ranks share cuda:0 on a 1-GPU box and the
    collectives carry device tensors over gloo): bench.py's N > 1 branches — scene shards summed over ranks, max-over-ranks time, one JSON
    line from rank 0, the training line's collective block (step without the all-reduce, exposed wait) — run end to end.  Not a
    performance statement: two ranks on one GPU halve each other's throughput."""
    views = _launch(['--steps', '2', '--warmup', '1', '--batch', '8', '--no-cpu-baseline', '--no-f32-arm'], n=2, backend='gloo')
    assert views['n_gpus'] == 2 and views['scaling'] == 'weak' and views['value'] > 0
    assert 'x2' in views['config']['parallelism']
    train = _launch(['--workload', 'train', '--steps', '2', '--warmup', '1', '--batch', '2', '--full'], n=2, backend='gloo')
    assert train['n_gpus'] == 2 and train['value'] > 0
    c = train['config']['collective']
    assert c['backend'] == 'gloo' and c['ms_per_step_without_allreduce'] > 0 and c['exposed_allreduce_wait_ms'] >= 0
    assert c['gradient_dtype_on_the_links'] == 'f32'
    half = _launch(['--workload', 'train', '--steps', '2', '--warmup', '1', '--batch', '2', '--grad-dtype', 'bf16', '--full'], n=2, backend='gloo')
    assert half['config']['collective']['gradient_dtype_on_the_links'] == 'bf16' and half['value'] > 0


def _bare(extra, n, backend=None, timeout=420):
    """the DRIVER's command form: ``python bench.py --gpus N ...`` with no launcher and no WORLD_SIZE / RANK in the environment"""
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT', 'VF_DIST_BACKEND')}
    if backend:
        env['VF_DIST_BACKEND'] = backend
    return subprocess.run([sys.executable, os.path.join(REPO, 'bench.py'), '--gpus', str(n)] + extra, cwd=REPO, env=env, capture_output=True,
                          text=True, timeout=timeout)


@pytest.mark.timeout(1500, method='thread')
def test_bare_command_starts_its_own_ranks():
    """``python bench.py --gpus 2`` (no torch.distributed.run around it) used to run one process and print n_gpus 1.
    Now the bare command starts the two ranks itself: n_gpus == 2, config.ranks == 2, the transport it really used is in the line —
    for the inference line and for the training line (whose collective block needs a real process group)."""
    r = _bare(['--steps', '2', '--warmup', '1', '--batch', '8', '--no-cpu-baseline', '--no-f32-arm'], n=2, backend='gloo')
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, r.stdout[-2000:]
    line = json.loads(lines[0])
    assert line['n_gpus'] == 2 and line['config']['ranks'] == 2 and line['config']['backend'] == 'gloo'
    assert line['config']['scenes_per_gpu_per_step'] == 8 and 'x2' in line['config']['parallelism'] and line['value'] > 0
    r = _bare(['--workload', 'train', '--steps', '2', '--warmup', '1', '--batch', '2', '--full'], n=2, backend='gloo')
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith('{')][0])
    assert line['n_gpus'] == 2 and line['config']['ranks'] == 2 and line['config']['communicator_world_size'] == 2
    assert line['config']['collective']['backend'] == 'gloo'
    r = _bare(['--workload', 'allimg', '--steps', '1', '--warmup', '0', '--batch', '16'], n=2, backend='gloo')
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith('{')][0])
    assert line['n_gpus'] == 2 and line['config']['ranks'] == 2


@pytest.mark.skipif(torch.cuda.is_available() and torch.cuda.device_count() >= 2, reason='box has >= 2 GPUs: the bare command may run')
def test_bare_command_refuses_more_ranks_than_gpus():
    """on a 1-GPU box, without the gloo plumbing switch, ``--gpus 2`` must fail loudly — not measure one GPU and call it two"""
    for wl in ([], ['--workload', 'train'], ['--workload', 'allimg']):
        r = _bare(wl + ['--steps', '1', '--warmup', '0'], n=2, timeout=300)
        assert r.returncode != 0, wl
        assert 'refusing' in r.stderr and not [l for l in r.stdout.splitlines() if l.startswith('{')], r.stderr[-500:]


RCCL_ONE = r'''
import os, sys, torch, torch.distributed as dist
sys.path.insert(0, sys.argv[1])
os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
torch.cuda.set_device(0)
dist.init_process_group('nccl', init_method=f'tcp://127.0.0.1:{sys.argv[2]}', rank=0, world_size=1)
assert dist.get_backend() == 'nccl'
from viewformer_amd import sharding
dev = torch.device('cuda:0')
flat = torch.randn(3_000_001, device=dev)
ref = flat.clone()
assert sharding.allreduce_sum_ranges(flat, [(0, 1000)], None) == []        # (the product skips the collective when there is one rank)
hs = [dist.all_reduce(flat[a:b], op=dist.ReduceOp.SUM, async_op=True)      # ... so issue its calls directly: the trainer's per-layer ranges
      for a, b in [(0, 1000), (1000, 2_000_000), (2_000_000, 3_000_001)]]
side = torch.cuda.Stream()
with torch.cuda.stream(side):                                   # kernels on another stream while the collectives are in flight
    x = torch.randn(2048, 2048, device=dev); y = x @ x
b16 = flat[:4096].to(torch.bfloat16)
h16 = dist.all_reduce(b16, op=dist.ReduceOp.SUM, async_op=True)  # the bf16-bucket form
for h in hs:
    h.wait()
h16.wait()
torch.cuda.synchronize()
assert torch.equal(flat, ref) and torch.equal(b16, ref[:4096].to(torch.bfloat16))      # a SUM over one rank
sharding.barrier()
assert sharding.max_over_ranks(1.25, dev) == 1.25
assert sharding.sum_over_ranks(3.0, dev) == 3.0
parts = sharding.gather_to_rank0(torch.arange(12, device=dev).view(4, 3))
assert len(parts) == 1 and parts[0].shape == (4, 3)
dist.destroy_process_group()
print('rccl-one ok', flush=True)
'''


def test_rccl_communicator_of_one_rank_runs_the_products_collectives():
    """No box here has two GPUs, so RCCL never sees N > 1 in this suite; what CAN be checked on one GPU is that the image's RCCL creates a
    communicator under the product's environment (HSA_ENABLE_IPC_MODE_LEGACY=0, device bound before init) and executes the collectives the
    product issues — per-range async SUM all-reduces of the flat gradient buffer (fp32 and bf16 buckets) beside kernels on another stream,
    barrier, max-over-ranks — with the arithmetic of a one-rank sum.  (The 2-rank launch tests above run wherever >= 2 GPUs exist.)"""
    r = subprocess.run([sys.executable, '-c', RCCL_ONE, REPO, str(_port())], cwd=REPO, capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY='0'))
    assert r.returncode == 0 and 'rccl-one ok' in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])


def _preflight_line(text):
    lines = [l for l in text.splitlines() if l.startswith('{') and '"preflight"' in l]
    assert len(lines) == 1, text[-2000:]
    return json.loads(lines[0])


@pytest.mark.timeout(900, method='thread')
def test_preflight_world1_rccl_and_world2_gloo():
    """``bench.py --gpus N --preflight`` — device binding, communicator, 28 MB all-reduces timed, per-rank HBM headroom for one
    encoder chunk — so that the first run on a multi-GPU node is not also the first debug session.  On a 1-GPU box: world 1 over RCCL (the
    communicator is created although one rank needs none) and world 2 over gloo (ranks share cuda:0); and the bare ``--gpus 2`` run prints
    the same line on stderr BEFORE its timed run."""
    r = _bare(['--preflight'], n=1)
    assert r.returncode == 0, r.stderr[-3000:]
    pf = _preflight_line(r.stdout)
    assert pf['preflight'] == 'ok' and pf['ranks'] == 1 and pf['backend'] == 'nccl' and pf['allreduce']['sum_exact']
    assert pf['allreduce']['bytes'] == (12 * 768 * 768 + 13 * 768) * 4 and pf['allreduce']['iters'] == 100 and pf['allreduce']['ms_max_over_ranks'] > 0
    assert pf['encoder_chunk']['images'] == 896 and pf['per_rank'][0]['hbm_headroom_gb_after_encoder_chunk'] > 0
    r = _bare(['--preflight'], n=2, backend='gloo')
    assert r.returncode == 0, r.stderr[-3000:]
    pf = _preflight_line(r.stdout)
    assert pf['preflight'] == 'ok' and pf['ranks'] == 2 and pf['backend'] == 'gloo' and pf['allreduce']['sum_exact']
    assert pf['allreduce']['busbw_gbs'] > 0 and len(pf['per_rank']) == 2 and {p['rank'] for p in pf['per_rank']} == {0, 1}
    assert pf['shared_device'] == (torch.cuda.device_count() < 2)
    r = _bare(['--steps', '1', '--warmup', '0', '--batch', '4', '--no-cpu-baseline', '--no-f32-arm'], n=2, backend='gloo')
    assert r.returncode == 0, r.stderr[-3000:]
    assert _preflight_line(r.stderr)['ranks'] == 2                       # before the timed run, on stderr: stdout stays ONE JSON line
    lines = [l for l in r.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1 and json.loads(lines[0])['shared_device'] == (torch.cuda.device_count() < 2)
