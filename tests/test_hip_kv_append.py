"""GPU: ``vf_kv_append`` (csrc/kv_append.hip) — the keys and values of new views go to each scene's own position in a
context cache with room, bit for bit, and nothing else of the cache changes.  The destination is a framed tensor (tests/framed.py) loaded
with values of its own: after the launch its logical window equals an expectation built with torch indexing — which covers the Q
thirds, every other row and every other scene — and no guard, row-gap or batch-gap byte has changed; the source frame keeps its bits."""
import numpy as np
import pytest
import torch

from framed import BACK, BATCH_GAP, FRONT, ROW_GAP, Frame

pytestmark = pytest.mark.gpu

L = 64
# (B, K, d, capacity, pos): one view into a two-view cache; a ragged batch (64-thread blocks); the model's width (256-thread blocks)
CASES = [(1, 1, 64, 2, [1]), (3, 2, 192, 7, [0, 5, 2]), (2, 3, 768, 4, [1, 1])]


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'needs the MI355X'
    return torch.device('cuda:0')


def _rand(shape, seed):
    g = np.random.Generator(np.random.PCG64(seed))
    return torch.from_numpy(g.standard_normal(shape).astype(np.float32))


def _run(dev, dt, B, K, d, capacity, pos, seed=0):
    """launch on framed tensors with ld_src, ld_dst > 3 d and a gap between the scenes -> (status is checked by ops; got, want)"""
    from viewformer_amd import ops
    ld_src, ld_dst = 3 * d + 16, 3 * d + 24
    stride = capacity * L * ld_dst + 64
    src = _rand((B * K * L, 3 * d), 300 + seed).to(dt)
    old = _rand((B, capacity * L, 3 * d), 400 + seed).to(dt)
    fs = Frame(B * K * L, 3 * d, ld_src, dt, dev).load(src)
    fd = Frame(capacity * L, 3 * d, ld_dst, dt, dev, batch=B, batch_stride=stride).load(old if B > 1 else old[0], accumulate=True)
    fp = Frame.raw(B * 4, dev, dtype=torch.int32).load(torch.tensor(pos, dtype=torch.int32))
    ops.kv_append(fs.view, fd.view, B, K, L, d, ld_src, ld_dst, stride, capacity, fp.view)
    torch.cuda.synchronize()
    want = old.clone()
    s = src.view(B, K, L, 3 * d)
    for b in range(B):
        for j in range(K):
            v = pos[b] + j
            if 0 <= v < capacity:
                want[b, v * L:(v + 1) * L, :d] = s[b, j, :, :d]                       # the V third
                want[b, v * L:(v + 1) * L, 2 * d:] = s[b, j, :, 2 * d:]               # the K third; the Q third stays
    assert fs.violations() == [] and fp.violations() == []                       # inputs unchanged, nothing written around them
    for region in (FRONT, BACK, ROW_GAP, BATCH_GAP):
        assert fd.offsets(region).numel() == 0, region                           # no guard or gap byte has changed
    idt = torch.int16 if dt == torch.bfloat16 else torch.int32
    got = fd.logical().view(B, capacity * L, 3 * d).cpu()
    return got.view(idt), want.view(idt), old.view(idt)


@pytest.mark.parametrize('dt', [torch.bfloat16, torch.float32], ids=['bf16', 'f32'])
@pytest.mark.parametrize('case', CASES, ids=lambda c: 'B{}K{}d{}cap{}'.format(*c[:4]))
def test_new_views_land_at_each_scenes_position_and_nothing_else_changes(dev, dt, case):
    B, K, d, capacity, pos = case
    got, want, old = _run(dev, dt, B, K, d, capacity, pos)
    assert not torch.equal(want, old)
    assert torch.equal(got, want)


@pytest.mark.parametrize('dt', [torch.bfloat16, torch.float32], ids=['bf16', 'f32'])
def test_a_view_beyond_the_capacity_is_not_written(dev, dt):
    """scene 1: pos + K > capacity (views 2, 3 and 4 of a 4-view cache): views 2 and 3 are written, view 4 is dropped, nothing else is
    touched and the call returns VF_OK (``ops.kv_append`` raises on any other status)"""
    got, want, old = _run(dev, dt, 2, 3, 192, 4, [1, 2], seed=1)
    assert torch.equal(got, want)
    assert not torch.equal(got[1, 3 * L:], old[1, 3 * L:]) and torch.equal(got[0, :L], old[0, :L])


def test_a_launch_larger_than_the_grid_walks_all_of_it(dev):
    """fp32, 88 views of d = 768: 24 576 16-byte chunks per view, which 96 blocks of 256 threads would cover; the grid is capped at
    8192 // 88 = 93 slices per view, so threads take a second chunk (the stride loop)"""
    got, want, old = _run(dev, torch.float32, 4, 22, 768, 24, [0, 2, 1, 2], seed=2)
    assert torch.equal(got, want)
