"""CPU: the host side of the novel-view renderer (viewformer_amd/render.py, csrc/attention_prefix.hip) — the prefix-attention entry
points validate their arguments before any launch, the renderer's pose bookkeeping equals the evaluator's bit for bit, and the chunk
planner walks N in whole views.  No device is touched."""
import ctypes

import numpy as np
import pytest
import torch


@pytest.fixture(scope='module')
def lib():
    from viewformer_amd import build, _lib
    build.build()                      # hipcc cross-compiles gfx950 without a GPU
    return _lib.load()


def _call(lib, arm, q=4096, k=4096, v=4096, kp=4096, vp=4096, out=4096, B=2, H=12, C=6, N=8, L=64, dh=64, ldq=2304, ldk=2304, ldv=2304,
          ldkp=2304, ldvp=2304, stride=6 * 64 * 2304, ldo=768):
    P = ctypes.c_void_p
    ptr = lambda x: None if x is None else P(x)          # never dereferenced: validation happens before any launch
    if arm == 'bf16':
        return lib.vf_attn_prefix_bf16(ptr(q), ptr(k), ptr(v), ptr(kp), ptr(vp), 1, ptr(out), 1, B, H, C, N, L, dh, ldq, ldk, ldv, ldkp, ldvp,
                                       stride, ldo, None)
    return lib.vf_attn_prefix_f32eq(ptr(q), ptr(k), ptr(v), ptr(kp), ptr(vp), ptr(out), B, H, C, N, L, dh, ldq, ldk, ldv, ldkp, ldvp,
                                    stride, ldo, None)


@pytest.mark.parametrize('arm', ['bf16', 'f32eq'])
def test_prefix_attention_validates_its_arguments_without_a_device(lib, arm):
    for name in ('q', 'k', 'v', 'kp', 'vp', 'out'):
        assert _call(lib, arm, **{name: None}) == -1, name                     # null pointers
    for name in ('ldq', 'ldk', 'ldv', 'ldkp', 'ldvp', 'ldo'):
        assert _call(lib, arm, **{name: 12 * 64 - 8}) == -1, name              # leading dimension below H * 64
    assert _call(lib, arm, ldk=2306) == -1                                     # rows are read as vectors: misaligned
    assert _call(lib, arm, L=16) == -2 and _call(lib, arm, L=128) == -2        # 64-token views only
    assert _call(lib, arm, dh=32) == -2 and _call(lib, arm, dh=128) == -2      # head dimension 64 only
    assert _call(lib, arm, C=0) == -2                                          # a prefix has at least one view
    assert _call(lib, arm, N=-1) == -1 and _call(lib, arm, B=-1) == -1 and _call(lib, arm, H=0) == -1
    assert _call(lib, arm, N=0) == 0 and _call(lib, arm, B=0) == 0             # nothing to do: no launch
    assert _call(lib, arm, N=0, L=32) == -2                                    # ... but an unsupported shape is still refused


def test_ops_attn_prefix_refuses_cpu_tensors(lib):
    from viewformer_amd import ops, _lib
    z = torch.zeros(64, 192)
    for bf16 in (False, True):
        with pytest.raises(_lib.VfError):
            ops.attn_prefix(z[:, 64:128], z[:, 128:], z[:, :64], z[:, 128:], z[:, :64], torch.zeros(64, 64), 1, 1, 1, 1, 64,
                            192, 192, 192, 192, 192, 64 * 192, 64, bf16=bf16)


def _cameras(B, V, seed):
    g = np.random.Generator(np.random.PCG64(seed))
    cam = g.standard_normal((B, V, 7)).astype(np.float32)
    cam[..., :3] *= 2.0
    return torch.from_numpy(cam)               # un-normalised quaternions of either sign: normalize_cameras has work to do


@pytest.mark.parametrize('augment', ['relative', 'no'])
def test_query_poses_equal_the_evaluators_per_call_bookkeeping(augment):
    """The renderer relativises every query with the context's view 0 once; the evaluator relativises the sequence (context..., query n)
    per call (evaluate_transformer.py:99-102).  Same cameras, bit for bit, for every n — and the context's poses are the first C."""
    from viewformer_amd import geometry
    from viewformer_amd.render import context_poses, query_poses
    B, C, N = 3, 6, 11
    ctx, q = _cameras(B, C, 1), _cameras(B, N, 2)
    cpos, transform = context_poses(ctx, augment)
    got = query_poses(q, transform)
    assert got.shape == (B, N, 7) and (transform is None) == (augment == 'no')
    for n in range(N):
        seq = torch.cat([ctx, q[:, n:n + 1]], 1)
        if augment == 'relative':
            seq = geometry.to_relative_cameras(seq)[0]
        seq = geometry.normalize_cameras(seq)
        assert torch.equal(got[:, n], seq[:, -1]), n
        assert torch.equal(cpos, seq[:, :-1])


def test_chunk_planner_walks_whole_views_exactly_once():
    from viewformer_amd.evaluate import MAX_SCENES_PER_CALL
    from viewformer_amd.render import default_views_per_call, plan_view_chunks
    assert plan_view_chunks(0) == [] and plan_view_chunks(0, 16, 4) == []
    for N in (1, 3, 4, 8, 120, 257, 1000):
        for B in (1, 2, 16, 300):
            for cap in (None, 1, 4, 7, 128, 5000):
                chunks = plan_view_chunks(N, B, cap)
                limit = cap if cap is not None else default_views_per_call(B)
                assert all(isinstance(a, int) and isinstance(b, int) and 0 <= a < b <= N for a, b in chunks)      # whole views
                assert all(b - a <= limit for a, b in chunks)                                                     # the cap
                assert [v for a, b in chunks for v in range(a, b)] == list(range(N))                              # each view once, in order
    # the default keeps a pass at the evaluator's own cap of view-rows over the batch (and never below one view per scene)
    assert default_views_per_call(1) == MAX_SCENES_PER_CALL and default_views_per_call(16) == MAX_SCENES_PER_CALL // 16
    assert default_views_per_call(MAX_SCENES_PER_CALL + 1) == 1
    assert all(B * default_views_per_call(B) <= MAX_SCENES_PER_CALL for B in range(1, MAX_SCENES_PER_CALL + 1))
    with pytest.raises(ValueError):
        plan_view_chunks(4, 1, 0)
