"""CPU: the host side of a context that grows (csrc/kv_append.hip, MIGT.append_to_context / rollout_from_context,
ViewRenderer.append / rollout) — ``vf_kv_append`` validates its arguments before any launch, the pure planners equal brute force, a
renderer without a context refuses, and path cameras through ``query_poses`` are the tail of the evaluator's bookkeeping on the whole
sequence, bit for bit.  No device is touched."""
import ctypes

import numpy as np
import pytest
import torch


@pytest.fixture(scope='module')
def lib():
    from viewformer_amd import build, _lib
    build.build()                      # hipcc cross-compiles gfx950 without a GPU
    return _lib.load()


def _call(lib, qkv=4096, cache=8192, elem_bytes=2, B=2, K=3, L=64, d=768, ld_src=2304, ld_dst=2304, cache_stride=7 * 64 * 2304, capacity=7,
          pos=4096):
    P = ctypes.c_void_p
    ptr = lambda x: None if x is None else P(x)          # never dereferenced: validation happens before any launch
    return lib.vf_kv_append(ptr(qkv), ptr(cache), elem_bytes, B, K, L, d, ld_src, ld_dst, cache_stride, capacity, ptr(pos), None)


@pytest.mark.parametrize('elem_bytes', [2, 4])
def test_kv_append_validates_its_arguments_without_a_device(lib, elem_bytes):
    call = lambda **kw: _call(lib, elem_bytes=elem_bytes, **kw)
    for name in ('qkv', 'cache', 'pos'):
        assert call(**{name: None}) == -1, name                                # null pointers
        assert call(**{name: None}, B=0) == -1, name                           # ... also where there would be no work
    for name in ('ld_src', 'ld_dst'):
        assert call(**{name: 3 * 768 - 8}) == -1, name                         # leading dimension below 3 d
    unit = 16 // elem_bytes                                                    # elements per 16-byte vector
    assert call(d=768 + unit // 2, ld_src=4096, ld_dst=4096, cache_stride=7 * 64 * 4096) == -1          # d * elem_bytes % 16
    assert call(ld_src=2304 + unit // 2) == -1 and call(ld_dst=2304 + unit // 2, cache_stride=7 * 64 * 2312) == -1
    assert call(cache_stride=7 * 64 * 2304 + unit // 2) == -1
    assert call(qkv=4096 + 8) == -1 and call(cache=8192 + 8) == -1             # rows are moved as 16-byte vectors
    for name in ('B', 'K', 'L', 'd', 'capacity', 'cache_stride'):
        assert call(**{name: -1}) == -1, name                                  # negative sizes
    assert call(cache_stride=7 * 64 * 2304 - 2304) == -1                       # scenes would overlap


def test_kv_append_elem_bytes_and_the_two_no_ops(lib):
    for eb in (0, 1, 3, 8, -2):
        assert _call(lib, elem_bytes=eb) == -1, eb                             # bf16 (2) and fp32 (4) only
    assert _call(lib, B=0) == 0 and _call(lib, K=0) == 0                       # nothing to do: no launch
    assert _call(lib, B=0, elem_bytes=4) == 0 and _call(lib, K=0, elem_bytes=4) == 0
    assert _call(lib, B=0, ld_src=100) == -1 and _call(lib, K=0, elem_bytes=3) == -1       # ... but bad arguments are still refused
    assert _call(lib, B=1 << 16, K=1 << 16) == -2                              # more views than a grid dimension holds: unsupported, not launched


def test_ops_kv_append_refuses_cpu_tensors_and_wrong_dtypes(lib):
    from viewformer_amd import ops, _lib
    q, c, pos = torch.zeros(64, 192), torch.zeros(128, 192), torch.zeros(1, dtype=torch.int32)
    with pytest.raises(_lib.VfError):
        ops.kv_append(q, c, 1, 1, 64, 64, 192, 192, 128 * 192, 2, pos)
    with pytest.raises(TypeError):
        ops.kv_append(q.half(), c.half(), 1, 1, 64, 64, 192, 192, 128 * 192, 2, pos)


# ---------------------------------------------------------------------------------------------- the planners against brute force
def test_capacity_growth_against_brute_force():
    from viewformer_amd.render import plan_capacity
    for cap in range(0, 40):
        for need in range(0, 100):
            got = plan_capacity(cap, need)
            assert got >= need and got >= cap
            assert got == (cap if need <= cap else max(2 * cap, need))
    # T appends of one view: every view has room, and the cache is reallocated O(log T) times
    cap, moves = 3, 0
    for filled in range(3, 1000):
        new = plan_capacity(cap, filled + 1)
        moves += new != cap
        cap = new
        assert cap >= filled + 1
    assert moves <= 10
    with pytest.raises(ValueError):
        plan_capacity(-1, 3)
    with pytest.raises(ValueError):
        plan_capacity(3, -1)


def test_rollout_lengths_against_the_explicit_loop():
    """the loop of the definition: step t generates from the lengths as they stand, then appends one view (lengths += 1)"""
    from viewformer_amd.render import plan_rollout_lengths
    for lengths in ([3], [1, 3, 2, 3], [0, 7], [5] * 16):
        for T in (0, 1, 2, 3, 9):
            gen, pair = plan_rollout_lengths(np.asarray(lengths, dtype=np.int32), T)
            assert gen.dtype == np.int32 and pair.dtype == np.int32 and gen.shape == (T, len(lengths)) and pair.shape == (T, len(lengths), 2)
            assert gen.flags['C_CONTIGUOUS'] and pair.flags['C_CONTIGUOUS']
            cur = list(lengths)
            for t in range(T):
                assert gen[t].tolist() == cur                                  # what the MASK view of step t sees = where view t is appended
                if t:
                    # the fused step: the append view of step t-1 sees the cache before it, the MASK view of step t one view more
                    assert pair[t, :, 0].tolist() == [c - 1 for c in cur] and pair[t, :, 1].tolist() == cur
                cur = [c + 1 for c in cur]
    for bad in ([[1, 2]], [1.0, 2.0], [True], [-1, 2]):
        with pytest.raises(ValueError):
            plan_rollout_lengths(np.asarray(bad), 2)
    with pytest.raises(ValueError):
        plan_rollout_lengths(np.asarray([1]), -1)


def test_replication_order_and_noise_row_ids_against_brute_force():
    from viewformer_amd.render import plan_replication, rollout_row_ids
    for B in (0, 1, 3):
        for S in (1, 2, 5):
            rep = plan_replication(B, S)
            assert rep.dtype == np.int64 and rep.tolist() == [b for b in range(B) for s in range(S)]     # scene b*S+s is a copy of scene b
    with pytest.raises(ValueError):
        plan_replication(2, 0)
    L = 64
    for n, t in ((1, 0), (6, 0), (6, 5), (2, (1 << 26) - 1)):
        ids = rollout_row_ids(n, t, L)
        assert ids.dtype == np.int64 and ids.shape == (n * L,)
        # sample_from_context's key for scene i, view t (view0 = t, N = 1), token l
        assert ids.tolist() == [(i << 32) | (t * L + l) for i in range(n) for l in range(L)]
    # a trajectory's keys do not depend on T (they are a function of the step), and no two (scene, step, token) share one
    a = np.concatenate([rollout_row_ids(4, t, L) for t in range(3)])
    assert len(set(a.tolist())) == a.size
    with pytest.raises(ValueError):
        rollout_row_ids(2, 1 << 26, L)


# ---------------------------------------------------------------------------------------------- the renderer
def test_append_and_rollout_refuse_a_renderer_without_a_context():
    from viewformer_amd.render import ViewRenderer
    r = ViewRenderer(None, None)
    cams = torch.zeros(1, 2, 7)
    with pytest.raises(RuntimeError, match='set_context'):
        r.append(codes=torch.zeros(1, 2, 8, 8, dtype=torch.int32), cameras=cams)
    with pytest.raises(RuntimeError, match='set_context'):
        r.rollout(cams)


def _cameras(B, V, seed):
    g = np.random.Generator(np.random.PCG64(seed))
    cam = g.standard_normal((B, V, 7)).astype(np.float32)
    cam[..., :3] *= 2.0
    return torch.from_numpy(cam)               # un-normalised quaternions of either sign: normalize_cameras has work to do


@pytest.mark.parametrize('augment', ['relative', 'no'])
def test_path_cameras_are_the_tail_of_the_whole_sequences_bookkeeping(augment):
    """``append`` and ``rollout`` send world-frame cameras through ``query_poses`` with the context's transform; a context that had held
    all views from the start would have relativised and normalised the whole sequence at once.  The same cameras, bit for bit — so an
    appended view's pose embedding is the one ``set_context`` of all views computes.  This pins a property of functions that existed
    before contexts could grow (``query_poses``, ``context_poses``): it is the premise of ``append`` / ``rollout``, not a test of new code."""
    from viewformer_amd import geometry
    from viewformer_amd.render import context_poses, query_poses
    B, C, T = 3, 4, 9
    ctx, path = _cameras(B, C, 11), _cameras(B, T, 12)
    cpos, transform = context_poses(ctx, augment)
    got = query_poses(path, transform)
    seq = torch.cat([ctx, path], 1)
    if augment == 'relative':
        seq = geometry.to_relative_cameras(seq)[0]
    seq = geometry.normalize_cameras(seq)
    assert torch.equal(got, seq[:, C:]) and torch.equal(cpos, seq[:, :C])
    # ... and view by view, as a roll-out appends them
    for t in range(T):
        assert torch.equal(query_poses(path[:, t:t + 1], transform), seq[:, C + t:C + t + 1]), t
