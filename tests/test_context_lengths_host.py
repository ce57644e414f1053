"""CPU: the host side of per-query context lengths — ``render.plan_context_lengths`` and ``render.sweep_layout`` are
pure functions, the fp64 reference of the GPU tests equals a masked softmax, and the two ``vf_attn_prefix_var_*`` entries validate their
arguments before any launch.  No device is touched."""
import ctypes

import numpy as np
import pytest
import torch

from context_lengths_ref import attn_fp64_lengths, rand


# ---------------------------------------------------------------------------------------------- plan_context_lengths
def test_plan_context_lengths_broadcasts_an_int_a_scene_list_and_a_view_table():
    from viewformer_amd.render import plan_context_lengths as plan
    B, N, C = 2, 3, 6
    a = plan(4, B, N, C)
    assert a.dtype == np.int32 and a.shape == (B, N) and (a == 4).all() and a.flags['C_CONTIGUOUS']
    assert plan(np.int64(0), B, N, C).tolist() == [[0, 0, 0], [0, 0, 0]]
    assert plan([2, 6], B, N, C).tolist() == [[2, 2, 2], [6, 6, 6]]
    assert plan(torch.tensor([2, 6]), B, N, C).tolist() == [[2, 2, 2], [6, 6, 6]]
    table = [[0, 1, 2], [6, 5, 4]]
    for form in (table, np.asarray(table, dtype=np.int16), torch.tensor(table)):
        got = plan(form, B, N, C)
        assert got.dtype == np.int32 and got.tolist() == table
    assert plan(np.zeros((B, 0), dtype=np.int64), B, 0, C).shape == (B, 0)
    assert plan(3, B, 0, C).shape == (B, 0)
    # B = N: a [B] list is one length per scene
    assert plan([1, 2], 2, 2, C).tolist() == [[1, 1], [2, 2]]


def test_plan_context_lengths_uses_the_scene_default_only_without_an_argument():
    from viewformer_amd.render import plan_context_lengths as plan
    B, N, C = 2, 3, 6
    assert plan(None, B, N, C) is None
    assert plan(None, B, N, C, scene_default=None) is None
    assert plan(None, B, N, C, scene_default=np.array([2, 6], dtype=np.int32)).tolist() == [[2, 2, 2], [6, 6, 6]]
    assert plan(1, B, N, C, scene_default=[2, 6]).tolist() == [[1, 1, 1], [1, 1, 1]]


@pytest.mark.parametrize('bad', [1.0, [1.0, 2.0], np.array([[1.5, 2, 3], [1, 2, 3]]), True, [True, False], -1, [0, -1], 7, [[0, 1, 2], [3, 4, 7]],
                                 [1, 2, 3], [[1, 2], [3, 4]], [[1, 2, 3]], [[[1, 2, 3], [1, 2, 3]]], [], 'two'])
def test_plan_context_lengths_refuses(bad):
    from viewformer_amd.render import plan_context_lengths as plan
    with pytest.raises(ValueError):
        plan(bad, 2, 3, 6)


# ---------------------------------------------------------------------------------------------- the fp64 helper
def _masked_softmax_attention(qkv_ctx, qkv_q, B, H, C, N, lengths, L=64):
    """all C*L + L keys with the invisible ones at -inf: torch.softmax gives them an exact zero"""
    ctx = qkv_ctx.double().view(B, C * L, 3, H, 64)
    qq = qkv_q.double().view(B, N, L, 3, H, 64)
    kc, vc = ctx[:, :, 2].permute(0, 2, 1, 3), ctx[:, :, 0].permute(0, 2, 1, 3)
    q, k, v = (qq[:, :, :, i].permute(0, 3, 1, 2, 4) for i in (1, 2, 0))
    kk = torch.cat([kc[:, :, None].expand(B, H, N, C * L, 64), k], 3)
    vv = torch.cat([vc[:, :, None].expand(B, H, N, C * L, 64), v], 3)
    s = q @ kk.transpose(-1, -2)                                                              # [B,H,N,L,C*L+L]
    view_of_key = torch.arange(C * L + L) // L
    ln = torch.as_tensor(lengths).view(B, 1, N, 1, 1)
    visible = (view_of_key.view(1, 1, 1, 1, -1) < ln) | (view_of_key.view(1, 1, 1, 1, -1) == C)
    p = torch.softmax(s.masked_fill(~visible, float('-inf')), -1)
    return (p @ vv).permute(0, 2, 3, 1, 4).reshape(B * N * L, H * 64)


def test_the_fp64_reference_equals_a_masked_softmax():
    B, H, C, N = 2, 2, 3, 5
    d = H * 64
    ctx, q = rand((B * C * 64, 3 * d), 1, 0.35), rand((B * N * 64, 3 * d), 2, 0.35)
    lengths = [[0, 3, 1, 3, 2], [2, 0, 0, 1, 3]]
    got = attn_fp64_lengths(ctx, q, B, H, C, N, lengths)
    want = _masked_softmax_attention(ctx, q, B, H, C, N, lengths)
    assert got.dtype == torch.float64 and got.shape == want.shape
    assert float((got - want).abs().max()) < 1e-14                     # fp64 sums in two orders
    full = attn_fp64_lengths(ctx, q, B, H, C, N, np.full((B, N), C))
    unmasked = _masked_softmax_attention(ctx, q, B, H, C, N, np.full((B, N), C + 1))   # nothing masked at all
    assert float((full - unmasked).abs().max()) < 1e-14
    assert float((got - full).abs().max()) > 1e-3                      # ... and the lengths matter


# ---------------------------------------------------------------------------------------------- sweep's layout
@pytest.mark.parametrize('N', [1, 2, 5])
@pytest.mark.parametrize('K', [1, 2, 5])
def test_sweep_layout_is_size_major_and_its_inverse_brings_views_back_per_camera(N, K):
    from viewformer_amd.render import sweep_layout
    cam, size, inverse = sweep_layout(N, K)
    assert cam.shape == (K * N,) and size.shape == (K * N,) and inverse.shape == (N, K)
    assert size.tolist() == sorted(size.tolist())                      # size-major: equal lengths are consecutive
    assert sorted(zip(cam.tolist(), size.tolist())) == [(n, k) for n in range(N) for k in range(K)]      # every pair once
    rendered = torch.from_numpy(cam * 100 + size).view(1, K * N)       # what "rendering" view j yields: its own (camera, size)
    back = rendered[:, torch.from_numpy(inverse.reshape(-1))].view(1, N, K)
    assert back[0].tolist() == [[n * 100 + k for k in range(K)] for n in range(N)]


def test_sweep_layout_of_nothing():
    from viewformer_amd.render import sweep_layout
    for N, K in ((0, 3), (3, 0)):
        cam, size, inverse = sweep_layout(N, K)
        assert cam.shape == (0,) and size.shape == (0,) and inverse.shape == (N, K)


# ---------------------------------------------------------------------------------------------- the entries' argument checks
@pytest.fixture(scope='module')
def lib():
    from viewformer_amd import build, _lib
    build.build()                      # hipcc cross-compiles gfx950 without a GPU
    return _lib.load()


def _call(lib, arm, ctx_len=4096, q=4096, B=2, H=12, C=6, N=8, L=64, dh=64, ldq=2304, ldo=768):
    P = ctypes.c_void_p
    ptr = lambda x: None if x is None else P(x)          # never dereferenced: validation happens before any launch
    ld, stride = 2304, 6 * 64 * 2304
    if arm == 'bf16':
        return lib.vf_attn_prefix_var_bf16(ptr(q), P(4096), P(4096), P(4096), P(4096), 1, P(4096), 1, B, H, C, N, L, dh, ldq, ld, ld, ld, ld,
                                           stride, ldo, ptr(ctx_len), None)
    return lib.vf_attn_prefix_var_f32eq(ptr(q), P(4096), P(4096), P(4096), P(4096), P(4096), B, H, C, N, L, dh, ldq, ld, ld, ld, ld,
                                        stride, ldo, ptr(ctx_len), None)


@pytest.mark.parametrize('arm', ['bf16', 'f32eq'])
def test_variable_length_prefix_attention_validates_its_arguments_without_a_device(lib, arm):
    assert _call(lib, arm, ctx_len=None) == -1                                 # NULL lengths
    assert _call(lib, arm, q=None) == -1
    assert _call(lib, arm, L=32) == -2                                         # 64-token views only
    assert _call(lib, arm, dh=32) == -2
    assert _call(lib, arm, C=0) == -2                                          # C is the cache's capacity: at least one view
    assert _call(lib, arm, ldq=12 * 64 - 8) == -1                              # leading dimension below H * 64
    assert _call(lib, arm, N=0) == 0 and _call(lib, arm, B=0) == 0             # nothing to do: no launch
    assert _call(lib, arm, N=0, ctx_len=None) == -1                            # ... but a missing argument is still refused


def test_both_new_entries_are_exported_and_the_abi_version_stays():
    from viewformer_amd import _lib
    for name in ('vf_attn_prefix_var_bf16', 'vf_attn_prefix_var_f32eq'):
        assert name in _lib.EXPORTS
        fixed = _lib.EXPORTS[name.replace('_var', '')]
        assert _lib.EXPORTS[name][0] is fixed[0]
        assert _lib.EXPORTS[name][1] == fixed[1][:-1] + [ctypes.c_void_p, ctypes.c_void_p]      # ..., ctx_len, stream
    from viewformer_amd import build
    build.build()
    assert _lib.load().vf_abi_version() == 20


def test_ops_attn_prefix_refuses_host_or_misshapen_lengths(lib):
    from viewformer_amd import ops, _lib
    z = torch.zeros(64, 192)
    with pytest.raises(_lib.VfError):                                          # lengths on the host: refused before anything else
        ops.attn_prefix(z[:, 64:128], z[:, 128:], z[:, :64], z[:, 128:], z[:, :64], torch.zeros(64, 64), 1, 1, 1, 1, 64,
                        192, 192, 192, 192, 192, 64 * 192, 64, ctx_len=torch.zeros(1, dtype=torch.int32))
