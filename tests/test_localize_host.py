"""CPU: the host side of localization from a cached context (viewformer_amd/render.py: ViewRenderer.localize,
MIGT.localize_from_context, csrc/pose_tail.hip).  This file holds the fp64 restatement of the pose head's tail that
tests/test_hip_localize.py measures the kernel against, and the inputs of that kernel test with the properties it relies on — checked
here, on the reference alone, where no kernel output can influence them.  No device is touched."""
import ctypes
import types

import numpy as np
import pytest
import torch

EPS32 = float(np.finfo(np.float32).eps)          # 2^-23


@pytest.fixture(scope='module')
def lib():
    from viewformer_amd import build, _lib
    build.build()                      # hipcc cross-compiles gfx950 without a GPU
    return _lib.load()


# ---------------------------------------------------------------------------------------------- the tail in fp64, from its definition
def tail_from_raw_fp64(raw, position_multiplier):
    """raw [views, L, 7] -> (tokens [views, L, 7], cameras [views, 7], rho_tok [views, L], rho_mean [views]) in fp64.
    token: xyz = raw.xyz / multiplier; q = raw.q * rsqrt(max(sum raw.q^2, 1e-12)), times (q.w >= 0 ? 1 : -1).
    camera: xyz = mean over the view's tokens; q = the mean of the token quaternions, normalised and sign-fixed the same way.
    rho_tok: the norm of each raw quaternion; rho_mean: the norm of each view's mean token quaternion."""
    raw = raw.double()
    xyz = raw[..., :3] / float(position_multiplier)
    ss = (raw[..., 3:] ** 2).sum(-1, keepdim=True)
    q = raw[..., 3:] * ss.clamp(min=1e-12).rsqrt()
    q = q * torch.where(q[..., :1] >= 0, 1.0, -1.0)
    tokens = torch.cat([xyz, q], -1)
    L = raw.shape[-2]
    mq = q.sum(-2) / L
    ms = (mq ** 2).sum(-1, keepdim=True)
    cq = mq * ms.clamp(min=1e-12).rsqrt()
    cq = cq * torch.where(cq[..., :1] >= 0, 1.0, -1.0)
    cameras = torch.cat([xyz.sum(-2) / L, cq], -1)
    return tokens, cameras, ss[..., 0].sqrt(), ms[..., 0].sqrt()


def pose_tail_fp64(x, W, b, position_multiplier, views, L):
    """x [views*L, K], W [K, 7], b [7] or None -> dict(raw, tokens, cameras, rho_tok, rho_mean, E): the tail of the fp32 inputs in
    fp64, and E [views, L, 7] = 16 eps32 (sum_k |x_k| |W_k| + |b|), the bound on an fp32 evaluation's error in raw."""
    x, W = x.double(), W.double()
    bb = torch.zeros(7, dtype=torch.float64) if b is None else b.double()
    raw = (x @ W + bb).view(views, L, 7)
    E = (16 * EPS32 * (x.abs() @ W.abs() + bb.abs())).view(views, L, 7)
    tokens, cameras, rho_tok, rho_mean = tail_from_raw_fp64(raw, position_multiplier)
    return dict(raw=raw, tokens=tokens, cameras=cameras, rho_tok=rho_tok, rho_mean=rho_mean, E=E)


def tail_bounds(E_max, rho_tok, rho_mean, position_multiplier):
    """(token q, token xyz, camera q, camera xyz) bounds of an fp32 evaluation of the tail whose raw is within E_max of the exact one:
    a unit quaternion moves by at most ~2 |d raw| / rho under normalisation (4 leaves room for the fp32 normalisation itself), the mean of
    such quaternions by the same, and its normalisation divides by rho_mean once more; xyz errors are E / multiplier, means no larger."""
    tq = 4 * E_max / rho_tok + 1e-6
    txyz = E_max / position_multiplier + 1e-6
    return tq, txyz, 4 * E_max / (rho_tok * rho_mean) + 1e-6, txyz


# ---------------------------------------------------------------------------------------------- the kernel test's inputs
TAIL_SHAPES = [(1, 64, 1536, 0), (5, 64, 1536, 0), (3, 16, 256, 0), (2, 1, 64, 0), (4, 100, 2048, 0), (3, 64, 100, 0), (5, 64, 1536, 12)]   # views, L, K, ldx - K
TAIL_MULTIPLIER = 0.2


def tail_inputs(views, L, K):
    """x ~ 0.5 N(0,1) [views*L, K], W ~ 0.03 N(0,1) [K, 7], b ~ 0.01 N(0,1) [7] (fp32), with one feature that alternates +-1 from row to
    row and carries three standard deviations of a raw output onto the quaternion's w: both signs of w occur in every view of two or
    more tokens, and |w| is rarely small.  The seed depends on the shape only."""
    g = np.random.Generator(np.random.PCG64(1000 + 7 * views + 3 * L + K))
    x = (0.5 * g.standard_normal((views * L, K))).astype(np.float32)
    W = (0.03 * g.standard_normal((K, 7))).astype(np.float32)
    b = (0.01 * g.standard_normal(7)).astype(np.float32)
    x[:, 0] = np.where(np.arange(views * L) % 2 == 0, 1.0, -1.0)
    W[0, 3] = 3 * 0.5 * 0.03 * np.sqrt(K)
    return torch.from_numpy(x), torch.from_numpy(W), torch.from_numpy(b)


def check_tail_preconditions(ref):
    """the properties of the reference that the kernel test's bounds rely on"""
    w_rel = ref['raw'][..., 3].abs() / ref['rho_tok']
    assert float(w_rel.min()) >= 1e-3, float(w_rel.min())                   # no token sits on the sign boundary
    assert float(ref['rho_mean'].min()) >= 0.1, float(ref['rho_mean'].min())
    assert bool((ref['raw'][..., 3] > 0).any()) and bool((ref['raw'][..., 3] < 0).any())


@pytest.mark.parametrize('views,L,K,pad', TAIL_SHAPES[:-1])
def test_kernel_test_inputs_have_the_properties_its_bounds_rely_on(views, L, K, pad):
    x, W, b = tail_inputs(views, L, K)
    check_tail_preconditions(pose_tail_fp64(x, W, b, TAIL_MULTIPLIER, views, L))


def test_fp64_restatement_equals_the_oracles_pose_head_and_reduce_cameras():
    from oracle import migt_oracle as mg
    from viewformer_amd import geometry
    g = np.random.Generator(np.random.PCG64(5))
    views, L, d, K = 3, 10, 24, 40
    name = 'pose_criterion.pose_classifier'
    sd = {name + '.c_fc.weight': g.standard_normal((d, K)) * 0.3, name + '.c_fc.bias': g.standard_normal(K) * 0.1,
          name + '.c_proj.weight': g.standard_normal((K, 7)) * 0.3, name + '.c_proj.bias': g.standard_normal(7) * 0.1}
    cfg = types.SimpleNamespace(pose_multiplier=0.2)
    hidden = torch.from_numpy(g.standard_normal((views, L, d)))
    want_tok = mg.pose_head(sd, cfg, hidden, torch.float64)
    want_cam = geometry.reduce_cameras(want_tok, -2)
    x = mg.gelu(mg.conv1d(sd, name + '.c_fc', hidden, torch.float64)).reshape(views * L, K)
    got = pose_tail_fp64(x, torch.from_numpy(sd[name + '.c_proj.weight']), torch.from_numpy(sd[name + '.c_proj.bias']), 0.2, views, L)
    assert bool((want_tok[..., 3] >= 0).all()) and bool((mg.mlp(sd, name, hidden, torch.float64)[..., 3] < 0).any())     # the sign fix had work to do
    assert float((got['tokens'] - want_tok).abs().max()) <= 1e-12
    assert float((got['cameras'] - want_cam).abs().max()) <= 1e-12
    assert float((got['cameras'] - mg.reduce_cameras(want_tok, -2)).abs().max()) <= 1e-12
    # b = None is b = 0
    z = pose_tail_fp64(x, torch.from_numpy(sd[name + '.c_proj.weight']), None, 0.2, views, L)
    assert torch.equal(z['raw'], (x @ torch.from_numpy(sd[name + '.c_proj.weight'])).view(views, L, 7))


def test_from_relative_cameras_broadcasts_one_transform_over_n_cameras():
    """ViewRenderer.localize maps [B,N,7] cameras back with the context's [B,1,7] transform in one call; the evaluator does it one
    camera at a time (evaluate_transformer.py:139-140).  Same bits."""
    from viewformer_amd import geometry
    g = np.random.Generator(np.random.PCG64(9))
    B, N = 3, 11
    cams = torch.from_numpy(g.standard_normal((B, N, 7)).astype(np.float32))
    transform = geometry.normalize_cameras(torch.from_numpy(g.standard_normal((B, 1, 7)).astype(np.float32)))
    got = geometry.from_relative_cameras(cams, transform)
    assert got.shape == (B, N, 7)
    for n in range(N):
        assert torch.equal(got[:, n:n + 1], geometry.from_relative_cameras(cams[:, n:n + 1], transform)), n


def _tail(lib, x=4096, ldx=1536, W=4096, b=4096, mult=0.2, views=4, L=64, K=1536, raw=4096, tokens=4096, cameras=4096):
    P = ctypes.c_void_p
    ptr = lambda v: None if v is None else P(v)          # never dereferenced: validation happens before any launch
    return lib.vf_pose_tail_f32(ptr(x), ldx, ptr(W), ptr(b), mult, views, L, K, ptr(raw), ptr(tokens), ptr(cameras), None)


def test_pose_tail_validates_its_arguments_without_a_device(lib):
    assert _tail(lib, x=None) == -1 and _tail(lib, W=None) == -1 and _tail(lib, cameras=None) == -1
    assert _tail(lib, x=4100) == -1                                            # rows are read as float4: misaligned
    assert _tail(lib, ldx=1000) == -1                                          # ldx < K
    assert _tail(lib, views=-1) == -1 and _tail(lib, K=0) == -1
    assert _tail(lib, mult=0.0) == -1 and _tail(lib, mult=float('nan')) == -1 and _tail(lib, mult=float('inf')) == -1
    assert _tail(lib, K=1534) == -2                                            # K % 4
    assert _tail(lib, K=4096, ldx=4096) == -2                                  # K > 2048: W^T would not fit the LDS budget
    assert _tail(lib, L=0) == -2 and _tail(lib, L=257) == -2
    assert _tail(lib, ldx=1538) == -2                                          # ldx % 4
    assert _tail(lib, views=1 << 31) == -2                                     # one workgroup per view: the grid's limit
    assert _tail(lib, views=0) == 0                                            # nothing to do: no launch
    assert _tail(lib, views=0, raw=None, tokens=None, b=None) == 0             # the optional pointers
    assert _tail(lib, views=0, L=300) == -2                                    # ... but an unsupported shape is still refused


def test_ops_pose_tail_refuses_cpu_tensors_and_reports_its_shapes(lib):
    from viewformer_amd import ops, _lib
    with pytest.raises(_lib.VfError):
        ops.pose_tail(torch.zeros(128, 64), torch.zeros(64, 7), torch.zeros(7), 0.2, 2, 64)
    with pytest.raises(ValueError):
        ops.pose_tail(torch.zeros(128, 64), torch.zeros(64, 8), None, 0.2, 2, 64)
    assert ops.pose_tail_supported(1536, 64) and ops.pose_tail_supported(4, 1) and ops.pose_tail_supported(2048, 256)
    assert not ops.pose_tail_supported(1534, 64) and not ops.pose_tail_supported(4096, 64)
    assert not ops.pose_tail_supported(1536, 0) and not ops.pose_tail_supported(1536, 257)


def test_localize_needs_a_context():
    from viewformer_amd.render import ViewRenderer
    r = ViewRenderer(types.SimpleNamespace(), types.SimpleNamespace(device='cpu'))
    with pytest.raises(RuntimeError, match='set_context'):
        r.localize(codes=torch.zeros((1, 1, 8, 8), dtype=torch.int32))
    with pytest.raises(RuntimeError, match='set_context'):
        r.localize(images=torch.zeros((1, 1, 8, 8, 3), dtype=torch.uint8))
