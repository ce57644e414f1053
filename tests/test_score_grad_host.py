"""CPU: the host side of the score gradient — ``render.ascend_poses`` against a numpy brute force, the float64 oracle
gradient that tests/test_hip_score_grad.py compares the device with against central differences of the same oracle, and the refusals of
``MIGT.score_grad_from_context`` / ``refine_from_context`` and ``ViewRenderer.score_gradient`` / ``refine`` before any launch.  No device
is touched."""
import numpy as np
import pytest
import torch

import score_grad_ref as G

SMALL = dict(n_embeddings=128, n_head=2, d_model=128, n_layer=2, token_image_size=8, pose_multiplier=0.2)      # tests/test_hip_score.py's


# ---------------------------------------------------------------------------------------------- ascend_poses
def _poses_and_grads(n, seed):
    g = np.random.Generator(np.random.PCG64(seed))
    p = g.standard_normal((n, 7)).astype(np.float32)
    p[:, 3:] /= np.linalg.norm(p[:, 3:], axis=1, keepdims=True)
    p[:, 3:] *= np.where(p[:, 3:4] >= 0, 1, -1)
    return p.astype(np.float32), g.standard_normal((n, 7)).astype(np.float32)


def test_ascend_poses_against_the_brute_force():
    from viewformer_amd.render import ascend_poses
    p, g = _poses_and_grads(24, 5)
    g[3, :3] = 0                       # no position gradient
    g[4, 3:] = 0                       # no rotation gradient
    g[5] = 0                           # neither
    g[6, 3:] = 3.0 * p[6, 3:]          # a radial quaternion gradient: no direction on the sphere
    p[7, 3:] = [0.0, 1.0, 0.0, 0.0]    # w = 0: the step decides the sign
    sx = np.linspace(0.01, 0.5, 24).astype(np.float32)
    sr = np.linspace(0.3, 0.001, 24).astype(np.float32)
    got = ascend_poses(torch.from_numpy(p), torch.from_numpy(g), torch.from_numpy(sx), torch.from_numpy(sr))
    want = G.ascend_brute(p, g, sx, sr)
    assert got.dtype == torch.float32 and tuple(got.shape) == (24, 7)
    np.testing.assert_allclose(got.numpy(), want, rtol=0, atol=2e-6)
    q = got[:, 3:].double()
    assert float((q.norm(dim=1) - 1).abs().max()) < 1e-6 and bool((q[:, 0] >= 0).all())          # unit quaternions, w >= 0
    moved = (got - torch.from_numpy(p)).double()
    np.testing.assert_allclose(moved[:, :3].norm(dim=1).numpy()[[0, 1, 2, 8]], sx[[0, 1, 2, 8]], rtol=1e-4)      # the step lengths
    chord = torch.minimum(moved[:, 3:].norm(dim=1), (got + torch.from_numpy(p)).double()[:, 3:].norm(dim=1)).numpy()     # (either sign)
    keep = [i for i in range(24) if i not in (4, 5, 6, 7)]
    np.testing.assert_allclose(chord[keep], (2 * np.sin(np.arctan(sr.astype(np.float64)) / 2))[keep], rtol=1e-3)  # q + s t: an angle atan(s)
    for i, blocks in ((3, [slice(0, 3)]), (4, [slice(3, 7)]), (5, [slice(0, 3), slice(3, 7)]), (6, [slice(3, 7)])):
        for b in blocks:
            assert torch.equal(got[i, b], torch.from_numpy(p)[i, b]), (i, b)                     # a zero block does not move, bit for bit
    # scalar steps and leading dimensions broadcast
    two = ascend_poses(torch.from_numpy(p).view(4, 6, 7), torch.from_numpy(g).view(4, 6, 7), 0.05, 0.05)
    np.testing.assert_allclose(two.view(24, 7).numpy(), G.ascend_brute(p, g, np.full(24, 0.05), np.full(24, 0.05)), rtol=0, atol=2e-6)
    with pytest.raises(ValueError):
        ascend_poses(torch.zeros(2, 7), torch.zeros(3, 7), 0.1, 0.1)
    with pytest.raises(ValueError):
        ascend_poses(torch.zeros(2, 6), torch.zeros(2, 6), 0.1, 0.1)


# ---------------------------------------------------------------------------------------------- the oracle's gradient
def test_the_oracle_gradient_against_central_differences_of_the_oracle():
    """float64 autograd of ``migt_forward(..., grad=True)`` on [ctx, MASK], sum of log_softmax at the codes, w.r.t. the last pose, against
    central differences (h = 2^-9, poses on that grid so that p +- h is exact) of the same function: truncation h^2 f''' / 6 — 1e-3 of
    the gradient's size covers it a hundred times at these curvatures.  Pins the reference of the GPU test; passes on any tree."""
    from viewformer_amd.config import MIGTConfig
    from viewformer_amd.weights import make_migt_weights
    C = 2
    cfg = MIGTConfig(sequence_size=C + 1, n_loss_skip=1, localization_weight='1', **SMALL)
    sd = make_migt_weights(cfg, seed=1, std=0.05)
    g = np.random.Generator(np.random.PCG64(9))
    ctx = torch.from_numpy(g.integers(0, cfg.n_embeddings, size=(C, 8, 8)))
    codes = torch.from_numpy(g.integers(0, cfg.n_embeddings, size=(1, 8, 8)))
    h = 2.0 ** -9
    grid = lambda x: torch.round(x / h) * h
    cpos = grid(torch.from_numpy(g.standard_normal((C, 7)).astype(np.float32)))
    pose = grid(torch.from_numpy(g.standard_normal(7).astype(np.float32)))          # the 7 numbers are free: no normalisation here
    g64, ll = G.oracle_grad(sd, cfg, ctx, cpos, pose[None], codes)
    fd = G.oracle_central_differences(sd, cfg, ctx, cpos, pose, codes[0], h)
    scale = float(g64.abs().max())
    assert scale > 0 and bool(torch.isfinite(ll).all())
    assert float((g64[0] - fd).abs().max()) <= 1e-3 * scale, (g64, fd)
    g32, _ = G.oracle_grad(sd, cfg, ctx, cpos, pose[None], codes, dtype=torch.float32)
    assert float((g32 - g64).abs().max()) <= 1e-3 * scale


# ---------------------------------------------------------------------------------------------- refusals before any launch
def test_the_new_entry_points_refuse_bad_arguments_without_a_device():
    from viewformer_amd.config import MIGTConfig
    from viewformer_amd.migt import MIGT
    from viewformer_amd.render import ViewRenderer
    m = MIGT(MIGTConfig(sequence_size=3, **SMALL))
    cams, codes = torch.zeros(1, 2, 7), torch.zeros(1, 2, 8, 8, dtype=torch.int32)
    for f in (m.score_grad_from_context, m.refine_from_context):
        with pytest.raises(TypeError, match='ContextCache'):
            f(None, cams, codes)
        with pytest.raises(TypeError, match='ContextCache'):
            f(dict(kv=[]), cams, codes)
    r = ViewRenderer(None, None)
    with pytest.raises(RuntimeError, match='set_context'):
        r.score_gradient(cams, codes=codes)
    with pytest.raises(RuntimeError, match='set_context'):
        r.refine(cams, codes=codes)
    with pytest.raises(RuntimeError, match='set_context'):
        r.refine(None, codes=codes)


def test_query_rows_keeps_its_signature_and_gains_one_keyword():
    import inspect
    from viewformer_amd.migt import MIGT
    sig = inspect.signature(MIGT._query_rows)
    assert list(sig.parameters) == ['self', 'cache', 'ids32', 'add', 'N', 'n_context', 'append_at', 'tail', 'save']
    assert sig.parameters['save'].default is None
    sig = inspect.signature(MIGT.refine_from_context)
    assert {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty} == dict(
        steps=16, step_xyz=0.05, step_rot=0.05, n_context=None, return_trace=False)
