"""GPU: localization of photos against a cached context (csrc/pose_tail.hip, MIGT.localize_from_context, ViewRenderer.localize) against
what the evaluator's route computes for the same scene: the fused pose-head tail against its fp64 restatement
(tests/test_localize_host.py) with derived bounds and on framed buffers, the fp32 arm against the full pass and the fp64 oracle, the
bf16 arm against the full pass's own error, ``localize`` against ``generate_batch_predictions`` on replicated contexts, and the
refusals.  Full-size models throughout.  Every measured figure goes through ``conftest.parity_report``.

Bounds of the tail (test_localize_host.tail_bounds): with E = 16 eps32 (sum_k |x_k| |W_k| + |b|) per element of raw, E_max its maximum,
rho_tok the smallest raw quaternion norm and rho_mean the smallest norm of a view's mean token quaternion, token quaternions lie within
4 E_max / rho_tok + 1e-6, token and camera xyz within E_max / multiplier + 1e-6 and camera quaternions within
4 E_max / (rho_tok rho_mean) + 1e-6 of the fp64 tail."""
import itertools
import types

import numpy as np
import pytest
import torch

from conftest import parity_report
from framed import Frame
from test_localize_host import (EPS32, TAIL_MULTIPLIER, TAIL_SHAPES, check_tail_preconditions, pose_tail_fp64, tail_bounds, tail_from_raw_fp64,
                                tail_inputs)

pytestmark = pytest.mark.gpu

F32_TOKEN_TOL = 1e-3            # fp32 arm against fp64, times max(1, peak): the project's bound (tests/test_hip_parity_scale.py)
NEAR_SIGN_TOKENS_MAX = 0.02     # tokens whose normalised |w| lies inside the two routes' own error: at most 2 % of all


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'needs the MI355X'
    return torch.device('cuda:0')


def _token_distance(a, b):
    """per token: max(|d xyz|, min(|q - q'|, |q + q'|)) (max norm over components); a, b [...,7] -> [...]"""
    a, b = a.double(), b.double()
    dx = (a[..., :3] - b[..., :3]).abs().amax(-1)
    dq = torch.minimum((a[..., 3:] - b[..., 3:]).abs().amax(-1), (a[..., 3:] + b[..., 3:]).abs().amax(-1))
    return torch.maximum(dx, dq)


def _sign_differs(a, b):
    a, b = a.double(), b.double()
    return (a[..., 3:] + b[..., 3:]).abs().amax(-1) < (a[..., 3:] - b[..., 3:]).abs().amax(-1)


def _as_raw(tokens):
    """tokens [...,7] -> a raw (fp64) whose fp64 tail has these tokens: the xyz times the multiplier, the unit quaternions as they are"""
    return tokens.double() * torch.tensor([0.2] * 3 + [1.0] * 4, dtype=torch.float64)


# ---------------------------------------------------------------------------------------------- (a) the kernel
_tail_refs = {}


def _tail_ref(views, L, K):
    """the shape's inputs and their fp64 tail: computed once, shared, never modified"""
    if (views, L, K) not in _tail_refs:
        x, W, b = tail_inputs(views, L, K)
        ref = pose_tail_fp64(x, W, b, TAIL_MULTIPLIER, views, L)
        check_tail_preconditions(ref)                                                # on the reference alone, before any kernel output
        _tail_refs[(views, L, K)] = (x, W, b, ref)
    return _tail_refs[(views, L, K)]


def _padded(x, pad, dev):
    """x on the device with ``pad`` floats of NaN behind every row"""
    if not pad:
        return x.to(dev)
    wide = torch.full((x.shape[0], x.shape[1] + pad), float('nan'), dtype=torch.float32, device=dev)
    wide[:, :x.shape[1]] = x.to(dev)
    return wide[:, :x.shape[1]]


@pytest.mark.parametrize('views,L,K,pad', TAIL_SHAPES)
def test_pose_tail_kernel_against_fp64_with_derived_bounds(dev, views, L, K, pad):
    from viewformer_amd import geometry, ops, train_ops
    x, W, b, ref = _tail_ref(views, L, K)
    xd, Wd, bd = _padded(x, pad, dev), W.to(dev), b.to(dev)
    assert xd.stride(0) == K + pad and ops.pose_tail_supported(K, L)
    runs = {}
    for want_raw, want_tokens in itertools.product((True, False), repeat=2):
        cam, tok, raw = ops.pose_tail(xd, Wd, bd, TAIL_MULTIPLIER, views, L, want_raw=want_raw, want_tokens=want_tokens)
        assert (raw is None) == (not want_raw) and (tok is None) == (not want_tokens)
        runs[(want_raw, want_tokens)] = (cam, tok, raw)
    torch.cuda.synchronize()
    cam, tok, raw = (t.cpu() for t in runs[(True, True)])
    assert tuple(cam.shape) == (views, 7) and tuple(tok.shape) == (views, L, 7) and tuple(raw.shape) == (views, L, 7)
    E_max, rho_tok, rho_mean = float(ref['E'].max()), float(ref['rho_tok'].min()), float(ref['rho_mean'].min())
    b_tq, b_txyz, b_cq, b_cxyz = tail_bounds(E_max, rho_tok, rho_mean, TAIL_MULTIPLIER)
    # the existing route on the same inputs, for information: the one-pass small-N layer and the two geometry functions on the GPU
    raw_old = train_ops.dense_small_n(xd, Wd, bd, views * L, K, 7).view(views, L, 7)
    tok_old = geometry.pose_head_postprocess(raw_old, TAIL_MULTIPLIER)
    cam_old = geometry.reduce_cameras(tok_old, -2)

    def errors(raw, tok, cam):
        return dict(raw_over_E=float(((raw.double() - ref['raw']).abs() / ref['E']).max()),
                    token_q=float((tok[..., 3:].double() - ref['tokens'][..., 3:]).abs().max()),
                    token_xyz=float((tok[..., :3].double() - ref['tokens'][..., :3]).abs().max()),
                    camera_q=float((cam[..., 3:].double() - ref['cameras'][..., 3:]).abs().max()),
                    camera_xyz=float((cam[..., :3].double() - ref['cameras'][..., :3]).abs().max()))
    fig, old = errors(raw, tok, cam), errors(raw_old.cpu(), tok_old.cpu(), cam_old.cpu())
    parity_report(test='pose_tail_kernel', views=views, L=L, K=K, ldx=K + pad, E_max=E_max, rho_tok=rho_tok, rho_mean=rho_mean,
                  bounds=dict(token_q=b_tq, token_xyz=b_txyz, camera_q=b_cq, camera_xyz=b_cxyz), fused=fig, existing_route=old,
                  raw_bit_identical_to_existing=bool(torch.equal(raw, raw_old.cpu())))
    assert not torch.isnan(raw).any() and not torch.isnan(tok).any() and not torch.isnan(cam).any()
    assert bool(((raw.double() - ref['raw']).abs() <= ref['E']).all()), fig
    assert fig['token_q'] <= b_tq and fig['token_xyz'] <= b_txyz, (fig, b_tq, b_txyz)
    assert fig['camera_q'] <= b_cq and fig['camera_xyz'] <= b_cxyz, (fig, b_cq, b_cxyz)
    # the outputs present are the same bits whichever optional outputs are NULL
    for key, (c2, t2, r2) in runs.items():
        assert torch.equal(c2.cpu(), cam), key
        assert t2 is None or torch.equal(t2.cpu(), tok), key
        assert r2 is None or torch.equal(r2.cpu(), raw), key
    # a view's outputs do not depend on the other views of the launch: view 0 alone
    if views > 1:
        c1, t1, r1 = ops.pose_tail(xd[:L], Wd, bd, TAIL_MULTIPLIER, 1, L, want_raw=True, want_tokens=True)
        assert torch.equal(c1.cpu(), cam[:1]) and torch.equal(t1.cpu(), tok[:1]) and torch.equal(r1.cpu(), raw[:1])
    # b = NULL is b = 0
    c0, t0, r0 = ops.pose_tail(xd, Wd, None, TAIL_MULTIPLIER, views, L, want_raw=True, want_tokens=True)
    cz, tz, rz = ops.pose_tail(xd, Wd, torch.zeros_like(bd), TAIL_MULTIPLIER, views, L, want_raw=True, want_tokens=True)
    assert torch.equal(c0, cz) and torch.equal(t0, tz) and torch.equal(r0, rz)


# ---------------------------------------------------------------------------------------------- (b) footprint
def test_pose_tail_kernel_footprint_on_framed_buffers(dev):
    """include/vf_hip.h "Memory footprint": every input and output inside a tests/framed.py Frame with NaN sentinels in every gap and
    guard; inputs unmodified, every guard intact, every logical output element written, the same bits as on compact tensors."""
    import ctypes
    from viewformer_amd import _lib, ops
    views, L, K, pad = 5, 64, 1536, 12
    x, W, b, _ = _tail_ref(views, L, K)
    fx = Frame(views * L, K, K + pad, torch.float32, dev).load(x)
    fW = Frame(K, 7, 7, torch.float32, dev).load(W)
    fb = Frame(1, 7, 7, torch.float32, dev).load(b.view(1, 7))
    fraw, ftok = Frame(views * L, 7, 7, torch.float32, dev), Frame(views * L, 7, 7, torch.float32, dev)
    fcam = Frame(views, 7, 7, torch.float32, dev)
    P = lambda f: ctypes.c_void_p(f.ptr)
    _lib.check(_lib.load().vf_pose_tail_f32(P(fx), K + pad, P(fW), P(fb), TAIL_MULTIPLIER, views, L, K, P(fraw), P(ftok), P(fcam),
                                            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), 'vf_pose_tail_f32')
    torch.cuda.synchronize()
    bad = {n: f.violations() for n, f in dict(x=fx, W=fW, b=fb, raw=fraw, tokens=ftok, cameras=fcam).items() if f.violations()}
    assert not bad, f'footprint violations (region, first offset, count): {bad}'
    cam, tok, raw = ops.pose_tail(x.to(dev), W.to(dev), b.to(dev), TAIL_MULTIPLIER, views, L, want_raw=True, want_tokens=True)
    assert torch.equal(fcam.logical(), cam) and torch.equal(ftok.logical().view(views, L, 7), tok) and torch.equal(fraw.logical().view(views, L, 7), raw)
    # the optional outputs withheld: the cameras alone, same bits, frames intact
    fcam2 = Frame(views, 7, 7, torch.float32, dev)
    _lib.check(_lib.load().vf_pose_tail_f32(P(fx), K + pad, P(fW), None, TAIL_MULTIPLIER, views, L, K, None, None, P(fcam2),
                                            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), 'vf_pose_tail_f32')
    torch.cuda.synchronize()
    assert not fcam2.violations() and not fx.violations() and not fW.violations()
    assert torch.equal(fcam2.logical(), ops.pose_tail(x.to(dev), W.to(dev), None, TAIL_MULTIPLIER, views, L)[0])


# ---------------------------------------------------------------------------------------------- shared model pieces
B_, C_, N_ = 2, 6, 4


def _model_cfg(**kw):
    from viewformer_amd.config import MIGTConfig
    return MIGTConfig(sequence_size=C_ + 1, n_loss_skip=1, pose_multiplier=0.2, localization_weight='1', **kw)


@pytest.fixture(scope='module')
def setup():
    from viewformer_amd import geometry
    from viewformer_amd.weights import make_migt_weights, synthetic_scene_batch
    cfg = _model_cfg()
    sd = make_migt_weights(cfg, seed=0, std=0.03)
    g = np.random.Generator(np.random.PCG64(41))
    codes = torch.from_numpy(g.integers(0, 1024, size=(B_, C_ + N_, 8, 8))).to(torch.int32)
    _, cams = synthetic_scene_batch(B_, C_ + N_, 8, 43)
    poses = geometry.normalize_cameras(geometry.to_relative_cameras(torch.from_numpy(cams))[0])
    return dict(cfg=cfg, sd=sd, ctx=codes[:, :C_].contiguous(), photos=codes[:, C_:].contiguous(), cpos=poses[:, :C_].contiguous())


def _full_route(m, ctx, photos, cpos):
    """the full pass per photo: model(dict(input_ids=[ctx, photo n], poses=ctx poses), last_view_logits_only=True) -> tokens [B,N,L,7]"""
    outs = []
    for n in range(photos.shape[1]):
        ids = torch.cat([ctx, photos[:, n:n + 1]], 1).to(m.device)
        outs.append(m(dict(input_ids=ids, poses=cpos.to(m.device)), last_view_logits_only=True)['pose_prediction'][:, -1])
    return torch.stack(outs, 1)


class _TailSpy:
    """records the rows ``ops.pose_tail`` / the unfused c_proj GEMM receive, so that E = 16 eps32 (|x| |W| + |b|) can be formed for the
    model's own activations"""

    def __init__(self, monkeypatch):
        from viewformer_amd import ops
        self.x = None
        real = ops.pose_tail

        def spy(x, *a, **k):
            self.x = x
            return real(x, *a, **k)
        monkeypatch.setattr(ops, 'pose_tail', spy)

    def E_max(self, sd):
        name = 'pose_criterion.pose_classifier.c_proj'
        W, b = torch.as_tensor(sd[name + '.weight']).double(), torch.as_tensor(sd[name + '.bias']).double().reshape(-1)
        return float((16 * EPS32 * (self.x.detach().cpu().double().abs() @ W.abs() + b.abs())).max())


def _check_cameras_against_own_raw(out, E_max, label):
    """each view's camera (and each token) within the tail's bounds of the fp64 tail applied to the route's own raw"""
    raw = out['raw'].cpu()
    B, N, L = raw.shape[:3]
    tok64, cam64, rho_tok, rho_mean = tail_from_raw_fp64(raw.view(B * N, L, 7), 0.2)
    b_tq, b_txyz, b_cq, b_cxyz = tail_bounds(E_max, float(rho_tok.min()), float(rho_mean.min()), 0.2)
    cam, tok = out['cameras'].cpu().view(B * N, 7).double(), out['pose_prediction'].cpu().view(B * N, L, 7)
    fig = dict(camera_q=float((cam[:, 3:] - cam64[:, 3:]).abs().max()), camera_xyz=float((cam[:, :3] - cam64[:, :3]).abs().max()),
               token_vs_own_raw=float(_token_distance(tok, tok64).max()), E_max=E_max, rho_tok=float(rho_tok.min()), rho_mean=float(rho_mean.min()),
               bound_camera_q=b_cq, bound_camera_xyz=b_cxyz)
    parity_report(test='localize_cameras_vs_own_raw', case=label, **fig)
    assert fig['camera_q'] <= b_cq and fig['camera_xyz'] <= b_cxyz, fig
    return fig


# ---------------------------------------------------------------------------------------------- (c) fp32 arm
def test_f32_arm_cached_localization_equals_the_full_pass_within_its_own_error(dev, setup, monkeypatch):
    """Measured on the CPU for exactly this setup (fp64 oracle, C = 6, four photos, 512 tokens): raw outputs <= 1.56, token quaternion
    norm >= 0.19, smallest |w| / ||q|| 1.9e-4, 0.4 % of the tokens below 1e-3; fp32 CPU oracle against the fp64 one 9.7e-6 in raw."""
    from oracle import migt_oracle as mg
    from viewformer_amd.migt import MIGT
    cfg, sd, ctx, photos, cpos = (setup[k] for k in ('cfg', 'sd', 'ctx', 'photos', 'cpos'))
    B, C, N = B_, C_, N_
    spy = _TailSpy(monkeypatch)
    m = MIGT(cfg).load_state_dict(sd).to(dev)
    full = _full_route(m, ctx, photos, cpos).cpu()
    cache = m.prefill_context(ctx, cpos)
    out = m.localize_from_context(cache, photos, return_tokens=True)
    assert spy.x is not None, 'the fused tail did not run'
    E_max = spy.E_max(sd)
    plain = m.localize_from_context(cache, photos)
    assert tuple(plain.shape) == (B, N, 7) and torch.equal(plain, out['cameras'])    # the cameras do not depend on the optional outputs
    cached = out['pose_prediction'].cpu()
    assert tuple(cached.shape) == (B, N, 64, 7) and tuple(out['raw'].shape) == (B, N, 64, 7)
    # fp64 oracle: scene 0, photos 0 and 1
    ref = torch.stack([mg.migt_forward(sd, cfg, torch.cat([ctx[:1], photos[:1, n:n + 1]], 1).long(), cpos[:1], dtype=torch.float64)['pose_prediction'][0, -1]
                       for n in (0, 1)])                                             # [2,L,7]
    peak = float(ref.abs().max())
    e_full = float(_token_distance(full[0, :2], ref).max())
    e_cached = float(_token_distance(cached[0, :2], ref).max())
    w_norm = full[..., 3].double().clone()                                           # sign-fixed unit quaternions: w IS |w| / ||q||
    w_norm[0, :2] = ref[..., 3]
    near = w_norm < 2 * (e_cached + e_full)
    differ = _sign_differs(cached, full)
    parity_report(test='localize_f32_arm', B=B, C=C, N=N, e_full=e_full, e_cached=e_cached, peak=peak, bit_identical=bool(torch.equal(cached, full)),
                  max_cached_vs_full=float(_token_distance(cached, full).max()), tokens=int(differ.numel()), tokens_sign_differing=int(differ.sum()),
                  tokens_near_sign_boundary=int(near.sum()), min_w_norm=float(w_norm.min()), E_max=E_max)
    assert e_cached <= 1.5 * e_full, (e_cached, e_full)
    assert e_cached < F32_TOKEN_TOL * max(1.0, peak), e_cached
    assert bool((~differ | near).all()), 'a token\'s sign differs from the full path outside the two paths\' error'
    assert float(near.float().mean()) <= NEAR_SIGN_TOKENS_MAX, float(near.float().mean())
    # cameras: against the fp64 tail of the route's own raw, and against the full route's reduction where no token sign differs
    _check_cameras_against_own_raw(out, E_max, 'f32 arm, fused tail')
    _, cam_full, _, rho_mean = tail_from_raw_fp64(_as_raw(full.view(B * N, 64, 7)), 0.2)
    stable = ~differ.view(B * N, 64).any(1)
    d_cam = (out['cameras'].cpu().view(B * N, 7).double() - cam_full).abs().amax(-1)
    bound = 2 * (e_cached + e_full) / rho_mean + 1e-6
    parity_report(test='localize_f32_arm_cameras', views=B * N, sign_stable_views=int(stable.sum()), max_camera_diff=float(d_cam[stable].max()),
                  min_bound=float(bound.min()), rho_mean=float(rho_mean.min()))
    assert bool(stable.any()) and bool((d_cam[stable] <= bound[stable]).all()), (d_cam, bound)
    # the unfused tail: both GEMMs are within E of the exact raw
    unf = m.localize_from_context(cache, photos, return_tokens=True, fused_tail=False)
    _, _, rho_tok, _ = tail_from_raw_fp64(out['raw'].cpu().view(B * N, 64, 7), 0.2)
    b_tq, b_txyz, _, _ = tail_bounds(E_max, float(rho_tok.min()), 1.0, 0.2)
    tu, tf = unf['pose_prediction'].cpu().double(), cached.double()
    dq = torch.minimum((tu[..., 3:] - tf[..., 3:]).abs().amax(-1), (tu[..., 3:] + tf[..., 3:]).abs().amax(-1))
    dxyz = (tu[..., :3] - tf[..., :3]).abs().amax(-1)
    parity_report(test='localize_f32_arm_unfused_vs_fused', token_q=float(dq.max()), token_xyz=float(dxyz.max()), bound_q=2 * b_tq, bound_xyz=2 * b_txyz,
                  raw_max_diff=float((unf['raw'] - out['raw']).abs().max()), raw_bit_identical=bool(torch.equal(unf['raw'], out['raw'])),
                  camera_max_diff=float((unf['cameras'] - out['cameras']).abs().max()))
    assert float((unf['raw'].cpu().double() - out['raw'].cpu().double()).abs().max()) <= 2 * E_max
    assert float(dq.max()) <= 2 * b_tq and float(dxyz.max()) <= 2 * b_txyz
    _check_cameras_against_own_raw(unf, E_max, 'f32 arm, unfused tail')


def test_f32_arm_a_photos_camera_does_not_depend_on_the_chunking(dev, setup):
    """The dense layers take the same kernel for row counts that are multiples of 256 (4 views) and the tail gives a view
    the same bits wherever it sits: for N and chunks that are multiples of 4 the cameras are ``torch.equal``; for other N the two
    evaluations are each within the arm's bound of the exact tokens, which moves a camera by at most twice that (over rho_mean for
    the quaternion)."""
    from viewformer_amd.migt import MIGT
    from viewformer_amd.render import ViewRenderer
    cfg, sd, ctx, photos, cpos = (setup[k] for k in ('cfg', 'sd', 'ctx', 'photos', 'cpos'))
    m = MIGT(cfg).load_state_dict(sd).to(dev)
    g = np.random.Generator(np.random.PCG64(42))
    more = torch.cat([photos, torch.from_numpy(g.integers(0, 1024, size=(B_, 4, 8, 8))).to(torch.int32)], 1)          # N = 8
    r = ViewRenderer(m, types.SimpleNamespace(device=dev))                          # (codes in, cameras out: no codebook model is run)
    r.set_context(codes=ctx, cameras=cpos)
    one = r.localize(codes=more, return_tokens=True)
    halves = r.localize(codes=more, max_views_per_call=4, return_tokens=True)
    a, b = r.localize(codes=more[:, :4]), r.localize(codes=more[:, 4:])
    for k in ('generated_cameras', 'pose_prediction', 'raw'):
        assert torch.equal(one[k], halves[k]), k
    assert torch.equal(one['generated_cameras'], torch.cat([a['generated_cameras'], b['generated_cameras']], 1))
    two = r.localize(codes=more[:, :2])['generated_cameras']                         # N = 2: other GEMM tiles, the arm's tolerance
    five = r.localize(codes=more[:, :5], max_views_per_call=4, return_tokens=True)
    peak = float(one['pose_prediction'].abs().max())
    _, _, _, rho_mean = tail_from_raw_fp64(one['raw'].cpu().view(B_ * 8, 64, 7), 0.2)
    tol_xyz = 2 * F32_TOKEN_TOL * max(1.0, peak)
    tol_q = tol_xyz / float(rho_mean.min()) + 1e-6
    fig = {}
    for label, got, n in (('five views in chunks of 4', five['generated_cameras'], 5), ('two views', two, 2)):
        d = (got - one['generated_cameras'][:, :n]).abs()
        fig[label] = dict(xyz=float(d[..., :3].max()), q=float(d[..., 3:].max()), bit_identical=bool(torch.equal(got, one['generated_cameras'][:, :n])))
        assert fig[label]['xyz'] <= tol_xyz and fig[label]['q'] <= tol_q, (fig, tol_xyz, tol_q)
    parity_report(test='localize_chunk_invariance', peak=peak, rho_mean=float(rho_mean.min()), tol_xyz=tol_xyz, tol_q=tol_q, **fig)


# ---------------------------------------------------------------------------------------------- (d) bf16 arm
def test_bf16_arm_cached_localization_against_the_full_pass_own_error(dev, setup, monkeypatch):
    """d_full = the bf16 full pass against the fp32 arm's full pass, d_cached = the cached bf16 pass against the same fp32 arm: the cache
    may not add to the arm's own error (the project has no absolute bf16 bound for this head; d_full is written to the parity report)."""
    from viewformer_amd.migt import MIGT
    cfg, sd, ctx, photos, cpos = (setup[k] for k in ('cfg', 'sd', 'ctx', 'photos', 'cpos'))
    m32 = MIGT(cfg).load_state_dict(sd).to(dev)
    f32 = _full_route(m32, ctx, photos, cpos).cpu()
    del m32
    spy = _TailSpy(monkeypatch)
    m16 = MIGT(cfg, precision='bf16').load_state_dict(sd).to(dev)
    f16 = _full_route(m16, ctx, photos, cpos).cpu()
    cache = m16.prefill_context(ctx, cpos)
    out = m16.localize_from_context(cache, photos, return_tokens=True)
    assert spy.x is not None and spy.x.dtype == torch.float32
    E_max = spy.E_max(sd)
    c16 = out['pose_prediction'].cpu()
    d_full, d_cached = _token_distance(f16, f32), _token_distance(c16, f32)
    fig = dict(d_full_max=float(d_full.max()), d_cached_max=float(d_cached.max()), d_full_rms=float(d_full.pow(2).mean().sqrt()),
               d_cached_rms=float(d_cached.pow(2).mean().sqrt()), cached_vs_full_bf16_max=float(_token_distance(c16, f16).max()),
               bit_identical=bool(torch.equal(c16, f16)), peak=float(f32.abs().max()),
               tokens_sign_differing_from_f32=int(_sign_differs(c16, f32).sum()), tokens=int(d_full.numel()))
    parity_report(test='localize_bf16_arm', B=B_, C=C_, N=N_, **fig)
    assert fig['d_cached_max'] <= 1.5 * fig['d_full_max'], fig
    assert fig['d_cached_rms'] <= 1.1 * fig['d_full_rms'], fig
    _check_cameras_against_own_raw(out, E_max, 'bf16 arm, fused tail')


# ---------------------------------------------------------------------------------------------- (e) end to end
class _CountingEncoder:
    def __init__(self, model):
        self.model, self.calls, self._encode = model, 0, model.encode

    def __enter__(self):
        def encode(x):
            self.calls += 1
            return self._encode(x)
        self.model.encode = encode
        return self

    def __exit__(self, *exc):
        del self.model.encode
        return False


def _compare_end_to_end(label, got, want, B, N):
    """(c)'s rules without an oracle: the two routes are each within the arm's 1e-3 of the exact tokens, a token's sign may differ only
    where the full route's normalised |w| is inside twice their distance, and such tokens are at most 2 %"""
    L = got['pose_prediction'].shape[2]
    assert torch.equal(got['codes'].reshape(B * N, 8, 8).cpu(), want['codes'][:, -1].cpu())
    tg, tw = got['pose_prediction'].reshape(B * N, L, 7).cpu(), want['pose_last'].reshape(B * N, L, 7).cpu()
    dist = _token_distance(tg, tw)
    d, peak = float(dist.max()), float(tw.abs().max())
    differ = _sign_differs(tg, tw)
    near = tw[..., 3].double() < 2 * d
    _, _, _, rho_mean = tail_from_raw_fp64(_as_raw(tw), 0.2)
    stable = ~differ.any(1)
    d_cam = (got['generated_cameras'].reshape(B * N, 7).cpu().double() - want['generated_cameras'].cpu().double()).abs().amax(-1)
    bound = 2 * F32_TOKEN_TOL * max(1.0, peak) / rho_mean
    fig = dict(token_distance_max=d, peak=peak, bit_identical=bool(torch.equal(tg, tw)), tokens=int(differ.numel()), tokens_sign_differing=int(differ.sum()),
               tokens_near_sign_boundary=int(near.sum()), sign_stable_views=int(stable.sum()), views=B * N,
               camera_diff_max_stable=float(d_cam[stable].max()) if bool(stable.any()) else None, camera_bound_min=float(bound.min()),
               cameras_bit_identical=bool(torch.equal(got['generated_cameras'].reshape(B * N, 7).cpu(), want['generated_cameras'].cpu())))
    parity_report(test='localize_end_to_end', case=label, B=B, N=N, **fig)
    assert d < 2 * F32_TOKEN_TOL * max(1.0, peak), fig
    assert bool((~differ | near).all()) and float(near.float().mean()) <= NEAR_SIGN_TOKENS_MAX, fig
    assert bool(stable.any()) and bool((d_cam[stable] <= bound[stable]).all()), fig
    return fig


@pytest.mark.parametrize('augment', ['relative', 'no'])
def test_localize_equals_the_evaluator_on_replicated_contexts_f32(dev, full_vq, augment):
    from viewformer_amd.evaluate import generate_batch_predictions
    from viewformer_amd.migt import MIGT
    from viewformer_amd.render import ViewRenderer, localize_views
    from viewformer_amd.scene_bank import SceneBank
    from viewformer_amd.vqgan import VQGAN
    from viewformer_amd.weights import make_migt_weights, synthetic_scene_batch
    vcfg, vsd, _ = full_vq
    B, C, N = B_, C_, N_
    cfg = _model_cfg(augment_poses=augment)
    tr_m = MIGT(cfg).load_state_dict(make_migt_weights(cfg, seed=0, std=0.03)).to(dev)
    vq_m = VQGAN(vcfg, data_format='NHWC', conv_arith='x3h').load_state_dict(vsd).to(dev)
    frames, cams = synthetic_scene_batch(B, C + N, 128, seed=51)
    frames, cams = torch.from_numpy(frames), torch.from_numpy(cams)
    ctx_f, ctx_c, photos = frames[:, :C], cams[:, :C], frames[:, C:]
    # the evaluator on the B * N replicated scenes whose last frame is the photo (its camera there is not read by the localization)
    img = torch.cat([ctx_f[:, None].expand(B, N, C, *frames.shape[2:]), photos[:, :, None]], 2).reshape(B * N, C + 1, *frames.shape[2:])
    cam = torch.cat([ctx_c[:, None].expand(B, N, C, 7), cams[:, C:, None]], 2).reshape(B * N, C + 1, 7)
    want = generate_batch_predictions(tr_m, vq_m, img.to(dev), cam.to(dev), return_codes=True)
    got_host = localize_views(tr_m, vq_m, ctx_f, ctx_c, photos, return_tokens=True)                  # host inputs, one call
    assert tuple(got_host['generated_cameras'].shape) == (B, N, 7)
    _compare_end_to_end(f'{augment}/host', got_host, want, B, N)
    with _CountingEncoder(vq_m) as enc:                                              # device inputs through the object, the encoder counted
        r = ViewRenderer(tr_m, vq_m).set_context(images=ctx_f.to(dev), cameras=ctx_c.to(dev))
        assert enc.calls == 1
        first = r.localize(images=photos[:, :2].to(dev), return_tokens=True)
        second = r.localize(images=photos[:, 2:].to(dev), return_tokens=True)
        assert enc.calls == 3, enc.calls                                             # one encoder call per localize call
        plain = r.localize(images=photos[:, 2:].to(dev))
        assert enc.calls == 4
        pictures = r.render(cams[:, C:C + 2].to(dev))                                # the same context serves the renderer: no encoder call
        assert enc.calls == 4, enc.calls
    assert tuple(pictures['generated_images'].shape) == (B, 2, 128, 128, 3)
    assert set(plain) == {'generated_cameras'} and torch.equal(plain['generated_cameras'], second['generated_cameras'])
    got_dev = {k: torch.cat([first[k], second[k]], 1) for k in first}
    _compare_end_to_end(f'{augment}/device,two calls', got_dev, want, B, N)
    # the photos' codes from a scene bank instead of their pixels
    bank = SceneBank(vq_m, frames.reshape(B * (C + N), 128, 128, 3), cams.reshape(B * (C + N), 7), batch_size=16)
    idx = torch.tensor([[b * (C + N) + C + n for n in range(N)] for b in range(B)])
    bank_codes, _ = bank.gather(idx)
    with _CountingEncoder(vq_m) as enc:
        from_bank = r.localize(codes=bank_codes, return_tokens=True)
        assert enc.calls == 0
    for k in ('generated_cameras', 'codes', 'pose_prediction', 'raw'):
        assert torch.equal(from_bank[k], got_host[k]), k
    empty = r.localize(images=photos[:, :0])
    assert torch.equal(empty['generated_cameras'], torch.empty((B, 0, 7), dtype=torch.float32, device=dev))
    empty = r.localize(codes=bank_codes[:, :0], return_tokens=True)
    assert tuple(empty['pose_prediction'].shape) == (B, 0, 64, 7) and tuple(empty['raw'].shape) == (B, 0, 64, 7) and tuple(empty['codes'].shape) == (B, 0, 8, 8)


# ---------------------------------------------------------------------------------------------- (f) refusals
def test_unsupported_models_arms_inputs_and_foreign_caches_are_refused(dev):
    from viewformer_amd import _lib
    from viewformer_amd.config import MIGTConfig
    from viewformer_amd.migt import MIGT
    from viewformer_amd.weights import make_migt_weights
    cfg = MIGTConfig(sequence_size=3, n_loss_skip=1, pose_multiplier=0.2, localization_weight='1', n_layer=2)
    sd = make_migt_weights(cfg, seed=0)
    codes = torch.zeros((2, 2, 8, 8), dtype=torch.int32)
    photos = torch.ones((2, 3, 8, 8), dtype=torch.int32)
    cpos = torch.tensor([0.0, 0, 0, 1, 0, 0, 0]).expand(2, 2, 7).contiguous()
    a = MIGT(cfg).load_state_dict(sd).to(dev)
    cache = a.prefill_context(codes, cpos)
    assert tuple(a.localize_from_context(cache, photos).shape) == (2, 3, 7)
    noloc = MIGTConfig(sequence_size=3, n_loss_skip=1, pose_multiplier=0.2, localization_weight='0', n_layer=2)
    assert not noloc.use_localization
    with pytest.raises(RuntimeError, match='localization head'):
        MIGT(noloc).load_state_dict(make_migt_weights(noloc, seed=0)).to(dev).localize_from_context(cache, photos)
    with pytest.raises(_lib.VfError):                                                # no fp8 arm of the prefix attention, and no fallback
        MIGT(cfg, precision='bf16', attention='fp8').load_state_dict(sd).to(dev).localize_from_context(cache, photos)
    with pytest.raises(ValueError):
        a.localize_from_context(cache, photos[:1])                                   # another batch size
    with pytest.raises(ValueError):
        a.localize_from_context(cache, torch.ones((2, 3, 4, 4), dtype=torch.int32))  # another token map
    with pytest.raises(ValueError):
        a.localize_from_context(cache, photos.float())                               # codes are integers
    with pytest.raises(TypeError):
        a.localize_from_context(dict(kv=cache.kv), photos)                           # not a cache
    with pytest.raises(TypeError):
        a.localize_from_context(None, photos)
    b = MIGT(cfg).load_state_dict(sd).to(dev)
    with pytest.raises(ValueError):
        b.localize_from_context(cache, photos)                                       # a cache of another model object
    a.load_state_dict(sd)                                                            # new weights: the cache is stale
    with pytest.raises(ValueError):
        a.localize_from_context(cache, photos)
    out = a.localize_from_context(a.prefill_context(codes, cpos), photos[:, :0], return_tokens=True)
    assert tuple(out['cameras'].shape) == (2, 0, 7) and tuple(out['pose_prediction'].shape) == (2, 0, 64, 7) and tuple(out['raw'].shape) == (2, 0, 64, 7)
