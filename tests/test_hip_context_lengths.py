"""GPU: a context length per query view and per scene for a cached context (csrc/attention_prefix.hip's
``vf_attn_prefix_var_*``, ``ops.attn_prefix(ctx_len=...)``, ``MIGT.*_from_context(n_context=...)``, ``ViewRenderer`` and
``render.evaluate_context_sizes``).

The first c views of a C-view cache ARE the cache of those c views, so everything here is checked against code that existed before: the
fixed-C kernels with C = c on the same buffers (bit for bit), the fp64 attention with the keys beyond a view's length removed, the model
with one length for all views, the multi-context evaluator's three-stream full pass and the fp64 oracle.  Every measured figure goes
through ``conftest.parity_report``."""
import numpy as np
import pytest
import torch

from conftest import parity_report
from context_lengths_ref import KERNEL_ARMS, KERNEL_CASES, L, attn_fp64_lengths, case_id, rand
from framed import Frame
from test_localize_host import tail_from_raw_fp64

pytestmark = pytest.mark.gpu

F32_LOGIT_TOL = 1e-3            # fp32 arm against fp64, times max(1, peak): the project's bound (tests/test_hip_parity_scale.py)
F32_TOKEN_TOL = 1e-3            # the same bound for the pose tokens (tests/test_hip_localize.py)
NEAR_SIGN_TOKENS_MAX = 0.02     # tokens whose normalised |w| lies inside the two routes' own error: at most 2 % of all (tests/test_hip_localize.py)
NEAR_TIE_ROWS_MAX = 0.02        # fp32 arm: rows inside the two paths' own error may be at most 2 % of all rows (a condition of the setup)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'needs the MI355X'
    return torch.device('cuda:0')


# ---------------------------------------------------------------------------------------------- (a), (b) the kernel
def _frames(dev, arm, B, H, C, N, lengths, seed=0, poison=None):
    """(q rows, cache frame, its scene-0 window, out frame, lengths frame): the cache with ldkp != ldk and a gap between the scenes"""
    d = H * 64
    dt = torch.bfloat16 if arm == 'bf16' else torch.float32
    ctx = rand((B, C * L, 3 * d), 100 + C + seed, 0.35).to(dt)
    if poison is not None:                                           # views >= poison[b] of scene b are NaN
        for b in range(B):
            ctx[b, poison[b] * L:] = float('nan')
    q = rand((B * N * L, 3 * d), 200 + N + seed, 0.35).to(dev).to(dt)
    ldp = 3 * d + 16
    fc = Frame(C * L, 3 * d, ldp, dt, dev, batch=B, batch_stride=C * L * ldp + 64).load(ctx if B > 1 else ctx[0])
    fo = Frame(B * N * L, d, d + 8, dt, dev)
    fl = Frame.raw(B * N * 4, dev, dtype=torch.int32).load(torch.as_tensor(lengths, dtype=torch.int32).reshape(-1))
    return q, ctx.to(dev), fc, (fc.view[0] if B > 1 else fc.view), fo, fl


def _launch(arm, q, c0, fc, out, B, H, C, N, ctx_len=None):
    from viewformer_amd import ops
    d = H * 64
    ops.attn_prefix(q[:, d:2 * d], q[:, 2 * d:], q[:, :d], c0[:, 2 * d:], c0[:, :d], out, B, H, C, N, L, 3 * d, 3 * d, 3 * d, fc.ld, fc.ld,
                    fc.batch_stride, out.stride(0), bf16=arm != 'f32eq', ctx_len=ctx_len)
    return out


@pytest.mark.parametrize('arm', KERNEL_ARMS)
@pytest.mark.parametrize('case', KERNEL_CASES, ids=case_id)
def test_a_view_of_length_c_gets_the_bits_of_the_fixed_kernel_with_C_equal_c(dev, arm, case):
    """For every distinct c >= 1 the existing entry runs with C = c and the full cache's prefix_stride over all N views; the rows of the
    views whose length is c must be ``torch.equal``.  Length-0 views are compared with the block-causal kernel on single-view sequences
    (another kernel: only the error criterion).  Error criterion over all views: max / rms error against fp64 at most 1.5x / 1.1x that of
    the existing kernels' rows assembled this way, both measured here — the margins of tests/test_hip_render.py, for the noise of a
    sample maximum between two evaluations that may sum in different orders, not for a looser kernel."""
    from viewformer_amd import ops
    (B, H, C, N), lengths = case
    d = H * 64
    dt = torch.bfloat16 if arm == 'bf16' else torch.float32
    lens = np.asarray(lengths).reshape(B, N)
    q, ctx, fc, c0, fo, fl = _frames(dev, arm, B, H, C, N, lens)
    ref = attn_fp64_lengths(ctx.view(B * C * L, 3 * d), q, B, H, C, N, lens)
    out = _launch(arm, q, c0, fc, fo.view, B, H, C, N, ctx_len=fl.view)
    torch.cuda.synchronize()
    assert fo.violations() == [] and fl.violations() == [] and fc.violations() == []          # writes exactly the logical output elements
    out = fo.logical()
    assert not torch.isnan(out.float()).any()
    view_len = torch.from_numpy(lens.reshape(-1))
    rows = lambda mask: mask.repeat_interleave(L).to(dev)
    old = torch.full((B * N * L, d), float('nan'), dtype=dt, device=dev)
    for c in sorted(set(lens.reshape(-1).tolist()) - {0}):
        fixed = _launch(arm, q, c0, fc, torch.full((B * N * L, d), float('nan'), dtype=dt, device=dev), B, H, c, N)
        sel = rows(view_len == c)
        assert torch.equal(out[sel], fixed[sel]), f'length {c}: not the bits of the fixed kernel with C = {c}'
        old[sel] = fixed[sel]
    if (view_len == 0).any():                                        # a view that sees only itself: a one-view block-causal sequence
        alone = torch.full((B * N * L, d), float('nan'), dtype=dt, device=dev)
        ops.attn_blockcausal(q[:, d:2 * d], q[:, 2 * d:], q[:, :d], alone, B * N, H, L, L, 3 * d, 3 * d, 3 * d, d, 1.0, True, -1,
                             bf16=arm != 'f32eq', x6=arm == 'f32eq')
        sel = rows(view_len == 0)
        old[sel] = alone[sel]
        zero_identical = bool(torch.equal(out[sel], alone[sel]))
    else:
        zero_identical = None
    assert not torch.isnan(old.float()).any()
    e_new, e_old = (out.double().cpu() - ref).abs(), (old.double().cpu() - ref).abs()
    fig = dict(max_new=e_new.max().item(), max_old=e_old.max().item(), rms_new=e_new.pow(2).mean().sqrt().item(),
               rms_old=e_old.pow(2).mean().sqrt().item(), length_0_views_bit_identical_to_blockcausal=zero_identical)
    parity_report(test='context_lengths_kernel', arm=arm, B=B, H=H, C=C, N=N, lengths=lens.tolist(), **fig)
    assert fig['max_new'] <= 1.5 * fig['max_old'], fig
    assert fig['rms_new'] <= 1.1 * fig['rms_old'], fig
    # independence: view 0 of every scene launched alone with its length gives its rows of the full launch
    q1 = q.view(B, N, L, 3 * d)[:, :1].reshape(B * L, 3 * d).contiguous()
    l1 = torch.from_numpy(lens[:, :1].astype(np.int32).reshape(-1).copy()).to(dev)
    one = _launch(arm, q1, c0, fc, torch.full((B * L, d), float('nan'), dtype=dt, device=dev), B, H, C, 1, ctx_len=l1)
    assert torch.equal(one.view(B, L, d), out.view(B, N, L, d)[:, 0])


@pytest.mark.parametrize('arm', KERNEL_ARMS)
@pytest.mark.parametrize('per_scene', [[2, 0], [1, 2]])
def test_cache_rows_beyond_a_scenes_length_are_not_used(dev, arm, per_scene):
    """all views of scene b have one length c_b < C; cache views >= c_b are NaN: no NaN in the output, the bits of the clean cache"""
    B, H, C, N = 2, 2, 3, 5
    lens = np.repeat(np.asarray(per_scene).reshape(B, 1), N, 1)
    q, _, fc, c0, fo, fl = _frames(dev, arm, B, H, C, N, lens)
    clean = _launch(arm, q, c0, fc, fo.view, B, H, C, N, ctx_len=fl.view).clone()
    q2, _, fc2, c02, fo2, fl2 = _frames(dev, arm, B, H, C, N, lens, poison=per_scene)
    assert torch.equal(q, q2) and torch.isnan(fc2.view[1, per_scene[1] * L:].float()).all()
    out = _launch(arm, q2, c02, fc2, fo2.view, B, H, C, N, ctx_len=fl2.view)
    torch.cuda.synchronize()
    assert fo2.violations() == [] and fc2.violations() == []
    assert not torch.isnan(out.float()).any()
    assert torch.equal(out, clean)


@pytest.mark.parametrize('arm', KERNEL_ARMS)
def test_a_nan_tile_staged_for_a_longer_neighbour_does_not_reach_a_shorter_view(dev, arm):
    """a mixed group: lengths [1, 3, 0, 2, 3] with cache views >= 1 NaN.  The groups of views 0 and 2 stage the NaN tiles for their
    longer neighbours (bf16 arms: one group of four; f32eq: the pairs (0, 1) and (2, 3)); views 0 and 2 must skip them: no NaN, the
    bits of the clean cache.  The other views read NaN and are not looked at."""
    B, H, C, N = 1, 2, 3, 5
    lens = np.asarray([[1, 3, 0, 2, 3]])
    d = H * 64
    q, _, fc, c0, fo, fl = _frames(dev, arm, B, H, C, N, lens)
    clean = _launch(arm, q, c0, fc, fo.view, B, H, C, N, ctx_len=fl.view).clone().view(N, L, d)
    q2, _, fc2, c02, fo2, fl2 = _frames(dev, arm, B, H, C, N, lens, poison=[1])
    assert torch.equal(q, q2) and torch.isnan(fc2.view[L:].float()).all() and not torch.isnan(fc2.view[:L].float()).any()
    out = _launch(arm, q2, c02, fc2, fo2.view, B, H, C, N, ctx_len=fl2.view).view(N, L, d)
    torch.cuda.synchronize()
    assert fo2.violations() == [] and fc2.violations() == []
    for n in (0, 2):
        assert not torch.isnan(out[n].float()).any(), n
        assert torch.equal(out[n], clean[n]), n
    assert torch.isnan(out[1].float()).any() and torch.isnan(out[4].float()).any()     # (the poison is where the longer views read)


# ---------------------------------------------------------------------------------------------- shared model pieces
B_, C_, N_ = 2, 6, 8
MIXED = [[0, 6, 1, 6, 3, 3, 2, 5], [6, 6, 0, 0, 4, 1, 2, 2]]          # every length 0 ... 6; mixed and homogeneous groups of both arms
_models = {}


def _cfg(C=C_, **kw):
    from viewformer_amd.config import MIGTConfig
    return MIGTConfig(sequence_size=C + 1, n_loss_skip=1, pose_multiplier=0.2, localization_weight='1', **kw)


def _poses(B, C, N, seed):
    from viewformer_amd import geometry
    from viewformer_amd.weights import synthetic_scene_batch
    _, cams = synthetic_scene_batch(B, C + N, 8, seed)
    p = geometry.normalize_cameras(geometry.to_relative_cameras(torch.from_numpy(cams))[0])
    return p[:, :C].contiguous(), p[:, C:].contiguous()


def _model(dev, arm):
    """full-size model, B = 2, C = 6, N = 8 (every row count a multiple of 256: the dense layers take one kernel whatever the call)"""
    if arm not in _models:
        from viewformer_amd.migt import MIGT
        from viewformer_amd.weights import make_migt_weights, synthetic_scene_batch
        cfg = _cfg()
        m = MIGT(cfg, precision=arm).load_state_dict(make_migt_weights(cfg, seed=0, std=0.03 if arm == 'f32' else 0.02)).to(dev)
        g = np.random.Generator(np.random.PCG64(141))
        codes = torch.from_numpy(g.integers(0, cfg.n_embeddings, size=(B_, C_ + N_, 8, 8))).to(torch.int32)
        cpos, qpos = _poses(B_, C_, N_, 143)
        _, cams = synthetic_scene_batch(B_, C_ + N_, 8, seed=144)
        _models[arm] = dict(cfg=cfg, m=m, ctx=codes[:, :C_].contiguous(), photos=codes[:, C_:].contiguous(), cpos=cpos, qpos=qpos,
                            cache=m.prefill_context(codes[:, :C_], cpos), cams=torch.from_numpy(cams))
    return _models[arm]


@pytest.fixture(scope='module')
def vq_m(dev, full_vq):
    from viewformer_amd.vqgan import VQGAN
    vcfg, vsd, _ = full_vq
    return VQGAN(vcfg, data_format='NHWC', conv_arith='x3h').load_state_dict(vsd).to(dev)


def _margin(lg):
    top2 = torch.topk(lg, 2, dim=-1).values
    return top2[..., 0] - top2[..., 1]


def _token_distance(a, b):
    """per token: max(|d xyz|, min(|q - q'|, |q + q'|)) (max norm over components), as tests/test_hip_localize.py"""
    a, b = a.double(), b.double()
    dx = (a[..., :3] - b[..., :3]).abs().amax(-1)
    dq = torch.minimum((a[..., 3:] - b[..., 3:]).abs().amax(-1), (a[..., 3:] + b[..., 3:]).abs().amax(-1))
    return torch.maximum(dx, dq)


def _sign_differs(a, b):
    a, b = a.double(), b.double()
    return (a[..., 3:] + b[..., 3:]).abs().amax(-1) < (a[..., 3:] - b[..., 3:]).abs().amax(-1)


# ---------------------------------------------------------------------------------------------- (c) the model, both arms
@pytest.mark.parametrize('arm', ['f32', 'bf16'])
def test_no_lengths_is_the_full_capacity_and_the_call_without_the_keyword(dev, arm):
    s = _model(dev, arm)
    m, cache, qpos = s['m'], s['cache'], s['qpos']
    none = m.generate_from_context(cache, qpos, codes_only=False, n_context=None)
    assert torch.equal(none, m.generate_from_context(cache, qpos, codes_only=False))
    for full in (C_, [C_] * B_, np.full((B_, N_), C_), torch.full((B_, N_), C_, device=dev)):
        assert torch.equal(none, m.generate_from_context(cache, qpos, codes_only=False, n_context=full))


@pytest.mark.parametrize('arm', ['f32', 'bf16'])
def test_every_views_result_is_that_of_its_length_given_to_all_views(dev, arm):
    """mixed lengths against the uniform call per length: logits (generate), cameras and tokens (localize), token_log_prob (score);
    and sampling with top_k = 1 is the arg-max of those logits"""
    s = _model(dev, arm)
    m, cache, qpos, photos = s['m'], s['cache'], s['qpos'], s['photos']
    lens = torch.tensor(MIXED)
    lg = m.generate_from_context(cache, qpos, codes_only=False, n_context=MIXED)
    gen = m.generate_from_context(cache, qpos, codes_only=True, n_context=MIXED)
    loc = m.localize_from_context(cache, photos, return_tokens=True, n_context=MIXED)
    sc = m.score_from_context(cache, qpos, photos, n_context=MIXED)
    smp = m.sample_from_context(cache, qpos, n_samples=2, top_k=1, seed=5, n_context=MIXED)
    assert torch.equal(gen, lg.argmax(-1))
    assert torch.equal(smp['codes'], gen[:, :, None].expand(B_, N_, 2, 8, 8))
    full_lg = m.generate_from_context(cache, qpos, codes_only=False)
    differs_from_full = 0
    for c in range(C_ + 1):
        sel = (lens == c).to(dev)
        assert bool(sel.any())
        u_lg = m.generate_from_context(cache, qpos, codes_only=False, n_context=c)
        u_loc = m.localize_from_context(cache, photos, return_tokens=True, n_context=[c] * B_)
        u_sc = m.score_from_context(cache, qpos, photos, n_context=np.full((B_, N_), c))
        assert torch.equal(lg[sel], u_lg[sel]), c
        assert torch.equal(loc['cameras'][sel], u_loc['cameras'][sel]) and torch.equal(loc['pose_prediction'][sel], u_loc['pose_prediction'][sel]), c
        assert torch.equal(sc['token_log_prob'][sel], u_sc['token_log_prob'][sel]) and torch.equal(sc['log_likelihood'][sel], u_sc['log_likelihood'][sel]), c
        if c < C_:
            differs_from_full += int(not torch.equal(u_lg, full_lg))
    assert differs_from_full == C_                                   # (the length is not ignored)
    parity_report(test='context_lengths_model_mixed_equals_uniform', arm=arm, B=B_, C=C_, N=N_, lengths=MIXED, bit_identical=True)


# ---------------------------------------------------------------------------------------------- (d) f32 arm: the full pass and the fp64 oracle
@pytest.mark.parametrize('augment', ['relative', 'no'])
def test_f32_arm_context_sizes_equal_the_multictx_full_pass_within_their_own_error(dev, vq_m, augment):
    """``evaluate_context_sizes`` against ``evaluate_multictx.generate_batch_predictions`` (the three-stream full pass) at B = 2, S = 4,
    scene 0 against the fp64 oracle.  Criteria of tests/test_hip_render.py (logits, codes, images): e_cached <= 1.5 e_full, e_cached <
    1e-3 max(1, peak), a code differs from the full pass only where the margin is below 2 (e_cached + e_full), images equal wherever
    the code maps agree, near-tie rows (margin inside the two paths' MEASURED error) at most 2 %.  Criteria of tests/test_hip_localize.py
    (pose): the same two bounds on the token distance; a token's quaternion sign differs from the full pass only where |w| / ||q|| <
    2 (e_cached + e_full), such tokens at most 2 %; on views without a differing sign the cameras (the context's frame, where both
    routes reduce their tokens) are within 2 (e_cached + e_full) / rho_mean + 1e-6 of the fp64 reduction of the full pass's tokens.
    Both routes' cameras in that frame are tied to the two functions' ``generated_cameras`` bit for bit (the same frame change on
    each), and against the evaluator's own fp32 reduction the bound grows by that reduction's measured distance from the fp64 one.
    On the CPU, for exactly these seeds, the fp64 oracle's own share of scene 0's 256 rows with margin < 4e-3 max(1, peak) — the width
    the near-tie band would have if both paths sat at the arm's bound — is 6.3 % ('relative', peak 3.54) and 3.9 % ('no', peak 3.57),
    NOT under the 2 % cap.  It is a property of a random-weight head, not of a seed: the top-2 gap of 1024 near-Gaussian logits is
    about exponential with mean 0.08 peak, so about 5 % of rows lie below 4e-3 peak.  The cap is therefore met only
    at the measured errors (1e-5 here), which is what the assertion below states, as in tests/test_hip_render.py."""
    from oracle import migt_oracle as mg
    from viewformer_amd import evaluate_multictx, geometry
    from viewformer_amd.migt import MIGT
    from viewformer_amd.render import ViewRenderer, evaluate_context_sizes
    from viewformer_amd.weights import make_migt_weights, synthetic_scene_batch
    B, S = 2, 4
    cfg = _cfg(C=S - 1, augment_poses=augment)
    sd = make_migt_weights(cfg, seed=0, std=0.03)
    m = MIGT(cfg).load_state_dict(sd).to(dev)
    frames, cams = synthetic_scene_batch(B, S, 128, seed=81)
    frames, cams = torch.from_numpy(frames), torch.from_numpy(cams)
    want = evaluate_multictx.generate_batch_predictions(m, vq_m, frames, cams)
    got = evaluate_context_sizes(m, vq_m, frames, cams)
    assert set(got) == set(want)
    for k in want:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, k
    for k in ('codes', 'ground_truth_images', 'ground_truth_cameras'):
        assert torch.equal(got[k], want[k]), k
    codes = got['codes']
    # both routes again, for their logits and pose tokens
    poses = cams.to(dev)
    transform = None
    if augment == 'relative':
        poses, transform = geometry.to_relative_cameras(poses)
    poses = geometry.normalize_cameras(poses)
    ids = torch.cat([codes[:, :-1], torch.full_like(codes[:, :1], m.mask_token)], 1)
    ctx_poses = torch.cat([poses[:, :-1], torch.zeros_like(poses[:, :1])], 1)
    target = codes[:, -1:].expand(B, S, 8, 8).contiguous()
    full = m(dict(input_ids=ids, poses=ctx_poses, localization_tokens=target, output_poses=poses[:, -1:].expand(B, S, 7).contiguous()))
    r = ViewRenderer(m, vq_m).set_context(codes=codes[:, :-1], cameras=cams[:, :-1])
    swp = r.sweep(cams[:, -1:], return_codes=True)
    assert swp['sizes'].tolist() == list(range(S)) and tuple(swp['logits'].shape) == (B, 1, S, 8, 8, cfg.n_embeddings)
    assert torch.equal(swp['generated_codes'][:, 0], got['generated_codes']) and torch.equal(swp['generated_images'][:, 0], got['generated_images'])
    loc = m.localize_from_context(r.cache, target, return_tokens=True, n_context=np.arange(S).reshape(1, S).repeat(B, 0))
    cam_world = geometry.from_relative_cameras(loc['cameras'], transform) if transform is not None else loc['cameras']
    assert torch.equal(cam_world, got['generated_cameras'])
    cam_eval = m.reduce_cameras(full['pose_prediction'], -2)                                              # the evaluator's reduction, [B,S,7]
    assert torch.equal(geometry.from_relative_cameras(cam_eval, transform) if transform is not None else cam_eval, want['generated_cameras'])
    l_full, l_cached = full['logits'].cpu().double(), swp['logits'][:, 0].cpu().double()
    p_full, p_cached = full['pose_prediction'].cpu().double(), loc['pose_prediction'].cpu().double()
    # fp64 oracle, scene 0
    ref = mg.migt_forward(sd, cfg, ids[:1].cpu().long(), ctx_poses[:1].cpu(), localization_tokens=target[:1].cpu().long(),
                          output_poses=poses[:1, -1:].expand(1, S, 7).cpu(), dtype=torch.float64)
    l_ref, p_ref = ref['logits'][0], ref['pose_prediction'][0]
    peak = float(l_ref.abs().max())
    e_full, e_cached = float((l_full[0] - l_ref).abs().max()), float((l_cached[0] - l_ref).abs().max())
    marg = _margin(l_full)
    marg[0] = _margin(l_ref)
    near = marg < 2 * (e_cached + e_full)
    differ = l_cached.argmax(-1) != l_full.argmax(-1)
    same_map = ~(got['generated_codes'] != want['generated_codes']).flatten(2).any(-1)                    # [B,S]
    img_equal = bool(torch.equal(got['generated_images'][same_map], want['generated_images'][same_map]))
    t_peak = float(p_ref.abs().max())
    t_full, t_cached = float(_token_distance(p_full[0], p_ref).max()), float(_token_distance(p_cached[0], p_ref).max())
    d_cam = (got['generated_cameras'] - want['generated_cameras']).abs()
    # pose: quaternion signs and cameras, tests/test_hip_localize.py's criteria over all B * S views
    w_norm = p_full[..., 3].clone()                                                  # sign-fixed unit quaternions: w IS |w| / ||q||
    w_norm[0] = p_ref[..., 3]
    t_near = w_norm < 2 * (t_cached + t_full)
    t_differ = _sign_differs(p_cached, p_full)
    raw_full = p_full.view(B * S, 64, 7) * torch.tensor([cfg.pose_multiplier] * 3 + [1.0] * 4, dtype=torch.float64)
    _, cam64, _, rho_mean = tail_from_raw_fp64(raw_full, cfg.pose_multiplier)       # the fp64 reduction of the full pass's tokens
    stable = ~t_differ.view(B * S, 64).any(1)
    cam_c, cam_e = loc['cameras'].cpu().view(B * S, 7).double(), cam_eval.cpu().view(B * S, 7).double()
    d_cam64, d_cam_eval, r_eval = ((x - y).abs().amax(-1) for x, y in ((cam_c, cam64), (cam_c, cam_e), (cam_e, cam64)))
    cam_bound = 2 * (t_cached + t_full) / rho_mean + 1e-6
    fig_pose = dict(tokens=int(t_differ.numel()), tokens_sign_differing=int(t_differ.sum()), tokens_near_sign_boundary=int(t_near.sum()),
                    min_w_norm=float(w_norm.min()), sign_stable_views=int(stable.sum()), views=B * S, rho_mean=float(rho_mean.min()),
                    camera_vs_fp64_of_full=float(d_cam64[stable].max()) if bool(stable.any()) else None,
                    camera_vs_evaluator=float(d_cam_eval[stable].max()) if bool(stable.any()) else None,
                    evaluator_vs_fp64_of_full=float(r_eval.max()), min_camera_bound=float(cam_bound.min()))
    parity_report(test='context_sizes_f32_arm_pose', augment=augment, B=B, S=S, **fig_pose)
    fig = dict(e_full=e_full, e_cached=e_cached, peak=peak, bit_identical=bool(torch.equal(l_cached, l_full)),
               max_cached_vs_full=float((l_cached - l_full).abs().max()), rows=int(differ.numel()), rows_differing=int(differ.sum()),
               rows_near_tie=int(near.sum()), min_margin=float(marg.min()), whole_maps_agreeing=int(same_map.sum()), maps=B * S,
               images_equal_where_maps_agree=img_equal, token_e_full=t_full, token_e_cached=t_cached, token_peak=t_peak,
               tokens_bit_identical=bool(torch.equal(p_cached, p_full)), camera_max_diff_xyz=float(d_cam[..., :3].max()),
               camera_max_diff_q=float(d_cam[..., 3:].max()))
    parity_report(test='context_sizes_f32_arm', augment=augment, B=B, S=S, **fig)
    assert e_cached <= 1.5 * e_full, fig
    assert e_cached < F32_LOGIT_TOL * max(1.0, peak), fig
    assert bool((~differ | near).all()), 'a generated code differs from the full pass outside the two paths\' error'
    assert float(near.float().mean()) <= NEAR_TIE_ROWS_MAX, fig
    assert torch.equal(got['generated_codes'].cpu(), l_cached.argmax(-1))
    assert img_equal, fig
    assert t_cached <= 1.5 * t_full, fig
    assert t_cached < F32_TOKEN_TOL * max(1.0, t_peak), fig
    assert bool((~t_differ | t_near).all()), 'a token\'s sign differs from the full pass outside the two paths\' error'
    assert float(t_near.float().mean()) <= NEAR_SIGN_TOKENS_MAX, fig_pose
    assert bool(stable.any()) and bool((d_cam64[stable] <= cam_bound[stable]).all()), (fig_pose, d_cam64, cam_bound)
    assert bool((d_cam_eval[stable] <= (cam_bound + r_eval)[stable]).all()), (fig_pose, d_cam_eval, cam_bound, r_eval)


# ---------------------------------------------------------------------------------------------- (e) a ragged batch, f32 arm
def test_f32_arm_a_ragged_batch_never_reads_its_padding_views(dev, vq_m):
    """B = 2, C = 6, scene 0 has 2 valid views: its results are ``torch.equal`` under a change of its padding views' codes and cameras,
    and within (d)'s bound, F32_LOGIT_TOL max(1, peak), of a renderer whose context is its two views alone: logits, token
    log-probabilities (peak: of the logits) and pose tokens (F32_TOKEN_TOL, the same figure, times max(1, peak of the tokens)).  Whether
    the two are bit-identical is recorded, not asserted (the prefill's row count differs)."""
    from viewformer_amd.render import ViewRenderer
    s = _model(dev, 'f32')
    m, ctx, photos, cams = s['m'], s['ctx'], s['photos'][:, :4], s['cams']
    ctx_c, q_c = cams[:, :C_], cams[:, C_:C_ + 4]
    run = lambda r: (r.render(q_c, return_codes=True), r.localize(codes=photos, return_tokens=True), r.score(q_c, codes=photos))
    a = run(ViewRenderer(m, vq_m).set_context(codes=ctx, cameras=ctx_c, n_context=[2, 6]))
    ctx2, ctx_c2 = ctx.clone(), ctx_c.clone()
    ctx2[0, 2:] = (ctx2[0, 2:] + 17) % 1024
    ctx_c2[0, 2:] = ctx_c[1, 2:] + 0.25
    b = run(ViewRenderer(m, vq_m).set_context(codes=ctx2, cameras=ctx_c2, n_context=torch.tensor([2, 6])))
    for x, y in zip(a, b):
        for k in x:
            assert torch.equal(x[k][0], y[k][0]), k
    full = ViewRenderer(m, vq_m).set_context(codes=ctx, cameras=ctx_c).render(q_c, return_codes=True)
    assert torch.equal(a[0]['logits'][1], full['logits'][1]) and not torch.equal(a[0]['logits'][0], full['logits'][0])
    run1 = lambda r: (r.render(q_c[:1], return_codes=True), r.localize(codes=photos[:1], return_tokens=True), r.score(q_c[:1], codes=photos[:1]))
    alone = run1(ViewRenderer(m, vq_m).set_context(codes=ctx[:1, :2], cameras=ctx_c[:1, :2]))
    peak = float(alone[0]['logits'].abs().max())
    t_peak = float(alone[1]['pose_prediction'].abs().max())
    d_lg = float((a[0]['logits'][:1] - alone[0]['logits']).abs().max())
    d_tok = float(_token_distance(a[1]['pose_prediction'][:1], alone[1]['pose_prediction']).max())
    d_lp = float((a[2]['token_log_prob'][:1] - alone[2]['token_log_prob']).abs().max())
    parity_report(test='context_lengths_ragged_batch', B=2, C=C_, n_context=[2, 6], peak=peak, token_peak=t_peak, logits_max_diff=d_lg,
                  tokens_max_diff=d_tok, token_log_prob_max_diff=d_lp, logits_bit_identical=bool(torch.equal(a[0]['logits'][:1], alone[0]['logits'])),
                  cameras_bit_identical=bool(torch.equal(a[1]['generated_cameras'][:1], alone[1]['generated_cameras'])),
                  token_log_prob_bit_identical=bool(torch.equal(a[2]['token_log_prob'][:1], alone[2]['token_log_prob'])))
    assert d_lg < F32_LOGIT_TOL * max(1.0, peak)
    assert d_lp < F32_LOGIT_TOL * max(1.0, peak)
    assert d_tok < F32_TOKEN_TOL * max(1.0, t_peak)
    assert float((a[1]['generated_cameras'][:1] - alone[1]['generated_cameras']).abs().max()) < F32_TOKEN_TOL * max(1.0, t_peak)

# ---------------------------------------------------------------------------------------------- (f) chunking
@pytest.mark.parametrize('arm', ['f32', 'bf16'])
def test_a_sweeps_logits_do_not_depend_on_the_chunking(dev, vq_m, arm):
    """N = 4 cameras at sizes 0 ... 3: 16 views in one call, in two and in four (multiples of 4 views: the dense layers take one kernel)"""
    from viewformer_amd.render import ViewRenderer
    s = _model(dev, arm)
    r = ViewRenderer(s['m'], vq_m).set_context(codes=s['ctx'], cameras=s['cams'][:, :C_])
    q_c = s['cams'][:, C_:C_ + 4]
    one = r.sweep(q_c, sizes=[0, 1, 2, 3], max_views_per_call=16, return_codes=True)
    assert tuple(one['logits'].shape) == (B_, 4, 4, 8, 8, 1024) and tuple(one['generated_images'].shape) == (B_, 4, 4, 128, 128, 3)
    for cap in (8, 4):
        other = r.sweep(q_c, sizes=[0, 1, 2, 3], max_views_per_call=cap, return_codes=True)
        for k in ('logits', 'generated_codes', 'generated_images'):
            assert torch.equal(one[k], other[k]), (cap, k)
    # the layout: entry [b, n, k] is camera n at size k
    direct = r.render(q_c, return_codes=True, n_context=2)
    assert torch.equal(one['logits'][:, :, 2], direct['logits']) and torch.equal(one['generated_images'][:, :, 2], direct['generated_images'])
    assert not torch.equal(one['logits'][:, :, 2], one['logits'][:, :, 3])


# ---------------------------------------------------------------------------------------------- (g) refusals
def test_lengths_out_of_range_wrong_shapes_and_the_fp8_arm_are_refused(dev, vq_m):
    from viewformer_amd import _lib
    from viewformer_amd.migt import MIGT
    from viewformer_amd.render import ViewRenderer, evaluate_context_sizes
    from viewformer_amd.weights import make_migt_weights, synthetic_scene_batch
    s = _model(dev, 'f32')
    m, cache, qpos, photos, ctx, cams = s['m'], s['cache'], s['qpos'], s['photos'], s['ctx'], s['cams']
    for bad in (C_ + 1, -1, [1, 2, 3], [[1] * N_], 2.0, [0, C_ + 1], torch.full((B_, N_), C_ + 1, device=dev)):
        with pytest.raises(ValueError):
            m.generate_from_context(cache, qpos, n_context=bad)
        with pytest.raises(ValueError):
            m.localize_from_context(cache, photos, n_context=bad)
        with pytest.raises(ValueError):
            m.score_from_context(cache, qpos, photos, n_context=bad)
        with pytest.raises(ValueError):
            m.sample_from_context(cache, qpos, n_context=bad)
    r = ViewRenderer(m, vq_m)
    for bad in (0, [0, 3], [1, C_ + 1], [1, 2, 3], [[1, 2]], 1.5):
        with pytest.raises(ValueError):
            r.set_context(codes=ctx, cameras=cams[:, :C_], n_context=bad)
    r.set_context(codes=ctx, cameras=cams[:, :C_], n_context=[3, C_])
    with pytest.raises(ValueError):
        r.render(cams[:, C_:], n_context=C_ + 1)
    with pytest.raises(ValueError):
        r.sweep(cams[:, C_:], sizes=[0, C_ + 1])
    with pytest.raises(ValueError):
        r.localize(codes=photos, n_context=[1, 2, 3])
    frames, c1 = synthetic_scene_batch(2, 1, 128, seed=3)
    with pytest.raises(ValueError):
        evaluate_context_sizes(m, vq_m, torch.from_numpy(frames), torch.from_numpy(c1))        # S = 1: no context view
    cfg = _cfg(n_layer=2)
    fp8 = MIGT(cfg, precision='bf16', attention='fp8').load_state_dict(make_migt_weights(cfg, seed=0)).to(dev)
    with pytest.raises(_lib.VfError):                                # the fp8 attention arm has no cached contexts, with or without lengths
        ViewRenderer(fp8, vq_m).set_context(codes=ctx, cameras=cams[:, :C_], n_context=[2, 6])
