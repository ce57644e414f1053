"""GPU: novel-view rendering from a prefilled context (csrc/attention_prefix.hip, MIGT.prefill_context / generate_from_context,
viewformer_amd/render.py) against what the evaluator's route computes for the same scene: the kernel against an fp64 reference and the
existing twin-mask kernel, the fp32 arm against the full pass and the fp64 oracle, the bf16 arm on a trained model's peaked logits,
``render_views`` against ``generate_batch_predictions`` on replicated contexts, invariance under chunking, and the refusals.
Full-size models throughout.  Every measured figure goes through ``conftest.parity_report``.

Rule for bit-identity: the attention kernel gives a query the same bits whatever N and wherever the view sits in the
launch; the dense layers take the same kernel for row counts that are multiples of 256 (4 views), so for N and chunk sizes that are
multiples of 4 views the logits are ``torch.equal`` across chunkings; for other N only the arm's tolerance is asserted."""
import numpy as np
import pytest
import torch

from conftest import parity_report

pytestmark = pytest.mark.gpu

F32_LOGIT_TOL = 1e-3            # fp32 arm against fp64, times max(1, peak): the project's bound (tests/test_hip_parity_scale.py)
BF16_LOGIT_TOL_REL = 3e-2       # bf16 arm against the fp32 arm, times peak (PEAKED_LOGIT_TOL_REL there)
PEAKED_MIN_MAX_LOGIT = 10.0
PEAKED_CODE_AGREEMENT = 0.99
NEAR_TIE_ROWS_MAX = 0.02        # fp32 arm: rows inside the two paths' own error may be at most 2 % of all rows


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'needs the MI355X'
    return torch.device('cuda:0')


def _rand(shape, seed, scale):
    g = np.random.Generator(np.random.PCG64(seed))
    return torch.from_numpy((g.standard_normal(shape) * scale).astype(np.float32))


# ---------------------------------------------------------------------------------------------- (a) the kernel
def _attn_fp64(qkv_ctx, qkv_q, B, H, C, N, L):
    """every query row against its scene's C*L context keys and the L keys of its own view, fp64; thirds (V, Q, K)"""
    d = H * 64
    ctx = qkv_ctx.double().view(B, C * L, 3, H, 64)
    qq = qkv_q.double().view(B, N, L, 3, H, 64)
    kc, vc = ctx[:, :, 2].permute(0, 2, 1, 3), ctx[:, :, 0].permute(0, 2, 1, 3)                  # [B,H,C*L,64]
    q, k, v = (qq[:, :, :, i].permute(0, 3, 1, 2, 4) for i in (1, 2, 0))                       # [B,H,N,L,64]
    kk = torch.cat([kc[:, :, None].expand(B, H, N, C * L, 64), k], 3)
    vv = torch.cat([vc[:, :, None].expand(B, H, N, C * L, 64), v], 3)
    p = torch.softmax(q @ kk.transpose(-1, -2), -1)                                             # un-scaled scores
    return (p @ vv).permute(0, 2, 3, 1, 4).reshape(B * N * L, d)


@pytest.mark.parametrize('arm', ['bf16', 'bf16-f32io', 'f32eq'])
@pytest.mark.parametrize('B,H,C,N', [(1, 12, 6, 8), (2, 3, 1, 5), (1, 2, 19, 1), (2, 2, 6, 5), (1, 3, 19, 8), (3, 2, 1, 1), (2, 12, 6, 1)])
def test_prefix_attention_against_fp64_and_the_twin_mask_kernel(dev, arm, B, H, C, N):
    """random q/k/v laid out as in the ``qkv`` buffer; the existing kernel runs the same data as ONE sequence of C + N views with the
    last N marked as twins (each sees the prefix and itself).  The new kernel's max / rms error against fp64 may be at most 1.5x / 1.1x
    the existing kernel's, both measured here: the margin is for the noise of a sample maximum between two evaluations that sum in
    different orders, not for a looser kernel."""
    from viewformer_amd import ops
    L, d = 64, H * 64
    io16 = arm == 'bf16'
    dt = torch.bfloat16 if io16 else torch.float32
    qkv_ctx = _rand((B * C * L, 3 * d), 100 + C, 0.35).to(dev).to(dt)
    qkv_q = _rand((B * N * L, 3 * d), 200 + N, 0.35).to(dev).to(dt)
    ref = _attn_fp64(qkv_ctx, qkv_q, B, H, C, N, L)
    out = torch.full((B * N * L, d), float('nan'), dtype=dt, device=dev)
    ops.attn_prefix(qkv_q[:, d:2 * d], qkv_q[:, 2 * d:], qkv_q[:, :d], qkv_ctx[:, 2 * d:], qkv_ctx[:, :d], out, B, H, C, N, L,
                    3 * d, 3 * d, 3 * d, 3 * d, 3 * d, C * L * 3 * d, d, bf16=arm != 'f32eq')
    # the existing kernel on the concatenated views, twin mode
    T = (C + N) * L
    seq = torch.cat([qkv_ctx.view(B, C * L, 3 * d), qkv_q.view(B, N * L, 3 * d)], 1).reshape(B * T, 3 * d).contiguous()
    old = torch.full((B * T, d), float('nan'), dtype=dt, device=dev)
    ops.attn_blockcausal(seq[:, d:2 * d], seq[:, 2 * d:], seq[:, :d], old, B, H, T, L, 3 * d, 3 * d, 3 * d, d, 1.0, True, C,
                         bf16=arm != 'f32eq', x6=arm == 'f32eq')
    old = old.view(B, T, d)[:, C * L:].reshape(B * N * L, d)
    assert not torch.isnan(out.float()).any() and not torch.isnan(old.float()).any()
    e_new, e_old = (out.double() - ref).abs(), (old.double() - ref).abs()
    fig = dict(max_new=e_new.max().item(), max_old=e_old.max().item(), rms_new=e_new.pow(2).mean().sqrt().item(),
               rms_old=e_old.pow(2).mean().sqrt().item(), bit_identical=bool(torch.equal(out, old)))
    parity_report(test='prefix_attention_kernel', arm=arm, B=B, H=H, C=C, N=N, **fig)
    assert fig['max_new'] <= 1.5 * fig['max_old'], fig
    assert fig['rms_new'] <= 1.1 * fig['rms_old'], fig
    # a query's result does not depend on the other views of the launch: view 0 alone gives view 0's rows
    if N > 1:
        q1 = qkv_q.view(B, N, L, 3 * d)[:, :1].reshape(B * L, 3 * d).contiguous()
        one = torch.full((B * L, d), float('nan'), dtype=dt, device=dev)
        ops.attn_prefix(q1[:, d:2 * d], q1[:, 2 * d:], q1[:, :d], qkv_ctx[:, 2 * d:], qkv_ctx[:, :d], one, B, H, C, 1, L,
                        3 * d, 3 * d, 3 * d, 3 * d, 3 * d, C * L * 3 * d, d, bf16=arm != 'f32eq')
        assert torch.equal(one.view(B, L, d), out.view(B, N, L, d)[:, 0])


# ---------------------------------------------------------------------------------------------- shared model pieces
def _poses(B, C, N, seed):
    """(context poses [B,C,7], query poses [B,N,7]): all C + N cameras relativised at once (the same query poses as the reference's
    per-call relativisation of (context..., query n), tests/test_render_host.py) and normalised"""
    from viewformer_amd import geometry
    from viewformer_amd.weights import synthetic_scene_batch
    _, cams = synthetic_scene_batch(B, C + N, 8, seed)
    p = geometry.normalize_cameras(geometry.to_relative_cameras(torch.from_numpy(cams))[0])
    return p[:, :C].contiguous(), p[:, C:].contiguous()


def _full_logits(m, codes, cpos, qpos):
    """the full pass per query: model(dict(input_ids=[ctx, MASK], poses=[ctx, query n]), last_view_logits_only=True) -> [B,N,t,t,nE]"""
    dev = m.device
    ids = torch.cat([codes, torch.full_like(codes[:, :1], m.mask_token)], 1).to(dev)
    outs = []
    for n in range(qpos.shape[1]):
        poses = torch.cat([cpos, qpos[:, n:n + 1]], 1).to(dev)
        outs.append(m(dict(input_ids=ids, poses=poses), last_view_logits_only=True)['logits_last'])
    return torch.stack(outs, 1)


def _margin(lg):
    top2 = torch.topk(lg, 2, dim=-1).values
    return top2[..., 0] - top2[..., 1]


# ---------------------------------------------------------------------------------------------- (b) fp32 arm
def test_f32_arm_cached_generation_equals_the_full_pass_within_its_own_error(dev):
    from oracle import migt_oracle as mg
    from viewformer_amd.config import MIGTConfig
    from viewformer_amd.migt import MIGT
    from viewformer_amd.weights import make_migt_weights
    B, C, N = 2, 6, 8
    cfg = MIGTConfig(sequence_size=C + 1, n_loss_skip=1, pose_multiplier=0.2, localization_weight='1')
    sd = make_migt_weights(cfg, seed=0, std=0.03)
    g = np.random.Generator(np.random.PCG64(41))
    codes = torch.from_numpy(g.integers(0, cfg.n_embeddings, size=(B, C, 8, 8))).to(torch.int32)
    cpos, qpos = _poses(B, C, N, 43)
    m = MIGT(cfg).load_state_dict(sd).to(dev)
    full = _full_logits(m, codes, cpos, qpos).cpu()
    cache = m.prefill_context(codes, cpos)
    cached = m.generate_from_context(cache, qpos, codes_only=False).cpu()
    gen = m.generate_from_context(cache, qpos, codes_only=True).cpu()
    assert tuple(cached.shape) == (B, N, 8, 8, cfg.n_embeddings) and tuple(gen.shape) == (B, N, 8, 8)
    assert torch.equal(gen, cached.argmax(-1))                                       # codes_only is the arg-max of the logits it did not return
    # fp64 oracle: scene 0, queries 0 and 1
    ids = torch.cat([codes, torch.full_like(codes[:, :1], cfg.n_embeddings)], 1).long()
    ref = torch.stack([mg.migt_forward(sd, cfg, ids[:1], torch.cat([cpos[:1], qpos[:1, n:n + 1]], 1), dtype=torch.float64)['logits'][0, -1]
                       for n in (0, 1)])                                             # [2,t,t,nE]
    peak = float(ref.abs().max())
    e_full = float((full[0, :2].double() - ref).abs().max())
    e_cached = float((cached[0, :2].double() - ref).abs().max())
    # codes: equal to the full path's, except inside the two paths' own error (oracle margin where there is an oracle row)
    marg = _margin(full.double())
    marg[0, :2] = _margin(ref)
    near = marg < 2 * (e_cached + e_full)
    differ = cached.argmax(-1) != full.argmax(-1)
    parity_report(test='render_f32_arm', B=B, C=C, N=N, e_full=e_full, e_cached=e_cached, peak=peak, bit_identical=bool(torch.equal(cached, full)),
                  max_cached_vs_full=float((cached - full).abs().max()), rows=int(differ.numel()), rows_differing=int(differ.sum()),
                  rows_near_tie=int(near.sum()), min_margin=float(marg.min()), oracle_rows_below_1e_3=float((_margin(ref) < 1e-3).float().mean()))
    assert e_cached <= 1.5 * e_full, (e_cached, e_full)
    assert e_cached < F32_LOGIT_TOL * max(1.0, peak), e_cached
    assert bool((~differ | near).all()), 'a generated code differs from the full path outside the two paths\' error'
    assert float(near.float().mean()) <= NEAR_TIE_ROWS_MAX, float(near.float().mean())


# ---------------------------------------------------------------------------------------------- (c) bf16 arm on peaked logits
@pytest.fixture(scope='module')
def trained(dev, full_vq):
    """the trained full-size model of tests/test_hip_parity_scale.py::test_mixed_arm_on_a_trained_model_with_peaked_logits, built the same way"""
    from viewformer_amd import geometry
    from viewformer_amd.config import MIGTConfig
    from viewformer_amd.migt import MIGT
    from viewformer_amd.train import MIGTTrainer
    from viewformer_amd.vqgan import VQGAN
    from viewformer_amd.weights import make_migt_weights, synthetic_scene_batch
    vcfg, vsd, _ = full_vq
    B, S = 8, 7
    frames, cams = synthetic_scene_batch(B, S, 128, seed=33)
    vq_m = VQGAN(vcfg, data_format='NHWC', conv_arith='x3h').load_state_dict(vsd).to(dev)
    codes = vq_m.encode(torch.from_numpy(frames.reshape(-1, 128, 128, 3)).to(dev))[-1].view(B, S, 8, 8)
    del vq_m
    poses = geometry.normalize_cameras(geometry.to_relative_cameras(torch.from_numpy(cams))[0])
    cfg = MIGTConfig(sequence_size=S, n_loss_skip=1, pose_multiplier=0.2, localization_weight='1', dropout=0.0, learning_rate=3e-4,
                     weight_decay=0.01, total_steps=2000)
    tr = MIGTTrainer(MIGT(cfg, precision='bf16').load_state_dict(make_migt_weights(cfg, seed=0)).to(dev), warmup_steps=20)
    ce, steps = float('inf'), 0
    while ce > 0.3 and steps < 700:
        for _ in range(50):
            met = tr.train_step(poses, codes, reduce_gradients=False)
        steps += 50
        ce = float(met['ce_loss'])
    sd = tr.state_dict()
    del tr
    torch.cuda.empty_cache()
    return dict(cfg=cfg, sd=sd, codes=codes.cpu(), poses=poses, frames=frames, cams=cams, steps=steps, ce=ce)


def _interpolate(a, b, w):
    """a pose between two normalised poses: positions linearly, quaternions by normalised linear interpolation on the same hemisphere"""
    from viewformer_amd import geometry
    qa, qb = a[..., 3:], b[..., 3:]
    qb = torch.where((qa * qb).sum(-1, keepdim=True) < 0, -qb, qb)
    return geometry.normalize_cameras(torch.cat([(1 - w) * a[..., :3] + w * b[..., :3], (1 - w) * qa + w * qb], -1))


def test_bf16_arm_cached_generation_on_a_trained_model_with_peaked_logits(dev, trained):
    """queries: every scene's training target pose (the poses the head is confident at) and three novel poses per scene interpolated
    between context cameras.  d_full = bf16 full pass against the fp32 arm, d_cached = cached bf16 pass against the fp32 arm."""
    from viewformer_amd.migt import MIGT
    cfg, sd, codes, poses = trained['cfg'], trained['sd'], trained['codes'], trained['poses']
    B, C = codes.shape[0], codes.shape[1] - 1
    ctx_codes, cpos = codes[:, :C].to(torch.int32), poses[:, :C].contiguous()
    qpos = torch.stack([poses[:, C], _interpolate(poses[:, 1], poses[:, 2], 0.5), _interpolate(poses[:, 3], poses[:, 4], 0.3),
                        _interpolate(poses[:, 2], poses[:, 5], 0.7)], 1)                                 # [B,4,7]
    N = qpos.shape[1]
    m32 = MIGT(cfg, precision='f32').load_state_dict(sd).to(dev)
    l32 = _full_logits(m32, ctx_codes, cpos, qpos).cpu().double()
    del m32
    m16 = MIGT(cfg, precision='bf16').load_state_dict(sd).to(dev)
    l16 = _full_logits(m16, ctx_codes, cpos, qpos).cpu().double()
    cache = m16.prefill_context(ctx_codes, cpos)
    lc = m16.generate_from_context(cache, qpos, codes_only=False).cpu().double()
    gen = m16.generate_from_context(cache, qpos, codes_only=True).cpu()
    del m16
    peak = float(l32[:, 0].abs().max())                                                                   # at the training target poses, as the model test
    d_full, d_cached = (l16 - l32).abs(), (lc - l32).abs()
    c32, c16, cc = l32.argmax(-1), l16.argmax(-1), lc.argmax(-1)
    bad = (cc != c16)
    gap_cached = l32.gather(-1, c32[..., None]) - l32.gather(-1, cc[..., None])
    gap_full = l32.gather(-1, c32[..., None]) - l32.gather(-1, c16[..., None])
    worst_gap = float(torch.maximum(gap_cached, gap_full)[..., 0][bad].max()) if bool(bad.any()) else 0.0
    marg = _margin(l32)
    fig = dict(train_steps=trained['steps'], final_ce=trained['ce'], peak=peak, peak_novel=float(l32[:, 1:].abs().max()),
               d_full_max=float(d_full.max()), d_cached_max=float(d_cached.max()), d_full_rms=float(d_full.pow(2).mean().sqrt()),
               d_cached_rms=float(d_cached.pow(2).mean().sqrt()), cached_vs_full_bf16_max=float((lc - l16).abs().max()),
               bit_identical=bool(torch.equal(lc, l16)),
               code_agreement_cached_vs_full=1.0 - float(bad.float().mean()), disagreements=int(bad.sum()), worst_f32_gap_at_disagreement=worst_gap,
               code_agreement_full_bf16_vs_f32_target=float((c16[:, 0] == c32[:, 0]).float().mean()),
               code_agreement_full_bf16_vs_f32_novel=float((c16[:, 1:] == c32[:, 1:]).float().mean()),
               code_agreement_cached_vs_f32_novel=float((cc[:, 1:] == c32[:, 1:]).float().mean()),
               median_margin_target=float(marg[:, 0].median()), median_margin_novel=float(marg[:, 1:].median()),
               target_token_accuracy=float((c32[:, 0] == codes[:, C].long()).float().mean()))
    parity_report(test='render_bf16_arm_peaked', B=B, C=C, N=N, **fig)
    assert peak >= PEAKED_MIN_MAX_LOGIT, f'training did not produce a peaked head: max |logit| {peak:.2f} after {trained["steps"]} steps'
    assert torch.equal(gen, cc)                                                      # the fused arg-max is the arg-max of the logits
    assert fig['d_cached_max'] <= 1.5 * fig['d_full_max'], fig
    assert fig['d_cached_rms'] <= 1.1 * fig['d_full_rms'], fig
    assert fig['d_cached_max'] < BF16_LOGIT_TOL_REL * peak, fig
    assert fig['code_agreement_cached_vs_full'] >= PEAKED_CODE_AGREEMENT, fig
    assert worst_gap <= 2 * BF16_LOGIT_TOL_REL * peak, fig                           # a disagreement only inside the logit tolerance


# ---------------------------------------------------------------------------------------------- (d) end to end
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


def _parent_route(tr_m, vq_m, frames, cams, qcams):
    """generate_batch_predictions on replicated contexts with dummy targets: scene (b, n) = (context of b..., any frame) with cameras
    (context cameras of b..., query n)"""
    from viewformer_amd.evaluate import generate_batch_predictions
    B, C = cams.shape[:2]
    N = qcams.shape[1]
    dummy = torch.zeros_like(frames[:, :1])
    img = torch.cat([frames, dummy], 1)[:, None].expand(B, N, C + 1, *frames.shape[2:]).reshape(B * N, C + 1, *frames.shape[2:])
    cam = torch.cat([cams[:, None].expand(B, N, C, 7), qcams[:, :, None]], 2).reshape(B * N, C + 1, 7)
    return generate_batch_predictions(tr_m, vq_m, img, cam, return_codes=True)


def _compare_end_to_end(label, got, want, B, N, arm, peak_tol=None):
    lg, lf = got['logits'].reshape(B * N, -1, got['logits'].shape[-1]).double().cpu(), want['logits_last'].reshape(B * N, -1, got['logits'].shape[-1]).double().cpu()
    cg, cf = got['generated_codes'].reshape(B * N, -1).cpu(), want['generated_codes'].reshape(B * N, -1).cpu()
    d = float((lg - lf).abs().max())
    peak = float(lf.abs().max())
    differ = cg != cf
    same_map = ~differ.any(1)
    ig, iw = got['generated_images'].reshape(B * N, *got['generated_images'].shape[2:]), want['generated_images']
    assert ig.dtype == torch.uint8 and ig.shape == iw.shape
    img_equal = bool(torch.equal(ig[same_map.to(ig.device)], iw[same_map.to(iw.device)]))
    best = lf.max(-1).values
    gap = best - lf.gather(-1, cg[..., None].long())[..., 0]                         # the full path's own gap to the renderer's choice
    fig = dict(logit_diff_max=d, peak=peak, bit_identical=bool(torch.equal(lg, lf)), rows=int(differ.numel()), rows_differing=int(differ.sum()),
               whole_maps_agreeing=int(same_map.sum()), maps=B * N, images_equal_where_maps_agree=img_equal,
               worst_gap_at_disagreement=float(gap[differ].max()) if bool(differ.any()) else 0.0)
    parity_report(test='render_end_to_end', case=label, arm=arm, B=B, N=N, **fig)
    if arm == 'f32':
        # (b)'s rules without an oracle: |cached - full| <= e_cached + e_full, each bounded by the arm's 1e-3; a code may differ only
        # where the full path's margin is inside twice that distance, and such rows are at most 2 %
        assert d < 2 * F32_LOGIT_TOL * max(1.0, peak), fig
        near = _margin(lf) < 2 * d
        assert bool((~differ | near).all()) and float(near.float().mean()) <= NEAR_TIE_ROWS_MAX, fig
    else:
        assert d < 2 * BF16_LOGIT_TOL_REL * peak_tol, fig
        assert 1.0 - float(differ.float().mean()) >= PEAKED_CODE_AGREEMENT, fig
        assert fig['worst_gap_at_disagreement'] <= 2 * BF16_LOGIT_TOL_REL * peak_tol, fig
    assert img_equal, fig
    return fig


@pytest.mark.parametrize('augment', ['relative', 'no'])
def test_render_views_equals_the_evaluator_on_replicated_contexts_f32(dev, full_vq, augment):
    from viewformer_amd.config import MIGTConfig
    from viewformer_amd.migt import MIGT
    from viewformer_amd.render import ViewRenderer, render_views
    from viewformer_amd.vqgan import VQGAN
    from viewformer_amd.weights import make_migt_weights, synthetic_scene_batch
    vcfg, vsd, _ = full_vq
    B, C, N = 2, 6, 4
    cfg = MIGTConfig(sequence_size=C + 1, n_loss_skip=1, pose_multiplier=0.2, localization_weight='1', augment_poses=augment)
    tr_m = MIGT(cfg).load_state_dict(make_migt_weights(cfg, seed=0, std=0.03)).to(dev)
    vq_m = VQGAN(vcfg, data_format='NHWC', conv_arith='x3h').load_state_dict(vsd).to(dev)
    frames, cams = synthetic_scene_batch(B, C + N, 128, seed=51)
    frames, cams = torch.from_numpy(frames), torch.from_numpy(cams)
    ctx_f, ctx_c, q_c = frames[:, :C], cams[:, :C], cams[:, C:]
    want = _parent_route(tr_m, vq_m, ctx_f.to(dev), ctx_c.to(dev), q_c.to(dev))
    # host inputs, one call; device inputs through the object, two render calls, the encoder counted
    got_host = render_views(tr_m, vq_m, ctx_f, ctx_c, q_c, return_codes=True)
    _compare_end_to_end(f'{augment}/host', got_host, want, B, N, 'f32')
    with _CountingEncoder(vq_m) as enc:
        r = ViewRenderer(tr_m, vq_m).set_context(images=ctx_f.to(dev), cameras=ctx_c.to(dev))
        first = r.render(q_c[:, :2].to(dev), return_codes=True)
        second = r.render(q_c[:, 2:].to(dev), return_codes=True)
        plain = r.render(q_c[:, 2:].to(dev))
        assert enc.calls == 1, enc.calls                                             # the context is encoded once, nothing else ever
    assert set(plain) == {'generated_images'} and tuple(plain['generated_images'].shape) == (B, 2, 128, 128, 3)
    assert torch.equal(plain['generated_images'], second['generated_images'])        # the fused arg-max route: the same pictures
    assert tuple(first['generated_codes'].shape) == (B, 2, 8, 8) and tuple(first['decoded'].shape) == (B, 2, 128, 128, 3)
    got_dev = {k: torch.cat([first[k], second[k]], 1) for k in first}
    _compare_end_to_end(f'{augment}/device,two calls', got_dev, want, B, N, 'f32')
    assert torch.equal(r.render(q_c[:, :0])['generated_images'], torch.empty((B, 0, 128, 128, 3), dtype=torch.uint8, device=dev))


def test_render_views_from_a_scene_bank_and_with_19_context_views_f32(dev, full_vq):
    from viewformer_amd.config import MIGTConfig
    from viewformer_amd.migt import MIGT
    from viewformer_amd.render import render_views
    from viewformer_amd.scene_bank import SceneBank
    from viewformer_amd.vqgan import VQGAN
    from viewformer_amd.weights import make_migt_weights, synthetic_scene_batch
    vcfg, vsd, _ = full_vq
    vq_m = VQGAN(vcfg, data_format='NHWC', conv_arith='x3h').load_state_dict(vsd).to(dev)
    frames, cams = synthetic_scene_batch(1, 40, 128, seed=21)
    bank = SceneBank(vq_m, torch.from_numpy(frames[0]), cams[0], batch_size=16)
    for C, B, N, idx in ((6, 2, 3, [[3, 1, 39, 7, 20, 11], [0, 5, 17, 18, 33, 2]]), (19, 1, 2, [list(range(1, 39, 2))])):
        cfg = MIGTConfig(sequence_size=C + 1, n_loss_skip=1, pose_multiplier=0.2, localization_weight='1')
        tr_m = MIGT(cfg).load_state_dict(make_migt_weights(cfg, seed=0, std=0.03)).to(dev)
        idx = torch.tensor(idx)
        codes, ctx_c = bank.gather(idx)
        _, qc = synthetic_scene_batch(B, N, 8, seed=60 + C)
        q_c = torch.from_numpy(qc).to(dev)
        with _CountingEncoder(vq_m) as enc:
            got = render_views(tr_m, vq_m, None, ctx_c, q_c, codes=codes, return_codes=True)
            assert enc.calls == 0                                                    # the bank's codes: no encoder pass at all
        want = _parent_route(tr_m, vq_m, bank.frames_at(idx), ctx_c, q_c)
        assert torch.equal(want['codes'].view(B * N, C + 1, 8, 8)[::N, :C], codes)   # (the evaluator's context codes are the bank's)
        _compare_end_to_end(f'scene bank, C={C}', got, want, B, N, 'f32')
        del tr_m


def test_render_views_equals_the_evaluator_on_the_trained_model_bf16(dev, full_vq, trained):
    from viewformer_amd.migt import MIGT
    from viewformer_amd.render import render_views
    from viewformer_amd.vqgan import VQGAN
    vcfg, vsd, _ = full_vq
    cfg, sd = trained['cfg'], trained['sd']
    B, C = 4, 6
    frames, cams = torch.from_numpy(trained['frames'][:B]), torch.from_numpy(trained['cams'][:B])
    tr_m = MIGT(cfg, precision='bf16').load_state_dict(sd).to(dev)
    vq_m = VQGAN(vcfg, data_format='NHWC', decoder_precision='bf16', conv_arith='x3h').load_state_dict(vsd).to(dev)
    ctx_f, ctx_c = frames[:, :C].to(dev), cams[:, :C].to(dev)
    mid = cams[:, 1:4].clone()                                                       # two more world-frame queries near context cameras
    mid[..., :3] = 0.5 * (cams[:, 1:4, :3] + cams[:, 2:5, :3])
    q_c = torch.cat([cams[:, C:], mid[:, :2]], 1).to(dev)                            # the training target pose first
    N = q_c.shape[1]
    want = _parent_route(tr_m, vq_m, ctx_f, ctx_c, q_c)
    got = render_views(tr_m, vq_m, ctx_f, ctx_c, q_c, return_codes=True)
    peak = float(want['logits_last'].reshape(B, N, -1)[:, 0].abs().max())
    assert peak >= PEAKED_MIN_MAX_LOGIT, peak
    _compare_end_to_end('trained model', got, want, B, N, 'bf16', peak_tol=peak)
    plain = render_views(tr_m, vq_m, ctx_f, ctx_c, q_c)                              # the fused arg-max route gives the same pictures
    assert torch.equal(plain['generated_images'], got['generated_images'])


# ---------------------------------------------------------------------------------------------- (e) invariance
@pytest.mark.parametrize('arm', ['f32', 'bf16'])
def test_a_views_logits_do_not_depend_on_the_chunking(dev, full_vq, arm):
    from viewformer_amd.config import MIGTConfig
    from viewformer_amd.migt import MIGT
    from viewformer_amd.render import ViewRenderer
    from viewformer_amd.vqgan import VQGAN
    from viewformer_amd.weights import make_migt_weights, synthetic_scene_batch
    vcfg, vsd, _ = full_vq
    B, C, N = 2, 6, 8
    cfg = MIGTConfig(sequence_size=C + 1, n_loss_skip=1, pose_multiplier=0.2, localization_weight='1')
    tr_m = MIGT(cfg, precision=arm).load_state_dict(make_migt_weights(cfg, seed=0, std=0.03 if arm == 'f32' else 0.02)).to(dev)
    vq_m = VQGAN(vcfg, data_format='NHWC', conv_arith='x3h').load_state_dict(vsd).to(dev)
    g = np.random.Generator(np.random.PCG64(71))
    codes = torch.from_numpy(g.integers(0, cfg.n_embeddings, size=(B, C, 8, 8))).to(torch.int32)
    _, cams = synthetic_scene_batch(B, C + N, 8, seed=72)
    cams = torch.from_numpy(cams).to(dev)
    r = ViewRenderer(tr_m, vq_m).set_context(codes=codes, cameras=cams[:, :C])
    q = cams[:, C:]
    one = r.render(q, return_codes=True)
    # multiples of 4 views: identical bits
    halves = r.render(q, max_views_per_call=4, return_codes=True)
    a, b = r.render(q[:, :4], return_codes=True), r.render(q[:, 4:], return_codes=True)
    among = r.render(q[:, 4:], return_codes=True)['logits']                          # views 4..7 alone against the same views among eight
    for k in ('logits', 'generated_codes', 'generated_images', 'decoded'):
        assert torch.equal(one[k], halves[k]), k
        assert torch.equal(one[k], torch.cat([a[k], b[k]], 1)), k
    assert torch.equal(among, one['logits'][:, 4:])
    # other N: the arm's tolerance (and what was measured)
    peak = float(one['logits'].abs().max())
    tol = F32_LOGIT_TOL * max(1.0, peak) if arm == 'f32' else BF16_LOGIT_TOL_REL * peak
    odd = {}
    for cap in (1, 3, 5):
        lg = r.render(q[:, :5], max_views_per_call=cap, return_codes=True)['logits']
        dmax = float((lg - one['logits'][:, :5]).abs().max())
        odd[cap] = dict(max_diff=dmax, bit_identical=bool(torch.equal(lg, one['logits'][:, :5])))
        assert dmax < tol, (cap, dmax, tol)
    parity_report(test='render_chunk_invariance', arm=arm, B=B, C=C, N=N, peak=peak, five_views_in_chunks_of=odd)


# ---------------------------------------------------------------------------------------------- (f) refusals
def test_unsupported_arms_shapes_and_foreign_caches_are_refused(dev):
    from conftest import TINY_MIGT
    from viewformer_amd import _lib
    from viewformer_amd.config import MIGTConfig
    from viewformer_amd.migt import MIGT
    from viewformer_amd.weights import make_migt_weights
    cfg = MIGTConfig(sequence_size=3, n_loss_skip=1, pose_multiplier=0.2, localization_weight='1', n_layer=2)
    sd = make_migt_weights(cfg, seed=0)
    codes = torch.zeros((2, 2, 8, 8), dtype=torch.int32)
    cpos, qpos = _poses(2, 2, 3, 5)
    with pytest.raises(_lib.VfError):                                                # no fp8 arm of the prefix attention, and no fallback
        MIGT(cfg, precision='bf16', attention='fp8').load_state_dict(sd).to(dev).prefill_context(codes, cpos)
    tiny = MIGTConfig(**TINY_MIGT)                                                   # 4 x 4 token maps: L = 16
    with pytest.raises(_lib.VfError):
        MIGT(tiny).load_state_dict(make_migt_weights(tiny, seed=0)).to(dev).prefill_context(torch.zeros((1, 2, 4, 4), dtype=torch.int32), cpos[:1])
    a = MIGT(cfg).load_state_dict(sd).to(dev)
    b = MIGT(cfg).load_state_dict(sd).to(dev)
    b16 = MIGT(cfg, precision='bf16').load_state_dict(sd).to(dev)
    cache = a.prefill_context(codes, cpos)
    assert tuple(a.generate_from_context(cache, qpos).shape) == (2, 3, 8, 8)
    for other in (b, b16):
        with pytest.raises(ValueError):
            other.generate_from_context(cache, qpos)
    with pytest.raises(ValueError):
        a.generate_from_context(cache, qpos[:1])                                     # another batch size
    a.load_state_dict(sd)                                                            # new weights: the cache is stale
    with pytest.raises(ValueError):
        a.generate_from_context(cache, qpos)
    assert a.generate_from_context(a.prefill_context(codes, cpos), qpos[:, :0]).shape == (2, 0, 8, 8)
