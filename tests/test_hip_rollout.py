"""GPU: a context cache that grows (``MIGT.prefill_context(capacity=...)``, ``append_to_context``,
``rollout_from_context``, ``ViewRenderer.append`` / ``rollout``, ``render.rollout_views``).

The first c views of a cache are the cache of those c views, so a view appended behind them changes none of them, and everything here is
checked against code that existed before: the tight cache, ``prefill_context`` of all views, the explicit loop of ``sample_from_context``
and ``append_to_context``, the full pass and the fp64 oracle.  The exact tests run at B = 4: every pass then has a multiple of 256 rows and
the dense layers take one kernel whatever the call.  Full-size models throughout; every measured figure goes through
``conftest.parity_report`` (profiles/rollout_parity.txt keeps a run's lines)."""
import numpy as np
import pytest
import torch

from conftest import parity_report
from test_hip_render import (BF16_LOGIT_TOL_REL, F32_LOGIT_TOL, NEAR_TIE_ROWS_MAX, PEAKED_CODE_AGREEMENT, PEAKED_MIN_MAX_LOGIT, _full_logits,
                             _interpolate, _margin, trained)  # noqa: F401  (``trained``: the module-scoped fixture, built here as there)

pytestmark = pytest.mark.gpu

L, T_ = 64, 8                     # tokens per view, token image size


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'needs the MI355X'
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def vq_m(dev, full_vq):
    from viewformer_amd.vqgan import VQGAN
    vcfg, vsd, _ = full_vq
    return VQGAN(vcfg, data_format='NHWC', conv_arith='x3h').load_state_dict(vsd).to(dev)


def _cfg(**kw):
    from viewformer_amd.config import MIGTConfig
    return MIGTConfig(sequence_size=7, n_loss_skip=1, pose_multiplier=0.2, localization_weight='1', **kw)


def _scene(B, V, seed):
    """(codes int32 [B,V,8,8], model poses [B,V,7] relative to view 0 and normalised, world cameras [B,V,7])"""
    from viewformer_amd import geometry
    from viewformer_amd.weights import synthetic_scene_batch
    g = np.random.Generator(np.random.PCG64(seed))
    codes = torch.from_numpy(g.integers(0, 1024, size=(B, V, T_, T_))).to(torch.int32)
    _, cams = synthetic_scene_batch(B, V, 8, seed + 1)
    cams = torch.from_numpy(cams)
    return codes, geometry.normalize_cameras(geometry.to_relative_cameras(cams)[0]).contiguous(), cams


_models = {}
B4, V4 = 4, 8


def _model(dev, arm):
    """full-size model and a B = 4 scene of 8 views"""
    if arm not in _models:
        from viewformer_amd.migt import MIGT
        from viewformer_amd.weights import make_migt_weights
        cfg = _cfg()
        sd = make_migt_weights(cfg, seed=0, std=0.03 if arm == 'f32' else 0.02)
        codes, poses, cams = _scene(B4, V4, 171)
        _models[arm] = dict(cfg=cfg, sd=sd, m=MIGT(cfg, precision=arm).load_state_dict(sd).to(dev), codes=codes, poses=poses.to(dev), cams=cams)
    return _models[arm]


def _thirds(cache, n_views):
    """every layer's V and K thirds of the first ``n_views`` views of every scene (the Q third is never read again)"""
    d = cache.kv[0].shape[1] // 3
    out = []
    for kv in cache.kv:
        v = kv.view(cache.B, cache.capacity, L, 3 * d)[:, :n_views]
        out.append((v[..., :d], v[..., 2 * d:]))
    return out


def _same_thirds(a, b, n_views):
    return all(torch.equal(va, vb) and torch.equal(ka, kb) for (va, ka), (vb, kb) in zip(_thirds(a, n_views), _thirds(b, n_views)))


def _answers(m, cache, qpos, photos):
    """logits, cameras, token log-probabilities and top-k-1 samples of one cache"""
    return dict(logits=m.generate_from_context(cache, qpos, codes_only=False), cameras=m.localize_from_context(cache, photos),
                token_log_prob=m.score_from_context(cache, qpos, photos)['token_log_prob'],
                samples=m.sample_from_context(cache, qpos, n_samples=2, top_k=1, seed=3)['codes'])


# ---------------------------------------------------------------------------------------------- exact tests, both arms, B = 4
@pytest.mark.parametrize('arm', ['f32', 'bf16'])
def test_a_cache_with_slack_answers_as_the_tight_cache_whatever_the_slack_holds(dev, arm):
    """(i) capacity = C + 3, nothing appended: ``torch.equal`` logits, cameras, token log-probabilities and top-k-1 samples;
    (ii) the slack filled with NaN changes nothing"""
    s = _model(dev, arm)
    m, codes, poses = s['m'], s['codes'], s['poses']
    C = 3
    qpos, photos = poses[:, 4:8], codes[:, 4:8]
    tight = m.prefill_context(codes[:, :C], poses[:, :C])
    assert tight.capacity == C and tight.lengths is None and not tight.ragged()
    exact = m.prefill_context(codes[:, :C], poses[:, :C], capacity=C)             # no room asked for: the tight cache, nothing moved
    assert exact.capacity == C and not exact.ragged() and tuple(exact.kv[0].shape) == tuple(tight.kv[0].shape)
    roomy = m.prefill_context(codes[:, :C], poses[:, :C], capacity=C + 3)
    assert roomy.capacity == C + 3 and roomy.C == C and roomy.B == B4 and roomy.ragged()
    assert tuple(roomy.kv[0].shape) == (B4 * (C + 3) * L, 3 * 768) and roomy.kv[0].dtype == tight.kv[0].dtype
    assert _same_thirds(tight, roomy, C)
    want = _answers(m, tight, qpos, photos)
    got = _answers(m, roomy, qpos, photos)
    for k in want:
        assert torch.equal(got[k], want[k]), k
    for kv in roomy.kv:                                                   # (ii)
        kv.view(B4, C + 3, L, -1)[:, C:] = float('nan')
    got = _answers(m, roomy, qpos, photos)
    for k in want:
        assert torch.equal(got[k], want[k]), k
    # an explicit length is validated against what is filled, not against the room
    with pytest.raises(ValueError):
        m.generate_from_context(roomy, qpos, n_context=C + 1)
    assert torch.equal(m.generate_from_context(roomy, qpos, codes_only=False, n_context=C), want['logits'])


@pytest.mark.parametrize('arm', ['f32', 'bf16'])
def test_appending_at_once_one_by_one_and_past_the_capacity_give_the_same_bits(dev, arm):
    """(iii) 3 views at once and one by one: ``torch.equal`` K and V thirds in every layer and logits of a following
    ``generate_from_context``; (iv) appending past the capacity reallocates inside the same object, to max(2 capacity, needed), and gives
    the bits of a cache that had the room from the start"""
    s = _model(dev, arm)
    m, codes, poses = s['m'], s['codes'], s['poses']
    C0, K = 2, 3
    qpos = poses[:, 5:8]
    roomy = m.prefill_context(codes[:, :C0], poses[:, :C0], capacity=C0 + K)
    at_once = m.append_to_context(roomy, codes[:, C0:C0 + K], poses[:, C0:C0 + K])
    assert at_once is roomy and roomy.C == C0 + K and roomy.capacity == C0 + K and roomy.filled().tolist() == [C0 + K] * B4
    one = m.prefill_context(codes[:, :C0], poses[:, :C0], capacity=C0 + K)
    for j in range(K):
        m.append_to_context(one, codes[:, C0 + j:C0 + j + 1], poses[:, C0 + j:C0 + j + 1])
        assert one.C == C0 + j + 1 and one.capacity == C0 + K
    assert _same_thirds(roomy, one, C0 + K)
    lg = m.generate_from_context(roomy, qpos, codes_only=False)
    assert torch.equal(lg, m.generate_from_context(one, qpos, codes_only=False))
    # (iv) from the tight cache: 2 -> max(4, 3) = 4 -> max(8, 5) = 8 views of room, the same object throughout
    grown = m.prefill_context(codes[:, :C0], poses[:, :C0])
    first_buffer = grown.kv[0]
    assert m.append_to_context(grown, codes[:, C0:C0 + 1], poses[:, C0:C0 + 1]) is grown and grown.capacity == 4
    assert grown.kv[0] is not first_buffer
    m.append_to_context(grown, codes[:, C0 + 1:C0 + K], poses[:, C0 + 1:C0 + K])
    assert grown.capacity == 8 and grown.C == C0 + K
    assert _same_thirds(roomy, grown, C0 + K)
    assert torch.equal(lg, m.generate_from_context(grown, qpos, codes_only=False))
    # against the cache of all five views: recorded, not asserted — the prefill's attention is the block-causal kernel, an appended
    # view's the prefix kernel (the tolerance tests below hold the two together)
    whole = m.prefill_context(codes[:, :C0 + K], poses[:, :C0 + K])
    lw = m.generate_from_context(whole, qpos, codes_only=False)
    parity_report(test='append_vs_prefill_of_all_views', arm=arm, B=B4, C0=C0, K=K, thirds_bit_identical=_same_thirds(whole, grown, C0 + K),
                  logits_bit_identical=bool(torch.equal(lg, lw)), logits_max_diff=float((lg - lw).abs().max()), peak=float(lw.abs().max()))


def _explicit_loop(m, cache, path, **kw):
    """the definition: ``sample_from_context`` of 1 view at path[t] (view0 = t), then ``append_to_context`` of what it drew"""
    codes, logits = [], []
    for t in range(path.shape[1]):
        s = m.sample_from_context(cache, path[:, t:t + 1], n_samples=1, view0=t, return_logits=True, **kw)
        codes.append(s['codes'][:, 0, 0])
        logits.append(s['logits'][:, 0])
        m.append_to_context(cache, s['codes'][:, :, 0], path[:, t:t + 1])
    return torch.stack(codes, 1), torch.stack(logits, 1)


@pytest.mark.parametrize('arm', ['f32', 'bf16'])
def test_the_fused_step_the_two_pass_step_and_the_explicit_loop_roll_out_the_same_bits(dev, arm):
    """(v) C0 = 2, T = 3: codes and logits ``torch.equal``; the grown caches hold the same keys and values"""
    s = _model(dev, arm)
    m, codes, poses = s['m'], s['codes'], s['poses']
    C0, T = 2, 3
    path = poses[:, 4:4 + T]
    new = lambda: m.prefill_context(codes[:, :C0], poses[:, :C0], capacity=C0 + T)
    fused = m.rollout_from_context(new(), path, return_logits=True)
    two = m.rollout_from_context(new(), path, return_logits=True, fused_step=False)
    loop_cache = new()
    lc, ll = _explicit_loop(m, loop_cache, path, top_k=1)
    assert tuple(fused['codes'].shape) == (B4, 1, T, T_, T_) and tuple(fused['logits'].shape) == (B4, 1, T, T_, T_, 1024)
    assert tuple(fused['log_likelihood'].shape) == (B4, 1, T) and tuple(fused['token_log_prob'].shape) == (B4, 1, T, T_, T_)
    for k in ('codes', 'logits', 'token_log_prob', 'log_likelihood'):
        assert torch.equal(fused[k], two[k]), k
    assert torch.equal(fused['codes'][:, 0], lc) and torch.equal(fused['logits'][:, 0], ll)
    assert torch.equal(fused['codes'][:, 0], fused['logits'][:, 0].argmax(-1))           # top_k = 1 (the default): the arg-max roll-out
    for c in (fused['cache'], two['cache'], loop_cache):
        assert c.C == C0 + T and c.capacity == C0 + T
    assert _same_thirds(fused['cache'], two['cache'], C0 + T) and _same_thirds(fused['cache'], loop_cache, C0 + T)
    # the frames depend on each other: frame 1 is not what the photographs alone give at its camera
    alone = m.generate_from_context(new(), path, codes_only=False)
    assert torch.equal(alone[:, 0], fused['logits'][:, 0, 0]) and not torch.equal(alone[:, 1], fused['logits'][:, 0, 1])


@pytest.mark.parametrize('arm', ['f32', 'bf16'])
def test_trajectories_are_reproducible_independent_and_prefixes_of_longer_ones(dev, arm):
    """(vii) ``n_samples = 3, top_k = 1`` is the arg-max roll-out in every trajectory; one seed, one result; another seed differs; the
    T = 2 roll-out is a prefix of the T = 3 one; the caller's cache is not the replicated one and stays as it was"""
    s = _model(dev, arm)
    m, codes, poses = s['m'], s['codes'], s['poses']
    C0, T, S = 2, 3, 3
    path = poses[:, 4:4 + T]
    base = m.prefill_context(codes[:, :C0], poses[:, :C0], capacity=C0 + T)
    greedy = m.rollout_from_context(m.prefill_context(codes[:, :C0], poses[:, :C0], capacity=C0 + T), path, return_logits=True)
    g3 = m.rollout_from_context(base, path, n_samples=S, top_k=1, seed=9, return_logits=True)
    assert tuple(g3['codes'].shape) == (B4, S, T, T_, T_) and g3['cache'] is not base and g3['cache'].B == B4 * S
    assert base.C == C0 and base.B == B4
    for k in ('codes', 'logits'):
        assert torch.equal(g3[k], greedy[k].expand(B4, S, *greedy[k].shape[2:])), k
    a = m.rollout_from_context(base, path, n_samples=S, top_k=0, seed=5)
    b = m.rollout_from_context(base, path, n_samples=S, top_k=0, seed=5)
    c = m.rollout_from_context(base, path, n_samples=S, top_k=0, seed=6)
    short = m.rollout_from_context(base, path[:, :2], n_samples=S, top_k=0, seed=5)
    for k in ('codes', 'token_log_prob', 'log_likelihood'):
        assert torch.equal(a[k], b[k]), k
        assert torch.equal(short[k], a[k][:, :, :2]), k
    assert not torch.equal(a['codes'], c['codes'])
    assert not torch.equal(a['codes'][:, 0], a['codes'][:, 1])                           # the trajectories of a scene are independent draws
    assert bool(torch.isfinite(a['log_likelihood']).all()) and bool((a['log_likelihood'] < 0).all())
    # the definition WITH its noise: the explicit loop of sample_from_context(view0 = t, seed) and append_to_context draws what the
    # roll-out draws — for one trajectory per scene, and for S per scene on a cache replicated by hand, whose scene b S + s is
    # trajectory (b, s)
    one = m.rollout_from_context(m.prefill_context(codes[:, :C0], poses[:, :C0], capacity=C0 + T), path, top_k=0, seed=5, return_logits=True)
    lc, ll = _explicit_loop(m, m.prefill_context(codes[:, :C0], poses[:, :C0], capacity=C0 + T), path, top_k=0, seed=5)
    assert torch.equal(one['codes'][:, 0], lc) and torch.equal(one['logits'][:, 0], ll)
    assert not torch.equal(lc, one['logits'][:, 0].argmax(-1))                           # (the noise is in use)
    rep = m.prefill_context(codes[:, :C0].repeat_interleave(S, 0), poses[:, :C0].repeat_interleave(S, 0), capacity=C0 + T)
    lc, _ = _explicit_loop(m, rep, path.repeat_interleave(S, 0), top_k=0, seed=5)
    assert torch.equal(a['codes'].reshape(B4 * S, T, T_, T_), lc)


@pytest.mark.parametrize('arm', ['f32', 'bf16'])
def test_a_ragged_batch_rolls_out_from_each_scenes_own_views(dev, vq_m, arm):
    """(vi) ``n_context = [1, 3, 2, 3]``: scene 0's roll-out is ``torch.equal`` under a change of the other scenes' codes and cameras and
    of its own padding views; its new views go behind its ONE valid view.  (The fused step's two views per scene have the lengths p and
    p + 1 and, on the bf16 arm, half fill an attention group of four.)"""
    from viewformer_amd.render import ViewRenderer
    s = _model(dev, arm)
    m, codes, cams = s['m'], s['codes'], s['cams']
    C, T = 3, 3
    path = cams[:, 4:4 + T]
    r = ViewRenderer(m, vq_m).set_context(codes=codes[:, :C], cameras=cams[:, :C], n_context=[1, 3, 2, 3])
    a = r.rollout(path, return_codes=True)
    assert r.n_context.tolist() == [4, 6, 5, 6] and r.cache.C == 6 and tuple(r.context_codes.shape) == (B4, 6, T_, T_)
    assert torch.equal(r.context_codes[0, 1:4].long(), a['generated_codes'][0]) and torch.equal(r.context_codes[1, :3], codes[1, :C].to(dev))
    codes2, cams2, path2 = codes.clone(), cams.clone(), path.clone()
    codes2[1:, :C] = (codes2[1:, :C] + 17) % 1024
    codes2[0, 1:C] = (codes2[0, 1:C] + 5) % 1024
    cams2[1:, :C] = cams[1:, 1:C + 1]
    cams2[0, 1:C] = cams[0, 5:5 + C - 1]
    path2[1:] = cams[1:, 3:3 + T]
    b = ViewRenderer(m, vq_m).set_context(codes=codes2[:, :C], cameras=cams2[:, :C], n_context=[1, 3, 2, 3]).rollout(path2, return_codes=True)
    for k in a:
        assert torch.equal(a[k][0], b[k][0]), k
    assert not torch.equal(a['logits'][1], b['logits'][1])
    # scene 0 alone, from its one view: the same model answer at step 0, where both routes have the same inputs (row counts differ:
    # the arm's own bound — fp32: F32_LOGIT_TOL max(1, peak); bf16: BF16_LOGIT_TOL_REL peak)
    alone = ViewRenderer(m, vq_m).set_context(codes=codes[:1, :1], cameras=cams[:1, :1]).rollout(path[:1], return_codes=True)
    d = float((alone['logits'][0, 0] - a['logits'][0, 0]).abs().max())                  # step 0: the same inputs on both routes
    peak = float(alone['logits'].abs().max())
    parity_report(test='rollout_ragged_scene_vs_alone', arm=arm, B=B4, n_context=[1, 3, 2, 3], step0_logits_max_diff=d, peak=peak,
                  codes_equal=bool(torch.equal(alone['generated_codes'][0], a['generated_codes'][0])))
    assert d < (F32_LOGIT_TOL * max(1.0, peak) if arm == 'f32' else BF16_LOGIT_TOL_REL * peak)


@pytest.mark.parametrize('arm', ['f32', 'bf16'])
def test_a_rollout_that_is_not_kept_leaves_the_renderers_answers_as_they_were(dev, vq_m, arm):
    """(viii) ``keep=False``: ``render``'s logits before and after are ``torch.equal``, on a tight cache and on one with room (where the
    roll-out writes beyond the renderer's lengths into the buffers they share); with ``keep=True`` the context has grown and ``render``
    sees the generated frames"""
    from viewformer_amd.render import ViewRenderer
    s = _model(dev, arm)
    m, codes, cams = s['m'], s['codes'], s['cams']
    C, T = 2, 2
    path, q = cams[:, 4:4 + T], cams[:, 6:8]
    for capacity in (None, C + T + 1):
        r = ViewRenderer(m, vq_m).set_context(codes=codes[:, :C], cameras=cams[:, :C], capacity=capacity)
        before = r.render(q, return_codes=True)['logits']
        out = r.rollout(path, keep=False, return_codes=True)
        assert r.cache.C == C and r.n_context is None and tuple(r.context_codes.shape) == (B4, C, T_, T_)
        assert torch.equal(r.render(q, return_codes=True)['logits'], before), capacity
        many = r.rollout(path, n_samples=2, top_k=1, return_codes=True)              # S > 1 never replaces the renderer's cache
        assert r.cache.C == C and r.cache.B == B4 and tuple(many['generated_images'].shape) == (B4, 2, T, 128, 128, 3)
        assert torch.equal(many['generated_codes'][:, 0], out['generated_codes']) and torch.equal(many['generated_codes'][:, 1], out['generated_codes'])
        kept = r.rollout(path, return_codes=True)
        assert torch.equal(kept['generated_codes'], out['generated_codes']) and torch.equal(kept['logits'], out['logits'])
        assert r.cache.C == C + T and torch.equal(r.context_codes[:, C:].long(), kept['generated_codes'])
        assert not torch.equal(r.render(q, return_codes=True)['logits'], before)


# ---------------------------------------------------------------------------------------------- f32 arm against the model
def _four_criteria(label, got, full, ref, extra):
    """``got`` and ``full`` [B,...,nE] logits (fp64, CPU), ``ref`` the fp64 oracle for scene 0's leading entries [n,...,nE]: the criteria
    of tests/test_hip_render.py::test_f32_arm_cached_generation_equals_the_full_pass_within_its_own_error"""
    n = ref.shape[0]
    peak = float(ref.abs().max())
    e_full = float((full[0, :n] - ref).abs().max())
    e_got = float((got[0, :n] - ref).abs().max())
    marg = _margin(full)
    marg[0, :n] = _margin(ref)
    near = marg < 2 * (e_got + e_full)
    differ = got.argmax(-1) != full.argmax(-1)
    fig = dict(e_full=e_full, e_grown=e_got, peak=peak, bit_identical_to_full=bool(torch.equal(got, full)),
               max_grown_vs_full=float((got - full).abs().max()), rows=int(differ.numel()), rows_differing=int(differ.sum()),
               rows_near_tie=int(near.sum()), near_tie_share=float(near.float().mean()), min_margin=float(marg.min()), **extra)
    parity_report(test=label, **fig)
    assert e_got <= 1.5 * e_full, fig
    assert e_got < F32_LOGIT_TOL * max(1.0, peak), fig
    assert bool((~differ | near).all()), 'a generated code differs from the full pass outside the two paths\' error'
    assert float(near.float().mean()) <= NEAR_TIE_ROWS_MAX, fig
    return fig


def _oracle_last(sd, cfg, codes, poses):
    """fp64 oracle: the MASK view's logits [t,t,nE] behind ``codes`` [1,V,t,t] with ``poses`` [1,V+1,7]"""
    from oracle import migt_oracle as mg
    ids = torch.cat([codes.long(), torch.full_like(codes[:, :1].long(), cfg.n_embeddings)], 1)
    return mg.migt_forward(sd, cfg, ids.cpu(), poses.cpu(), dtype=torch.float64)['logits'][0, -1]


def test_f32_arm_a_grown_cache_equals_the_full_pass_within_its_own_error(dev):
    """B = 2, C0 = 2, K = 2 appended, N = 4 queries: the grown cache's logits against ``prefill_context`` of all 4 views, the full pass
    and the fp64 oracle (scene 0, queries 0 and 1).  The near-tie cap is evaluated at the measured errors, as in the existing tests: on
    a random-weight head the top-2 gap is about exponential with mean 0.08 peak, so at errors near 1e-5 the expected
    share of rows inside 2 (e_grown + e_full) is about 1e-4 — 0 of these 512 rows — and at the arm's bound it would be about 5 %: the
    cap binds only if the errors grow."""
    from viewformer_amd.migt import MIGT
    from viewformer_amd.weights import make_migt_weights
    B, C0, K, N = 2, 2, 2, 4
    cfg = _cfg()
    sd = make_migt_weights(cfg, seed=0, std=0.03)
    m = MIGT(cfg).load_state_dict(sd).to(dev)
    codes, poses, _ = _scene(B, C0 + K + N, 181)
    cpos, qpos = poses[:, :C0 + K].contiguous(), poses[:, C0 + K:].contiguous()
    ctx = codes[:, :C0 + K]
    cache = m.prefill_context(ctx[:, :C0], cpos[:, :C0])
    m.append_to_context(cache, ctx[:, C0:], cpos[:, C0:])
    grown = m.generate_from_context(cache, qpos, codes_only=False).cpu().double()
    whole = m.generate_from_context(m.prefill_context(ctx, cpos), qpos, codes_only=False).cpu().double()
    full = _full_logits(m, ctx, cpos, qpos).cpu().double()
    ref = torch.stack([_oracle_last(sd, cfg, ctx[:1], torch.cat([cpos[:1], qpos[:1, n:n + 1]], 1)) for n in (0, 1)])
    e_whole = float((whole[0, :2] - ref).abs().max())
    _four_criteria('grown_cache_f32_arm', grown, full, ref,
                   dict(B=B, C0=C0, K=K, N=N, e_prefill_of_all=e_whole, bit_identical_to_prefill_of_all=bool(torch.equal(grown, whole)),
                        max_grown_vs_prefill_of_all=float((grown - whole).abs().max())))
    e_grown = float((grown[0, :2] - ref).abs().max())
    assert e_grown <= 1.5 * e_whole, (e_grown, e_whole)
    differ = grown.argmax(-1) != whole.argmax(-1)
    assert bool((~differ | (_margin(whole) < 2 * (e_grown + e_whole))).all())


def test_f32_arm_a_teacher_forced_rollout_equals_the_full_pass_within_its_own_error(dev):
    """B = 2, C0 = 2, T = 3: step t's logits against the full pass and the oracle (scene 0) on [context, the roll-out's OWN generated maps
    0 ... t-1, MASK], so that a flipped near-tie token cannot compound.  Same four criteria, over the 3 x 128 rows of all steps."""
    from viewformer_amd.migt import MIGT
    from viewformer_amd.weights import make_migt_weights
    B, C0, T = 2, 2, 3
    cfg = _cfg()
    sd = make_migt_weights(cfg, seed=0, std=0.03)
    m = MIGT(cfg).load_state_dict(sd).to(dev)
    codes, poses, _ = _scene(B, C0 + T, 191)
    ctx, cpos, path = codes[:, :C0], poses[:, :C0].contiguous(), poses[:, C0:].contiguous()
    out = m.rollout_from_context(m.prefill_context(ctx, cpos), path, return_logits=True)
    gen = out['codes'][:, 0].cpu().to(torch.int32)                                    # [B,T,t,t]
    got = out['logits'][:, 0].cpu().double()                                         # [B,T,t,t,nE]
    assert out['cache'].C == C0 + T
    full, ref = [], []
    for t in range(T):
        seq = torch.cat([ctx, gen[:, :t]], 1)
        full.append(_full_logits(m, seq, torch.cat([cpos, path[:, :t]], 1), path[:, t:t + 1])[:, 0])
        ref.append(_oracle_last(sd, cfg, seq[:1], torch.cat([cpos[:1], path[:1, :t + 1]], 1)))
    full, ref = torch.stack(full, 1).cpu().double(), torch.stack(ref)
    _four_criteria('teacher_forced_rollout_f32_arm', got, full, ref, dict(B=B, C0=C0, T=T))


# ---------------------------------------------------------------------------------------------- bf16 arm on peaked logits
def test_bf16_arm_grown_cache_and_rollout_on_a_trained_model_with_peaked_logits(dev, trained):
    """the trained, peaked model of tests/test_hip_render.py.  Appended cache: context views 0, 1, views 2, 3 appended, queries at the
    training pose 4 and a novel pose between views 1 and 2; teacher-forced roll-out: context 0, 1, path = the training poses 2, 3, 4, step t against the full pass on
    [context, the roll-out's own maps, MASK].  Logits within BF16_LOGIT_TOL_REL peak of the f32 arm's full pass, code agreement with the
    bf16 full pass at least PEAKED_CODE_AGREEMENT."""
    from viewformer_amd.migt import MIGT
    cfg, sd, codes, poses = trained['cfg'], trained['sd'], trained['codes'].to(torch.int32), trained['poses']
    B, C0, K, T = codes.shape[0], 2, 2, 3
    ctx, cpos = codes[:, :C0 + K], poses[:, :C0 + K].contiguous()
    qpos, path = torch.stack([poses[:, 4], _interpolate(poses[:, 1], poses[:, 2], 0.5)], 1), poses[:, C0:C0 + T].contiguous()
    m16 = MIGT(cfg, precision='bf16').load_state_dict(sd).to(dev)
    cache = m16.prefill_context(ctx[:, :C0], cpos[:, :C0])
    m16.append_to_context(cache, ctx[:, C0:], cpos[:, C0:])
    lg = m16.generate_from_context(cache, qpos, codes_only=False).cpu().double()
    l16 = _full_logits(m16, ctx, cpos, qpos).cpu().double()
    out = m16.rollout_from_context(m16.prefill_context(ctx[:, :C0], cpos[:, :C0]), path, return_logits=True)
    gen, rl = out['codes'][:, 0].cpu().to(torch.int32), out['logits'][:, 0].cpu().double()
    seqs = [(torch.cat([ctx[:, :C0], gen[:, :t]], 1), torch.cat([cpos[:, :C0], path[:, :t]], 1), path[:, t:t + 1]) for t in range(T)]
    r16 = torch.stack([_full_logits(m16, *sq)[:, 0] for sq in seqs], 1).cpu().double()
    del m16
    m32 = MIGT(cfg, precision='f32').load_state_dict(sd).to(dev)
    l32 = _full_logits(m32, ctx, cpos, qpos).cpu().double()
    r32 = torch.stack([_full_logits(m32, *sq)[:, 0] for sq in seqs], 1).cpu().double()
    del m32
    peak = float(l32[:, 0].abs().max())                                              # at a training target pose, as the existing test
    fig = dict(train_steps=trained['steps'], final_ce=trained['ce'], peak=peak, peak_rollout=float(r32.abs().max()),
               d_grown_max=float((lg - l32).abs().max()), d_full_max=float((l16 - l32).abs().max()),
               grown_vs_full_bf16_max=float((lg - l16).abs().max()),
               code_agreement_grown_vs_full=float((lg.argmax(-1) == l16.argmax(-1)).float().mean()),
               d_rollout_max=float((rl - r32).abs().max()), d_rollout_full_max=float((r16 - r32).abs().max()),
               rollout_vs_full_bf16_max=float((rl - r16).abs().max()),
               code_agreement_rollout_vs_full=float((rl.argmax(-1) == r16.argmax(-1)).float().mean()),
               code_agreement_rollout_vs_f32=float((rl.argmax(-1) == r32.argmax(-1)).float().mean()))
    parity_report(test='rollout_bf16_arm_peaked', B=B, C0=C0, K=K, T=T, **fig)
    assert peak >= PEAKED_MIN_MAX_LOGIT, f'training did not produce a peaked head: max |logit| {peak:.2f} after {trained["steps"]} steps'
    assert torch.equal(gen.long(), rl.argmax(-1))
    assert fig['d_grown_max'] < BF16_LOGIT_TOL_REL * peak, fig
    assert fig['code_agreement_grown_vs_full'] >= PEAKED_CODE_AGREEMENT, fig
    assert fig['d_rollout_max'] < BF16_LOGIT_TOL_REL * peak, fig
    assert fig['code_agreement_rollout_vs_full'] >= PEAKED_CODE_AGREEMENT, fig


# ---------------------------------------------------------------------------------------------- the renderer
@pytest.mark.parametrize('augment', ['relative', 'no'])
def test_rollout_views_decodes_the_models_codes_from_world_frame_cameras(dev, vq_m, augment):
    """``rollout_views`` (images in, world-frame cameras) against the model-level roll-out on the encoder's codes and the poses of
    ``context_poses`` / ``query_poses``; ``append(images=...)`` equals ``append(codes=encode(images))``"""
    from viewformer_amd.evaluate import _frames_for_encode
    from viewformer_amd.migt import MIGT
    from viewformer_amd.render import ViewRenderer, context_poses, query_poses, rollout_views
    from viewformer_amd.weights import make_migt_weights, synthetic_scene_batch
    B, C, T = 2, 2, 2
    cfg = _cfg(augment_poses=augment)
    m = MIGT(cfg).load_state_dict(make_migt_weights(cfg, seed=0, std=0.03)).to(dev)
    frames, cams = synthetic_scene_batch(B, C + T + 1, 128, seed=61)
    frames, cams = torch.from_numpy(frames), torch.from_numpy(cams)
    ctx_f, ctx_c, path = frames[:, :C], cams[:, :C], cams[:, C:C + T]
    got = rollout_views(m, vq_m, ctx_f, ctx_c, path, return_codes=True)
    assert got['generated_images'].dtype == torch.uint8 and tuple(got['generated_images'].shape) == (B, T, 128, 128, 3)
    assert tuple(got['log_likelihood'].shape) == (B, T) and tuple(got['logits'].shape) == (B, T, T_, T_, 1024)
    codes = vq_m.encode(_frames_for_encode(ctx_f.to(dev), vq_m.config.image_size))[-1].to(torch.int32).view(B, C, T_, T_)
    cpos, transform = context_poses(ctx_c.to(dev), augment)
    want = m.rollout_from_context(m.prefill_context(codes, cpos, capacity=C + T), query_poses(path.to(dev), transform), return_logits=True)
    assert torch.equal(got['generated_codes'], want['codes'][:, 0]) and torch.equal(got['logits'], want['logits'][:, 0])
    img, _ = ViewRenderer(m, vq_m)._decode(want['codes'].reshape(B * T, T_, T_))
    assert torch.equal(got['generated_images'].reshape(B * T, 128, 128, 3), img)
    # append: images are encoded once, as set_context encodes them
    q = cams[:, C + T:]
    a = ViewRenderer(m, vq_m).set_context(images=ctx_f, cameras=ctx_c)
    a.append(images=frames[:, C:C + T], cameras=path)
    new_codes = vq_m.encode(_frames_for_encode(frames[:, C:C + T].to(dev), vq_m.config.image_size))[-1].view(B, T, T_, T_)
    b = ViewRenderer(m, vq_m).set_context(codes=codes, cameras=ctx_c).append(codes=new_codes, cameras=path)
    assert a.cache.C == C + T and torch.equal(a.context_codes, b.context_codes) and torch.equal(a.context_codes[:, C:], new_codes.to(torch.int32))
    la, lb = a.render(q, return_codes=True)['logits'], b.render(q, return_codes=True)['logits']
    assert torch.equal(la, lb)
    # ... and the grown context answers as the context of all views, within the arm's bound
    whole = ViewRenderer(m, vq_m).set_context(images=frames[:, :C + T], cameras=cams[:, :C + T]).render(q, return_codes=True)['logits']
    d, peak = float((la - whole).abs().max()), float(whole.abs().max())
    parity_report(test='renderer_append_vs_set_context_of_all', augment=augment, B=B, C=C, K=T, logits_max_diff=d, peak=peak,
                  bit_identical=bool(torch.equal(la, whole)))
    assert d < 2 * F32_LOGIT_TOL * max(1.0, peak)


def test_wrong_shapes_foreign_caches_the_fp8_arm_and_no_samples_are_refused(dev, vq_m):
    from viewformer_amd import _lib
    from viewformer_amd.migt import MIGT
    from viewformer_amd.render import ViewRenderer
    from viewformer_amd.weights import make_migt_weights
    s = _model(dev, 'f32')
    m, codes, poses, cams = s['m'], s['codes'], s['poses'], s['cams']
    cache = m.prefill_context(codes[:, :2], poses[:, :2], capacity=4)
    one, cam1 = codes[:, 2:3], poses[:, 2:3]
    for bad_codes, bad_cams in ((codes[:3, 2:3], cam1), (one, poses[:, 2:4]), (one.float(), cam1), (one[:, :, :4], cam1), (one, cam1[..., :6]),
                                (one.reshape(B4, 1, 64), cam1)):
        with pytest.raises(ValueError):
            m.append_to_context(cache, bad_codes, bad_cams)
    for bad_path in (poses[:3, 2:4], poses[:, 2:4, :6], poses[0, 2:4]):
        with pytest.raises(ValueError):
            m.rollout_from_context(cache, bad_path)
    for bad in (dict(n_samples=0), dict(n_samples=-1), dict(n_samples=1.5), dict(temperature=0.0), dict(top_p=0.0), dict(top_k=-1)):
        with pytest.raises(ValueError):
            m.rollout_from_context(cache, poses[:, 2:4], **bad)
    with pytest.raises(TypeError):
        m.append_to_context(cache.kv, one, cam1)
    with pytest.raises(TypeError):
        m.rollout_from_context(None, poses[:, 2:4])
    for bad in (1, 1.5, True):
        with pytest.raises(ValueError):
            m.prefill_context(codes[:, :2], poses[:, :2], capacity=bad)
    assert cache.C == 2 and cache.capacity == 4                          # nothing was launched, nothing grew
    cfg2 = _cfg(n_layer=2)
    other = MIGT(cfg2).load_state_dict(make_migt_weights(cfg2, seed=0)).to(dev)
    with pytest.raises(ValueError):                                      # a foreign cache
        other.append_to_context(cache, one, cam1)
    with pytest.raises(ValueError):
        other.rollout_from_context(cache, poses[:, 2:4])
    fp8 = MIGT(cfg2, precision='bf16', attention='fp8').load_state_dict(make_migt_weights(cfg2, seed=0)).to(dev)
    with pytest.raises(_lib.VfError):                                    # the fp8 attention arm has no cached contexts, growing or not
        fp8.append_to_context(cache, one, cam1)
    with pytest.raises(_lib.VfError):
        fp8.rollout_from_context(cache, poses[:, 2:4])
    with pytest.raises(_lib.VfError):
        ViewRenderer(fp8, vq_m).set_context(codes=codes[:, :2], cameras=cams[:, :2], capacity=4)
    r = ViewRenderer(m, vq_m).set_context(codes=codes[:, :2], cameras=cams[:, :2])
    for kw in (dict(codes=one, cameras=cams[:, 2:4]), dict(codes=one, cameras=cams[:3, 2:3]), dict(codes=one), dict(cameras=cams[:, 2:3]),
               dict(codes=one, images=torch.zeros(B4, 1, 128, 128, 3, dtype=torch.uint8), cameras=cams[:, 2:3]),
               dict(images=torch.zeros(B4, 2, 128, 128, 3, dtype=torch.uint8), cameras=cams[:, 2:3])):
        with pytest.raises(ValueError):
            r.append(**kw)
    for bad in (0, -2, 1.5):
        with pytest.raises(ValueError):
            r.rollout(cams[:, 2:4], n_samples=bad)
    with pytest.raises(ValueError):
        r.rollout(cams[:3, 2:4])
    assert r.cache.C == 2
