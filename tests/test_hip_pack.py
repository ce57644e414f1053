"""GPU: packed context caches (``ContextCache.pack`` / ``unpack``, ``ViewRenderer.pack`` / ``unpack``).

The K/V-only form holds the source cache's own K and V values and is served by the same attention entries, so every answer is
``torch.equal`` to the plain cache's, on both arms.  The e4m3 form (bf16 arm) is served by ``vf_attn_prefix_q8_bf16``, whose bits are
those of the bf16 arm on the dequantised cache: every answer is ``torch.equal`` to that of ``unpack()``.  What the e4m3 form loses is the
quantisation alone, held to the project's bound for its e4m3 arm against the f32 arm.  Full-size models, 4 scenes, 2 query views per
scene: every pass has a multiple of 256 rows and the dense layers take one kernel whatever the call.  Every case goes through
``conftest.parity_report`` (profiles/pack_parity.txt keeps a run's lines)."""
import numpy as np
import pytest
import torch

from conftest import parity_report
from test_hip_fp8 import FP8_LOGIT_TOL_REL

pytestmark = pytest.mark.gpu

L, T_ = 64, 8                     # tokens per view, token image size
B_, C0 = 4, 3                     # scenes, photographs
RAGGED = [1, 3, 2, 3]
ARMS = ['f32', 'bf16']


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


def _model(dev, arm):
    """one set of weights (std 0.02) on both arms: the e4m3 accuracy is measured against the f32 arm on the same scenes"""
    if arm not in _models:
        from viewformer_amd.migt import MIGT
        from viewformer_amd.weights import make_migt_weights
        cfg = _cfg()
        sd = make_migt_weights(cfg, seed=0, std=0.02)
        codes, poses, cams = _scene(B_, 8, 211)
        _models[arm] = dict(cfg=cfg, m=MIGT(cfg, precision=arm).load_state_dict(sd).to(dev), codes=codes.to(dev), poses=poses.to(dev), cams=cams)
    return _models[arm]


def _source(s, kind):
    """a plain cache of the B_ scenes: 'tight', 'slack' (room for 2 more views) or 'ragged' (lengths RAGGED)"""
    m = s['m']
    if kind == 'slack':
        return m.prefill_context(s['codes'][:, :C0], s['poses'][:, :C0], capacity=C0 + 2)
    c = m.prefill_context(s['codes'][:, :C0], s['poses'][:, :C0])
    if kind == 'ragged':
        c.lengths = np.array(RAGGED, dtype=np.int32)
        c.C = int(c.lengths.max())
    return c


def _answers(m, cache, qpos, photos, n_context=None):
    """logits, cameras, pose tokens, token log-probabilities and samples (arg-max and seeded) of one cache"""
    kw = {} if n_context is None else dict(n_context=n_context)
    loc = m.localize_from_context(cache, photos, return_tokens=True, **kw)
    sc = m.score_from_context(cache, qpos, photos, **kw)
    s1 = m.sample_from_context(cache, qpos, n_samples=2, top_k=1, seed=3, **kw)
    s0 = m.sample_from_context(cache, qpos, n_samples=2, top_k=0, seed=11, **kw)
    return dict(logits=m.generate_from_context(cache, qpos, codes_only=False, **kw), codes=m.generate_from_context(cache, qpos, **kw),
                cameras=loc['cameras'], pose_tokens=loc['pose_prediction'], token_log_prob=sc['token_log_prob'],
                log_likelihood=sc['log_likelihood'], samples_top1=s1['codes'], samples_seeded=s0['codes'],
                samples_seeded_logp=s0['token_log_prob'])


def _equal(test, arm, got, want, **kw):
    for k in want:
        same = bool(torch.equal(got[k], want[k]))
        diff = 0.0 if same or not got[k].dtype.is_floating_point else float((got[k].double() - want[k].double()).abs().max())
        parity_report(test=test, arm=arm, what=k, equal=same, max_abs_diff=diff, **kw)
        assert same, (test, k, diff)


def _queries(s):
    return s['poses'][:, 4:6].contiguous(), s['codes'][:, 4:6].contiguous()          # N = 2: B_ * 2 * 64 = 512 rows


N_CONTEXT = {'tight': [None, [1, 3, 2, 0], [[0, 3], [2, 1], [3, 3], [1, 2]]],
             'slack': [None, 2],
             'ragged': [None, [[1, 0], [3, 2], [0, 2], [3, 1]]]}


# ---------------------------------------------------------------------------------------------- the K/V-only form: both arms, the source's bits
@pytest.mark.parametrize('kind', ['tight', 'slack', 'ragged'])
@pytest.mark.parametrize('arm', ARMS)
def test_the_kv_only_pack_answers_with_the_bits_of_its_source(dev, arm, kind):
    from viewformer_amd.render import plan_cache_bytes
    s = _model(dev, arm)
    m = s['m']
    src = _source(s, kind)
    before = [t.clone() for t in src.kv]
    p = src.pack()
    C = C0
    assert p.packed == 'kv' and p.B == B_ and p.C == C and p.capacity == C and src.packed is None
    assert (p.lengths is None) == (kind == 'tight') and p.filled().tolist() == src.filled().tolist()
    eb = src.kv[0].element_size()
    assert p.nbytes() == plan_cache_bytes(B_, C, L, 768, 12, 12, eb, 'kv') and 3 * p.nbytes() == 2 * plan_cache_bytes(B_, C, L, 768, 12, 12, eb)
    assert src.nbytes() == plan_cache_bytes(B_, src.capacity, L, 768, 12, 12, eb)
    qpos, photos = _queries(s)
    for n_ctx in N_CONTEXT[kind]:
        _equal('pack_kv_vs_plain', arm, _answers(m, p, qpos, photos, n_ctx), _answers(m, src, qpos, photos, n_ctx), source=kind, n_context=n_ctx)
    ib = torch.int16 if eb == 2 else torch.int32                                 # bits: the slack rows are uninitialised and may hold NaN
    assert all(torch.equal(a.view(ib), b.view(ib)) for a, b in zip(before, src.kv))      # the source is left untouched
    u = p.unpack()
    assert u.packed is None and u.capacity == C and u.filled().tolist() == src.filled().tolist()
    d = 768
    for t, kv in zip(u.kv, src.kv):
        full = kv.view(B_, src.capacity * L, 3 * d)[:, :C * L].reshape(-1, 3 * d)
        assert torch.equal(t[:, :d], full[:, :d]) and torch.equal(t[:, 2 * d:], full[:, 2 * d:]) and bool((t[:, d:2 * d] == 0).all())
    # ... and the unpacked cache grows again
    m.append_to_context(u, s['codes'][:, 6:7], s['poses'][:, 6:7])
    ref = m.append_to_context(_source(s, kind), s['codes'][:, 6:7], s['poses'][:, 6:7])
    assert torch.equal(m.generate_from_context(u, qpos, codes_only=False), m.generate_from_context(ref, qpos, codes_only=False))


# ---------------------------------------------------------------------------------------------- the e4m3 form: the bits of the dequantised cache
@pytest.mark.parametrize('kind', ['tight', 'slack', 'ragged'])
def test_the_e4m3_pack_answers_with_the_bits_of_its_dequantised_cache(dev, kind):
    import kv_pack_ref as R
    from viewformer_amd.render import plan_cache_bytes
    arm = 'bf16'
    s = _model(dev, arm)
    m = s['m']
    src = _source(s, kind)
    p = src.pack('e4m3')
    assert p.packed == 'e4m3' and p.C == C0 and p.capacity == C0 and p.filled().tolist() == src.filled().tolist()
    assert [tuple(t.shape) for t in p.kv[0]] == [(B_ * C0, 12, 64, 64)] * 2 + [(B_ * C0, 12)] * 2
    assert p.nbytes() == plan_cache_bytes(B_, C0, L, 768, 12, 12, 2, 'e4m3') and p.nbytes() < 0.34 * plan_cache_bytes(B_, C0, L, 768, 12, 12, 2)
    u = p.unpack()
    assert u.packed is None and u.kv[0].dtype == torch.bfloat16 and bool((u.kv[0][:, 768:1536] == 0).all())
    # layer 0 of the pack against the restatement on the source's values: scales bit for bit, values equal (views inside the lengths)
    d, lens = 768, src.filled()
    x = src.kv[0].float().cpu().view(B_, src.capacity, L, 3, 12, 64)[:, :C0]
    kq, vq, ks, vs = (t.cpu() for t in p.kv[0])
    for b in range(B_):
        n = int(lens[b])
        rq, rs = R.pack_tiles(x[b, :n, :, 2].permute(0, 2, 1, 3).contiguous())
        assert torch.equal(ks.view(B_, C0, 12)[b, :n].contiguous().view(torch.int32), rs.contiguous().view(torch.int32))
        assert torch.equal(R.unpack_tiles(kq.view(B_, C0, 12, 64, 64)[b, :n].contiguous(), ks.view(B_, C0, 12)[b, :n]), R.unpack_tiles(rq, rs))
        rq, rs = R.pack_tiles(x[b, :n, :, 0].permute(0, 2, 3, 1).contiguous())
        assert torch.equal(R.unpack_tiles(vq.view(B_, C0, 12, 64, 64)[b, :n].contiguous(), vs.view(B_, C0, 12)[b, :n]), R.unpack_tiles(rq, rs))
    qpos, photos = _queries(s)
    for n_ctx in N_CONTEXT[kind]:
        _equal('pack_e4m3_vs_unpacked', arm, _answers(m, p, qpos, photos, n_ctx), _answers(m, u, qpos, photos, n_ctx), source=kind, n_context=n_ctx)


def test_the_e4m3_pack_is_inside_the_projects_e4m3_bound_against_the_f32_arm(dev):
    """logits of ``generate_from_context`` on the e4m3 cache against the f32 arm's on the same scenes and weights, relative to max
    |logit|: below FP8_LOGIT_TOL_REL, the project's bound for its e4m3 arm (which rounds more operands than this does).  The plain bf16
    cache's error and the arg-max agreement with it are recorded, not asserted."""
    s32, s16 = _model(dev, 'f32'), _model(dev, 'bf16')
    qpos, _ = _queries(s16)
    ref = s32['m'].generate_from_context(_source(s32, 'tight'), qpos, codes_only=False)
    plain = _source(s16, 'tight')
    lg16 = s16['m'].generate_from_context(plain, qpos, codes_only=False)
    lgq = s16['m'].generate_from_context(plain.pack('e4m3'), qpos, codes_only=False)
    top = ref.abs().max().item()
    e_q, e_16 = (lgq - ref).abs().max().item() / top, (lg16 - ref).abs().max().item() / top
    agree = (lgq.argmax(-1) == lg16.argmax(-1)).float().mean().item()
    agree32 = (lgq.argmax(-1) == ref.argmax(-1)).float().mean().item()
    parity_report(test='pack_e4m3_accuracy', rel_logit_err_e4m3=e_q, rel_logit_err_bf16=e_16, logit_max=top, argmax_agreement_with_bf16=agree,
                  argmax_agreement_with_f32=agree32, bound=FP8_LOGIT_TOL_REL)
    assert e_q < FP8_LOGIT_TOL_REL


# ---------------------------------------------------------------------------------------------- the renderer
@pytest.mark.parametrize('form', [None, 'e4m3'])
def test_the_renderer_packs_in_place_and_unpack_restores_what_grows(dev, vq_m, form):
    from viewformer_amd.render import ViewRenderer, query_poses, plan_cache_bytes
    arm = 'bf16'
    s = _model(dev, arm)
    m, codes, cams = s['m'], s['codes'], s['cams']
    r = ViewRenderer(m, vq_m).set_context(codes=codes[:, :C0], cameras=cams[:, :C0])
    plain_bytes = r.context_bytes()
    assert plain_bytes == plan_cache_bytes(B_, C0, L, 768, 12, 12, 2)
    want_cache = r.cache.pack(form)
    assert r.pack(form) is r and r.cache.packed == ('kv' if form is None else 'e4m3')
    assert r.context_bytes() == plan_cache_bytes(B_, C0, L, 768, 12, 12, 2, r.cache.packed)
    assert (3 * r.context_bytes() == 2 * plain_bytes) if form is None else (r.context_bytes() < 0.34 * plain_bytes)
    q, photos = cams[:, 4:6], codes[:, 4:6]
    qpos = query_poses(q.to(dev), r.transform)
    out = r.render(q, return_codes=True)
    lg = m.generate_from_context(want_cache, qpos, codes_only=False)
    assert torch.equal(out['logits'], lg) and torch.equal(out['generated_codes'], m.generate_from_context(want_cache, qpos))
    img, _ = r._decode(out['generated_codes'].reshape(B_ * 2, T_, T_))
    assert torch.equal(out['generated_images'].reshape(B_ * 2, *img.shape[1:]), img)
    sc = r.score(q, codes=photos)
    assert torch.equal(sc['log_likelihood'], m.score_from_context(want_cache, qpos, photos)['log_likelihood'])
    assert torch.equal(r.localize(codes=photos, return_tokens=True)['pose_prediction'],
                       m.localize_from_context(want_cache, photos, return_tokens=True)['pose_prediction'])
    assert torch.equal(r.sample(q, n_samples=2, seed=5, return_codes=True)['generated_codes'],
                       m.sample_from_context(want_cache, qpos, n_samples=2, seed=5)['codes'])
    sw = r.sweep(q, return_codes=True)
    assert torch.equal(sw['generated_codes'][:, :, -1], out['generated_codes'])
    for refused, args in ((r.append, dict(codes=photos, cameras=q)), (r.rollout, dict(path_cameras=q)), (r.fork, dict(S=2)),
                          (r.score_gradient, dict(query_cameras=q, codes=photos)), (r.refine, dict(cameras0=q, codes=photos))):
        with pytest.raises(ValueError, match=r'unpack\(\)'):
            refused(**args)
    assert r.unpack() is r and r.cache.packed is None and r.context_bytes() == plain_bytes
    ro = r.rollout(q, return_codes=True, keep=False)
    ref = ViewRenderer(m, vq_m).set_context(codes=codes[:, :C0], cameras=cams[:, :C0])
    if form is None:                                                              # the K/V-only form comes back bit for bit
        assert torch.equal(ro['generated_codes'], ref.rollout(q, return_codes=True, keep=False)['generated_codes'])
    else:
        assert tuple(ro['generated_codes'].shape) == (B_, 2, T_, T_)
    parity_report(test='pack_renderer', arm=arm, form=str(form), plain_bytes=plain_bytes, equal=True)


# ---------------------------------------------------------------------------------------------- refusals
def test_packed_caches_refuse_what_grows_and_the_f32_arm_refuses_e4m3(dev):
    s = _model(dev, 'f32')
    m, codes, poses = s['m'], s['codes'], s['poses']
    src = _source(s, 'tight')
    with pytest.raises(ValueError, match=r"precision='bf16'"):
        src.pack('e4m3')
    with pytest.raises(ValueError, match=r'materialize\(\)'):
        src.fork(2).pack()
    p = src.pack()
    qpos, photos = _queries(s)
    for f in (lambda: m.append_to_context(p, photos, qpos), lambda: m.rollout_from_context(p, qpos), lambda: p.fork(2), lambda: p.pack(),
              lambda: m.score_grad_from_context(p, qpos, photos), lambda: m.refine_from_context(p, qpos, photos, steps=1)):
        with pytest.raises(ValueError, match=r'unpack\(\)'):
            f()
    with pytest.raises(ValueError, match='another model'):
        _model(dev, 'bf16')['m'].generate_from_context(p, qpos)
