"""GPU: GROWING packed context caches (``ContextCache.pack(room=...)``, ``MIGT.prefill_context(pack=...)``,
``append_to_context`` / ``rollout_from_context`` on them, ``ViewRenderer.set_context(pack=...)``).

The K/V-only growing form holds the plain cache's own K and V values and walks them with the same kernels: every answer is
``torch.equal`` to that of a plain cache grown the same way, on both arms.  The e4m3 growing form (bf16 arm): the first view of an append
pass gets the bits of the same pass on ``unpack()``, and what is stored for it is the restatement's ``pack_tiles`` of what the plain
cache stores; later views of a pass read the earlier ones quantised, so the exact reference for K views is the loop ``unpack()`` ->
``append_to_context(view j)`` -> ``pack('e4m3')``, compared BY VALUE (re-packing dequantised tiles keeps every value and may pick a
smaller scale: tests/test_pack_grow_host.py).  Full-size models and the scenes of tests/test_hip_pack.py, 4 scenes: every pass has a
multiple of 256 rows.  Every case goes through ``conftest.parity_report`` (profiles/pack_grow_parity.txt keeps a run's lines)."""
import pytest
import torch

import kv_pack_ref as R
from conftest import parity_report
from test_hip_fp8 import FP8_LOGIT_TOL_REL
from test_hip_pack import ARMS, B_, C0, L, T_, _answers, _equal, _model, _source
from test_hip_rollout import _explicit_loop

pytestmark = pytest.mark.gpu

D, H, NL = 768, 12, 12
ROOM = {'tight': 0, 'room': 3, 'ragged': 0}


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'needs the MI355X'
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def vq_m(dev, full_vq):
    from viewformer_amd.vqgan import VQGAN
    vcfg, vsd, _ = full_vq
    return VQGAN(vcfg, data_format='NHWC', conv_arith='x3h').load_state_dict(vsd).to(dev)


def _plain(s, kind):
    return _source(s, 'ragged' if kind == 'ragged' else 'tight')


def _growing(s, kind, form):
    return _plain(s, kind).pack(form, room=ROOM[kind])


def _new(s, a, b):
    return s['codes'][:, a:b].contiguous(), s['poses'][:, a:b].contiguous()


def _thirds(cache):
    """(K, V) [B, capacity, L, d] of every layer, as stored (plain and K/V-only) or dequantised (e4m3)"""
    if cache.packed is None:
        return [(kv.view(cache.B, cache.capacity, L, 3 * D)[..., 2 * D:], kv.view(cache.B, cache.capacity, L, 3 * D)[..., :D]) for kv in cache.kv]
    dt = torch.bfloat16 if cache.qkv16 else torch.float32
    return [(k.view(cache.B, cache.capacity, L, D), v.view(cache.B, cache.capacity, L, D)) for k, v in cache._thirds(dt)]


def _same_filled_views(a, b):
    """every filled view of every scene and layer holds equal K and V values in the two caches"""
    la, lb = a.filled(), b.filled()
    if la.tolist() != lb.tolist():
        return False
    for (ka, va), (kb, vb) in zip(_thirds(a), _thirds(b)):
        for s in range(a.B):
            n = int(la[s])
            if not (torch.equal(ka[s, :n], kb[s, :n]) and torch.equal(va[s, :n], vb[s, :n])):
                return False
    return True


def _queries(s, a=5):
    return s['poses'][:, a:a + 2].contiguous(), s['codes'][:, a:a + 2].contiguous()          # N = 2: 512 rows


# ---------------------------------------------------------------------------------------------- the K/V-only form: both arms, the plain cache's bits
@pytest.mark.parametrize('kind', ['tight', 'room', 'ragged'])
@pytest.mark.parametrize('arm', ARMS)
def test_a_growing_kv_cache_appends_with_the_bits_of_a_plain_cache(dev, arm, kind):
    from viewformer_amd.render import plan_cache_bytes
    s = _model(dev, arm)
    m = s['m']
    g = _growing(s, kind, None)
    assert g.packed == 'kv' and g.capacity == C0 + ROOM[kind] and g.C == C0 and g.filled().tolist() == _plain(s, kind).filled().tolist()
    eb = g.kv[0][0].element_size()
    assert g.nbytes() == plan_cache_bytes(B_, g.capacity, L, D, H, NL, eb, 'kv')
    qpos, photos = _queries(s)
    # 2 views at once
    p = m.append_to_context(_plain(s, kind), *_new(s, 3, 5))
    assert m.append_to_context(g, *_new(s, 3, 5)) is g
    assert g.C == p.C and g.capacity == p.capacity == 6 and _same_filled_views(g, p)
    _equal('grow_kv_vs_plain', arm, _answers(m, g, qpos, photos), _answers(m, p, qpos, photos), source=kind, how='2 at once')
    # one by one
    g1 = _growing(s, kind, None)
    for j in (3, 4):
        m.append_to_context(g1, *_new(s, j, j + 1))
    assert _same_filled_views(g1, p)
    assert torch.equal(m.generate_from_context(g1, qpos, codes_only=False), m.generate_from_context(p, qpos, codes_only=False))
    # past the capacity: the cache moves to buffers of twice the views and keeps every value
    held = [t for t in g.kv[0]]
    m.append_to_context(g, *_new(s, 5, 7))
    m.append_to_context(p, *_new(s, 5, 7))
    assert g.capacity == 12 and p.capacity == 12 and g.kv[0][0] is not held[0] and _same_filled_views(g, p)
    q7 = (s['poses'][:, 7:8].contiguous(), s['codes'][:, 7:8].contiguous())
    _equal('grow_kv_vs_plain', arm, _answers(m, g, *q7), _answers(m, p, *q7), source=kind, how='past the capacity')
    u = g.unpack()
    assert u.packed is None and u.capacity == 12 and _same_filled_views(u, p) and bool((u.kv[0][:, D:2 * D] == 0).all())


@pytest.mark.parametrize('arm', ARMS)
def test_a_growing_kv_cache_rolls_out_the_plain_caches_codes_and_logits(dev, arm):
    """C0 = 2, T = 3, room for one view (the roll-out reallocates): fused and two-pass, arg-max and seeded"""
    s = _model(dev, arm)
    m, codes, poses = s['m'], s['codes'], s['poses']
    T = 3
    path = poses[:, 4:4 + T].contiguous()
    new = lambda: m.prefill_context(codes[:, :2], poses[:, :2])
    for fused in (True, False):
        for kw in (dict(top_k=1), dict(top_k=0, seed=5)):
            a = m.rollout_from_context(new().pack(room=1), path, return_logits=True, fused_step=fused, **kw)
            b = m.rollout_from_context(new(), path, return_logits=True, fused_step=fused, **kw)
            keys = ('codes', 'logits', 'token_log_prob', 'log_likelihood')
            _equal('grow_kv_rollout_vs_plain', arm, {k: a[k] for k in keys}, {k: b[k] for k in keys}, fused=fused, **kw)
            assert a['cache'].packed == 'kv' and a['cache'].C == 2 + T and _same_filled_views(a['cache'], b['cache'])
    g = new().pack(room=T)
    many = m.rollout_from_context(g, path, n_samples=2, top_k=0, seed=5)       # S > 1: a replicated growing cache, the caller's untouched
    ref = m.rollout_from_context(new(), path, n_samples=2, top_k=0, seed=5)
    assert many['cache'] is not g and many['cache'].packed == 'kv' and many['cache'].B == 2 * B_ and g.C == 2
    assert torch.equal(many['codes'], ref['codes']) and torch.equal(many['log_likelihood'], ref['log_likelihood'])


# ---------------------------------------------------------------------------------------------- the e4m3 form (bf16 arm)
@pytest.mark.parametrize('kind', ['room', 'ragged'])
def test_the_first_appended_view_of_an_e4m3_cache_is_the_restatement_of_the_plain_append(dev, kind):
    s = _model(dev, 'bf16')
    m = s['m']
    P = _growing(s, kind, 'e4m3')
    U = P.unpack()
    lens = P.filled()
    assert U.packed is None and U.capacity == P.capacity and U.filled().tolist() == lens.tolist()
    m.append_to_context(P, *_new(s, 3, 4))
    m.append_to_context(U, *_new(s, 3, 4))
    assert P.capacity == U.capacity and P.filled().tolist() == (lens + 1).tolist()
    cap = P.capacity
    for i in (0, NL - 1):
        x = U.kv[i].float().cpu().view(B_, cap, L, 3, H, 64)
        kq, vq, ks, vs = (t.cpu() for t in P.kv[i])
        for b in range(B_):
            slot = int(lens[b])
            for name, tiles, q, sc in (('K', x[b, slot, :, 2].permute(1, 0, 2), kq, ks), ('V', x[b, slot, :, 0].permute(1, 2, 0), vq, vs)):
                rq, rs = R.pack_tiles(tiles.contiguous())
                same_s = torch.equal(sc.view(B_, cap, H)[b, slot].contiguous().view(torch.int32), rs.contiguous().view(torch.int32))
                same_q = torch.equal(q.view(B_, cap, H, 64, 64)[b, slot], rq.view(torch.uint8))
                if not (same_s and same_q):
                    parity_report(test='grow_e4m3_first_view_vs_restatement', source=kind, layer=i, scene=b, third=name, scales_equal=same_s, bytes_equal=same_q)
                assert same_s and same_q, (kind, i, b, name)
    parity_report(test='grow_e4m3_first_view_vs_restatement', source=kind, layers=[0, NL - 1], equal=True)


def _reference_loop(m, s, kind, views):
    """the exact reference for views appended to an e4m3 cache: one at a time through the plain form"""
    Pr = _plain(s, kind).pack('e4m3')
    for j in views:
        U = Pr.unpack()
        m.append_to_context(U, *_new(s, j, j + 1))
        Pr = U.pack('e4m3')
    return Pr


@pytest.mark.parametrize('kind', ['room', 'ragged'])
def test_an_e4m3_cache_grows_at_once_one_by_one_and_as_the_reference_loop_by_value(dev, kind):
    s = _model(dev, 'bf16')
    m = s['m']
    qpos, photos = _queries(s)
    P1 = m.append_to_context(_growing(s, kind, 'e4m3'), *_new(s, 3, 5))
    P2 = _growing(s, kind, 'e4m3')
    for j in (3, 4):
        m.append_to_context(P2, *_new(s, j, j + 1))
    Pr = _reference_loop(m, s, kind, (3, 4))
    assert P1.packed == 'e4m3' and P1.C == C0 + 2 and P1.capacity == 6 and Pr.capacity == C0 + 2
    for name, other in (('one by one', P2), ('reference loop', Pr)):
        same = _same_filled_views(P1, other)
        parity_report(test='grow_e4m3_by_value', source=kind, against=name, values_equal=same)
        assert same, name
    want = _answers(m, Pr, qpos, photos)
    _equal('grow_e4m3_vs_reference_loop', 'bf16', _answers(m, P1, qpos, photos), want, source=kind, how='2 at once')
    assert torch.equal(m.generate_from_context(P2, qpos, codes_only=False), want['logits'])
    for a, b in zip(P1.kv, P2.kv):                                             # at once and one by one: the same launches on the same values, so bytes too
        for x, y, n in zip(a, b, ('kq', 'vq', 'kscale', 'vscale')):
            x, y = x.view(B_, 6, -1), y.view(B_, 6, -1)
            assert all(torch.equal(x[i, :int(c)], y[i, :int(c)]) for i, c in enumerate(P1.filled())), n
    # growth past the capacity keeps bytes and scales
    before = [tuple(t.clone() for t in ts) for ts in P1.kv]
    m.append_to_context(P1, *_new(s, 5, 7))
    assert P1.capacity == 12 and P1.C == C0 + 4
    for ts, olds in zip(P1.kv, before):
        for t, o in zip(ts, olds):
            t, o = t.view(B_, 12, -1), o.view(B_, 6, -1)
            assert all(torch.equal(t[i, :int(c) - 2], o[i, :int(c) - 2]) for i, c in enumerate(P1.filled()))
    Pr2 = _reference_loop(m, s, kind, (3, 4, 5, 6))
    assert _same_filled_views(P1, Pr2)
    q7 = s['poses'][:, 7:8].contiguous()
    assert torch.equal(m.generate_from_context(P1, q7, codes_only=False), m.generate_from_context(Pr2, q7, codes_only=False))
    # whatever the slack holds changes nothing
    P3 = _growing(s, kind, 'e4m3')
    for kq, vq, ks, vs in P3.kv:
        for b, n in enumerate(P3.filled()):
            for t, junk in ((kq, 0xFF), (vq, 0xFF), (ks, float('nan')), (vs, float('nan'))):
                t.view(B_, P3.capacity, -1)[b, int(n):] = junk
    m.append_to_context(P3, *_new(s, 3, 5))
    assert _same_filled_views(P3, Pr)
    assert torch.equal(m.generate_from_context(P3, qpos, codes_only=False), want['logits'])


def test_an_e4m3_cache_rolls_out_the_same_bits_fused_two_pass_and_in_the_explicit_loop(dev):
    s = _model(dev, 'bf16')
    m, codes, poses = s['m'], s['codes'], s['poses']
    T, S = 3, 3
    path = poses[:, 4:4 + T].contiguous()
    new = lambda room: m.prefill_context(codes[:, :2], poses[:, :2]).pack('e4m3', room=room)
    fused = m.rollout_from_context(new(T), path, return_logits=True)
    two = m.rollout_from_context(new(1), path, return_logits=True, fused_step=False)       # (reallocates on the way)
    loop_cache = new(T)
    lc, ll = _explicit_loop(m, loop_cache, path, top_k=1)
    for k in ('codes', 'logits', 'token_log_prob', 'log_likelihood'):
        assert torch.equal(fused[k], two[k]), k
    assert torch.equal(fused['codes'][:, 0], lc) and torch.equal(fused['logits'][:, 0], ll)
    for c in (fused['cache'], two['cache'], loop_cache):
        assert c.packed == 'e4m3' and c.C == 2 + T
    assert _same_filled_views(fused['cache'], two['cache']) and _same_filled_views(fused['cache'], loop_cache)
    parity_report(test='grow_e4m3_rollout_routes', T=T, equal=True)
    # S trajectories per scene: a replicated growing cache, whose scene b S + s is trajectory (b, s) — as on a cache replicated by hand
    base = new(T)
    a = m.rollout_from_context(base, path, n_samples=S, top_k=0, seed=5)
    assert a['cache'] is not base and a['cache'].packed == 'e4m3' and a['cache'].B == B_ * S and base.C == 2 and base.B == B_
    from viewformer_amd.context_cache import GrowingE4M3Cache
    hand = GrowingE4M3Cache(m, [tuple(t.view(B_, base.capacity, *t.shape[1:]).repeat_interleave(S, 0).reshape(-1, *t.shape[1:]) for t in ts)
                                for ts in base.kv], B_ * S, base.C, base.tshape, base.capacity)
    b = m.rollout_from_context(hand, path.repeat_interleave(S, 0), top_k=0, seed=5)
    assert torch.equal(a['codes'].reshape(B_ * S, T, T_, T_), b['codes'][:, 0]) and torch.equal(a['log_likelihood'].reshape(-1, T), b['log_likelihood'][:, 0])
    assert not torch.equal(a['codes'][:, 0], a['codes'][:, 1])                 # independent draws


def test_a_grown_e4m3_cache_is_inside_the_projects_e4m3_bound_against_the_f32_arm(dev):
    """teacher-forced: the same two views (their true codes) appended on the e4m3 growing cache and on the f32 arm's plain cache, then
    the logits of ``generate_from_context`` relative to max |logit|: below FP8_LOGIT_TOL_REL = 1.5e-1, the project's bound for its e4m3
    arm.  The plain bf16 cache's error and the agreement of a free-running roll-out's codes with the plain bf16 cache's are recorded,
    not asserted."""
    s32, s16 = _model(dev, 'f32'), _model(dev, 'bf16')
    qpos, _ = _queries(s16)
    ref = s32['m'].generate_from_context(s32['m'].append_to_context(_plain(s32, 'tight'), *_new(s32, 3, 5)), qpos, codes_only=False)
    lg16 = s16['m'].generate_from_context(s16['m'].append_to_context(_plain(s16, 'tight'), *_new(s16, 3, 5)), qpos, codes_only=False)
    lgq = s16['m'].generate_from_context(s16['m'].append_to_context(_growing(s16, 'room', 'e4m3'), *_new(s16, 3, 5)), qpos, codes_only=False)
    top = ref.abs().max().item()
    e_q, e_16 = (lgq - ref).abs().max().item() / top, (lg16 - ref).abs().max().item() / top
    path = s16['poses'][:, 4:7].contiguous()
    m = s16['m']
    ro_q = m.rollout_from_context(_growing(s16, 'room', 'e4m3'), path)['codes']
    ro_16 = m.rollout_from_context(_plain(s16, 'tight'), path)['codes']
    parity_report(test='grow_e4m3_accuracy', rel_logit_err_e4m3=e_q, rel_logit_err_bf16=e_16, logit_max=top, bound=FP8_LOGIT_TOL_REL,
                  argmax_agreement_with_bf16=(lgq.argmax(-1) == lg16.argmax(-1)).float().mean().item(),
                  rollout_code_agreement_with_bf16=(ro_q == ro_16).float().mean().item())
    assert e_q < FP8_LOGIT_TOL_REL


# ---------------------------------------------------------------------------------------------- prefill straight into a growing packed cache
@pytest.mark.parametrize('arm,form', [('f32', 'kv'), ('bf16', 'kv'), ('bf16', 'e4m3')])
def test_prefill_into_a_packed_cache_equals_prefill_then_pack_in_every_tensor(dev, arm, form):
    s = _model(dev, arm)
    m, codes, poses = s['m'], s['codes'][:, :C0].contiguous(), s['poses'][:, :C0].contiguous()
    dtype = None if form == 'kv' else form
    peaks = {}
    for capacity in (None, C0 + 3):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        a = m.prefill_context(codes, poses, capacity=capacity, pack=form)
        torch.cuda.synchronize()
        peaks['direct'] = torch.cuda.max_memory_allocated() - base
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        b = m.prefill_context(codes, poses).pack(dtype, room=0 if capacity is None else capacity - C0)
        torch.cuda.synchronize()
        peaks['prefill_then_pack'] = torch.cuda.max_memory_allocated() - base
        assert type(a) is type(b) and a.packed == form and (a.B, a.C, a.capacity) == (b.B, b.C, b.capacity) == (B_, C0, capacity or C0)
        assert a.lengths is None and b.lengths is None and len(a.kv) == len(b.kv) == NL
        for i, (ta, tb) in enumerate(zip(a.kv, b.kv)):
            for x, y in zip(ta, tb):
                assert x.shape == y.shape and x.dtype == y.dtype
                bits = {1: torch.uint8, 2: torch.int16, 4: torch.int32}[x.element_size()]
                assert torch.equal(x.view(bits), y.view(bits)), (i, capacity)
        parity_report(test='prefill_pack_vs_prefill_then_pack', arm=arm, form=form, capacity=capacity, equal=True, cache_bytes=a.nbytes(),
                      peak_bytes_direct=peaks['direct'], peak_bytes_prefill_then_pack=peaks['prefill_then_pack'])
    qpos, _ = _queries(s)
    assert torch.equal(m.generate_from_context(a, qpos, codes_only=False), m.generate_from_context(b, qpos, codes_only=False))


# ---------------------------------------------------------------------------------------------- the renderer
def test_the_renderer_grows_a_packed_context_and_answers_as_the_model(dev, vq_m):
    from viewformer_amd.evaluate import _frames_for_encode
    from viewformer_amd.render import ViewRenderer, context_poses, query_poses, plan_cache_bytes
    from viewformer_amd.weights import synthetic_scene_batch
    s = _model(dev, 'bf16')
    m, codes, cams = s['m'], s['codes'], s['cams']
    cap = C0 + 3
    r = ViewRenderer(m, vq_m).set_context(codes=codes[:, :C0], cameras=cams[:, :C0], pack='e4m3', capacity=cap)
    assert r.cache.packed == 'e4m3' and r.cache.capacity == cap and r.context_bytes() == plan_cache_bytes(B_, cap, L, D, H, NL, 2, 'e4m3')
    frames, _ = synthetic_scene_batch(B_, 2, 128, seed=77)
    frames = torch.from_numpy(frames)
    new_cams = cams[:, 3:5]
    assert r.append(images=frames, cameras=new_cams) is r and r.cache.C == C0 + 2 and tuple(r.context_codes.shape) == (B_, C0 + 2, T_, T_)
    new_codes = vq_m.encode(_frames_for_encode(frames.to(dev), vq_m.config.image_size))[-1].view(B_, 2, T_, T_).to(torch.int32)
    assert torch.equal(r.context_codes[:, C0:], new_codes)
    want = m.prefill_context(codes[:, :C0], context_poses(cams[:, :C0].to(dev), m.config.augment_poses)[0], capacity=cap, pack='e4m3')
    m.append_to_context(want, new_codes, query_poses(new_cams.to(dev), r.transform))
    assert _same_filled_views(r.cache, want)
    q, photos = cams[:, 5:7], codes[:, 5:7]
    qpos = query_poses(q.to(dev), r.transform)
    out = r.render(q, return_codes=True)
    assert torch.equal(out['logits'], m.generate_from_context(want, qpos, codes_only=False))
    assert torch.equal(r.score(q, codes=photos)['log_likelihood'], m.score_from_context(want, qpos, photos)['log_likelihood'])
    assert torch.equal(r.localize(codes=photos, return_tokens=True)['pose_prediction'],
                       m.localize_from_context(want, photos, return_tokens=True)['pose_prediction'])
    assert torch.equal(r.sample(q, n_samples=2, seed=5, return_codes=True)['generated_codes'],
                       m.sample_from_context(want, qpos, n_samples=2, seed=5)['codes'])
    # keep=False leaves render's logits as they were; S > 1 never replaces the renderer's cache; keep=True grows it
    path = cams[:, 6:8]
    ro = r.rollout(path, keep=False, return_codes=True)
    assert r.cache.C == C0 + 2 and torch.equal(r.render(q, return_codes=True)['logits'], out['logits'])
    many = r.rollout(path, n_samples=2, top_k=1, return_codes=True)
    assert r.cache.C == C0 + 2 and r.cache.B == B_ and torch.equal(many['generated_codes'][:, 1], ro['generated_codes'])
    mo = m.rollout_from_context(want, query_poses(path.to(dev), r.transform), return_logits=True)
    kept = r.rollout(path, return_codes=True)
    assert torch.equal(kept['generated_codes'], ro['generated_codes']) and torch.equal(kept['generated_codes'], mo['codes'][:, 0])
    assert torch.equal(kept['logits'], mo['logits'][:, 0])
    assert r.cache.C == C0 + 4 and r.cache.packed == 'e4m3' and r.cache.capacity == 12 and torch.equal(r.context_codes[:, C0 + 2:].long(), kept['generated_codes'])
    assert r.context_bytes() == plan_cache_bytes(B_, 12, L, D, H, NL, 2, 'e4m3')
    # the refusals hold, and unpack() restores fork and refine
    for refused, args in ((r.fork, dict(S=2)), (r.score_gradient, dict(query_cameras=q, codes=photos)), (r.refine, dict(cameras0=q, codes=photos)),
                          (r.rollout, dict(path_cameras=path, n_samples=2, fork=True)), (r.pack, dict()), (r.pack, dict(room=1))):
        with pytest.raises(ValueError, match=r'unpack\(\)'):
            refused(**args)
    assert r.unpack() is r and r.cache.packed is None and r.cache.capacity == 12 and r.context_bytes() == plan_cache_bytes(B_, 12, L, D, H, NL, 2)
    assert r.fork(2).cache.forked()
    ref = r.refine(cameras0=q, codes=photos, steps=1)
    assert isinstance(ref, dict)
    # the one-call form
    from viewformer_amd.render import rollout_views
    one = rollout_views(m, vq_m, None, cams[:, :C0], cams[:, 4:6], codes=codes[:, :C0], pack='kv', return_codes=True)
    two = rollout_views(m, vq_m, None, cams[:, :C0], cams[:, 4:6], codes=codes[:, :C0], return_codes=True)
    assert torch.equal(one['generated_codes'], two['generated_codes']) and torch.equal(one['logits'], two['logits'])
    parity_report(test='grow_renderer', arm='bf16', form='e4m3', equal=True)
