"""GPU: forked context caches (``ContextCache.fork`` / ``materialize``, ``MIGT.rollout_from_context(fork=True)``,
``MIGT.adopt_from_fork``, ``ViewRenderer.fork`` / ``rollout(fork=, adopt=)``).

A child reads the parent's views where they lie and owns only what it adds; the attention walks the same keys in the same order with the
same arithmetic as on a replicated cache, so EVERY comparison here is ``torch.equal``: against ``child.materialize()``, against a
hand-replicated parent, against ``fork=False``.  Full-size models, 2 parent scenes, S = 2, N = 2: every pass has a multiple of 256 rows
and the dense layers take one kernel whatever the call.  Every case goes through ``conftest.parity_report``
(profiles/fork_parity.txt keeps a run's lines)."""
import numpy as np
import pytest
import torch

from conftest import parity_report

pytestmark = pytest.mark.gpu

L, T_ = 64, 8                     # tokens per view, token image size
B_, S_, C0, ROOM = 2, 2, 2, 3     # parent scenes, children per scene, photographs, room for 3 more views
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
    if arm not in _models:
        from viewformer_amd.migt import MIGT
        from viewformer_amd.weights import make_migt_weights
        cfg = _cfg()
        sd = make_migt_weights(cfg, seed=0, std=0.03 if arm == 'f32' else 0.02)
        codes, poses, cams = _scene(B_, 10, 191)
        _models[arm] = dict(cfg=cfg, m=MIGT(cfg, precision=arm).load_state_dict(sd).to(dev), codes=codes.to(dev), poses=poses.to(dev), cams=cams)
    return _models[arm]


def _parent(s, capacity=C0 + ROOM):
    return s['m'].prefill_context(s['codes'][:, :C0], s['poses'][:, :C0], capacity=capacity)


def _per_child(x, a, b):
    """views a ... b-1 of every parent scene dealt to its S_ children: [B_, (b-a), ...] -> [B_*S_, (b-a)/S_, ...]"""
    v = x[:, a:b]
    return v.reshape(B_ * S_, (b - a) // S_, *v.shape[2:]).contiguous()


def _answers(m, cache, qpos, photos):
    """logits, cameras, pose tokens, token log-probabilities and samples (arg-max and seeded) of one cache"""
    loc = m.localize_from_context(cache, photos, return_tokens=True)
    sc = m.score_from_context(cache, qpos, photos)
    s1 = m.sample_from_context(cache, qpos, n_samples=2, top_k=1, seed=3)
    s0 = m.sample_from_context(cache, qpos, n_samples=2, top_k=0, seed=11)
    return dict(logits=m.generate_from_context(cache, qpos, codes_only=False), cameras=loc['cameras'], pose_tokens=loc['pose_prediction'],
                token_log_prob=sc['token_log_prob'], log_likelihood=sc['log_likelihood'], samples_top1=s1['codes'], samples_seeded=s0['codes'],
                samples_seeded_logp=s0['token_log_prob'])


def _equal(test, arm, got, want, **kw):
    for k in want:
        same = bool(torch.equal(got[k], want[k]))
        diff = 0.0 if same or not got[k].dtype.is_floating_point else float((got[k].double() - want[k].double()).abs().max())
        parity_report(test=test, arm=arm, what=k, equal=same, max_abs_diff=diff, **kw)
        assert same, (test, k, diff)


def _thirds(kv, B, views, a, b):
    """the V and K thirds of views a ... b-1 of a per-layer buffer of ``views`` views per scene"""
    d = kv.shape[1] // 3
    v = kv.view(B, views, L, 3 * d)[:, a:b]
    return v[..., :d], v[..., 2 * d:]


def _own_equals_rows_of(child, plain, n_own):
    """the fork's own views 0 ... n_own-1 against the views behind each scene's split of a plain cache of the same scenes (equal splits)"""
    sp = int(child.split[0])
    assert (child.split == sp).all() and child.B == plain.B
    for own, kv in zip(child.kv, plain.kv):
        (v1, k1), (v2, k2) = _thirds(own, child.B, child.room, 0, n_own), _thirds(kv, plain.B, plain.capacity, sp, sp + n_own)
        if not (torch.equal(v1, v2) and torch.equal(k1, k2)):
            return False
    return True


# ---------------------------------------------------------------------------------------------- 1, 6
@pytest.mark.parametrize('arm', ARMS)
def test_a_fork_answers_as_its_materialised_cache_and_as_a_replicated_parent(dev, arm):
    s = _model(dev, arm)
    m, codes, poses = s['m'], s['codes'], s['poses']
    parent = _parent(s)
    qpos, photos = _per_child(poses, 4, 8), _per_child(codes, 4, 8)               # two different query views per sibling
    child = parent.fork(S_)
    assert child.B == B_ * S_ and child.share == S_ and child.room == 0 and child.split.tolist() == [C0] * 4 and child.C == C0
    assert all(tuple(t.shape) == (0, 3 * 768) for t in child.kv) and len(child.kv) == len(parent.kv)          # nothing allocated
    assert all(a is b for a, b in zip(child.parent_kv, parent.kv))
    want = _answers(m, m._replicate(parent, S_), qpos, photos)
    _equal('fork_vs_replicated', arm, _answers(m, child, qpos, photos), want, own_views=0)
    mat = child.materialize()
    assert not mat.forked() and mat.B == 4 and mat.filled().tolist() == [C0] * 4 and mat.kv[0].data_ptr() != parent.kv[0].data_ptr()
    _equal('materialised_vs_replicated', arm, _answers(m, mat, qpos, photos), want, own_views=0)
    # with own views: one appended view per sibling (a different one each), room for exactly it
    roomy = parent.fork(S_, room=1)
    assert all(tuple(t.shape) == (B_ * S_ * 1 * L, 3 * 768) for t in roomy.kv)                                 # B S room L rows per layer, nothing else
    nc, npose = _per_child(codes, 2, 4), _per_child(poses, 2, 4)
    m.append_to_context(roomy, nc, npose)
    rep = m.append_to_context(m._replicate(parent, S_), nc, npose)
    assert roomy.filled().tolist() == [C0 + 1] * 4 and roomy.room == 1 and roomy.capacity == C0 + 1
    want = _answers(m, rep, qpos, photos)
    _equal('fork_vs_replicated', arm, _answers(m, roomy, qpos, photos), want, own_views=1)
    mat = roomy.materialize()
    assert mat.filled().tolist() == [C0 + 1] * 4 and _own_equals_rows_of(roomy, mat, 1)
    _equal('materialised_vs_replicated', arm, _answers(m, mat, qpos, photos), want, own_views=1)
    # n_context may stop inside the parent, at the split, or inside the own views
    for n_ctx in (0, 1, C0, C0 + 1, [[0, 3], [1, 2], [3, 3], [2, 0]]):
        a = m.generate_from_context(roomy, qpos, codes_only=False, n_context=n_ctx)
        b = m.generate_from_context(rep, qpos, codes_only=False, n_context=n_ctx)
        parity_report(test='fork_n_context', arm=arm, n_context=n_ctx, equal=bool(torch.equal(a, b)))
        assert torch.equal(a, b), n_ctx
    with pytest.raises(ValueError):
        m.generate_from_context(roomy, qpos, n_context=C0 + 2)
    # the materialised cache is the route to the gradient
    g = m.score_grad_from_context(mat, qpos, photos)
    assert torch.equal(g['token_log_prob'], want['token_log_prob']) and torch.isfinite(g['grad_cameras']).all()


# ---------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize('arm', ARMS)
def test_appending_to_a_fork_at_once_one_by_one_and_past_its_room_gives_the_replicated_bits(dev, arm):
    s = _model(dev, arm)
    m, codes, poses = s['m'], s['codes'], s['poses']
    parent = _parent(s)
    nc, npose = _per_child(codes, 2, 6), _per_child(poses, 2, 6)                  # two different views per sibling
    qpos = _per_child(poses, 6, 10)
    rep = m.append_to_context(m._replicate(parent, S_), nc, npose)
    at_once = m.append_to_context(parent.fork(S_, room=ROOM), nc, npose)
    assert at_once.room == ROOM and at_once.filled().tolist() == [C0 + 2] * 4
    one = parent.fork(S_, room=1)
    first_own = one.kv[0]
    m.append_to_context(one, nc[:, :1], npose[:, :1])
    assert one.kv[0] is first_own and one.room == 1
    m.append_to_context(one, nc[:, 1:], npose[:, 1:])                             # past the room: the own buffers move, to max(2 room, needed)
    assert one.kv[0] is not first_own and one.room == 2 and one.capacity == C0 + 2 and one.filled().tolist() == [C0 + 2] * 4
    assert all(tuple(t.shape) == (B_ * S_ * 2 * L, 3 * 768) for t in one.kv)
    assert all(a is b for a, b in zip(one.parent_kv, parent.kv))                  # ... and only they
    lazy = parent.fork(S_)                                                        # no room at all until the first append
    m.append_to_context(lazy, nc, npose)
    assert lazy.room == 2
    want = m.generate_from_context(rep, qpos, codes_only=False)
    for name, c in (('at_once', at_once), ('one_by_one', one), ('no_room', lazy)):
        same = _own_equals_rows_of(c, rep, 2)
        lg = bool(torch.equal(m.generate_from_context(c, qpos, codes_only=False), want))
        parity_report(test='fork_append', arm=arm, route=name, own_thirds_equal=same, logits_equal=lg)
        assert same and lg, name


# ---------------------------------------------------------------------------------------------- 3, 6
@pytest.mark.parametrize('arm', ARMS)
def test_a_forked_rollout_equals_the_replicated_one(dev, arm):
    s = _model(dev, arm)
    m, poses = s['m'], s['poses']
    parent = _parent(s)
    T = 3
    path = poses[:, 4:4 + T]
    keys = ('codes', 'token_log_prob', 'log_likelihood', 'logits')
    seeded = {}
    for name, kw in (('fused', {}), ('two_pass', dict(fused_step=False)), ('top1', dict(top_k=1, seed=9)), ('seed1', dict(top_k=0, seed=1)),
                     ('seed2', dict(top_k=0, seed=2))):
        f = m.rollout_from_context(parent, path, n_samples=S_, fork=True, return_logits=True, **kw)
        r = m.rollout_from_context(parent, path, n_samples=S_, return_logits=True, **kw)
        _equal('fork_rollout', arm, {k: f[k] for k in keys}, {k: r[k] for k in keys}, route=name)
        fc = f['cache']
        assert fc.forked() and fc.share == S_ and fc.room == T and fc.filled().tolist() == [C0 + T] * 4 and not r['cache'].forked()
        assert all(tuple(t.shape) == (B_ * S_ * T * L, 3 * 768) for t in fc.kv)                                # B S T L rows per layer, nothing else
        assert all(a is b for a, b in zip(fc.parent_kv, parent.kv))
        assert _own_equals_rows_of(fc, r['cache'], T)
        seeded[name] = f
    assert not torch.equal(seeded['seed1']['codes'], seeded['seed2']['codes'])
    short = m.rollout_from_context(parent, path[:, :2], n_samples=S_, fork=True, return_logits=True, top_k=0, seed=1)
    _equal('fork_rollout_prefix', arm, {k: short[k] for k in keys}, {k: seeded['seed1'][k][:, :, :2] for k in keys})
    assert parent.filled().tolist() == [C0] * B_ and parent.capacity == C0 + ROOM
    # fork=True with one trajectory is today's roll-out; a fork rolls out as any cache (S = 1: in place, in its own buffers)
    one = m.rollout_from_context(_parent(s), path, fork=True)
    assert not one['cache'].forked() and torch.equal(one['codes'], m.rollout_from_context(_parent(s), path)['codes'])
    inplace = m.rollout_from_context(parent.fork(S_, room=T), path.repeat_interleave(S_, 0), top_k=0, seed=1)
    assert torch.equal(inplace['codes'].view(B_, S_, T, T_, T_), seeded['seed1']['codes'])


# ---------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize('arm', ARMS)
def test_the_parent_is_untouched_and_what_it_appends_later_reaches_no_child(dev, arm):
    s = _model(dev, arm)
    m, codes, poses = s['m'], s['codes'], s['poses']
    parent = _parent(s)
    q2 = poses[:, 8:10]
    before = [kv.clone() for kv in parent.kv]
    buffers = list(parent.kv)
    lg0 = m.generate_from_context(parent, q2, codes_only=False)
    qpos, photos = _per_child(poses, 4, 8), _per_child(codes, 4, 8)
    child = parent.fork(S_, room=1)
    m.append_to_context(child, _per_child(codes, 2, 4), _per_child(poses, 2, 4))
    m.rollout_from_context(child, _per_child(poses, 6, 10), top_k=0, seed=4)      # reallocates the child's own buffers
    m.rollout_from_context(parent, poses[:, 4:7], n_samples=S_, fork=True)
    child = parent.fork(S_, room=1)
    m.append_to_context(child, _per_child(codes, 2, 4), _per_child(poses, 2, 4))
    want = _answers(m, child, qpos, photos)
    # view 0 may hold NaN only in the Q third, which nothing reads again: compare the bits
    same = all(a is b and torch.equal(a.view(torch.int16 if a.dtype == torch.bfloat16 else torch.int32),
                                      c.view(torch.int16 if c.dtype == torch.bfloat16 else torch.int32))
               for a, b, c in zip(parent.kv, buffers, before))
    parity_report(test='fork_parent_untouched', arm=arm, equal=same)
    assert same and parent.filled().tolist() == [C0] * B_
    assert torch.equal(m.generate_from_context(parent, q2, codes_only=False), lg0)
    # the parent grows in the buffers it shares with the child: its new views land in rows split, split + 1 of every scene
    m.append_to_context(parent, codes[:, 6:8], poses[:, 6:8])
    assert parent.C == C0 + 2 and all(a is b for a, b in zip(child.parent_kv, parent.kv))
    _equal('fork_after_parent_append', arm, _answers(m, child, qpos, photos), want, parent_reallocated=False)
    m.append_to_context(parent, codes[:, 8:10], poses[:, 8:10])                   # past its capacity: the parent moves, the child keeps the old buffers
    assert parent.C == C0 + 4 and all(a is not b for a, b in zip(child.parent_kv, parent.kv)) and child.parent_capacity == C0 + ROOM
    _equal('fork_after_parent_append', arm, _answers(m, child, qpos, photos), want, parent_reallocated=True)
    with pytest.raises(ValueError, match='grown since the fork'):
        m.adopt_from_fork(parent, child, [0, 0])


# ---------------------------------------------------------------------------------------------- 5
@pytest.mark.parametrize('arm', ARMS)
def test_a_ragged_parent_forks_at_each_scenes_own_length(dev, arm):
    """n_context = [1, 2]: scene 0's children start behind its ONE valid view; they are unchanged under a change of the parent's padding
    view and of scene 1"""
    s = _model(dev, arm)
    m, codes, poses = s['m'], s['codes'], s['poses']
    T = 2
    path, qpos, photos = poses[:, 4:4 + T], _per_child(poses, 6, 10), _per_child(codes, 6, 10)

    def run(codes, poses):
        parent = m.prefill_context(codes[:, :C0], poses[:, :C0])
        parent.lengths, parent.C = np.array([1, 2], dtype=np.int32), 2          # as ViewRenderer.set_context(n_context=[1, 2]) leaves it before it grows
        child = parent.fork(S_, room=T)
        assert child.split.tolist() == [1, 1, 2, 2] and child.C == 2 and child.capacity == 2 + T
        out = m.rollout_from_context(child, path.repeat_interleave(S_, 0), top_k=0, seed=6, return_logits=True)
        assert child.filled().tolist() == [3, 3, 4, 4]
        res = _answers(m, child, qpos, photos)
        res.update(rollout_codes=out['codes'], rollout_logits=out['logits'])
        rep = m._replicate(parent, S_)
        ref = m.rollout_from_context(rep, path.repeat_interleave(S_, 0), top_k=0, seed=6, return_logits=True)
        assert torch.equal(out['codes'], ref['codes']) and torch.equal(out['logits'], ref['logits'])
        return res
    a = run(codes, poses)
    codes2, poses2 = codes.clone(), poses.clone()
    codes2[0, 1] = (codes2[0, 1] + 17) % 1024                                     # scene 0's padding view
    poses2[0, 1] = poses[0, 3]
    codes2[1, :C0] = (codes2[1, :C0] + 5) % 1024                                  # all of scene 1
    poses2[1, 1] = poses[1, 3]
    b = run(codes2, poses2)
    _equal('fork_ragged_parent', arm, {k: v[:S_] for k, v in b.items()}, {k: v[:S_] for k, v in a.items()})
    assert not torch.equal(a['logits'][S_:], b['logits'][S_:])


# ---------------------------------------------------------------------------------------------- 7
@pytest.mark.parametrize('arm', ARMS)
def test_adopting_a_child_leaves_the_parent_as_if_its_views_had_been_appended(dev, arm):
    s = _model(dev, arm)
    m, poses = s['m'], s['poses']
    T = 2
    path, q2 = poses[:, 4:4 + T], poses[:, 8:10]
    parent = _parent(s)
    out = m.rollout_from_context(parent, path, n_samples=S_, fork=True, top_k=0, seed=5)
    which = m.adopt_from_fork(parent, out['cache'], [1, 0])
    assert which.tolist() == [1, 0] and parent.filled().tolist() == [C0 + T] * B_
    chosen = out['codes'][torch.arange(B_, device=dev), torch.tensor([1, 0], device=dev)]        # [B,T,t,t]
    ref = m.append_to_context(_parent(s), chosen, path)
    thirds = all(torch.equal(a, b) for kv1, kv2 in zip(parent.kv, ref.kv)
                 for a, b in zip(_thirds(kv1, B_, parent.capacity, 0, C0 + T), _thirds(kv2, B_, ref.capacity, 0, C0 + T)))
    lg = bool(torch.equal(m.generate_from_context(parent, q2, codes_only=False), m.generate_from_context(ref, q2, codes_only=False)))
    parity_report(test='fork_adopt', arm=arm, which=[1, 0], thirds_equal=thirds, logits_equal=lg)
    assert thirds and lg
    with pytest.raises(ValueError, match='grown since the fork'):                 # the parent has moved on: its other children are of the past
        m.adopt_from_fork(parent, out['cache'], [0, 0])
    # 'best': the largest sum of log_likelihood over T, in fp32 and in order; ties go to the lowest index
    parent = _parent(s, capacity=C0)                                              # a tight parent: adopting reallocates it
    out = m.rollout_from_context(parent, path, n_samples=S_, fork=True, top_k=0, seed=5)
    ll = out['log_likelihood'].cpu().numpy()
    brute = []
    for b in range(B_):
        tot = [np.float32(0)] * S_
        for t in range(T):
            tot = [np.float32(tot[j] + ll[b, j, t]) for j in range(S_)]
        brute.append(max(range(S_), key=lambda j: (tot[j], -j)))
    got = m.adopt_from_fork(parent, out['cache'], 'best', score=out['log_likelihood'])
    assert got.tolist() == brute and parent.capacity >= C0 + T
    best = out['codes'][torch.arange(B_, device=dev), torch.from_numpy(got).to(dev)]
    ref = m.append_to_context(_parent(s), best, path)
    assert torch.equal(m.generate_from_context(parent, q2, codes_only=False), m.generate_from_context(ref, q2, codes_only=False))
    tie = _parent(s)
    assert m.adopt_from_fork(tie, m.rollout_from_context(tie, path, n_samples=S_, fork=True)['cache'], 'best',
                             score=torch.tensor([[1.0, 1.0], [0.0, 2.0]], device=dev)).tolist() == [0, 1]


# ---------------------------------------------------------------------------------------------- 8
def test_the_renderer_forks_rolls_out_and_adopts(dev, vq_m):
    from viewformer_amd.render import ViewRenderer, query_poses
    arm = 'bf16'
    s = _model(dev, arm)
    m, codes, cams = s['m'], s['codes'], s['cams']
    T = 2
    r = ViewRenderer(m, vq_m).set_context(codes=codes[:, :C0], cameras=cams[:, :C0], capacity=C0 + ROOM)
    path = cams[:, 4:4 + T]
    want = m.rollout_from_context(r.cache.alias(), query_poses(path.to(dev), r.transform), n_samples=S_, top_k=0, seed=3)
    img, _ = r._decode(want['codes'].reshape(B_ * S_ * T, T_, T_))
    # a forked renderer: B S scenes, its own roll-out kept in its own context, the parent as it was
    rf = r.fork(S_)
    assert rf.transformer is m and rf.codebook is vq_m and rf.cache.forked() and rf.cache.B == B_ * S_
    assert tuple(rf.context_codes.shape) == (B_ * S_, C0, T_, T_) and torch.equal(rf.context_codes[1], r.context_codes[0]) and rf.n_context is None
    out = rf.rollout(path.repeat_interleave(S_, 0), top_k=0, seed=3, return_codes=True)
    assert torch.equal(out['generated_codes'].reshape(B_, S_, T, T_, T_), want['codes'])
    assert torch.equal(out['generated_images'].reshape(B_ * S_ * T, *img.shape[1:]), img)
    assert rf.cache.filled().tolist() == [C0 + T] * 4 and torch.equal(rf.context_codes[:, C0:], want['codes'].reshape(B_ * S_, T, T_, T_).to(torch.int32))
    lg = rf.render(cams[:, 8:10].repeat_interleave(S_, 0), return_codes=True)['logits']
    assert torch.equal(lg, m.generate_from_context(want['cache'], query_poses(cams[:, 8:10].to(dev), r.transform).repeat_interleave(S_, 0),
                                                   codes_only=False))
    rf.append(codes=codes[:, 6:7].repeat_interleave(S_, 0), cameras=cams[:, 6:7].repeat_interleave(S_, 0))
    assert rf.cache.C == C0 + T + 1 and r.cache.C == C0 and tuple(r.context_codes.shape) == (B_, C0, T_, T_)
    for refused in (rf.score_gradient, rf.refine):
        with pytest.raises(ValueError, match=r'materialize\(\)'):
            refused(cams[:, 8:9].repeat_interleave(S_, 0), codes=codes[:, 8:9].repeat_interleave(S_, 0))
    # rollout(fork=True, adopt='best'): one trajectory per scene stays
    out = r.rollout(path, n_samples=S_, top_k=0, seed=3, return_codes=True, fork=True, adopt='best')
    assert torch.equal(out['generated_codes'], want['codes']) and torch.equal(out['generated_images'].reshape(B_ * S_ * T, *img.shape[1:]), img)
    tot = want['log_likelihood'][:, :, 0]
    for t in range(1, T):
        tot = tot + want['log_likelihood'][:, :, t]
    brute = [max(range(S_), key=lambda j: (float(tot[b, j]), -j)) for b in range(B_)]
    assert out['adopted'].tolist() == brute
    kept = want['codes'][torch.arange(B_, device=dev), out['adopted'].to(dev)]
    assert r.cache.C == C0 + T and not r.cache.forked() and r.n_context is None
    assert tuple(r.context_codes.shape) == (B_, C0 + T, T_, T_) and torch.equal(r.context_codes[:, C0:], kept.to(torch.int32))
    ref = ViewRenderer(m, vq_m).set_context(codes=codes[:, :C0], cameras=cams[:, :C0], capacity=C0 + ROOM).append(codes=kept, cameras=path)
    q = cams[:, 8:10]
    assert torch.equal(r.render(q, return_codes=True)['logits'], ref.render(q, return_codes=True)['logits'])
    parity_report(test='fork_renderer', arm=arm, equal=True)


# ---------------------------------------------------------------------------------------------- 9
def test_gradients_the_fp8_arm_wrong_shapes_and_foreign_models_are_refused(dev):
    from viewformer_amd import _lib
    from viewformer_amd.migt import MIGT
    from viewformer_amd.weights import make_migt_weights
    s = _model(dev, 'f32')
    m, codes, poses = s['m'], s['codes'], s['poses']
    parent = _parent(s)
    child = parent.fork(S_, room=1)
    qpos, photos = _per_child(poses, 4, 8), _per_child(codes, 4, 8)
    for refused in (m.score_grad_from_context, m.refine_from_context):
        with pytest.raises(ValueError, match=r'materialize\(\)'):
            refused(child, qpos, photos)
    with pytest.raises(ValueError, match=r'materialize\(\)'):
        child.fork(2)
    with pytest.raises(ValueError, match=r'materialize\(\)'):
        m.rollout_from_context(child, qpos, n_samples=2, fork=True)
    for S, room in ((0, 1), (1.5, 1), (True, 1), (2, -1), (2, 1.5)):
        with pytest.raises(ValueError):
            parent.fork(S, room)
    for bad in (poses[:, 4:6], qpos[:, :, :6]):                                   # the fork has B S scenes
        with pytest.raises(ValueError):
            m.generate_from_context(child, bad)
    with pytest.raises(ValueError):
        m.append_to_context(child, codes[:, 2:3], poses[:, 2:3])
    cfg2 = _cfg(n_layer=2)
    other = MIGT(cfg2).load_state_dict(make_migt_weights(cfg2, seed=0)).to(dev)
    with pytest.raises(ValueError):                                               # a fork used with another model
        other.generate_from_context(child, qpos)
    with pytest.raises(ValueError):
        other.adopt_from_fork(parent, child, [0, 0])
    fp8 = MIGT(cfg2, precision='bf16', attention='fp8').load_state_dict(make_migt_weights(cfg2, seed=0)).to(dev)
    with pytest.raises(_lib.VfError):                                             # the fp8 attention arm has no cached contexts, forked or not
        fp8.rollout_from_context(parent, poses[:, 4:6], n_samples=2, fork=True)
    with pytest.raises(_lib.VfError):
        fp8.score_from_context(child, qpos, photos)
    assert child.filled().tolist() == [C0] * 4 and parent.C == C0                # nothing was launched, nothing grew
