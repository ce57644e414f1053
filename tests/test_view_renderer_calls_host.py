"""CPU: everything ``ViewRenderer`` hands across its boundary, scenario by scenario.  The renderer runs over the
stand-ins of tests/render_fakes.py — a transformer and a codebook that record their arguments and answer with exact functions of them,
CPU stand-ins for ``ops.postprocess_u8`` / ``argmax_rows`` / ``logits_score`` / ``resize_u8``, and a real ``ContextCache`` on small CPU
tensors — and every call that reaches them is written down: the function's name and each argument, a tensor or array as
'dtype[shape]/[strides]:the first 16 hex digits of the SHA-256 of its bytes', a scalar as it is, a cache as '#its number among the
caches seen=filled()'.  Per scenario the ordered calls, the result key by key in order and the renderer's state afterwards must equal
``tests/golden/view_renderer_calls.json``, recorded before the renderer's front matter had one definition per rule: a call whose slice,
order, dtype, contiguity or keyword set moved would change what the device computes.  The fixture keeps every call as 'name:digest' (the
first 12 hex digits of the SHA-256 of the call's arguments as JSON) and results and states in full; a call that differs is reported with
its live arguments.  Every float that crosses the boundary is exact (dyadic positions, quaternions on the signed unit axes), so the
digests do not depend on the CPU; the premise is asserted below.  The second half holds the renderer's refusals: each one raises before
any boundary call.  No device is touched.

``python tests/test_view_renderer_calls_host.py`` prints the fixture of the code as it stands, ``... --full`` every call with its
arguments, one per line, for a diff between two checkouts."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [p for p in (HERE, os.path.dirname(HERE)) if p not in sys.path]      # (for the run as a script)
import render_fakes as F  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'view_renderer_calls.json')
B, C, N, T_IMG, SIZE, NE, P = 2, 3, 5, 8, 32, 64, 4
MODES = ('relative', 'absolute')


def sha(raw):
    return hashlib.sha256(raw).hexdigest()[:16]


class Recorder:
    def __init__(self):
        self.calls, self.caches, self.keep = [], {}, []

    def reset(self):
        self.calls, self.caches = [], {}

    def arg(self, x):
        from viewformer_amd.context_cache import ContextCache
        if isinstance(x, torch.Tensor):
            return '%s%s/%s:%s' % (str(x.dtype)[6:], list(x.shape), list(x.stride()), sha(x.contiguous().numpy().tobytes()))
        if isinstance(x, np.ndarray):
            return 'np.%s%s/%s:%s' % (x.dtype, list(x.shape), [s // x.itemsize for s in x.strides], sha(np.ascontiguousarray(x).tobytes()))
        if isinstance(x, ContextCache):
            self.keep.append(x)                                                # alive: a freed cache's id would come back as another's
            return '#%d=%s' % (self.caches.setdefault(id(x), len(self.caches)), x.filled().tolist())
        if isinstance(x, (tuple, list)):
            return [self.arg(y) for y in x]
        if isinstance(x, (np.integer, np.floating)):
            return x.item()
        assert x is None or isinstance(x, (bool, int, float, str)), type(x)
        return x

    def log(self, name, *a, **k):
        self.calls.append([name] + [self.arg(x) for x in a] + [{n: self.arg(k[n]) for n in sorted(k)}] * bool(k))

    def value(self, x):
        """a result: a dict key by key in order, a renderer by name"""
        from viewformer_amd.render import ViewRenderer
        if isinstance(x, dict):
            return [[k, self.arg(v)] for k, v in x.items()]
        return 'ViewRenderer' if isinstance(x, ViewRenderer) else self.arg(x)

    def state(self, r):
        none = lambda x: None if x is None else self.arg(x)
        c = r.cache
        return dict(context_codes=none(r.context_codes), transform=none(r.transform), n_context=None if r.n_context is None else r.n_context.tolist(),
                    cache=type(c).__name__, C=c.C, filled=c.filled().tolist(), capacity=c.capacity)


# ------------------------------------------------------------------ exact inputs
def cameras(n, seed, scenes=B):
    """[scenes,n,7]: positions in quarters, quaternions on the signed unit axes — every frame change is exact"""
    out = torch.zeros(scenes, n, 7)
    for b in range(scenes):
        for i in range(n):
            out[b, i, :3] = torch.tensor([((7 * b + 3 * i + 5 * k + 11 * seed) % 17 - 8) / 4 for k in range(3)])
            out[b, i, 3 + (b + 2 * i + seed) % 4] = 1.0 if (b + i + seed) % 3 else -1.0
    return out


def codes(n, seed, scenes=B, dtype=torch.int64):
    b, i = torch.arange(scenes).view(-1, 1, 1, 1), torch.arange(n).view(1, -1, 1, 1)
    y, x = torch.arange(T_IMG).view(1, 1, -1, 1), torch.arange(T_IMG).view(1, 1, 1, -1)
    return ((13 * b + 7 * i + 3 * y + x + seed) % NE).to(dtype)


def images(n, seed, scenes=B, size=SIZE):
    b, i = torch.arange(scenes).view(-1, 1, 1, 1, 1), torch.arange(n).view(1, -1, 1, 1, 1)
    y, x, c = torch.arange(size).view(1, 1, -1, 1, 1), torch.arange(size).view(1, 1, 1, -1, 1), torch.arange(3).view(1, 1, 1, 1, -1)
    return ((5 * b + 11 * i + 3 * y + x + c + seed) % NE).to(torch.uint8)


def test_every_pose_that_crosses_the_boundary_is_exact():
    """the premise of the digests: ``context_poses`` / ``query_poses`` / ``from_relative_cameras`` of these inputs make no rounding —
    float32 equals a float64 evaluation cast to float32, exactly"""
    from viewformer_amd import geometry
    from viewformer_amd.render import context_poses, query_poses
    for seed in range(8):
        ctx, q = cameras(C, seed), cameras(N, seed + 1)
        for mode in MODES:
            p32, t32 = context_poses(ctx, mode)
            p64, t64 = context_poses(ctx.double(), mode)
            assert torch.equal(p32, p64.float())
            assert torch.equal(query_poses(q, t32), query_poses(q.double(), t64).float())
            if t32 is not None:
                assert torch.equal(geometry.from_relative_cameras(q, t32), geometry.from_relative_cameras(q.double(), t64).float())


# ------------------------------------------------------------------ the scenarios
def record(monkeypatch, mode):
    from viewformer_amd import ops, render
    rec = Recorder()
    cfg = F.Cfg(n_embeddings=NE, augment_poses=mode)
    host = F.host_model()
    for name, fn in F.fake_ops(rec.log).items():
        monkeypatch.setattr(ops, name, fn)
    monkeypatch.setattr(ops, 'kv_append', lambda *a, **k: None)                # a real cache that reallocates on the CPU: nothing to copy
    out = {}

    def parts():
        return F.FakeModel(cfg, host, rec.log), F.FakeCodebook(cfg, rec.log)

    def ctx(**kw):
        return render.ViewRenderer(*parts()).set_context(codes=codes(C, 1), cameras=cameras(C, 1), **kw)

    def seq(name, fn, r=None):
        rec.reset()
        res = fn()
        r = res if r is None and isinstance(res, render.ViewRenderer) else r
        out[name] = dict(calls=rec.calls, result=rec.value(res))
        if r is not None:
            out[name]['state'] = rec.state(r)
        return res

    def on(name, r, fn):
        return seq(name, lambda: fn(r), r)

    q, q0 = cameras(N, 2), cameras(0, 2)
    per_view = (np.arange(B * N, dtype=np.int64).reshape(B, N) % (C + 1)).astype(np.int32)
    ragged = dict(n_context=[2, 3])

    # set_context
    seq('set_context_images', lambda: render.ViewRenderer(*parts()).set_context(images=images(C, 3), cameras=cameras(C, 1)))
    seq('set_context_images_resized', lambda: render.ViewRenderer(*parts()).set_context(images=images(C, 3, size=64), cameras=cameras(C, 1)))
    seq('set_context_codes', ctx)
    seq('set_context_codes_int32', lambda: render.ViewRenderer(*parts()).set_context(codes=codes(C, 1, dtype=torch.int32), cameras=cameras(C, 1).numpy()))
    seq('set_context_ragged', lambda: ctx(**ragged))
    seq('set_context_n_context_int', lambda: ctx(n_context=2))
    seq('set_context_capacity', lambda: ctx(capacity=5))
    seq('set_context_pack_kv', lambda: ctx(pack='kv'))
    seq('set_context_pack_kv_capacity', lambda: ctx(pack='kv', capacity=5, **ragged))

    # render
    for rc in (False, True):
        for cf in (False, True):
            for cap in (None, 2):
                on(f'render_codes{int(rc)}_conf{int(cf)}_cap{cap}', ctx(), lambda r: r.render(q, max_views_per_call=cap, return_codes=rc, return_confidence=cf))
            on(f'render_codes{int(rc)}_conf{int(cf)}_empty', ctx(), lambda r: r.render(q0, return_codes=rc, return_confidence=cf))
    on('render_scene_default', ctx(**ragged), lambda r: r.render(q, max_views_per_call=2))
    on('render_scene_default_empty', ctx(**ragged), lambda r: r.render(q0))
    on('render_per_view', ctx(), lambda r: r.render(q, max_views_per_call=2, n_context=per_view, return_codes=True, return_confidence=True))
    on('render_per_scene', ctx(**ragged), lambda r: r.render(q, n_context=[1, 2]))
    on('render_int', ctx(), lambda r: r.render(q, max_views_per_call=3, n_context=1, return_confidence=True))

    # sample
    skw = dict(n_samples=3, temperature=0.5, top_k=5, top_p=0.75, seed=3)
    on('sample', ctx(), lambda r: r.sample(q, **skw))
    on('sample_chunked_codes', ctx(), lambda r: r.sample(q, max_views_per_call=2, return_codes=True, **skw))
    on('sample_defaults', ctx(), lambda r: r.sample(q))
    on('sample_lengths', ctx(**ragged), lambda r: r.sample(q, max_views_per_call=2, n_samples=2))
    on('sample_per_view', ctx(), lambda r: r.sample(q, max_views_per_call=2, n_samples=2, n_context=per_view, return_codes=True))
    on('sample_empty', ctx(), lambda r: r.sample(q0, n_samples=3, return_codes=True))
    on('sample_empty_lengths', ctx(**ragged), lambda r: r.sample(q0, n_samples=3))

    # score and score_gradient
    for name in ('score', 'score_gradient'):
        call = lambda r, *a, **k: getattr(r, name)(*a, **k)
        on(f'{name}_codes', ctx(), lambda r: call(r, q, codes=codes(N, 4)))
        on(f'{name}_codes_int32_chunked', ctx(), lambda r: call(r, q, codes=codes(N, 4, dtype=torch.int32), max_views_per_call=2))
        on(f'{name}_one_photo', ctx(), lambda r: call(r, q, codes=codes(1, 4)))
        on(f'{name}_one_photo_chunked', ctx(), lambda r: call(r, q, codes=codes(1, 4), max_views_per_call=2))
        on(f'{name}_one_photo_one_camera', ctx(), lambda r: call(r, q[:, :1], codes=codes(1, 4)))
        on(f'{name}_images_chunked', ctx(), lambda r: call(r, q, images=images(N, 5), max_views_per_call=2))
        on(f'{name}_one_image', ctx(), lambda r: call(r, q, images=images(1, 5, size=64)))
        on(f'{name}_lengths', ctx(**ragged), lambda r: call(r, q, codes=codes(N, 4), max_views_per_call=2))
        on(f'{name}_per_view', ctx(), lambda r: call(r, q, codes=codes(N, 4), max_views_per_call=2, n_context=per_view))
        on(f'{name}_empty', ctx(), lambda r: call(r, q0, codes=codes(0, 4)))
        on(f'{name}_empty_images_lengths', ctx(**ragged), lambda r: call(r, q0, images=images(0, 5)))
    for fused in (False, True):
        r = ctx()
        r.fused_score = fused
        on(f'score_fused_{fused}', r, lambda r: r.score(q, codes=codes(N, 4), max_views_per_call=2))
        on(f'score_fused_{fused}_empty', r, lambda r: r.score(q0, codes=codes(0, 4)))

    # match
    for scenes in (B, 1):
        on(f'match_scenes{scenes}', ctx(), lambda r: r.match(q, codes=codes(P, 6, scenes)))
        on(f'match_scenes{scenes}_chunked', ctx(), lambda r: r.match(q, codes=codes(P, 6, scenes, torch.int32), max_views_per_call=2))
        on(f'match_scenes{scenes}_images', ctx(), lambda r: r.match(q, images=images(P, 6, scenes), max_views_per_call=2))
        on(f'match_scenes{scenes}_no_camera', ctx(), lambda r: r.match(q0, codes=codes(P, 6, scenes)))
        on(f'match_scenes{scenes}_no_photo', ctx(), lambda r: r.match(q, codes=codes(0, 6, scenes), max_views_per_call=2))
        on(f'match_scenes{scenes}_no_photo_images', ctx(), lambda r: r.match(q, images=images(0, 6, scenes)))
    on('match_lengths', ctx(**ragged), lambda r: r.match(q, codes=codes(P, 6), max_views_per_call=2))
    on('match_per_view', ctx(), lambda r: r.match(q, codes=codes(P, 6), max_views_per_call=2, n_context=per_view))

    # refine
    rkw = dict(steps=3, step_xyz=0.25, step_rot=0.125)
    on('refine', ctx(), lambda r: r.refine(q, codes=codes(N, 7), **rkw))
    on('refine_defaults', ctx(), lambda r: r.refine(q, codes=codes(N, 7)))
    on('refine_chunked_trace', ctx(), lambda r: r.refine(q, codes=codes(N, 7), max_views_per_call=2, return_trace=True, **rkw))
    on('refine_one_photo', ctx(), lambda r: r.refine(q, images=images(1, 7), max_views_per_call=2, **rkw))
    on('refine_from_localize', ctx(), lambda r: r.refine(None, codes=codes(N, 7), **rkw))
    on('refine_from_localize_chunked', ctx(**ragged), lambda r: r.refine(None, images=images(N, 7), max_views_per_call=2, return_trace=True, **rkw))
    on('refine_per_view', ctx(), lambda r: r.refine(None, codes=codes(N, 7), max_views_per_call=2, n_context=per_view, **rkw))
    on('refine_empty', ctx(), lambda r: r.refine(q0, codes=codes(0, 7), return_trace=True, **rkw))
    on('refine_from_localize_empty', ctx(), lambda r: r.refine(None, codes=codes(0, 7), **rkw))

    # localize
    for tokens in (False, True):
        on(f'localize_codes_tokens{int(tokens)}', ctx(), lambda r: r.localize(codes=codes(N, 8), return_tokens=tokens))
        on(f'localize_images_chunked_tokens{int(tokens)}', ctx(), lambda r: r.localize(images=images(N, 8), max_views_per_call=2, return_tokens=tokens))
        on(f'localize_empty_tokens{int(tokens)}', ctx(), lambda r: r.localize(codes=codes(0, 8), return_tokens=tokens))
    on('localize_codes_int32_chunked', ctx(), lambda r: r.localize(codes=codes(N, 8, dtype=torch.int32), max_views_per_call=2))
    on('localize_images_resized', ctx(), lambda r: r.localize(images=images(N, 8, size=64)))
    on('localize_empty_images', ctx(**ragged), lambda r: r.localize(images=images(0, 8)))
    on('localize_lengths', ctx(**ragged), lambda r: r.localize(codes=codes(N, 8), max_views_per_call=2))
    on('localize_per_view', ctx(), lambda r: r.localize(codes=codes(N, 8), max_views_per_call=2, n_context=per_view, return_tokens=True))
    for tail in (False, True):
        r = ctx()
        r.fused_tail = tail
        on(f'localize_fused_tail_{tail}', r, lambda r: r.localize(codes=codes(N, 8), max_views_per_call=2))
        on(f'localize_fused_tail_{tail}_empty', r, lambda r: r.localize(codes=codes(0, 8), return_tokens=True))

    # sweep
    on('sweep', ctx(), lambda r: r.sweep(q))
    on('sweep_sizes', ctx(), lambda r: r.sweep(q, sizes=[0, 2], max_views_per_call=3))
    on('sweep_sizes_tensor_codes', ctx(), lambda r: r.sweep(q, sizes=torch.tensor([3, 1]), return_codes=True))
    on('sweep_ragged', ctx(**ragged), lambda r: r.sweep(q, max_views_per_call=4))
    on('sweep_ragged_sizes_codes', ctx(**ragged), lambda r: r.sweep(q, sizes=np.array([0, 2, 3]), return_codes=True))
    on('sweep_empty', ctx(), lambda r: r.sweep(q0, sizes=[1]))
    on('sweep_no_sizes', ctx(), lambda r: r.sweep(q, sizes=np.zeros(0, dtype=np.int64)))

    # append
    add = cameras(2, 9)
    on('append_codes', ctx(), lambda r: r.append(codes=codes(2, 9), cameras=add))
    on('append_images', ctx(), lambda r: r.append(images=images(2, 9), cameras=add))
    on('append_ragged_capacity', ctx(capacity=5, **ragged), lambda r: r.append(codes=codes(2, 9, dtype=torch.int32), cameras=add))
    on('append_ragged_images_grows', ctx(**ragged), lambda r: r.append(images=images(2, 9, size=64), cameras=add.numpy()))
    on('append_nothing_codes', ctx(**ragged), lambda r: r.append(codes=codes(0, 9), cameras=add[:, :0]))
    on('append_nothing_images', ctx(), lambda r: r.append(images=images(0, 9), cameras=add[:, :0]))
    r = ctx(capacity=5, **ragged)
    r.append(codes=codes(2, 9), cameras=add)
    on('render_after_append', r, lambda r: r.render(q, max_views_per_call=2))
    on('score_after_append', r, lambda r: r.score(q, codes=codes(1, 4), max_views_per_call=2))

    # rollout
    path, okw = cameras(2, 10), dict(temperature=0.5, top_k=4, top_p=0.75, seed=2)
    for keep in (True, False):
        on(f'rollout_keep{int(keep)}', ctx(), lambda r: r.rollout(path, keep=keep))
        on(f'rollout_ragged_keep{int(keep)}', ctx(capacity=6, **ragged), lambda r: r.rollout(path, keep=keep, return_codes=True, **okw))
    on('rollout_samples', ctx(), lambda r: r.rollout(path, n_samples=2, **okw))
    on('rollout_samples_codes', ctx(**ragged), lambda r: r.rollout(path, n_samples=2, return_codes=True))
    on('rollout_fork', ctx(), lambda r: r.rollout(path, n_samples=2, fork=True, **okw))
    on('rollout_fork_adopt_best', ctx(), lambda r: r.rollout(path, n_samples=2, fork=True, adopt='best', **okw))
    on('rollout_fork_adopt_list', ctx(**ragged), lambda r: r.rollout(path, n_samples=2, fork=True, adopt=[1, 0], return_codes=True))
    on('rollout_fork_adopt_empty_path', ctx(), lambda r: r.rollout(path[:, :0], n_samples=2, fork=True, adopt='best'))
    on('rollout_unfused_step', ctx(), lambda r: r.rollout(path, fused_step=False))
    on('rollout_fused_step', ctx(), lambda r: r.rollout(path, fused_step=True, return_codes=True))
    on('rollout_empty_path', ctx(**ragged), lambda r: r.rollout(path[:, :0]))
    on('rollout_packed', ctx(pack='kv', capacity=5), lambda r: r.rollout(path, n_samples=2))
    r = ctx(**ragged)
    r.rollout(path)
    on('render_after_rollout', r, lambda r: r.render(q, max_views_per_call=2))

    # fork
    for name, parent in (('fork', ctx()), ('fork_ragged', ctx(**ragged))):
        parent.fused_score, parent.fused_tail = False, True
        child = on(name, parent, lambda r: r.fork(2))
        out[name]['child'] = dict(rec.state(child), fused_score=child.fused_score, fused_tail=child.fused_tail)
        on(name + '_child_render', child, lambda r: r.render(cameras(N, 2, 2 * B), max_views_per_call=2))
        on(name + '_child_append', child, lambda r: r.append(codes=codes(2, 9, 2 * B), cameras=cameras(2, 9, 2 * B)))
        on(name + '_child_score', child, lambda r: r.score(cameras(N, 2, 2 * B), codes=codes(1, 4, 2 * B)))
        on(name + '_child_localize', child, lambda r: r.localize(codes=codes(N, 8, 2 * B), max_views_per_call=2))
        on(name + '_parent_after', parent, lambda r: r.render(q))
    on('fork_room', ctx(), lambda r: r.fork(3, room=2))

    # pack
    r = ctx(**ragged)
    on('pack', r, lambda r: r.pack())
    on('pack_context_bytes', r, lambda r: r.context_bytes())
    on('pack_render', r, lambda r: r.render(q, max_views_per_call=2))
    on('pack_localize', r, lambda r: r.localize(codes=codes(N, 8)))
    on('unpack', r, lambda r: r.unpack())
    on('unpack_context_bytes', r, lambda r: r.context_bytes())
    r = ctx()
    on('pack_room', r, lambda r: r.pack(room=1))
    on('pack_room_append', r, lambda r: r.append(codes=codes(1, 9), cameras=add[:, :1]))
    on('pack_room_append_grows', r, lambda r: r.append(codes=codes(2, 9), cameras=add))
    on('pack_room_rollout', r, lambda r: r.rollout(path))
    on('pack_room_context_bytes', r, lambda r: r.context_bytes())
    on('pack_room_unpack', r, lambda r: r.unpack())

    # the one-call functions
    fm, cb = parts()
    im, cm = images(C, 3), cameras(C, 1)
    seq('render_views', lambda: render.render_views(fm, cb, im, cm, q, max_views_per_call=2, return_codes=True))
    seq('render_views_codes', lambda: render.render_views(fm, cb, None, cm, q, codes=codes(C, 1)))
    seq('sweep_views', lambda: render.sweep_views(fm, cb, im, cm, q, n_context=[2, 3], sizes=[1, 3]))
    seq('sweep_views_codes', lambda: render.sweep_views(fm, cb, None, cm, q, codes=codes(C, 1), return_codes=True))
    seq('sample_views', lambda: render.sample_views(fm, cb, im, cm, q, n_samples=2, seed=5, max_views_per_call=2))
    seq('rollout_views', lambda: render.rollout_views(fm, cb, im, cm, path, n_context=[2, 3], n_samples=2, top_k=3))
    seq('rollout_views_pack', lambda: render.rollout_views(fm, cb, None, cm.numpy(), path.numpy(), codes=codes(C, 1), pack='kv', return_codes=True))
    seq('score_views', lambda: render.score_views(fm, cb, im, cm, q, images(1, 5), max_views_per_call=2))
    seq('score_views_codes', lambda: render.score_views(fm, cb, None, cm, q, codes=codes(C, 1), photo_codes=codes(N, 4)))
    seq('match_views', lambda: render.match_views(fm, cb, im, cm, q, images(P, 6, 1), max_views_per_call=2, n_context=[2, 3]))
    seq('match_views_codes', lambda: render.match_views(fm, cb, None, cm, q, codes=codes(C, 1), photo_codes=codes(P, 6)))
    seq('refine_views', lambda: render.refine_views(fm, cb, im, cm, images(N, 7), q, steps=2, return_trace=True))
    seq('refine_views_codes', lambda: render.refine_views(fm, cb, None, cm, codes=codes(C, 1), photo_codes=codes(N, 7), steps=2, max_views_per_call=2))
    seq('localize_views', lambda: render.localize_views(fm, cb, im, cm, images(N, 8), max_views_per_call=2, return_tokens=True))
    seq('localize_views_codes', lambda: render.localize_views(fm, cb, None, cm, codes=codes(C, 1), photo_codes=codes(N, 8)))
    seq('evaluate_context_sizes', lambda: render.evaluate_context_sizes(fm, cb, images(C + 1, 3), cameras(C + 1, 1)))
    return out


def digest(call):
    return call[0] + ':' + hashlib.sha256(json.dumps(call[1:], separators=(',', ':'), sort_keys=True).encode()).hexdigest()[:12]


@pytest.mark.parametrize('mode', MODES)
def test_every_scenario_crosses_the_boundary_as_recorded(monkeypatch, mode):
    got = json.loads(json.dumps(record(monkeypatch, mode)))
    with open(GOLDEN) as fh:
        want = json.load(fh)[mode]
    assert sorted(got) == sorted(want)
    for name in want:
        assert len(got[name]['calls']) == len(want[name]['calls']), (name, [c[0] for c in got[name]['calls']])
        for i, (g, w) in enumerate(zip(got[name]['calls'], want[name]['calls'])):
            assert digest(g) == w, (name, i, g)
        for k in ('result', 'state', 'child'):
            assert got[name].get(k) == want[name].get(k), (name, k)


# ------------------------------------------------------------------ the refusals: each before any boundary call
@pytest.fixture
def renderer(monkeypatch):
    """a renderer with a context of B scenes x C views over recording stand-ins, and its recorder, emptied"""
    from viewformer_amd import ops, render
    rec = Recorder()
    cfg = F.Cfg(n_embeddings=NE)
    for name, fn in F.fake_ops(rec.log).items():
        monkeypatch.setattr(ops, name, fn)
    monkeypatch.setattr(ops, 'kv_append', lambda *a, **k: None)
    r = render.ViewRenderer(F.FakeModel(cfg, F.host_model(), rec.log), F.FakeCodebook(cfg, rec.log))
    r.set_context(codes=codes(C, 1), cameras=cameras(C, 1))
    rec.reset()
    return r, rec


def refused(rec, fn, error=ValueError, match=None):
    with pytest.raises(error, match=match):
        fn()
    assert rec.calls == []


def test_codes_follow_one_rule_in_every_method(renderer):
    """integers, not bool, not floating point, exactly [scenes, views, t, t] with the caller's scene and view axes"""
    from viewformer_amd.render import ViewRenderer
    r, rec = renderer
    fresh = lambda: ViewRenderer(r.transformer, r.codebook)
    cm, good, add = cameras(C, 1), codes(C, 1), cameras(2, 9)
    # set_context: anything but [B,C,t,t] integers
    for bad in (good.transpose(0, 1).contiguous(), good.reshape(B, C, T_IMG * T_IMG), good.reshape(B * C, T_IMG, T_IMG), good.float(),
                good.bool(), good[:, :2], good[..., :4]):
        refused(rec, lambda: fresh().set_context(codes=bad, cameras=cm))
    # append: anything but [B,K,t,t] integers
    k = codes(2, 9)
    for bad in (k.reshape(B, 2, T_IMG * T_IMG), k.reshape(B * 2, T_IMG, T_IMG), k.reshape(B, 1, 2 * T_IMG, T_IMG), k.float(), k.bool(), k[:, :1]):
        refused(rec, lambda: r.append(codes=bad, cameras=add))
    # localize: anything but [B,N,t,t] integers
    n = codes(N, 8)
    for bad in (n.reshape(B, N * T_IMG, T_IMG), n.reshape(B, N, T_IMG * T_IMG), n.reshape(B, N * T_IMG * T_IMG), n.float(), n.bool(),
                n[:1], n[..., :4]):
        refused(rec, lambda: r.localize(codes=bad))
    # score: bool codes at the renderer
    refused(rec, lambda: r.score(cameras(N, 2), codes=codes(N, 4).bool()))
    assert r.cache.C == C and tuple(r.context_codes.shape) == (B, C, T_IMG, T_IMG)


def test_refusals_come_in_order_and_before_any_call(renderer):
    """no context first, then the cache's own refusals and rollout's adopt / fork check, and only then the codebook — the refusals the
    per-feature host tests assert, on one renderer"""
    from viewformer_amd.render import ViewRenderer
    r, rec = renderer
    q, cd, im = cameras(N, 2), codes(N, 4), images(N, 5)
    # no context: before anything touches the model objects
    bare = ViewRenderer(None, None)
    for fn in (lambda: bare.render(q), lambda: bare.sample(q), lambda: bare.score(q, codes=cd), lambda: bare.match(q, codes=cd),
               lambda: bare.score_gradient(q, codes=cd), lambda: bare.refine(q, codes=cd), lambda: bare.refine(None, codes=cd),
               lambda: bare.localize(codes=cd), lambda: bare.localize(images=im), lambda: bare.sweep(q),
               lambda: bare.append(codes=cd, cameras=q), lambda: bare.rollout(q), lambda: bare.fork(2), lambda: bare.pack(),
               lambda: bare.pack(room=1), lambda: bare.unpack(), lambda: bare.context_bytes()):
        with pytest.raises(RuntimeError, match='set_context'):
            fn()
    # the cache's refusals and rollout's argument check: on a renderer without a codebook
    cache = r.transformer.prefill_context(codes(C, 1), cameras(C, 1))
    rec.reset()
    nocb = ViewRenderer(r.transformer.host, None)
    nocb.cache = cache
    path = cameras(1, 10)
    for kw in (dict(adopt='best'), dict(adopt='best', n_samples=2), dict(adopt=[0, 0], n_samples=2), dict(adopt='best', fork=True),
               dict(adopt='worst', fork=True, n_samples=2)):
        with pytest.raises(ValueError):
            nocb.rollout(path, **kw)
    with pytest.raises(ValueError, match='room'):
        nocb.pack(room=-1)
    nocb.cache = cache.fork(2)
    for fn in (lambda: nocb.score_gradient(cameras(N, 2, 2 * B), codes=codes(N, 4, 2 * B)), lambda: nocb.refine(cameras(N, 2, 2 * B), codes=codes(N, 4, 2 * B))):
        with pytest.raises(ValueError, match=r'materialize\(\)'):
            fn()
    nocb.cache = cache.pack()
    for fn in (lambda: nocb.append(codes=codes(1, 9), cameras=path), lambda: nocb.rollout(path), lambda: nocb.fork(2),
               lambda: nocb.score_gradient(q, codes=cd), lambda: nocb.refine(q, codes=cd), lambda: nocb.pack()):
        with pytest.raises(ValueError, match=r'unpack\(\)'):
            fn()
    nocb.cache = cache.pack(room=2)
    for fn in (lambda: nocb.fork(2), lambda: nocb.score_gradient(q, codes=cd), lambda: nocb.refine(q, codes=cd), lambda: nocb.rollout(path, fork=True),
               lambda: nocb.rollout(path, n_samples=2, fork=True), lambda: nocb.pack(), lambda: nocb.pack(room=1)):
        with pytest.raises(ValueError, match=r'unpack\(\)'):
            fn()
    assert rec.calls == []
    # the arguments: every refusal before the model, the codebook or ops are asked
    bad_cameras = (q[:1], q[..., :6], q[0], torch.zeros(B, 7))
    for qq in bad_cameras:
        for fn in (lambda: r.render(qq), lambda: r.sample(qq), lambda: r.score(qq, codes=cd), lambda: r.match(qq, codes=cd),
                   lambda: r.score_gradient(qq, codes=cd), lambda: r.refine(qq, codes=cd), lambda: r.sweep(qq), lambda: r.rollout(qq),
                   lambda: r.append(codes=cd, cameras=qq)):
            refused(rec, fn)
    for name in ('score', 'score_gradient', 'refine', 'match'):
        f = getattr(r, name)
        refused(rec, lambda: f(q))                                                     # neither photos nor codes
        refused(rec, lambda: f(q, images=im, codes=cd))
        refused(rec, lambda: f(q, codes=cd.float()))
        refused(rec, lambda: f(q, codes=cd.bool()))
        refused(rec, lambda: f(q, codes=cd.view(B, N, T_IMG * T_IMG)))                 # token maps are [t, t], as the model requires
        refused(rec, lambda: f(q, codes=cd[:, :, :4]))
        refused(rec, lambda: f(q, codes=codes(N, 4, 3)))                               # another batch size
        refused(rec, lambda: f(q, images=im[0]))
        refused(rec, lambda: f(q, images=images(N, 5, 3)))
        if name != 'match':
            refused(rec, lambda: f(q, codes=cd[:, :3]))                                # 3 photos for 5 cameras
            refused(rec, lambda: f(q, images=im[:, :3]))
            refused(rec, lambda: f(q, codes=codes(N, 4, 1)))                           # a shared photo set is match's alone
    refused(rec, lambda: r.localize())
    refused(rec, lambda: r.localize(images=im, codes=cd))
    refused(rec, lambda: r.localize(images=im[0]))
    refused(rec, lambda: r.localize(images=im[:1]))
    refused(rec, lambda: r.append(codes=cd, cameras=None))
    refused(rec, lambda: r.append(cameras=q))
    refused(rec, lambda: r.append(images=im, codes=cd, cameras=q))
    refused(rec, lambda: r.append(images=im[:, :3], cameras=q))
    refused(rec, lambda: r.sample(q, max_views_per_call=0))
    refused(rec, lambda: r.render(q, max_views_per_call=0))
    refused(rec, lambda: r.rollout(q, n_samples=0))
    refused(rec, lambda: r.rollout(q, n_samples=1.5))
    refused(rec, lambda: r.fork(0))
    refused(rec, lambda: r.fork(True))
    for sizes in ([C + 1], [-1], [0.5], [True], [[0, 1]], []):             # (an empty list is an array of floats)
        refused(rec, lambda: r.sweep(q, sizes=sizes))
    for n in (-1, C + 1, [1], [1, 2, 3], [[1, 2]], 1.0, True):
        refused(rec, lambda: r.render(q, n_context=n))
        refused(rec, lambda: r.score(q, codes=cd, n_context=n))
    fresh = lambda: ViewRenderer(r.transformer, r.codebook)
    cm = cameras(C, 1)
    for kw in (dict(codes=codes(C, 1)), dict(cameras=cm), dict(images=images(C, 3), codes=codes(C, 1), cameras=cm), dict(codes=codes(C, 1), cameras=cm[0]),
               dict(codes=codes(C, 1), cameras=cm[..., :6]), dict(codes=codes(0, 1), cameras=cm[:, :0]), dict(images=images(C, 3)[0], cameras=cm),
               dict(images=images(2, 3), cameras=cm), dict(codes=codes(C, 1), cameras=cm, n_context=[1, 2, 3]), dict(codes=codes(C, 1), cameras=cm, n_context=0),
               dict(codes=codes(C, 1), cameras=cm, n_context=[1, C + 1]), dict(codes=codes(C, 1), cameras=cm, n_context=[[1, 2]]),
               dict(codes=codes(C, 1), cameras=cm, n_context=[1.0, 2.0])):
        refused(rec, lambda: fresh().set_context(**kw))


if __name__ == '__main__':
    mp = pytest.MonkeyPatch()
    rec = json.loads(json.dumps({mode: record(mp, mode) for mode in MODES}))
    mp.undo()
    if '--full' in sys.argv:
        for mode in rec:
            for name, v in rec[mode].items():
                for i, c in enumerate(v['calls']):
                    print(mode, name, i, json.dumps(c, separators=(',', ':')))
                print(mode, name, 'result', json.dumps({k: v[k] for k in v if k != 'calls'}, separators=(',', ':')))
    else:                                                                      # one scenario per line
        one = lambda v: json.dumps(dict(v, calls=[digest(c) for c in v['calls']]), separators=(',', ':'))
        print('{' + ',\n'.join('"%s":{\n%s}' % (mode, ',\n'.join('"%s":%s' % (n, one(v)) for n, v in rec[mode].items())) for mode in rec) + '}')
