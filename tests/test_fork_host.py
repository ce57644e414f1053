"""CPU: the host side of a forked context cache (``vf_attn_prefix_fork_*``, ``ContextCache.fork`` / ``materialize``,
``MIGT.adopt_from_fork``, ``ViewRenderer.fork`` / ``rollout(fork=, adopt=)``) — the pure planners equal brute force, both new entries
validate their arguments before any launch, and the refusals that need no device refuse.  No device is touched."""
import ctypes

import numpy as np
import pytest
import torch


@pytest.fixture(scope='module')
def lib():
    from viewformer_amd import build, _lib
    build.build()                      # hipcc cross-compiles gfx950 without a GPU
    return _lib.load()


# ---------------------------------------------------------------------------------------------- the planners against brute force
SPLITS = [[0], [3], [0, 2, 5], [4, 4, 0, 1], []]


@pytest.mark.parametrize('split', SPLITS)
@pytest.mark.parametrize('n_views', [0, 1, 7])
def test_the_logical_view_mapping_against_brute_force(split, n_views):
    from viewformer_amd.render import map_fork_views
    seg, view = map_fork_views(np.array(split, dtype=np.int32), n_views)
    assert seg.shape == view.shape == (len(split), n_views) and seg.dtype == np.int8 and view.dtype == np.int32
    for b, sp in enumerate(split):
        own_seen = 0
        for s in range(n_views):
            if s < sp:
                assert (seg[b, s], view[b, s]) == (0, s)
            else:
                assert (seg[b, s], view[b, s]) == (1, own_seen)              # own views count from 0, in order, behind the parent's
                own_seen += 1
    for bad in ([-1], [[1]], [True], [1.0]):
        with pytest.raises(ValueError):
            map_fork_views(np.array(bad), 2)
    with pytest.raises(ValueError):
        map_fork_views(np.array([1]), -1)


@pytest.mark.parametrize('lengths', [[2], [1, 2], [0, 3, 1], []])
@pytest.mark.parametrize('S', [1, 2, 5])
def test_the_fork_plan_against_brute_force(lengths, S):
    from viewformer_amd.render import plan_fork, plan_replication
    split, parent = plan_fork(np.array(lengths, dtype=np.int32), S)
    assert split.dtype == np.int32 and split.shape == parent.shape == (len(lengths) * S,)
    assert np.array_equal(parent, plan_replication(len(lengths), S))
    for b, n in enumerate(lengths):
        for s in range(S):
            assert split[b * S + s] == n and parent[b * S + s] == b            # scene b's children at b S ... b S + S - 1
    for bad, s in (([-1], 2), ([1], 0), ([[1]], 2), ([1.5], 2), ([True], 2)):
        with pytest.raises(ValueError):
            plan_fork(np.array(bad), s)


def test_the_own_lengths_of_a_fork_against_brute_force():
    from viewformer_amd.render import plan_fork_lengths
    split = np.array([0, 2, 5], dtype=np.int32)
    for own in range(4):
        got = plan_fork_lengths(split, split + own, 3)
        assert got.dtype == np.int32 and got.tolist() == [own] * 3
    assert plan_fork_lengths(np.array([], dtype=np.int32), np.array([], dtype=np.int32), 0).size == 0
    assert plan_fork_lengths(np.array([0]), np.array([0]), 0).tolist() == [0]                 # split 0, length 0
    with pytest.raises(ValueError):
        plan_fork_lengths(split, split + 4, 3)                                                # beyond the room
    with pytest.raises(ValueError):
        plan_fork_lengths(split, split - np.array([0, 1, 0]), 3)                              # inside the parent
    with pytest.raises(ValueError):
        plan_fork_lengths(split, split + np.array([1, 2, 1]), 3)                              # children grow together
    with pytest.raises(ValueError):
        plan_fork_lengths(split, split[:2], 3)


def test_the_best_choice_against_brute_force():
    from viewformer_amd.render import choose_best
    g = np.random.Generator(np.random.PCG64(7))
    for B, S in ((1, 1), (3, 4), (5, 7)):
        sc = g.integers(-3, 3, size=(B, S)).astype(np.float32)                                # small integers: many ties
        got = choose_best(sc)
        assert got.dtype == np.int64 and got.shape == (B,)
        for b in range(B):
            best = 0
            for s in range(1, S):
                if sc[b, s] > sc[b, best]:                                                    # strictly: a tie stays with the lowest index
                    best = s
            assert got[b] == best
    nan, inf = float('nan'), float('inf')
    assert choose_best([[nan, -inf, -inf], [nan, nan, nan], [1.0, nan, 1.0], [-inf, nan, -5.0]]).tolist() == [0, 0, 0, 2]
    for bad in ([1.0, 2.0], np.zeros((2, 0)), np.zeros((1, 2, 3))):
        with pytest.raises(ValueError):
            choose_best(bad)


# ---------------------------------------------------------------------------------------------- the entries' argument validation
P = ctypes.c_void_p
_ptr = lambda x: None if x is None else P(x)          # never dereferenced: validation happens before any launch
BASE = dict(q=4096, k=4096, v=4096, kp=8192, vp=8192, out=4096, B=4, H=2, C=3, N=5, L=64, dh=64, ldq=384, ldk=384, ldv=384, ldkp=384, ldvp=384,
            prefix_stride=3 * 64 * 384, ldo=128, ctx_len=4096, kp2=8192, vp2=8192, C2=2, ldkp2=384, ldvp2=384, prefix_stride2=2 * 64 * 384,
            split=4096, share=2)


def _call(lib, entry, **kw):
    a = dict(BASE, **kw)
    head = [_ptr(a[n]) for n in ('q', 'k', 'v', 'kp', 'vp')]
    if entry == 'bf16':
        head += [a.get('in_bf16', 1), _ptr(a['out']), a.get('out_bf16', 1)]
        fn = lib.vf_attn_prefix_fork_bf16
    else:
        head += [_ptr(a['out'])]
        fn = lib.vf_attn_prefix_fork_f32eq
    return fn(*head, a['B'], a['H'], a['C'], a['N'], a['L'], a['dh'], a['ldq'], a['ldk'], a['ldv'], a['ldkp'], a['ldvp'], a['prefix_stride'],
              a['ldo'], _ptr(a['ctx_len']), _ptr(a['kp2']), _ptr(a['vp2']), a['C2'], a['ldkp2'], a['ldvp2'], a['prefix_stride2'],
              _ptr(a['split']), a['share'], None)


@pytest.mark.parametrize('entry', ['bf16', 'bf16-f32in', 'f32eq'])
def test_the_fork_entries_validate_their_arguments_without_a_device(lib, entry):
    kind = 'bf16' if entry.startswith('bf16') else 'f32eq'
    extra = dict(in_bf16=0) if entry == 'bf16-f32in' else {}
    call = lambda **kw: _call(lib, kind, **extra, **kw)
    unit = 8 if entry == 'bf16' else 4                                         # elements per vector a row is read by
    for name in ('q', 'k', 'v', 'kp', 'vp', 'out', 'ctx_len', 'split', 'kp2', 'vp2'):
        assert call(**{name: None}) == -1, name                                # null pointers
        assert call(**{name: None}, B=0) == -1, name                           # ... also where there would be no work
    assert call(kp2=None, vp2=None, C2=0, B=0) == 0                            # C2 = 0: the own segment is never read
    assert call(share=0) == -1 and call(share=-3) == -1
    assert call(C2=-1) == -1
    for name in ('ldq', 'ldk', 'ldv', 'ldkp', 'ldvp', 'ldkp2', 'ldvp2', 'ldo'):
        assert call(**{name: 2 * 64 - 8}) == -1, name                          # a leading dimension below H * 64
    for name in ('ldq', 'ldk', 'ldv', 'ldkp', 'ldvp', 'ldkp2', 'ldvp2'):
        assert call(**{name: 384 + unit // 2}) == -1, name                     # rows are read as 8- / 16-byte vectors: both segments
    assert call(prefix_stride=3 * 64 * 384 + unit // 2) == -1
    assert call(prefix_stride2=2 * 64 * 384 + unit // 2) == -1
    assert call(prefix_stride2=-unit) == -1
    assert call(ldo=130) == -1
    assert call(L=32) == -2 and call(dh=32) == -2 and call(L=128) == -2 and call(dh=128) == -2
    assert call(B=0) == 0 and call(N=0) == 0                                   # nothing to do: no launch
    assert call(B=0, share=0) == -1 and call(N=0, ldkp2=100) == -1             # ... but bad arguments are still refused


def test_ops_attn_prefix_fork_refuses_cpu_tensors(lib):
    from viewformer_amd import ops, _lib
    d = 64
    q, par, own = torch.zeros(64, 3 * d), torch.zeros(64, 3 * d), torch.zeros(64, 3 * d)
    out, ln, sp = torch.zeros(64, d), torch.zeros(1, dtype=torch.int32), torch.zeros(1, dtype=torch.int32)
    args = lambda ln=ln, sp=sp, own=own: (q[:, d:2 * d], q[:, 2 * d:], q[:, :d], par[:, 2 * d:], par[:, :d], own[:, 2 * d:], own[:, :d], out,
                                          1, 1, 1, 1, 1, 64, 3 * d, 3 * d, 3 * d, 3 * d, 3 * d, 64 * 3 * d, 3 * d, 3 * d, 64 * 3 * d, d, ln, sp, 1)
    with pytest.raises(_lib.VfError):
        ops.attn_prefix_fork(*args())                                          # no CPU fallback for the hot path


# ---------------------------------------------------------------------------------------------- refusals that need no device
def _host_model():
    """a model object on the host that owns caches: enough for the checks that run before any launch"""
    from viewformer_amd.config import MIGTConfig
    from viewformer_amd.migt import MIGT
    m = MIGT(MIGTConfig(n_embeddings=64, n_head=2, d_model=128, n_layer=2, token_image_size=8, sequence_size=4))
    m.device, m._sd_host = torch.device('cpu'), {}
    m._act_dtypes = lambda: (False, False)
    return m


def _host_cache(m, B=2, C=2, lengths=None):
    from viewformer_amd.migt import ContextCache
    kv = [torch.zeros(B * C * 64, 3 * 128) for _ in range(2)]
    return ContextCache(m, kv, B, C, (8, 8), lengths=lengths)


def test_a_fork_counts_logical_views_and_allocates_only_its_own_room():
    m = _host_model()
    parent = _host_cache(m, lengths=[1, 2])
    child = parent.fork(3, room=4)
    assert child.forked() and not parent.forked() and child.B == 6 and child.share == 3 and child.room == 4
    assert child.split.dtype == np.int32 and child.split.tolist() == [1, 1, 1, 2, 2, 2]
    assert child.filled().tolist() == [1, 1, 1, 2, 2, 2] and child.C == 2 and child.capacity == 6 and child.ragged()
    assert [tuple(t.shape) for t in child.kv] == [(6 * 4 * 64, 384)] * 2
    assert all(a is b for a, b in zip(child.parent_kv, parent.kv)) and child.parent_kv is not parent.kv
    assert parent.fork(1).kv[0].shape[0] == 0                                  # no room until the first append
    for S, room in ((0, 1), (-1, 1), (1.5, 1), (True, 1), (2, -1), (2, 0.5), (40000, 0)):
        with pytest.raises(ValueError):
            parent.fork(S, room)


def test_a_fork_of_a_fork_is_refused_and_names_materialize():
    m = _host_model()
    child = _host_cache(m).fork(2, room=1)
    with pytest.raises(ValueError, match=r'materialize\(\)'):
        child.fork(2)
    with pytest.raises(ValueError, match=r'materialize\(\)'):
        m.rollout_from_context(child, torch.zeros(4, 1, 7), n_samples=2, fork=True)
    with pytest.raises(ValueError, match=r'materialize\(\)'):
        m.score_grad_from_context(child, torch.zeros(4, 1, 7), torch.zeros(4, 1, 8, 8, dtype=torch.int64))
    with pytest.raises(ValueError, match=r'materialize\(\)'):
        m.refine_from_context(child, torch.zeros(4, 1, 7), torch.zeros(4, 1, 8, 8, dtype=torch.int64))


def test_a_fork_belongs_to_its_model_and_the_fp8_arm_is_refused():
    from viewformer_amd import _lib
    m, other = _host_model(), _host_model()
    parent = _host_cache(m)
    child = parent.fork(2, room=1)
    with pytest.raises(ValueError, match='another model'):
        child.check(other)
    with pytest.raises(ValueError, match='another model'):
        other.adopt_from_fork(parent, child, [0, 0])
    m.attention = 'fp8'
    with pytest.raises((_lib.VfError, ValueError)):
        _host_cache(m).fork(2)


def test_adopt_refuses_a_foreign_child_a_grown_parent_and_bad_choices():
    m = _host_model()
    parent, stranger = _host_cache(m), _host_cache(m)
    child = parent.fork(2, room=1)
    with pytest.raises(ValueError, match='not forked from this parent'):
        m.adopt_from_fork(stranger, child, [0, 0])
    with pytest.raises(ValueError):
        m.adopt_from_fork(child, child, [0, 0])                                # the parent is a plain cache, the child a fork
    with pytest.raises(ValueError):
        m.adopt_from_fork(parent, stranger, [0, 0])
    for which in ([0], [0, 2], [-1, 0], [0.0, 1.0], [True, False], 'first'):
        with pytest.raises(ValueError):
            m.adopt_from_fork(parent, child, which)
    with pytest.raises(ValueError):
        m.adopt_from_fork(parent, child, 'best')                               # 'best' goes with a score
    with pytest.raises(ValueError):
        m.adopt_from_fork(parent, child, 'best', score=np.zeros((2, 3)))
    with pytest.raises(ValueError):
        m.adopt_from_fork(parent, child, [0, 1], score=np.zeros((2, 2)))
    assert m.adopt_from_fork(parent, child, 'best', score=np.array([[1.0, 1.0], [0.0, 2.0]])).tolist() == [0, 1]    # no own views: nothing moves
    assert parent.filled().tolist() == [2, 2]
    parent.C += 1                                                              # the parent grew after the fork
    with pytest.raises(ValueError, match='grown since the fork'):
        m.adopt_from_fork(parent, child, [0, 0])


def test_the_renderer_refuses_adopt_without_fork_and_gradients_on_a_fork():
    from viewformer_amd.render import ViewRenderer
    m = _host_model()
    r = ViewRenderer(m, None)
    with pytest.raises(RuntimeError):
        r.fork(2)
    r.cache = _host_cache(m)
    cams = torch.zeros(2, 1, 7)
    for kw in (dict(adopt='best'), dict(adopt='best', n_samples=2), dict(adopt=[0, 0], n_samples=2), dict(adopt='best', fork=True),
               dict(adopt='worst', fork=True, n_samples=2)):
        with pytest.raises(ValueError):
            r.rollout(cams, **kw)
    r.cache = r.cache.fork(2)
    with pytest.raises(ValueError, match=r'materialize\(\)'):
        r.score_gradient(torch.zeros(4, 1, 7), codes=torch.zeros(4, 1, 8, 8, dtype=torch.int64))
    with pytest.raises(ValueError, match=r'materialize\(\)'):
        r.refine(torch.zeros(4, 1, 7), codes=torch.zeros(4, 1, 8, 8, dtype=torch.int64))
