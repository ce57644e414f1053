"""CPU: the host side of a GROWING packed context cache (``vf_kv_append_e4m3``, ``vf_kv_append_split``,
``ContextCache.pack(room=...)``, ``MIGT.prefill_context(pack=...)``, ``ViewRenderer.pack(room=...)``) — both entries validate their
arguments before any launch, re-packing dequantised tiles keeps every value, the restatement of a launch equals brute force, the
K/V-only growing form keeps the source's values through ``reserve`` / ``replicate`` / ``unpack``, the byte counts follow from the
shapes, and the refusals that need no device refuse.  No device is touched."""
import ctypes

import numpy as np
import pytest
import torch

import kv_grow_ref as G
import kv_pack_ref as R
from test_pack_host import _host_cache, _host_model


@pytest.fixture(scope='module')
def lib():
    from viewformer_amd import build, _lib
    build.build()                      # hipcc cross-compiles gfx950 without a GPU
    return _lib.load()


def test_both_symbols_are_exported_declared_and_the_abi_number_stays(lib):
    import os
    from viewformer_amd import _lib
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'vf_hip.h')).read()
    for name in ('vf_kv_append_e4m3', 'vf_kv_append_split'):
        assert name in _lib.EXPORTS and hasattr(lib, name)
        assert f'int {name}(' in header
    assert lib.vf_abi_version() == 20                                          # the additions are additive


# ---------------------------------------------------------------------------------------------- the entries' argument validation
P = ctypes.c_void_p
_ptr = lambda x: None if x is None else P(x)          # never dereferenced: validation happens before any launch
H_ = 2
CAP = 3
E4 = dict(qkv=4096, elem_bytes=2, kq=8192, vq=8192, kscale=4096, vscale=4096, B=2, K=2, H=H_, L=64, ld_src=3 * 64 * H_,
          q_view_stride=4096 * H_, q_scene_stride=CAP * 4096 * H_, s_view_stride=H_, s_scene_stride=CAP * H_, capacity=CAP, pos=4096)


def _e4(lib, **kw):
    a = dict(E4, **kw)
    return lib.vf_kv_append_e4m3(_ptr(a['qkv']), a['elem_bytes'], _ptr(a['kq']), _ptr(a['vq']), _ptr(a['kscale']), _ptr(a['vscale']), a['B'], a['K'],
                                 a['H'], a['L'], a['ld_src'], a['q_view_stride'], a['q_scene_stride'], a['s_view_stride'], a['s_scene_stride'],
                                 a['capacity'], _ptr(a['pos']), None)


def test_the_e4m3_append_entry_validates_its_arguments_without_a_device(lib):
    call = lambda **kw: _e4(lib, **kw)
    for name in ('qkv', 'kq', 'vq', 'kscale', 'vscale', 'pos'):
        assert call(**{name: None}) == -1, name
        assert call(**{name: None}, B=0) == -1, name                           # ... also where there would be no work
    for name in ('qkv', 'kq', 'vq'):
        assert call(**{name: 4096 + 8}) == -1, name                            # 16-byte vectors
    assert call(kscale=4096 + 2) == -1 and call(vscale=4096 + 1) == -1
    assert call(elem_bytes=1) == -1 and call(elem_bytes=8) == -1
    assert call(B=-1) == -1 and call(K=-1) == -1 and call(H=0) == -1 and call(capacity=-1) == -1
    assert call(ld_src=3 * 64 * H_ - 8) == -1                                  # below the three thirds
    assert call(ld_src=3 * 64 * H_ + 4) == -1 and call(ld_src=3 * 64 * H_ + 2, elem_bytes=4) == -1
    assert call(q_view_stride=4096 * H_ - 16) == -1 and call(q_view_stride=4096 * H_ + 8) == -1
    assert call(q_scene_stride=E4['q_scene_stride'] + 8) == -1 and call(q_scene_stride=-16) == -1
    assert call(q_scene_stride=(CAP - 1) * 4096 * H_) == -1 and call(s_scene_stride=(CAP - 1) * H_) == -1      # capacity views overlap the next scene
    assert call(s_view_stride=H_ - 1) == -1 and call(s_scene_stride=-1) == -1
    assert call(L=32) == -2 and call(L=128) == -2
    assert call(H=70000, ld_src=3 * 64 * 70000, q_view_stride=4096 * 70000, s_view_stride=70000, B=1) == -2     # grid dimension y
    assert call(B=1 << 16, K=1 << 15, q_scene_stride=0, s_scene_stride=0, capacity=0) == -2                     # B K above 2^31 - 1
    assert call(B=0) == 0 and call(K=0) == 0 and call(capacity=0) == 0         # nothing to do: no launch
    assert call(B=0, elem_bytes=3) == -1 and call(K=0, ld_src=8) == -1 and call(capacity=0, pos=None) == -1    # ... but bad arguments are still refused
    assert call(B=0, L=32) == -2
    assert call(ld_src=3 * 64 * H_ + 8, q_scene_stride=E4['q_scene_stride'] + 256, s_scene_stride=E4['s_scene_stride'] + 5, B=0) == 0     # padding is fine


SP = dict(qkv=4096, k=8192, v=8192, elem_bytes=2, B=2, K=2, L=64, d=128, ld_src=384, ld_k=128, ld_v=136, k_stride=CAP * 64 * 128,
          v_stride=CAP * 64 * 136, capacity=CAP, pos=4096)


def _sp(lib, **kw):
    a = dict(SP, **kw)
    return lib.vf_kv_append_split(_ptr(a['qkv']), _ptr(a['k']), _ptr(a['v']), a['elem_bytes'], a['B'], a['K'], a['L'], a['d'], a['ld_src'], a['ld_k'],
                                  a['ld_v'], a['k_stride'], a['v_stride'], a['capacity'], _ptr(a['pos']), None)


def test_the_split_append_entry_validates_its_arguments_without_a_device(lib):
    call = lambda **kw: _sp(lib, **kw)
    for name in ('qkv', 'k', 'v', 'pos'):
        assert call(**{name: None}) == -1, name
        assert call(**{name: None}, B=0) == -1, name
    for name in ('qkv', 'k', 'v'):
        assert call(**{name: 4096 + 8}) == -1, name
    assert call(elem_bytes=1) == -1 and call(elem_bytes=8) == -1
    for name in ('B', 'K', 'L', 'd', 'capacity', 'k_stride', 'v_stride'):
        assert call(**{name: -1}) == -1, name
    assert call(ld_src=3 * 128 - 8) == -1 and call(ld_k=120) == -1 and call(ld_v=120) == -1
    assert call(d=132, ld_src=400, ld_k=136) == -1                             # d * elem_bytes: whole 16-byte chunks
    assert call(ld_src=388) == -1 and call(ld_k=132) == -1 and call(ld_v=132) == -1
    assert call(k_stride=SP['k_stride'] + 4) == -1 and call(v_stride=SP['v_stride'] + 4) == -1
    assert call(k_stride=(CAP - 1) * 64 * 128) == -1 and call(v_stride=(CAP - 1) * 64 * 136) == -1             # scenes overlap
    assert call(B=1 << 16, K=1 << 15, capacity=0) == -2                        # B K above 2^31 - 1
    assert call(L=1 << 26, d=1 << 10, ld_src=3 << 10, ld_k=1 << 10, ld_v=1 << 10, B=1) == -2                   # chunks of one view above 2^31 - 1
    for name in ('B', 'K', 'L', 'd', 'capacity'):
        assert call(**{name: 0}) == 0, name                                    # nothing to do: no launch
    assert call(B=0, elem_bytes=3) == -1 and call(K=0, ld_k=8) == -1 and call(capacity=0, pos=None) == -1      # ... but bad arguments are still refused
    assert call(B=0, ld_k=144, k_stride=CAP * 64 * 144 + 8) == 0               # a wider row and a gap are fine


def test_the_ops_refuse_cpu_tensors_and_wrong_dtypes(lib):
    from viewformer_amd import ops, _lib
    d = 64
    qkv = torch.zeros(64, 3 * d)
    kq, vq = torch.zeros(1, 1, 64, 64, dtype=torch.uint8), torch.zeros(1, 1, 64, 64, dtype=torch.uint8)
    ks, vs, pos = torch.ones(1, 1), torch.ones(1, 1), torch.zeros(1, dtype=torch.int32)
    with pytest.raises(_lib.VfError):
        ops.kv_append_e4m3(qkv, kq, vq, ks, vs, 1, 1, 1, 64, 3 * d, 1, pos)    # no CPU fallback
    with pytest.raises(TypeError):
        ops.kv_append_e4m3(qkv.half(), kq, vq, ks, vs, 1, 1, 1, 64, 3 * d, 1, pos)
    k, v = torch.zeros(64, d), torch.zeros(64, d)
    with pytest.raises(_lib.VfError):
        ops.kv_append_split(qkv, k, v, 1, 1, 64, d, 3 * d, d, d, 64 * d, 64 * d, 1, pos)
    with pytest.raises(TypeError):
        ops.kv_append_split(qkv.half(), k, v, 1, 1, 64, d, 3 * d, d, d, 64 * d, 64 * d, 1, pos)


# ---------------------------------------------------------------------------------------------- why the reference loop compares by value
def test_repacking_dequantised_tiles_keeps_every_value_and_may_change_the_scale():
    g = torch.Generator().manual_seed(23)
    x = (torch.randn(40, 192, 64, 64, generator=g) * torch.exp2(torch.arange(-20, 20).float().view(40, 1, 1, 1))).bfloat16().float()
    k = 5
    x[7, 3].clamp_(-100 * 2.0 ** k, 100 * 2.0 ** k)
    x[7, 3, 11, 13] = 225.0 * 2.0 ** k                                          # absmax 225 * 2^k: scale 2^k, and 225 rounds DOWN to 224 = 1.75 * 2^7
    q1, s1 = R.pack_tiles(x)
    v1 = R.unpack_tiles(q1, s1)
    q2, s2 = R.pack_tiles(v1)
    v2 = R.unpack_tiles(q2, s2)
    assert torch.equal(v2, v1)                                                 # every element, every tile
    assert s1[7, 3].item() == 2.0 ** k and s2[7, 3].item() == 2.0 ** (k - 1)   # the planted tile: a smaller scale, ...
    assert not torch.equal(q1[7, 3].view(torch.uint8), q2[7, 3].view(torch.uint8))       # ... other bytes, the same values
    changed = int((s1 != s2).sum())
    assert 0 < changed < 40 * 192 // 2 and bool((s2 <= s1).all())              # the scale never grows
    assert torch.equal(R.pack_tiles(v1.bfloat16())[0].view(torch.uint8), q2.view(torch.uint8))     # dequantised values are bf16 numbers


# ---------------------------------------------------------------------------------------------- the restatement against brute force
def test_the_restatement_of_a_launch_against_brute_force():
    B, K, H, cap = 2, 3, 2, 4
    d = 64 * H
    g = torch.Generator().manual_seed(4)
    qkv = torch.randn(B * K * 64, 3 * d, generator=g) * 3
    pos = [-1, 2]                                                              # scene 0: view 0 skipped (slot -1); scene 1: view 2 overflows (slot 4)
    kq = torch.full((B, cap, H, 64, 64), 0x5A, dtype=torch.uint8)
    ks = torch.full((B, cap, H), -7.0)
    nkq, nvq, nks, nvs = G.append_e4m3(qkv, kq, kq.clone(), ks, ks.clone(), B, K, H, cap, pos)
    lut = torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).float()
    written = set()
    for b, j, slot in ((0, 1, 0), (0, 2, 1), (1, 0, 2), (1, 1, 3)):
        rows = qkv[(b * K + j) * 64:(b * K + j + 1) * 64]
        for h in range(H):
            kt, vt = rows[:, 2 * d + 64 * h:2 * d + 64 * (h + 1)], rows[:, 64 * h:64 * (h + 1)]
            for tile, q, s in ((kt, nkq, nks), (vt.t(), nvq, nvs)):
                e = R.brute_exponent(tile.abs().max().item())
                assert s[b, slot, h].item() == 2.0 ** e
                for r, c in ((0, 0), (5, 60), (63, 63), (17, 2)):               # element by element: x * 2^-e through the e4m3 cast
                    want = (tile[r, c] * 2.0 ** -e).clamp(-448, 448).to(torch.float8_e4m3fn).float().item()
                    assert lut[q[b, slot, h, r, c].long()].item() == want
        written.add((b, slot))
    for b in range(B):
        for slot in range(cap):
            if (b, slot) not in written:                                       # every other slot keeps its bytes and scales
                assert bool((nkq[b, slot] == 0x5A).all()) and bool((nvq[b, slot] == 0x5A).all())
                assert bool((nks[b, slot] == -7.0).all()) and bool((nvs[b, slot] == -7.0).all())
    assert written == {(0, 0), (0, 1), (1, 2), (1, 3)}
    k0 = torch.full((B, cap * 64, d), -5.0)
    nk, nv = G.append_split(qkv, k0, k0.clone(), B, K, d, cap, pos)
    x = qkv.view(B, K, 64, 3 * d)
    assert torch.equal(nk[0, :64], x[0, 1, :, 2 * d:]) and torch.equal(nv[0, 64:128], x[0, 2, :, :d])
    assert torch.equal(nk[1, 192:], x[1, 1, :, 2 * d:]) and torch.equal(nv[1, 128:192], x[1, 0, :, :d])
    assert bool((nk[0, 128:] == -5).all()) and bool((nv[1, :128] == -5).all())


# ---------------------------------------------------------------------------------------------- the K/V-only growing form on the host
def _thirds(kv, B, cap, C, d):
    full = kv.view(B, cap * 64, 3 * d)[:, :C * 64]
    return full[:, :, 2 * d:], full[:, :, :d]


def test_pack_with_room_on_a_host_kv_cache_keeps_the_values_and_grows():
    from viewformer_amd.context_cache import GrowingKVCache, PackedKVCache
    m = _host_model()
    src = _host_cache(m, B=2, C=2, lengths=[1, 2], capacity=3)
    before = [t.clone() for t in src.kv]
    g = src.pack(room=3)
    assert isinstance(g, GrowingKVCache) and isinstance(g, PackedKVCache) and g.packed == 'kv' and src.packed is None
    assert g.B == 2 and g.C == 2 and g.capacity == 5 and g.lengths.tolist() == [1, 2] and g.ragged()
    assert all(torch.equal(a, b) for a, b in zip(before, src.kv))              # the source is left untouched
    for (k, v), kv in zip(g.kv, src.kv):
        assert k.shape == v.shape == (2 * 5 * 64, 128) and k.is_contiguous() and v.is_contiguous()
        sk, sv = _thirds(kv, 2, 3, 2, 128)
        assert torch.equal(k.view(2, 320, 128)[:, :128], sk) and torch.equal(v.view(2, 320, 128)[:, :128], sv)
        assert bool((k.view(2, 320, 128)[:, 128:] == 0).all()) and bool((v.view(2, 320, 128)[:, 128:] == 0).all())      # the slack: zeros
    assert src.pack(room=0).capacity == 2 and src.pack(room=np.int64(1)).capacity == 3
    assert _host_cache(m).pack(room=0).lengths is None                         # lengths are data, as in the plain form
    # reserve: within the capacity nothing moves; beyond it the cache grows by plan_capacity and keeps every value
    held = [tuple(t for t in ts) for ts in g.kv]
    g.reserve(5)
    assert g.capacity == 5 and all(a is b for x, y in zip(held, g.kv) for a, b in zip(x, y))
    g.reserve(6)
    assert g.capacity == 10                                                    # max(2 * 5, 6)
    for (k, v), (ok, ov) in zip(g.kv, held):
        assert k.shape == (2 * 10 * 64, 128)
        assert torch.equal(k.view(2, 640, 128)[:, :320], ok.view(2, 320, 128)) and torch.equal(v.view(2, 640, 128)[:, :320], ov.view(2, 320, 128))
    g.reserve(27)
    assert g.capacity == 27                                                    # max(2 * 10, 27)
    g.grown(g.filled(), 2)
    assert g.lengths.tolist() == [3, 4] and g.C == 4
    # replicate: scene b's copies at b S ...
    r = g.replicate(3)
    assert type(r) is GrowingKVCache and r.B == 6 and r.capacity == 27 and r.lengths.tolist() == [3, 3, 3, 4, 4, 4]
    for (k, v), (rk, rv) in zip(g.kv, r.kv):
        assert torch.equal(rk.view(2, 3, -1), k.view(2, 1, -1).expand(2, 3, -1)) and torch.equal(rv.view(2, 3, -1), v.view(2, 1, -1).expand(2, 3, -1))
    # alias: the same buffers, lengths of its own
    a = g.alias()
    a.grown(a.filled(), 1)
    assert a.kv[0][0] is g.kv[0][0] and g.lengths.tolist() == [3, 4] and a.lengths.tolist() == [4, 5]
    # unpack: a plain cache of the same capacity and lengths, the stored bits, the Q third zeros
    u = g.unpack()
    assert u.packed is None and u.capacity == 27 and u.lengths.tolist() == [3, 4] and u.C == 4
    for t, (k, v) in zip(u.kv, g.kv):
        assert t.shape == (2 * 27 * 64, 384)
        assert torch.equal(t[:, 256:], k) and torch.equal(t[:, :128], v) and bool((t[:, 128:256] == 0).all())


def test_the_byte_counts_of_the_growing_forms_from_shapes():
    from viewformer_amd.render import plan_cache_bytes
    m = _host_model()
    g = _host_cache(m, B=2, C=2).pack(room=3)
    assert g.nbytes() == plan_cache_bytes(2, 5, 64, 128, 2, 2, 4, 'kv') == 2 * 2 * 2 * 5 * 64 * 128 * 4
    assert 3 * g.nbytes() == 2 * _host_cache(m, B=2, C=5).nbytes()             # 2/3 of the plain cache of the same capacity
    for B, cap in ((1, 19), (16, 35)):
        q = plan_cache_bytes(B, cap, 64, 768, 12, 12, 2, 'e4m3')
        assert q == 12 * 2 * (B * cap * 12 * 4096 + B * cap * 12 * 4)          # kq, vq [B*cap, H, 64, 64] bytes; kscale, vscale [B*cap, H] fp32
        assert round(q / plan_cache_bytes(B, cap, 64, 768, 12, 12, 2), 4) == 0.3337
    from viewformer_amd.context_cache import GrowingE4M3Cache
    t = GrowingE4M3Cache.buffers(2, 5, 2, torch.device('cpu'))
    assert [tuple(x.shape) for x in t] == [(10, 2, 64, 64), (10, 2, 64, 64), (10, 2), (10, 2)]
    assert [x.dtype for x in t] == [torch.uint8, torch.uint8, torch.float32, torch.float32]
    assert 2 * sum(x.numel() * x.element_size() for x in t) == plan_cache_bytes(2, 5, 64, 128, 2, 2, 2, 'e4m3')


# ---------------------------------------------------------------------------------------------- refusals that need no device
def test_a_bad_room_and_e4m3_on_the_f32_arm_are_refused():
    m = _host_model()
    c = _host_cache(m)
    for bad in (True, False, -1, 1.0, 2.5, '2', [1]):
        with pytest.raises(ValueError, match='room'):
            c.pack(room=bad)
        with pytest.raises(ValueError):
            c.pack('e4m3', room=bad)
    with pytest.raises(ValueError, match=r"precision='bf16'"):
        c.pack('e4m3', room=2)                                                 # refused like pack('e4m3')
    with pytest.raises(ValueError, match=r"precision='bf16'"):
        m.prefill_context(torch.zeros(2, 2, 8, 8, dtype=torch.int64), torch.zeros(2, 2, 7), pack='e4m3')
    for bad in ('fp8', True, 8):
        with pytest.raises(ValueError, match='pack'):
            m.prefill_context(torch.zeros(2, 2, 8, 8, dtype=torch.int64), torch.zeros(2, 2, 7), pack=bad)


def test_a_growing_cache_refuses_forks_packs_the_backward_and_adoption_and_names_unpack():
    m = _host_model()
    parent = _host_cache(m)
    child = parent.fork(2, room=1)
    g = parent.pack(room=2)
    cams, codes = torch.zeros(2, 1, 7), torch.zeros(2, 1, 8, 8, dtype=torch.int64)
    calls = [lambda: g.fork(2),
             lambda: g.materialize(),
             lambda: g.pack(),
             lambda: g.pack(room=1),
             lambda: g.pack('e4m3'),
             lambda: g.attend_backward(0, None, None, None, 1, None),
             lambda: g.plan_pass(torch.zeros(2, dtype=torch.int32), None, save=[]),
             lambda: m.adopt_from_fork(g, child, [0, 0]),
             lambda: m.adopt_from_fork(parent, g, [0, 0]),
             lambda: m.score_grad_from_context(g, cams, codes),
             lambda: m.refine_from_context(g, cams, codes),
             lambda: m.rollout_from_context(g, cams, fork=True),
             lambda: m.rollout_from_context(g, cams, n_samples=2, fork=True)]
    for i, f in enumerate(calls):
        with pytest.raises(ValueError, match=r'unpack\(\)'):
            f()
    assert g.packed == 'kv' and g.C == 2 and g.capacity == 4                   # nothing happened to it
    g.refuse_growth('append_to_context')                                       # what it is for: no refusal
    t = parent.pack()                                                          # without room: read-only as before
    for f in (lambda: m.append_to_context(t, codes, cams), lambda: m.rollout_from_context(t, cams), lambda: t.reserve(9)):
        with pytest.raises(ValueError, match=r'unpack\(\)'):
            f()


def test_the_renderer_packs_with_room_and_keeps_refusing_forks_and_gradients():
    from viewformer_amd.render import ViewRenderer
    m = _host_model()
    r = ViewRenderer(m, None)
    with pytest.raises(RuntimeError):
        r.pack(room=1)
    r.cache = _host_cache(m)
    plain = r.context_bytes()
    with pytest.raises(ValueError, match='room'):
        r.pack(room=-1)
    assert r.cache.packed is None
    assert r.pack(room=2) is r and r.cache.packed == 'kv' and r.cache.capacity == 4
    assert 3 * r.context_bytes() == 2 * 2 * plain                              # the K and V thirds of twice the views
    cams, codes = torch.zeros(2, 1, 7), torch.zeros(2, 1, 8, 8, dtype=torch.int64)
    for f in (lambda: r.fork(2), lambda: r.score_gradient(cams, codes=codes), lambda: r.refine(cams, codes=codes),
              lambda: r.rollout(cams, fork=True), lambda: r.rollout(cams, n_samples=2, fork=True), lambda: r.pack(), lambda: r.pack(room=1)):
        with pytest.raises(ValueError, match=r'unpack\(\)'):
            f()
    assert r.unpack() is r and r.cache.packed is None and r.cache.capacity == 4 and r.context_bytes() == 2 * plain
    assert r.cache.fork(2).forked()                                            # works again
    r.pack()
    for f in (lambda: r.append(codes=codes, cameras=cams), lambda: r.rollout(cams)):      # pack() without room still refuses what grows
        with pytest.raises(ValueError, match=r'unpack\(\)'):
            f()
