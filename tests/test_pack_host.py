"""CPU: the host side of a packed context cache (``vf_kv_pack_e4m3``, ``vf_attn_prefix_q8_bf16``, ``ContextCache.pack`` /
``unpack``, ``ViewRenderer.pack`` / ``unpack``) — the scale's bit rule equals brute force, the restatement dequantises to bf16 numbers,
the byte counts follow from the shapes, both new entries validate their arguments before any launch, and the refusals that need no
device refuse.  No device is touched."""
import ctypes

import numpy as np
import pytest
import torch

import kv_pack_ref as R


@pytest.fixture(scope='module')
def lib():
    from viewformer_amd import build, _lib
    build.build()                      # hipcc cross-compiles gfx950 without a GPU
    return _lib.load()


# ---------------------------------------------------------------------------------------------- the scale: bit rule against brute force
def _boundaries():
    vals = [0.0, float('inf'), 448.0, float(np.nextafter(np.float32(448.0), np.float32(1e9))), float(np.nextafter(np.float32(448.0), np.float32(0)))]
    for k in range(-130, 128, 7):
        for m in (1.0, 1.75, 1.5):
            x = np.float32(m) * np.float32(2.0) ** np.float32(k)
            if np.isfinite(x) and x > 0:
                vals += [float(x), float(np.nextafter(x, np.float32(np.inf))), float(np.nextafter(x, np.float32(0)))]
    vals += [float(np.float32(448.0) * np.float32(2.0) ** k) for k in range(-120, 119, 9)]
    vals += [float(np.finfo(np.float32).tiny), float(np.finfo(np.float32).max), 1e-45, 3e-39]
    return [v for v in vals if np.isfinite(v) or v == float('inf')]


def test_the_exponent_rule_against_brute_force():
    g = torch.Generator().manual_seed(11)
    mags = torch.exp2(torch.rand(2000, generator=g) * 250 - 125) * (1 + torch.rand(2000, generator=g))
    vals = torch.cat([mags.float(), torch.tensor(_boundaries(), dtype=torch.float32)])
    got = R.pack_exponent(vals)
    assert got.dtype == torch.int32
    for a, e in zip(vals.tolist(), got.tolist()):
        assert e == R.brute_exponent(a), (a, e)
    # where the definition is not clamped: the scale covers absmax, and the next smaller one does not
    ok = (vals > 0) & torch.isfinite(vals) & (got > R.E_MIN) & (got < R.E_MAX)
    v, e = vals[ok].double(), got[ok].double()
    assert bool((v <= 448.0 * torch.exp2(e)).all()) and bool((v > 448.0 * torch.exp2(e - 1)).all())
    assert R.pack_exponent(torch.tensor([448.0])).item() == 0 and R.pack_exponent(torch.tensor([448.0 * (1 + 2.0 ** -23)])).item() == 1
    assert R.pack_exponent(torch.tensor([1.75, 1.7500001, 1.0, 0.0, float('inf')])).tolist() == [-8, -7, -8, 0, 0]


# ---------------------------------------------------------------------------------------------- the restatement's numbers
def test_dequantised_values_are_bf16_numbers_and_finite_inputs_stay_finite():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(6, 3, 64, 64, generator=g) * torch.exp2(torch.randint(-110, 100, (6, 3, 1, 1), generator=g).float())
    x[0, 0] = 0
    x[1, 1, 3, 5] = 448.0 * 2.0 ** 40                                         # absmax exactly 448 * 2^k
    x[2, 2] *= 1e-30
    q, s = R.pack_tiles(x)
    assert q.dtype == torch.float8_e4m3fn and s.shape == (6, 3) and s.dtype == torch.float32
    v = R.unpack_tiles(q, s)
    assert not torch.isnan(v).any() and torch.isfinite(v).all()               # no finite input packs to NaN (0x7f / 0xff)
    assert torch.equal(v.bfloat16().float(), v)                               # 3 mantissa bits times a power of two: a bf16 number
    assert bool(((v == 0) | (v.abs() >= torch.finfo(torch.bfloat16).tiny)).all())      # never a subnormal
    assert s[0, 0].item() == 1.0 and bool((v[0, 0] == 0).all())               # an all-zero tile gets scale 1
    assert v[1, 1, 3, 5].item() == 448.0 * 2.0 ** 40
    am = x.abs().amax((-2, -1))
    assert bool((v.abs().amax((-2, -1)) <= am * (1 + 2.0 ** -4)).all())
    # the rounding error: half an e4m3 ulp of the value, and 2^-10 of the scale in the subnormal range
    err = (v - x).abs()
    bound = torch.maximum(x.abs() * 2.0 ** -4, s[..., None, None] * 2.0 ** -10)
    assert bool((err <= bound).all())


def test_ties_round_to_even_small_values_vanish_and_nan_stays():
    x = torch.zeros(1, 64, 64)
    x[0, 0, 0] = 448.0                                                        # scale 1
    x[0, 1, :6] = torch.tensor([17.0, 19.0, 21.0, 23.0, 2.0 ** -10, 2.0 ** -10 * 1.01])     # e4m3 steps of 2 in [16, 32): ties at odd integers
    x[0, 2, :4] = torch.tensor([3 * 2.0 ** -10, 5 * 2.0 ** -10, 2.0 ** -9, -2.0 ** -11])    # subnormal steps of 2^-9: ties at odd multiples of 2^-10
    x[0, 3, 0] = float('nan')
    q, s = R.pack_tiles(x)
    v = R.unpack_tiles(q, s)[0]
    assert s.item() == 1.0
    assert v[1, :4].tolist() == [16.0, 20.0, 20.0, 24.0]                      # to the even mantissa
    # the smallest e4m3 step is 2^-9 of the scale: under round-to-nearest-even what is below HALF of it vanishes, the half itself ties to
    # 0 (even), and (2^-10, 2^-9) rounds up to 2^-9 — "below 2^-9 goes to 0" holds for the magnitudes below 2^-10 only
    assert v[1, 4].item() == 0.0 and v[1, 5].item() == 2.0 ** -9
    small = torch.zeros(1, 64, 64)
    small[0, 0, 0] = 448.0
    small[0, 1] = torch.linspace(-1, 1, 64) * 2.0 ** -10 * 0.999
    assert bool((R.unpack_tiles(*R.pack_tiles(small))[0, 1] == 0).all())
    assert v[2, :4].tolist() == [2 * 2.0 ** -9, 2 * 2.0 ** -9, 2.0 ** -9, 0.0]
    assert torch.isnan(v[3, 0]) and int(torch.isnan(v).sum()) == 1            # the NaN stays, alone, and did not enter absmax
    y = torch.full((1, 64, 64), 1.0)
    y[0, 0, 0], y[0, 0, 1] = float('inf'), float('-inf')
    y[0, 0, 2] = 500.0
    qy, sy = R.pack_tiles(y)
    vy = R.unpack_tiles(qy, sy)[0]
    assert sy.item() == 1.0 and vy[0, :3].tolist() == [448.0, -448.0, 448.0] and vy[1, 1].item() == 1.0     # absmax not finite: scale 1, saturation


# ---------------------------------------------------------------------------------------------- bytes from shapes
def test_the_byte_counts_from_shapes():
    from viewformer_amd.render import plan_cache_bytes
    for B, C in ((1, 6), (16, 19), (3, 1)):
        plain16 = plan_cache_bytes(B, C, 64, 768, 12, 12, 2)
        plain32 = plan_cache_bytes(B, C, 64, 768, 12, 12, 4)
        assert plain16 == 12 * B * C * 64 * 2304 * 2 and plain32 == 2 * plain16
        assert 3 * plan_cache_bytes(B, C, 64, 768, 12, 12, 2, 'kv') == 2 * plain16         # exactly 2/3, either dtype
        assert 3 * plan_cache_bytes(B, C, 64, 768, 12, 12, 4, 'kv') == 2 * plain32
        q = plan_cache_bytes(B, C, 64, 768, 12, 12, 2, 'e4m3')
        assert q < 0.34 * plain16 and abs(q / plain16 - (2 * 768 * 64 + 2 * 12 * 4) / (6 * 768 * 64)) < 1e-12
        assert round(q / plain16, 4) == 0.3337
    assert plan_cache_bytes(1, 6, 64, 768, 12, 12, 2) == 21233664                          # 21 MB per scene at C = 6, bf16
    for bad in (dict(form='fp8'), dict(elem_bytes=3), dict(B=-1)):
        kw = dict(B=1, C=1, L=64, d_model=768, n_head=12, n_layer=12, elem_bytes=2)
        kw.update(bad)
        with pytest.raises(ValueError):
            plan_cache_bytes(**kw)


# ---------------------------------------------------------------------------------------------- the entries' argument validation
P = ctypes.c_void_p
_ptr = lambda x: None if x is None else P(x)          # never dereferenced: validation happens before any launch
H_ = 2
PACK = dict(cache=4096, elem_bytes=2, kq=8192, vq=8192, kscale=4096, vscale=4096, B=2, C=3, H=H_, L=64, ld_src=3 * 64 * H_,
            cache_stride=3 * 64 * 3 * 64 * H_, q_view_stride=4096 * H_, q_scene_stride=3 * 4096 * H_, s_view_stride=H_, s_scene_stride=3 * H_,
            lengths=4096)


def _pack(lib, **kw):
    a = dict(PACK, **kw)
    return lib.vf_kv_pack_e4m3(_ptr(a['cache']), a['elem_bytes'], _ptr(a['kq']), _ptr(a['vq']), _ptr(a['kscale']), _ptr(a['vscale']), a['B'], a['C'],
                               a['H'], a['L'], a['ld_src'], a['cache_stride'], a['q_view_stride'], a['q_scene_stride'], a['s_view_stride'],
                               a['s_scene_stride'], _ptr(a['lengths']), None)


def test_the_pack_entry_validates_its_arguments_without_a_device(lib):
    call = lambda **kw: _pack(lib, **kw)
    for name in ('cache', 'kq', 'vq', 'kscale', 'vscale', 'lengths'):
        assert call(**{name: None}) == -1, name
        assert call(**{name: None}, B=0) == -1, name                           # ... also where there would be no work
    for name in ('cache', 'kq', 'vq'):
        assert call(**{name: 4096 + 8}) == -1, name                            # 16-byte vectors
    assert call(elem_bytes=1) == -1 and call(elem_bytes=8) == -1
    assert call(B=-1) == -1 and call(C=-1) == -1 and call(H=0) == -1 and call(cache_stride=-8) == -1
    assert call(ld_src=3 * 64 * H_ - 8) == -1                                  # below the three thirds
    assert call(ld_src=3 * 64 * H_ + 4) == -1 and call(ld_src=3 * 64 * H_ + 2, elem_bytes=4) == -1
    assert call(cache_stride=PACK['cache_stride'] + 4) == -1
    assert call(q_view_stride=4096 * H_ - 16) == -1 and call(q_view_stride=4096 * H_ + 8) == -1
    assert call(q_scene_stride=PACK['q_scene_stride'] + 8) == -1 and call(q_scene_stride=-16) == -1
    assert call(q_scene_stride=2 * 4096 * H_) == -1 and call(s_scene_stride=2 * H_) == -1 and call(cache_stride=64 * 3 * 64 * H_) == -1   # scenes overlap
    assert call(s_view_stride=H_ - 1) == -1 and call(s_scene_stride=-1) == -1
    assert call(L=32) == -2 and call(L=128) == -2
    assert call(H=70000, ld_src=3 * 64 * 70000, q_view_stride=4096 * 70000, s_view_stride=70000, B=1) == -2     # grid dimension y
    assert call(B=0) == 0 and call(C=0) == 0                                   # nothing to do: no launch
    assert call(B=0, elem_bytes=3) == -1 and call(C=0, ld_src=8) == -1         # ... but bad arguments are still refused
    assert call(ld_src=3 * 64 * H_ + 8, cache_stride=PACK['cache_stride'] + 3 * 64 * 8 + 8, B=0) == 0    # a wider row and a gap are fine


Q8 = dict(q=4096, k=4096, v=4096, kq=8192, vq=8192, kscale=4096, vscale=4096, in_bf16=1, out=4096, out_bf16=1, B=4, H=H_, C=3, N=5, L=64, dh=64,
          ldq=384, ldk=384, ldv=384, q_view_stride=4096 * H_, q_scene_stride=3 * 4096 * H_, s_view_stride=H_, s_scene_stride=3 * H_, ldo=128,
          ctx_len=4096)


def _q8(lib, **kw):
    a = dict(Q8, **kw)
    return lib.vf_attn_prefix_q8_bf16(_ptr(a['q']), _ptr(a['k']), _ptr(a['v']), _ptr(a['kq']), _ptr(a['vq']), _ptr(a['kscale']), _ptr(a['vscale']),
                                      a['in_bf16'], _ptr(a['out']), a['out_bf16'], a['B'], a['H'], a['C'], a['N'], a['L'], a['dh'], a['ldq'], a['ldk'],
                                      a['ldv'], a['q_view_stride'], a['q_scene_stride'], a['s_view_stride'], a['s_scene_stride'], a['ldo'],
                                      _ptr(a['ctx_len']), None)


@pytest.mark.parametrize('in_bf16', [1, 0])
def test_the_q8_entry_validates_its_arguments_without_a_device(lib, in_bf16):
    call = lambda **kw: _q8(lib, in_bf16=in_bf16, **kw)
    unit = 8 if in_bf16 else 4
    for name in ('q', 'k', 'v', 'kq', 'vq', 'kscale', 'vscale', 'out', 'ctx_len'):
        assert call(**{name: None}) == -1, name
        assert call(**{name: None}, B=0) == -1, name
    for name in ('ldq', 'ldk', 'ldv', 'ldo'):
        assert call(**{name: H_ * 64 - 8}) == -1, name                         # the VAR entry's checks
    for name in ('ldq', 'ldk', 'ldv'):
        assert call(**{name: 384 + unit // 2}) == -1, name
    assert call(ldo=130) == -1
    assert call(L=32) == -2 and call(dh=32) == -2 and call(C=0) == -2
    assert call(kq=8192 + 8) == -1 and call(vq=8192 + 4) == -1                 # tiles are fetched as 16-byte vectors
    assert call(q_view_stride=4096 * H_ - 16) == -1 and call(q_view_stride=4096 * H_ + 8) == -1
    assert call(q_scene_stride=3 * 4096 * H_ + 4) == -1 and call(q_scene_stride=-16) == -1
    assert call(s_view_stride=H_ - 1) == -1 and call(s_scene_stride=-1) == -1
    assert call(B=0) == 0 and call(N=0) == 0
    assert call(B=0, q_view_stride=8) == -1 and call(N=0, kscale=None) == -1


def test_both_symbols_are_exported_and_the_abi_number_stays(lib):
    from viewformer_amd import _lib
    for name in ('vf_kv_pack_e4m3', 'vf_attn_prefix_q8_bf16'):
        assert name in _lib.EXPORTS and hasattr(lib, name)
    assert lib.vf_abi_version() == 20                                          # the additions are additive


def test_the_ops_refuse_cpu_tensors_and_wrong_dtypes(lib):
    from viewformer_amd import ops, _lib
    d = 64
    cache = torch.zeros(64, 3 * d)
    kq, vq = torch.zeros(1, 1, 64, 64, dtype=torch.uint8), torch.zeros(1, 1, 64, 64, dtype=torch.uint8)
    ks, vs, ln = torch.ones(1, 1), torch.ones(1, 1), torch.ones(1, dtype=torch.int32)
    with pytest.raises(_lib.VfError):
        ops.kv_pack_e4m3(cache, kq, vq, ks, vs, 1, 1, 1, 64, 3 * d, 64 * 3 * d, ln)      # no CPU fallback
    with pytest.raises(TypeError):
        ops.kv_pack_e4m3(cache.half(), kq, vq, ks, vs, 1, 1, 1, 64, 3 * d, 64 * 3 * d, ln)
    q, out = torch.zeros(64, 3 * d), torch.zeros(64, d)
    with pytest.raises(_lib.VfError):
        ops.attn_prefix_q8(q[:, d:2 * d], q[:, 2 * d:], q[:, :d], kq, vq, ks, vs, out, 1, 1, 1, 1, 64, 3 * d, 3 * d, 3 * d, d, ln)


# ---------------------------------------------------------------------------------------------- refusals that need no device
def _host_model(precision='f32'):
    """a model object on the host that owns caches: enough for the checks that run before any launch"""
    from viewformer_amd.config import MIGTConfig
    from viewformer_amd.migt import MIGT
    m = MIGT(MIGTConfig(n_embeddings=64, n_head=2, d_model=128, n_layer=2, token_image_size=8, sequence_size=4), precision=precision)
    m.device, m._sd_host = torch.device('cpu'), {}
    m._act_dtypes = lambda: (False, False)
    return m


def _host_cache(m, B=2, C=2, lengths=None, capacity=None):
    from viewformer_amd.migt import ContextCache
    cap = C if capacity is None else capacity
    g = torch.Generator().manual_seed(3)
    kv = [torch.randn(B * cap * 64, 3 * 128, generator=g) for _ in range(2)]
    return ContextCache(m, kv, B, C, (8, 8), capacity=capacity, lengths=lengths)


def test_the_kv_only_pack_is_tight_keeps_the_thirds_and_unpacks_bit_for_bit():
    m = _host_model()
    src = _host_cache(m, B=2, C=2, lengths=[1, 2], capacity=3)
    before = [t.clone() for t in src.kv]
    p = src.pack()
    assert p.packed == 'kv' and src.packed is None and p.B == 2 and p.C == 2 and p.capacity == 2 and p.lengths.tolist() == [1, 2]
    assert all(torch.equal(a, b) for a, b in zip(before, src.kv))              # the source is left untouched
    for (k, v), kv in zip(p.kv, src.kv):
        assert k.shape == v.shape == (2 * 2 * 64, 128) and k.is_contiguous() and v.is_contiguous()
        full = kv.view(2, 3 * 64, 384)[:, :2 * 64]
        assert torch.equal(k.view(2, 128, 128), full[:, :, 256:]) and torch.equal(v.view(2, 128, 128), full[:, :, :128])
    assert 3 * p.nbytes() == 2 * _host_cache(m, B=2, C=2).nbytes()             # exactly 2/3 of the tight plain cache
    u = p.unpack()
    assert u.packed is None and u.capacity == 2 and u.lengths.tolist() == [1, 2]
    for t, kv in zip(u.kv, src.kv):
        full = kv.view(2, 3 * 64, 384)[:, :2 * 64].reshape(-1, 384)
        assert torch.equal(t[:, :128], full[:, :128]) and torch.equal(t[:, 256:], full[:, 256:]) and bool((t[:, 128:256] == 0).all())
    assert _host_cache(m).pack().lengths is None                               # a tight source without lengths keeps the fixed route
    assert _host_cache(m, C=2, capacity=4).pack().lengths.tolist() == [2, 2]   # a source with slack took the length route: so does its pack


def test_pack_refuses_forks_packed_caches_and_e4m3_on_the_f32_arm():
    m = _host_model()
    c = _host_cache(m)
    with pytest.raises(ValueError, match=r'materialize\(\)'):
        c.fork(2, room=1).pack()
    with pytest.raises(ValueError, match=r'unpack\(\)'):
        c.pack().pack()
    with pytest.raises(ValueError, match=r'unpack\(\)'):
        c.pack().pack('e4m3')
    with pytest.raises(ValueError, match=r"precision='bf16'"):
        c.pack('e4m3')                                                         # the f32 arm exists for exactness
    for bad in ('fp8', 'bf16', 8, True):
        with pytest.raises(ValueError):
            c.pack(bad)
    with pytest.raises(ValueError):
        c.unpack()                                                             # not packed
    with pytest.raises(ValueError, match='another model'):
        c.check(_host_model())


def test_whatever_grows_forks_or_differentiates_refuses_a_packed_cache_and_names_unpack():
    m = _host_model()
    parent = _host_cache(m)
    child = parent.fork(2, room=1)
    p = parent.pack()
    cams, codes = torch.zeros(2, 1, 7), torch.zeros(2, 1, 8, 8, dtype=torch.int64)
    calls = [lambda: m.append_to_context(p, codes, cams),
             lambda: m.rollout_from_context(p, cams),
             lambda: p.fork(2),
             lambda: p.materialize(),
             lambda: m.adopt_from_fork(p, child, [0, 0]),
             lambda: m.score_grad_from_context(p, cams, codes),
             lambda: m.refine_from_context(p, cams, codes)]
    for f in calls:
        with pytest.raises(ValueError, match=r'unpack\(\)'):
            f()
    assert p.packed == 'kv' and p.C == 2                                       # nothing happened to it


def test_the_renderer_packs_in_place_refuses_what_grows_and_unpacks():
    from viewformer_amd.render import ViewRenderer
    m = _host_model()
    r = ViewRenderer(m, None)
    with pytest.raises(RuntimeError):
        r.pack()
    with pytest.raises(RuntimeError):
        r.context_bytes()
    r.cache = _host_cache(m)
    plain = r.context_bytes()
    assert plain == 2 * 2 * 2 * 64 * 384 * 4
    assert r.pack() is r and r.cache.packed == 'kv' and 3 * r.context_bytes() == 2 * plain
    cams, codes = torch.zeros(2, 1, 7), torch.zeros(2, 1, 8, 8, dtype=torch.int64)
    for f in (lambda: r.append(codes=codes, cameras=cams), lambda: r.rollout(cams), lambda: r.fork(2),
              lambda: r.score_gradient(cams, codes=codes), lambda: r.refine(cams, codes=codes)):
        with pytest.raises(ValueError, match=r'unpack\(\)'):
            f()
    with pytest.raises(ValueError, match=r'unpack\(\)'):
        r.pack()
    assert r.unpack() is r and r.cache.packed is None and r.context_bytes() == plain
    assert r.cache.fork(2).forked()                                            # works again
