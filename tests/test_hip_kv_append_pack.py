"""GPU: ``vf_kv_append_e4m3`` (csrc/kv_append_e4m3.hip) and ``vf_kv_append_split`` (csrc/kv_append.hip), DESIGN.md §6.22 — the keys and
values of new views go to each scene's own slot of a PACKED cache with room and nothing else changes.  The e4m3 entry: bytes and scales
of the written slots equal the torch restatement (tests/kv_grow_ref.py) bit for bit (a NaN's byte up to e4m3fn's two encodings of
NaN, which the restatement cannot tell apart: ``kv_grow_ref.canonical_nan``), and equal — raw bytes, NaN included — what ``ops.kv_pack_e4m3`` writes for the
same views held in a plain buffer, bit for bit (one tile routine for both kernels).  The split entry: K and V are ``torch.equal`` to the
source's thirds.  Source, destinations and ``pos`` lie in ``tests/framed.py`` frames (padded strides, a gap between the scenes) loaded
with values of their own: every other slot, gap and guard keeps its bits, and the Q third, filled with NaN, reaches nothing."""
import numpy as np
import pytest
import torch

import kv_grow_ref as G
from context_lengths_ref import L, rand
from framed import BACK, BATCH_GAP, FRONT, ROW_GAP, Frame
from test_hip_kv_pack import KINDS, plant

pytestmark = pytest.mark.gpu

# (B, K, H, capacity, pos, dtype, ld_src - 3d, views that land): one tile pair; a ragged batch whose scene 1 overflows (its second view is skipped), padded
# source rows; the model's width, three views into the middle of a cache; a negative position (view 0 skipped, view 1 lands in slot 0)
E4M3_CASES = [(1, 1, 1, 1, [0], torch.bfloat16, 0, 1),
              (2, 2, 2, 4, [1, 3], torch.float32, 12, 3),
              (1, 3, 12, 5, [2], torch.bfloat16, 0, 3),
              (1, 2, 1, 2, [-1], torch.bfloat16, 0, 1)]
FILL_BYTE, FILL_SCALE = 0x5A, -7.0


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'needs the MI355X'
    return torch.device('cuda:0')


def _e4m3_id(case):
    B, K, H, cap, pos, dt, pad, landed = case
    return f'B{B}-K{K}-H{H}-cap{cap}-{"bf16" if dt == torch.bfloat16 else "f32"}'


def build(case, seed):
    """the new views' fused c_attn rows [B*K*L, 3d] in the case's dtype: random over 40 binades, one planted tile kind per K and V tile
    in turn (k reaching the clamp at +-99 / -90), the Q third NaN"""
    B, K, H, cap, pos, dt, pad, landed = case
    d = 64 * H
    x = rand((B * K, L, 3 * d), seed, 0.35) * torch.exp2(torch.from_numpy(
        np.random.Generator(np.random.PCG64(seed + 1)).integers(-20, 20, size=(B * K, 1, 3 * H, 1)).astype(np.float32)
    )).expand(B * K, L, 3 * H, 64).reshape(B * K, L, 3 * d)
    i = seed
    planted = []
    for v in range(B * K):
        for h in range(H):
            for third in (2, 0):
                kind = KINDS[i % len(KINDS)]
                plant(x[v, :, third * d + h * 64:third * d + (h + 1) * 64], kind, (-90, -3, 0, 40, 99)[i % 5])
                planted.append(kind)
                i += 3                                                 # 3 and 8 are coprime: every kind comes up
    x[:, :, d:2 * d] = float('nan')                                    # the Q third: never read
    return x.reshape(B * K * L, 3 * d).to(dt), planted


@pytest.mark.parametrize('case', E4M3_CASES, ids=_e4m3_id)
def test_e4m3_append_writes_the_restatements_bytes_and_scales_and_nothing_else(dev, case):
    from viewformer_amd import ops
    B, K, H, cap, pos, dt, pad, landed = case
    d = 64 * H
    x, planted = build(case, 70 + B + H + K)
    assert B * K * H < 4 or set(planted) == set(KINDS)
    ld = 3 * d + pad
    fsrc = Frame(B * K * L, 3 * d, ld, dt, dev).load(x)
    qv, sv = H * 4096 + 64, H + 3                                      # padded view strides
    fq = [Frame(cap, H * 4096, qv, torch.uint8, dev, batch=B, batch_stride=cap * qv + 256) for _ in range(2)]
    fs = [Frame(cap, H, sv, torch.float32, dev, batch=B, batch_stride=cap * sv + 5) for _ in range(2)]
    old_q = torch.full((B, cap, H * 4096), FILL_BYTE, dtype=torch.uint8)
    old_s = torch.full((B, cap, H), FILL_SCALE)
    for f in fq:
        f.load(old_q if B > 1 else old_q[0], accumulate=True)
    for f in fs:
        f.load(old_s if B > 1 else old_s[0], accumulate=True)
    fp = Frame.raw(B * 4, dev, dtype=torch.int32).load(torch.tensor(pos, dtype=torch.int32))
    ops.kv_append_e4m3(fsrc.view, fq[0].view, fq[1].view, fs[0].view, fs[1].view, B, K, H, L, ld, cap, fp.view,
                       q_view_stride=qv, q_scene_stride=fq[0].batch_stride, s_view_stride=sv, s_scene_stride=fs[0].batch_stride)
    torch.cuda.synchronize()
    assert fsrc.violations() == [] and fp.violations() == []         # inputs keep their bits
    for f in fq + fs:
        for region in (FRONT, BACK, ROW_GAP, BATCH_GAP):
            assert f.offsets(region).numel() == 0, region             # no guard or gap byte has changed
    got = [f.logical().cpu().view(B, cap, H, 64, 64) for f in fq] + [f.logical().cpu().view(B, cap, H) for f in fs]
    want = G.append_e4m3(x, old_q.view(B, cap, H, 64, 64), old_q.view(B, cap, H, 64, 64),
                         old_s, old_s, B, K, H, cap, pos)
    slots = [(b, pos[b] + j) for b in range(B) for j in range(K) if 0 <= pos[b] + j < cap]
    assert len(slots) == landed                                        # the overflowing and the negative slot are skipped
    for name, g, w in zip(('kq', 'vq', 'kscale', 'vscale'), got, want):
        bits = G.canonical_nan if g.dtype == torch.uint8 else (lambda t: t.contiguous().view(torch.int32))
        assert torch.equal(bits(g), bits(w)), name                    # written slots: the restatement; every other slot: what it held
        for b in range(B):
            for c in range(cap):
                if (b, c) not in slots:
                    assert bool((g[b, c] == (FILL_BYTE if g.dtype == torch.uint8 else FILL_SCALE)).all()), (name, b, c)
    # ... and what vf_kv_pack_e4m3 writes for the same views held in a plain buffer: one tile routine, equal bytes and scales
    pk = [torch.zeros((B * K, H, 64, 64), dtype=torch.uint8, device=dev) for _ in range(2)] + [torch.zeros((B * K, H), device=dev) for _ in range(2)]
    plain = x.to(dev).contiguous()
    ops.kv_pack_e4m3(plain, *pk, B, K, H, L, 3 * d, K * L * 3 * d, torch.full((B,), K, dtype=torch.int32, device=dev))
    torch.cuda.synchronize()
    for name, g, p in zip(('kq', 'vq', 'kscale', 'vscale'), got, pk):
        p = p.cpu().view(B, K, *p.shape[1:])
        for b in range(B):
            for j in range(K):
                if (b, pos[b] + j) in slots:
                    a, w = g[b, pos[b] + j], p[b, j]
                    assert torch.equal(a if a.dtype == torch.uint8 else a.view(torch.int32), w if w.dtype == torch.uint8 else w.view(torch.int32)), (name, b, j)


def test_an_empty_e4m3_append_is_a_no_op(dev):
    from viewformer_amd import ops
    z8, zf = torch.full((4096,), FILL_BYTE, dtype=torch.uint8, device=dev), torch.full((4,), FILL_SCALE, device=dev)
    src = torch.zeros((64, 192), dtype=torch.bfloat16, device=dev)
    ops.kv_append_e4m3(src, z8, z8.clone(), zf, zf.clone(), 1, 1, 1, L, 192, 0, torch.zeros(1, dtype=torch.int32, device=dev))     # no room
    ops.kv_append_e4m3(src, z8, z8.clone(), zf, zf.clone(), 1, 1, 1, L, 192, 1, torch.ones(1, dtype=torch.int32, device=dev))      # slot 1 of 1: skipped
    torch.cuda.synchronize()
    assert bool((z8 == FILL_BYTE).all()) and bool((zf == FILL_SCALE).all())


# ---------------------------------------------------------------------------------------------- vf_kv_append_split
# tests/test_hip_kv_append.py's shapes (B, K, d, capacity, pos)
SPLIT_CASES = [(1, 1, 64, 2, [1]), (3, 2, 192, 7, [0, 5, 2]), (2, 3, 768, 4, [1, 1])]


def _rand(shape, seed):
    g = np.random.Generator(np.random.PCG64(seed))
    return torch.from_numpy(g.standard_normal(shape).astype(np.float32))


def _run_split(dev, dt, B, K, d, capacity, pos, seed=0):
    """launch on framed tensors with ld_src > 3 d, ld_k != ld_v > d and a gap between the scenes -> (got K, V; want K, V; old K, V) as bits"""
    from viewformer_amd import ops
    ld_src, ld_k, ld_v = 3 * d + 16, d + 8, d + 24
    src = _rand((B * K * L, 3 * d), 500 + seed).to(dt)
    src[:, d:2 * d] = float('nan')                                              # the Q third reaches nothing
    olds = [_rand((B, capacity * L, d), 600 + seed + i).to(dt) for i in range(2)]
    fs = Frame(B * K * L, 3 * d, ld_src, dt, dev).load(src)
    fk = Frame(capacity * L, d, ld_k, dt, dev, batch=B, batch_stride=capacity * L * ld_k + 64).load(olds[0] if B > 1 else olds[0][0], accumulate=True)
    fv = Frame(capacity * L, d, ld_v, dt, dev, batch=B, batch_stride=capacity * L * ld_v + 32).load(olds[1] if B > 1 else olds[1][0], accumulate=True)
    fp = Frame.raw(B * 4, dev, dtype=torch.int32).load(torch.tensor(pos, dtype=torch.int32))
    ops.kv_append_split(fs.view, fk.view, fv.view, B, K, L, d, ld_src, ld_k, ld_v, fk.batch_stride, fv.batch_stride, capacity, fp.view)
    torch.cuda.synchronize()
    assert fs.violations() == [] and fp.violations() == []                       # inputs unchanged, nothing written around them
    for f in (fk, fv):
        for region in (FRONT, BACK, ROW_GAP, BATCH_GAP):
            assert f.offsets(region).numel() == 0, region                        # no guard or gap byte has changed
    idt = torch.int16 if dt == torch.bfloat16 else torch.int32
    want = G.append_split(src, olds[0], olds[1], B, K, d, capacity, pos)
    got = [f.logical().view(B, capacity * L, d).cpu() for f in (fk, fv)]
    return [t.view(idt) for t in got], [t.view(idt) for t in want], [t.view(idt) for t in olds]


@pytest.mark.parametrize('dt', [torch.bfloat16, torch.float32], ids=['bf16', 'f32'])
@pytest.mark.parametrize('case', SPLIT_CASES, ids=lambda c: 'B{}K{}d{}cap{}'.format(*c[:4]))
def test_split_append_copies_the_k_and_v_thirds_and_nothing_else_changes(dev, dt, case):
    got, want, old = _run_split(dev, dt, *case)
    for g, w, o in zip(got, want, old):
        assert not torch.equal(w, o)
        assert torch.equal(g, w)


@pytest.mark.parametrize('dt', [torch.bfloat16, torch.float32], ids=['bf16', 'f32'])
def test_split_append_skips_a_view_beyond_the_capacity(dev, dt):
    """scene 1: pos + K > capacity (views 2, 3 and 4 of a 4-view cache): views 2 and 3 are written, view 4 is dropped"""
    got, want, old = _run_split(dev, dt, 2, 3, 192, 4, [1, 2], seed=1)
    for g, w, o in zip(got, want, old):
        assert torch.equal(g, w)
        assert not torch.equal(g[1, 3 * L:], o[1, 3 * L:]) and torch.equal(g[0, :L], o[0, :L])


def test_a_split_launch_larger_than_the_grid_walks_all_of_it(dev):
    """fp32, 88 views of d = 768: 24 576 16-byte chunks per view; the grid is capped at 8192 // 88 = 93 slices of 256 threads per view, so
    threads take a second chunk (the stride loop)"""
    got, want, old = _run_split(dev, torch.float32, 4, 22, 768, 24, [0, 2, 1, 2], seed=2)
    for g, w in zip(got, want):
        assert torch.equal(g, w)
