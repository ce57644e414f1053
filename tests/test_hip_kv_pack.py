"""GPU: ``vf_kv_pack_e4m3`` (csrc/kv_pack.hip) against its torch restatement (tests/kv_pack_ref.py): the scales bit for
bit, the dequantised values ``torch.equal`` (values, not bytes: +-0 cannot matter) with the NaN positions equal, views at or beyond a
scene's length untouched.  Source, destinations, scales and lengths lie in ``tests/framed.py`` frames (padded strides, a gap between the
scenes) whose guards and gaps are sentinels: a stray write shows in ``violations()``."""
import numpy as np
import pytest
import torch

import kv_pack_ref as R
from context_lengths_ref import L, rand
from framed import Frame, UNWRITTEN, MODIFIED

pytestmark = pytest.mark.gpu

# (B, C, H, lengths, dtype, ld - 3d, gap between scenes in elements)
CASES = [(1, 1, 1, [1], torch.bfloat16, 0, 0),
         (2, 3, 2, [3, 1], torch.float32, 12, 40),
         (1, 2, 12, [2], torch.bfloat16, 0, 0)]
KINDS = ['zero', 'abs448', 'mant175', 'mant175_above', 'ties', 'subnormal', 'inf', 'nan']
FILL_BYTE, FILL_SCALE = 0x5A, -7.0


def case_id(case):
    B, C, H, lens, dt, pad, gap = case
    return f'B{B}-C{C}-H{H}-{"bf16" if dt == torch.bfloat16 else "f32"}'


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'needs the MI355X'
    return torch.device('cuda:0')


def plant(tile, kind, k):
    """tile: fp32 [64, 64] view, written in place; every planted number is a bf16 number, so both source dtypes hold it exactly"""
    s = 2.0 ** k
    if kind == 'zero':
        tile.zero_()
    elif kind == 'abs448':
        tile.clamp_(-1, 1).mul_(300 * s)
        tile[5, 7] = -448.0 * s                                       # absmax exactly 448 * 2^k
    elif kind == 'mant175':
        tile.clamp_(-1, 1).mul_(s)
        tile[63, 0] = 1.75 * s                                        # the mantissa on the boundary: the smaller exponent
    elif kind == 'mant175_above':
        tile.clamp_(-1, 1).mul_(s)
        tile[0, 63] = (1.75 + 2.0 ** -7) * s                          # one bf16 step above it: the larger exponent
    elif kind == 'ties':
        tile.clamp_(-1, 1)
        tile[0, 0] = 448.0                                            # scale 1
        tile[1, :8] = torch.tensor([17.0, 19.0, 21.0, 23.0, -17.0, 2.0 ** -10, 3 * 2.0 ** -10, 5 * 2.0 ** -10])
    elif kind == 'subnormal':
        tile.clamp_(-1, 1).mul_(2.0 ** -8 * s)                        # everything but absmax below the smallest e4m3 normal of the scale
        tile[9, 9] = 448.0 * s
    elif kind == 'inf':
        tile.mul_(300)
        tile[3, 3], tile[4, 4] = float('inf'), float('-inf')
    elif kind == 'nan':
        tile[10, 20] = float('nan')


def build(case, seed):
    """logical source values [B, C*L, 3d] in the case's dtype: random, with one planted tile kind per valid tile in turn"""
    B, C, H, lens, dt, pad, gap = case
    d = 64 * H
    x = rand((B, C * L, 3 * d), seed, 0.35) * torch.exp2(torch.from_numpy(
        np.random.Generator(np.random.PCG64(seed + 1)).integers(-20, 20, size=(B, C, 1, 3 * H, 1)).astype(np.float32)
    )).expand(B, C, L, 3 * H, 64).reshape(B, C * L, 3 * d)
    i = seed
    planted = []
    for b in range(B):
        for c in range(lens[b]):
            for h in range(H):
                for third in (2, 0):
                    kind = KINDS[i % len(KINDS)]
                    plant(x[b, c * L:(c + 1) * L, third * d + h * 64:third * d + (h + 1) * 64], kind, (-90, -3, 0, 40, 99)[i % 5])
                    planted.append(kind)
                    i += 3                                             # 3 and 8 are coprime: every kind comes up
        x[b, lens[b] * L:] = float('nan')                             # views beyond the length: never read into a result
    return x.to(dt), planted


@pytest.mark.parametrize('case', CASES, ids=case_id)
def test_scales_and_dequantised_values_equal_the_restatement(dev, case):
    from viewformer_amd import ops
    B, C, H, lens, dt, pad, gap = case
    d = 64 * H
    x, planted = build(case, 40 + B + H)
    assert B * H * C < 8 or set(planted) == set(KINDS)
    ld = 3 * d + pad
    fsrc = Frame(C * L, 3 * d, ld, dt, dev, batch=B, batch_stride=C * L * ld + gap).load(x if B > 1 else x[0])
    qv, sv = H * 4096 + 64, H + 3                                      # padded view strides
    fk = Frame(C, H * 4096, qv, torch.uint8, dev, batch=B, batch_stride=C * qv + 256)
    fv = Frame(C, H * 4096, qv, torch.uint8, dev, batch=B, batch_stride=C * qv + 256)
    fks = Frame(C, H, sv, torch.float32, dev, batch=B, batch_stride=C * sv + 5)
    fvs = Frame(C, H, sv, torch.float32, dev, batch=B, batch_stride=C * sv + 5)
    for f in (fk, fv):
        f.view.fill_(FILL_BYTE)
    for f in (fks, fvs):
        f.view.fill_(FILL_SCALE)
    fl = Frame.raw(B * 4, dev, dtype=torch.int32).load(torch.tensor(lens, dtype=torch.int32))
    src0 = fsrc.view[0] if B > 1 else fsrc.view
    ops.kv_pack_e4m3(src0, fk.view, fv.view, fks.view, fvs.view, B, C, H, L, ld, fsrc.batch_stride, fl.view,
                     q_view_stride=qv, q_scene_stride=fk.batch_stride, s_view_stride=sv, s_scene_stride=fks.batch_stride)
    torch.cuda.synchronize()
    assert fsrc.violations() == [] and fl.violations() == []         # inputs keep their bits
    for f in (fk, fv, fks, fvs):                                      # outputs: guards and gaps intact (the window is compared below)
        assert [v for v in f.violations() if v[0] not in (UNWRITTEN, MODIFIED)] == []
    kq = fk.logical().contiguous().cpu().view(B, C, H, 64, 64)
    vq = fv.logical().contiguous().cpu().view(B, C, H, 64, 64)
    ks, vs = fks.logical().contiguous().cpu().view(B, C, H), fvs.logical().contiguous().cpu().view(B, C, H)
    xf = x.float().view(B, C, L, 3, H, 64)
    ktile = xf[:, :, :, 2].permute(0, 1, 3, 2, 4)                     # [B, C, H, token, feature]
    vtile = xf[:, :, :, 0].permute(0, 1, 3, 4, 2)                     # [B, C, H, feature, token]: V is stored transposed
    for name, q, s, tiles in (('K', kq, ks, ktile), ('V', vq, vs, vtile)):
        for b in range(B):
            n = lens[b]
            if n < C:                                                 # views at or beyond the length: untouched
                assert bool((q[b, n:] == FILL_BYTE).all()) and bool((s[b, n:] == FILL_SCALE).all()), (name, b)
            rq, rs = R.pack_tiles(tiles[b, :n].contiguous())
            assert torch.equal(s[b, :n].contiguous().view(torch.int32), rs.contiguous().view(torch.int32)), (name, b, s[b, :n], rs)
            got, want = R.unpack_tiles(q[b, :n].contiguous(), s[b, :n]), R.unpack_tiles(rq, rs)
            assert torch.equal(torch.isnan(got), torch.isnan(want)), (name, b)
            assert torch.equal(torch.nan_to_num(got, nan=0.0), torch.nan_to_num(want, nan=0.0)), (name, b, (got - want).abs().nan_to_num().max())
            assert torch.equal(got.bfloat16().float().nan_to_num(), got.nan_to_num())      # bf16 numbers


def test_an_empty_launch_is_a_no_op(dev):
    from viewformer_amd import ops
    z8, zf = torch.full((4096,), FILL_BYTE, dtype=torch.uint8, device=dev), torch.full((4,), FILL_SCALE, device=dev)
    src = torch.zeros((64, 192), dtype=torch.bfloat16, device=dev)
    ln = torch.zeros(1, dtype=torch.int32, device=dev)
    ops.kv_pack_e4m3(src, z8, z8.clone(), zf, zf.clone(), 1, 0, 1, L, 192, 64 * 192, ln)       # (B = 0: tests/test_pack_host.py)
    ops.kv_pack_e4m3(src, z8, z8.clone(), zf, zf.clone(), 1, 1, 1, L, 192, 64 * 192, ln)       # length 0: every view is skipped
    torch.cuda.synchronize()
    assert bool((z8 == FILL_BYTE).all()) and bool((zf == FILL_SCALE).all())
