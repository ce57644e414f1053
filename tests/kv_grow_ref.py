"""The torch restatement of what one launch of ``vf_kv_append_e4m3`` (csrc/kv_append_e4m3.hip) and of ``vf_kv_append_split``
(csrc/kv_append.hip) leaves in its destinations, built on tests/kv_pack_ref.py: new view j of scene b goes to slot
``pos[b] + j``; a slot outside [0, capacity) is skipped; nothing else changes.  Tensors are LOGICAL (no padding): the tests frame them."""
import torch

import kv_pack_ref as R

L = 64


def new_view_tiles(qkv, B, K, H):
    """fused c_attn rows [B*K*64, 3*64 H] (thirds V, Q, K; any float dtype) -> (K tiles [B, K, H, key, feature], V tiles
    [B, K, H, feature, key]) in fp32: the two tile layouts of the packed buffers"""
    x = qkv.float().view(B, K, L, 3, H, 64)
    return x[:, :, :, 2].permute(0, 1, 3, 2, 4).contiguous(), x[:, :, :, 0].permute(0, 1, 3, 4, 2).contiguous()


def canonical_nan(q):
    """uint8 e4m3 bytes with both NaN encodings of e4m3fn (0x7F, 0xFF) written as 0x7F: "a NaN stays NaN" is the kernels' contract, and
    which of the two bytes the hardware conversion leaves for a NaN is not part of it (torch's cast keeps the sign of the fp32 NaN)"""
    return torch.where(q == 0xFF, torch.full_like(q, 0x7F), q)


def append_e4m3(qkv, kq, vq, kscale, vscale, B, K, H, capacity, pos):
    """``kq`` / ``vq`` uint8 [B, capacity, H, 64, 64] and ``kscale`` / ``vscale`` fp32 [B, capacity, H] before the launch -> the four
    after it (copies)"""
    out = [t.clone() for t in (kq, vq, kscale, vscale)]
    kt, vt = new_view_tiles(qkv, B, K, H)
    for b in range(B):
        for j in range(K):
            slot = int(pos[b]) + j
            if not 0 <= slot < capacity:
                continue
            for tiles, q, s in ((kt, out[0], out[2]), (vt, out[1], out[3])):
                rq, rs = R.pack_tiles(tiles[b, j])
                q[b, slot] = rq.view(torch.uint8)
                s[b, slot] = rs
    return out


def append_split(qkv, k, v, B, K, d, capacity, pos):
    """``k`` / ``v`` [B, capacity*64, d] before the launch -> the two after it (copies): the K third / the V third of the new views' rows"""
    k, v = k.clone(), v.clone()
    x = qkv.view(B, K, L, 3 * d)
    for b in range(B):
        for j in range(K):
            slot = int(pos[b]) + j
            if 0 <= slot < capacity:
                k[b, slot * L:(slot + 1) * L] = x[b, j, :, 2 * d:]
                v[b, slot * L:(slot + 1) * L] = x[b, j, :, :d]
    return k, v
