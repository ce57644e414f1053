"""The torch restatement of csrc/kv_pack.hip: e4m3 tiles with one power-of-two scale each.

A tile is the last two dimensions of a tensor (64 tokens x 64 features in the kernel; any size here).  Its scale is 2^e with e the
smallest integer such that absmax <= 448 * 2^e, read off the exponent and mantissa FIELDS of absmax as the kernel does; elements are
x * 2^-e, clamped to +-448 by comparisons (a NaN stays), converted round-to-nearest-even.  ``brute_exponent`` is the definition itself,
searched in exact arithmetic, for the tests of the bit rule."""
import torch

E4M3_MAX = 448.0
E_MIN, E_MAX = -100, 100


def pack_exponent(absmax):
    """fp32 tensor of non-negative magnitudes (NaN not expected) -> int32 e per element, by the kernel's bit rule"""
    bits = absmax.float().contiguous().view(torch.int32) & 0x7FFFFFFF
    ea = (bits >> 23) - 127
    e = torch.where((bits & 0x7FFFFF) <= 0x600000, ea - 8, ea - 7).clamp(E_MIN, E_MAX)
    return torch.where((bits == 0) | (bits >= 0x7F800000), torch.zeros_like(e), e).to(torch.int32)


def brute_exponent(a: float) -> int:
    """the smallest integer e with a <= 448 * 2^e (exact: both sides are doubles with few mantissa bits), clamped as the kernel clamps;
    0 for a == 0 and for a non-finite a"""
    a = float(a)
    if a == 0.0 or a != a or a in (float('inf'), float('-inf')):
        return 0
    e = -200
    while a > E4M3_MAX * 2.0 ** e:
        e += 1
    return min(max(e, E_MIN), E_MAX)


def tile_scales(x):
    """x [..., r, c] -> (e int32 [...], scale fp32 [...] = 2^e); NaN elements do not enter absmax"""
    a = x.float().abs()
    a = torch.where(torch.isnan(a), torch.zeros_like(a), a)
    e = pack_exponent(a.amax(dim=(-2, -1)))
    return e, torch.ldexp(torch.ones_like(e, dtype=torch.float32), e)


def pack_tiles(x):
    """x [..., r, c] (any float dtype) -> (float8_e4m3fn [..., r, c], scale fp32 [...])"""
    e, scale = tile_scales(x)
    inv = torch.ldexp(torch.ones_like(scale), -e)
    y = x.float() * inv[..., None, None]
    hi, lo = torch.full_like(y, E4M3_MAX), torch.full_like(y, -E4M3_MAX)
    y = torch.where(y > E4M3_MAX, hi, torch.where(y < -E4M3_MAX, lo, y))          # comparisons: a NaN fails both and stays
    return y.to(torch.float8_e4m3fn), scale


def unpack_tiles(q, scale):
    """(e4m3 bytes as float8_e4m3fn or uint8 [..., r, c], scale [...]) -> fp32 values"""
    if q.dtype == torch.uint8:
        q = q.view(torch.float8_e4m3fn)
    return q.float() * scale[..., None, None]


def cache_tiles(third, B, C, H):
    """a K or V third [B*C*64, 64 H] (logical values) -> tiles [B*C, H, 64 tokens, 64 features]"""
    return third.reshape(B * C, 64, H, 64).permute(0, 2, 1, 3)
